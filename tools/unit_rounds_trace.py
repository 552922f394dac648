#!/usr/bin/env python3
"""The launches of the unit discoveries and the unit-round loops, for a comparison of two builds of the library.

    rocprofv3 --kernel-trace -d DIR -o p --output-format csv -- python tools/unit_rounds_trace.py run
    python tools/unit_rounds_trace.py compare A_kernel_trace.csv B_kernel_trace.csv [--out DIR] [--map FILE]

`run` builds one fixed small input per entry point that goes over units in rounds -- seven chunks of seeded text,
compressed by zlib on the CPU with a full flush behind each, so that every chunk is one dynamic block and one unit --
sets "one_round_units" to 3 (three rounds, the last of one unit; the two range reads select all seven units, and G's
units are the archive's one entry) and makes one call each:
  A flate_hip_inflate_one, B _inflate_one_seek_index, C _inflate_one_ranges on the stream as one gzip member;
  D flate_hip_gzfile_read with "gzfile_serial_max" off and on, E _gzfile_seek_index, F _gzfile_ranges on the chunks as
    three members of 3 + 1 + 3 units (with the option on the middle member is decoded whole: two runs of units);
  G flate_hip_zip_read with "zip_unit_min" = 1 on the stream as the one entry of an archive;
  H flate_hip_inflate_one_index on A's stream, I flate_hip_gzfile_index on D's file with "gzfile_serial_max" off and on
    (the discoveries alone; flate_hip_gzfile_seek_index does not read that option, so E is not repeated with it);
  J flate_hip_one_reader_* over A's stream in three parts cut inside units, K flate_hip_gzfile_reader_* over D's file in
    three parts -- one cut inside a member, one inside a gzip header -- with room for one unit a call, so that calls
    deliver fewer units than they found;
  L A and D's first read once more with DEVICE pointers (A to G pass host pointers: the output is staged and comes down);
  M flate_hip_gzfile_reader_* with set_serial_max over forty short members in three parts (cuts inside members: a call
    stops in front of an OPEN member, the next one starts at its header).
Every result is compared with the input.  FLATE_HIP_LIB chooses the library, as for every tool here.

`compare` reads the kernel traces of two such runs and holds the ordered lists of (kernel name, grid size, workgroup
size) against each other; with --out it writes both lists and a one-line verdict there.  --map FILE: lines "old new" of
kernels that the second build has under another name (several old names may share a new one); a kernel on either side
of the map is compared by its name without its parameter list, which changes with the merge.  No counters, no times."""
import argparse
import csv
import os
import re
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 12000  # bytes of text per unit: one dynamic block at level 6 (fewer symbols than zlib's buffer holds)
UNITS = 7
GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


def text(n, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    words = [bytes(rng.randint(97, 123, rng.randint(2, 9)).astype(np.uint8)) for _ in range(500)]
    out = b" ".join(words[i] for i in rng.randint(0, len(words), n // 3))
    return out[:n]


def raw_stream(chunks):
    """The chunks as one raw DEFLATE stream, a full flush (an empty stored block) behind each but the last."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts = [c.compress(p) + c.flush(zlib.Z_FULL_FLUSH) for p in chunks[:-1]]
    return b"".join(parts) + c.compress(chunks[-1]) + c.flush()


def member(chunks):
    plain = b"".join(chunks)
    return GZ_HEADER + raw_stream(chunks) + struct.pack("<II", zlib.crc32(plain), len(plain))


def archive(raw, plain):
    name = b"e0"
    crc = zlib.crc32(plain)
    local = struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, len(raw), len(plain), len(name), 0) + name
    central = struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, 0x0800, 8, 0, 0x0021, crc, len(raw), len(plain),
                          len(name), 0, 0, 0, 0, 0, 0) + name
    return local + raw + central + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 1, 1, len(central), len(local) + len(raw), 0)


def forty_members():
    """Forty gzip members of 200 .. 900 bytes of text, zlib level 6 -> (file, plain)."""
    import random
    rng = random.Random(40)
    plain = [text(rng.randrange(200, 901), 400 + k) for k in range(40)]
    return b"".join(member([p]) for p in plain), b"".join(plain)


def run():
    import importlib
    import numpy as np
    flate = importlib.import_module("moonbit-flate_amd")
    chunks = [text(CHUNK, 100 + k) for k in range(UNITS)]
    plain = b"".join(chunks)
    one = member(chunks)
    members = member(chunks[:3]) + member(chunks[3:4]) + member(chunks[4:])
    serial_max = len(member(chunks[3:4])) + 64  # the middle member is short, the two around it are not
    assert serial_max < len(member(chunks[4:]))
    # the ranges touch all seven units, so that the two range reads go over three rounds too
    ranges = [(5, 700), (CHUNK - 10, 3 * CHUNK + 10), (4 * CHUNK + 5, 4 * CHUNK + 6), (5 * CHUNK, len(plain))]
    begin, end = [b for b, _ in ranges], [e for _, e in ranges]
    want = b"".join(plain[b:e] for b, e in ranges)
    buf = lambda: np.empty(len(plain) + 64, np.uint8)  # (a buffer of the caller's: no size query in front of the call)
    eng = flate.FlateEngine(0)
    eng.set_option("one_round_units", 3)
    done = []

    def check(what, ok, units=None):
        assert ok, what
        assert units is None or units == UNITS, (what, units)
        done.append(what)

    out, r = eng.inflate_one(one, "gzip", out=buf())                                          # A
    check("A inflate_one", r.rc == 0 and bytes(out[:r.out_len]) == plain, r.n_units)
    si = eng.inflate_one_seek_index(one, "gzip", span=CHUNK)                                # B
    check("B inflate_one_seek_index", si.rc == 0 and si.n_points > 2, si.n_units)
    out, r = eng.inflate_one_ranges(one, si, begin, end, out=buf(), wrap="gzip")            # C
    check("C inflate_one_ranges", r.rc == 0 and bytes(out[:int(r.out_off[-1])]) == want, r.n_decoded)
    for serial in (0, serial_max):                                                          # D
        eng.set_option("gzfile_serial_max", serial)
        out, r = eng.gzfile_read(members, out=buf())
        check("D gzfile_read, gzfile_serial_max %d" % serial, r.rc == 0 and bytes(out[:r.out_len]) == plain, r.n_units)
        assert r.n_members == 3 and (eng.gzfile_last_route()[0] == 1) == (serial != 0)
    eng.set_option("gzfile_serial_max", 0)
    gi = eng.gzfile_seek_index(members, span=CHUNK)                                         # E
    check("E gzfile_seek_index", gi.rc == 0 and gi.n_members == 3 and gi.n_points > 3, gi.n_units)
    out, r = eng.gzfile_ranges(members, gi, begin, end, out=buf())                          # F
    check("F gzfile_ranges", r.rc == 0 and bytes(out[:int(r.out_off[-1])]) == want, r.n_decoded)
    eng.set_option("zip_unit_min", 1)                                                       # G
    out, r = eng.zip_read(archive(raw_stream(chunks), plain), out=buf())
    check("G zip_read through units", r.rc == 0 and bytes(out[:int(r.out_len[0])]) == plain and eng.zip_last_route()[0] == 1)
    eng.set_option("zip_unit_min", 0)
    ix = eng.inflate_one_index(one, "gzip")                                                 # H
    check("H inflate_one_index", ix.rc == 0 and ix.out_bytes == len(plain), ix.n_units)
    for serial in (0, serial_max):                                                          # I
        eng.set_option("gzfile_serial_max", serial)
        gx = eng.gzfile_index(members)
        check("I gzfile_index, gzfile_serial_max %d" % serial, gx.rc == 0 and gx.n_members == 3 and gx.out_bytes == len(plain),
              gx.n_units)
    eng.set_option("gzfile_serial_max", 0)

    def feed(rd, f, ends, out_cap):
        """f through a reader, a part per entry of `ends`, each beginning with what the last call left unused"""
        got, pos, units, rc = b"", 0, 0, 0
        for end in ends:
            for _ in range(UNITS + 2):  # (a call that delivers fewer units than it found is made again over the rest)
                used, out, r = rd.read(f[pos:end], final=end == len(f), out_cap=out_cap)
                got, pos, units, rc = got + bytes(out), pos + used, units + r.n_units, r.rc
                if rc != 0 or used == 0 or pos == end:
                    break
        rd.close()
        return rc == 1 and got == plain and pos == len(f), units

    third = len(one) // 3                                                                   # J
    check("J one reader in three parts", *feed(eng.open_one_reader("gzip"), one, [third, 2 * third, len(one)], None))
    m0, m1 = len(member(chunks[:3])), len(member(chunks[3:4]))                              # K
    check("K gzfile reader in three parts", *feed(eng.open_gzfile_reader(), members, [m0 // 2, m0 + m1 + 4, len(members)],
                                                  CHUNK + 100))
    import torch                                                                            # L
    dev = lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()
    room = lambda: torch.empty(len(plain) + 64, dtype=torch.uint8, device="cuda")
    out, r = eng.inflate_one(dev(one), "gzip", out=room())
    check("L inflate_one, device pointers", r.rc == 0 and bytes(out[:r.out_len].cpu().numpy()) == plain, r.n_units)
    out, r = eng.gzfile_read(dev(members), out=room())
    check("L gzfile_read, device pointers", r.rc == 0 and bytes(out[:r.out_len].cpu().numpy()) == plain, r.n_units)
    forty, forty_plain = forty_members()                                                    # M
    got, pos, rd = b"", 0, eng.open_gzfile_reader(serial_max=4096)
    for end in (len(forty) // 3, 2 * len(forty) // 3, len(forty)):
        for _ in range(4):  # (a call that stops in front of an OPEN member is made again with the rest)
            used, out, r = rd.read(forty[pos:end], final=end == len(forty))
            got, pos = got + bytes(out), pos + used
            if r.rc != 0 or used == 0 or pos == end:
                break
    rd.close()
    check("M gzfile reader with whole members in three parts", r.rc == 1 and got == forty_plain and pos == len(forty))
    eng.close()
    print("unit_rounds_trace: %d calls ok (%s)" % (len(done), "; ".join(done)))


def launches(path):
    """[(kernel name, grid, workgroup)] of a rocprofv3 kernel trace, in dispatch order."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, k: "x".join(r["%s_Size_%s" % (k, a)] for a in "XYZ")
    return [(r["Kernel_Name"], dims(r, "Grid"), dims(r, "Workgroup")) for r in rows]


def base_name(kernel):
    words = re.findall(r"[A-Za-z_]\w*", kernel.split("(")[0])
    return words[-1] if words else kernel


def compare(a, b, out, rename=None):
    la, lb = launches(a), launches(b)
    names = {}
    if rename:
        with open(rename) as f:
            names = dict(line.split() for line in f if line.strip() and not line.startswith("#"))
    merged = set(names) | set(names.values())
    norm = lambda x: (names.get(base_name(x[0]), base_name(x[0])),) + x[1:] if base_name(x[0]) in merged else x
    full_a, full_b = la, lb
    la, lb = [norm(x) for x in la], [norm(x) for x in lb]
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None)
    if first is None and len(la) != len(lb):
        first = min(len(la), len(lb))
    verdict = "identical: %d launches, the same kernel, grid and workgroup at every place" % len(la) if first is None else \
        "DIFFERENT at launch %d of %d / %d: %s | %s" % (first, len(la), len(lb), la[first:first + 1], lb[first:first + 1])
    if out:
        os.makedirs(out, exist_ok=True)
        for name, l in (("launches_parent.txt", full_a), ("launches_new.txt", full_b)):
            with open(os.path.join(out, name), "w") as f:
                f.writelines("%s\t%s\t%s\n" % x for x in l)
        with open(os.path.join(out, "verdict.txt"), "w") as f:
            f.write(verdict + "\n")
    print(verdict)
    return 0 if first is None else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run")
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("new")
    c.add_argument("--out")
    c.add_argument("--map")
    args = ap.parse_args()
    sys.exit(run() if args.cmd == "run" else compare(args.parent, args.new, args.out, args.map))
