#!/usr/bin/env python3
"""Whole-call times of the unit calls, for a comparison of two builds of the library.

    python tools/unit_rounds_ab.py gen
    [FLATE_HIP_LIB=other/libflate_hip.so] python tools/unit_rounds_ab.py time TAG

`gen` builds the inputs once, files under $FLATE_AB_TMP (default /tmp/unit_rounds_ab): 256 MiB of S-text, zlib level 6,
as one gzip member (16 pieces joined by full flushes), as a gzip file of 16 members, the same file with 8 members of
4 KiB behind every long one, and as a ZIP archive of 16 entries.  `time TAG` loads them, times every call that goes over
units in rounds -- flate_hip_inflate_one, its seek index and ranges, flate_hip_gzfile_read without and with
"gzfile_serial_max", its seek index and ranges, flate_hip_zip_read with "zip_unit_min" -- 7 times behind one uncounted
call (device pointers, whole calls, a host clock around a synchronised call) and writes median, min and max per call to
$FLATE_OUT_ROOT (default results/)/unit_rounds_ab/TAG.json.  Start a fresh process per build and alternate the builds;
profiles/r13/README.md has a table made this way."""
import importlib
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")

MIB = 256
PARTS = 16
REPS = 7
TMP = os.environ.get("FLATE_AB_TMP", "/tmp/unit_rounds_ab")
HDR = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


def gen():
    os.makedirs(TMP, exist_ok=True)
    plain = flate.synth("text", MIB * 16, 65536).reshape(-1)
    size = plain.size // PARTS

    def part(k):
        p = plain[k * size:(k + 1) * size].tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        whole = c.compress(p) + c.flush()
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        open_ = c.compress(p) + c.flush(zlib.Z_FULL_FLUSH)  # (no BFINAL: the next piece follows)
        return whole, open_, zlib.crc32(p), len(p)

    with ThreadPoolExecutor(max_workers=16) as pool:
        parts = list(pool.map(part, range(PARTS)))
    # one long stream: the open pieces, the last one closed
    raw = b"".join(o for _, o, _, _ in parts[:-1]) + parts[-1][0]
    one = HDR + raw + struct.pack("<II", zlib.crc32(plain.tobytes()), plain.size & 0xffffffff)
    gz = b"".join(HDR + w + struct.pack("<II", crc, n) for w, _, crc, n in parts)
    # short members between the long ones, for "gzfile_serial_max"
    small = plain[:4096].tobytes()
    sm = HDR + zlib.compress(small, 6)[2:-4] + struct.pack("<II", zlib.crc32(small), len(small))
    gz_mixed = b"".join(HDR + w + struct.pack("<II", crc, n) + sm * 8 for w, _, crc, n in parts)
    files, central, at = [], [], 0
    for k, (w, _, crc, n) in enumerate(parts):
        name = b"e%d" % k
        files.append(struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, len(w), n, len(name), 0) + name + w)
        central.append(struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", 20, 20, 0x0800, 8, 0, 0x0021, crc, len(w), n,
                                   len(name), 0, 0, 0, 0, 0, at) + name)
        at += len(files[-1])
    cd = b"".join(central)
    zf = b"".join(files) + cd + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, PARTS, PARTS, len(cd), at, 0)
    for name, b in (("one", one), ("gz", gz), ("gz_mixed", gz_mixed), ("zip", zf)):
        with open(os.path.join(TMP, name), "wb") as f:
            f.write(b)
    print("gen ok", len(one), len(gz), len(gz_mixed), len(zf))


def timed(tag):
    import torch
    load = lambda n: torch.from_numpy(np.fromfile(os.path.join(TMP, n), np.uint8)).cuda()
    one, gz, gzm, zf = load("one"), load("gz"), load("gz_mixed"), load("zip")
    total = MIB << 20
    mixed_total = total + PARTS * 8 * 4096
    out = torch.empty(mixed_total + 64, dtype=torch.uint8, device="cuda")
    eng = flate.FlateEngine(0)
    rng = np.random.RandomState(5)
    begin = np.sort(rng.randint(0, total - (1 << 20), 64)).astype(np.uint64)
    end = begin + np.uint64(1 << 20)
    res = {"tag": tag, "lib": os.environ.get("FLATE_HIP_LIB", "tree"), "mib": MIB, "reps": REPS, "build_id": flate.build_id()}

    def run(name, fn, ok):
        ts = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        assert ok(r), (name, r if not isinstance(r, tuple) else r[1])
        ts = sorted(ts[1:])
        res[name] = {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}
        return r

    run("A_inflate_one", lambda: eng.inflate_one(one, "gzip", out=out), lambda r: r[1].rc == 0 and r[1].out_len == total)
    si = run("B_one_seek_index", lambda: eng.inflate_one_seek_index(one, "gzip", span=1 << 20), lambda r: r.rc == 0)
    run("C_one_ranges", lambda: eng.inflate_one_ranges(one, si, begin, end, out=out, wrap="gzip"), lambda r: r[1].rc == 0)
    run("D_gzfile_read", lambda: eng.gzfile_read(gz, out=out), lambda r: r[1].rc == 0 and r[1].out_len == total)
    eng.set_option("gzfile_serial_max", 1 << 20)
    run("D_gzfile_read_serial", lambda: eng.gzfile_read(gzm, out=out), lambda r: r[1].rc == 0 and r[1].out_len == mixed_total)
    eng.set_option("gzfile_serial_max", 0)
    gi = run("E_gzfile_seek_index", lambda: eng.gzfile_seek_index(gz, span=1 << 20), lambda r: r.rc == 0)
    run("F_gzfile_ranges", lambda: eng.gzfile_ranges(gz, gi, begin, end, out=out), lambda r: r[1].rc == 0)
    eng.set_option("zip_unit_min", 1)
    run("G_zip_read_units", lambda: eng.zip_read(zf, out=out), lambda r: r[1].rc == 0 and eng.zip_last_route()[0] == PARTS)
    eng.close()
    out_dir = os.path.join(os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results")), "unit_rounds_ab")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, tag + ".json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    gen() if sys.argv[1] == "gen" else timed(sys.argv[2])
