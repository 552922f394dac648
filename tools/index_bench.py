#!/usr/bin/env python3
"""The whole calls that run a discovery (chain_walk.h), timed on the workloads DESIGN.md records figures for.

    python tools/index_bench.py [--reps 5] [--one-mib 256] [--only bgzf,gzip,zip,one] [--no-check]

1 GiB of S-text is written on the device as a BGZF file (default block size), as the 16 384 gzip members
flate_hip_deflate_fast_batch_framed writes, and as a ZIP archive of 16 384 entries of 64 KiB; --one-mib MiB of it is
compressed by zlib at level 6 into ONE gzip member (tools/one_bench.py's, on the CPU).  Timed with device pointers, host
time around the synchronous call, one warm-up call (it sizes the ctx's scratch) and then --reps: flate_hip_bgzf_index,
flate_hip_bgzf_read, flate_hip_gzip_index, flate_hip_gzip_read, flate_hip_zip_index, flate_hip_inflate_one_index.  Every
call's result is compared once with the CPU: the BGZF index with a walk over BSIZE and ISIZE, the gzip index with zlib's
own reader over the file, the ZIP index with zipfile's, the reads with the input, the one-stream index with the
stream's size.  To compare two builds, run it once per library (FLATE_HIP_LIB), each in a process of its own, and set
the lines side by side.  For a per-kernel split run it under a kernel trace with --reps 1 --no-check.  Prints one JSON
line; also written to $FLATE_OUT_ROOT (default results/)/index_bench.json."""
import argparse
import importlib
import io
import json
import os
import struct
import sys
import time
import zipfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")

N, BLEN = 16384, 65536


def bgzf_walk(f):
    """(member_off, out_off) of a well-formed BGZF file whose members carry BSIZE at byte 16."""
    moff, ooff, p = [], [0], 0
    while p < len(f):
        total = struct.unpack_from("<H", f, p + 16)[0] + 1
        moff.append(p)
        ooff.append(ooff[-1] + struct.unpack_from("<I", f, p + total - 4)[0])
        p += total
    return moff + [len(f)], ooff


def gzip_walk(f):
    moff, ooff, p = [], [0], 0
    while p < len(f):
        d = zlib.decompressobj(31)
        n = len(d.decompress(f[p:p + 2 * BLEN + 4096]))
        assert d.eof
        moff.append(p)
        ooff.append(ooff[-1] + n)
        p += min(len(f) - p, 2 * BLEN + 4096) - len(d.unused_data)
    return moff + [len(f)], ooff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-mib", type=int, default=256)
    ap.add_argument("--only", default="bgzf,gzip,zip,one")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch

    only, check = set(a.only.split(",")), not a.no_check
    eng = flate.FlateEngine(0)
    plain = flate.synth("text", N, BLEN)
    d_plain = torch.from_numpy(plain).cuda()
    off = flate.uniform_offsets(N, BLEN)
    out = torch.empty(plain.size + 64, dtype=torch.uint8, device="cuda")
    res = {"what": "whole calls, device pointers, ms: best and all of --reps behind one warm-up call", "plain_bytes": int(plain.size),
           "reps": a.reps, "checked_against_the_cpu": check, "build_id": flate.build_id()}

    def timed(name, fn):
        times = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            times.append(round((time.perf_counter() - t0) * 1e3, 3))
        res[name + "_ms_best"], res[name + "_ms_all"] = min(times[1:]), times[1:]
        return r

    def same(d_file, n):
        return bool((out[:n] == d_file[:n]).all())

    if "bgzf" in only:
        d_f, n_f = eng.bgzf_write(d_plain)
        d_f = d_f[:n_f].clone()
        res["bgzf_file_bytes"] = n_f
        ix = timed("bgzf_index", lambda: eng.bgzf_index(d_f, index_cap=plain.size // 65280 + 4))
        _, rd = timed("bgzf_read", lambda: eng.bgzf_read(d_f, out=out))
        assert (ix.rc, rd.rc, rd.out_len) == (0, 0, plain.size), (ix, rd)
        if check:
            moff, ooff = bgzf_walk(d_f.cpu().numpy().tobytes())
            assert ix.member_off.tolist() == moff and ix.out_off.tolist() == ooff and same(d_plain, plain.size), "bgzf"
        res["bgzf_members"] = ix.n_members
        del d_f
    if "gzip" in only:
        d_f, f_off = eng.deflate_batch_framed(d_plain, off, "gzip")
        d_f = d_f[:int(f_off[-1])].clone()
        res["gzip_file_bytes"] = int(f_off[-1])
        ix = timed("gzip_index", lambda: eng.gzip_index(d_f, index_cap=N + 1))
        _, rd = timed("gzip_read", lambda: eng.gzip_read(d_f, out=out))
        assert (ix.rc, rd.rc, rd.out_len) == (0, 0, plain.size), (ix, rd)
        if check:
            moff, ooff = gzip_walk(d_f.cpu().numpy().tobytes())
            assert ix.member_off.tolist() == moff and ix.out_off.tolist() == ooff and same(d_plain, plain.size), "gzip"
        res["gzip_members"], res["gzip_candidates"] = ix.n_members, ix.n_candidates
        del d_f
    if "zip" in only:
        d_f, n_f = eng.zip_write(d_plain, off, ["entry-%05d.txt" % i for i in range(N)])
        d_f = d_f[:n_f].clone()
        res["zip_file_bytes"] = n_f
        ix = timed("zip_index", lambda: eng.zip_index(d_f))
        assert (ix.rc, ix.n_entries, ix.out_bytes) == (0, N, plain.size), ix
        if check:
            infos = zipfile.ZipFile(io.BytesIO(d_f.cpu().numpy().tobytes())).infolist()
            e = ix.entries
            assert [i.filename for i in infos] == ix.names and e["header_off"].tolist() == [i.header_offset for i in infos], "zip"
            assert e["comp_size"].tolist() == [i.compress_size for i in infos] and e["crc32"].tolist() == [i.CRC for i in infos], "zip"
            assert e["size"].tolist() == [i.file_size for i in infos] and not e["status"].any(), "zip"
        del d_f
    if "one" in only:
        part = plain[:a.one_mib << 20]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = co.compress(part.tobytes()) + co.flush()
        member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(part), part.size & 0xffffffff)
        d_f = torch.from_numpy(np.frombuffer(member, np.uint8).copy()).cuda()
        res["one_member_bytes"], res["one_plain_bytes"] = len(member), int(part.size)
        ix = timed("inflate_one_index", lambda: eng.inflate_one_index(d_f, "gzip"))
        assert ix.rc == 0 and ix.out_bytes == part.size and int(ix.out_off[-1]) == part.size and int(ix.unit_bit[0]) == 0, ix
        assert (np.diff(ix.unit_bit.astype(np.int64)) > 0).all() and (np.diff(ix.out_off.astype(np.int64)) >= 0).all()
        res["one_units"], res["one_candidates"] = ix.n_units, ix.n_candidates
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "index_bench.json"), "w") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
