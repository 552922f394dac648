#!/usr/bin/env python3
"""The packed windows of the seek index of one long gzip member: flate_hip_seek_windows_pack and
flate_hip_inflate_one_ranges_packed against the raw windows of the same index.

    python tools/seek_pack_bench.py [--mib 1024] [--level 6] [--reps 5] [--spans 1048576,65536]
    python tools/seek_pack_bench.py --untouched [--mib 1024] [--reps 5]

The input is tools/seek_bench.py's: --mib MiB of S-text compressed with zlib at --level into ONE gzip member (on the
CPU, once), on the device; whole calls with device pointers, best of --reps after one call that sizes the ctx's scratch.
Per span:
  sizes   the windows raw / COMPRESS / COMPRESS | SPARSE, the share of kept bytes, the empty blocks
  pack    both modes, ALTERNATED with the build call pair by pair on the same card
  (c)     4096 random ranges of 64 KiB through flate_hip_inflate_one_ranges_packed (both modes), alternated with
          flate_hip_inflate_one_ranges on the raw windows          (d) one range of 1 byte, the same pairs
`spread` is the largest difference between two calls of the same kind inside the alternated pairs: a difference between
the kinds below it says nothing.  Every delivered range is compared with the input on the device.
--untouched: flate_hip_inflate_one and flate_hip_inflate_one_ranges (4096 ranges, span 1 MiB) alone, for a run per
library (FLATE_HIP_LIB) alternated process by process: the calls this feature must leave what they were.
Prints one JSON line; also written to $FLATE_OUT_ROOT (default results/)/seek_pack_bench[_untouched].json."""
import argparse
import importlib
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
flate = importlib.import_module("moonbit-flate_amd")
from one_bench import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spans", default="1048576,65536")
    ap.add_argument("--untouched", action="store_true")
    a = ap.parse_args()
    import torch

    plain = workload("text", a.mib)
    co = zlib.compressobj(a.level, zlib.DEFLATED, -15)
    raw = co.compress(plain.tobytes()) + co.flush()
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain), plain.size & 0xffffffff)
    T = int(plain.size)
    eng = flate.FlateEngine(0)
    d = torch.from_numpy(np.frombuffer(member, np.uint8).copy()).cuda()
    out = torch.empty(T + 16, dtype=torch.uint8, device="cuda")
    d_plain = torch.from_numpy(plain).cuda()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, round((time.perf_counter() - t0) * 1e3, 3)

    def alternated(*fns):
        """reps + 1 rounds over fns; the first round sizes the scratch -> (last results, the times per fn)."""
        times, res = [[] for _ in fns], [None] * len(fns)
        for _ in range(a.reps + 1):
            for k, fn in enumerate(fns):
                res[k], t = timed(fn)
                times[k].append(t)
        return res, times

    def spread(*lists):
        return round(max(max(t[1:]) - min(t[1:]) for t in lists), 3)

    rng = np.random.default_rng(5)
    begin = rng.integers(0, max(T - 65536, 1), 4096).astype(np.uint64)
    end = np.minimum(begin + np.uint64(65536), np.uint64(T))
    at = T // 2 + 12345
    res = {"what": "one gzip member, device pointers, whole calls, ms", "plain_bytes": T, "member_bytes": len(member),
           "zlib_level": a.level, "build_id": flate.build_id(), "lib": os.environ.get("FLATE_HIP_LIB", "")}

    def same(o, r, b, e, which):
        for k in which:
            assert bool((o[int(r.out_off[k]):int(r.out_off[k + 1])] == d_plain[int(b[k]):int(e[k])]).all()), k

    if a.untouched:
        s = eng.inflate_one_seek_index(d, "gzip", 1 << 20)
        assert s.rc == 0
        (r_one, r_rng), (t_one, t_rng) = alternated(lambda: eng.inflate_one(d, "gzip", out=out),
                                                    lambda: eng.inflate_one_ranges(d, s, begin, end, out=out))
        assert r_one[1].rc == 0 and r_rng[1].rc == 0
        res.update(inflate_one_ms_best=min(t_one[1:]), inflate_one_ms_all=t_one, ranges_4096_ms_best=min(t_rng[1:]),
                   ranges_4096_ms_all=t_rng, spread_ms=spread(t_one, t_rng))
        name = "seek_pack_bench_untouched.json"
    else:
        for span in [int(x) for x in a.spans.split(",")]:
            build = lambda: eng.inflate_one_seek_index(d, "gzip", span)
            s = build()
            assert s.rc == 0
            packs = {}
            (pc, ps, _), (t_c, t_s, t_b) = alternated(lambda: eng.seek_windows_pack(s, None, sparse=False),
                                                      lambda: eng.seek_windows_pack(s, d, sparse=True), build)
            assert pc.rc == 0 and ps.rc == 0, (pc.rc, ps.rc)
            # the packs hold what they say: COMPRESS unpacks to the build's windows
            w, u = eng.seek_windows_unpack(pc)
            assert u.rc == 0 and bool((w == s.windows).all()), "COMPRESS does not unpack to the windows"
            nb = s.n_points - 1
            sz = {"n_points": s.n_points, "n_units": s.n_units, "index_bytes": int(s.index.size) * 8,
                  "windows_raw_bytes": int(s.windows.numel()), "pack_index_bytes": int(pc.pack_index.size) * 8,
                  "compress_bytes": pc.packed_bytes, "sparse_bytes": ps.packed_bytes, "kept_bytes": ps.kept_bytes,
                  "kept_share": round(ps.kept_bytes / max(nb * 32768, 1), 4),
                  "compress_empty_blocks": int((np.diff(pc.pack_index[16:].astype(np.int64)) == 0).sum()),
                  "sparse_empty_blocks": int((np.diff(ps.pack_index[16:].astype(np.int64)) == 0).sum()),
                  "pack_compress_ms_best": min(t_c[1:]), "pack_compress_ms_all": t_c, "pack_sparse_ms_best": min(t_s[1:]),
                  "pack_sparse_ms_all": t_s, "build_ms_best": min(t_b[1:]), "build_ms_all": t_b, "pack_spread_ms": spread(t_c, t_s, t_b)}
            for tag, b, e in (("c_4096_ranges_64k", begin, end), ("d_one_byte", [at], [at + 1])):
                b, e = np.asarray(b, np.uint64), np.asarray(e, np.uint64)
                (r_raw, r_c, r_s), (t_raw, t_pc, t_ps) = alternated(
                    lambda: eng.inflate_one_ranges(d, s, b, e, out=out),
                    lambda: eng.inflate_one_ranges_packed(d, s.index, pc, b, e, out=out),
                    lambda: eng.inflate_one_ranges_packed(d, s.index, ps, b, e, out=out))
                for o, r in (r_raw, r_c, r_s):
                    assert r.rc == 0 and int(r.out_off[-1]) == int((e - b).sum()), r
                for fn in (lambda: eng.inflate_one_ranges_packed(d, s.index, pc, b, e, out=out),
                           lambda: eng.inflate_one_ranges_packed(d, s.index, ps, b, e, out=out)):
                    o, r = fn()
                    same(o, r, b, e, sorted({0, len(b) // 2, len(b) - 1}))
                sz.update({tag + "_raw_ms_best": min(t_raw[1:]), tag + "_raw_ms_all": t_raw,
                           tag + "_compress_ms_best": min(t_pc[1:]), tag + "_compress_ms_all": t_pc,
                           tag + "_sparse_ms_best": min(t_ps[1:]), tag + "_sparse_ms_all": t_ps,
                           tag + "_spread_ms": spread(t_raw, t_pc, t_ps), tag + "_n_decoded": r_s[1].n_decoded})
            res["span_%d" % span] = sz
            del s, pc, ps, w
        name = "seek_pack_bench.json"
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, name), "w") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
