#!/usr/bin/env python3
"""flate_hip_zip_write with the option "zip_piece_bytes" (long entries written from pieces, spliced into one stream)
against the option at 0, on S-text resident on the device.

    python tools/zip_write_bench.py [--mib 64] [--reps 5] [--only ABCD] [--parent-lib PATH]

  (A) ONE entry of --mib MiB              option off against P = 65535, 256 KiB, 1 MiB: times and archive sizes (the size
                                          is the ratio cost of piece boundaries: pieces share no history);
  (B) 16 entries of --mib MiB             off against on (P = 256 KiB);
  (C) --mib * 256 entries of 64 KiB       P = 65536 against option 0: no entry is longer than P, so both take the same
                                          route and must lie inside each other's spread;
  (D) the archive of (C), option 0, against the library at --parent-lib (the parent commit's build), through ctypes on
      the same card: the path is unchanged.
Device pointers, whole calls, best of --reps, the two calls of a pair ALTERNATED on the same card (a, b, a, b, ...; the
first call of each sizes the ctx's scratch and is not counted).  Every option-on archive is read back once on the device
(flate_hip_zip_read) and compared with the input.  Prints one JSON line; also written to $FLATE_OUT_ROOT (default
results/)/zip_write_bench.json."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
flate = importlib.import_module("moonbit-flate_amd")
SIZES = {"65535": 65535, "256 KiB": 256 << 10, "1 MiB": 1 << 20}


def tables(n, size):
    in_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(size)).astype(np.uint64)
    names = b"".join(b"e%d" % k for k in range(n))
    name_off = np.zeros(n + 1, np.uint64)
    np.cumsum([len(b"e%d" % k) for k in range(n)], out=name_off[1:])
    return in_off, np.frombuffer(names, np.uint8).copy(), name_off


def raw_zip_write(L, ctx, d, in_off, names, name_off, out):
    """ONE flate_hip_zip_write call, device pointers -> (rc, archive bytes)."""
    n = in_off.size - 1
    out_len = C.c_uint64(0)
    rc = L.flate_hip_zip_write(ctx, d.data_ptr(), in_off.ctypes.data, n, names.ctypes.data, name_off.ctypes.data,
                               out.data_ptr(), out.numel(), C.byref(out_len), None, 1)
    return rc, int(out_len.value)


class ParentLib:
    """flate_hip_zip_write of another build of the library, through ctypes alone."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.flate_hip_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        self.L.flate_hip_zip_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
        self.L.flate_hip_build_id.restype = C.c_char_p
        self.L.flate_hip_destroy.argtypes = [C.c_void_p]
        self.ctx = C.c_void_p()
        assert self.L.flate_hip_init(0, C.byref(self.ctx)) == 0
        self.build_id = self.L.flate_hip_build_id().decode()

    def close(self):
        self.L.flate_hip_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="ABCD")
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    import torch

    eng = flate.FlateEngine(0)
    res = {"what": "flate_hip_zip_write on S-text, device pointers, whole calls, ms, pairs alternated",
           "entry_mib": a.mib, "reps": a.reps, "build_id": flate.build_id()}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()  # (every call ends with a read-back of its result words behind a synchronise)
        return r, (time.perf_counter() - t0) * 1e3

    def pair(ours, theirs):
        t_a, t_b, r_a, r_b = [], [], None, None
        for _ in range(a.reps + 1):
            r_a, t = timed(ours)
            assert r_a[0] == 0, r_a
            t_a.append(round(t, 3))
            if theirs:
                r_b, t = timed(theirs)
                assert r_b[0] == 0, r_b
                t_b.append(round(t, 3))
        return t_a, t_b, r_a, r_b

    def best(ts):
        return min(ts[1:])

    def spread(ts):
        return round(max(ts[1:]) - min(ts[1:]), 3)

    def workload(n, size):
        plain = flate.synth("text", n, size)
        in_off, names, name_off = tables(n, size)
        bound = int(eng._L.flate_hip_zip_bound(in_off.ctypes.data, n, name_off.ctypes.data)) + 340 * (n * size // 65535 + n)
        return plain, torch.from_numpy(plain).cuda(), in_off, names, name_off, torch.empty(bound, dtype=torch.uint8, device="cuda")

    def write(w, P):
        eng.set_option("zip_piece_bytes", P)
        return raw_zip_write(eng._L, eng._ctx, w[1], w[2], w[3], w[4], w[5])

    def reads_back(w, nbytes):
        """the archive in w's output, read on the device, is the input"""
        eng.set_option("zip_unit_min", 1)
        back, r = eng.zip_read(w[5][:nbytes])
        eng.set_option("zip_unit_min", 0)
        assert r.rc == 0 and int(r.out_off[-1]) == w[0].size
        assert bool((back[:w[0].size] == w[1]).all()), "the archive does not read back as the input"

    for key in a.only:
        if key == "A":
            w = workload(1, a.mib << 20)
            row = {"entries": 1}
            for k, (label, P) in enumerate(SIZES.items()):
                t_on, t_off, r_on, r_off = pair(lambda: write(w, P), (lambda: write(w, 0)) if k == 0 else None)
                assert write(w, P) == r_on  # (the pair's last call was the other one's)
                route = eng.zip_write_last_route()
                reads_back(w, r_on[1])
                row[label] = {"on_ms_best": best(t_on), "on_ms_all": t_on, "archive_bytes": r_on[1], "pieces": route[1]}
                if k == 0:
                    row["off"] = {"ms_best": best(t_off), "ms_all": t_off, "archive_bytes": r_off[1],
                                  "mib_per_s": round(a.mib / (best(t_off) * 1e-3), 1)}
            row["fastest"] = min(SIZES, key=lambda s: row[s]["on_ms_best"])
        elif key == "B":
            w = workload(16, a.mib << 20)
            P = SIZES["256 KiB"]
            t_on, t_off, r_on, r_off = pair(lambda: write(w, P), lambda: write(w, 0))
            assert write(w, P) == r_on  # (the pair's last call was the other one's)
            reads_back(w, r_on[1])
            row = {"entries": 16, "P": P, "on_ms_best": best(t_on), "on_ms_all": t_on, "off_ms_best": best(t_off),
                   "off_ms_all": t_off, "on_archive_bytes": r_on[1], "off_archive_bytes": r_off[1]}
        elif key in "CD":
            n = a.mib * 256
            w = workload(n, 65536)
            if key == "C":
                t_on, t_off, r_on, r_off = pair(lambda: write(w, 65536), lambda: write(w, 0))
                assert eng.zip_write_last_route() == (0, 0) and r_on == r_off
                row = {"entries": n, "p65536_ms_best": best(t_on), "p65536_ms_all": t_on, "off_ms_best": best(t_off),
                       "off_ms_all": t_off, "spread_ms": {"p65536": spread(t_on), "off": spread(t_off)}}
            else:
                assert a.parent_lib, "(D) needs --parent-lib"
                par = ParentLib(a.parent_lib)
                t_off, t_par, r_off, r_par = pair(lambda: write(w, 0),
                                                  lambda: raw_zip_write(par.L, par.ctx, w[1], w[2], w[3], w[4], w[5]))
                assert r_off == r_par
                row = {"entries": n, "off_ms_best": best(t_off), "off_ms_all": t_off, "parent_build_id": par.build_id,
                       "parent_ms_best": best(t_par), "parent_ms_all": t_par,
                       "spread_ms": {"this": spread(t_off), "parent": spread(t_par)}}
                par.close()
        else:
            continue
        del w
        res[key] = row
        print(json.dumps({key: row}), file=sys.stderr, flush=True)
    eng.close()
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "zip_write_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
