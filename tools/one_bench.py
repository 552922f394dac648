#!/usr/bin/env python3
"""flate_hip_inflate_one on one long gzip member, against flate_hip_inflate_stream_read on the same file.

    python tools/one_bench.py [--mib 1024] [--level 6] [--reps 5] [--serial-seconds 150]
                              [--workload text|random|mixed] [--stored-units]

Builds --mib MiB of S-text, compresses it with zlib at --level into ONE gzip member (on the CPU, once), puts the member
on the device and times, best of --reps, whole calls with device pointers: flate_hip_inflate_one (discovery, decode,
checksum; the output is compared with the input once) and flate_hip_inflate_one_index (discovery alone), with n_units
and n_candidates.  The comparison is flate_hip_inflate_stream_read, the call that read such a member before: the raw
stream fed from host memory (the call takes nothing else) in 64 MiB pieces with room for 256 MiB of output per call.  It
runs for at most --serial-seconds; if that does not reach the end of the stream, the time for the whole stream is its
measured rate extrapolated and labelled so.  For a per-kernel split run this script under a kernel trace with --reps 1
--serial-seconds 0.  --workload: S-text (the default), random bytes (zlib writes them as stored blocks of about 16 KiB),
or 1 MiB of S-text and 1 MiB of random bytes in turn.  --stored-units sets the option "one_stored_units", so that stored
block headers start units too; without it a run of stored blocks is one unit, and a call that refuses the member
(FLATE_HIP_E_TOO_LARGE for a unit of 2^28 bytes) is recorded, not timed.  Prints one JSON line; also written to $FLATE_OUT_ROOT (default results/)/one_bench.json."""
import argparse
import ctypes as C
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
flate = importlib.import_module("moonbit-flate_amd")


def serial(eng, raw, limit_s):
    """flate_hip_inflate_stream_read over raw until its end or limit_s -> (bytes out, seconds, reached the end)."""
    L = eng._L
    st = C.c_void_p()
    eng._check(L.flate_hip_inflate_stream_open(eng._ctx, C.byref(st)))
    src = np.frombuffer(raw, np.uint8)
    room = np.empty(1 << 28, np.uint8)
    used, n, eo = C.c_uint64(0), C.c_uint64(0), C.c_int64(-1)
    pos, got, rc, piece = 0, 0, 0, 1 << 26
    t0 = time.perf_counter()
    while rc == 0 and time.perf_counter() - t0 < limit_s:
        take = min(piece, src.size - pos)
        rc = L.flate_hip_inflate_stream_read(st, src.ctypes.data + pos, take, 1 if pos + take == src.size else 0,
                                             room.ctypes.data, room.size, C.byref(used), C.byref(n), C.byref(eo))
        pos += used.value
        got += n.value
    dt = time.perf_counter() - t0
    L.flate_hip_inflate_stream_free(st)
    return got, dt, rc == 1


def workload(kind, mib):
    """mib MiB of plain bytes: S-text, random bytes, or 1 MiB of each in turn."""
    if kind == "text":
        return flate.synth("text", mib * 16, 65536)
    rnd = np.random.default_rng(7).integers(0, 256, mib << 20, dtype=np.uint8)
    if kind == "mixed":
        text = flate.synth("text", mib * 16, 65536).reshape(mib, 1 << 20)
        rnd = rnd.reshape(mib, 1 << 20)
        rnd[0::2] = text[0::2]
    return rnd.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--serial-seconds", type=float, default=150)
    ap.add_argument("--workload", choices=("text", "random", "mixed"), default="text")
    ap.add_argument("--stored-units", action="store_true")
    a = ap.parse_args()
    import torch

    plain = workload(a.workload, a.mib)
    co = zlib.compressobj(a.level, zlib.DEFLATED, -15)
    raw = co.compress(plain.tobytes()) + co.flush()
    member = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain), plain.size & 0xffffffff)
    eng = flate.FlateEngine(0)
    eng.set_option("one_stored_units", 1 if a.stored_units else 0)
    d = torch.from_numpy(np.frombuffer(member, np.uint8).copy()).cuda()
    out = torch.empty(plain.size + 16, dtype=torch.uint8, device="cuda")

    def best(fn):
        times = []
        for _ in range(a.reps + 1):  # (the first call sizes the ctx's scratch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return r, [round(t, 3) for t in times]

    res = {"workload": a.workload, "one_stored_units": int(a.stored_units)}
    (_, rd), t_one = best(lambda: eng.inflate_one(d, "gzip", out=out))
    if rd.rc == -6:  # a unit of 2^28 bytes of input or more: the member is refused whole
        res.update({"what": "one gzip member: refused", "status": "FLATE_HIP_E_TOO_LARGE", "plain_bytes": int(plain.size),
                    "member_bytes": len(member), "n_units": rd.n_units, "n_candidates": rd.n_candidates,
                    "build_id": flate.build_id()})
        print(json.dumps(res))
        eng.close()
        return
    assert rd.rc == 0 and rd.out_len == plain.size, rd
    assert bool((out[:plain.size].cpu() == torch.from_numpy(plain)).all()), "the output is not the input"
    ix, t_ix = best(lambda: eng.inflate_one_index(d, "gzip", query=True))
    res.update({
        "what": "one gzip member, device pointers, whole calls, ms",
        "plain_bytes": int(plain.size), "member_bytes": len(member), "zlib_level": a.level,
        "inflate_one_ms_best": min(t_one[1:]), "inflate_one_ms_all": t_one,
        "inflate_one_gib_per_s": round(plain.size / 2**30 / (min(t_one[1:]) * 1e-3), 2),
        "index_ms_best": min(t_ix[1:]), "index_ms_all": t_ix,
        "n_units": ix.n_units, "n_candidates": ix.n_candidates,
        "decoys_per_gib_of_input": round((ix.n_candidates - ix.n_units) * (1 << 30) / len(raw)),
        "build_id": flate.build_id(),
    })
    print(json.dumps(res), file=sys.stderr, flush=True)
    if a.serial_seconds > 0:
        got, dt, done = serial(eng, raw, a.serial_seconds)
        whole = dt if done else dt * plain.size / max(got, 1)
        res.update({"stream_read_bytes": int(got), "stream_read_seconds": round(dt, 2), "stream_read_reached_the_end": done,
                    "stream_read_whole_stream_seconds": round(whole, 2),
                    "stream_read_whole_stream_is": "measured" if done else "extrapolated from the measured rate",
                    "ratio": round(whole / (min(t_one[1:]) * 1e-3), 1)})
    line = json.dumps(res)
    print(line)
    out_root = os.environ.get("FLATE_OUT_ROOT", os.path.join(ROOT, "results"))
    os.makedirs(out_root, exist_ok=True)
    with open(os.path.join(out_root, "one_bench.json"), "w") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
