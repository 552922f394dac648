"""Timing guards of batch deflate with preset dictionaries (flate_hip_deflate_fast_batch_dict).  RATIOS on the same
box in the same test (no absolute milliseconds), in the style of tests/test_gpu_inflate_dict_perf.py: best of a
few runs of the match finder's plus the entropy stage's kernel time, data resident on the device, S-text payloads
and a 32 KiB S-text dictionary from another seed, FLATE_HIP_COMPAT_GO (the mode in which a dictionary is used).

Measured on 1 x MI355X (best of 4): 65536 x 4 KiB 6.34 ms with the shared dictionary against 38.06 ms with it pasted in
front of every stream (0.167 x); 16384 x 64 KiB 20.37 ms against 17.64 ms plain (1.155 x).  DESIGN.md section 4.1."""
import numpy as np
import pytest

from util import flate

pytestmark = pytest.mark.gpu


def _best_ms(eng, run, reps):
    best = 1e9
    for _ in range(reps):
        run()
        t = eng.last_timing()
        best = min(best, t["lz77_match"] + t["huff_pack"])
    return best


def _setup(n, blen):
    import torch
    eng = flate.FlateEngine(0)
    eng.set_profiling(True)
    zd = flate.synth("text", 1, 32768, seed=77).tobytes()
    host = flate.synth("text", n, blen)
    return eng, zd, host, torch


def test_priming_is_shared_by_the_streams_of_a_dictionary():
    """65536 x 4 KiB payloads with one dictionary against the plain call on the same payloads with the dictionary
    pasted in front of each (65536 x 36 KiB): what priming per stream would cost.  Required: less than half."""
    n, blen = 65536, 4096
    eng, zd, host, torch = _setup(n, blen)
    try:
        d = torch.from_numpy(host).cuda()
        off = flate.uniform_offsets(n, blen)
        out = torch.empty(n * blen + (n * blen >> 2) + 4096, dtype=torch.uint8, device="cuda")
        with_dict = _best_ms(eng, lambda: eng.deflate_batch(d, off, out=out, compat_go=True, zdicts=zd), 4)
        csize = int(eng.deflate_batch(d, off, out=out, compat_go=True, zdicts=zd)[1][-1])
        plain = _best_ms(eng, lambda: eng.deflate_batch(d, off, out=out, compat_go=True), 4)
        psize = int(eng.deflate_batch(d, off, out=out, compat_go=True)[1][-1])
        del out
        dl = len(zd)
        pasted = torch.empty(n * (dl + blen) + 16, dtype=torch.uint8, device="cuda")
        view = pasted[:n * (dl + blen)].view(n, dl + blen)
        view[:, :dl] = torch.from_numpy(np.frombuffer(zd, dtype=np.uint8).copy()).cuda()
        view[:, dl:] = d[:n * blen].view(n, blen)
        del d, view
        poff = flate.uniform_offsets(n, dl + blen)
        pout = torch.empty(n * (dl + blen) // 2 + 4096, dtype=torch.uint8, device="cuda")
        per_stream = _best_ms(eng, lambda: eng.deflate_batch(pasted, poff, out=pout, compat_go=True), 3)
        gib = n * blen / 2.0 ** 30
        print("deflate 65536 x 4 KiB: with a shared 32 KiB dictionary %.2f ms (%.1f GiB/s of payload, ratio %.3f), "
              "plain %.2f ms (%.1f GiB/s, ratio %.3f); dictionary pasted in front of every stream %.2f ms -> %.3f x"
              % (with_dict, gib / with_dict * 1e3, n * blen / csize, plain, gib / plain * 1e3, n * blen / psize,
                 per_stream, with_dict / per_stream))
        assert with_dict < 0.5 * per_stream, "%.2f ms with a shared dictionary, %.2f ms priming per stream" \
            % (with_dict, per_stream)
    finally:
        eng.close()


def test_a_dictionary_nobody_needs_costs_little():
    """16384 x 64 KiB payloads, same dictionary, against the plain call on the same payloads.  The streams run
    through the multi-window build from a table snapshot: gate at 1.5 x the plain call's time."""
    n, blen = 16384, 65536
    eng, zd, host, torch = _setup(n, blen)
    try:
        d = torch.from_numpy(host).cuda()
        off = flate.uniform_offsets(n, blen)
        out = torch.empty(n * blen + (n * blen >> 3) + 4096, dtype=torch.uint8, device="cuda")
        plain = _best_ms(eng, lambda: eng.deflate_batch(d, off, out=out, compat_go=True), 4)
        psize = int(eng.deflate_batch(d, off, out=out, compat_go=True)[1][-1])
        with_dict = _best_ms(eng, lambda: eng.deflate_batch(d, off, out=out, compat_go=True, zdicts=zd), 4)
        csize = int(eng.deflate_batch(d, off, out=out, compat_go=True, zdicts=zd)[1][-1])
        gib = n * blen / 2.0 ** 30
        print("deflate 16384 x 64 KiB: with a shared 32 KiB dictionary %.2f ms (%.1f GiB/s of payload, ratio %.3f), "
              "plain %.2f ms (%.1f GiB/s, ratio %.3f) -> %.3f x"
              % (with_dict, gib / with_dict * 1e3, n * blen / csize, plain, gib / plain * 1e3, n * blen / psize,
                 with_dict / plain))
        assert with_dict < 1.5 * plain, "%.2f ms with a dictionary, %.2f ms without" % (with_dict, plain)
    finally:
        eng.close()
