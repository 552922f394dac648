"""Timing guard of the decoders' dictionary builds: a batch whose streams carry a 32 KiB dictionary that none of
them references must decode about as fast as the same batch through the plain call.  A RATIO on the same box in
the same test (no absolute milliseconds), in the style of tests/test_gpu_perf_guard.py."""
import numpy as np
import pytest

from util import flate

pytestmark = pytest.mark.gpu


def _best_inflate_ms(eng, run, reps):
    best = 1e9
    for _ in range(reps):
        run()
        best = min(best, eng.last_timing()["inflate"])
    return best


@pytest.mark.parametrize("decoder", ["sub_block_default", "lane_per_stream"])
def test_unreferenced_dictionary_costs_little(decoder):
    import torch
    n, blen = 16384, 65536
    eng = flate.FlateEngine(0)
    try:
        eng.set_profiling(True)
        if decoder == "lane_per_stream":
            eng.set_option("inflate_spec", 0)
            eng.set_option("inflate_simt_min_streams", 0)
        d = torch.from_numpy(flate.synth("text", n, blen)).cuda()
        off = flate.uniform_offsets(n, blen)
        comp, coff = eng.deflate_batch(d, off)
        del d
        sizes = np.full(n, blen, dtype=np.uint64)
        out = torch.empty(n * blen + 16, dtype=torch.uint8, device="cuda")
        zd = flate.synth("rand", 1, 32768, seed=3).tobytes()
        plain = _best_inflate_ms(eng, lambda: eng.inflate_batch(comp, coff, sizes, out=out), 4)
        with_dict = _best_inflate_ms(eng, lambda: eng.inflate_batch(comp, coff, sizes, out=out, zdicts=zd), 4)
        st = eng.inflate_batch(comp, coff, sizes, out=out, zdicts=zd)[3]
        assert (st == 0).all()
        print("inflate %s: plain %.2f ms, with an unreferenced 32 KiB dictionary %.2f ms (%.3f x)"
              % (decoder, plain, with_dict, with_dict / plain))
        assert with_dict < 1.15 * plain, "%s: %.2f ms with a dictionary, %.2f ms without" % (decoder, with_dict, plain)
    finally:
        eng.close()
