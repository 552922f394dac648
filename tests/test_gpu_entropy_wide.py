"""The entropy stage's wide tiles (huff_pack_kernels.hip: 512 positions per walk step, eight per lane) at their
edges, byte for byte against oracle.deflate in both compat modes:
  * stream lengths around every multiple of 256 and 512, one block and several, for inputs that give 258-byte
    matches (S-zero), no matches (S-rand: the literal-only loops), short ones (S-ramp) and a mix (S-text);
  * neighbouring blocks with odd numbers of 256-position rows, whose last wide tile reaches into the first row of
    the next block's hand-over bytes (tile_meta), on one engine whose scratch is reused from call to call;
  * a match every four bytes and 15-bit codes with the match starts on every position of a lane.
No tolerance anywhere."""
import numpy as np
import pytest

import encode_corpus as E
from util import flate

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = ([128, 129, 255, 256, 257] + list(range(503, 522)) + [767, 768, 769, 1023, 1024, 1025,
                65535, 65536, 65537, 2 * 65535 + 300])
KINDS = ["text", "zero", "ramp", "rand"]


class Batch:
    def __init__(self, named):
        self.names = [n for n, _ in named]
        self.streams = [bytes(s) for _, s in named]
        self.off = np.zeros(len(named) + 1, np.uint64)
        np.cumsum(np.array([len(s) for s in self.streams], dtype=np.uint64), out=self.off[1:])
        self.data = np.frombuffer(b"".join(self.streams), np.uint8).copy()
        self._want = {}

    def want(self, oracle, go):
        if go not in self._want:
            self._want[go] = [oracle.deflate(s, compat=oracle.COMPAT_GO if go else 0) for s in self.streams]
        return self._want[go]


def _check(batch, want, out, out_off, what):
    out = np.asarray(out)
    bad = []
    for i, name in enumerate(batch.names):
        got = bytes(out[int(out_off[i]):int(out_off[i + 1])])
        if got != want[i]:
            first = next((j for j in range(min(len(got), len(want[i]))) if got[j] != want[i][j]), None)
            bad.append("%s: len got %d want %d first diff at %s" % (name, len(got), len(want[i]), first))
    assert not bad, "%s: %d of %d streams differ from the oracle: %s" % (what, len(bad), len(batch.names), bad[:10])


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def edges():
    flate.build()
    return Batch([("%s_%d" % (kind, n), flate.synth(kind, 1, n, first_stream=7 * i + k).tobytes())
                  for i, n in enumerate(EDGE_LENGTHS) for k, kind in enumerate(KINDS)])


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
@pytest.mark.parametrize("per_block", [0, 1], ids=["per_stream", "per_block"])
def test_tile_edges(oracle, edges, per_block, go):
    e = flate.FlateEngine(0)
    try:
        e.set_option("entropy_per_block", per_block)
        out, out_off = e.deflate_batch(edges.data, edges.off, compat_go=go)
        _check(edges, edges.want(oracle, go), out, out_off, "per_block=%d go=%d" % (per_block, go))
    finally:
        e.close()


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_tile_edges_misaligned(eng, oracle, edges, go):
    """Input and output one and three bytes past their allocations: no base is dword-aligned."""
    import torch
    want = edges.want(oracle, go)
    buf = torch.zeros(edges.data.size + 8, dtype=torch.uint8, device="cuda")
    buf[1:1 + edges.data.size] = torch.from_numpy(edges.data).cuda()
    obuf = torch.zeros(sum(len(w) for w in want) + 64, dtype=torch.uint8, device="cuda")
    out, out_off = eng.deflate_batch(buf[1:1 + edges.data.size], edges.off, out=obuf[3:], compat_go=go)
    assert out.data_ptr() % 4 == 3 and buf[1:].data_ptr() % 4 == 1
    _check(edges, want, out.cpu().numpy(), out_off, "device")


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_tile_edges_spliced(eng, oracle, edges, go):
    one, nb, bit_off = eng.deflate_spliced(edges.data, edges.off, compat_go=go)
    ref, ref_off = oracle.deflate_spliced(edges.data, edges.off, oracle.COMPAT_GO if go else 0)
    got = bytes(one[:nb])
    first = next((j for j in range(min(len(got), len(ref))) if got[j] != ref[j]), None)
    stream = None if first is None else edges.names[int(np.searchsorted(ref_off, 8 * first, side="right")) - 1]
    assert got == ref, "len got %d want %d first diff at %s in %s" % (len(got), len(ref), first, stream)
    assert (bit_off == ref_off).all()


# 256-position rows per length: 2, 3, 6, 2, 3, 4, 5, 6, 1, 4, 2, 7 -- odd and even counts next to each other
ROW_LENGTHS = [300, 700, 1290, 257, 513, 769, 1025, 1281, 255, 1000, 511, 1793]


@pytest.mark.parametrize("per_block", [0, 1], ids=["per_stream", "per_block"])
def test_neighbouring_blocks_with_odd_row_counts(oracle, per_block):
    """A block with an odd number of rows ends in half a wide tile; the other half is its neighbour's first row.
    Three batches in a row on one engine, each with other bytes and the lengths shifted by one stream: what a call
    leaves in the scratch is wrong for the next, so a meta byte written to or read from a neighbour's row gives
    wrong bytes or trips the packer's self-check."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("entropy_per_block", per_block)
        for seed in range(3):
            lens = [ROW_LENGTHS[(i + seed) % len(ROW_LENGTHS)] for i in range(96)]
            assert any((-(-a // 256)) % 2 != (-(-b // 256)) % 2 for a, b in zip(lens, lens[1:]))
            b = Batch([("text_%d_%d" % (i, n), flate.synth("text", 1, n, first_stream=1000 * (seed + 1) + i).tobytes())
                       for i, n in enumerate(lens)])
            for go in (False, True):
                out, out_off = e.deflate_batch(b.data, b.off, compat_go=go)
                _check(b, b.want(oracle, go), out, out_off, "seed %d per_block=%d go=%d" % (seed, per_block, go))
    finally:
        e.close()


DENSE_AND_LONG = ("dense_words", "fib_literals", "fib_literals_dynamic", "fib_offsets", "fib_code_lengths")


@pytest.fixture(scope="module")
def shifted():
    flate.build()
    pre = flate.synth("text", 1, 8, first_stream=77).tobytes()
    picked = [(name, data) for name, data, _ in E.cases() if name in DENSE_AND_LONG]
    assert len(picked) == len(DENSE_AND_LONG)
    return Batch([("%s+%d" % (name, k), pre[:k] + data) for name, data in picked for k in range(8)])


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
@pytest.mark.parametrize("per_block", [0, 1], ids=["per_stream", "per_block"])
def test_dense_starts_and_long_codes(oracle, shifted, per_block, go):
    """A match every four bytes (128 records in a tile, two starts in every lane) and 15-bit codes (the longest
    bit strings a lane places), behind 0..7 bytes of text: the starts fall on every position of a lane."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("entropy_per_block", per_block)
        out, out_off = e.deflate_batch(shifted.data, shifted.off, compat_go=go)
        _check(shifted, shifted.want(oracle, go), out, out_off, "per_block=%d go=%d" % (per_block, go))
    finally:
        e.close()
