"""The encoder's edge corpus (tests/encode_corpus.py) through the HIP encoder: all cases in ONE batch -- every stream
then lies at an arbitrary input and output alignment -- and every stream byte for byte what the oracle writes.  The
corpus drives the entropy stage (huff_hist / huff_code / huff_pack and their one-wavefront-per-block forms) into the
15-bit and 7-bit code limits, the enc_speed switch and the Go-mode stored decision at their edges, every run form of
the code-length coding, mixed block sequences with stored blocks at every bit phase, and windows with a match every
four bytes.  No tolerance anywhere; tests/test_encode_corpus.py says, without a GPU, which case reaches which branch."""
import numpy as np
import pytest

import encode_corpus as E
from util import INFLATE_CONFIGS, flate, force_inflate_config, oracle_tokens_per_chunk, raw_inflate

pytestmark = pytest.mark.gpu
W = E.W


class Batch:
    def __init__(self, cases):
        self.names = [name for name, _, _ in cases]
        self.streams = [data for _, data, _ in cases]
        self.off = np.zeros(len(cases) + 1, np.uint64)
        np.cumsum(np.array([len(s) for s in self.streams], dtype=np.uint64), out=self.off[1:])
        self.data = np.frombuffer(b"".join(self.streams), np.uint8).copy()
        self.sizes = [len(s) for s in self.streams]
        self._want = {}

    def want(self, oracle, go):
        """The oracle's stream of every case -- of EVERY case in both compat modes, not only in those a case is
        meant for."""
        if go not in self._want:
            self._want[go] = [oracle.deflate(s, compat=oracle.COMPAT_GO if go else 0) for s in self.streams]
        return self._want[go]

    def sub(self, keep):
        return Batch([(n, s, ()) for n, s in zip(self.names, self.streams) if keep(n, s)])


@pytest.fixture(scope="module")
def batch():
    return Batch(E.cases())


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def _check(batch, want, out, out_off, what):
    """As test_gpu_parity._check_streams: case name, lengths and the first differing byte of every stream that is
    not the oracle's."""
    out = np.asarray(out)
    bad = []
    for i, name in enumerate(batch.names):
        got = bytes(out[int(out_off[i]):int(out_off[i + 1])])
        if got != want[i]:
            first = next((j for j in range(min(len(got), len(want[i]))) if got[j] != want[i][j]), None)
            bad.append("%s: len got %d want %d first diff at %s" % (name, len(got), len(want[i]), first))
    assert not bad, "%s: %d of %d streams differ from the oracle: %s" % (what, len(bad), len(batch.names), bad[:10])


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_batch_host_pointers(eng, oracle, batch, go):
    out, out_off = eng.deflate_batch(batch.data, batch.off, compat_go=go)
    _check(batch, batch.want(oracle, go), out, out_off, "host")
    for i in range(0, len(batch.names), 7):   # (the oracle's streams inflate with zlib: checked without a GPU)
        assert raw_inflate(bytes(out[int(out_off[i]):int(out_off[i + 1])])) == batch.streams[i]


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_batch_device_pointers_misaligned(eng, oracle, batch, go):
    """Input and output one and three bytes past their allocations: no base is dword-aligned."""
    import torch
    buf = torch.zeros(batch.data.size + 8, dtype=torch.uint8, device="cuda")
    buf[1:1 + batch.data.size] = torch.from_numpy(batch.data).cuda()
    host, host_off = eng.deflate_batch(batch.data, batch.off, compat_go=go)
    obuf = torch.zeros(int(host_off[-1]) + 64, dtype=torch.uint8, device="cuda")
    out, out_off = eng.deflate_batch(buf[1:1 + batch.data.size], batch.off, out=obuf[3:], compat_go=go)
    assert out.data_ptr() % 4 == 3 and buf[1:].data_ptr() % 4 == 1
    _check(batch, batch.want(oracle, go), out.cpu().numpy(), out_off, "device")


@pytest.mark.parametrize("per_block", [0, 1])
def test_entropy_per_stream_and_per_block(oracle, batch, per_block):
    """The per-stream and the one-wavefront-per-block histogram and pack kernels give the same bytes."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("entropy_per_block", per_block)
        for go in (False, True):
            out, out_off = e.deflate_batch(batch.data, batch.off, compat_go=go)
            _check(batch, batch.want(oracle, go), out, out_off, "entropy_per_block=%d go=%d" % (per_block, go))
    finally:
        e.close()


def test_launch_geometries(oracle, batch):
    """The geometries of test_guest_blocks_give_identical_streams (LDS-table and guest blocks share one queue), and
    multi-window streams kept on their block (window_units = 0)."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("guest_min_streams", 1)
        for resident, guest, units in ((4, 8, 1), (1, 64, 1), (4, 8, 0)):
            e.set_option("resident_blocks", resident)
            e.set_option("guest_blocks", guest)
            e.set_option("window_units", units)
            for go in (False, True):
                out, out_off = e.deflate_batch(batch.data, batch.off, compat_go=go)
                _check(batch, batch.want(oracle, go), out, out_off, "blocks %d/%d units %d go=%d" %
                       (resident, guest, units, go))
    finally:
        e.close()


def _check_tokens(eng, oracle, b, lz_serial, go):
    chunks = eng.lz77_matches(b.data, b.off, lz_serial=lz_serial, compat_go=go)
    k, bad = 0, []
    for name, s in zip(b.names, b.streams):
        sb = np.frombuffer(s, np.uint8)
        for (start, cn), w in zip(flate.lz_chunks(len(s)), oracle_tokens_per_chunk(oracle, sb, compat=1 if go else 0)):
            pos, tok = chunks[k]
            got = flate.tokens_from_matches(sb[start:start + cn], pos, tok)
            k += 1
            if got.size != w.size:
                bad.append((name, start, "tokens", got.size, w.size))
            elif (got != w).any():
                j = int(np.nonzero(got != w)[0][0])
                bad.append((name, start, "token %d" % j, hex(int(got[j])), hex(int(w[j]))))
    assert k == len(chunks)
    assert not bad, "%d chunks differ from the oracle's tokens: %s" % (len(bad), bad[:10])


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_tokens_wave_kernel(eng, oracle, batch, go):
    _check_tokens(eng, oracle, batch, False, go)


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_tokens_serial_kernel_single_window(eng, oracle, batch, go):
    _check_tokens(eng, oracle, batch.sub(lambda n, s: len(s) <= W), True, go)


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_spliced(eng, oracle, batch, go):
    """One DEFLATE stream of all cases: every block -- the stored ones between Huffman and dynamic blocks of the
    mixed streams too -- starts where the block before it ended, whatever stream that belonged to."""
    one, nb, bit_off = eng.deflate_spliced(batch.data, batch.off, compat_go=go)
    ref, ref_off = oracle.deflate_spliced(batch.data, batch.off, oracle.COMPAT_GO if go else 0)
    got = bytes(one[:nb])
    first = next((j for j in range(min(len(got), len(ref))) if got[j] != ref[j]), None)
    stream = None if first is None else batch.names[int(np.searchsorted(ref_off, 8 * first, side="right")) - 1]
    assert got == ref, "len got %d want %d first diff at %s in %s" % (len(got), len(ref), first, stream)
    assert (bit_off == ref_off).all(), [batch.names[i] for i in np.nonzero(bit_off[:-1] != ref_off[:-1])[0][:5]]


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_stream_writer_in_windows(eng, oracle, batch, go):
    """The multi-window cases written window by window: the pieces are the one-shot stream."""
    multi = batch.sub(lambda n, s: len(s) > W)
    assert len(multi.names) >= 10
    want = multi.want(oracle, go)
    for name, s, ref in zip(multi.names, multi.streams, want):
        sb = np.frombuffer(s, np.uint8)
        w = eng.open_stream(compat_go=go)
        try:
            full = len(s) // W
            parts = [w.write(sb[k * W:(k + 1) * W]) for k in range(full)]
            parts.append(w.close(sb[full * W:]))
        finally:
            w.free()
        got = np.concatenate(parts).tobytes()
        first = next((j for j in range(min(len(got), len(ref))) if got[j] != ref[j]), None)
        assert got == ref, "%s: len got %d want %d first diff at %s" % (name, len(got), len(ref), first)


@pytest.mark.parametrize("config", INFLATE_CONFIGS)
def test_round_trip_through_every_decoder(eng, batch, config):
    """The GPU's own streams back through every decoder configuration: blocks with 15-bit literal and offset codes
    and with a four-byte match every four bytes are decoder inputs the inflate corpus does not have."""
    d = force_inflate_config(flate.FlateEngine(0), config)
    try:
        for go in (False, True):
            comp, coff = eng.deflate_batch(batch.data, batch.off, compat_go=go)
            back, boff, olen, status, _ = d.inflate_batch(comp, coff, batch.sizes)
            bad = [(batch.names[i], int(status[i]), int(olen[i]), batch.sizes[i]) for i in range(len(batch.names))
                   if int(status[i]) != 0 or int(olen[i]) != batch.sizes[i] or
                   bytes(back[int(boff[i]):int(boff[i]) + int(olen[i])]) != batch.streams[i]]
            assert not bad, (config, go, bad[:10])
    finally:
        d.close()
