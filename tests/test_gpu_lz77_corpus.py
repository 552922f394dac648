"""The match finder's edge corpus (tests/lz77_corpus.py) through the HIP match finder: all cases in ONE batch -- every
stream then lies at an arbitrary alignment -- tokens (lz77_matches) and bytes (deflate_batch) compared with the oracle
without tolerance, in both compat modes, through every way a stream reaches the parser: the single-lane kernel, one
block per stream, the persistent launch with all streams on the LDS-table blocks and with all on the guests, window
units on and off, the stream writer window by window, and the dictionary builds.  tests/test_lz77_corpus.py says,
without a GPU, which case reaches which edge and which fault each case would expose."""
import zlib

import numpy as np
import pytest

import lz77_corpus as Z
from deflate_dict_ref import deflate_dict
from util import flate, oracle_tokens_per_chunk

pytestmark = pytest.mark.gpu
W = Z.W
MODES = [False, True]


class Batch:
    def __init__(self, cases):
        self.names = [n for n, _ in cases]
        self.streams = [d for _, d in cases]
        self.off = np.zeros(len(cases) + 1, np.uint64)
        np.cumsum(np.array([len(s) for s in self.streams], dtype=np.uint64), out=self.off[1:])
        self.data = np.frombuffer(b"".join(self.streams) + b"\0" * 16, np.uint8).copy()
        self._want, self._tok = {}, {}

    def want(self, oracle, go):
        if go not in self._want:
            self._want[go] = [oracle.deflate(s, compat=oracle.COMPAT_GO if go else 0) for s in self.streams]
        return self._want[go]

    def want_tokens(self, oracle, go):
        if go not in self._tok:
            self._tok[go] = [oracle_tokens_per_chunk(oracle, np.frombuffer(s, np.uint8), compat=1 if go else 0)
                             for s in self.streams]
        return self._tok[go]


@pytest.fixture(scope="module")
def batch():
    return Batch(Z.cases())


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def _check_bytes(batch, want, out, out_off, what, first=0):
    out = np.asarray(out)
    bad = []
    for i, name in enumerate(batch.names):
        got = bytes(out[int(out_off[first + i]):int(out_off[first + i + 1])])
        if got != want[i]:
            at = next((j for j in range(min(len(got), len(want[i]))) if got[j] != want[i][j]), None)
            bad.append("%s: len got %d want %d first diff at %s" % (name, len(got), len(want[i]), at))
    assert not bad, "%s: %d of %d streams differ from the oracle: %s" % (what, len(bad), len(batch.names), bad[:10])


def _check_tokens(eng, oracle, batch, lz_serial, go, what):
    chunks = eng.lz77_matches(batch.data[:int(batch.off[-1])], batch.off, lz_serial=lz_serial, compat_go=go)
    k, bad = 0, []
    for name, s, want in zip(batch.names, batch.streams, batch.want_tokens(oracle, go)):
        sb = np.frombuffer(s, np.uint8)
        for (start, cn), w in zip(flate.lz_chunks(len(s)), want):
            pos, tok = chunks[k]
            got = flate.tokens_from_matches(sb[start:start + cn], pos, tok)
            k += 1
            if got.size != w.size:
                bad.append((name, start, "tokens", got.size, w.size))
            elif (got != w).any():
                j = int(np.nonzero(got != w)[0][0])
                bad.append((name, start, "token %d" % j, hex(int(got[j])), hex(int(w[j]))))
    assert k == len(chunks)
    assert not bad, "%s: %d chunks differ from the oracle's tokens: %s" % (what, len(bad), bad[:10])


@pytest.mark.parametrize("go", MODES, ids=["default", "go"])
def test_tokens_one_block_per_stream(eng, oracle, batch, go):
    _check_tokens(eng, oracle, batch, False, go, "wave kernel")


@pytest.mark.parametrize("go", MODES, ids=["default", "go"])
def test_tokens_single_lane_kernel(eng, oracle, batch, go):
    _check_tokens(eng, oracle, batch, True, go, "FLATE_HIP_LZ_SERIAL")


@pytest.mark.parametrize("go", MODES, ids=["default", "go"])
def test_bytes_one_block_per_stream(eng, oracle, batch, go):
    out, out_off = eng.deflate_batch(batch.data[:int(batch.off[-1])], batch.off, compat_go=go)
    _check_bytes(batch, batch.want(oracle, go), out, out_off, "one block per stream")


def _counts(batch):
    single = sum(1 for s in batch.streams if len(s) <= W)
    return single, len(batch.streams) - single


def _dummies(rng, singles, multis):
    return [("dummy_single_%d" % i, rng.integers(0, 256, 200, dtype=np.uint8).tobytes()) for i in range(singles)] + \
           [("dummy_multi_%d" % i, rng.integers(0, 256, W + 200, dtype=np.uint8).tobytes()) for i in range(multis)]


@pytest.fixture(scope="module")
def padded():
    """The corpus with dummy streams BEHIND it, so that both queues (single-window and multi-window streams; queue
    order is batch order) hold K + 1 entries, K = the larger count of cases: a fixed split of K then gives the
    LDS-table blocks every case of both queues and the guests one dummy of each."""
    cases = Z.cases()
    single = sum(1 for _, d in cases if len(d) <= W)
    multi = len(cases) - single
    K = max(single, multi)
    b = Batch(cases + _dummies(np.random.default_rng(2), K + 1 - single, K + 1 - multi))
    b.K = K
    return b


@pytest.mark.parametrize("units", [0, 1])
def test_persistent_launch_all_on_lds_table_blocks(oracle, padded, units):
    """guest_min_streams = 1 makes the launch persistent, and profile_split_streams = K (see `padded`) hands the
    first K entries of a queue to the LDS-table blocks: every case.  window_units = 0: whole streams, both queues
    split, asserted exactly.  window_units = 1: the single-window queue is split in the same way; the windows of
    the multi-window streams go through the unit queue that both kinds of block share and that no option splits,
    so there the share is only bounded.  Tokens and bytes."""
    K = padded.K
    assert _counts(padded) == (K + 1, K + 1)
    windows = sum(len(flate.lz_chunks(len(s))) for s in padded.streams if len(s) > W)
    e = flate.FlateEngine(0)
    try:
        e.set_option("guest_min_streams", 1)
        e.set_option("resident_blocks", 8)
        e.set_option("guest_blocks", 8)
        e.set_option("window_units", units)
        e.set_option("profile_split_streams", K)
        for go in MODES:
            _check_tokens(e, oracle, padded, False, go, "LDS-table blocks, units %d" % units)
            out, out_off = e.deflate_batch(padded.data[:int(padded.off[-1])], padded.off, compat_go=go)
            _check_bytes(padded, padded.want(oracle, go), out, out_off, "LDS-table blocks, units %d go %d" % (units, go))
            res, queued = e.last_resident_share()
            if units == 0:
                assert (res, queued) == (2 * K, 2 * K + 2), (res, queued, K)
            else:
                assert queued == K + 1 + windows and K <= res <= K + windows, (res, queued, K, windows)
    finally:
        e.close()


def test_persistent_launch_all_on_guests(oracle, batch):
    """A dummy first stream of each kind and profile_split_streams = 1: the LDS-table blocks take queue entry 0 of
    the single-window and of the multi-window queue (queue order is batch order), the guests -- L2 tables, slot
    tags on the single-window streams -- every case.  window_units = 0: the fixed split is for whole streams."""
    dummies = _dummies(np.random.default_rng(1), 1, 1)
    b = Batch(dummies + Z.cases())
    single, multi = _counts(b)
    e = flate.FlateEngine(0)
    try:
        e.set_option("guest_min_streams", 1)
        e.set_option("resident_blocks", 4)
        e.set_option("guest_blocks", 16)
        e.set_option("window_units", 0)
        e.set_option("profile_split_streams", 1)
        for go in MODES:
            _check_tokens(e, oracle, b, False, go, "guests")
            out, out_off = e.deflate_batch(b.data[:int(b.off[-1])], b.off, compat_go=go)
            _check_bytes(b, b.want(oracle, go), out, out_off, "guests go %d" % go)
            res, queued = e.last_resident_share()
            assert (res, queued) == (2, single + multi), (res, queued, single, multi)
    finally:
        e.close()


@pytest.mark.parametrize("go", MODES, ids=["default", "go"])
def test_stream_writer_window_by_window(oracle, batch, go):
    """open_stream with stream_rebase_bytes = 65535: the origin of the positions moves at every window."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("stream_rebase_bytes", 65535)
        want = batch.want(oracle, go)
        picked = [i for i, s in enumerate(batch.streams) if len(s) > W]
        assert len(picked) >= 100
        for i in picked:
            sb = np.frombuffer(batch.streams[i], np.uint8)
            w = e.open_stream(compat_go=go)
            try:
                full = sb.size // W
                parts = [w.write(sb[k * W:(k + 1) * W]) for k in range(full)]
                parts.append(w.close(sb[full * W:]))
            finally:
                w.free()
            got = np.concatenate(parts).tobytes()
            assert got == want[i], "%s: len got %d want %d" % (batch.names[i], len(got), len(want[i]))
    finally:
        e.close()


class Twins:
    """The dictionary twin of every multi-window case: dictionary = the bytes up to a cut, payload = the rest; the
    cut is the start of the case's last window (30000 earlier where that window is short), at most 32768 in front of
    a second plant that lies there, so the plants of the windows before reach the payload through the dictionary's
    table.  Expected bytes: tests/deflate_dict_ref.py, computed once."""

    def __init__(self, batch):
        self.items = []
        for name, s in zip(batch.names, batch.streams):
            if len(s) > W:
                cut = (len(s) // W) * W
                if len(s) - cut < 600:
                    cut -= 30000
                self.items.append((name, s[max(0, cut - 32768):cut], s[cut:]))
        self.dicts = [d for _, d, _ in self.items]
        payloads = [p for _, _, p in self.items]
        self.off = np.zeros(len(payloads) + 1, np.uint64)
        np.cumsum(np.array([len(p) for p in payloads], dtype=np.uint64), out=self.off[1:])
        self.data = np.frombuffer(b"".join(payloads) + b"\0" * 16, np.uint8).copy()
        self.want = {go: [deflate_dict(p, d, 1 if go else 0) for _, d, p in self.items] for go in MODES}

    def check(self, e, what):
        for go in MODES:
            out, out_off = e.deflate_batch(self.data, self.off, compat_go=go, zdicts=self.dicts,
                                           dict_of=list(range(len(self.dicts))))
            bad = [name for i, (name, _, _) in enumerate(self.items)
                   if bytes(out[int(out_off[i]):int(out_off[i + 1])]) != self.want[go][i]]
            assert not bad, (what, go, len(bad), bad[:10])


@pytest.fixture(scope="module")
def twins(batch):
    return Twins(batch)


def _needs_dictionary(stream, zdict, payload):
    """True if the raw stream holds a match whose source lies in the dictionary: zlib inflates it to the payload
    with the dictionary and refuses it (distance too far back) without."""
    d = zlib.decompressobj(-15, zdict=zdict)
    assert d.decompress(stream) + d.flush() == payload
    try:
        zlib.decompressobj(-15).decompress(stream)
    except zlib.error:
        return True
    return False


def test_dictionary_twins_reach_into_the_dictionary(twins):
    """The twins test the cut only if matches cross it.  Every ladder case with d = 32767 or 32768 whose second
    plant lies in window 1 or 2 has its first plant inside the dictionary and in range (both modes: the default
    mode cuts such a match to 4 bytes, it does not drop it); so have the candidates at W-16 and W-17, the last
    positions of the dictionary that its table can name.  Counted from the expected streams themselves."""
    for go in MODES:
        need = {name for (name, d, p), w in zip(twins.items, twins.want[go]) if _needs_dictionary(w, d, p)}
        far = [n for n, _, _ in twins.items if n.startswith(("ladder_d32767_", "ladder_d32768_")) and not n.endswith("_w0")]
        far += ["edge_cand_W-16", "edge_cand_W-17"]
        assert len(far) >= 14 and set(far) <= need, (go, sorted(set(far) - need))
        print("\ntwins with a match into the dictionary (go %d): %d of %d" % (go, len(need), len(twins.items)))


def test_dictionary_twins_one_block_per_stream(twins):
    assert len(twins.items) >= 100
    e = flate.FlateEngine(0)
    try:
        twins.check(e, "one block per stream")
    finally:
        e.close()


@pytest.mark.parametrize("geometry", [(4, 8), (1, 64)], ids=["4+8", "1+64"])
def test_dictionary_twins_persistent(twins, geometry):
    """The two geometries of test_large_batch_takes_lds_table_and_guest_blocks."""
    e = flate.FlateEngine(0)
    try:
        e.set_option("guest_min_streams", 1)
        e.set_option("resident_blocks", geometry[0])
        e.set_option("guest_blocks", geometry[1])
        twins.check(e, "persistent %d+%d" % geometry)
    finally:
        e.close()
