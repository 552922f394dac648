"""The one-workgroup scans of the index and layout kernels (csrc/block_scan.h) at the element counts where a
wavefront, a chunk of 1024 or the carry between two chunks can go wrong -- through the calls that run them:
    scan_sizes_kernel          deflate_batch on device pointers
    frame_scan_kernel          deflate_batch_framed (zlib, gzip) and bgzf_write
    chain_scan_kernel           bgzf_index / bgzf_read of files of more than 1024 and 2048 tiles of 4 KiB
    bgzf_range_layout_kernel   bgzf_read_ranges with more than 1024 and 2048 ranges
Every expectation is exact and comes from the CPU (the oracle, tests/bgzf_ref.py, tests/bgzf_range_ref.py), computed
once for the largest count; the smaller counts use its prefixes."""
import numpy as np
import pytest

import bgzf_range_ref as model
import bgzf_ref as ref
from util import flate, make_streams

pytestmark = pytest.mark.gpu

E_OUT_TOO_SMALL = -2
COUNTS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049]
N = max(COUNTS)
KINDS = ["ramp", "zero", "rand", "text", "low", "period", "runs"]  # (util.make_streams)
WRAPS = ["zlib", "gzip"]
BLOCK = 16  # bgzf_write: bytes per member
TILE = 4096  # bgzf_count_kernel: bytes per workgroup, one element of chain_scan_kernel each
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def offsets(parts):
    off = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum(np.array([len(p) for p in parts], dtype=np.uint64), out=off[1:])
    return off


class Streams:
    """2049 payloads of (7 * i) % 41 bytes (empty ones among every 41), their raw streams and their members."""

    def __init__(self, oracle):
        data, self.off = make_streams([(KINDS[i % len(KINDS)], (7 * i) % 41) for i in range(N)], seed=77)
        payloads = [data[int(self.off[i]):int(self.off[i + 1])].tobytes() for i in range(N)]
        assert sum(1 for p in payloads if not p) == -(-N // 41)
        self.d_data = to_dev(np.concatenate([data, np.zeros(16, np.uint8)]))
        raw = [oracle.deflate(p) for p in payloads]
        kind = {"zlib": oracle.FRAME_ZLIB, "gzip": oracle.FRAME_GZIP}
        members = {w: [oracle.frame(kind[w], r, p) for r, p in zip(raw, payloads)] for w in WRAPS}
        self.bytes = {"raw": b"".join(raw), **{w: b"".join(m) for w, m in members.items()}}
        self.out_off = {"raw": offsets(raw), **{w: offsets(m) for w, m in members.items()}}

    def want(self, form, n):
        off = self.out_off[form][:n + 1]
        return self.bytes[form][:int(off[-1])], off


@pytest.fixture(scope="module")
def streams(oracle):
    return Streams(oracle)


def room(total):
    """A device buffer of exactly `total` bytes with guard bytes behind it."""
    import torch
    buf = torch.full((total + 64,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[:total]


def delivered(buf, total):
    b = buf.cpu().numpy()
    assert (b[total:] == GUARD).all(), "bytes behind the capacity were written"
    return b[:total].tobytes()


# ---- 1. scan_sizes_kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_raw_stream_offsets(eng, streams, n):
    want, want_off = streams.want("raw", n)
    buf, out = room(len(want))
    _, off = eng.deflate_batch(streams.d_data, streams.off[:n + 1], out=out)
    assert np.array_equal(off, want_off), n
    assert delivered(buf, len(want)) == want, n
    buf, out = room(len(want) - 1)
    with pytest.raises(flate.FlateError) as ei:
        eng.deflate_batch(streams.d_data, streams.off[:n + 1], out=out)
    assert ei.value.code == E_OUT_TOO_SMALL


# ---- 2. frame_scan_kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("wrap", WRAPS)
def test_member_offsets(eng, streams, wrap, n):
    want, want_off = streams.want(wrap, n)
    out, off = eng.deflate_batch_framed(streams.d_data, streams.off[:n + 1], wrap, out_cap=len(want))
    assert np.array_equal(off, want_off), (wrap, n)
    assert out[:len(want)].cpu().numpy().tobytes() == want, (wrap, n)
    with pytest.raises(flate.FlateError) as ei:
        eng.deflate_batch_framed(streams.d_data, streams.off[:n + 1], wrap, out_cap=len(want) - 1)
    assert ei.value.code == E_OUT_TOO_SMALL


@pytest.fixture(scope="module")
def blocks(oracle):
    """16 * 2049 bytes, the file bgzf_write makes of them with 16 bytes per member, and its member offsets."""
    data = ref.text(BLOCK * N, seed=11)
    f, off = ref.build_file(oracle, data, BLOCK)
    assert len(off) == N + 1 and f[int(off[-1]):] == ref.EOF
    return to_dev(np.frombuffer(data, np.uint8)), f, off


@pytest.mark.parametrize("n", COUNTS)
def test_bgzf_member_offsets(eng, blocks, n):
    d_data, f, off = blocks
    want = f[:int(off[n])] + ref.EOF  # (a member depends on its own block only: ref.build_file of the first n blocks)
    out, out_len, member_off = eng.bgzf_write(d_data[:BLOCK * n], block_bytes=BLOCK, out_cap=len(want), index=True)
    assert out_len == len(want) and np.array_equal(member_off, off[:n + 1]), n
    assert out[:out_len].cpu().numpy().tobytes() == want, n
    with pytest.raises(flate.FlateError) as ei:
        eng.bgzf_write(d_data[:BLOCK * n], block_bytes=BLOCK, out_cap=len(want) - 1)
    assert ei.value.code == E_OUT_TOO_SMALL


# ---- 3. chain_scan_kernel -------------------------------------------------------------------------------------------
TILE_COUNTS = [1023, 1024, 1025, 2048, 2049]


@pytest.fixture(scope="module")
def full_members():
    """Stored members of 65536 bytes (16 tiles each), enough for the largest file.  The payloads are random bytes with
    0 .. 39 decoy headers each at random places (4 MiB of random bytes alone hold a magic by chance once in four
    files): the tiles' candidate counts differ, and most candidates are not members of the chain."""
    rng = np.random.default_rng(31)
    payloads = []
    for _ in range(max(TILE_COUNTS) // 16 + 1):
        p = bytearray(rng.integers(0, 256, ref.FULL_PAYLOAD, dtype=np.uint8).tobytes())
        for j in range(int(rng.integers(0, 40))):
            at = int(rng.integers(0, len(p) - 18))
            p[at:at + 18] = ref.decoy_header(26 + j)
        payloads.append(bytes(p))
    return payloads, [ref.stored_member(p) for p in payloads]


@pytest.mark.parametrize("tiles", TILE_COUNTS)
def test_files_of_more_tiles_than_one_chunk(eng, full_members, tiles):
    payloads, members = full_members
    size = tiles * TILE - (TILE - 1 if tiles % 2 else 0)  # the last tile full, or one byte of it
    k, rest = divmod(size - len(ref.EOF), ref.MEMBER_MAX)
    assert rest >= 31
    last = payloads[k][:rest - 31]
    f = b"".join(members[:k]) + ref.stored_member(last) + ref.EOF
    plain = b"".join(payloads[:k]) + last
    d_f = to_dev(np.frombuffer(f, np.uint8))
    assert len(f) == size and d_f.data_ptr() % 16 == 0 and -(-size // TILE) == tiles
    w = ref.Walk(f)
    assert (w.rc, w.n_members, w.out_bytes) == (0, k + 2, len(plain))
    assert f.count(ref.HEAD16[:4]) > 4 * w.n_members  # (the decoys)
    ix = eng.bgzf_index(d_f)
    assert (ix.rc, ix.n_members, ix.out_bytes, ix.eof_marker, ix.err_off) == (0, w.n_members, w.out_bytes, 1, -1)
    assert ix.member_off.tolist() == w.member_off and ix.out_off.tolist() == w.out_off
    out, r = eng.bgzf_read(d_f)
    assert (r.rc, r.out_len, r.n_members, r.bad_member, r.err_off, r.eof_marker) == (0, len(plain), w.n_members, 0xffffffff, -1, 1)
    assert out[:r.out_len].cpu().numpy().tobytes() == plain


# ---- 4. bgzf_range_layout_kernel -----------------------------------------------------------------------------------
RANGE_COUNTS = [1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def range_case():
    """ref.many_members(65) and 2049 ranges in bytes and in virtual offsets: every third empty, and -- virtual offsets
    only, bytes have no invalid positions -- every 100th invalid."""
    f, plain = ref.many_members(65)
    w = ref.Walk(f)
    rng = np.random.default_rng(41)
    T = w.out_bytes
    filled = [k for k in range(w.n_members) if w.out_off[k + 1] > w.out_off[k]]

    def vpoint():
        k = int(rng.choice(filled))
        return w.member_off[k] << 16 | int(rng.integers(0, w.out_off[k + 1] - w.out_off[k] + 1))
    by_bytes, by_virtual = [], []
    for r in range(max(RANGE_COUNTS)):
        b = int(rng.integers(0, T + 1))
        e = b if r % 3 == 0 else min(T + 5, b + int(rng.integers(1, 400)))
        by_bytes.append((b, e))
        vb, ve = sorted((vpoint(), vpoint()))
        if r % 3 == 0:
            ve = vb
        if r % 100 == 50:
            ve = (ve | 0xffff) if r % 200 == 50 else ((ve >> 16) + 1) << 16  # past ISIZE; inside a member
        by_virtual.append((vb, ve))
    return to_dev(np.frombuffer(f, np.uint8)), f, {False: by_bytes, True: by_virtual}


@pytest.mark.parametrize("n", RANGE_COUNTS)
@pytest.mark.parametrize("virtual", [False, True], ids=["bytes", "virtual"])
def test_more_ranges_than_one_chunk(eng, range_case, virtual, n):
    d_f, f, ranges = range_case
    begin, end = [b for b, _ in ranges[virtual][:n]], [e for _, e in ranges[virtual][:n]]
    R = model.read_ranges(f, model.POS_VIRTUAL if virtual else model.POS_BYTES, begin, end)
    assert R.rc == (model.INVALID if virtual else model.OK) and (model.INVALID in R.range_status) == virtual
    assert sum(1 for r in range(n) if R.out_off[r] == R.out_off[r + 1]) >= n // 3
    out, r = eng.bgzf_read_ranges(d_f, begin, end, virtual=virtual)
    assert (r.rc, r.n_members, r.n_decoded, r.bad_member, r.err_off) == (R.rc, R.n_members, R.n_decoded, R.bad_member, R.err_off)
    assert [int(x) for x in r.out_off] == R.out_off
    assert [int(x) for x in r.range_status] == R.range_status
    assert all(R.exact[i] or R.out_off[i] == R.out_off[i + 1] for i in range(n))  # (an invalid range has no bytes)
    assert out[:R.out_off[-1]].cpu().numpy().tobytes() == R.data
