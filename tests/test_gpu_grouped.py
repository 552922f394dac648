"""GPU tests of flate_hip_deflate_fast_grouped_framed: several spliced members in one call.  Every output -- bytes,
out_off and the bit index -- is compared BYTE FOR BYTE with tests/grouped_ref.py (header, the oracle's spliced stream over
the group's pieces, trailer from zlib's checksums), read back by zlib / gzip on the CPU and by
flate_hip_inflate_spliced_framed from every member's index slice.  The expectations are computed once per module."""
import ctypes as C
import gzip
import importlib
import zlib

import numpy as np
import pytest

import grouped_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

engine = importlib.import_module("moonbit-flate_amd.engine")
E_INVALID, E_OUT_TOO_SMALL = -1, -2
WRAPS = ["raw", "zlib", "gzip"]
MODES = [False, True]  # compat_go
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    return ref.corpus()


@pytest.fixture(scope="module")
def expects(oracle, corpus):
    """{(layout, compat_go): Expect}: computed once, shared, never changed."""
    data, off = corpus
    return {(name, go): ref.Expect(data, off, lay, go) for name, lay in ref.layouts(off.size - 1).items() for go in MODES}


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(data):
    """(the input with some room behind it: an empty batch still has an address)"""
    return np.concatenate([data, np.zeros(16, dtype=np.uint8)])


def cpu_read(wrap, member):
    if wrap == "raw":
        return zlib.decompress(member, -15)
    return zlib.decompress(member) if wrap == "zlib" else gzip.decompress(member)


def guarded(total, shift):
    """A device buffer of 0xA5 and the `total` bytes of it that start `shift` bytes behind an aligned address."""
    import torch
    buf = torch.full((GUARD + 4 + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, buf[GUARD + shift:GUARD + shift + total]


def run_checked(eng, e, wrap, device, what):
    """One call; bytes, out_off and the index against the reference."""
    want, want_off = e.want(wrap)
    data = padded(e.data)
    out, out_off, bit_off = eng.deflate_grouped_framed(to_dev(data) if device else data, e.in_off, e.group_off, wrap,
                                                       compat_go=e.compat_go, index=True)
    got = (out.cpu().numpy() if device else out)[:int(out_off[-1])].tobytes()
    assert np.array_equal(out_off, want_off), what
    assert np.array_equal(bit_off, e.bit_off), what
    assert got == want, what
    return got, out_off, bit_off


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("go", MODES)
@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("name", ["ones", "one", "mixed"])
def test_bytes_offsets_and_index_equal_the_reference(eng, expects, name, wrap, go, device):
    run_checked(eng, expects[(name, go)], wrap, device, (name, wrap, go, device))


@pytest.mark.parametrize("go", MODES)
def test_one_group_of_everything_is_deflate_spliced(eng, expects, go):
    e = expects[("one", go)]
    got, _, bit_off = run_checked(eng, e, "raw", True, go)
    one, nbytes, bits = eng.deflate_spliced(to_dev(padded(e.data)), e.in_off, compat_go=go)
    assert one.cpu().numpy()[:nbytes].tobytes() == got and np.array_equal(bits, bit_off)


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
@pytest.mark.parametrize("go", MODES)
def test_groups_of_one_piece_equal_deflate_batch_framed(eng, expects, wrap, go):
    e = expects[("ones", go)]
    got, out_off, _ = run_checked(eng, e, wrap, True, (wrap, go))
    out, off = eng.deflate_batch_framed(to_dev(padded(e.data)), e.in_off, wrap, compat_go=go)
    assert np.array_equal(off, out_off)
    assert out.cpu().numpy()[:int(off[-1])].tobytes() == got


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("wrap", WRAPS)
def test_out_at_every_byte_misalignment_and_nothing_around_it(eng, expects, wrap, shift):
    e = expects[("mixed", False)]
    want, want_off = e.want(wrap)
    total = len(want) + (3 if wrap == "raw" else 0)  # raw: the pack kernel stores whole dwords
    buf, out = guarded(total, shift)
    _, out_off = eng.deflate_grouped_framed(to_dev(padded(e.data)), e.in_off, e.group_off, wrap, out=out, out_cap=total)
    b = buf.cpu().numpy()
    assert np.array_equal(out_off, want_off)
    assert (b[:GUARD + shift] == 0xA5).all(), "bytes in front of out were written"
    assert (b[GUARD + shift + total:] == 0xA5).all(), "bytes behind the room were written"
    assert b[GUARD + shift:GUARD + shift + len(want)].tobytes() == want
    if wrap != "raw":
        assert (b[GUARD + shift + len(want):] == 0xA5).all(), "bytes behind the total were written"


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_exact_room_is_enough_and_one_byte_less_is_refused_on_the_device(eng, expects, wrap):
    e = expects[("mixed", False)]
    want, want_off = e.want(wrap)
    buf, out = guarded(len(want), 1)
    with pytest.raises(flate.FlateError) as ei:
        eng.deflate_grouped_framed(to_dev(padded(e.data)), e.in_off, e.group_off, wrap, out=out, out_cap=len(want) - 1)
    assert ei.value.code == E_OUT_TOO_SMALL
    assert (buf.cpu().numpy() == 0xA5).all(), "a refused call wrote"
    _, out_off = eng.deflate_grouped_framed(to_dev(padded(e.data)), e.in_off, e.group_off, wrap, out=out, out_cap=len(want))
    assert np.array_equal(out_off, want_off) and out.cpu().numpy().tobytes() == want


def test_raw_needs_three_bytes_behind_the_total(eng, expects):
    e = expects[("mixed", False)]
    want, want_off = e.want("raw")
    buf, out = guarded(len(want) + 3, 0)
    with pytest.raises(flate.FlateError) as ei:
        eng.deflate_grouped_framed(to_dev(padded(e.data)), e.in_off, e.group_off, "raw", out=out, out_cap=len(want) + 2)
    assert ei.value.code == E_OUT_TOO_SMALL
    assert (buf.cpu().numpy() == 0xA5).all(), "a refused call wrote"
    _, out_off = eng.deflate_grouped_framed(to_dev(padded(e.data)), e.in_off, e.group_off, "raw", out=out,
                                            out_cap=len(want) + 3)
    assert np.array_equal(out_off, want_off) and out.cpu().numpy()[:len(want)].tobytes() == want


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
@pytest.mark.parametrize("name", ["mixed", "ones"])
def test_members_read_back_on_the_cpu_and_through_their_index_slices(eng, expects, name, wrap):
    e = expects[(name, True)]
    got, out_off, bit_off = run_checked(eng, e, wrap, False, (name, wrap))
    arr = np.frombuffer(got, dtype=np.uint8)
    sizes = (e.in_off[1:] - e.in_off[:-1]).astype(np.uint64)
    for g in range(e.n_groups):
        member = arr[int(out_off[g]):int(out_off[g + 1])]
        assert cpu_read(wrap, member.tobytes()) == e.inputs[g], g
        if name == "ones" and g % 9:  # (every ninth single: the whole set is covered by the mixed layout's shapes)
            continue
        lo, hi = int(e.group_off[g]), int(e.group_off[g + 1])
        back, slot, olen, status, _, ms = eng.inflate_spliced_framed(
            np.concatenate([member, np.zeros(8, np.uint8)]), member.size, wrap, ref.member_index(bit_off, e.group_off, g),
            sizes[lo:hi])
        assert ms == 0 and (status == 0).all() and np.array_equal(olen, sizes[lo:hi]), g
        assert back[:int(slot[-1])].tobytes() == e.inputs[g], g


@pytest.mark.parametrize("wrap", WRAPS)
def test_empty_pieces_and_empty_groups(eng, oracle, wrap):
    data, off, lay = ref.empties()
    e = ref.Expect(data, off, lay)
    for device in (False, True):
        got, out_off, _ = run_checked(eng, e, wrap, device, (wrap, device))
    for g in range(e.n_groups):
        assert cpu_read(wrap, got[int(out_off[g]):int(out_off[g + 1])]) == e.inputs[g]


@pytest.mark.parametrize("n", [1025, 2049])
def test_more_pieces_than_the_scan_has_threads(eng, oracle, n):
    data, off, lay = ref.many(n)
    e = ref.Expect(data, off, lay, True)
    for wrap in ("raw", "gzip"):
        run_checked(eng, e, wrap, True, (n, wrap))


def test_refused_arguments(eng, expects):
    e = expects[("mixed", False)]
    data = padded(e.data)
    n = e.n_pieces
    for bad in ([0, 5, 5, n], [0, 7, 5, n], [1, 5, n], [0, 5, n - 1], [0, 5, n + 1]):
        with pytest.raises(flate.FlateError) as ei:
            eng.deflate_grouped_framed(data, e.in_off, np.array(bad, np.uint32), "zlib")
        assert ei.value.code == E_INVALID, bad
    L = importlib.import_module("moonbit-flate_amd._lib").load()
    out = np.full(1 << 20, 0xA5, np.uint8)
    out_off = np.zeros(e.n_groups + 1, np.uint64)
    rc = L.flate_hip_deflate_fast_grouped_framed(eng._ctx, data.ctypes.data, e.in_off.ctypes.data, n,
                                                 e.group_off.ctypes.data, e.n_groups, 3, out.ctypes.data, out.size,
                                                 out_off.ctypes.data, None, 0)
    assert rc == E_INVALID and (out == 0xA5).all()
    # no groups: nothing but out_off[0]
    out_off[:] = 7
    rc = L.flate_hip_deflate_fast_grouped_framed(eng._ctx, data.ctypes.data, np.zeros(1, np.uint64).ctypes.data, 0,
                                                 np.zeros(1, np.uint32).ctypes.data, 0, 1, out.ctypes.data, out.size,
                                                 out_off.ctypes.data, None, 0)
    assert rc == 0 and out_off[0] == 0 and (out == 0xA5).all()


def test_a_ctx_that_made_a_grouped_call_makes_the_other_calls_with_unchanged_bytes(expects, corpus):
    data, off = corpus
    data = padded(data)
    names = ["e%d" % i for i in range(off.size - 1)]

    def others(e):
        b, boff = e.deflate_batch(data, off)
        s, slen, sbits = e.deflate_spliced(data, off)
        z = e.zip_write(data, off, names)
        return b[:int(boff[-1])].tobytes(), boff.tolist(), s[:slen].tobytes(), sbits.tolist(), z

    fresh = flate.FlateEngine(0)
    want = others(fresh)
    fresh.close()
    used = flate.FlateEngine(0)
    ex = expects[("mixed", False)]
    for wrap in WRAPS:
        run_checked(used, ex, wrap, False, wrap)
    got = others(used)
    run_checked(used, ex, "gzip", True, "again")
    used.close()
    assert got == want
