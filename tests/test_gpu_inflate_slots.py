"""The write footprint of every batch decoder configuration (tests/slot_corpus.py): with device pointers, a stream
writes only inside its own output slot, and one that produces nothing writes nothing.  The output buffer is prefilled
with 0xA5, every real stream lies between two guard streams, and after each call the WHOLE buffer is compared with
the image the oracle's results give -- every byte but the real streams' tails beyond out_len -- so a store across a
slot border shows whichever lane stores last.  Run at a 16-byte-aligned output and 3 bytes behind one."""
import ctypes as C

import numpy as np
import pytest

import slot_corpus as S
from util import INFLATE_CONFIGS, flate, force_inflate_config

pytestmark = pytest.mark.gpu

SHIFTS = (0, 3)
DEVICE_PTRS, WRAP_ZLIB = 1, 1


@pytest.fixture(scope="module", params=INFLATE_CONFIGS)
def eng(request):
    e = force_inflate_config(flate.FlateEngine(0), request.param)
    yield e
    e.close()


def _prefilled(batch, shift):
    """(the whole device buffer: `shift` bytes, then the batch's image before the call; its part that is `out`)."""
    import torch
    whole = torch.full((shift + batch.image.size,), S.FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole, whole[shift + S.OUTER:]


def _assert_footprint(batch, whole, shift, out_len, status, err_off, what):
    import torch
    torch.cuda.synchronize()
    back = whole.cpu().numpy()
    assert (back[:shift] == S.FILL).all(), what
    bad = batch.check(back[shift:], out_len, status, err_off)
    assert not bad, "%s, out %d bytes behind a 16-byte boundary: %s" % (what, shift, S.report(bad))


def _run_batch(eng, batch, what):
    import torch
    data, in_off = batch.in_blob()
    d_in = torch.from_numpy(data).cuda()
    for shift in SHIFTS:
        whole, out = _prefilled(batch, shift)
        res = eng.inflate_batch(d_in, in_off, batch.caps, out=out, check=False, zdicts=batch.zdict,
                                dict_of=batch.dict_of)
        assert res[0] is out and np.array_equal(res[1], batch.out_off)
        _assert_footprint(batch, whole, shift, res[2], res[3], res[4], what)


def test_plain_batch(eng, oracle):
    _run_batch(eng, S.plain(oracle, "A"), "flate_hip_inflate_batch, every slot large enough")


def test_plain_batch_with_slots_too_small(eng, oracle):
    _run_batch(eng, S.plain(oracle, "B"), "flate_hip_inflate_batch, every third slot too small")


def test_dictionary_batch(eng, oracle):
    _run_batch(eng, S.dictionary(oracle), "flate_hip_inflate_batch_dict")


# The lane-per-stream decoder sets up `out` and `bit_off` of a spliced piece on a path of its own, so its forms are
# run on spliced input too: 16 lanes (what the batch size gives), 32, and 64 without a row and with rows of 8 and 16.
SPLICED_LANE_FORMS = [(0, 0), (32, 0), (64, 0), (64, 8), (64, 16)]  # (inflate_lanes, inflate_row_dwords)


def test_spliced(oracle):
    import torch
    from test_splice import _inflaters
    batch = S.spliced(oracle)
    d_in = torch.from_numpy(np.frombuffer(batch.spliced + b"\0" * 16, np.uint8).copy()).cuda()
    e = flate.FlateEngine(0)
    try:
        for kernel in _inflaters(e):
            for lanes, row in SPLICED_LANE_FORMS if kernel == "lane_per_stream" else [(0, 0)]:
                e.set_option("inflate_lanes", lanes)
                e.set_option("inflate_row_dwords", row)
                for shift in SHIFTS:
                    whole, out = _prefilled(batch, shift)
                    res = e.inflate_spliced(d_in, len(batch.spliced), batch.bit_off, batch.caps, out=out, check=False)
                    assert res[0] is out and np.array_equal(res[1], batch.out_off)
                    _assert_footprint(batch, whole, shift, res[2], res[3], res[4],
                                      "flate_hip_inflate_spliced, %s, lanes %d, row %d" % (kernel, lanes, row))
    finally:
        e.close()


@pytest.mark.parametrize("config", [None, "lane_per_stream_64_row8", "lane_per_stream_64_row16"],
                         ids=["default_options", "lane_per_stream_64_row8", "lane_per_stream_64_row16"])
def test_framed_zlib(oracle, config):
    """flate_hip_inflate_batch_framed through ctypes, so that the slots are the corpus's."""
    import torch
    batch = S.framed(oracle)
    data, in_off = batch.in_blob()
    d_in = torch.from_numpy(data).cuda()
    e = flate.FlateEngine(0)
    try:
        if config:
            force_inflate_config(e, config)
        for shift in SHIFTS:
            whole, out = _prefilled(batch, shift)
            out_len = np.zeros(batch.n, np.uint64)
            status = np.full(batch.n, 99, np.int32)
            err_off = np.full(batch.n, 77, np.int64)
            used = np.full(batch.n, 12345, np.uint32)
            rc = e._L.flate_hip_inflate_batch_framed(
                e._ctx, d_in.data_ptr(), in_off.ctypes.data, batch.n, WRAP_ZLIB, None, None, 0, out.data_ptr(),
                batch.out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data,
                used.ctypes.data, DEVICE_PTRS)
            assert rc == -4 and (used == S.NO_DICT).all()  # (the first member is a guard: a bad header)
            _assert_footprint(batch, whole, shift, out_len, status, err_off, "flate_hip_inflate_batch_framed")
    finally:
        e.close()


def test_host_pointers_keep_the_outer_guards(oracle):
    """A host-pointer call copies the whole range of the slots back, so the guards between the slots mean nothing
    there: the bytes outside the range stay, and every stream's result and bytes are the oracle's."""
    batch = S.plain(oracle, "A")
    data, in_off = batch.in_blob()
    eng = flate.FlateEngine(0)
    try:
        for shift in SHIFTS:
            whole = np.full(shift + batch.image.size, S.FILL, np.uint8)
            out = whole[shift + S.OUTER:]
            res = eng.inflate_batch(data, in_off, batch.caps, out=out, check=False)
            assert res[0] is out
            after = whole[shift:].copy()
            lo, hi = S.OUTER, S.OUTER + batch.total
            assert (whole[:shift + lo] == S.FILL).all() and (after[hi:] == S.FILL).all()
            for g in range(0, batch.n, 2):  # (what the copy brought back into the guards' slots is not compared)
                after[lo + int(batch.out_off[g]):lo + int(batch.out_off[g + 1])] = S.FILL
            bad = batch.check(after, res[2], res[3], res[4])
            assert not bad, S.report(bad)
    finally:
        eng.close()


# One sequence of calls over the 70000-byte text payload in which every room of ROOMS is the room of many calls, at
# different places of the stream, and the whole takes a hundred calls rather than 70000.  Two orders: the 65536-byte
# room first and the small ones behind byte 65536, and the small ones first, at the head of the stream, with the
# 65536-byte room behind them (65604 bytes are still to come then).
ROOMS = [65536] + [1] * 50 + [7] * 50 + [333] * 12
ROOM_ORDERS = {"large_room_first": ROOMS, "small_rooms_first": ROOMS[1:] + ROOMS[:1]}


@pytest.mark.parametrize("order", sorted(ROOM_ORDERS))
def test_piecewise_reader_stays_inside_out_cap(oracle, order):
    """flate_hip_inflate_stream_read with an out array larger than out_cap: the bytes at and behind out + out_cap
    stay what they were, at every call."""
    rooms = ROOM_ORDERS[order]
    p = next(p for fill, p in S.payloads() if fill == "text" and len(p) == 70000)
    comp = np.frombuffer(oracle.deflate(np.frombuffer(p, np.uint8)), np.uint8)
    e = flate.FlateEngine(0)
    L = e._L
    st = C.c_void_p()
    e._check(L.flate_hip_inflate_stream_open(e._ctx, C.byref(st)))
    try:
        got, pos, rc, calls, seen = [], 0, 0, 0, set()
        while rc == 0:
            room = rooms[calls % len(rooms)]
            calls += 1
            assert calls < 1000, "no progress"
            out = np.full(room + 300, S.FILL, np.uint8)
            rest = comp[pos:].copy()
            used, n, eo = C.c_uint64(0), C.c_uint64(0), C.c_int64(-1)
            rc = L.flate_hip_inflate_stream_read(st, rest.ctypes.data if rest.size else None, rest.size, 1,
                                                 out.ctypes.data, room, C.byref(used), C.byref(n), C.byref(eo))
            assert rc in (0, 1), (rc, calls)
            assert n.value <= room and (out[room:] == S.FILL).all(), (calls, room, n.value)
            if n.value == room:
                seen.add(room)
            pos += used.value
            got.append(out[:n.value].tobytes())
        assert rc == 1 and b"".join(got) == p and pos == comp.size
        assert seen == set(ROOMS)  # every room was filled to its last byte
    finally:
        L.flate_hip_inflate_stream_free(st)
        e.close()
