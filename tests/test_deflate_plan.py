"""The encode plan and its launch routing (moonbit-flate_amd/csrc/deflate_plan.h) on the CPU: how a batch is cut into
windows and blocks, which match-finder list every stream joins, when the entropy stage runs per block, when multi-window
streams are scheduled by window, which lists get the paired launch, how a host-pointer batch is cut into groups, and what
the call's index arrays take of the control-array staging -- at the edges no GPU test can afford to reach (a 2 GiB
stream, window 32766, 131071 multi-window streams).  Offsets are just numbers here.  tests/host_model/
deflate_plan_model.cpp includes the header the driver includes; the `expected_*` functions restate the documented
rules."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "deflate_plan_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "deflate_plan.h"), os.path.join(CSRC, "flate_common.h"), os.path.join(INC, "flate_hip.h")]
LIB = os.path.join(HERE, "host_model", "libdeflate_plan_model.so")

OK, INVALID, TOO_LARGE = 0, -1, -6  # include/flate_hip.h
DEVICE_PTRS, COMPAT_GO, LZ_SERIAL = 1, 2, 4
W = 65535  # one LZ77 window, one block
LIMIT = 0x7ffe0000
NONE, SINGLE, MULTI, DICT = 0, 1, 2, 3
KEYS = ["guest_blocks", "guest_min", "resident_blocks", "window_units", "entropy_per_block", "spin_limit", "profile_split"]
DEFAULTS = dict(guest_blocks=0, guest_min=1280, resident_blocks=1024, window_units=1, entropy_per_block=-1,
                spin_limit=8 << 20, profile_split=0)  # (a ctx sets the first three from the device's CU count)
OPTS = dict(DEFAULTS, guest_blocks=1536, guest_min=1280)  # an MI355X's
EDGE_LENS = [0, 1, 16, 17, 127, 128, 65534, 65535, 65536, W + 127, W + 128, 4 * W]


def windows(length):
    return length // W + (1 if length % W >= 128 else 0)


def blocks(length):
    return length // W + (1 if length % W else 0)


def expected_plan(lens, has=None, compat_go=False):
    """rc, or (chunk_base, blk_base, list per stream)"""
    has = has or [0] * len(lens)
    cb, bb, lists = [0], [0], []
    for length, d in zip(lens, has):
        if length + (W if d else 0) >= LIMIT:
            return TOO_LARGE
        if not compat_go and windows(length) + (1 if d else 0) > 32766:
            return TOO_LARGE
        nch = windows(length)
        lists.append(NONE if nch == 0 else DICT if d else SINGLE if nch == 1 else MULTI)
        cb.append(cb[-1] + nch)
        bb.append(bb[-1] + blocks(length))
    return cb, bb, lists


def expected_route(lens, has, o, flags, spliced):
    """(per_block, uq_units, pair16, pair32, pairD)"""
    _, bb, lists = expected_plan(lens, has, bool(flags & COMPAT_GO))
    n, n_blocks = len(lens), bb[-1]
    per_block = o["entropy_per_block"] != 0 and n_blocks > 0 and not spliced and \
        (o["entropy_per_block"] == 1 or n_blocks >= 3 * n) and all(blocks(x) > 0 for x in lens)
    count = {k: lists.count(k) for k in (SINGLE, MULTI, DICT)}
    pair = {k: o["guest_blocks"] > 0 and count[k] >= o["guest_min"] for k in count}
    by_window = o["window_units"] and o["guest_blocks"] > 0 and o["guest_min"] <= count[MULTI] < 2 ** 17 - 1 and \
        not flags & LZ_SERIAL
    units = sum(windows(x) for x, k in zip(lens, lists) if k == MULTI)
    return (int(per_block), units if by_window and units < 0xffffffff else 0, int(pair[SINGLE]), int(pair[MULTI]),
            int(pair[DICT]))


def expected_groups(o, host_groups, host_group_streams, flags, n, total_bytes):
    if flags & DEVICE_PTRS or host_groups <= 1 or total_bytes < 64 << 20:
        return 0
    return min(host_groups, n // max(o["guest_min"], host_group_streams))


def old_ctl_begin(lens, has, framed, sum_up, dictid_up):
    """The expression deflate_common passed to ctl_begin before its terms moved beside their steps."""
    cb, bb, lists = expected_plan(lens, has)
    n = len(lens)
    f_up = 0
    if framed:
        f_up = n * 4 + 256 + sum_up
        if framed == "dict_of":
            f_up += dictid_up
    in_lists = sum(1 for k in lists if k != NONE)
    return (n + 1) * 16 + (in_lists + bb[-1]) * 4 + f_up, (n + 1) * 8 + 64


class Model:
    def __init__(self, L):
        self.L = L

    @staticmethod
    def _index(lens, start=0):
        off = np.zeros(len(lens) + 1, np.uint64)
        off[0] = start
        np.cumsum(np.asarray(lens, dtype=np.uint64), out=off[1:])
        off[1:] += np.uint64(start)
        return off

    def plan_off(self, off, flags=0, has=None):
        off = np.ascontiguousarray(off, np.uint64)
        n = off.size - 1
        cb, bb = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        lists, counts = np.zeros(max(n, 1), np.int32), np.zeros(5, np.uint64)
        h = None if has is None else np.asarray(has, np.uint8)
        rc = self.L.plan_model(off.ctypes.data, n, flags, None if h is None else h.ctypes.data, cb.ctypes.data, bb.ctypes.data,
                               lists.ctypes.data, counts.ctypes.data)
        if rc:
            return rc
        lists = lists[:n].tolist()
        assert counts.tolist() == [cb[-1], bb[-1], lists.count(SINGLE), lists.count(MULTI), lists.count(DICT)]
        return cb.tolist(), bb.tolist(), lists

    def plan(self, lens, flags=0, has=None, start=0):
        got = self.plan_off(self._index(lens, start), flags, has)
        assert got == expected_plan(lens, has, bool(flags & COMPAT_GO)), (lens, flags, has)
        return got

    def route(self, lens, has=None, flags=0, spliced=False, **opts):
        o = dict(OPTS, **opts)
        off = self._index(lens)
        h = None if has is None else np.asarray(has, np.uint8)
        out = (C.c_int64 * 5)()
        rc = self.L.route_model(off.ctypes.data, len(lens), flags, None if h is None else h.ctypes.data,
                                (C.c_int64 * 7)(*[o[k] for k in KEYS]), int(spliced), out)
        assert rc == 0
        got = tuple(out)
        assert got == expected_route(lens, has or [0] * len(lens), o, flags, spliced), (len(lens), lens[:4], flags, spliced, o)
        return got

    def groups(self, host_groups, host_group_streams, flags, n, total_bytes, **opts):
        o = dict(OPTS, **opts)
        got = self.L.groups_model((C.c_int64 * 7)(*[o[k] for k in KEYS]), host_groups, host_group_streams, flags, n, total_bytes)
        want = expected_groups(o, host_groups, host_group_streams, flags, n, total_bytes)
        assert (got if got > 1 else 0) == (want if want > 1 else 0), (host_groups, host_group_streams, flags, n, total_bytes, o)
        return got

    def ctl(self, lens, has, framed, sum_up, dictid_up):
        off = self._index(lens)
        h = None if has is None else np.asarray(has, np.uint8)
        out = (C.c_uint64 * 2)()
        rc = self.L.ctl_model(off.ctypes.data, len(lens), 0, None if h is None else h.ctypes.data, 1 if framed else 0,
                              dictid_up if framed == "dict_of" else 0, sum_up if framed else 0, out)
        assert rc == 0
        return tuple(out)


@pytest.fixture(scope="module")
def m():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    p = C.c_void_p
    L.plan_defaults.argtypes = [C.c_int64 * 7]
    L.plan_defaults.restype = None
    L.plan_model.argtypes = [p, C.c_uint32, C.c_uint32, p, p, p, p, p]
    L.route_model.argtypes = [p, C.c_uint32, C.c_uint32, p, C.c_int64 * 7, C.c_int, C.c_int64 * 5]
    L.groups_model.argtypes = [C.c_int64 * 7, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    L.groups_model.restype = C.c_uint32
    L.ctl_model.argtypes = [p, C.c_uint32, C.c_uint32, p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64 * 2]
    return Model(L)


def test_the_structs_defaults_are_the_documented_option_defaults(m):
    d = (C.c_int64 * 7)()
    m.L.plan_defaults(d)
    assert dict(zip(KEYS, d)) == DEFAULTS


# ---- make_plan ----

@pytest.mark.parametrize("compat_go", [False, True])
def test_plan_at_the_block_policy_edges(m, compat_go):
    flags = COMPAT_GO if compat_go else 0
    cb, bb, lists = m.plan(EDGE_LENS, flags, start=7)
    # under 128 bytes: blocks but no LZ77 window; one window up to 65535 + 127 bytes (the tail is a block of its own)
    assert lists == [NONE] * 5 + [SINGLE] * 5 + [MULTI] * 2
    assert np.diff(cb).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 4]
    assert np.diff(bb).tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 4]
    # with a dictionary: every stream that reaches the match finder starts from its table, the others are in no list
    has = [1] * len(EDGE_LENS)
    cbd, bbd, listsd = m.plan(EDGE_LENS, flags, has)
    assert (cbd, bbd) == (cb, bb) and listsd == [NONE] * 5 + [DICT] * 7
    # mixed: the prefix arrays do not depend on who has a dictionary
    has = [i % 2 for i in range(len(EDGE_LENS))]
    assert m.plan(EDGE_LENS, flags, has)[:2] == (cb, bb)
    assert m.plan([], flags) == ([0], [0], [])


def test_plan_refuses_a_decreasing_index(m):
    assert m.plan_off([5, 9, 8]) == INVALID
    assert m.plan_off([5, 9, 8], has=[1, 1]) == INVALID
    assert m.plan_off([0, 1, 0, LIMIT]) == INVALID
    assert m.plan_off([0, LIMIT, 1]) == TOO_LARGE  # (entry by entry, in order)


def test_plan_limits_of_one_stream(m):
    # 32-bit positions: a stream below 0x7ffe0000 bytes, a dictionary counting as one window of it.  (Without
    # FLATE_HIP_COMPAT_GO the window rule below refuses such a stream first.)
    assert m.plan([3, LIMIT - 1], COMPAT_GO)[2] == [NONE, MULTI]
    assert m.plan([3, LIMIT], COMPAT_GO) == TOO_LARGE
    assert m.plan([3, LIMIT - 1]) == TOO_LARGE
    assert m.plan([3, LIMIT - W - 1], COMPAT_GO, [0, 1])[2] == [NONE, DICT]
    assert m.plan([3, LIMIT - W], COMPAT_GO, [0, 1]) == TOO_LARGE
    assert m.plan([3, LIMIT - W], COMPAT_GO, [1, 0])[2] == [NONE, MULTI]  # (the dictionary is another stream's)
    # the reference clears its table at window 32766: batch streams end before it, with a dictionary one window earlier
    # (the last window is 128 bytes long: 32767 whole windows would pass the byte limit too)
    w = lambda k: (k - 1) * W + 128  # noqa: E731
    assert windows(w(32766)) == 32766
    assert m.plan([w(32766)])[0] == [0, 32766]
    assert m.plan([w(32767)]) == TOO_LARGE
    assert m.plan([w(32765)], has=[1])[0] == [0, 32765]
    assert m.plan([w(32766)], has=[1]) == TOO_LARGE
    for length, has in ((w(32766), None), (w(32767), None), (w(32765), [1]), (w(32766), [1])):
        assert m.plan([length], COMPAT_GO, has) != TOO_LARGE


def test_a_dictionary_stream_under_128_bytes_is_in_no_list(m):
    assert m.plan([127, 128, 0], has=[1, 1, 1])[2] == [NONE, DICT, NONE]


# ---- EncodeRoute ----

@pytest.mark.parametrize("per_block", [-1, 0, 1])
@pytest.mark.parametrize("spliced", [False, True])
def test_entropy_per_block(m, per_block, spliced):
    n = 6
    for n_blocks in (3 * n - 1, 3 * n):
        lens = [3 * W] * (n - 1) + [(n_blocks - 3 * (n - 1)) * W]
        got = m.route(lens, spliced=spliced, entropy_per_block=per_block)[0]
        assert got == int(not spliced and (per_block == 1 or (per_block == -1 and n_blocks >= 3 * n)))
        # one stream without a block: nobody would write its closing block
        lens = [4 * W] * (n - 2) + [(n_blocks - 4 * (n - 2)) * W, 0]
        assert sum(blocks(x) for x in lens) == n_blocks
        assert m.route(lens, spliced=spliced, entropy_per_block=per_block)[0] == 0
    assert m.route([], spliced=spliced, entropy_per_block=per_block)[0] == 0


def test_multi_window_streams_by_window(m):
    gm = OPTS["guest_min"]
    two = W + 128  # two windows
    for n32 in (gm - 1, gm, 2 ** 17 - 2, 2 ** 17 - 1):
        lens = [two] * n32 + [100, 200]  # (and streams of the other kinds, which do not count)
        on = gm <= n32 < 2 ** 17 - 1
        assert m.route(lens)[1] == (2 * n32 if on else 0)
        assert m.route(lens, window_units=0)[1] == 0
        assert m.route(lens, guest_blocks=0)[1] == 0
        assert m.route(lens, flags=LZ_SERIAL)[1] == 0
        assert m.route(lens, flags=COMPAT_GO)[1] == (2 * n32 if on else 0)
    # a dictionary's streams are scheduled whole: they are not in the multi-window list
    assert m.route([two] * gm, has=[1] * gm)[1:] == (0, 0, 0, 1)


def test_the_paired_launch_per_list(m):
    gm = 7
    shapes = {SINGLE: (200, 0), MULTI: (W + 128, 0), DICT: (200, 1)}
    for kind, (length, d) in shapes.items():
        for count in (gm - 1, gm):
            lens, has = [length] * count + [5], [d] * count + [d]
            got = m.route(lens, has, guest_min=gm)
            assert got[2:] == tuple(int(k == kind and count >= gm) for k in (SINGLE, MULTI, DICT)), (kind, count)
            assert m.route(lens, has, guest_min=gm, guest_blocks=0)[2:] == (0, 0, 0)
    # the lists are counted one by one: three lists one short of guest_min are three plain launches
    lens = [200] * (gm - 1) + [W + 128] * (gm - 1) + [200] * (gm - 1)
    has = [0] * (2 * gm - 2) + [1] * (gm - 1)
    assert m.route(lens, has, guest_min=gm)[2:] == (0, 0, 0)


# ---- encode_host_groups ----

def test_host_groups(m):
    MiB64 = 64 << 20
    for gm, hgs in ((1280, 2048), (5000, 2048), (1280, 4096)):
        per = max(gm, hgs)
        for host_groups, flags, total in itertools.product((0, 1, 8), (0, DEVICE_PTRS), (MiB64 - 1, MiB64)):
            for n in (per - 1, 2 * per - 1, 2 * per, 8 * per - 1, 8 * per, 9 * per):
                g = m.groups(host_groups, hgs, flags, n, total, guest_min=gm)
                pipelined = flags == 0 and host_groups == 8 and total >= MiB64 and n >= 2 * per
                assert (g > 1) == pipelined
                if pipelined:
                    assert g == min(8, n // per)
    assert m.groups(8, 2048, 0, 16384, MiB64) == 8 and m.groups(8, 2048, 0, 16383, MiB64) == 7


# ---- the control-array budget ----

@pytest.mark.parametrize("framed", [None, "framed", "dict_of"])
def test_the_budget_is_the_expression_it_replaced(m, framed):
    sizes = (0, 1, 5)
    for n16, n32, nD, rest in itertools.product(sizes, sizes, sizes, (0, 2)):
        lens = [200] * n16 + [2 * W + 128] * n32 + [W + 300] * nD + [20] * rest
        has = [0] * (n16 + n32) + [1] * nD + [1, 0][:rest]
        if not lens:
            continue
        sum_up, dictid_up = 8 * len(lens) + 64, 3 * 24 + 64
        got = m.ctl(lens, has, framed, sum_up, dictid_up)
        assert got == old_ctl_begin(lens, has, framed, sum_up, dictid_up), (n16, n32, nD, rest)
        # (the block list is counted whether or not the per-block form runs: the sum does not depend on the route)
        for per_block in (0, 1):
            m.route(lens, has, entropy_per_block=per_block)
