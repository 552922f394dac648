"""The dense batch's chase over its fast events, two events per step against one (moonbit-flate_amd/csrc/
lz77_chase_rule.h), on the CPU.  tests/host_model/lz77_chase_model.cpp includes the header the kernels include.

The pair word of a lane is a pure function of the 64 event words, and the two-event chase must leave what the batch
reads behind the chase -- the start lanes visited (VIS), the match lanes (MF), the lane it ended at and bits 16 / 17 of
the last word -- exactly as the one-event chase does, from every start lane.  Constructed arrays hold the edges, each
also against a chase written out here; a few hundred thousand random legal arrays follow.  Two mutant builds of the
model -- one forgets the intermediate start lane in VIS, one ignores the second event's stop bit -- must fail the same
checks: the checks can see both faults."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "lz77_chase_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "lz77_chase_rule.h")]
KEEP = 61  # kDenseKeep
SLOW, ENDS, STOP = 1 << 16, 1 << 17, 1 << 18


def _load(tag, flags):
    lib = os.path.join(HERE, "host_model", "liblz77_chase_model%s.so" % tag)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in DEPS):
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC] + flags + [SRC, "-o", tmp])
        os.replace(tmp, lib)
    L = C.CDLL(lib)
    L.chase_compare.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64)]
    L.chase_compare.restype = C.c_int
    L.chase_pair_word.argtypes = [C.c_uint32] * 3
    L.chase_pair_word.restype = C.c_uint32
    L.chase_ev_word.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.chase_ev_word.restype = C.c_uint32
    L.chase_random.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.chase_random.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def model():
    return _load("", [])


MUTANTS = ["CHASE_MUTANT_DROP_MIDDLE", "CHASE_MUTANT_IGNORE_STOP2"]


@pytest.fixture(scope="module", params=MUTANTS)
def mutant(request):
    return _load("_" + request.param.lower(), ["-D" + request.param])


def fast(L, lane_of_match, length, ends=False):
    assert lane_of_match > 0 and 4 <= length <= 15
    return L.chase_ev_word(lane_of_match, length, 0, int(ends))


def slow(L, fv=64, length=4):
    return L.chase_ev_word(fv, length, 1, 0)


def chase_here(ev, a):
    """The one-event chase of lz77_stream, written out: x = ev[a]; slow => out; visit; a = next; stop => out."""
    vis = mf = 0
    while True:
        x = ev[a]
        if x & SLOW:
            return vis, mf, a, SLOW
        vis |= 1 << a
        mf |= 1 << (x & 63)
        a = x >> 24
        if x & STOP:
            return vis, mf, a, x & ENDS


def cases(L):
    """name -> (64 event words, start lane).  Lanes that are not named hold an event without a match lane (slow)."""
    out = {}

    def arr(**lanes):
        ev = [slow(L)] * 64
        for k, v in lanes.items():
            ev[int(k[1:])] = v
        return ev

    out["first event slow"] = (arr(), 0)
    out["first event slow, long match"] = (arr(l0=slow(L, 3, 15)), 0)
    out["second event of a pair slow"] = (arr(l0=fast(L, 2, 5)), 0)  # next lane 6: slow
    out["a chain of one event, stop on the first hop"] = (arr(l0=fast(L, 60, 6)), 0)  # next lane 65
    out["stop on the second hop"] = (arr(l0=fast(L, 5, 4), l8=fast(L, 56, 9)), 0)  # 0 -> 8 -> 64
    out["ends on the first hop"] = (arr(l0=fast(L, 5, 4, ends=True), l8=fast(L, 10, 4)), 0)
    out["ends on the second hop"] = (arr(l0=fast(L, 5, 4), l8=fast(L, 10, 4, ends=True), l13=fast(L, 15, 4)), 0)
    out["ends on the third hop, behind a pair"] = (
        arr(l0=fast(L, 5, 4), l8=fast(L, 10, 4), l13=fast(L, 15, 4, ends=True), l18=fast(L, 20, 4)), 0)
    out["next lane exactly 61, first hop"] = (arr(l0=fast(L, 50, 12)), 0)  # 61 <= kDenseKeep: goes on, lane 61 is slow
    out["next lane exactly 62, first hop"] = (arr(l0=fast(L, 50, 13), l62=fast(L, 63, 4)), 0)  # stop: lane 62 not read
    out["next lane exactly 61, second hop"] = (arr(l0=fast(L, 1, 4), l4=fast(L, 47, 15), l61=fast(L, 63, 5)), 0)
    out["next lane exactly 62, second hop"] = (arr(l0=fast(L, 1, 4), l4=fast(L, 48, 15), l62=fast(L, 63, 4)), 0)
    out["fv = 63 on the first hop"] = (arr(l10=fast(L, 63, 4)), 10)
    out["fv = 63 on the second hop"] = (arr(l10=fast(L, 12, 4), l15=fast(L, 63, 15)), 10)
    out["start lane 61"] = (arr(l61=fast(L, 62, 4)), 61)
    out["three events: a pair and one more"] = (arr(l0=fast(L, 1, 4), l4=fast(L, 5, 4), l8=fast(L, 9, 4)), 0)
    out["four events, then a slow one"] = (
        arr(l2=fast(L, 3, 7), l9=fast(L, 12, 5), l16=fast(L, 17, 4), l20=fast(L, 30, 11), l40=slow(L, 50, 15)), 2)
    longest = [fast(L, l + 1, 4) if l < 63 else slow(L) for l in range(64)]  # matches of 4 from lane 0: 0, 4, .., 60
    out["the longest chain"] = (longest, 0)
    out["the longest chain from lane 1"] = (longest, 1)  # 1, 5, .., 61: lane 61 stops (next 65)
    out["the longest chain from lane 2"] = (longest, 2)  # 2, 6, .., 58 -> 62: stop on a second hop
    return out


def compare(L, ev, a):
    buf = (C.c_uint64 * 8)()
    same = L.chase_compare((C.c_uint32 * 64)(*ev), a, buf)
    return same, tuple(buf[0:4]), tuple(buf[4:8])


def test_constructed_edges(model):
    for name, (ev, a) in cases(model).items():
        same, single, paired = compare(model, ev, a)
        assert single == chase_here(ev, a), name
        assert same == 1 and paired == single, (name, [hex(v) for v in single], [hex(v) for v in paired])


def test_the_edges_are_the_edges_they_say(model):
    c = cases(model)
    vis, mf, a, ex = chase_here(*c["the longest chain"])
    assert bin(vis).count("1") == 16 and a == 64 and ex == 0
    assert chase_here(*c["next lane exactly 61, first hop"])[2:] == (61, SLOW)
    assert chase_here(*c["next lane exactly 62, first hop"])[2:] == (62, 0)
    assert chase_here(*c["next lane exactly 61, second hop"])[0] == (1 << 0) | (1 << 4) | (1 << 61)
    assert chase_here(*c["next lane exactly 62, second hop"])[2:] == (62, 0)
    assert chase_here(*c["ends on the second hop"])[2:] == (13, ENDS)
    assert chase_here(*c["fv = 63 on the second hop"])[1] == (1 << 12) | (1 << 63)


def test_every_start_lane_of_every_edge_array(model):
    for name, (ev, _) in cases(model).items():
        for a in range(KEEP + 1):
            same, single, paired = compare(model, ev, a)
            assert same == 1 and single == chase_here(ev, a), (name, a)


def test_the_pair_word_has_the_stated_layout(model):
    e0, e1 = fast(model, 5, 4), fast(model, 20, 9, ends=True)  # lane 3 -> 8 -> 28, the second ends the chunk
    w = model.chase_pair_word(3, e0, e1)
    assert (w & 0x7f, (w >> 8) & 63, (w >> 19) & 63, w >> 25) == (20, 5, 8, 28)
    assert w & (1 << 15) == 0 and w & SLOW == 0 and w & ENDS and w & STOP
    # my event alone (it stops): both halves name it; the next word is not looked at
    e = fast(model, 60, 6)
    for other in (0, 0xffffffff, e1):
        w = model.chase_pair_word(7, e, other)
        assert (w & 0x7f, (w >> 8) & 63, (w >> 19) & 63, w >> 25) == (60, 60, 7, 65) and w & STOP and not w & SLOW
    # my event, then one that needs the general path: out at its lane with bit 16
    w = model.chase_pair_word(3, e0, slow(model))
    assert (w & 0x7f, (w >> 8) & 63, (w >> 19) & 63, w >> 25) == (5, 5, 3, 8) and w & STOP and w & SLOW
    # my own event needs the general path: nothing to do
    assert model.chase_pair_word(3, slow(model, 9, 15), e1) == (1 << 15) | SLOW


RANDOM = [(1, 60000, 10, 50), (2, 60000, 3, 90), (3, 60000, 30, 20), (4, 60000, 0, 100), (5, 60000, 60, 50)]


@pytest.mark.parametrize("seed,count,slow_pct,short_pct", RANDOM)
def test_random_legal_arrays(model, seed, count, slow_pct, short_pct):
    # 300 000 arrays in all, each from the 62 start lanes
    assert model.chase_random(seed, count, slow_pct, short_pct) == 0


def test_a_mutant_fails_the_constructed_edges(mutant):
    failed = [name for name, (ev, a) in cases(mutant).items() if compare(mutant, ev, a)[0] != 1]
    assert failed, "no constructed array sees this mutant"


def test_a_mutant_fails_the_random_arrays(mutant):
    assert mutant.chase_random(1, 2000, 10, 50) > 0
