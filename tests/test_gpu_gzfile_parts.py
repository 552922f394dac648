"""A gzip file of any members read in PARTS on the GPU: flate_hip_gzfile_reader_* (FlateEngine.open_gzfile_reader).
Every call's eight words and bytes must equal tests/gzfile_parts_ref.py (built on gzfile_ref.Walk, one_ref.Walk's reach
and zlib) whatever the cuts, with host and device pointers; failing files must end with flate_hip_gzfile_read's status
and words on the whole file (but for the one documented difference) and deliver the prefix the contract defines.  Every
feeding loop runs under a cap of calls: the reference's own count plus 4."""
import random

import numpy as np
import pytest

import gzfile_parts_ref as R
import gzfile_ref as gf
from util import flate

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROOM = 1 << 20


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def fixed(step):
    return lambda: iter(lambda: step, 0)


def reader(rd, device, guard=False, shift=0, wrong_trailer=False):
    """`read` of gzfile_parts_ref.feed over an engine reader: (Call, the bytes).  shift (device pointers): the part's
    address is that many bytes off a 256-byte boundary.  guard (device pointers): the output lies between guard
    regions; nothing outside out[0, out_len) may change (a call that reports a wrong trailer: out[0, out_cap))."""
    import torch

    def read(buf, final, out_cap):
        cap = ROOM if out_cap is None else out_cap
        part = np.frombuffer(buf, np.uint8)
        out = None
        if device:
            box = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
            part_t = box[shift:shift + len(buf)]
            part_t.copy_(torch.from_numpy(part.copy()))
            part = part_t
            if guard:
                whole = torch.full((cap + 512,), GUARD, dtype=torch.uint8, device="cuda")
                out = whole[256:256 + max(cap, 1)]
        used, got, res = rd.read(part, final=final, out=out, out_cap=cap)
        if guard and device:
            torch.cuda.synchronize()
            img = whole.cpu().numpy()
            n = res.out_len if res.rc != R.OUT_TOO_SMALL else 0
            if wrong_trailer and res.rc == R.CORRUPT:  # out[out_len, planned total) is unspecified there
                assert (img[:256] == GUARD).all() and (img[256 + cap:] == GUARD).all(), "bytes outside out[0, out_cap) changed"
            else:
                assert (img[:256] == GUARD).all() and (img[256 + n:] == GUARD).all(), "bytes outside out[0, out_len) changed"
        got = got.cpu().numpy() if device else got
        return R.Call(res.rc, used, res.out_len, res.n_members, res.n_units, res.bad_member, res.err_off,
                      res.stream_err_off), bytes(got)
    return read


def check(eng, m, sizes_of, device=False, out_cap=None, grow=4096, guard=False, shift=0, what="", twice=False,
          wrong_trailer=False):
    """The same feeding loop over the reference and over the device: every call's words and the bytes are equal."""
    f = m.f
    m.reset()
    want_calls, want, want_rest = R.feed(R.model_reader(m), f, sizes_of(), out_cap, 100000, grow)
    rd = eng.open_gzfile_reader(device=device)
    try:
        for _ in range(2 if twice else 1):
            calls, got, rest = R.feed(reader(rd, device, guard, shift, wrong_trailer), f, sizes_of(), out_cap,
                                      len(want_calls) + 4, grow)
            bad = [(i, a, b) for i, (a, b) in enumerate(zip(calls, want_calls)) if a != b][:3]
            assert calls == want_calls, (what, device, out_cap, bad, len(calls), len(want_calls))
            assert got == want and rest == want_rest, (what, device)
            if want_calls[-1].rc < 0 and want_calls[-1].rc != R.OUT_TOO_SMALL:  # sticky, with the same words
                import torch
                none = torch.zeros(0, dtype=torch.uint8, device="cuda") if device else b""
                _, _, res = rd.read(none, final=True, out_cap=64)
                c = want_calls[-1]
                assert (res.rc, res.out_len, res.bad_member, res.err_off, res.stream_err_off) == \
                    (c.rc, 0, c.bad_member, c.err_off, c.stream_err_off), what
            rd.reset()
    finally:
        rd.close()
    return want_calls, want


@pytest.fixture(scope="module")
def corpus():
    """{name: (Model, plain)}: every walk computed once, shared, never changed."""
    out = {}
    three = gf.three_members()
    out["three_members"] = (b"".join(x for x, _ in three), b"".join(p for _, p in three))
    out["tiny_file"] = gf.tiny_file()
    pm = gf.phase_members()
    out["phase_members"] = (b"".join(x for x, _ in pm), b"".join(p for _, p in pm))
    for what, f, plain in gf.decoy_files():
        out["decoy: " + what] = (f, plain)
    legal, lplain = gf.history_files()[:2]
    out["history: legal"] = (legal, lplain)
    models = {}
    for name, (f, plain) in out.items():
        m = R.Model(f)
        assert m.plain == plain and m.w.status == 0, name
        models[name] = (m, plain)
    return models


def good(calls, m, plain, got):
    assert calls[-1].rc == R.STREAM_END and got == plain
    assert sum(c.in_used for c in calls) == len(m.f)
    assert sum(c.n_members for c in calls) == m.w.n_members and sum(c.n_units for c in calls) == m.w.n_units


# ---- 1. the corpus, whatever the cuts ----

def test_fixed_parts(eng, corpus):
    for name, (m, plain) in corpus.items():
        for step, device in ((1024, False), (4096, True), (65536, False)):
            if step == 1024 and len(m.f) > 40000:
                continue
            calls, got = check(eng, m, fixed(step), device=device, guard=device, grow=step, what=(name, step))
            good(calls, m, plain, got)


def test_random_and_growing_parts(eng, corpus):
    rnd = random.Random(11)
    for name in ("three_members", "tiny_file", "phase_members"):
        m, plain = corpus[name]
        s = rnd.randrange(1 << 30)
        sizes = lambda s=s: (random.Random(s).randrange(1, 6000) for _ in iter(int, 1))
        for device in (False, True):
            calls, got = check(eng, m, sizes, device=device, grow=1500, what=(name, "random", s))
            good(calls, m, plain, got)
    # growing: three bytes short of the first unit of the middle member, then a byte a call
    m, plain = corpus["three_members"]
    first = m.reach[m.w.member_unit[1]] + 8 - 3
    calls, got = check(eng, m, lambda: iter([first, 0]), grow=1, what="growing by one byte")
    good(calls, m, plain, got)
    assert [c.n_units for c in calls[:4]] == [m.w.member_unit[1], 0, 0, 0] and calls[4].n_units >= 1


def test_every_cut_inside_a_trailer_and_a_header(eng, corpus):
    """tiny_file's member with FEXTRA, and three_members' middle one: the first part ends at every byte from the
    trailer in front to the first unit's end."""
    for name, j in (("tiny_file", 6), ("three_members", 1)):
        m, plain = corpus[name]
        w = m.w
        lo, hi = w.member_off[j] - 9, min(m.reach[w.member_unit[j]] + 10, w.member_off[j] + 48)
        for cut in range(lo, hi):
            device = cut % 4 == 0
            calls, got = check(eng, m, lambda c=cut: iter([c]), device=device, grow=len(m.f), what=(name, "cut", cut))
            good(calls, m, plain, got)


def test_tile_edges_at_shifted_addresses(eng):
    for i, (what, f, plain) in enumerate(gf.tile_edge_files()):
        m = R.Model(f)
        assert m.plain == plain
        for shift in (0, 1, 15):
            calls, got = check(eng, m, fixed(4096 if (i + shift) % 2 else 5000), device=True, shift=shift, grow=4096,
                               what=(what, shift))
            good(calls, m, plain, got)


def test_a_long_member_between_tiny_ones(eng):
    f, plain = gf.interleaved_file()
    m = R.Model(f)
    for step, device in ((65536, True), (20000, False)):
        calls, got = check(eng, m, fixed(step), device=device, guard=device, grow=step, what=("interleaved", step))
        good(calls, m, plain, got)
    # "one_round_units" lowered: the long member spans several rounds AND several parts -- the window's carry
    eng.set_option("one_round_units", 3)
    try:
        for step, device in ((30000, True), (9000, False)):
            calls, got = check(eng, m, fixed(step), device=device, grow=step, what=("interleaved, rounds of 3", step))
            good(calls, m, plain, got)
    finally:
        eng.set_option("one_round_units", 4096)


def test_stored_headers_start_units_too(eng, corpus):
    """Option "one_stored_units" at 1, recorded at open: the bytes, the end and the members are the same; the units
    are another rule's, so the calls are not held against the reference."""
    for name, (m, plain) in corpus.items():
        eng.set_option("one_stored_units", 1)
        try:
            readers = [(eng.open_gzfile_reader(device=dev), dev) for dev in (False, True)]
        finally:
            eng.set_option("one_stored_units", 0)
        for rd, dev in readers:
            try:
                calls, got, rest = R.feed(reader(rd, dev), m.f, fixed(1500)(), None, len(m.f) // 1500 + 40, 1500)
            finally:
                rd.close()
            assert calls[-1].rc == R.STREAM_END and got == plain and not rest, (name, dev)
            assert sum(c.in_used for c in calls) == len(m.f) and sum(c.n_members for c in calls) == m.w.n_members


# ---- 2. capacities ----

def test_out_cap_smaller_than_the_first_unit(eng, corpus):
    m, plain = corpus["three_members"]
    w = m.w
    size = w.out_off[1]
    for device in (False, True):
        rd = eng.open_gzfile_reader(device=device)
        try:
            read = reader(rd, device, guard=device)
            c, got = read(m.f, True, size - 1)
            assert (c.rc, c.in_used, c.out_len, got) == (R.OUT_TOO_SMALL, 0, size, b""), device
            # the state is unchanged: the same file from its first byte reads as ever
            calls, got, rest = R.feed(read, m.f, fixed(3000)(), None, 40, 3000)
            assert calls[-1].rc == R.STREAM_END and got == plain
        finally:
            rd.close()


def test_out_cap_that_cuts_at_a_members_first_unit(eng, corpus):
    """The capacity holds exactly the members in front: the call stops where a member's first unit starts, its
    trailer judged and the next header used."""
    for name in ("three_members", "tiny_file"):
        m, plain = corpus[name]
        w = m.w
        for j in (1, 2):
            cap = w.out_off[w.member_unit[j]]
            for device in (False, True):
                calls, got = check(eng, m, fixed(1 << 20), device=device, out_cap=max(cap, 1), guard=device,
                                   what=(name, "cap at member", j))
                if calls[-1].rc == R.STREAM_END:
                    assert got == plain
    m, plain = corpus["tiny_file"]
    for cap in (700, 1200, 3000):
        calls, got = check(eng, m, fixed(2000), out_cap=cap, grow=2000, what=("tiny_file", "cap", cap))
        assert plain.startswith(got)


# ---- 3. history never crosses a member ----

def test_history_behind_a_member_in_front(eng):
    legal, lplain, illegal, m0, p0, raw = gf.history_files()
    want = eng.gzfile_read(np.frombuffer(illegal, np.uint8))
    whole_out, q = want
    assert q.status == R.CORRUPT and q.bad_member == 1 and q.err_off == len(m0) and q.stream_err_off > 0
    delivered = bytes(whole_out[:q.out_len])
    # the cut puts the member in front into an earlier part (its bytes sit in the handle's window and in `out`), or
    # leaves both in one part
    for first, device in ((len(m0), False), (len(m0), True), (len(m0) + 10, True), (len(illegal), False), (20000, True)):
        rd = eng.open_gzfile_reader(device=device)
        try:
            calls, got, rest = R.feed(reader(rd, device, guard=device), illegal, iter([first]), None, 12, len(illegal))
        finally:
            rd.close()
        c = calls[-1]
        assert (c.rc, c.bad_member, c.err_off, c.stream_err_off) == (q.status, q.bad_member, q.err_off, q.stream_err_off), \
            (first, device, c)
        assert got == delivered and c.in_used == 0, (first, device, len(got), len(delivered))


# ---- 4. failing files ----

def failing_files():
    """[(what, file, the plain it was made from, documented difference)]"""
    three = gf.three_members()
    f = b"".join(x for x, _ in three)
    plain = b"".join(p for _, p in three)
    w = gf.Walk(f)
    out = []
    for k in range(3):
        for what, at, bit in (("CRC-32", -8, 0x40), ("ISIZE", -4, 0x01)):
            bad = bytearray(f)
            bad[w.member_off[k + 1] + at] ^= bit
            out.append(("a wrong %s in member %d" % (what, k), bytes(bad), plain, False))
    a, ab = w.member_off[1], w.member_off[2]
    out.append(("cut inside the last member's stream", f[:ab + (len(f) - ab) // 2], plain, False))
    out.append(("cut inside the last member's trailer", f[:-3], plain, False))
    out.append(("cut inside the middle member's header", f[:a + 7], plain, False))
    u = w.member_unit[1] + 2
    bad = bytearray(f)
    bit = w.unit_bit[u] + 1  # BTYPE = 2 -> 3
    bad[bit >> 3] |= 1 << (bit & 7)
    out.append(("BTYPE = 3 in the middle member", bytes(bad), plain, False))
    out.append(("eight zero bytes behind the last member", f + b"\0" * 8, plain, False))
    out.append(("garbage behind the last member", f + b"garbage, and more of it", plain, False))
    bad[w.member_off[1] - 8] ^= 1  # ... and member 0's CRC-32: the reader reports the trailer, the whole call the break
    out.append(("a wrong trailer in front of a corrupt member", bytes(bad), plain, True))
    return out


@pytest.mark.parametrize("case", failing_files(), ids=[c[0] for c in failing_files()])
def test_failing_files(eng, case):
    what, f, plain, differs = case
    m = R.Model(f, plain=plain)
    out, q = eng.gzfile_read(np.frombuffer(f, np.uint8), out_cap=len(plain) + 64)
    assert q.status < 0, what
    ends = set()
    for sizes_of, device, grow in ((fixed(1024), False, 1024), (fixed(5000), True, 5000), (fixed(1 << 20), False, 1)):
        calls, got = check(eng, m, sizes_of, device=device, guard=device, grow=grow, what=what,
                           wrong_trailer="wrong" in what)
        c = calls[-1]
        ends.add((c.rc, c.bad_member, c.err_off, c.stream_err_off, got))
        assert plain.startswith(got) and c.in_used == 0
        if not differs:
            assert (c.rc, c.bad_member, c.err_off, c.stream_err_off) == (q.status, q.bad_member, q.err_off, q.stream_err_off), \
                (what, c, q)
            trailer = q.stream_err_off >= 0 and q.err_off + q.stream_err_off <= len(f) and "wrong" in what
            if not trailer:
                assert got == bytes(out[:q.out_len]), what
            else:  # up to and including that member's last byte, and nothing behind it
                assert len(got) == m.w.out_off[m.w.member_unit[c.bad_member + 1]], what
        else:
            assert (q.status, q.bad_member) == (R.CORRUPT, 1) and (c.rc, c.bad_member, c.err_off) == (R.CORRUPT, 0, 0)
            assert c.stream_err_off == m.w.member_off[1] and len(got) == m.w.out_off[m.w.member_unit[1]]
    assert len(ends) == 1, what  # whatever the cut


def test_an_empty_file_and_reset(eng, corpus):
    rd = eng.open_gzfile_reader()
    try:
        used, got, res = rd.read(b"", final=True)
        assert (used, len(got), res.rc, res.n_members, res.n_units) == (0, 0, R.STREAM_END, 0, 0)
        used, got, res = rd.read(b"", final=True)
        assert res.rc == R.STREAM_END  # sticky
        rd.reset()
        used, got, res = rd.read(b"", final=False)
        assert (used, res.rc) == (0, R.OK)
    finally:
        rd.close()
    m, plain = corpus["three_members"]
    check(eng, m, fixed(2000), grow=2000, twice=True, what="reset, then the same file again")
    check(eng, m, fixed(3000), device=True, grow=3000, twice=True, what="reset, then the same file again")
