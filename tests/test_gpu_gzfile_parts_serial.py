"""A gzip file read in PARTS with short members decoded WHOLE inside a part, on the GPU:
flate_hip_gzfile_reader_set_serial_max / _last_route (GzFileReader.set_serial_max, .last_route).  Every call's eight
words, the bytes and last_route() must equal tests/gzfile_parts_serial_ref.py under gzfile_parts_ref.feed's capped loop
(the cap: the reference's own call count + 4), with host and device pointers, whatever the cuts and the capacity."""
import random

import numpy as np
import pytest

import gzfile_parts_ref as R0
import gzfile_parts_serial_ref as R
import gzfile_ref as gf
import gzfile_serial_ref as gs
import gzip_ref as gz
import one_ref
from util import flate

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROOM = 1 << 20
S = 4096


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def fixed(step):
    return lambda: iter(lambda: step, 0)


def reader(rd, device, routes, guard=False, shift=0, wrong_trailer=False):
    """`read` of gzfile_parts_ref.feed over an engine reader: (Call, the bytes); every call's last_route() goes to
    `routes`.  shift (device pointers): the part's address is that many bytes off a 256-byte boundary.  guard (device
    pointers): the output lies between guard regions; nothing outside out[0, out_len) may change (a call that reports a
    wrong trailer: out[0, out_cap))."""
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
        routes.append(rd.last_route())
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


def check(eng, m, sizes_of, device=False, out_cap=None, grow=4096, guard=False, shift=0, what="", wrong_trailer=False, rd=None):
    """The same feeding loop over the reference and over the device: every call's words, its route and the bytes are
    equal.  -> (the calls, the routes, the bytes)"""
    f = m.f
    m.reset()
    want_routes = []
    want_calls, want, want_rest = R.feed(R.model_reader(m, want_routes), f, sizes_of(), out_cap, 100000, grow)
    own = rd is None
    if own:
        rd = eng.open_gzfile_reader(device=device, serial_max=m.S)
    try:
        routes = []
        calls, got, rest = R.feed(reader(rd, device, routes, guard, shift, wrong_trailer), f, sizes_of(), out_cap,
                                  len(want_calls) + 4, grow)
        for i, (a, b) in enumerate(zip(calls, want_calls)):
            print(what, device, out_cap, i, a, b, routes[i], want_routes[i])
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(calls, want_calls)) if a != b][:3]
        assert calls == want_calls, (what, device, out_cap, bad, len(calls), len(want_calls))
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(routes, want_routes)) if a != b][:3]
        assert routes == want_routes, (what, device, out_cap, bad)
        assert got == want and rest == want_rest, (what, device)
    finally:
        if own:
            rd.close()
    return want_calls, want_routes, want


def forty_members():
    """Forty members of 200 .. 900 bytes of gzip_ref.text, two of three written with memLevel 1 so that they have
    several blocks (with S = 0 they are several units each) -> (file, plain)."""
    rng = random.Random(40)
    t = gz.text(40000, seed=40)
    parts, plain, at = [], [], 0
    for k in range(40):
        n = rng.randrange(200, 901)
        p = t[at:at + n]
        at += n
        parts.append(gf.wrap(one_ref.deflate(p, 6, mem=1), p) if k % 3 else gz.fixed(p))
        plain.append(p)
    return b"".join(parts), b"".join(plain)


@pytest.fixture(scope="module")
def forty():
    f, plain = forty_members()
    m = R.Model(f, S)
    assert m.plain == plain and m.w.status == 0 and m.w.n_members == 40 and m.w.n_units > 40
    return m, plain


@pytest.fixture(scope="module")
def mixed():
    f, plain, long_ones = gs.mixed_file()
    m = R.Model(f, S)
    assert m.plain == plain and m.w.status == 0
    return m, plain, long_ones


def good(calls, m, plain, got):
    assert calls[-1].rc == R.STREAM_END and got == plain
    assert sum(c.in_used for c in calls) == len(m.f) and sum(c.n_members for c in calls) == m.w.n_members


# ---- 1. one final part: every member whole ----

@pytest.mark.parametrize("device", (False, True))
def test_forty_short_members_in_one_final_part(eng, forty, device):
    m, plain = forty
    calls, routes, got = check(eng, m, fixed(1 << 20), device=device, guard=device, what="forty, one part")
    good(calls, m, plain, got)
    assert len(calls) == 1 and (calls[0].n_units, calls[0].n_members) == (40, 40)
    assert routes[0] == (40, 0, len(m.f))  # every member whole, no stop, no bit-offset search


# ---- 2. the same file in parts ----

@pytest.mark.parametrize("step", (256, 1024, 4096, 65536, "random"))
def test_forty_short_members_in_parts(eng, forty, step):
    """Which members a cut sends through units is the reference's to say.  A part that begins at a header always holds
    the step's new bytes, and no member of this file is longer than 1016 bytes: with parts of 1024 bytes and more every
    member is whole in some part.  Parts of 256 bytes, and the random ones, cut a member that is the part's first: that
    one is read through units."""
    m, plain = forty
    if step == "random":
        sizes = lambda: (random.Random(7).randrange(1, 3001) for _ in iter(int, 1))
        grow = 1500
    else:
        sizes, grow = fixed(step), step
    for device in (False, True):
        calls, routes, got = check(eng, m, sizes, device=device, guard=device, grow=grow, what=("forty", step))
        good(calls, m, plain, got)
    serial = sum(r[0] for r, c in zip(routes, calls) if c.in_used or c.out_len)
    if step != 65536:  # a part cuts a member: the chain stops in front of it, and the next call takes it whole
        stops = [i for i, r in enumerate(routes[:-1]) if r[1] == 1 and calls[i].in_used]
        assert stops and any(routes[i + 1][0] >= 1 and routes[i + 1][2] > 0 for i in stops)
    if step == 256:  # ... unless it is the part's first member: that one is read through units
        assert serial < 40 and sum(c.n_units for c in calls) > 40
    if step == 1024:
        assert max(m.w.member_off[j + 1] - m.w.member_off[j] for j in range(40)) <= 1016 and serial == 40
    if step == 65536:
        assert serial == 40 and len(calls) == 1


# ---- 3. long members between short ones ----

@pytest.mark.parametrize("step", (65536, 200000))
def test_long_members_through_units_short_ones_whole(eng, mixed, step):
    m, plain, long_ones = mixed
    for device in (False, True):
        calls, routes, got = check(eng, m, fixed(step), device=device, guard=device, grow=step, what=("mixed", step))
        good(calls, m, plain, got)
    w = m.w
    # both long members go through units across several calls
    long_units = sum(w.member_unit[j + 1] - w.member_unit[j] for j in long_ones)
    assert sum(c.n_units for c in calls) == w.n_members - len(long_ones) + long_units
    ends = [sum(c.in_used for c in calls[:i + 1]) for i in range(len(calls))]
    split = [any(w.member_off[j] < e < w.member_off[j + 1] for e in ends) for j in long_ones]  # a call ends inside it
    assert all(split) if step == 65536 else any(split)  # (a part of 200 000 bytes holds the first long member whole)
    for j in long_ones:
        assert w.member_unit[j + 1] - w.member_unit[j] >= 3 and w.member_off[j + 1] - w.member_off[j] > S
    # tiny members behind a continued long member are whole in the same call
    assert any(r[2] == 0 and r[0] >= 1 and c.n_units > r[0] for r, c in zip(routes[1:], calls[1:]))
    assert sum(r[0] for r in routes) == w.n_members - len(long_ones)


def test_rounds_of_three_units_between_whole_members(eng):
    """"one_round_units" lowered: the long member spans several rounds AND several parts, with whole members in front
    of it and behind it in the same calls -- the runs between whole members, and the window's carry out of the last."""
    f, plain = gf.interleaved_file()
    m = R.Model(f, S)
    eng.set_option("one_round_units", 3)
    try:
        for step, device in ((30000, True), (9000, False)):
            calls, routes, got = check(eng, m, fixed(step), device=device, grow=step, what=("interleaved, rounds of 3", step))
            good(calls, m, plain, got)
            assert sum(r[0] for r in routes) == 16 and any(r[0] and c.n_units > r[0] for r, c in zip(routes, calls))
    finally:
        eng.set_option("one_round_units", 4096)


# ---- 4. capacities ----

def test_out_cap_that_cuts_in_front_of_a_whole_member(eng, forty):
    m, plain = forty
    w = m.w
    for j in (1, 7):
        cap = w.out_off[w.member_unit[j]]
        for device in (False, True):
            calls, routes, got = check(eng, m, fixed(1 << 20), device=device, out_cap=cap, guard=device,
                                       what=("forty", "cap at member", j))
            # a BOUNDARY state: the first call uses the bytes up to member j's header, not its header too
            assert (calls[0].rc, calls[0].in_used, calls[0].out_len, calls[0].n_units) == (R.OK, w.member_off[j], cap, j)
            assert plain.startswith(got)


def test_out_cap_below_a_whole_members_size(eng, forty):
    """Such a member is cut into units (or its first unit does not fit: FLATE_HIP_E_OUT_TOO_SMALL), as the reference
    says; between guard regions nothing outside out[0, out_len) changes."""
    m, plain = forty
    sizes = m.w.sizes
    for cap in (min(sizes) - 1, sorted(sizes)[20], max(sizes) - 1):
        for device in (False, True):
            calls, routes, got = check(eng, m, fixed(1 << 20), device=device, out_cap=cap, guard=device,
                                       what=("forty", "cap", cap))
            assert plain.startswith(got) and calls[-1].rc in (R.STREAM_END, R.OUT_TOO_SMALL)
    f = bytearray(m.f)
    f[m.w.member_off[3] - 8] ^= 0x10  # member 2's CRC-32: the call that reports it may write up to its planned total
    bad = R.Model(bytes(f), S, plain=plain)
    calls, routes, got = check(eng, bad, fixed(1 << 20), device=True, out_cap=sum(sizes[:5]), guard=True, wrong_trailer=True,
                               what="a wrong trailer of a whole member")
    assert (calls[-1].rc, calls[-1].bad_member) == (R.CORRUPT, 2) and got == plain[:sum(sizes[:3])]


# ---- 5. every cut of a trailer and a header ----

def test_every_cut_inside_a_trailer_and_a_header(eng):
    f, plain = gf.tiny_file()
    m = R.Model(f, S)
    w = m.w
    j = 6  # the member with FEXTRA
    lo, hi = w.member_off[j] - 9, min(m.reach[w.member_unit[j]] + 10, w.member_off[j] + 48)
    for cut in range(lo, hi):
        device = cut % 2 == 0
        calls, routes, got = check(eng, m, lambda c=cut: iter([c]), device=device, shift=(0, 1, 15)[cut % 3],
                                   grow=len(f), what=("tiny_file", "cut", cut))
        good(calls, m, plain, got)


# ---- 6. failing files ----

def failing_files():
    """[(what, file, the plain it was made from)]"""
    three = gf.three_members()
    f = b"".join(x for x, _ in three)
    plain = b"".join(p for _, p in three)
    w = gf.Walk(f)
    out = []
    for k in range(3):
        for what, at, bit in (("CRC-32", -8, 0x40), ("ISIZE", -4, 0x01)):
            bad = bytearray(f)
            bad[w.member_off[k + 1] + at] ^= bit
            out.append(("a wrong %s in member %d" % (what, k), bytes(bad), plain))
    a, ab = w.member_off[1], w.member_off[2]
    out.append(("cut inside the last member's stream", f[:ab + (len(f) - ab) // 2], plain))
    out.append(("cut inside the last member's trailer", f[:-3], plain))
    out.append(("cut inside the middle member's header", f[:a + 7], plain))
    u = w.member_unit[1] + 2
    bad = bytearray(f)
    bit = w.unit_bit[u] + 1  # BTYPE = 2 -> 3
    bad[bit >> 3] |= 1 << (bit & 7)
    out.append(("BTYPE = 3 in the middle member", bytes(bad), plain))
    out.append(("eight zero bytes behind the last member", f + b"\0" * 8, plain))
    out.append(("garbage behind the last member", f + b"garbage, and more of it", plain))
    bad[w.member_off[1] - 8] ^= 1
    out.append(("a wrong trailer in front of a corrupt member", bytes(bad), plain))
    return out


@pytest.mark.parametrize("case", failing_files(), ids=[c[0] for c in failing_files()])
def test_failing_files(eng, case):
    what, f, plain = case
    m = R.Model(f, S, plain=plain)
    m0 = R0.Model(f, plain=plain)
    ends = set()
    for sizes_of, device, grow in ((fixed(1024), False, 1024), (fixed(5000), True, 5000), (fixed(1 << 20), False, 1)):
        calls, routes, got = check(eng, m, sizes_of, device=device, guard=device, grow=grow, what=what,
                                   wrong_trailer="wrong" in what)
        c = calls[-1]
        assert plain.startswith(got) and c.in_used == 0 and c.rc < 0
        # the S = 0 reader on the same cuts: the same sticky status and words
        rd = eng.open_gzfile_reader(device=device)
        try:
            m0.reset()
            n0 = len(R0.feed(R0.model_reader(m0), f, sizes_of(), None, 100000, grow)[0])
            calls0, got0, _ = R0.feed(reader(rd, device, []), f, sizes_of(), None, n0 + 4, grow)
        finally:
            rd.close()
        c0 = calls0[-1]
        assert (c.rc, c.bad_member, c.err_off, c.stream_err_off) == (c0.rc, c0.bad_member, c0.err_off, c0.stream_err_off), what
        assert got == got0, what
        ends.add((c.rc, c.bad_member, c.err_off, c.stream_err_off, got))
    assert len(ends) == 1, what  # whatever the cut


# ---- 7. the setting on the handle ----

def test_S_0_after_a_reset_is_the_reader_without_the_setting(eng, forty):
    m, plain = forty
    m0 = R.Model(m.f, 0)
    for device in (False, True):
        rd = eng.open_gzfile_reader(device=device, serial_max=S)
        try:
            calls, routes, got = check(eng, m, fixed(4096), device=device, grow=4096, what="S set", rd=rd)
            good(calls, m, plain, got)
            with pytest.raises(flate.FlateError):  # not fresh any more
                rd.set_serial_max(0)
            rd.reset()  # keeps S
            calls2, routes2, _ = check(eng, m, fixed(4096), device=device, grow=4096, what="S kept by reset", rd=rd)
            assert calls2 == calls and routes2 == routes
            rd.reset()
            rd.set_serial_max(0)
            calls0, routes0, got0 = check(eng, m0, fixed(4096), device=device, grow=4096, what="S back to 0", rd=rd)
            assert got0 == plain and set(routes0) == {R.NO_ROUTE}
            assert sum(c.n_units for c in calls0) == m.w.n_units
            # ... and every call is the one of gzfile_parts_ref.Model
            base = R0.Model(m.f)
            assert calls0 == R0.feed(R0.model_reader(base), m.f, fixed(4096)(), None, 100000, 4096)[0]
        finally:
            rd.close()
