"""tests/gzfile_parts_serial_ref.py on its own, without a GPU: the reference of the reader with whole members is held
against zlib and against gzfile_parts_ref.Model -- for every cut of two small files, S in (64, 4096) and out_cap in
(None, 300) the bytes are the plain text, the last call is FLATE_HIP_STREAM_END and the in_used sum to the file's
length; the sticky words of the failing files are the same for every cut and equal those at S = 0; with S = 0 every
call equals gzfile_parts_ref.Model's.

out_cap = 300 is below the size of some single units of both files (a stored block of 900 bytes, for one).  The
reader answers FLATE_HIP_E_OUT_TOO_SMALL with the size it needs and changes nothing; the loop here then repeats THAT
call with the capacity it asked for, as a caller with a bounded buffer has to, and goes on with 300."""
import pytest

import gzfile_parts_ref as R0
import gzfile_parts_serial_ref as R
import gzfile_ref as gf
from test_gzfile_parts_rule_model import failing_files


def files():
    three = b"".join(x for x, _ in gf.three_members())
    return [("three_members", three), ("tiny_file", gf.tiny_file()[0])]


def growing(read):
    """`read` of feed() that repeats a call that was FLATE_HIP_E_OUT_TOO_SMALL with the capacity it asked for."""
    def again(buf, final, out_cap):
        c, got = read(buf, final, out_cap)
        if c.rc == R.OUT_TOO_SMALL:
            assert c.out_len > out_cap and c.in_used == 0 and not got
            c, got = read(buf, final, c.out_len)
            assert c.rc != R.OUT_TOO_SMALL
        return c, got
    return again


@pytest.mark.parametrize("S", (64, 4096))
@pytest.mark.parametrize("what,f", files(), ids=[x for x, _ in files()])
def test_every_cut_gives_the_plain_text(what, f, S):
    plain = b"".join(gf.members_of(f))
    m = R.Model(f, S)
    walk_units = m.w.n_units
    some_whole = some_open = False
    for out_cap in (None, 300):
        for cut in range(0, len(f) + 1):
            m.reset()
            routes = []
            read = R.model_reader(m, routes)
            calls, out, rest = R.feed(growing(read) if out_cap else read, f, [cut], out_cap, 4000, grow=len(f))
            assert calls[-1].rc == R.STREAM_END and out == plain and not rest, (cut, out_cap)
            assert sum(c.in_used for c in calls) == len(f), (cut, out_cap)
            assert sum(c.n_units for c in calls) <= walk_units
            some_whole = some_whole or any(r[0] for r in routes)
            some_open = some_open or any(r[1] for r in routes)
    assert S == 64 or (some_whole and some_open)  # the new paths are taken (no member of three_members fits 64 bytes)


@pytest.mark.parametrize("case", failing_files()[1], ids=[x for x, _ in failing_files()[1]])
def test_the_sticky_words_do_not_depend_on_the_cut_or_on_S(case):
    what, f = case
    plain = failing_files()[0]
    ends = {}
    for S in (0, 64, 4096):
        m = R.Model(f, S, plain=plain)
        ends[S] = set()
        for cut in list(range(0, len(f) + 1, 7)) + [len(f)]:
            m.reset()
            calls, out, rest = R.feed(R.model_reader(m), f, [cut], None, 8, grow=len(f))
            c = calls[-1]
            assert c.rc < 0 and c.in_used == 0 and plain.startswith(out), (what, S, cut)
            ends[S].add((c.rc, c.bad_member, c.err_off, c.stream_err_off, len(out)))
            again, _ = m.read(5, False, 1 << 62)  # sticky
            assert again == R.Call(c.rc, 0, 0, 0, 0, c.bad_member, c.err_off, c.stream_err_off)
        assert len(ends[S]) == 1, (what, S, ends[S])
    assert ends[64] == ends[0] and ends[4096] == ends[0], (what, ends)


@pytest.mark.parametrize("what,f", files(), ids=[x for x, _ in files()])
def test_S_0_is_the_reader_without_the_setting(what, f):
    m0, m = R0.Model(f), R.Model(f, 0)
    for cut in range(0, len(f) + 1):
        m0.reset(), m.reset()
        routes = []
        a = R0.feed(R0.model_reader(m0), f, [cut], None, 8, grow=len(f))
        b = R.feed(R.model_reader(m, routes), f, [cut], None, 8, grow=len(f))
        assert a == b, cut
        assert set(routes) <= {R.NO_ROUTE}
    for cap, step in ((1, 700), (300, 64), (1500, 1000), (4096, 333)):
        m0.reset(), m.reset()
        a = R0.feed(R0.model_reader(m0), f, iter(lambda: step, 0), cap, 4000, grow=step)
        b = R.feed(R.model_reader(m), f, iter(lambda: step, 0), cap, 4000, grow=step)
        assert a == b, (cap, step)
