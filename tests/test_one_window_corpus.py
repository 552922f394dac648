"""The test of the tests: tests/one_window_corpus.py on the CPU.  A hand-built stream proves something about the
window of flate_hip_inflate_one only if it is a stream zlib reads, if its units are the ones the case intends, if the
marked copy's source really starts in the unit the case says, and if a source that is off by one byte in either
direction gives other bytes.  Every expectation here is zlib's or the Python walker's (tests/one_ref.py), neither of
which shares a line with the code under test."""
import bisect
import zlib

import pytest

import one_ref as ref
import one_window_corpus as corpus

W = corpus.W
# the cases whose marked copy reaches the far end of the window: their largest marked distance is exactly 32768
CLAIM_W = (["far reach", "long pass-through", "stored blocks of 65535 and 0 bytes", "a unit starts at total == 32768"]
           + ["distance 32768, the source %d units back" % k for k in corpus.UNITS_BACK]
           + ["a unit of exactly %d bytes" % n for n in corpus.UNIT_SIZES])


@pytest.fixture(scope="module")
def good():
    return [(what, raw, plain, marks, ref.Walk(raw)) for what, raw, plain, marks in corpus.good_streams()]


def test_the_corpus_holds_every_case_by_name(good):
    names = [g[0] for g in good]
    assert len(set(names)) == len(names)
    for need in corpus.REQUIRED + CLAIM_W:
        assert sum(1 for n in names if n.startswith(need) or need in n) == 1, need
    twins = [t[0] for t in corpus.failing_twins()]
    assert sum("distance + 1" in t for t in twins) >= 3 and sum("cut inside unit" in t for t in twins) == 2
    assert any(t.startswith("a unit starts at total == 32767") and t.endswith("distance + 1") for t in twins)
    assert max(len(g[2]) for g in good) <= 140000


def test_good_streams_are_zlibs_and_have_the_units_they_intend(good):
    for what, raw, plain, marks, w in good:
        assert zlib.decompress(raw, -15) == plain, what
        n_units, src = corpus.intent(what)
        assert (w.status, w.out_bytes, w.far, w.n_units) == (0, len(plain), False, n_units), what
        assert len(src) == len(marks), what
        assert all(typ == 2 for at, typ, _, _ in w.blocks if at in w.unit_bit[1:-1]), what


def test_every_marked_source_starts_where_the_case_says_and_is_off_by_one_sensitive(good):
    """An overlapping copy (distance < length) has only `distance` bytes of source, and its slice moved up by one must
    end in front of the copy: there the comparison is over the bytes that exist before the copy runs."""
    n_marks = 0
    for what, raw, plain, marks, w in good:
        _, src = corpus.intent(what)
        for (pos, length, d), unit in zip(marks, src):
            n_marks += 1
            a = pos - d
            assert 0 <= a and 1 <= d <= W and 3 <= length <= 258, (what, pos)
            # Walk.out_off: unit u writes out_off[u] <= p < out_off[u + 1]; empty units own no byte
            assert bisect.bisect_right(w.out_off, a) - 1 == unit, (what, pos, d, w.out_off[:unit + 2])
            assert w.out_off[unit] <= a < w.out_off[unit + 1], (what, pos)
            n = min(length, d)
            assert plain[pos:pos + n] == plain[a:a + n], (what, pos)
            if a >= 1:
                assert plain[a - 1:a - 1 + n] != plain[a:a + n], (what, pos, "one byte further back reads the same")
            up = plain[a + 1:min(a + 1 + n, pos)]
            if up:
                assert up != plain[a:a + len(up)], (what, pos, "one byte nearer reads the same")
    assert n_marks >= 40


def test_the_far_end_of_the_window_is_read(good):
    """zlib writes no distance above 32506: the corpus is here for the ones above it."""
    for what, raw, plain, marks, w in good:
        if any(what.startswith(c) or c in what for c in CLAIM_W):
            assert max(m[2] for m in marks) == W, what
    reach = {m[2] for g in good for m in g[3]}
    assert {W, W - 1, corpus.ZLIB_MAX_DIST + 1, corpus.ZLIB_MAX_DIST} <= reach
    assert sum(1 for g in good if g[3] and max(m[2] for m in g[3]) > corpus.ZLIB_MAX_DIST) >= 15
    # the unit of 32767 bytes is read THROUGH: of the 258 source bytes exactly one lies in the unit in front of it
    what, raw, plain, marks, w = next(g for g in good if g[0].startswith("a unit of exactly 32767 bytes"))
    pos, length, d = marks[0]
    assert d == W and pos - d == w.out_off[2] - W == w.out_off[1] - 1 and w.out_off[2] - w.out_off[1] == W - 1
    # the chain of the long pass-through is deeper than 64 units
    what, raw, plain, marks, w = next(g for g in good if g[0].startswith("long pass-through"))
    (pos, _, d), (pos2, n2, d2) = marks
    assert w.n_units - 1 - 0 > 64 and w.out_off[1] == W and pos == w.out_off[-2] and pos - d < w.out_off[1]
    assert [w.out_off[k + 1] - w.out_off[k] for k in range(1, 71)] == [1] * 70 and (pos2 - d2, n2) == (w.out_off[1], 70)


def test_failing_twins_fail_as_they_should(good):
    twins = corpus.failing_twins()
    for what, raw, front, kind in twins:
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        w = ref.Walk(raw)
        if kind == "far":
            # (history-free, the walk goes through; the copy that reaches in front of the stream is noted)
            assert w.far and w.status == 0, what
            d = zlib.decompressobj(-15)
            try:
                d.decompress(raw)
            except zlib.error as e:
                assert "too far back" in str(e), (what, e)
        else:
            assert (w.status, w.far) == (ref.UNEXPECTED_EOF, False), what
            assert front[:w.out_len] == zlib.decompressobj(-15).decompress(raw)[:w.out_len], what
    by_name = {g[0]: g for g in good}
    for what, raw, front, kind in twins:
        base = by_name[what.split("; ")[0]]
        assert base[2].startswith(front) if kind == "far" else base[2] == front, what
        if kind == "far":
            assert any(pos == len(front) == d for pos, _, d in base[3]), what  # the good copy reaches byte 0 exactly
