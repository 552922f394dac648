"""The reference of BGZF files in parts against itself (tests/bgzf_parts_ref.py): for every file of
bgzf_ref.index_corpus() and every schedule the GPU tests use, the concatenated bytes, the final status with bad_member
and err_off and the summed in_used are the same for every cut; good files come out as gzip.decompress says; the index
of the calls is the whole file's; the writer's concatenation is bgzf_ref.build_file's file for every cut.  (The call
that reaches a failure uses nothing, so for a file that fails the summed in_used is where the calls before it got to:
at most err_off, and the same for every cut only together with the members that call delivered.)"""
import gzip

import pytest

import bgzf_parts_ref as R
import bgzf_ref as ref

CORPUS = ref.index_corpus()
WINDOW = {"XLEN > 6 and padding subfields behind BC": True}


def run(f, sizes, grow, out_cap=R.UNBOUNDED, index_cap=None):
    m = R.ReaderModel(f)
    return R.feed(lambda part, final: m.read(part, final, out_cap, index_cap), f, sizes, 4 * len(f) + 64, grow)


@pytest.mark.parametrize("what,f", CORPUS, ids=[w for w, _ in CORPUS])
def test_every_cut_gives_the_same(what, f):
    w = ref.Walk(f)
    window_at = w.member_off[1] if what in WINDOW else None
    calls, data, rest = run(f, iter(()), 1)
    want = R.summary(calls, data)
    assert len(calls) == 1 and calls[0].rc != R.OK
    for name, sizes, grow in R.schedules(f, window_at):
        calls, data, rest = run(f, sizes(), grow)
        got = R.summary(calls, data)
        assert got[:4] == want[:4], name
        assert got[4] == want[4] if want[1] == R.STREAM_END else got[4] <= want[3], name
        assert all(c.rc == R.OK for c in calls[:-1]), name
    if want[1] == R.STREAM_END:
        assert data == (gzip.decompress(f) if f else b"") and want[4] == len(f)
    else:
        assert want[1] < 0 and want[4] == 0


@pytest.mark.parametrize("what,f,err_off,n", ref.malformed_files(), ids=[w for w, _, _, _ in ref.malformed_files()])
def test_malformed_words(what, f, err_off, n):
    calls, data, _ = run(f, R.fixed(100), 100)
    last = calls[-1]
    assert (last.rc, last.bad_member, last.err_off) == (R.CORRUPT, n, err_off)
    assert data == b"".join(R.member_verdict(m)[1] for m in ref.Walk(f[:err_off]).members(f[:err_off]))


@pytest.mark.parametrize("what,f,rc,bad", ref.failing_files(), ids=[w for w, _, _, _ in ref.failing_files()])
def test_failing_words(what, f, rc, bad):
    w = ref.Walk(f)
    for sizes, grow in ((iter(()), 1), (R.fixed(100), 100)):
        calls, data, _ = run(f, sizes, grow)
        last = calls[-1]
        assert (last.rc, last.bad_member, last.err_off) == (rc, bad, w.member_off[bad])
        assert len(data) == w.out_off[bad] and last.in_used == 0


@pytest.mark.parametrize("index_cap", [1, 2, 3, 1 << 30])
@pytest.mark.parametrize("what,f", ref.header_files() + [("65 members", ref.many_members(65)[0])])
def test_the_index_is_the_whole_files(what, f, index_cap):
    w = ref.Walk(f)
    m = R.ReaderModel(f)
    moff, ooff, calls = [0], [0], 0
    buf, pos = b"", 0
    while True:
        calls += 1
        assert calls < 4 * len(f) + 64
        buf, pos = buf + f[pos:pos + 1000], min(len(f), pos + 1000)
        c = m.read(buf, pos == len(f), R.UNBOUNDED, index_cap)
        if c.rc == R.OUT_TOO_SMALL:  # index_cap 1 holds no member: repeatable, nothing changed
            assert index_cap == 1 and c.bad_member == R.NONE
            return
        assert c.member_off[0] == moff[-1] and c.out_off[0] == ooff[-1] and len(c.member_off) == c.n_members + 1 <= index_cap
        moff += c.member_off[1:]
        ooff += c.out_off[1:]
        buf = buf[c.in_used:]
        if c.rc != R.OK:
            break
    assert c.rc == R.STREAM_END and moff == list(w.member_off) and ooff == list(w.out_off)


def test_small_rooms_change_nothing():
    f = ref.header_files()[1][1]
    w = ref.Walk(f)
    plain = gzip.decompress(f)
    for cap in (0, 1, w.out_off[1] - 1, w.out_off[1], w.out_off[2] - 1):
        m = R.ReaderModel(f)
        out, buf, cur = [], f, cap
        for _ in range(20):
            c = m.read(buf, True, cur)
            if c.rc == R.OUT_TOO_SMALL:
                assert c.bad_member == R.NONE and c.in_used == 0 and c.out_len > cur
                cur = c.out_len
                continue
            out.append(c.data)
            buf = buf[c.in_used:]
            cur = cap
            if c.rc != R.OK:
                break
        assert c.rc == R.STREAM_END and b"".join(out) == plain


def test_part_stop():
    assert [R.part_stop(a, False) for a in (0, 1, 65535, 65536)] == [R.BOUNDARY, R.STOP, R.STOP, R.DEAD]
    assert [R.part_stop(a, True) for a in (0, 1, 65536)] == [R.BOUNDARY, R.DEAD, R.DEAD]


@pytest.mark.parametrize("bb", [0, 4096, 1])
def test_writer_concatenation(oracle, bb):
    for n, data in ref.write_inputs().items():
        if bb == 1 and n > 300:
            continue
        step = bb or ref.BLOCK_DEFAULT
        want, off = ref.build_file(oracle, data, bb, 0)
        for sizes, grow in ((iter(()), 1), (R.fixed(step), step), (R.fixed(2 * step + 5), step), (R.fixed(step - 1 or 1), step - 1 or 1),
                            (R.random_sizes(n + bb, 3 * step), step)):
            m = R.WriterModel(oracle, data, bb, 0)
            calls, got, rest = R.feed(m.write, data, sizes, 4 * len(data) + 64, grow)
            assert got == want and calls[-1].rc == R.STREAM_END and rest == b""
            assert sum(c.in_used for c in calls) == len(data)
            moff = [0]
            for c in calls:
                assert c.member_off[0] == moff[-1]
                moff += c.member_off[1:]
            assert moff == [int(x) for x in off]
            assert m.write(b"", True).rc == R.INVALID
        assert gzip.decompress(want) == data
