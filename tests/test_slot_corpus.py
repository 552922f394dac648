"""The slot corpus (tests/slot_corpus.py) without a GPU: a plain Python decoder that writes exactly the oracle's bytes
passes the checker, and each mutant of it -- the wide stores of the decoders, one slot-edge condition wrong -- fails it
for the stated reason, with the right stream named."""
import numpy as np
import pytest

import slot_corpus as S

VARIANTS = {"plain_A": lambda o: S.plain(o, "A"), "plain_B": lambda o: S.plain(o, "B"), "dictionary": S.dictionary,
            "spliced": S.spliced, "framed": S.framed}


@pytest.fixture(scope="module", params=list(VARIANTS))
def batch(request, oracle):
    return VARIANTS[request.param](oracle)


@pytest.fixture(scope="module")
def plain_a(oracle):
    return S.plain(oracle, "A")


def test_plain_decoder_passes(batch):
    assert batch.check(*S.plain_decode(batch)) == []
    # and what a stream leaves in its own slot beyond out_len is nobody's business
    assert batch.check(*S.plain_decode(batch, scribble_tails=True)) == []


def test_conditions(batch, oracle):
    starts = batch.slot_starts()
    assert {s % 16 for s in starts} == set(range(16))
    assert len({s % 64 for s in starts}) >= 32
    if all(batch.meta[i].slack >= 0 for i in batch.real):  # (pass B trades some of the slack for slots too small)
        assert 2 * sum(1 for i in batch.real if batch.meta[i].slack == 0) >= len(batch.real)
        assert {batch.meta[i].slack for i in batch.real} == set(S.SLACKS)
    guards = [i for i in range(batch.n) if batch.meta[i] is None]
    assert len(guards) == len(batch.real) + 1 and guards[0] == 0 and guards[-1] == batch.n - 1
    assert all(batch.want_len[i] == 0 for i in guards)
    assert {int(batch.caps[i]) for i in guards} == set(S.GUARD_SLOTS)
    assert batch.image.size == 2 * S.OUTER + batch.total and S.OUTER >= 256
    assert (batch.image[:S.OUTER] == S.FILL).all() and (batch.image[-S.OUTER:] == S.FILL).all()


def test_both_guard_kinds_give_nothing(oracle):
    assert oracle.inflate(b"", 64, full=True)[:2] == (oracle.E_UNEXPECTED_EOF, b"")
    rc, got, _, err_off = oracle.inflate(b"\x07", 64, full=True)
    assert (rc, got, err_off) == (oracle.E_CORRUPT, b"", 1)
    b = S.plain(oracle, "A")
    assert {(int(b.want_status[i]), int(b.want_err_off[i])) for i in range(0, b.n, 2)} == {(-7, -1), (-4, 1)}
    assert {bytes(b.streams[i]) for i in range(0, b.n, 2)} == {b"", b"\x07"}


def test_sizes(oracle):
    a, b = S.plain(oracle, "A"), S.plain(oracle, "B")
    assert len(a.real) == len(S.LENGTHS) * len(S.FILLS) * len(S.ENCODERS) == 600
    assert 4_000_000 < a.total < 4_500_000
    short = [i for i in b.real if b.meta[i].slack < 0]
    assert {-b.meta[i].slack for i in short} == set(S.SHORT_BY)
    assert all(int(b.want_status[i]) == -2 and int(b.want_len[i]) <= int(b.caps[i]) for i in short)
    assert all(int(b.want_status[i]) == 0 for i in b.real if b.meta[i].slack >= 0)
    # slots too small end both at a refused literal (the slot full) and at a refused match (bytes left over)
    assert any(int(b.want_len[i]) == int(b.caps[i]) for i in short)
    assert any(int(b.want_len[i]) < int(b.caps[i]) for i in short)


def _pick(batch, cond, guard_in_front=2, guard_behind=2, guard_behind_max=64):
    """The first real stream that meets cond(meta), with guards of at least the given sizes around it."""
    for i in batch.real:
        if cond(batch.meta[i]) and batch.caps[i - 1] >= guard_in_front and \
                guard_behind <= batch.caps[i + 1] <= guard_behind_max:
            return i
    raise AssertionError("no such stream in the corpus")


_DECODED = {}


def _violations(batch, mutate):
    """What the checker finds in the plain decoder's image after mutate(image)."""
    if id(batch) not in _DECODED:
        _DECODED[id(batch)] = (batch, S.plain_decode(batch))
    clean, olen, status, err = _DECODED[id(batch)][1]
    img = clean.copy()
    mutate(img)
    vs = batch.check(img, olen, status, err)
    assert vs, "the mutant passed"
    assert all(v.message for v in vs)
    return vs


def _names(batch, v, i):
    m = batch.meta[i]
    return v.stream == i and all(s in v.message for s in (
        "fill %s" % m.fill, "encoder %s" % m.encoder, "length %d" % m.length, "slack %d" % m.slack,
        "slot start mod 64 = %d" % (int(batch.out_off[i]) % 64)))


def test_mutant_one_byte_behind_a_full_slot(plain_a):
    b = plain_a
    for length in (1, 17, 258, 70000):
        i = _pick(b, lambda m: m.slack == 0 and m.length == length)
        vs = _violations(b, lambda img: S.store(img, b, i, length, 1))
        assert len(vs) == 1 and vs[0].kind == "guard_slot" and vs[0].distance == 1 and _names(b, vs[0], i), vs


def test_mutant_16_byte_copy_store_across_the_slot_end(plain_a):
    b = plain_a
    for back in (1, 8, 15):  # the store starts inside the last 15 bytes of the slot
        i = _pick(b, lambda m: m.slack == 0 and m.length >= 16, guard_behind=16)
        vs = _violations(b, lambda img: S.store(img, b, i, b.meta[i].length - back, 16))
        assert len(vs) == 1 and vs[0].kind == "guard_slot" and vs[0].distance == 1 and _names(b, vs[0], i), vs
    # into a small guard the same store also reaches the next stream's bytes: both are reported
    i = _pick(b, lambda m: m.slack == 0 and m.length >= 16, guard_behind=1, guard_behind_max=13)
    vs = _violations(b, lambda img: S.store(img, b, i, b.meta[i].length - 1, 16))
    assert [v.kind for v in vs] == ["guard_slot", "bytes"] and _names(b, vs[0], i) and vs[1].stream == i + 2
    assert vs[1].distance == 0


def test_mutant_8_byte_literal_store_at_out_len_minus_3(plain_a):
    b = plain_a
    for slack in (0, 1, 3, 4):
        i = _pick(b, lambda m: m.slack == slack and m.length >= 3, guard_behind=8)
        vs = _violations(b, lambda img: S.store(img, b, i, b.meta[i].length - 3, 8))
        assert len(vs) == 1 and vs[0].kind == "guard_slot" and vs[0].distance == 1 and _names(b, vs[0], i), vs
    # with five bytes of slack or more the same store stays inside the slot: no violation
    i = _pick(b, lambda m: m.slack == 7 and m.length >= 3)
    img, olen, status, err = S.plain_decode(b)
    S.store(img, b, i, b.meta[i].length - 3, 8)
    assert b.check(img, olen, status, err) == []


def test_mutant_32_byte_row_store_across_the_slot_end(plain_a):
    b = plain_a
    for slack in (0, 7, 16):
        i = _pick(b, lambda m: m.slack == slack and m.length > 32 and
                  (m.length - 1) // 32 * 32 + 32 > m.length + slack)
        rbase = (b.meta[i].length - 1) // 32 * 32  # the row that holds the last byte, aligned to the slot start
        assert rbase + 32 > int(b.caps[i])
        vs = _violations(b, lambda img: S.store(img, b, i, rbase, 32))
        assert vs[0].kind == "guard_slot" and vs[0].distance == 1 and _names(b, vs[0], i), vs


def test_mutant_one_byte_in_front_of_a_slot(plain_a):
    b = plain_a
    for length in (1, 16, 65536):
        i = _pick(b, lambda m: m.length == length)
        vs = _violations(b, lambda img: S.store(img, b, i, -1, 1))
        assert len(vs) == 1 and vs[0].kind == "guard_slot" and vs[0].distance == -1 and _names(b, vs[0], i), vs


def test_mutant_any_write_into_an_empty_output_slot(plain_a, oracle):
    b = plain_a
    for g in list(range(0, 22, 2)) + list(range(22, b.n, 14)) + [b.n - 1]:  # every byte of a slot of each size,
        at = range(int(b.caps[g])) if g < 22 else [int(b.caps[g]) // 2]       # and one byte of guards all along
        for k in at:
            vs = _violations(b, lambda img: S.store(img, b, g, k, 1))
            assert len(vs) == 1 and vs[0].kind == "guard_slot" and b.meta[vs[0].stream] is not None, (g, k, vs)
            assert abs(vs[0].stream - g) == 1 and "slot of stream %d," % g in vs[0].message
    # a real stream that delivers nothing (its slot too small for its first token) may not be written either
    pb = S.plain(oracle, "B")
    empty = [i for i in pb.real if pb.want_len[i] == 0]
    for i in empty[:3]:
        vs = _violations(pb, lambda img: S.store(img, pb, i, 0, 1))
        assert len(vs) == 1 and vs[0].kind == "guard_slot" and vs[0].stream == i and vs[0].distance == 0


def test_mutant_a_write_behind_the_last_slot(plain_a):
    b = plain_a
    last = b.n - 1
    for k in (0, 1, 15, S.OUTER - 1):
        vs = _violations(b, lambda img: S.store(img, b, last, int(b.caps[last]) + k, 1))
        assert len(vs) == 1 and vs[0].kind == "outer_guard" and vs[0].distance == k + 1, vs
        assert _names(b, vs[0], b.real[-1])
    vs = _violations(b, lambda img: S.store(img, b, 0, -1, 1))  # and in front of the first
    assert len(vs) == 1 and vs[0].kind == "outer_guard" and vs[0].distance == -1 and _names(b, vs[0], b.real[0])


def test_mutant_wrong_bytes_and_wrong_results(plain_a):
    b = plain_a
    i = _pick(b, lambda m: m.length == 4097)
    vs = _violations(b, lambda img: img.__setitem__(S.OUTER + int(b.out_off[i]) + 4000,
                                                    img[S.OUTER + int(b.out_off[i]) + 4000] ^ 1))
    assert len(vs) == 1 and vs[0].kind == "bytes" and vs[0].distance == 4000 and _names(b, vs[0], i)
    for what in range(3):
        res = list(S.plain_decode(b))
        res[1 + what][i] += 1
        vs = b.check(*res)
        assert len(vs) == 1 and vs[0].kind == "result" and _names(b, vs[0], i)


def test_report_names_the_first_violations(plain_a):
    b = plain_a
    img, olen, status, err = S.plain_decode(b)
    for i in b.real[:20]:
        S.store(img, b, i, -1, 1)
    text = S.report(b.check(img, olen, status, err))
    assert text.startswith("20 violations") and text.count("fill ") == 6
