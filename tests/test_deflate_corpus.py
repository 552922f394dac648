"""The hand-built DEFLATE edge corpus (tests/deflate_corpus.py) against the oracle and zlib, without a GPU: every
base case reaches the rule it is written for, with the status, output and error offset pinned in it."""
import zlib

import pytest

import deflate_corpus as D

IDS = [c.name for c in D.CASES]


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_case_pins_the_oracle_result(case, oracle):
    rc, out, _, err_off = oracle.inflate(case.data, case.cap, full=True, zdict=case.zdict or None)
    assert rc == case.status, (rc, case.status)
    assert err_off == case.err_off, (err_off, case.err_off)
    assert len(out) == len(case.out)
    assert out == case.out


def test_every_required_rule_is_covered():
    rules = {c.rule for c in D.CASES}
    missing = [r for r in D.REQUIRED_RULES if r not in rules]
    assert not missing, missing
    assert len(IDS) == len(set(IDS))
    # errors of each kind, and valid streams of each block type, are all in the corpus
    assert {c.status for c in D.CASES} == {D.E_OK, D.E_CORRUPT, D.E_EOF, D.E_OUT_TOO_SMALL}


def _zlib(data, zdict):
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    try:
        out = d.decompress(data)
    except zlib.error:
        return "error", b""
    return ("end" if d.eof else "more"), out


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_zlib_agrees_or_the_difference_is_marked(case, oracle):
    verdict, out = _zlib(case.data, case.zdict)
    if case.status == D.E_OK:
        assert verdict == "end" and out == case.out
    elif case.status == D.E_OUT_TOO_SMALL:  # a valid stream and a slot that is too small
        assert verdict == "end" and out[:len(case.out)] == case.out and len(out) > case.cap
    elif case.status == D.E_CORRUPT:
        assert verdict == "error"
    elif case.zlib_rejects_at is None:  # E_UNEXPECTED_EOF: zlib waits for more input as well
        assert verdict == "more"
        assert out == case.out + case.zlib_more
    else:
        assert verdict == "error"
    if case.zlib_rejects_at is not None:
        # the documented difference: on this prefix zlib has rejected the stream, the reference still wants input
        cut = case.data[:case.zlib_rejects_at]
        assert _zlib(cut, case.zdict)[0] == "error"
        assert oracle.inflate(cut, 1 << 20, full=True, zdict=case.zdict or None)[0] == D.E_EOF


def test_lit_min_case_is_one_literal_short_of_zlib():
    """The reference reads lit_min bits before every literal/length code (inflate.mbt:545-547): a complete last
    code with fewer bits behind it is an unexpected end, where zlib delivers the literal."""
    c = next(c for c in D.CASES if c.rule == "lit_min")
    assert len(c.zlib_more) == 1
    assert _zlib(c.data, b"")[1] == c.out + c.zlib_more


def test_variants_are_well_formed():
    vs = D.variants()
    assert len({name for name, _, _, _ in vs}) == len(vs)
    small = [c for c in D.CASES if len(c.data) < 200]
    assert sum(1 for name, *_ in vs if "/cut" in name) == sum(len(c.data) for c in small)
    assert sum(1 for name, *_ in vs if "/prefix" in name) == len(D.CASES)
    # the prefix variants put every case at each of the eight bit phases behind some history
    for c in D.CASES[:8]:
        assert D.with_prefix(c, 3) != c.data
