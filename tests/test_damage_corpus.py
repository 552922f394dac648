"""The damage corpus (tests/damage_corpus.py) without a GPU: the three references -- the oracle, one_ref.Walk and
zlib -- agree on every damaged stream, the classes the sweep exists for are all populated, and the build is
deterministic.

The counts this corpus reaches (1276 streams): corrupt 629, eof 72, valid_same_bytes 12, valid_other_bytes 563,
history_only 44, past_header 214, other_chain 70, good_units_behind_damage 583, corrupt with err_off in a later unit
198, damaged stored headers 70.  The minima below are the issue's, lower than these on purpose; they are conditions on
the references alone."""
import collections

import pytest

import damage_corpus as D

MINIMA = {"past_header": 150, "other_chain": 30, "valid_other_bytes": 200, "eof": 25, "history_only": 8, "later_unit": 100,
          "stored_header": 10}
CLASSES = ("corrupt", "eof", "valid_same_bytes", "valid_other_bytes", "history_only", "past_header", "other_chain",
           "good_units_behind_damage")


@pytest.fixture(scope="module")
def corpus(oracle):
    return D.corpus(oracle)


def test_the_bases_are_what_the_damage_is_planned_for(corpus):
    want = {"a": (29, 29, 0, 0), "b": (21, 21, 2, 23), "c": (18, 18, 0, 0)}  # units, dynamic, fixed, stored blocks
    for name, b in corpus.bases.items():
        assert D.composition(b.walk) == want[name], (name, D.composition(b.walk))
        assert 17 <= b.walk.n_units and 6000 <= len(b.raw) <= 8192 and len(b.plain) < 32768, name
        assert len(b.walk.reach) == b.walk.n_units
    assert not any(b[1] == 1 for b in corpus.bases["c"].walk.blocks) and corpus.bases["a"].plain == corpus.bases["c"].plain


def test_the_three_references_agree_on_every_stream(corpus):
    for c in corpus.cases:
        w, name = c.walk, c.damage.name
        mine = (c.status, c.err_off, len(c.out))
        if w.far and mine != (w.status, w.err_off, w.out_len):
            # the one verdict that needs history: the oracle's, at an offset that is not behind the walk's end
            end = w.err_off if w.status == D.CORRUPT else (w.end_bit + 7) // 8 if w.status == D.OK else len(c.damage.raw)
            assert c.status == D.CORRUPT and 0 < c.err_off <= end and len(c.out) < w.out_len, (name, mine, end)
        else:
            assert mine == (w.status, w.err_off, w.out_len), (name, mine, w.status, w.err_off, w.out_len)
        assert c.zlib_ok == (c.status == D.OK), (name, c.zlib_ok, c.status)
        if c.zlib_ok:
            assert c.zlib_out == c.out, name
        elif c.zlib_out:  # where zlib waits for more input, what it has delivered starts with the oracle's bytes or is their head
            n = min(len(c.zlib_out), len(c.out))
            assert c.zlib_out[:n] == c.out[:n], name
        assert ("history_only" in c.flags) <= w.far, name


def test_no_class_is_vacuous(corpus):
    got = D.counts(corpus.cases)
    print("damage corpus: %d streams, %s" % (len(corpus.cases), got))
    assert len(corpus.cases) >= 600
    for flag, least in MINIMA.items():
        assert got[flag] >= least, (flag, got[flag], least)
    per = collections.defaultdict(set)
    for c in corpus.cases:
        per["base " + c.damage.base] |= c.flags & set(CLASSES)
        per["kind " + c.damage.kind] |= c.flags & set(CLASSES)
    assert set(per) == {"base " + b for b in corpus.bases} | {"kind " + k for k in D.KINDS}
    for what, classes in per.items():
        assert len(classes) >= 2, (what, classes)
    # never the first and never the last unit; every flip and overwrite keeps the length
    for c in corpus.cases:
        d, b = c.damage, corpus.bases[c.damage.base]
        assert 0 < d.unit < b.walk.n_units - 1, d.name
        if d.kind in ("header", "eob", "body", "stored", "overwrite"):
            assert len(d.raw) == len(b.raw) and d.raw != b.raw, d.name
            assert b.walk.unit_bit[d.unit] <= (d.at if d.kind != "overwrite" else 8 * d.at) < b.walk.unit_bit[d.unit + 1], d.name


def test_two_builds_are_byte_identical(corpus):
    a, b = D.damages(), D.damages()
    assert a == b and D.digest(a) == D.digest(b)
    assert [c.damage for c in corpus.cases] == a
    assert len({d.name for d in a}) == len(a)
