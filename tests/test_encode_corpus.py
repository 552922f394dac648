"""The encoder's edge corpus (tests/encode_corpus.py) against the oracle, without a GPU: every rule the corpus is
built for is reached by a case -- judged from the oracle's output alone --, the oracle's streams inflate with zlib,
and the header reader that detects the rules agrees with the oracle block by block."""
import numpy as np
import pytest

import encode_corpus as E
from util import flate, raw_inflate


@pytest.fixture(scope="module")
def analyses(oracle):
    return E.analyses(oracle)


def test_every_required_rule_is_covered(analyses):
    cov = E.coverage(analyses)
    missing = [r for r in E.REQUIRED_RULES if r not in cov]
    assert not missing, missing
    names = [name for name, _, _ in E.cases()]
    assert len(names) == len(set(names))
    assert len(E.REQUIRED_RULES) == len(set(E.REQUIRED_RULES))


def test_each_rule_is_reached_by_the_case_built_for_it(analyses):
    cov = E.coverage(analyses)
    assert sorted(E.COVERED_BY) == E.REQUIRED_RULES
    wrong = [(r, c) for r, c in E.COVERED_BY.items() if c not in cov.get(r, [])]
    assert not wrong, wrong


def test_limit_cases_state_what_the_oracle_showed(analyses):
    """The three length limits, with the figures: the longest code is the limit, a plain Huffman tree is deeper."""
    by = {(a.name, a.compat): a.blocks[0] for a in analyses}
    for compat in E.BOTH:
        b = by[("fib_literals", compat)]
        assert b["kind"] == E.HUFF and max(b["hdr"]["lit_lens"]) == 15 and E.unlimited_depth(b["lit_hist"]) == 19
        b = by[("fib_literals_dynamic", compat)]
        assert b["kind"] == E.DYN and max(b["hdr"]["lit_lens"]) == 15 and E.unlimited_depth(b["lit_hist"]) == 18
        b = by[("fib_offsets", compat)]
        assert b["kind"] == E.DYN and max(b["hdr"]["dist_lens"]) == 15 and E.unlimited_depth(b["dist_hist"]) == 17
        assert b["dist_hist"][b["dist_hist"] > 0].tolist() == sorted(E.fib(18), reverse=True)[:2] + [987] + \
            sorted(E.fib(18), reverse=True)[3:]
        b = by[("fib_code_lengths", compat)]
        cl_hist = np.bincount([s for s, _ in b["hdr"]["items"]], minlength=19)
        assert max(b["hdr"]["cl_lens"]) == 7 and E.unlimited_depth(cl_hist) == 8
        assert sorted(cl_hist[cl_hist > 0].tolist()) == E.fib(9)


def test_oracle_streams_inflate_with_zlib(oracle):
    for name, data, _ in E.cases():
        for compat in E.BOTH:
            assert raw_inflate(oracle.deflate(data, compat=compat)) == data, (name, compat)


def test_header_reader_agrees_with_the_oracle(analyses):
    """Codes re-made from the parsed lengths decode every block to in_len bytes and to the next block's bit_start;
    the block type, LEN and the token count are the oracle's."""
    for an in analyses:
        for i, b in enumerate(an.blocks):
            h = b["hdr"]
            assert h["btype"] == (0 if b["kind"] == E.STORED else 2), (an.name, i)
            assert h["final"] == (1 if i == len(an.blocks) - 1 else 0), (an.name, i)
            nbytes, ntok, end = E.walk_block(an.out, h)
            nxt = an.blocks[i + 1]["bit_start"] if i + 1 < len(an.blocks) else 8 * len(an.out)
            assert (nbytes, end) == (b["in_len"], nxt), (an.name, an.compat, i, nbytes, b["in_len"], end, nxt)
            if b["kind"] == E.DYN:
                assert ntok == b["ntokens"], (an.name, i)
            elif b["kind"] == E.HUFF:
                assert ntok == b["in_len"] and (h["nlit"], h["ndist"], h["dist_lens"]) == (257, 1, [1]), (an.name, i)


def test_blocks_follow_the_switch(analyses):
    """enc_speed (deflate.mbt:266): more than n - (n >> 4) tokens -> the Huffman-only writer; and the sweeps
    reach every distance -4 .. +4 from the edge, for a full window and a small one."""
    seen = {}
    for an in analyses:
        for b in an.blocks[:-1]:
            if b["in_len"] == E.W or b["in_len"] >= 128:
                d = E.switch_distance(b)
                assert b["kind"] in ((E.HUFF, E.STORED) if d > 0 else (E.DYN, E.STORED)), (an.name, d, b["kind"])
                if an.name.startswith("switch_"):
                    seen.setdefault(b["in_len"], set()).add(d)
    assert all(set(range(-4, 5)) <= v for v in seen.values()) and set(seen) == {E.W, 272}, seen


def test_stored_decision_family_is_a_sweep_of_one_byte(analyses):
    cov = E.family_facts(analyses)["stored_flip_both_sides"]
    assert any("n65535" in c for c in cov) and any("n2000" in c for c in cov), cov


def test_chunks_are_the_engines():
    for n in (0, 1, 127, 128, 400, E.W - 1, E.W, E.W + 1, E.W + 127, E.W + 128, 3 * E.W, 10 * E.W + 5000):
        assert E.lz_chunks(n) == flate.lz_chunks(n), n


def test_generation_is_deterministic():
    assert E._build_cases() == E.cases()


def test_dense_window_stays_below_the_record_cap(analyses):
    """kMatchCapPerChunk = 16384 records per chunk: no case may reach it (65535 / 4 < 16384 by construction)."""
    most = max(E.token_stats(t)[2].size for an in analyses for t in an.tokens)
    assert 14000 <= most < 16384, most
