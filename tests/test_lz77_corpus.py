"""The match finder's edge corpus (tests/lz77_corpus.py) without a GPU: every rule the corpus is built for is reached
by its witness, both table modes of the host model (tests/host_model/lz77_wave_model.cpp) give the oracle's tokens on
every case with the modular table never disagreeing with its shadow, and every deliberate fault the model can be
built with (-DLZ_MODEL_MUTANT=k, host model only) changes the tokens of some case -- so the corpus would notice
that fault in the kernel, which tests/test_gpu_lz77_corpus.py compares with the same oracle."""
import pytest

import lz77_corpus as Z
from util import flate, raw_inflate


def test_every_required_rule_is_reached_by_its_witness(oracle):
    by_name = dict(Z.cases())
    assert len(by_name) == len(Z.cases())
    missing = [(r, c) for r, c in sorted(Z.REQUIRED_RULES.items())
               if c not in by_name or r not in Z.facts(oracle, by_name[c])]
    assert not missing, missing


def test_ladder_has_every_distance_phase_and_window():
    names = {n for n, _ in Z.cases()}
    for d in Z.LADDER_D:
        for win in (0, 1, 2):
            for ph in Z.PHASES:
                fits = Z._ladder_geometry(d, ph, win) is not None
                assert ("ladder_d%d_ph%d_w%d" % (d, ph, win) in names) == fits, (d, ph, win)
        assert any(n.startswith("ladder_d%d_" % d) for n in names), d


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_both_model_modes_give_the_oracle_tokens(oracle, go):
    bad, disagree = [], []
    for name, data in Z.cases():
        want = Z.oracle_tokens(oracle, data, go)
        for multi in (False, True):
            for tags in (False, True):
                m = Z.run_model(data, go=go, tags=tags, multi=multi, log=False)
                if not Z.same_tokens(m.tokens, want):
                    bad.append((name, multi, tags))
                if m.stats[Z.S_SHADOW_DISAGREE]:
                    disagree.append((name, multi, tags, int(m.stats[Z.S_SHADOW_DISAGREE])))
    assert not bad, bad[:10]
    assert not disagree, disagree[:10]


def test_every_mutant_is_killed(oracle):
    table = Z.kill_table(oracle)
    print("\nmutant: cases that kill it")
    for k in sorted(table):
        more = " (and %d more)" % (len(table[k]) - 16) if len(table[k]) > 16 else ""
        print("%2d %-62s %3d %s%s" % (k, Z.MUTANTS[k], len(table[k]), " ".join(table[k][:16]), more))
    alive = [k for k in table if not table[k] and k not in Z.EQUIVALENT_MUTANTS]
    assert not alive, [(k, Z.MUTANTS[k]) for k in alive]
    # a mutant listed as equivalent must indeed survive: once a case kills it, it leaves that list
    assert not [k for k in Z.EQUIVALENT_MUTANTS if table[k]]
    wrong = [(k, c) for k, c in sorted(Z.PINNED_KILLERS.items()) if c not in table[k]]
    assert not wrong, wrong


def test_oracle_streams_inflate_with_zlib(oracle):
    for name, data in Z.cases():
        for compat in Z.BOTH:
            assert raw_inflate(oracle.deflate(data, compat=compat)) == data, (name, compat)


def test_chunks_and_tokens_are_the_engines():
    for n in (0, 127, 128, Z.W, Z.W + 127, Z.W + 128, 3 * Z.W):
        assert Z.lz_chunks(n) == flate.lz_chunks(n), n


def test_generation_is_deterministic():
    assert Z._build_cases() == Z.cases()
