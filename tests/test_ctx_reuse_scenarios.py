"""The scenario table of tests/ctx_reuse_scenarios.py on the CPU: every expectation is consistent with what zlib,
gzip and zipfile read out of the scenario's own input, every dirty twin really is poison for its X (same counts, another
size and offset at every index, another verdict where the call has one), every big twin leaves stale words behind X's
arrays, and the seeded walks hold what the GPU test relies on.  These are conditions on the INPUTS: a failure here means
the input has to change, not the check."""
import pytest

import ctx_reuse_scenarios as sc


@pytest.fixture(scope="module", autouse=True)
def bound(oracle):
    sc.bind(oracle)


FAMILY_NAMES = sorted(sc.FAMILIES)


def test_every_family_has_its_three_scenarios_and_every_read_family_its_failures():
    for name, f in sc.FAMILIES.items():
        assert {"X", "dirty", "big"} <= set(f), name
    want = {(f, c) for f in sc.READ_FAMILIES for c in sc.READ_CLASSES} | \
        {(f, c) for f in sc.INDEX_FAMILIES for c in sc.INDEX_CLASSES}
    have = {(name, c) for name, f in sc.FAMILIES.items() for c in f["fail"]}
    assert not set(sc.IMPOSSIBLE) & have, "a class listed as impossible has a scenario"
    assert set(sc.IMPOSSIBLE) <= want
    missing = want - have - set(sc.IMPOSSIBLE)
    assert not missing, sorted(missing)
    assert set(sc.READ_FAMILIES) | set(sc.INDEX_FAMILIES) == {f for f in sc.FAMILIES if f.startswith(
        ("inflate", "bgzf_r", "bgzf_i", "gzip", "seek", "gzfile", "zip_r", "zip_i"))}
    assert {s.fail for s in sc.FAILS} == set(sc.FAIL_CLASSES)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_expected_is_what_the_standard_readers_make_of_the_input(family):
    f = sc.FAMILIES[family]
    for s in [f["X"], f["dirty"], f["big"]] + f["more"] + list(f["fail"].values()):
        d = s.data
        assert isinstance(d["expected"], tuple) and isinstance(d["expected"][0], int), s
        if d["proof"] is None:
            continue   # (token lists: no standard reader states them)
        for got, want in d["proof"]:
            assert got == want, s
        if s.role in ("X", "big", "more") and not s.fail:
            assert d["proof"], s
        if s.fail:
            assert d["expected"][0] != 0, s


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_dirty_twin_differs_at_every_index(family):
    x, y = sc.FAMILIES[family]["X"].data["meta"], sc.FAMILIES[family]["dirty"].data["meta"]
    assert x["counts"] == y["counts"], family
    for a, b in zip(x["sizes"] + x["offs"], y["sizes"] + y["offs"]):
        assert len(a) == len(b) and len(a) > 0, family
        same = [i for i, (u, v) in enumerate(zip(a, b)) if u == v]
        assert not same, (family, same, a, b)
    if family in sc.NO_STATUS:
        assert x["status"] is None and y["status"] is None, family
    else:
        assert x["status"] != y["status"] and len(x["status"]) == len(y["status"]), (family, x["status"], y["status"])
    assert sc.FAMILIES[family]["X"].expected != sc.FAMILIES[family]["dirty"].expected


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_big_twin_has_three_times_the_counts(family):
    x, y = sc.FAMILIES[family]["X"].data["meta"], sc.FAMILIES[family]["big"].data["meta"]
    assert len(x["counts"]) == len(y["counts"])
    for a, b in zip(x["counts"], y["counts"]):
        assert b >= 3 * a, (family, x["counts"], y["counts"])


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_a_walk_meets_every_scenario_and_every_kind_of_step(seed):
    steps = sc.walk(seed)
    assert steps == sc.walk(seed)
    calls = [s for s in steps if s[0] == "call"]
    assert len(calls) >= sc.WALK_LEN and {s[1] for s in calls} == set(sc.BY_NAME)
    assert any(not a[2] and b[2] for a, b in zip(calls, calls[1:])), "no host -> device switch"
    after_failure = [(sc.BY_NAME[a[1]], sc.BY_NAME[b[1]]) for a, b in zip(calls, calls[1:])]
    assert any(a.fail and not b.fail and a.family != b.family for a, b in after_failure)
    options = [s for s in steps if s[0] == "option"]
    assert [s[1:] for s in options] == sc.OPTION_STEPS
    last = {}
    for _, name, value in options:
        last[name] = value
    assert {k: v for k, v in last.items() if k != "inflate_config"} == sc.OPTION_DEFAULTS, \
        "a walk leaves the options it can restore as it found them"
    assert [s[1] for s in options if s[1] == "inflate_config"] == [s[1] for s in options[-2:]], "the decoder configurations last"
    # every value of every option is in force while at least one scenario that reads it runs
    for k, step in enumerate(steps):
        if step[0] != "option":
            continue
        until = next((j for j in range(k + 1, len(steps)) if steps[j][0] == "option" and steps[j][1] == step[1]), len(steps))
        ran = {s[1] for s in steps[k + 1:until] if s[0] == "call"}
        assert set(sc.OPTION_READERS[step[1]]) <= ran, (step, sorted(set(sc.OPTION_READERS[step[1]]) - ran))
    for name, readers in sc.OPTION_READERS.items():
        assert all(r in sc.BY_NAME for r in readers), name
