"""engine.py marshals the two gzfile calls into the C ABI exactly as the recorded fixture says (no GPU: the library is
tests/engine_trace.py's recording stand-in, the scenarios and their fixture are tests/engine_trace_gzfile.py's).  What
tests/test_engine_marshalling.py asks of the methods in FlateEngine's own body is asked here of the ones it inherits
from engine.GzFileCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_gzfile as gzf

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(gzf.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(gzf.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gzf.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = gzf.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_device_branch_sets_device_ptrs_and_returns_device_results(recorded):
    seen = 0
    for name, (_, _, device) in gzf.SCENARIOS.items():
        if not device or "raises" in recorded[name]:
            continue
        for call, args, *_ in recorded[name]["trace"]:
            names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
            assert args[names.index("flags")] & E.DEVICE_PTRS, (name, call)
            seen += 1
        assert '"numpy"' not in json.dumps(recorded[name]["ret"]), name
    assert seen >= 6
    assert '"tensor"' in json.dumps(recorded["gzfile_read/dev"]["ret"])
    assert '"numpy"' in json.dumps(recorded["gzfile_read/host"]["ret"])


def test_every_inherited_method_that_calls_the_library_has_a_scenario(recorded):
    assert E.GzFileCalls in E.FlateEngine.__mro__
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.GzFileCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_gzfile_index", "flate_hip_gzfile_read"} and named <= reached
    public = [m for m in vars(E.GzFileCalls) if not m.startswith("_") and callable(vars(E.GzFileCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in gzf.SCENARIOS}


def test_what_the_recorded_calls_say(recorded):
    """A guess and one retry sized from the counts; the size query first when no buffer is given; a pair that is too
    small comes back as None beside the other pair."""
    two = recorded["gzfile_index/second_sizing_call"]
    assert len(two["trace"]) == 2 and two["trace"][1][1][3] == 100 and two["trace"][1][1][6] == 81
    assert len(recorded["gzfile_index/host"]["trace"]) == 1 and len(recorded["gzfile_index/query"]["trace"]) == 1
    short = recorded["gzfile_index/index_cap_too_small"]["ret"]["GzFileIndex"]
    assert short[0] == E.E_OUT_TOO_SMALL and short[9] is None and short[10] is None and short[11] is not None
    reads = recorded["gzfile_read/host"]["trace"]
    assert len(reads) == 2 and reads[0][1][3:5] == ["null", 0] and reads[1][1][4] == 25
    assert len(recorded["gzfile_read/out"]["trace"]) == 1
    assert recorded["gzfile_read/raises"]["raises"] == "FlateError"
