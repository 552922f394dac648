"""engine.py marshals the seek index's two calls into the C ABI exactly as the recorded fixture says (no GPU: the
library is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are tests/engine_trace_seek.py's).
What tests/test_engine_marshalling.py asks of the methods in FlateEngine's own body is asked here of the ones it
inherits from engine.OneSeekCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_seek as seek

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(seek.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(seek.SCENARIOS)


@pytest.mark.parametrize("name", sorted(seek.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = seek.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_device_branch_sets_device_ptrs_and_returns_device_results(recorded):
    seen = 0
    for name, (_, _, device) in seek.SCENARIOS.items():
        if not device or "raises" in recorded[name]:
            continue
        for call, args, *_ in recorded[name]["trace"]:
            names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
            assert args[names.index("flags")] & E.DEVICE_PTRS, (name, call)
            seen += 1
        assert '"numpy"' not in json.dumps(recorded[name]["ret"]), name
    assert seen >= 6
    assert '"tensor"' in json.dumps(recorded["inflate_one_seek_index/dev"]["ret"])
    assert '"tensor"' in json.dumps(recorded["inflate_one_ranges/dev"]["ret"])
    assert '"numpy"' in json.dumps(recorded["inflate_one_seek_index/host"]["ret"])


def test_every_inherited_method_that_calls_the_library_has_a_scenario(recorded):
    assert E.FlateEngine.__mro__[1] is E.OneSeekCalls
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.OneSeekCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_inflate_one_seek_index", "flate_hip_inflate_one_ranges"} and named <= reached
    public = [m for m in vars(E.OneSeekCalls) if not m.startswith("_") and callable(vars(E.OneSeekCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in seek.SCENARIOS}
    # every status the methods hand back was scripted, and one they do not
    for head, ok in (("inflate_one_seek_index", (-2, -4, -6, -7)), ("inflate_one_ranges", (-2, -4, -6, -7))):
        for rc in ok:
            assert "raises" not in recorded["%s/status%d" % (head, rc)], (head, rc)
        assert recorded[head + "/raises"]["code"] == E.E_INTERNAL
