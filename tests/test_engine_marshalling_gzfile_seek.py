"""engine.py marshals the two calls of a gzip file's seek index into the C ABI exactly as the recorded fixture says (no
GPU: the library is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are
tests/engine_trace_gzfile_seek.py's).  What tests/test_engine_marshalling.py asks of the methods in FlateEngine's own
body is asked here of the ones it inherits from engine.GzFileSeekCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_gzfile_seek as gzs

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(gzs.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(gzs.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gzs.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = gzs.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_device_branch_sets_device_ptrs_and_returns_device_results(recorded):
    seen = 0
    for name, (_, _, device) in gzs.SCENARIOS.items():
        if not device or "raises" in recorded[name]:
            continue
        for call, args, *_ in recorded[name]["trace"]:
            names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
            assert args[names.index("flags")] & E.DEVICE_PTRS, (name, call)
            seen += 1
        assert '"numpy"' not in json.dumps(recorded[name]["ret"]), name
    assert seen >= 6
    assert '"tensor"' in json.dumps(recorded["gzfile_seek_index/dev"]["ret"])
    assert '"tensor"' in json.dumps(recorded["gzfile_ranges/dev"]["ret"])
    assert '"numpy"' in json.dumps(recorded["gzfile_seek_index/host"]["ret"])


def test_every_inherited_method_that_calls_the_library_has_a_scenario(recorded):
    assert E.GzFileSeekCalls in E.FlateEngine.__mro__
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.GzFileSeekCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_gzfile_seek_index", "flate_hip_gzfile_ranges"} and named <= reached
    public = [m for m in vars(E.GzFileSeekCalls) if not m.startswith("_") and callable(vars(E.GzFileSeekCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in gzs.SCENARIOS}
    # every status the methods hand back was scripted, and one they do not
    for head in ("gzfile_seek_index", "gzfile_ranges"):
        for rc in (-2, -4, -6, -7):
            assert "raises" not in recorded["%s/status%d" % (head, rc)], (head, rc)
        assert recorded[head + "/raises"]["code"] == E.E_INTERNAL


def test_what_the_recorded_calls_say(recorded):
    """A guess and one retry sized from the counts; a file that fails has no index; the size query first when no
    buffer is given; the index travels as it came."""
    two = recorded["gzfile_seek_index/second_sizing_call"]["trace"]
    names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_gzfile_seek_index"]]
    assert len(two) == 2 and two[1][1][names.index("index_cap_words")] == 300 and two[1][1][names.index("cap")] == 5 * 32768
    assert len(recorded["gzfile_seek_index/host"]["trace"]) == 1
    assert recorded["gzfile_seek_index/span_none"]["trace"][0][1][names.index("cap")] == 0
    failed = recorded["gzfile_seek_index/failing_file"]["ret"]["GzFileSeekIndex"]
    assert failed[0] == E.E_CORRUPT and failed[1] is None and failed[2] is None and failed[9:] == [1, 150, 33]
    again = recorded["gzfile_seek_index/too_small_again"]["ret"]["GzFileSeekIndex"]
    assert again[0] == E.E_OUT_TOO_SMALL and again[1] is None
    rn = [a[0] for a in engine_trace.SIGNATURES["flate_hip_gzfile_ranges"]]
    reads = recorded["gzfile_ranges/host"]["trace"]
    assert len(reads) == 2 and reads[0][1][rn.index("out")] == "null" and reads[0][1][rn.index("cap")] == 0
    assert reads[1][1][rn.index("cap")] == 25 and reads[1][1][rn.index("index_words")] == 31
    assert len(recorded["gzfile_ranges/out"]["trace"]) == 1
    assert recorded["gzfile_ranges/windows_on_the_other_side"]["raises"] == "FlateError"
    assert recorded["gzfile_ranges/seek_index_tuple"]["trace"][0][1][rn.index("windows_bytes")] == 0
