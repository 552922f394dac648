"""engine.py marshals flate_hip_gzfile_last_route into the C ABI exactly as the recorded fixture says (no GPU: the
library is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are
tests/engine_trace_gzfile_serial.py's).  What tests/test_engine_marshalling.py asks of the methods in FlateEngine's own
body is asked here of the one it inherits from engine.GzFileSerialCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_gzfile_serial as gs

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(gs.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(gs.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gs.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = gs.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_inherited_method_has_its_scenarios(recorded):
    assert E.GzFileSerialCalls in E.FlateEngine.__mro__ and callable(E.FlateEngine.gzfile_last_route)
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.GzFileSerialCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_gzfile_last_route"} and named <= reached
    public = [m for m in vars(E.GzFileSerialCalls) if not m.startswith("_") and callable(vars(E.GzFileSerialCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in gs.SCENARIOS}


def test_what_the_recorded_calls_say(recorded):
    """One call without a device round trip of its own; the three words come back as a tuple in the header's order, the
    64-bit offset whole."""
    assert len(recorded["gzfile_last_route"]["trace"]) == 1
    assert "[6,2,%d]" % ((1 << 33) + 5) in json.dumps(recorded["gzfile_last_route"]["ret"], separators=(",", ":"))
    assert "[0,0,0]" in json.dumps(recorded["gzfile_last_route/option_off"]["ret"], separators=(",", ":"))
    assert recorded["gzfile_last_route/raises"]["code"] == E.E_INVALID
