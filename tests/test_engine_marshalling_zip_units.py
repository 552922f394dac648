"""engine.py marshals flate_hip_zip_last_route into the C ABI exactly as the recorded fixture says (no GPU: the library
is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are tests/engine_trace_zip_units.py's).
What tests/test_engine_marshalling.py asks of the methods in FlateEngine's own body is asked here of the one it inherits
from engine.ZipUnitsCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_zip_units as zu

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(zu.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(zu.SCENARIOS)


@pytest.mark.parametrize("name", sorted(zu.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = zu.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_inherited_method_has_its_scenarios(recorded):
    assert E.ZipUnitsCalls in E.FlateEngine.__mro__
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.ZipUnitsCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_zip_last_route"} and named <= reached
    public = [m for m in vars(E.ZipUnitsCalls) if not m.startswith("_") and callable(vars(E.ZipUnitsCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in zu.SCENARIOS}


def test_what_the_recorded_calls_say(recorded):
    """One call without a device round trip of its own; the four counts come back as a tuple in the header's order."""
    assert len(recorded["zip_last_route"]["trace"]) == 1
    assert "[3,2,41,97]" in json.dumps(recorded["zip_last_route"]["ret"], separators=(",", ":"))
    assert "[0,0,0,0]" in json.dumps(recorded["zip_last_route/option_off"]["ret"], separators=(",", ":"))
    assert recorded["zip_last_route/raises"]["code"] == E.E_INVALID
