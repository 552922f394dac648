"""engine.py marshals flate_hip_deflate_fast_grouped_framed into the C ABI exactly as the recorded fixture says (no GPU:
the library is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are
tests/engine_trace_grouped.py's).  What tests/test_engine_marshalling.py asks of the methods in FlateEngine's own body is
asked here of the one it inherits from engine.GroupedCalls."""
import inspect
import json
import re

import pytest

from util import flate

import engine_trace
import engine_trace_grouped as gr

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(gr.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(gr.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gr.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = gr.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_inherited_method_has_its_scenarios(recorded):
    assert E.GroupedCalls in E.FlateEngine.__mro__
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.GroupedCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == {"flate_hip_deflate_fast_grouped_framed", "flate_hip_zip_write_last_route"} and named <= reached
    public = [m for m in vars(E.GroupedCalls) if not m.startswith("_") and callable(vars(E.GroupedCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in gr.SCENARIOS}


def test_what_the_recorded_calls_say(recorded):
    """One library call per method call; the tables go in as uint64 / uint32 whatever the caller's dtype; the index is
    asked for only with index=True; device data sets the device-pointer flag; the members' bytes come back cut to
    out_off[-1] on the host."""
    assert "[2,131]" in json.dumps(recorded["zip_write_last_route"]["ret"], separators=(",", ":"))
    assert "[0,0]" in json.dumps(recorded["zip_write_last_route/unchanged_route"]["ret"], separators=(",", ":"))
    assert recorded["zip_write_last_route/raises"]["code"] == E.E_INVALID
    for name, v in recorded.items():
        if name.startswith("zip_write_last_route"):
            continue
        if "out_wrong" in name or "_for_" in name:
            assert v.get("raises") == "FlateError" and v["trace"] == [], name
        else:
            assert len([t for t in v["trace"] if t[0] == "deflate_fast_grouped_framed"]) == 1, name
    host = recorded["deflate_grouped_framed/host"]["trace"][0]
    assert host[2] == {"in_off": gr.IN_OFF, "group_off": gr.GROUP_OFF}
    assert recorded["deflate_grouped_framed/numpy_tables"]["trace"] == recorded["deflate_grouped_framed/host"]["trace"]
    args = dict(zip([a[0] for a in engine_trace.SIGNATURES["flate_hip_deflate_fast_grouped_framed"]], host[1]))
    assert (args["n"], args["n_groups"], args["wrap"], args["bit_off"], args["flags"]) == (3, 2, E.WRAP_ZLIB, "null", 0)
    idx = recorded["deflate_grouped_framed/index"]
    assert idx["trace"][0][1][10] == "ptr" and idx["ret"]["t"][2] == {"<u8": [0, 180, 370, 0, 200]}
    dev = recorded["deflate_grouped_framed/dev"]["trace"][0][1]
    assert dev[-1] == E.DEVICE_PTRS
    assert recorded["deflate_grouped_framed/compat_go"]["trace"][0][1][-1] == E.COMPAT_GO
    assert recorded["deflate_grouped_framed/host"]["ret"]["t"][0] == {"numpy": [80, 80]}
    assert recorded["deflate_grouped_framed/refused"]["code"] == E.E_INVALID
    assert recorded["deflate_grouped_framed/too_small"]["code"] == E.E_OUT_TOO_SMALL
    assert recorded["deflate_grouped_framed/empty"]["ret"]["t"][1] == {"<u8": [0]}
