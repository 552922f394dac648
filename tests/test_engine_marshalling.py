"""engine.py marshals every call into the C ABI exactly as the recorded fixture says (no GPU: the library is a
recording stand-in, tests/engine_trace.py).  tests/golden/engine_calls.json was recorded from the wrapper before its
methods were rebuilt on shared helpers; a difference here is a change of behaviour, not a reason to record again."""
import importlib
import inspect
import json

import pytest

from util import flate

import engine_trace

E = engine_trace.engine


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(engine_trace.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(engine_trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(engine_trace.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = engine_trace.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def _nodes(x):
    yield x
    for v in (x.values() if isinstance(x, dict) else x if isinstance(x, list) else ()):
        yield from _nodes(v)


def test_the_device_branch_sets_device_ptrs_and_returns_device_results(recorded):
    """Every call of a scenario whose data is a (stand-in) CUDA tensor carries FLATE_HIP_DEVICE_PTRS, and what comes
    back is in device form: a tensor where the host form has an array, and no bytes."""
    seen = 0
    for name, (_, _, device) in engine_trace.SCENARIOS.items():
        if not device or "raises" in recorded[name]:
            continue
        for call, args, *_ in recorded[name]["trace"]:
            names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
            assert args[names.index("flags")] & E.DEVICE_PTRS, (name, call)
            seen += 1
        ret = recorded[name]["ret"]
        nodes = [n for n in _nodes(ret) if isinstance(n, dict)]
        assert not any("numpy" in n for n in nodes), name
        assert not any("bytes" in n for n in [ret] + (ret["t"] if isinstance(ret, dict) and "t" in ret else [])
                       if isinstance(n, dict)), name
        host = recorded.get(name[:-len("/dev")] if name.endswith("/dev") else name + "/host")
        if host and any("numpy" in n or "bytes" in n for n in _nodes(host.get("ret")) if isinstance(n, dict)):
            assert any("tensor" in n for n in nodes), name
    assert seen > 40


def test_every_public_method_that_calls_the_library_has_a_scenario():
    """A method of FlateEngine, StreamWriter or StreamReader that names self._L must be driven by some scenario: the
    entry points the scenarios reached cover the ones the classes' source names."""
    import re
    named = set()
    for cls in (E.FlateEngine, E.StreamWriter, E.StreamReader):
        named |= set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(cls)))
    named -= set(engine_trace.PASS_THROUGH) | {"flate_hip_init"}
    with open(engine_trace.FIXTURE) as f:
        reached = {"flate_hip_" + t[0] for v in json.load(f).values() for t in v["trace"]}
    assert named and named <= reached, sorted(named - reached)
    public = [m for cls in (E.FlateEngine, E.StreamWriter, E.StreamReader) for m in vars(cls)
              if not m.startswith("_") and callable(vars(cls)[m])]
    heads = {s.split("/")[0] for s in engine_trace.SCENARIOS}
    driven = heads | {"open_stream", "open_inflate_stream", "write", "close", "free", "feed", "reset"}  # the stream_* cases
    assert set(public) <= driven, sorted(set(public) - driven)


def test_exports_are_the_tables_keys():
    """_lib.EXPORTS lists what the signature table declares, and every int-returning function says so."""
    import ctypes as C
    flate.build()
    lib_mod = importlib.import_module("moonbit-flate_amd._lib")
    L = lib_mod.load()
    for name in lib_mod.EXPORTS:
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
    table = getattr(lib_mod, "SIGNATURES", None)
    if table is not None:
        assert list(table) == list(lib_mod.EXPORTS)
        for name, (restype, _) in table.items():
            assert getattr(L, name).restype is restype, name
        import os
        import re
        hdr = open(os.path.join(engine_trace.ROOT, "include", "flate_hip.h")).read()
        void = set(re.findall(r"^void (flate_hip_\w+)\(", hdr, re.M))
        assert void and void == {name for name, (restype, _) in table.items() if restype is None}
    assert L.flate_hip_set_option.restype is C.c_int
