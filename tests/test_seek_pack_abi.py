"""The packed windows' calls on the CPU side: exported, listed and declared with the same arguments, refused without a
ctx before any device is touched with nothing written, and marshalled by engine.py exactly as the recorded fixture says
(no GPU: the library is tests/engine_trace.py's recording stand-in, the scenarios and their fixture are
tests/engine_trace_seek_pack.py's).  The refusals of a bad mode, flag or buffer are api_checks.h's, held on the CPU by
tests/test_seek_pack_rule_model.py and on the GPU, with a ctx, by tests/test_gpu_seek_pack.py."""
import ctypes as C
import inspect
import json
import os
import re
from importlib import import_module

import pytest

from util import flate

import engine_trace
import engine_trace_seek_pack as trace

E = engine_trace.engine
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_seek_windows_pack_bound", "flate_hip_seek_windows_pack", "flate_hip_seek_windows_unpack",
         "flate_hip_inflate_one_ranges_packed")


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return import_module("moonbit-flate_amd._lib").load()


@pytest.fixture(scope="module")
def recorded():
    flate.build()
    with open(trace.FIXTURE) as f:
        return json.load(f)


def declared():
    """{name: number of arguments} of the header's declarations of the four symbols."""
    text = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(flate_hip_(?:seek_windows\w*|inflate_one_ranges_packed))\s*\(([^;]*?)\)\s*;", text, re.S):
        out[m.group(1)] = len(m.group(2).split(","))
    return out


def test_the_exports_equal_the_headers_declarations(lib):
    mod = import_module("moonbit-flate_amd._lib")
    decl = declared()
    assert sorted(decl) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(lib, name) and name in mod.EXPORTS, name
        assert len(mod.SIGNATURES[name][1]) == decl[name], name
    assert [decl[n] for n in NAMES] == [1, 17, 10, 20]
    assert (flate.engine.SEEK_PACK_COMPRESS, flate.engine.SEEK_PACK_SPARSE) == (1, 2)
    text = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    assert re.search(r"#define FLATE_HIP_SEEK_PACK_COMPRESS 1u", text) and re.search(r"#define FLATE_HIP_SEEK_PACK_SPARSE 2u", text)
    for method in ("seek_windows_pack", "seek_windows_unpack", "inflate_one_ranges_packed"):
        assert hasattr(flate.FlateEngine, method), method
    # host only: n_blocks * flate_hip_deflate_bound(32768)
    assert lib.flate_hip_seek_windows_pack_bound(0) == 0
    assert lib.flate_hip_seek_windows_pack_bound(7) == 7 * lib.flate_hip_deflate_bound(32768)


def test_each_refuses_a_null_ctx_before_it_touches_a_device(lib):
    buf = (C.c_uint8 * 4)(3, 0, 0, 0)
    idx = (C.c_uint64 * 32)()
    pk = (C.c_uint64 * 32)(*([9] * 32))
    a, b, c = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    rc = lib.flate_hip_seek_windows_pack(None, buf, 4, 0, idx, 32, None, 0, 3, pk, 32, C.byref(a), buf, 4, C.byref(b), C.byref(c), 0)
    assert rc == -1 and (a.value, b.value, c.value) == (7, 7, 7) and list(pk) == [9] * 32 and list(buf) == [3, 0, 0, 0]
    bad = C.c_uint32(7)
    rc = lib.flate_hip_seek_windows_unpack(None, pk, 32, buf, 4, buf, 4, C.byref(a), C.byref(bad), 0)
    assert rc == -1 and (a.value, bad.value) == (7, 7) and list(buf) == [3, 0, 0, 0]
    lo, hi, off = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(1), (C.c_uint64 * 2)(9, 9)
    rc = lib.flate_hip_inflate_one_ranges_packed(None, buf, 4, 0, idx, 32, pk, 32, None, 0, lo, hi, 1, buf, 4, off, None, None,
                                                 None, 0)
    assert rc == -1 and list(off) == [9, 9]


def test_the_fixture_and_the_scenarios_name_the_same_cases(recorded):
    assert sorted(recorded) == sorted(trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(trace.SCENARIOS))
def test_trace_and_result_are_the_recorded_ones(recorded, name):
    got, want = trace.run(name), recorded[name]
    assert got["trace"] == want["trace"]
    assert got == want


def test_the_device_branch_sets_device_ptrs_and_returns_device_results(recorded):
    seen = 0
    for name, (_, _, device) in trace.SCENARIOS.items():
        if not device or "raises" in recorded[name]:
            continue
        for call, args, *_ in recorded[name]["trace"]:
            names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
            assert args[names.index("flags")] & E.DEVICE_PTRS, (name, call)
            seen += 1
        assert '"numpy"' not in json.dumps(recorded[name]["ret"]), name
    assert seen >= 8
    for method in ("seek_windows_pack", "seek_windows_unpack", "inflate_one_ranges_packed"):
        assert '"tensor"' in json.dumps(recorded[method + "/dev"]["ret"]), method
        assert '"numpy"' in json.dumps(recorded[method + "/host"]["ret"]), method
    # without sparse the stream is not handed over, only its length from the index's head
    call, args = recorded["seek_windows_pack/compress_without_the_stream"]["trace"][0][:2]
    names = [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]
    assert (args[names.index("in")], args[names.index("in_len")], args[names.index("mode")]) == ("null", 200, 1)
    call, args = recorded["seek_windows_pack/host"]["trace"][0][:2]
    assert (args[names.index("in")], args[names.index("mode")], args[names.index("pack_cap_words")]) == ("data", 3, 19)


def test_every_inherited_method_that_calls_the_library_has_a_scenario(recorded):
    assert E.SeekPackCalls in E.FlateEngine.__mro__
    named = set(re.findall(r"_L\.(flate_hip_\w+)", inspect.getsource(E.SeekPackCalls)))
    reached = {"flate_hip_" + t[0] for v in recorded.values() for t in v["trace"]}
    assert named == set(NAMES) and named - {NAMES[0]} <= reached
    public = [m for m in vars(E.SeekPackCalls) if not m.startswith("_") and callable(vars(E.SeekPackCalls)[m])]
    assert set(public) == {s.split("/")[0] for s in trace.SCENARIOS}
