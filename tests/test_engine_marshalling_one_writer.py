"""FlateEngine.open_one_writer / engine.OneWriter without a GPU: what engine.py hands to flate_hip_one_writer_* --
recorded against a library that answers from a script (tests/engine_trace_one_writer.py) and held against
tests/golden/engine_calls_one_writer.json: host and device, the index on and off, the FLATE_HIP_E_OUT_TOO_SMALL retry."""
import json

import engine_trace
import engine_trace_one_writer as trace
from util import flate

E = engine_trace.engine


def names(call):
    return [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]


def test_the_python_writer_hands_the_calls_what_the_header_asks_for():
    want = json.load(open(trace.FIXTURE))
    assert list(want) == list(trace.SCENARIOS)
    got = {name: trace.run(name) for name in trace.SCENARIOS}
    for name in trace.SCENARIOS:
        assert got[name] == want[name], name


def test_the_side_the_piece_and_the_flags_are_fixed_at_open():
    for dev, flags in (("host", 0), ("dev", E.DEVICE_PTRS)):
        t = trace.run("write/zlib/final/index/" + dev)["trace"]
        assert [c[0] for c in t] == ["one_writer_open", "one_writer_write", "one_writer_free"]
        opened = dict(zip(names("one_writer_open"), t[0][1]))
        assert (opened["wrap"], opened["piece_bytes"], opened["flags"]) == (1, 50, flags)
        w = dict(zip(names("one_writer_write"), t[1][1]))
        assert (w["in"], w["in_len"], w["final"], w["bit_off"]) == ("data", 200, 1, "ptr")
        assert w["cap"] == 200 + 200 // 8 + 4096  # the part and an eighth
    opened = dict(zip(names("one_writer_open"), trace.run("write/compat_go/dev")["trace"][0][1]))
    assert opened["flags"] == E.DEVICE_PTRS | E.COMPAT_GO


def test_the_index_is_asked_for_only_where_it_is_wanted():
    for dev in ("host", "dev"):
        off = dict(zip(names("one_writer_write"), trace.run("write/" + dev)["trace"][1][1]))
        on = dict(zip(names("one_writer_write"), trace.run("write/index/" + dev)["trace"][1][1]))
        assert (off["bit_off"], on["bit_off"]) == ("null", "ptr")
        assert trace.run("write/" + dev)["ret"]["t"][2] == {"OnePartWrite": [0, 90, 4, None]}
        # k entries for a call that is not final, one more -- the end bit -- for a final one
        assert trace.run("write/index/" + dev)["ret"]["t"][2] == {"OnePartWrite": [0, 90, 4, {"<u8": [0, 170, 340, 511]}]}
        assert trace.run("write/zlib/final/index/" + dev)["ret"]["t"][2] == {
            "OnePartWrite": [1, 90, 4, {"<u8": [0, 170, 340, 511, 700]}]}


def test_a_call_that_does_not_fit_is_repeated_once_with_the_reported_size():
    for dev in ("host", "dev"):
        got = trace.run("write/second_sizing_call/" + dev)
        caps = [dict(zip(names("one_writer_write"), c[1]))["cap"] for c in got["trace"][1:3]]
        assert caps == [4321, 5000]
        assert got["ret"]["t"][0] == 200 and got["ret"]["t"][2]["OnePartWrite"][:3] == [0, 5000, 4]
    # ... but not when the caller set the capacity: the status comes back with the bytes needed and no bytes
    got = trace.run("write/too_small_with_out_cap")
    assert len(got["trace"]) == 3 and got["ret"]["t"] == [0, {"numpy": [0, 0]}, {"OnePartWrite": [-2, 5000, 0, None]}]


def test_statuses_buffers_and_the_handle():
    assert trace.run("write/raises")["raises"] == "FlateError" and trace.run("write/raises")["code"] == -8
    assert trace.run("write/too_large_raises")["code"] == -6
    assert trace.run("write/raises")["trace"][-1][0] == "one_writer_free"  # the handle is freed all the same
    assert trace.run("write/wrong_side")["raises"] == "FlateError" and len(trace.run("write/wrong_side")["trace"]) == 2
    # an empty part, or none, goes in as NULL with length 0; the caller's buffer and capacity as they are
    assert trace.run("write/empty_final")["trace"][1][1][1:4] == ["null", 0, 1]
    assert trace.run("write/none_final")["trace"][1][1][1:4] == ["null", 0, 1]
    assert trace.run("write/empty_final")["ret"]["t"][2] == {"OnePartWrite": [1, 5, 0, {"<u8": [0]}]}
    w = dict(zip(names("one_writer_write"), trace.run("write/out_and_out_cap")["trace"][1][1]))
    assert (w["out"], w["cap"]) == ("out", 95)
    assert [c[0] for c in trace.run("reset_and_a_second_stream")["trace"]] == [
        "one_writer_open", "one_writer_write", "one_writer_reset", "one_writer_write", "one_writer_free"]
    assert callable(flate.FlateEngine.open_one_writer)
