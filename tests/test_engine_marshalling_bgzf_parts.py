"""What FlateEngine.open_bgzf_reader / open_bgzf_writer hand to the C ABI, without a device: recorded against a library
that answers from a script (tests/engine_trace_bgzf_parts.py) and held against
tests/golden/engine_calls_bgzf_parts.json."""
import json

import engine_trace
import engine_trace_bgzf_parts as trace

E = engine_trace.engine


def names(call):
    return [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + call]]


def args(name, call, k=1):
    return dict(zip(names(call), trace.run(name)["trace"][k][1]))


def test_the_python_classes_hand_the_calls_what_the_header_asks_for():
    want = json.load(open(trace.FIXTURE))
    assert list(want) == list(trace.SCENARIOS)
    for name in trace.SCENARIOS:
        assert trace.run(name) == want[name], name


def test_the_reader():
    for dev, flags in (("host", 0), ("dev", E.DEVICE_PTRS)):
        t = trace.run("read/final/index/" + dev)["trace"]
        assert [c[0] for c in t] == ["bgzf_reader_open", "bgzf_reader_read", "bgzf_reader_free"]
        assert dict(zip(names("bgzf_reader_open"), t[0][1]))["flags"] == flags  # the side is fixed at open
        r = args("read/final/index/" + dev, "bgzf_reader_read")
        assert (r["in"], r["in_len"], r["final"], r["cap"]) == ("data", 200, 1, 65536)  # four times the part, 64 KiB at least
        # the index: HOST arrays on either side, room for every member 200 bytes can hold and one entry more
        assert (r["index_cap"], r["member_off"], r["out_off"]) == (200 // 28 + 2, "ptr", "ptr")
        off = args("read/" + dev, "bgzf_reader_read")
        assert (off["index_cap"], off["member_off"], off["out_off"]) == (0, "null", "null")
        assert args("read/index_cap/" + dev, "bgzf_reader_read")["index_cap"] == 2
        # a first member that does not fit: one more call with exactly the room it asked for
        t = trace.run("read/second_sizing_call/" + dev)["trace"]
        assert [dict(zip(names("bgzf_reader_read"), c[1]))["cap"] for c in t[1:3]] == [65536, 5000]
    res = trace.run("read/final/index/host")["ret"]["t"]
    assert res[0] == 200 and res[2] == {"BgzfPartRead": [1, 25, 2, 0xffffffff, -1, 1, {"<u8": [1000, 1070, 1150]}, {"<u8": [500, 510, 525]}]}
    # ... but not when the caller set the capacity, and not for the sticky -2, which names its member and keeps its bytes
    assert trace.run("read/too_small_with_out_cap")["ret"]["t"][1:] == [
        {"numpy": [0, 0]}, {"BgzfPartRead": [-2, 5000, 0, 0xffffffff, -1, 0, None, None]}]
    got = trace.run("read/sticky_too_small")
    assert len(got["trace"]) == 3 and got["ret"]["t"][1:] == [{"numpy": [25, 25]}, {"BgzfPartRead": [-2, 25, 2, 7, 4321, 1, None, None]}]
    # the file's errors come back with their words and the bytes in front; anything else raises, the handle freed all the same
    for rc in (-4, -7, -6, -10):
        assert trace.run("read/status%d" % rc)["ret"]["t"][2]["BgzfPartRead"][:6] == [rc, 25, 2, 5, 1234, 1]
    got = trace.run("read/raises")
    assert got["raises"] == "FlateError" and got["code"] == -8 and got["trace"][-1][0] == "bgzf_reader_free"
    assert trace.run("read/wrong_side")["raises"] == "FlateError" and len(trace.run("read/wrong_side")["trace"]) == 2
    assert trace.run("read/empty_part")["trace"][1][1][1:3] == ["null", 0]
    assert [c[0] for c in trace.run("read/reset_and_a_second_file")["trace"]] == [
        "bgzf_reader_open", "bgzf_reader_read", "bgzf_reader_reset", "bgzf_reader_read", "bgzf_reader_free"]


def test_the_writer():
    for dev, flags in (("host", 0), ("dev", E.DEVICE_PTRS)):
        t = trace.run("write/final/index/" + dev)["trace"]
        assert [c[0] for c in t] == ["bgzf_writer_open", "bgzf_writer_write", "bgzf_writer_free"]
        opened = dict(zip(names("bgzf_writer_open"), t[0][1]))
        assert (opened["block_bytes"], opened["flags"]) == (50, flags)
        w = dict(zip(names("bgzf_writer_write"), t[1][1]))
        assert (w["in"], w["in_len"], w["final"], w["member_off"]) == ("data", 200, 1, "ptr")
        assert w["cap"] == E.bgzf_writer_bound(200, 50)
        assert args("write/" + dev, "bgzf_writer_write")["member_off"] == "null"
        assert trace.run("write/" + dev)["ret"]["t"][2] == {"BgzfPartWrite": [0, 90, 4, None]}
        assert trace.run("write/index/" + dev)["ret"]["t"][2] == {"BgzfPartWrite": [0, 90, 4, {"<u8": [300, 320, 345, 365, 390]}]}
    assert dict(zip(names("bgzf_writer_open"), trace.run("write/compat_go/dev")["trace"][0][1]))["flags"] == E.DEVICE_PTRS | E.COMPAT_GO
    assert dict(zip(names("bgzf_writer_open"), trace.run("write/default_block")["trace"][0][1]))["block_bytes"] == 0
    # too little room and a block BSIZE cannot express come back as statuses: one call, no bytes
    assert trace.run("write/too_small")["ret"]["t"] == [0, {"numpy": [0, 0]}, {"BgzfPartWrite": [-2, 0, 0, None]}]
    assert trace.run("write/too_large")["ret"]["t"][2] == {"BgzfPartWrite": [-6, 0, 0, None]}
    assert trace.run("write/raises")["raises"] == "FlateError" and trace.run("write/open_raises")["code"] == -1
    # a final write of nothing: NULL and 0 in, the marker out
    w = args("write/none_final", "bgzf_writer_write")
    assert (w["in"], w["in_len"], w["final"]) == ("null", 0, 1)
    assert [c[0] for c in trace.run("write/reset_and_a_second_file")["trace"]] == [
        "bgzf_writer_open", "bgzf_writer_write", "bgzf_writer_reset", "bgzf_writer_write", "bgzf_writer_free"]
