"""What FlateEngine.open_gzfile_reader hands to the C ABI, without a device: recorded against a library that answers
from a script (tests/engine_trace_gzfile_parts.py) and held against tests/golden/engine_calls_gzfile_parts.json."""
import json

import engine_trace
import engine_trace_gzfile_parts as trace
from util import flate


def test_the_python_reader_hands_the_calls_what_the_header_asks_for():
    want = json.load(open(trace.FIXTURE))
    assert list(want) == list(trace.SCENARIOS)
    got = {name: trace.run(name) for name in trace.SCENARIOS}
    for name in trace.SCENARIOS:
        assert got[name] == want[name], name
    names = {c: [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + c]] for c in ("gzfile_reader_open", "gzfile_reader_read")}
    for dev, flags in (("host", 0), ("dev", flate.DEVICE_PTRS if hasattr(flate, "DEVICE_PTRS") else 1)):
        t = got["read/final/" + dev]["trace"]
        assert [c[0] for c in t] == ["gzfile_reader_open", "gzfile_reader_read", "gzfile_reader_free"]
        opened = dict(zip(names["gzfile_reader_open"], t[0][1]))
        assert opened["flags"] == flags  # the side is fixed at open
        read = dict(zip(names["gzfile_reader_read"], t[1][1]))
        assert (read["in"], read["in_len"], read["final"]) == ("data", 200, 1)
        assert read["cap"] == 65536  # four times the part, 64 KiB at least
    # a first unit that does not fit: one more call with exactly the room it asked for
    t = got["read/second_sizing_call/host"]["trace"]
    assert [dict(zip(names["gzfile_reader_read"], c[1]))["cap"] for c in t[1:3]] == [65536, 5000]
    # ... but not when the caller set the capacity; the statuses come back with the file's words, anything else raises
    assert got["read/too_small_with_out_cap"]["ret"]["t"][2] == {"GzFilePartRead": [-2, 5000, 0, 0, 0xffffffff, -1, -1]}
    assert got["read/status-4"]["ret"]["t"][2] == {"GzFilePartRead": [-4, 25, 2, 3, 5, 1234, 77]}
    assert got["read/status-7"]["ret"]["t"][2] == {"GzFilePartRead": [-7, 25, 2, 3, 5, 1234, -1]}
    assert got["read/raises"]["raises"] == "FlateError" and got["read/raises"]["code"] == -8
    assert got["read/raises"]["trace"][-1][0] == "gzfile_reader_free"  # the handle is freed all the same
    assert got["read/wrong_side"]["raises"] == "FlateError" and len(got["read/wrong_side"]["trace"]) == 2
    # an empty part goes in as NULL with length 0 (an empty file: the end); reset between two files; freed once
    assert got["read/empty_part"]["trace"][1][1][1:3] == ["null", 0]
    assert got["read/empty_part"]["ret"]["t"][2]["GzFilePartRead"][0] == 1
    assert [c[0] for c in got["reset_and_a_second_file"]["trace"]] == [
        "gzfile_reader_open", "gzfile_reader_read", "gzfile_reader_reset", "gzfile_reader_read", "gzfile_reader_free"]
