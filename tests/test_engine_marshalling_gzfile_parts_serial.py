"""What GzFileReader.set_serial_max, GzFileReader.last_route and FlateEngine.open_gzfile_reader(serial_max=...) hand
to the C ABI, without a device: recorded against a library that answers from a script
(tests/engine_trace_gzfile_parts_serial.py) and held against tests/golden/engine_calls_gzfile_parts_serial.json."""
import json

import engine_trace
import engine_trace_gzfile_parts_serial as trace


def test_the_python_reader_hands_the_new_calls_what_the_header_asks_for():
    want = json.load(open(trace.FIXTURE))
    assert list(want) == list(trace.SCENARIOS)
    got = {name: trace.run(name) for name in trace.SCENARIOS}
    for name in trace.SCENARIOS:
        assert got[name] == want[name], name
    names = {c: [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + c]]
             for c in ("gzfile_reader_set_serial_max", "gzfile_reader_last_route")}
    for dev in ("host", "dev"):
        t = got["open/serial_max/" + dev]["trace"]
        assert [c[0] for c in t] == ["gzfile_reader_open", "gzfile_reader_set_serial_max", "gzfile_reader_read",
                                     "gzfile_reader_last_route", "gzfile_reader_free"]
        assert dict(zip(names["gzfile_reader_set_serial_max"], t[1][1]))["serial_max"] == 1 << 20
        assert t[1][1][0] == t[2][1][0] == t[3][1][0]  # the one handle
        assert got["open/serial_max/" + dev]["ret"]["t"][1] == {"t": [2, 1, (1 << 33) + 5]}  # 64 bits of find_from
    # serial_max == 0: no new ABI call at open -- the recorded scenarios of the reader stay valid
    t = got["open/serial_max_0"]["trace"]
    assert [c[0] for c in t] == ["gzfile_reader_open", "gzfile_reader_read", "gzfile_reader_last_route", "gzfile_reader_free"]
    assert got["open/serial_max_0"]["ret"]["t"][1] == {"t": [0, 0, 0]}
    # the setter between open and the first read, and again behind reset
    assert [c[0] for c in got["set/reset/set"]["trace"]] == [
        "gzfile_reader_open", "gzfile_reader_set_serial_max", "gzfile_reader_read", "gzfile_reader_reset",
        "gzfile_reader_set_serial_max", "gzfile_reader_read", "gzfile_reader_last_route", "gzfile_reader_free"]
    assert [c[1][1] for c in got["set/reset/set"]["trace"] if c[0] == "gzfile_reader_set_serial_max"] == [4096, 0]
    # a refusal raises, and the handle is freed all the same
    for name in ("set/raises", "open/serial_max/raises", "last_route/raises"):
        assert got[name]["raises"] == "FlateError" and got[name]["code"] == -1, name
    assert got["set/raises"]["trace"][-1][0] == "gzfile_reader_free"
    assert got["last_route/raises"]["trace"][-1][0] == "gzfile_reader_free"
