"""What engine.py hands to the C ABI for GzFileReader.set_serial_max, GzFileReader.last_route and
FlateEngine.open_gzfile_reader(serial_max=...), recorded without a device
(tests/test_engine_marshalling_gzfile_parts_serial.py): the machinery is tests/engine_trace.py's, the reader's four
signatures are tests/engine_trace_gzfile_parts.py's, and the two new entry points' signatures and scenarios are kept
HERE, in a table and a fixture of their own (tests/golden/engine_calls_gzfile_parts_serial.json).

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et
import engine_trace_gzfile_parts  # noqa: F401  (the reader's signatures)

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_gzfile_parts_serial.json")

et.SIGNATURES.setdefault("flate_hip_gzfile_reader_set_serial_max", et._parse("stream serial_max"))
et.SIGNATURES.setdefault("flate_hip_gzfile_reader_last_route", et._parse(
    "stream serial_members:u32[1]> open_stop:u32[1]> find_from:u64[1]>"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def build_scenarios():
    done = {"in_used": 150, "out": 25, "out_len": 25, "n_members": 2, "n_units": 2}
    route = {"serial_members": 2, "open_stop": 1, "find_from": (1 << 33) + 5}

    def opened_with(serial_max):
        def fn(e):
            rd = e.eng.open_gzfile_reader(device=e.device, serial_max=serial_max)
            try:
                return rd.read(e.data()), rd.last_route()
            finally:
                rd.close()
        return fn
    for dev in (False, True):
        tag = "/dev" if dev else "/host"
        add("open/serial_max" + tag, opened_with(1 << 20),
            {"gzfile_reader_read": [done], "gzfile_reader_last_route": [route]}, device=dev)
    # serial_max == 0 makes no new call: the trace of the reader as it was, and then the route of S = 0
    add("open/serial_max_0", opened_with(0), {"gzfile_reader_read": [done], "gzfile_reader_last_route": [{}]})

    def set_then_reset(e):
        rd = e.eng.open_gzfile_reader()
        rd.set_serial_max(4096)
        a = rd.read(e.data())
        rd.reset()
        rd.set_serial_max(0)
        b = rd.read(e.data(120), final=True)
        r = rd.last_route()
        rd.close()
        return a, b, r
    add("set/reset/set", set_then_reset,
        {"gzfile_reader_read": [done, dict(done, rc=1, in_used=120)], "gzfile_reader_last_route": [{}]})

    def refused(e):
        rd = e.eng.open_gzfile_reader()
        try:
            rd.set_serial_max(1 << 28)
        finally:
            rd.close()
    add("set/raises", refused, {"gzfile_reader_set_serial_max": [{"rc": E.E_INVALID}]})
    add("open/serial_max/raises", opened_with(7), {"gzfile_reader_set_serial_max": [{"rc": E.E_INVALID}]})

    def route_refused(e):
        rd = e.eng.open_gzfile_reader()
        try:
            return rd.last_route()
        finally:
            rd.close()
    add("last_route/raises", route_refused, {"gzfile_reader_last_route": [{"rc": E.E_INVALID}]})


build_scenarios()


def run(name):
    fn, script, device = SCENARIOS[name]
    env = et.Env(script, device)
    try:
        res = {"ret": et.serialise(fn(env), env.lib)}
    except E.FlateError as e:
        res = {"raises": "FlateError", "code": e.code, "msg": str(e)}
    except (ValueError, KeyError, AssertionError) as e:
        res = {"raises": type(e).__name__, "msg": "" if isinstance(e, AssertionError) else str(e)}
    res = json.loads(json.dumps({"trace": env.lib.trace, **res}))
    env.eng._ctx = None  # nothing to destroy
    return res


if __name__ == "__main__":
    got = {name: run(name) for name in SCENARIOS}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in got.items()) + "\n}\n")
    print("%d scenarios, %d calls -> %s" % (len(got), sum(len(v["trace"]) for v in got.values()), FIXTURE))
