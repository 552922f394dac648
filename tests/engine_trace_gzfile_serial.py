"""What engine.py hands to the C ABI for flate_hip_gzfile_last_route, recorded without a device
(tests/test_engine_marshalling_gzfile_serial.py): the machinery is tests/engine_trace.py's -- its recording library, its
Env and its serialiser -- with the entry point's signature added to its table and the scenarios of
engine.GzFileSerialCalls kept HERE, in a table and a fixture of their own
(tests/golden/engine_calls_gzfile_serial.json), so that the recording of the methods that were there before stays what
it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_gzfile_serial.json")

et.SIGNATURES.setdefault("flate_hip_gzfile_last_route", et._parse(
    "ctx serial_members:u32[1]> unit_members:u32[1]> find_from:u64[1]>"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


add("gzfile_last_route", lambda e: e.eng.gzfile_last_route(),
    {"gzfile_last_route": [{"serial_members": 6, "unit_members": 2, "find_from": (1 << 33) + 5}]})
add("gzfile_last_route/option_off", lambda e: e.eng.gzfile_last_route(), {"gzfile_last_route": [{}]})
add("gzfile_last_route/raises", lambda e: e.eng.gzfile_last_route(), {"gzfile_last_route": [{"rc": E.E_INVALID}]})


def run(name):
    fn, script, device = SCENARIOS[name]
    env = et.Env(script, device)
    try:
        res = {"ret": et.serialise(fn(env), env.lib)}
    except E.FlateError as e:
        res = {"raises": "FlateError", "code": e.code, "msg": str(e)}
    res = json.loads(json.dumps({"trace": env.lib.trace, **res}))
    env.eng._ctx = None  # nothing to destroy
    return res


if __name__ == "__main__":
    got = {name: run(name) for name in SCENARIOS}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in got.items()) + "\n}\n")
    print("%d scenarios, %d calls -> %s" % (len(got), sum(len(v["trace"]) for v in got.values()), FIXTURE))
