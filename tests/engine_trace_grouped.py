"""What engine.py hands to the C ABI for flate_hip_deflate_fast_grouped_framed, recorded without a device
(tests/test_engine_marshalling_grouped.py): the machinery is tests/engine_trace.py's -- its recording library, its Env
and its serialiser -- with the entry point's signature added to its table and the scenarios of engine.GroupedCalls kept
HERE, in a table and a fixture of their own (tests/golden/engine_calls_grouped.json), so that the recording of the
methods that were there before stays what it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import numpy as np

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_grouped.json")
IN_OFF = et.IN_OFF          # three pieces over 200 bytes ...
GROUP_OFF = [0, 2, 3]       # ... in two groups

et.SIGNATURES.setdefault("flate_hip_deflate_fast_grouped_framed", et._parse(
    "ctx in in_off:u64[n+1]< n group_off:u32[n_groups+1]< n_groups wrap out cap out_off:u64[n_groups+1]> "
    "bit_off:u64[n+n_groups]> flags"))

et.SIGNATURES.setdefault("flate_hip_zip_write_last_route", et._parse("ctx long_entries:u32[1]> n_pieces:u32[1]>"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)
ENTRY = "deflate_fast_grouped_framed"
ANSWER = {ENTRY: [{"out": 80, "out_off": [0, 50, 80], "bit_off": [0, 180, 370, 0, 200]}]}


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, ANSWER if script is None else script, device)


def call(e, d, wrap="zlib", **k):
    return e.eng.deflate_grouped_framed(d, IN_OFF, GROUP_OFF, wrap, **k)


P = "deflate_grouped_framed"
add(P + "/host", lambda e: call(e, e.data()))
add(P + "/dev", lambda e: call(e, e.data()), device=True)
add(P + "/gzip", lambda e: call(e, e.data(), "gzip"))
add(P + "/raw", lambda e: call(e, e.data(), "raw"))
add(P + "/compat_go", lambda e: call(e, e.data(), compat_go=True))
add(P + "/index", lambda e: call(e, e.data(), index=True))
add(P + "/index/dev", lambda e: call(e, e.data(), "gzip", index=True), device=True)
add(P + "/numpy_tables", lambda e: e.eng.deflate_grouped_framed(e.data(), np.array(IN_OFF, np.int64),
                                                                np.array(GROUP_OFF, np.int64), "zlib"))
add(P + "/raises", lambda e: call(e, e.data()), et.with_rc(ANSWER, et.BAD, ENTRY))
add(P + "/refused", lambda e: e.eng.deflate_grouped_framed(e.data(), IN_OFF, [0, 2, 2, 3], "zlib"),
    et.with_rc(ANSWER, E.E_INVALID, ENTRY))
add(P + "/too_small", lambda e: call(e, e.data(), out_cap=9), et.with_rc(ANSWER, E.E_OUT_TOO_SMALL, ENTRY))
add(P + "/empty", lambda e: e.eng.deflate_grouped_framed(e.data(0), [0], [0], "zlib", index=True),
    {ENTRY: [{"out_off": [0]}]})
for dev in (False, True):
    add(P + "/out" + ("/dev" if dev else ""), lambda e: call(e, e.data(), out=e.out(300)), device=dev)
add(P + "/out_cap_smaller", lambda e: call(e, e.data(), out=e.out(300), out_cap=293))
add(P + "/out_cap_larger", lambda e: call(e, e.data(), out=e.out(300), out_cap=1299))
add(P + "/out_cap_alone", lambda e: call(e, e.data(), out_cap=305))
add(P + "/out_wrong_dtype", lambda e: call(e, e.data(), out=e.out(300, dtype=np.uint16)))
add(P + "/out_numpy_for_tensor", lambda e: call(e, e.data(), out=e.out(300, device=False)), device=True)
add(P + "/out_tensor_for_numpy", lambda e: call(e, e.data(), out=e.out(300, device=True)))


add("zip_write_last_route", lambda e: e.eng.zip_write_last_route(),
    {"zip_write_last_route": [{"long_entries": 2, "n_pieces": 131}]})
add("zip_write_last_route/unchanged_route", lambda e: e.eng.zip_write_last_route(), {"zip_write_last_route": [{}]})
add("zip_write_last_route/raises", lambda e: e.eng.zip_write_last_route(), {"zip_write_last_route": [{"rc": E.E_INVALID}]})


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
