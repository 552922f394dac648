"""What engine.py hands to the C ABI for the reader of a gzip file in parts (FlateEngine.open_gzfile_reader), recorded
without a device (tests/test_engine_marshalling_gzfile_parts.py): the machinery is tests/engine_trace.py's -- its
recording library, its Env and its serialiser -- with the four entry points' signatures added to its table and the
scenarios of engine.GzFileReader kept HERE, in a table and a fixture of their own
(tests/golden/engine_calls_gzfile_parts.json).

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_gzfile_parts.json")

et.SIGNATURES.setdefault("flate_hip_gzfile_reader_open", et._parse("ctx flags stream:u64[1]>"))
et.SIGNATURES.setdefault("flate_hip_gzfile_reader_read", et._parse(
    "stream in in_len final out cap in_used:u64[1]> out_len:u64[1]> n_members:u32[1]> n_units:u32[1]> "
    "bad_member:u32[1]> err_off:i64[1]> stream_err_off:i64[1]>"))
et.SIGNATURES.setdefault("flate_hip_gzfile_reader_reset", et._parse("stream"))
et.SIGNATURES.setdefault("flate_hip_gzfile_reader_free", et._parse("stream"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def session(final=False, data=None, device=None, **kw):
    """open, one read of the scenario's 200 bytes (or of data(env)), close -> what read returned."""
    def fn(e):
        rd = e.eng.open_gzfile_reader(device=e.device if device is None else device)
        try:
            return rd.read(data(e) if data else e.data(), final=final,
                           **{k: (v(e) if callable(v) else v) for k, v in kw.items()})
        finally:
            rd.close()
    return fn


def build_scenarios():
    done = {"in_used": 150, "out": 25, "out_len": 25, "n_members": 2, "n_units": 3}
    for dev in (False, True):
        tag = "/dev" if dev else "/host"
        add("read" + tag, session(), {"gzfile_reader_read": [done]}, device=dev)
        add("read/final" + tag, session(final=True), {"gzfile_reader_read": [dict(done, rc=1, in_used=200)]}, device=dev)
        add("read/out" + tag, session(out=lambda e: e.out(64)), {"gzfile_reader_read": [done]}, device=dev)
        add("read/out_cap" + tag, session(out_cap=40), {"gzfile_reader_read": [done]}, device=dev)
        # a first unit that does not fit and no capacity given: a second call with room for it
        add("read/second_sizing_call" + tag, session(),
            {"gzfile_reader_read": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}, dict(done, out=5000, out_len=5000, n_units=1)]},
            device=dev)
    add("read/out_and_out_cap", session(out=lambda e: e.out(64), out_cap=30), {"gzfile_reader_read": [done]})
    add("read/too_small_with_out_cap", session(out_cap=40), {"gzfile_reader_read": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}]})
    for rc, eo, so in ((E.E_CORRUPT, 1234, 77), (E.E_UNEXPECTED_EOF, 1234, -1), (E.E_TOO_LARGE, 0, -1)):
        add("read/status%d" % rc, session(final=True),
            {"gzfile_reader_read": [dict(done, rc=rc, bad_member=5, err_off=eo, stream_err_off=so, in_used=0)]})
    add("read/raises", session(), {"gzfile_reader_read": [{"rc": E.E_INTERNAL}]})
    add("open/raises", session(), {"gzfile_reader_open": [{"rc": E.E_INVALID}]})
    add("read/empty_part", session(final=True, data=lambda e: e.data(0)), {"gzfile_reader_read": [{"rc": 1}]})
    add("read/bytes", session(data=lambda e: bytes(range(200))), {"gzfile_reader_read": [done]})
    add("read/wrong_side", session(device=True, data=lambda e: e.data(device=False)))

    def twice(e):
        rd = e.eng.open_gzfile_reader()
        a = rd.read(e.data())
        rd.reset()
        b = rd.read(e.data(120), final=True)
        rd.close()
        rd.close()  # (the handle is freed once)
        return a, b
    add("reset_and_a_second_file", twice, {"gzfile_reader_read": [done, dict(done, rc=1, in_used=120)]})


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
