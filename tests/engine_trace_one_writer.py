"""What engine.py hands to the C ABI for the writer of one stream in parts (FlateEngine.open_one_writer), recorded
without a device (tests/test_engine_marshalling_one_writer.py): the machinery is tests/engine_trace.py's -- its
recording library, its Env and its serialiser -- with the entry points' signatures added to its table and the scenarios
of engine.OneWriter kept HERE, in a table and a fixture of their own (tests/golden/engine_calls_one_writer.json).

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_one_writer.json")

et.SIGNATURES.setdefault("flate_hip_one_writer_open", et._parse("ctx wrap piece_bytes flags stream:u64[1]>"))
et.SIGNATURES.setdefault("flate_hip_one_writer_write", et._parse(
    "stream in in_len final out cap in_used:u64[1]> out_len:u64[1]> bit_off:u64[*]> n_pieces:u32[1]>"))
et.SIGNATURES.setdefault("flate_hip_one_writer_reset", et._parse("stream"))
et.SIGNATURES.setdefault("flate_hip_one_writer_free", et._parse("stream"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def session(wrap="gzip", piece_bytes=50, final=False, data=None, device=None, compat_go=False, **kw):
    """open, one write of the scenario's 200 bytes (or of data(env)), close -> what write returned."""
    def fn(e):
        wr = e.eng.open_one_writer(wrap, piece_bytes, device=e.device if device is None else device, compat_go=compat_go)
        try:
            return wr.write(data(e) if data else e.data(), final=final,
                            **{k: (v(e) if callable(v) else v) for k, v in kw.items()})
        finally:
            wr.close()
    return fn


def build_scenarios():
    done = {"in_used": 200, "out": 90, "out_len": 90, "n_pieces": 4, "bit_off": [0, 170, 340, 511, 700]}
    for dev in (False, True):
        tag = "/dev" if dev else "/host"
        add("write" + tag, session(), {"one_writer_write": [done]}, device=dev)
        add("write/index" + tag, session(index=True), {"one_writer_write": [done]}, device=dev)
        add("write/zlib/final/index" + tag, session("zlib", final=True, index=True), {"one_writer_write": [dict(done, rc=1)]},
            device=dev)
        add("write/out" + tag, session(out=lambda e: e.out(128)), {"one_writer_write": [done]}, device=dev)
        add("write/out_cap" + tag, session(out_cap=100), {"one_writer_write": [done]}, device=dev)
        # a call that does not fit and no capacity given: a second call with the room it asked for
        add("write/second_sizing_call" + tag, session("raw", index=True),
            {"one_writer_write": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}, dict(done, out=5000, out_len=5000)]}, device=dev)
    add("write/out_and_out_cap", session(out=lambda e: e.out(128), out_cap=95), {"one_writer_write": [done]})
    add("write/too_small_with_out_cap", session(out_cap=40, index=True), {"one_writer_write": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}]})
    add("write/nothing_to_do", session(piece_bytes=0), {"one_writer_write": [{}]})
    add("write/compat_go/dev", session(compat_go=True), {"one_writer_write": [done]}, device=True)
    add("write/raises", session(), {"one_writer_write": [{"rc": E.E_INTERNAL}]})
    add("write/too_large_raises", session(), {"one_writer_write": [{"rc": E.E_TOO_LARGE}]})
    add("open/raises", session(), {"one_writer_open": [{"rc": E.E_INVALID}]})
    add("write/empty_final", session("raw", final=True, data=lambda e: e.data(0), index=True),
        {"one_writer_write": [{"rc": 1, "out": 5, "out_len": 5, "bit_off": [0]}]})
    add("write/none_final", session(final=True, data=lambda e: None), {"one_writer_write": [{"rc": 1, "out": 23, "out_len": 23}]})
    add("write/bytes", session(data=lambda e: bytes(range(200))), {"one_writer_write": [done]})
    add("write/wrong_side", session(device=True, data=lambda e: e.data(device=False)))

    def twice(e):
        wr = e.eng.open_one_writer("gzip", 50)
        a = wr.write(e.data())
        wr.reset()
        b = wr.write(e.data(120), final=True, index=True)
        wr.close()
        wr.close()  # (the handle is freed once)
        return a, b
    add("reset_and_a_second_stream", twice,
        {"one_writer_write": [done, {"rc": 1, "in_used": 120, "out": 70, "out_len": 70, "n_pieces": 3, "bit_off": [0, 9, 18, 27]}]})


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
