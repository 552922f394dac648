"""What engine.py hands to the C ABI for a BGZF file in parts (FlateEngine.open_bgzf_reader / open_bgzf_writer), recorded
without a device (tests/test_engine_marshalling_bgzf_parts.py): the machinery is tests/engine_trace.py's -- its recording
library, its Env and its serialiser -- with the entry points' signatures added to its table and the scenarios of
engine.BgzfReader and engine.BgzfWriter kept HERE, in a table and a fixture of their own
(tests/golden/engine_calls_bgzf_parts.json).

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_bgzf_parts.json")

et.SIGNATURES.setdefault("flate_hip_bgzf_reader_open", et._parse("ctx flags stream:u64[1]>"))
et.SIGNATURES.setdefault("flate_hip_bgzf_reader_read", et._parse(
    "stream in in_len final out cap in_used:u64[1]> out_len:u64[1]> index_cap member_off:u64[index_cap]> "
    "out_off:u64[index_cap]> n_members:u32[1]> bad_member:u32[1]> err_off:i64[1]> eof_marker:i32[1]>"))
et.SIGNATURES.setdefault("flate_hip_bgzf_reader_reset", et._parse("stream"))
et.SIGNATURES.setdefault("flate_hip_bgzf_reader_free", et._parse("stream"))
et.SIGNATURES.setdefault("flate_hip_bgzf_writer_open", et._parse("ctx block_bytes flags stream:u64[1]>"))
et.SIGNATURES.setdefault("flate_hip_bgzf_writer_write", et._parse(
    "stream in in_len final out cap in_used:u64[1]> out_len:u64[1]> member_off:u64[*]> n_blocks:u32[1]>"))
et.SIGNATURES.setdefault("flate_hip_bgzf_writer_reset", et._parse("stream"))
et.SIGNATURES.setdefault("flate_hip_bgzf_writer_free", et._parse("stream"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def reading(final=False, data=None, device=None, **kw):
    """open, one read of the scenario's 200 bytes (or of data(env)), close -> what read returned."""
    def fn(e):
        rd = e.eng.open_bgzf_reader(device=e.device if device is None else device)
        try:
            return rd.read(data(e) if data else e.data(), final=final,
                           **{k: (v(e) if callable(v) else v) for k, v in kw.items()})
        finally:
            rd.close()
    return fn


def writing(block_bytes=50, final=False, data=None, device=None, compat_go=False, **kw):
    """open, one write of the scenario's 200 bytes (or of data(env)), close -> what write returned."""
    def fn(e):
        wr = e.eng.open_bgzf_writer(block_bytes, device=e.device if device is None else device, compat_go=compat_go)
        try:
            return wr.write(data(e) if data else e.data(), final=final,
                            **{k: (v(e) if callable(v) else v) for k, v in kw.items()})
        finally:
            wr.close()
    return fn


def build_scenarios():
    done = {"in_used": 150, "out": 25, "out_len": 25, "n_members": 2, "member_off": [1000, 1070, 1150], "out_off": [500, 510, 525],
            "eof_marker": 1}
    for dev in (False, True):
        tag = "/dev" if dev else "/host"
        add("read" + tag, reading(), {"bgzf_reader_read": [done]}, device=dev)
        add("read/final/index" + tag, reading(final=True, index=True), {"bgzf_reader_read": [dict(done, rc=1, in_used=200)]}, device=dev)
        add("read/index_cap" + tag, reading(index=2), {"bgzf_reader_read": [dict(done, n_members=1)]}, device=dev)
        add("read/out" + tag, reading(out=lambda e: e.out(64)), {"bgzf_reader_read": [done]}, device=dev)
        add("read/out_cap" + tag, reading(out_cap=40), {"bgzf_reader_read": [done]}, device=dev)
        # a first member that does not fit and no capacity given: a second call with room for it
        add("read/second_sizing_call" + tag, reading(),
            {"bgzf_reader_read": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}, dict(done, out=5000, out_len=5000, n_members=1)]},
            device=dev)
    add("read/too_small_with_out_cap", reading(out_cap=40), {"bgzf_reader_read": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 5000}]})
    # a sticky -2 (a member that produced more than its ISIZE names the member): no second call, the bytes in front stay
    add("read/sticky_too_small", reading(), {"bgzf_reader_read": [dict(done, rc=E.E_OUT_TOO_SMALL, bad_member=7, err_off=4321, in_used=0)]})
    for rc in (E.E_CORRUPT, E.E_UNEXPECTED_EOF, E.E_TOO_LARGE, E.E_UNSUPPORTED):
        add("read/status%d" % rc, reading(final=True, index=True),
            {"bgzf_reader_read": [dict(done, rc=rc, bad_member=5, err_off=1234, in_used=0)]})
    add("read/raises", reading(), {"bgzf_reader_read": [{"rc": E.E_INTERNAL}]})
    add("read/open_raises", reading(), {"bgzf_reader_open": [{"rc": E.E_INVALID}]})
    add("read/empty_part", reading(final=True, data=lambda e: e.data(0)), {"bgzf_reader_read": [{"rc": 1}]})
    add("read/bytes", reading(data=lambda e: bytes(range(200))), {"bgzf_reader_read": [done]})
    add("read/wrong_side", reading(device=True, data=lambda e: e.data(device=False)))

    def two_files(e):
        rd = e.eng.open_bgzf_reader()
        a = rd.read(e.data())
        rd.reset()
        b = rd.read(e.data(120), final=True)
        rd.close()
        rd.close()  # (the handle is freed once)
        return a, b
    add("read/reset_and_a_second_file", two_files, {"bgzf_reader_read": [done, dict(done, rc=1, in_used=120)]})

    wrote = {"in_used": 200, "out": 90, "out_len": 90, "n_blocks": 4, "member_off": [300, 320, 345, 365, 390]}
    for dev in (False, True):
        tag = "/dev" if dev else "/host"
        add("write" + tag, writing(), {"bgzf_writer_write": [wrote]}, device=dev)
        add("write/index" + tag, writing(index=True), {"bgzf_writer_write": [wrote]}, device=dev)
        add("write/final/index" + tag, writing(final=True, index=True), {"bgzf_writer_write": [dict(wrote, rc=1)]}, device=dev)
        add("write/out" + tag, writing(out=lambda e: e.out(128)), {"bgzf_writer_write": [wrote]}, device=dev)
        add("write/out_cap" + tag, writing(out_cap=100), {"bgzf_writer_write": [wrote]}, device=dev)
    add("write/default_block", writing(block_bytes=0), {"bgzf_writer_write": [{}]})
    add("write/too_small", writing(out_cap=40, index=True), {"bgzf_writer_write": [{"rc": E.E_OUT_TOO_SMALL}]})
    add("write/too_large", writing(), {"bgzf_writer_write": [{"rc": E.E_TOO_LARGE}]})
    add("write/compat_go/dev", writing(compat_go=True), {"bgzf_writer_write": [wrote]}, device=True)
    add("write/raises", writing(), {"bgzf_writer_write": [{"rc": E.E_INTERNAL}]})
    add("write/open_raises", writing(block_bytes=65536), {"bgzf_writer_open": [{"rc": E.E_INVALID}]})
    add("write/none_final", writing(final=True, data=lambda e: None), {"bgzf_writer_write": [{"rc": 1, "out": 28, "out_len": 28}]})
    add("write/bytes", writing(data=lambda e: bytes(range(200))), {"bgzf_writer_write": [wrote]})
    add("write/wrong_side", writing(device=True, data=lambda e: e.data(device=False)))

    def two_outputs(e):
        wr = e.eng.open_bgzf_writer(50)
        a = wr.write(e.data())
        wr.reset()
        b = wr.write(e.data(120), final=True, index=True)
        wr.close()
        wr.close()  # (the handle is freed once)
        return a, b
    add("write/reset_and_a_second_file", two_outputs,
        {"bgzf_writer_write": [wrote, {"rc": 1, "in_used": 120, "out": 70, "out_len": 70, "n_blocks": 3, "member_off": [0, 9, 18, 27]}]})


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
