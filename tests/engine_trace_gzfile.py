"""What engine.py hands to the C ABI for the two gzfile calls, recorded without a device
(tests/test_engine_marshalling_gzfile.py): the machinery is tests/engine_trace.py's -- its recording library, its Env
and its serialiser -- with the two entry points' signatures added to its table and the scenarios of engine.GzFileCalls
kept HERE, in a table and a fixture of their own (tests/golden/engine_calls_gzfile.json), so that the recording of the
methods that were there before stays what it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import engine_trace as et
import engine_trace_seek as seek

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_gzfile.json")

et.SIGNATURES.setdefault("flate_hip_gzfile_index", et._parse(
    "ctx in in_len index_cap unit_bit:u64[index_cap]> out_off:u64[index_cap]> member_cap member_off:u64[member_cap]> "
    "member_unit:u64[member_cap]> n_units:u32[1]> n_members:u32[1]> out_bytes:u64[1]> n_candidates:u32[1]> "
    "status:i32[1]> bad_member:u32[1]> err_off:i64[1]> stream_err_off:i64[1]> flags"))
et.SIGNATURES.setdefault("flate_hip_gzfile_read", et._parse(
    "ctx in in_len out cap out_len:u64[1]> n_members:u32[1]> n_units:u32[1]> n_candidates:u32[1]> status:i32[1]> "
    "bad_member:u32[1]> err_off:i64[1]> stream_err_off:i64[1]> flags"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)
PER_CHAIN = seek.PER_CHAIN
NONE = 0xffffffff


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def family(*args, **kw):
    """engine_trace_seek.family into this module's table."""
    table, seek.SCENARIOS = seek.SCENARIOS, SCENARIOS
    try:
        seek.family(*args, **kw)
    finally:
        seek.SCENARIOS = table


def build_scenarios():
    counts = {"n_units": 3, "n_members": 2, "out_bytes": 900, "n_candidates": 11, "status": 0, "bad_member": NONE}
    filled = dict(counts, unit_bit=[80, 500, 1200, 1500], out_off=[0, 300, 600, 900], member_off=[0, 150, 200],
                  member_unit=[0, 2, 3])
    gxi = lambda e, d, **k: e.eng.gzfile_index(d, **k)
    family("gzfile_index", gxi, {"gzfile_index": [filled]}, PER_CHAIN, empty=lambda e: gxi(e, e.data(0)))
    add("gzfile_index/query", lambda e: gxi(e, e.data(), query=True), {"gzfile_index": [counts]})
    add("gzfile_index/query/dev", lambda e: gxi(e, e.data(), query=True), {"gzfile_index": [counts]}, device=True)
    broken = dict(rc=E.E_CORRUPT, status=E.E_CORRUPT, n_units=2, n_members=1, bad_member=1, err_off=150, stream_err_off=33,
                  n_candidates=9, unit_bit=[80, 500, 1200], out_off=[0, 300, 600], member_off=[0, 150], member_unit=[0, 2])
    add("gzfile_index/broken_chain", lambda e: gxi(e, e.data()), {"gzfile_index": [broken]})
    add("gzfile_index/caps_given", lambda e: gxi(e, e.data(), index_cap=4, member_cap=3), {"gzfile_index": [filled]})
    add("gzfile_index/index_cap_too_small", lambda e: gxi(e, e.data(), index_cap=2),
        {"gzfile_index": [dict(filled, rc=E.E_OUT_TOO_SMALL)]})
    add("gzfile_index/member_cap_too_small", lambda e: gxi(e, e.data(), member_cap=1),
        {"gzfile_index": [dict(filled, rc=E.E_OUT_TOO_SMALL)]})
    many = dict(counts, n_units=99, n_members=80)
    units = dict(unit_bit=list(range(80, 180)), out_off=list(range(100)), member_off=list(range(81)),
                 member_unit=list(range(81)))
    for dev in (False, True):
        add("gzfile_index/second_sizing_call" + ("/dev" if dev else ""), lambda e: gxi(e, e.data()),
            {"gzfile_index": [dict(many, rc=E.E_OUT_TOO_SMALL), dict(many, **units)]}, device=dev)

    done = {"out": 25, "out_len": 25, "n_members": 2, "n_units": 3, "n_candidates": 11, "status": 0, "bad_member": NONE}
    two = {"gzfile_read": [{"rc": E.E_OUT_TOO_SMALL, "out_len": 25, "n_members": 2, "n_units": 3, "n_candidates": 11}, done]}
    gxr = lambda e, d, **k: e.eng.gzfile_read(d, **k)
    with_out = lambda e, d: gxr(e, d, out=e.out(64))
    family("gzfile_read", gxr, two, PER_CHAIN, single=with_out, outs=64, empty=lambda e: gxr(e, e.data(0)))
    add("gzfile_read/nothing_to_deliver", lambda e: gxr(e, e.data()),
        {"gzfile_read": [{"n_members": 3, "n_units": 3, "n_candidates": 4, "bad_member": NONE}]})
    add("gzfile_read/wrong_trailer", lambda e: with_out(e, e.data()),
        {"gzfile_read": [dict(done, rc=E.E_CORRUPT, status=E.E_CORRUPT, bad_member=1, err_off=150, stream_err_off=50)]})
    add("gzfile_read/broken_chain/dev", lambda e: with_out(e, e.data()),
        {"gzfile_read": [dict(done, out=7, out_len=7, rc=E.E_UNEXPECTED_EOF, status=E.E_UNEXPECTED_EOF, n_members=1,
                              n_units=2, bad_member=1, err_off=150)]}, device=True)


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
