"""What engine.py hands to the C ABI for the seek index's two calls, recorded without a device
(tests/test_engine_marshalling_seek.py): the machinery is tests/engine_trace.py's -- its recording library, its Env and
its serialiser -- with the two entry points' signatures added to its table and the scenarios of engine.OneSeekCalls
kept HERE, in a table and a fixture of their own (tests/golden/engine_calls_seek.json), so that the recording of the
methods that were there before stays what it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import numpy as np

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_seek.json")

# (out, cap of the build: the windows)
et.SIGNATURES.setdefault("flate_hip_inflate_one_seek_index", et._parse(
    "ctx in in_len wrap span index:u64[index_cap_words]> index_cap_words index_words:u64[1]> out cap "
    "windows_bytes:u64[1]> n_units:u32[1]> n_points:u32[1]> out_bytes:u64[1]> n_candidates:u32[1]> status:i32[1]> "
    "err_off:i64[1]> flags"))
et.SIGNATURES.setdefault("flate_hip_inflate_one_ranges", et._parse(
    "ctx in in_len wrap index:u64[index_words]< index_words windows windows_bytes begin:u64[n_ranges]< "
    "end:u64[n_ranges]< n_ranges out cap out_off:u64[n_ranges+1]> range_status:i32[n_ranges]> n_decoded:u32[1]> "
    "bad_unit:u32[1]> flags"))

SCENARIOS = {}  # name -> (function(env) -> result, script, device)
PER_CHAIN = et.PER_STREAM + (E.E_TOO_LARGE,)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def family(name, call, script, tolerated, single=None, outs=None, empty=None):
    """The scenarios engine_trace.family gives every method: host, device, bytes, every tolerated status, a status that
    raises, no input and -- outs: the method takes out= and out_cap= -- the forms of a supplied buffer."""
    single = single or call
    add(name + "/host", lambda e: call(e, e.data()), script)
    add(name + "/dev", lambda e: call(e, e.data()), script, device=True)
    add(name + "/bytes", lambda e: call(e, bytes(range(200))), script)
    for rc in tolerated:
        add("%s/status%d" % (name, rc), lambda e: single(e, e.data()), et.with_rc(script, rc, name))
    add(name + "/raises", lambda e: single(e, e.data()), et.with_rc(script, et.BAD, name))
    add(name + "/empty", empty, script)
    if outs is None:
        return
    for dev in (False, True):
        add(name + "/out" + ("/dev" if dev else ""), lambda e: call(e, e.data(), out=e.out(outs)), script, device=dev)
    add(name + "/out_cap_smaller", lambda e: call(e, e.data(), out=e.out(outs), out_cap=outs - 7), script)
    add(name + "/out_cap_larger", lambda e: call(e, e.data(), out=e.out(outs), out_cap=outs + 999), script)
    add(name + "/out_cap_alone", lambda e: call(e, e.data(), out_cap=outs + 5), script)
    add(name + "/out_wrong_dtype", lambda e: call(e, e.data(), out=e.out(outs, dtype=np.uint16)), script)
    add(name + "/out_numpy_for_tensor", lambda e: call(e, e.data(), out=e.out(outs, device=False)), script, device=True)
    add(name + "/out_tensor_for_numpy", lambda e: call(e, e.data(), out=e.out(outs, device=True)), script)


def build_scenarios():
    words = list(range(100, 125))  # (the library judges an index; the wrapper passes it on)
    counts = {"index_words": 25, "windows_bytes": 32768, "n_units": 3, "n_points": 2, "out_bytes": 900,
              "n_candidates": 11, "status": 0}
    built = dict(counts, index=words, out=32768)
    sxi = lambda e, d, **k: e.eng.inflate_one_seek_index(d, **k)
    family("inflate_one_seek_index", sxi, {"inflate_one_seek_index": [built]},
           (E.E_CORRUPT, E.E_UNEXPECTED_EOF, E.E_TOO_LARGE, E.E_OUT_TOO_SMALL), empty=lambda e: sxi(e, e.data(0)))
    add("inflate_one_seek_index/raw_span", lambda e: sxi(e, e.data(), wrap="raw", span=4096), {"inflate_one_seek_index": [built]})
    add("inflate_one_seek_index/span_none", lambda e: sxi(e, e.data(), wrap="zlib", span=E.SEEK_SPAN_NONE),
        {"inflate_one_seek_index": [dict(counts, index=words[:24], index_words=24, windows_bytes=0, n_points=1)]})
    add("inflate_one_seek_index/unknown_wrap", lambda e: sxi(e, e.data(), wrap="lzma"))
    big = dict(counts, index_words=300, windows_bytes=5 * 32768, n_points=6)
    for dev in (False, True):
        add("inflate_one_seek_index/second_sizing_call" + ("/dev" if dev else ""), lambda e: sxi(e, e.data(), span=1),
            {"inflate_one_seek_index": [dict(big, rc=E.E_OUT_TOO_SMALL), dict(big, index=list(range(300)), out=5 * 32768)]},
            device=dev)
    add("inflate_one_seek_index/too_small_again", lambda e: sxi(e, e.data()),
        {"inflate_one_seek_index": [dict(big, rc=E.E_OUT_TOO_SMALL), dict(big, index_words=400, rc=E.E_OUT_TOO_SMALL)]})
    add("inflate_one_seek_index/failing_stream", lambda e: sxi(e, e.data()),
        {"inflate_one_seek_index": [dict(rc=E.E_CORRUPT, status=E.E_CORRUPT, err_off=77, n_units=2, n_candidates=5)]})

    rng = {"inflate_one_ranges": [{"rc": E.E_OUT_TOO_SMALL, "out_off": [0, 5, 25]},
                                  {"out": 25, "out_off": [0, 5, 25], "range_status": [0, 0], "n_decoded": 4,
                                   "bad_unit": 0xffffffff}]}

    def pair(e):
        return np.array(words, np.uint64), e._buffer(np.zeros(32768, np.uint8), "windows", e.device)
    ranges = lambda e, d, **k: e.eng.inflate_one_ranges(d, pair(e), [0, 10], [5, 30], wrap="zlib", **k)
    with_out = lambda e, d: ranges(e, d, out=e.out(64))
    family("inflate_one_ranges", ranges, rng, PER_CHAIN, single=with_out, outs=64,
           empty=lambda e: e.eng.inflate_one_ranges(e.data(), pair(e), [], []))
    add("inflate_one_ranges/seek_index_tuple",
        lambda e: e.eng.inflate_one_ranges(e.data(), E.SeekIndex(0, np.array(words[:24], np.uint64), None, 3, 1, 900, 0, -1),
                                           [7], [9], out=e.out(16)),
        {"inflate_one_ranges": [{"out": 2, "out_off": [0, 2], "range_status": [0], "n_decoded": 1, "bad_unit": 0xffffffff}]})
    add("inflate_one_ranges/does_not_fit", lambda e: with_out(e, e.data()),
        {"inflate_one_ranges": [{"rc": E.E_CORRUPT, "out": 25, "out_off": [0, 5, 25], "range_status": [0, E.E_CORRUPT],
                                 "n_decoded": 4, "bad_unit": 2}]})
    add("inflate_one_ranges/another_stream", lambda e: ranges(e, e.data()),
        {"inflate_one_ranges": [{"rc": E.E_CORRUPT, "out_off": [0, 0, 0], "range_status": [E.E_CORRUPT, E.E_CORRUPT]}]})
    add("inflate_one_ranges/nothing_to_deliver/dev", lambda e: ranges(e, e.data()),
        {"inflate_one_ranges": [{"out_off": [0, 0, 0]}]}, device=True)
    add("inflate_one_ranges/index_refused", lambda e: with_out(e, e.data()), {"inflate_one_ranges": [{"rc": E.E_INVALID}]})
    add("inflate_one_ranges/windows_on_the_other_side",
        lambda e: e.eng.inflate_one_ranges(e.data(), (np.array(words, np.uint64),
                                                      e._buffer(np.zeros(32768, np.uint8), "windows", True)), [0], [5]))
    add("inflate_one_ranges/shapes_differ", lambda e: e.eng.inflate_one_ranges(e.data(), pair(e), [0, 1], [5]))


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
