"""What engine.py hands to the C ABI for the two calls of a gzip file's seek index, recorded without a device
(tests/test_engine_marshalling_gzfile_seek.py): the machinery is tests/engine_trace.py's -- its recording library, its
Env and its serialiser -- with the two entry points' signatures added to its table and the scenarios of
engine.GzFileSeekCalls kept HERE, in a table and a fixture of their own (tests/golden/engine_calls_gzfile_seek.json),
so that the recording of the methods that were there before stays what it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import numpy as np

import engine_trace as et
import engine_trace_seek as seek

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_gzfile_seek.json")

# (out, cap of the build: the windows)
et.SIGNATURES.setdefault("flate_hip_gzfile_seek_index", et._parse(
    "ctx in in_len span index:u64[index_cap_words]> index_cap_words index_words:u64[1]> out cap windows_bytes:u64[1]> "
    "n_units:u32[1]> n_members:u32[1]> n_points:u32[1]> out_bytes:u64[1]> n_candidates:u32[1]> status:i32[1]> "
    "bad_member:u32[1]> err_off:i64[1]> stream_err_off:i64[1]> flags"))
et.SIGNATURES.setdefault("flate_hip_gzfile_ranges", et._parse(
    "ctx in in_len index:u64[index_words]< index_words windows windows_bytes begin:u64[n_ranges]< end:u64[n_ranges]< "
    "n_ranges out cap out_off:u64[n_ranges+1]> range_status:i32[n_ranges]> n_decoded:u32[1]> bad_unit:u32[1]> flags"))

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
    words = list(range(100, 131))  # (the library judges an index; the wrapper passes it on)
    counts = {"index_words": 31, "windows_bytes": 32768, "n_units": 3, "n_members": 2, "n_points": 3, "out_bytes": 900,
              "n_candidates": 11, "status": 0, "bad_member": NONE}
    built = dict(counts, index=words, out=32768)
    gsi = lambda e, d, **k: e.eng.gzfile_seek_index(d, **k)
    family("gzfile_seek_index", gsi, {"gzfile_seek_index": [built]},
           (E.E_CORRUPT, E.E_UNEXPECTED_EOF, E.E_TOO_LARGE, E.E_OUT_TOO_SMALL), empty=lambda e: gsi(e, e.data(0)))
    add("gzfile_seek_index/span", lambda e: gsi(e, e.data(), span=4096), {"gzfile_seek_index": [built]})
    add("gzfile_seek_index/span_none", lambda e: gsi(e, e.data(), span=E.SEEK_SPAN_NONE),
        {"gzfile_seek_index": [dict(counts, index=words[:30], index_words=30, windows_bytes=0, n_points=2)]})
    big = dict(counts, index_words=300, windows_bytes=5 * 32768, n_points=7)
    for dev in (False, True):
        add("gzfile_seek_index/second_sizing_call" + ("/dev" if dev else ""), lambda e: gsi(e, e.data(), span=1),
            {"gzfile_seek_index": [dict(big, rc=E.E_OUT_TOO_SMALL), dict(big, index=list(range(300)), out=5 * 32768)]},
            device=dev)
    add("gzfile_seek_index/too_small_again", lambda e: gsi(e, e.data()),
        {"gzfile_seek_index": [dict(big, rc=E.E_OUT_TOO_SMALL), dict(big, index_words=400, rc=E.E_OUT_TOO_SMALL)]})
    add("gzfile_seek_index/failing_file", lambda e: gsi(e, e.data()),
        {"gzfile_seek_index": [dict(rc=E.E_CORRUPT, status=E.E_CORRUPT, n_units=2, n_members=1, bad_member=1, err_off=150,
                                    stream_err_off=33, n_candidates=5)]})

    rng = {"gzfile_ranges": [{"rc": E.E_OUT_TOO_SMALL, "out_off": [0, 5, 25]},
                             {"out": 25, "out_off": [0, 5, 25], "range_status": [0, 0], "n_decoded": 4, "bad_unit": NONE}]}

    def pair(e):
        return np.array(words, np.uint64), e._buffer(np.zeros(32768, np.uint8), "windows", e.device)
    ranges = lambda e, d, **k: e.eng.gzfile_ranges(d, pair(e), [0, 10], [5, 30], **k)
    with_out = lambda e, d: ranges(e, d, out=e.out(64))
    family("gzfile_ranges", ranges, rng, PER_CHAIN, single=with_out, outs=64,
           empty=lambda e: e.eng.gzfile_ranges(e.data(), pair(e), [], []))
    add("gzfile_ranges/seek_index_tuple",
        lambda e: e.eng.gzfile_ranges(e.data(), E.GzFileSeekIndex(0, np.array(words[:30], np.uint64), None, 3, 2, 2, 900, 11,
                                                                  0, NONE, -1, -1), [7], [9], out=e.out(16)),
        {"gzfile_ranges": [{"out": 2, "out_off": [0, 2], "range_status": [0], "n_decoded": 1, "bad_unit": NONE}]})
    add("gzfile_ranges/does_not_fit", lambda e: with_out(e, e.data()),
        {"gzfile_ranges": [{"rc": E.E_CORRUPT, "out": 25, "out_off": [0, 5, 25], "range_status": [0, E.E_CORRUPT],
                            "n_decoded": 4, "bad_unit": 2}]})
    add("gzfile_ranges/another_file", lambda e: ranges(e, e.data()),
        {"gzfile_ranges": [{"rc": E.E_CORRUPT, "out_off": [0, 0, 0], "range_status": [E.E_CORRUPT, E.E_CORRUPT]}]})
    add("gzfile_ranges/nothing_to_deliver/dev", lambda e: ranges(e, e.data()),
        {"gzfile_ranges": [{"out_off": [0, 0, 0]}]}, device=True)
    add("gzfile_ranges/index_refused", lambda e: with_out(e, e.data()), {"gzfile_ranges": [{"rc": E.E_INVALID}]})
    add("gzfile_ranges/windows_on_the_other_side",
        lambda e: e.eng.gzfile_ranges(e.data(), (np.array(words, np.uint64),
                                                 e._buffer(np.zeros(32768, np.uint8), "windows", True)), [0], [5]))
    add("gzfile_ranges/shapes_differ", lambda e: e.eng.gzfile_ranges(e.data(), pair(e), [0, 1], [5]))


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
