"""What engine.py hands to the C ABI for the three calls of the packed windows, recorded without a device
(tests/test_seek_pack_abi.py): the machinery is tests/engine_trace.py's -- its recording library, its Env and its
serialiser -- with the three entry points' signatures added to its table and the scenarios of engine.SeekPackCalls kept
HERE, in a table and a fixture of their own (tests/golden/engine_calls_seek_pack.json), so that the recording of the
methods that were there before stays what it is.

Run as a script, this writes the fixture from the engine.py and _lib.py that are in the tree."""
import json
import os

import numpy as np

import engine_trace as et

E = et.engine
FIXTURE = os.path.join(et.ROOT, "tests", "golden", "engine_calls_seek_pack.json")

# (out, cap of the pack: the packed bytes; of the unpack: the windows)
et.SIGNATURES.setdefault("flate_hip_seek_windows_pack", et._parse(
    "ctx in in_len wrap index:u64[index_words]< index_words windows windows_bytes mode pack_index:u64[pack_cap_words]> "
    "pack_cap_words pack_words:u64[1]> out cap packed_bytes:u64[1]> kept_bytes:u64[1]> flags"))
et.SIGNATURES.setdefault("flate_hip_seek_windows_unpack", et._parse(
    "ctx pack_index:u64[pack_words]< pack_words packed packed_bytes out cap windows_bytes:u64[1]> bad_block:u32[1]> flags"))
et.SIGNATURES.setdefault("flate_hip_inflate_one_ranges_packed", et._parse(
    "ctx in in_len wrap index:u64[index_words]< index_words pack_index:u64[pack_words]< pack_words packed packed_bytes "
    "begin:u64[n_ranges]< end:u64[n_ranges]< n_ranges out cap out_off:u64[n_ranges+1]> range_status:i32[n_ranges]> "
    "n_decoded:u32[1]> bad_unit:u32[1]> flags"))
if "flate_hip_seek_windows_pack_bound" not in et.PASS_THROUGH:  # (host arithmetic: the real library answers)
    et.PASS_THROUGH = et.PASS_THROUGH + ("flate_hip_seek_windows_pack_bound",)

SCENARIOS = {}  # name -> (function(env) -> result, script, device)
PER_CHAIN = et.PER_STREAM + (E.E_TOO_LARGE,)


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def build_scenarios():
    # (the library judges an index; the wrapper passes it on -- but reads in_len and n_points from its head)
    words = [0] * 25
    words[3], words[9] = 200, 3
    pwords = list(range(500, 519))
    pwords[3] = 2

    def pair(e, device=None):
        return np.array(words, np.uint64), e._buffer(np.zeros(2 * 32768, np.uint8), "windows", e.device if device is None else device)

    packed = {"seek_windows_pack": [{"pack_index": pwords, "pack_words": 19, "out": 700, "packed_bytes": 700, "kept_bytes": 4242}]}
    pack = lambda e, d, **k: e.eng.seek_windows_pack(pair(e), d, **k)
    for dev in (False, True):
        add("seek_windows_pack/" + ("dev" if dev else "host"), lambda e: pack(e, e.data()), packed, device=dev)
        add("seek_windows_pack/compress_without_the_stream" + ("/dev" if dev else ""),
            lambda e: e.eng.seek_windows_pack(pair(e), sparse=False, wrap="zlib"), packed, device=dev)
        add("seek_windows_pack/out" + ("/dev" if dev else ""), lambda e: pack(e, e.data(), out=e.out(900)), packed, device=dev)
    add("seek_windows_pack/bytes", lambda e: pack(e, bytes(range(200))), packed)
    add("seek_windows_pack/raw", lambda e: pack(e, e.data(), wrap="raw", sparse=False), packed)
    add("seek_windows_pack/out_cap_smaller", lambda e: pack(e, e.data(), out=e.out(900), out_cap=650),
        {"seek_windows_pack": [{"rc": E.E_OUT_TOO_SMALL, "pack_words": 19, "packed_bytes": 700}]})
    add("seek_windows_pack/another_stream", lambda e: pack(e, e.data()), {"seek_windows_pack": [{"rc": E.E_CORRUPT, "pack_words": 19}]})
    add("seek_windows_pack/raises", lambda e: pack(e, e.data()), et.with_rc(packed, et.BAD, "seek_windows_pack"))
    add("seek_windows_pack/index_refused", lambda e: pack(e, e.data()), {"seek_windows_pack": [{"rc": E.E_INVALID}]})
    add("seek_windows_pack/seek_index_tuple_no_windows",
        lambda e: e.eng.seek_windows_pack(E.SeekIndex(0, np.array(words[:9] + [1] + words[10:24], np.uint64), None, 3, 1, 900, 0, -1),
                                          e.data()),
        {"seek_windows_pack": [{"pack_index": pwords[:17], "pack_words": 17}]})
    add("seek_windows_pack/windows_on_the_other_side", lambda e: e.eng.seek_windows_pack(pair(e, True), e.data()))
    add("seek_windows_pack/unknown_wrap", lambda e: pack(e, e.data(), wrap="lzma"))

    def pk(e, device=None):
        return np.array(pwords, np.uint64), e._buffer(np.zeros(700, np.uint8), "packed", e.device if device is None else device)

    unpacked = {"seek_windows_unpack": [{"out": 65536, "windows_bytes": 65536, "bad_block": 0xffffffff}]}
    for dev in (False, True):
        add("seek_windows_unpack/" + ("dev" if dev else "host"), lambda e: e.eng.seek_windows_unpack(pk(e)), unpacked, device=dev)
        add("seek_windows_unpack/out" + ("/dev" if dev else ""), lambda e: e.eng.seek_windows_unpack(pk(e), out=e.out(70000)),
            unpacked, device=dev)
    add("seek_windows_unpack/seek_pack_tuple",
        lambda e: e.eng.seek_windows_unpack(E.SeekPack(0, pk(e)[0], pk(e)[1], 700, 4242)), unpacked)
    add("seek_windows_unpack/out_cap_smaller", lambda e: e.eng.seek_windows_unpack(pk(e), out=e.out(70000), out_cap=65535),
        {"seek_windows_unpack": [{"rc": E.E_OUT_TOO_SMALL, "windows_bytes": 65536}]})
    add("seek_windows_unpack/bad_block", lambda e: e.eng.seek_windows_unpack(pk(e)),
        {"seek_windows_unpack": [{"rc": E.E_CORRUPT, "out": 65536, "windows_bytes": 65536, "bad_block": 1}]})
    add("seek_windows_unpack/raises", lambda e: e.eng.seek_windows_unpack(pk(e)), et.with_rc(unpacked, et.BAD, "seek_windows_unpack"))
    add("seek_windows_unpack/wrong_out", lambda e: e.eng.seek_windows_unpack(pk(e), out=e.out(70000, dtype=np.uint16)), unpacked)

    rng = {"inflate_one_ranges_packed": [{"rc": E.E_OUT_TOO_SMALL, "out_off": [0, 5, 25]},
                                         {"out": 25, "out_off": [0, 5, 25], "range_status": [0, 0], "n_decoded": 4,
                                          "bad_unit": 0xffffffff}]}
    ranges = lambda e, d, **k: e.eng.inflate_one_ranges_packed(d, np.array(words, np.uint64), pk(e), [0, 10], [5, 30],
                                                               wrap="zlib", **k)
    with_out = lambda e, d: ranges(e, d, out=e.out(64))
    for dev in (False, True):
        add("inflate_one_ranges_packed/" + ("dev" if dev else "host"), lambda e: ranges(e, e.data()), rng, device=dev)
        add("inflate_one_ranges_packed/out" + ("/dev" if dev else ""), lambda e: with_out(e, e.data()), rng, device=dev)
    add("inflate_one_ranges_packed/bytes", lambda e: ranges(e, bytes(range(200))), rng)
    for rc in PER_CHAIN:
        add("inflate_one_ranges_packed/status%d" % rc, lambda e: with_out(e, e.data()), et.with_rc(rng, rc, "inflate_one_ranges_packed"))
    add("inflate_one_ranges_packed/raises", lambda e: with_out(e, e.data()), et.with_rc(rng, et.BAD, "inflate_one_ranges_packed"))
    add("inflate_one_ranges_packed/empty", lambda e: e.eng.inflate_one_ranges_packed(e.data(), np.array(words, np.uint64), pk(e), [], []),
        rng)
    add("inflate_one_ranges_packed/out_cap_smaller", lambda e: ranges(e, e.data(), out=e.out(64), out_cap=57), rng)
    add("inflate_one_ranges_packed/seek_index_and_pack_tuples",
        lambda e: e.eng.inflate_one_ranges_packed(e.data(), E.SeekIndex(0, np.array(words, np.uint64), None, 3, 3, 900, 0, -1),
                                                  E.SeekPack(0, pk(e)[0], pk(e)[1], 700, 4242), [7], [9], out=e.out(16)),
        {"inflate_one_ranges_packed": [{"out": 2, "out_off": [0, 2], "range_status": [0], "n_decoded": 1, "bad_unit": 0xffffffff}]})
    add("inflate_one_ranges_packed/bad_block", lambda e: with_out(e, e.data()),
        {"inflate_one_ranges_packed": [{"rc": E.E_CORRUPT, "out": 25, "out_off": [0, 5, 25], "range_status": [0, E.E_CORRUPT],
                                        "n_decoded": 4, "bad_unit": 2}]})
    add("inflate_one_ranges_packed/no_packed_bytes",
        lambda e: e.eng.inflate_one_ranges_packed(e.data(), np.array(words, np.uint64), (np.array(pwords, np.uint64), None), [0], [5],
                                                  out=e.out(16)),
        {"inflate_one_ranges_packed": [{"out": 5, "out_off": [0, 5], "range_status": [0], "n_decoded": 1, "bad_unit": 0xffffffff}]})
    add("inflate_one_ranges_packed/packed_on_the_other_side",
        lambda e: e.eng.inflate_one_ranges_packed(e.data(), np.array(words, np.uint64), pk(e, True), [0], [5]))
    add("inflate_one_ranges_packed/shapes_differ",
        lambda e: e.eng.inflate_one_ranges_packed(e.data(), np.array(words, np.uint64), pk(e), [0, 1], [5]))


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
