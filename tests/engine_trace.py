"""What engine.py hands to the C ABI, recorded without a device (tests/test_engine_marshalling.py).

A FlateEngine is put together without flate_hip_init around a recording stand-in for the library: the pure host
functions pass through to the real one, every other flate_hip_* call is written down as [name, arguments, tables read] -- its
scalar arguments, of every pointer whether it is null or the address of a buffer the scenario supplied, and the contents
of the host tables it reads -- and answered by a responder that
writes through the output pointers what include/flate_hip.h says the call writes, sized by the counts and capacities
it was passed, and returns a scripted rc.  SCENARIOS drives every public method that calls the library; run_all()
gives {scenario: {"trace": ..., "ret": ... | "raises": ...}}.

Run as a script, this writes tests/golden/engine_calls.json from the engine.py and _lib.py that are in the tree.
The committed fixture is a recording of the wrapper as it was BEFORE its methods were rebuilt on shared helpers:
regenerate it only for a new scenario, and then from a tree whose other scenarios still match it.
"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_calls.json")

engine = importlib.import_module("moonbit-flate_amd.engine")
_lib = importlib.import_module("moonbit-flate_amd._lib")

PASS_THROUGH = ("flate_hip_deflate_bound", "flate_hip_frame_overhead", "flate_hip_bgzf_bound", "flate_hip_zip_bound",
                "flate_hip_stream_bound", "flate_hip_strerror", "flate_hip_synth_fill")
CTX, HANDLE = 0x1000, 0x2000  # what stands in for a flate_hip_ctx * and a stream handle: never dereferenced

# The arguments of every recorded call in the header's order.  name:type[count]< is a host table the call reads (its
# contents are recorded), name:type[count]> one it writes (from the scripted answer, never more than count entries);
# count is an expression over the call's scalar arguments, * = as many as the answer holds.  `out` is filled with a
# byte pattern as long as the answer says, cut to `cap` (or to out_off[n] where the call takes no capacity).
SIGNATURES = {
    "init": "device ctx:u64[1]>",
    "destroy": "ctx",
    "set_stream": "ctx stream",
    "set_option": "ctx name value",
    "set_profiling": "ctx on",
    "last_hip_error": "ctx",
    "last_resident_share": "ctx resident:u32[1]> queued:u32[1]>",
    "last_timing": "ctx ms:f32[n]> n",
    "host_register": "ctx ptr bytes",
    "host_unregister": "ctx ptr",
    "deflate_fast_batch": "ctx in in_off:u64[n+1]< n out cap out_off:u64[n+1]> flags",
    "deflate_fast_batch_dict": "ctx in in_off:u64[n+1]< n dicts dict_off:u64[n_dicts+1]< n_dicts dict_of:u32[n]< "
                               "out cap out_off:u64[n+1]> flags",
    "deflate_fast_spliced": "ctx in in_off:u64[n+1]< n out cap out_len:u64[1]> bit_off:u64[n+1]> flags",
    "deflate_fast_batch_framed": "ctx in in_off:u64[n+1]< n wrap dicts dict_off:u64[n_dicts+1]< n_dicts "
                                 "dict_of:u32[n]< out cap out_off:u64[n+1]> flags",
    "deflate_fast_spliced_framed": "ctx in in_off:u64[n+1]< n wrap out cap out_len:u64[1]> bit_off:u64[n+1]> flags",
    "lz77_matches": "ctx in in_off:u64[n+1]< n flags n_chunks:u32[1]> n_recs_cap:u64[1]> chunk_nmatch:u32[*]> "
                    "chunk_rec_off:u64[*]> recs:u32[*]>",
    "inflate_batch": "ctx in in_off:u64[n+1]< n out out_off:u64[n+1]< out_len:u64[n]> status:i32[n]> "
                     "err_off:i64[n]> flags",
    "inflate_batch_dict": "ctx in in_off:u64[n+1]< n dicts dict_off:u64[n_dicts+1]< n_dicts dict_of:u32[n]< out "
                          "out_off:u64[n+1]< out_len:u64[n]> status:i32[n]> err_off:i64[n]> flags",
    "inflate_spliced": "ctx in in_len bit_off:u64[n+1]< n out out_off:u64[n+1]< out_len:u64[n]> status:i32[n]> "
                       "err_off:i64[n]> flags",
    "inflate_batch_framed": "ctx in in_off:u64[n+1]< n wrap dicts dict_off:u64[n_dicts+1]< n_dicts out "
                            "out_off:u64[n+1]< out_len:u64[n]> status:i32[n]> err_off:i64[n]> dict_used:u32[n]> flags",
    "inflate_spliced_framed": "ctx in in_len wrap bit_off:u64[n+1]< n out out_off:u64[n+1]< out_len:u64[n]> "
                              "status:i32[n]> err_off:i64[n]> member_status:i32[1]> member_err_off:i64[1]> flags",
    "checksum_batch": "ctx in in_off:u64[n+1]< n kind sums:u32[n]> flags",
    "stream_open": "ctx flags stream:u64[1]>",
    "stream_write": "stream in n final out cap out_len:u64[1]>",
    "stream_free": "stream",
    "inflate_stream_open": "ctx stream:u64[1]>",
    "inflate_stream_read": "stream in in_len final out cap in_used:u64[1]> out_len:u64[1]> err_off:i64[1]>",
    "inflate_stream_reset": "stream dict dict_len",
    "inflate_stream_free": "stream",
    "bgzf_write": "ctx in in_len block_bytes out cap out_len:u64[1]> member_off:u64[*]> flags",
    "bgzf_index": "ctx in in_len index_cap member_off:u64[index_cap]> out_off:u64[index_cap]> n_members:u32[1]> "
                  "out_bytes:u64[1]> eof_marker:i32[1]> err_off:i64[1]> flags",
    "bgzf_read": "ctx in in_len out cap out_len:u64[1]> n_members:u32[1]> bad_member:u32[1]> err_off:i64[1]> "
                 "eof_marker:i32[1]> flags",
    "bgzf_read_ranges": "ctx in in_len pos_kind begin:u64[n_ranges]< end:u64[n_ranges]< n_ranges out cap "
                        "out_off:u64[n_ranges+1]> range_status:i32[n_ranges]> n_members:u32[1]> n_decoded:u32[1]> "
                        "bad_member:u32[1]> err_off:i64[1]> flags",
    "gzip_index": "ctx in in_len index_cap member_off:u64[index_cap]> out_off:u64[index_cap]> n_members:u32[1]> "
                  "out_bytes:u64[1]> n_candidates:u32[1]> err_off:i64[1]> flags",
    "gzip_read": "ctx in in_len out cap out_len:u64[1]> n_members:u32[1]> bad_member:u32[1]> err_off:i64[1]> flags",
    "inflate_one": "ctx in in_len wrap out cap out_len:u64[1]> status:i32[1]> err_off:i64[1]> n_units:u32[1]> "
                   "n_candidates:u32[1]> flags",
    "inflate_one_index": "ctx in in_len wrap index_cap unit_bit:u64[index_cap]> out_off:u64[index_cap]> "
                         "n_units:u32[1]> out_bytes:u64[1]> n_candidates:u32[1]> status:i32[1]> err_off:i64[1]> flags",
    "zip_write": "ctx in in_off:u64[n+1]< n names name_off:u64[n+1]< out cap out_len:u64[1]> entry_off:u64[n+1]> "
                 "flags",
    "zip_index": "ctx in in_len index_cap entries:zip[index_cap]> out_off:u64[index_cap+1]> n_entries:u32[1]> "
                 "out_bytes:u64[1]> err_off:i64[1]> flags",
    "zip_read": "ctx in in_len sel:u32[n_sel]< n_sel n_cap out cap out_off:u64[n_cap+1]> out_len:u64[n_cap]> "
                "status:i32[n_cap]> err_off:i64[n_cap]> n_entries:u32[1]> archive_err_off:i64[1]> flags",
}
DTYPES = {"u8": np.uint8, "u32": np.uint32, "u64": np.uint64, "i32": np.int32, "i64": np.int64, "f32": np.float32,
          "zip": engine.ZIP_ENTRY}


def _parse(sig):
    args = []
    for tok in sig.split():
        name, _, rest = tok.partition(":")
        if rest:
            typ, _, count = rest[:-1].partition("[")
            args.append((name, DTYPES[typ], count.rstrip("]"), rest[-1]))
        else:
            args.append((name, None, None, None))
    return args


SIGNATURES = {"flate_hip_" + k: _parse(v) for k, v in SIGNATURES.items()}


def _view(addr, dtype, count):
    """The table of `count` entries at a raw address, as a numpy array over that memory."""
    nbytes = count * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * nbytes).from_address(addr), dtype=dtype)


def _fill(k):
    """The k bytes a responder writes into an output buffer."""
    return (np.arange(k) * 7 + 1).astype(np.uint8)


def _head(lib, addr, host):
    """How many bytes a responder wrote at addr, if `host` (the buffer there, as numpy) still begins with them."""
    k = min(lib.written.get(addr, 0), host.size)
    return k if np.array_equal(host[:k], _fill(k)) else host[:k].tobytes().hex()


def _address(x):
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if isinstance(x, C.c_void_p):
        return x.value or 0
    if hasattr(x, "_obj"):  # ctypes.byref(...)
        return C.addressof(x._obj)
    return C.addressof(x)


class RecordingLibrary:
    def __init__(self, real, script):
        self._real = real
        self.script = {k: [dict(a) for a in v] for k, v in (script or {}).items()}
        self.trace = []
        self.labels = {}   # address -> "data" / "out": the buffers the scenario itself supplied
        self.written = {}  # address of an output buffer -> bytes a responder wrote there

    def __getattr__(self, name):
        if not name.startswith("flate_hip_"):
            raise AttributeError(name)
        fn = getattr(self._real, name)
        if name in PASS_THROUGH:
            return fn
        return lambda *args: self._call(name, fn.argtypes, args)

    def _call(self, name, argtypes, args):
        sig = SIGNATURES[name]
        assert len(args) == len(argtypes) == len(sig), name
        rec, val, reads = {}, {}, {}
        for (arg, _, _, _), t, x in zip(sig, argtypes, args):
            if t is C.c_char_p:
                rec[arg] = x.decode()
            elif issubclass(t, (C._Pointer, C.c_void_p)):
                val[arg] = _address(x)
                rec[arg] = self.labels.get(val[arg], "ptr" if val[arg] else "null")
            else:
                rec[arg] = val[arg] = int(x)
        queue = self.script.get(name.replace("flate_hip_", ""), [{}])
        answer = queue.pop(0) if len(queue) > 1 else queue[0]
        if name.endswith("_open") and not answer.get("rc"):
            answer = dict(answer, stream=HANDLE)
        for arg, dtype, count, way in sig:
            if way is None or not val[arg]:
                continue
            if way == "<":
                reads[arg] = _view(val[arg], dtype, eval(count, {}, val)).tolist()
            elif arg in answer:
                given = np.atleast_1d(np.array([tuple(v) for v in answer[arg]] if dtype is engine.ZIP_ENTRY
                                               else answer[arg], dtype=dtype))
                k = given.size if count == "*" else min(given.size, eval(count, {}, val))
                _view(val[arg], dtype, k)[:] = given[:k]
        if val.get("out") and "out" in answer:
            room = val["cap"] if "cap" in val else (reads["out_off"][-1] if "out_off" in reads else answer["out"])
            k = min(int(answer["out"]), int(room))
            _view(val["out"], np.uint8, k)[:] = _fill(k)
            self.written[val["out"]] = k
        # (the arguments by position: SIGNATURES has their names)
        self.trace.append([name[len("flate_hip_"):], list(rec.values())] + ([reads] if reads else []))
        if name == "flate_hip_last_hip_error":
            return answer.get("text", "").encode()
        return answer.get("rc", 0)


class FakeDeviceTensor:
    """A CPU torch.uint8 tensor that says it is a CUDA tensor: enough for engine.py to take its device branch here."""
    __module__ = "torch.stand_in"
    is_cuda = True

    def __init__(self, t):
        self._t = t

    dtype = property(lambda self: self._t.dtype)
    device = property(lambda self: self._t.device)

    def is_contiguous(self):
        return self._t.is_contiguous()

    def numel(self):
        return self._t.numel()

    def data_ptr(self):
        return self._t.data_ptr()

    def cpu(self):
        return self._t

    def __getitem__(self, k):
        return FakeDeviceTensor(self._t[k])


PATTERN = ((np.arange(200) * 37 + 11) % 251).astype(np.uint8)  # the input bytes of every scenario


class Env:
    """One scenario's engine, its recording library and the buffers it hands in."""

    def __init__(self, script, device):
        self.lib = RecordingLibrary(_lib.load(), script)
        self.device = device
        self.eng = engine.FlateEngine.__new__(engine.FlateEngine)
        self.eng._L, self.eng._ctx, self.eng.device = self.lib, C.c_void_p(CTX), 0
        self._keep = []

    def _buffer(self, a, label, device):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if device:
            import torch
            a = FakeDeviceTensor(torch.from_numpy(a))
        self._keep.append(a)
        if a.numel() if device else a.size:  # (an empty buffer has no address of its own)
            self.lib.labels[a.data_ptr() if device else a.ctypes.data] = label
        return a

    def data(self, n=200, tail=None, device=None):
        """n input bytes (tail: the little-endian number in the last four, where a gzip member keeps ISIZE)."""
        a = PATTERN[:n].copy()
        if tail is not None:
            a[n - 4:] = np.frombuffer(int(tail).to_bytes(4, "little"), dtype=np.uint8)
        return self._buffer(a, "data", self.device if device is None else device)

    def members(self, sizes):
        """Three "gzip members" over 200 bytes whose last four bytes say sizes[i]."""
        a = PATTERN.copy()
        for end, s in zip(IN_OFF[1:], sizes):
            a[end - 4:end] = np.frombuffer(int(s).to_bytes(4, "little"), dtype=np.uint8)
        return self._buffer(a, "data", self.device)

    def out(self, n, device=None, dtype=np.uint8):
        if dtype is not np.uint8:
            a = np.zeros(n, dtype=dtype)
            self._keep.append(a)
            self.lib.labels[a.ctypes.data] = "out"
            return a
        return self._buffer(np.zeros(n, np.uint8), "out", self.device if device is None else device)


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def serialise(x, lib):
    """A method's result as JSON: {"t": [...]} a tuple, {"<namedtuple>": [fields]}, {"<dtype>": contents} a numpy array,
    {"numpy" | "tensor": [size, head]} a uint8 buffer on the host or the device side -- head: how many of a responder's
    bytes it begins with (the rest of a buffer the engine allocated is not part of any contract) -- and {"bytes": head}."""
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, (bytes, bytearray)):
        k = len(x)
        return {"bytes": k if np.array_equal(np.frombuffer(x, dtype=np.uint8), _fill(k)) else bytes(x).hex()}
    if _is_tensor(x):
        assert "uint8" in str(x.dtype)
        return {"tensor": [int(x.numel()), _head(lib, x.data_ptr(), x.cpu().numpy())]}
    if isinstance(x, np.ndarray) and x.dtype == np.uint8:
        return {"numpy": [int(x.size), _head(lib, x.ctypes.data, x)]}
    if isinstance(x, np.ndarray):
        return {x.dtype.str if x.dtype.names is None else "ZIP_ENTRY": json.loads(json.dumps(x.tolist()))}
    if isinstance(x, tuple) and hasattr(x, "_fields"):
        return {type(x).__name__: [serialise(v, lib) for v in x]}
    if isinstance(x, tuple):
        return {"t": [serialise(v, lib) for v in x]}
    if isinstance(x, list):
        return [serialise(v, lib) for v in x]
    if isinstance(x, dict):
        return {"dict": {k: serialise(v, lib) for k, v in x.items()}}
    raise TypeError(type(x))


SCENARIOS = {}  # name -> (function(env) -> result, script, device)
IN_OFF = [0, 50, 120, 200]
SIZES = [10, 20, 30]
E = engine
PER_STREAM = (E.E_OUT_TOO_SMALL, E.E_CORRUPT, E.E_UNEXPECTED_EOF)
BAD = E.E_INTERNAL  # tolerated by no method


def add(name, fn, script=None, device=False):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = (fn, script or {}, device)


def with_rc(script, rc, only=None):
    """The script with rc as the answer of every call (only: of that entry point's calls)."""
    return {k: [dict(a, rc=rc) for a in v] if only in (None, k) else v for k, v in script.items()}


def family(name, call, script, entry, tolerated=(), single=None, outs=None, out_cap=True, need=0, empty=None,
           bytes_ok=False):
    """The scenarios every method gets.  call(env, data, **kw) is the method on its plain arguments; single (default:
    call) a form of it that makes ONE library call, for the statuses; outs: the method takes out= (a buffer of `outs`
    bytes suffices), out_cap: and out_cap=; need: what _check_out asks of a supplied out."""
    single = single or call
    add(name + "/host", lambda e: call(e, e.data()), script)
    add(name + "/dev", lambda e: call(e, e.data()), script, device=True)
    for rc in tolerated:
        add("%s/status%d" % (name, rc), lambda e: single(e, e.data()), with_rc(script, rc, entry))
    add(name + "/raises", lambda e: single(e, e.data()), with_rc({**script, entry: script.get(entry, [{}])}, BAD, entry))
    if empty:
        add(name + "/empty", empty, script)
    if bytes_ok:
        add(name + "/bytes", lambda e: call(e, bytes(range(200))), script)
    if outs is None:
        return
    for dev in (False, True):
        add(name + "/out" + ("/dev" if dev else ""), lambda e: call(e, e.data(), out=e.out(outs)), script, device=dev)
    if out_cap:
        add(name + "/out_cap_smaller", lambda e: call(e, e.data(), out=e.out(outs), out_cap=outs - 7), script)
        add(name + "/out_cap_larger", lambda e: call(e, e.data(), out=e.out(outs), out_cap=outs + 999), script)
        add(name + "/out_cap_alone", lambda e: call(e, e.data(), out_cap=outs + 5), script)
    add(name + "/out_wrong_dtype", lambda e: call(e, e.data(), out=e.out(outs, dtype=np.uint16)), script)
    add(name + "/out_numpy_for_tensor", lambda e: call(e, e.data(), out=e.out(outs, device=False)), script, device=True)
    add(name + "/out_tensor_for_numpy", lambda e: call(e, e.data(), out=e.out(outs, device=True)), script)
    if need:
        add(name + "/out_too_small", lambda e: call(e, e.data(), out=e.out(need - 1)), script)


def build_scenarios():
    one_dict, two_dicts = b"d" * 40, [b"a" * 10, np.frombuffer(b"b" * 20, dtype=np.uint8)]
    dict_of = [0, 1, E.NO_DICT]
    streams = {"out_len": SIZES, "status": [0, 0, 0], "err_off": [-1, -1, -1], "out": 60}
    failing = {"out_len": [10, 3, 30], "status": [0, E.E_CORRUPT, 0], "err_off": [-1, 17, -1], "out": 60}

    # ---- the engine's own small calls
    add("use_stream", lambda e: [e.eng.use_stream(0), e.eng.use_stream(0x5550)])
    add("set_option", lambda e: e.eng.set_option("guest_blocks", 3))
    add("set_option/raises", lambda e: e.eng.set_option("nonsense", 1),
        {"set_option": [{"rc": E.E_INVALID}], "last_hip_error": [{"text": "hipErrorSomething"}]})
    add("set_profiling", lambda e: [e.eng.set_profiling(), e.eng.set_profiling(False)])
    add("last_resident_share", lambda e: e.eng.last_resident_share(),
        {"last_resident_share": [{"resident": 5, "queued": 9}]})
    add("last_timing", lambda e: e.eng.last_timing(), {"last_timing": [{"ms": [0.5, 1.5, 0.25, 2.0]}]})
    add("close", lambda e: [e.eng.close(), e.eng.close()])

    def registered(e):
        with e.eng.host_register(e.data(device=False)) as reg:
            return reg.ptr is not None
    add("host_register", registered)
    add("host_register/raises", registered, {"host_register": [{"rc": BAD}]})

    # ---- deflate
    batch = {"deflate_fast_batch": [{"out": 90, "out_off": [0, 30, 60, 90]}],
             "deflate_fast_batch_dict": [{"out": 90, "out_off": [0, 30, 60, 90]}]}
    family("deflate_batch", lambda e, d, **k: e.eng.deflate_batch(d, IN_OFF, **k), batch, "deflate_fast_batch",
           outs=300, need=1, empty=lambda e: e.eng.deflate_batch(e.data(0), [0]))
    add("deflate_batch/flags", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, compat_go=True, lz_serial=True), batch)
    add("deflate_batch/small_out_cap", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, out_cap=5), batch)
    add("deflate_batch/one_dict", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, zdicts=one_dict), batch)
    add("deflate_batch/dict_list", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, zdicts=two_dicts, dict_of=dict_of),
        batch)
    add("deflate_batch/device_dict", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, zdicts=e.out(40)), batch,
        device=True)
    add("deflate_batch/dict_raises", lambda e: e.eng.deflate_batch(e.data(), IN_OFF, zdicts=one_dict),
        with_rc(batch, BAD))

    family("checksum_batch", lambda e, d: e.eng.checksum_batch(d, IN_OFF), {"checksum_batch": [{"sums": [7, 8, 9]}]},
           "checksum_batch", empty=lambda e: e.eng.checksum_batch(e.data(0), [0]))
    add("checksum_batch/crc32", lambda e: e.eng.checksum_batch(e.data(), IN_OFF, "crc32"),
        {"checksum_batch": [{"sums": [7, 8, 9]}]})
    add("checksum_batch/empty_streams", lambda e: e.eng.checksum_batch(e.data(0), [0, 0, 0]),
        {"checksum_batch": [{"sums": [1, 1]}]})

    framed = {"deflate_fast_batch_framed": [{"out": 108, "out_off": [0, 36, 72, 108]}]}
    for wrap in ("zlib", "gzip", "raw", "anything else"):
        family("deflate_batch_framed/" + wrap, lambda e, d, wrap=wrap, **k: e.eng.deflate_batch_framed(d, IN_OFF, wrap, **k),
               framed, "deflate_fast_batch_framed", outs=300 if wrap == "zlib" else None,
               empty=lambda e, wrap=wrap: e.eng.deflate_batch_framed(e.data(0), [0], wrap))
    add("deflate_batch_framed/one_dict", lambda e: e.eng.deflate_batch_framed(e.data(), IN_OFF, "zlib", zdicts=one_dict),
        framed)
    add("deflate_batch_framed/dict_list",
        lambda e: e.eng.deflate_batch_framed(e.data(), IN_OFF, "zlib", compat_go=True, zdicts=two_dicts, dict_of=dict_of),
        framed)
    add("deflate_batch_framed/gzip_dict", lambda e: e.eng.deflate_batch_framed(e.data(), IN_OFF, "gzip", zdicts=one_dict),
        framed)

    spliced = {"deflate_fast_spliced": [{"out": 70, "out_len": 70, "bit_off": [0, 180, 370, 555]}],
               "deflate_fast_spliced_framed": [{"out": 70, "out_len": 70, "bit_off": [0, 180, 370, 555]}]}
    family("deflate_spliced", lambda e, d, **k: e.eng.deflate_spliced(d, IN_OFF, **k), spliced, "deflate_fast_spliced",
           outs=300, out_cap=False, need=8, empty=lambda e: e.eng.deflate_spliced(e.data(0), [0]))
    add("deflate_spliced/compat_go", lambda e: e.eng.deflate_spliced(e.data(), IN_OFF, compat_go=True), spliced)
    for wrap in ("zlib", "gzip"):
        family("deflate_spliced_framed/" + wrap,
               lambda e, d, wrap=wrap, **k: e.eng.deflate_spliced_framed(d, IN_OFF, wrap, **k), spliced,
               "deflate_fast_spliced_framed", outs=300 if wrap == "gzip" else None,
               empty=lambda e, wrap=wrap: e.eng.deflate_spliced_framed(e.data(0), [0], wrap))
    add("deflate_spliced_framed/index",
        lambda e: e.eng.deflate_spliced_framed(e.data(), IN_OFF, "zlib", compat_go=True, index=True), spliced)

    add("lz77_matches", lambda e: e.eng.lz77_matches(e.data(), IN_OFF, compat_go=True),
        {"lz77_matches": [{"n_chunks": 2, "n_recs_cap": 3},
                          {"n_chunks": 2, "n_recs_cap": 3, "chunk_nmatch": [1, 2], "chunk_rec_off": [0, 1, 3],
                           "recs": [4, 100, 9, 200, 30, 300]}]})
    add("lz77_matches/none", lambda e: e.eng.lz77_matches(e.data(), IN_OFF))
    add("lz77_matches/raises", lambda e: e.eng.lz77_matches(e.data(), IN_OFF), {"lz77_matches": [{"rc": BAD}]})

    # ---- batch inflate
    inflate = {"inflate_batch": [streams], "inflate_batch_dict": [streams]}
    for check in (True, False):
        tag = "inflate_batch" + ("" if check else "/unchecked")
        family(tag, lambda e, d, check=check, **k: e.eng.inflate_batch(d, IN_OFF, SIZES, check=check, **k),
               {k: [failing] for k in inflate} if not check else inflate, "inflate_batch",
               tolerated=() if check else PER_STREAM, outs=100 if check else None, out_cap=False, need=60,
               empty=lambda e, check=check: e.eng.inflate_batch(e.data(0), [0], [], check=check))
    for rc in PER_STREAM:
        add("inflate_batch/checked_status%d" % rc, lambda e: e.eng.inflate_batch(e.data(), IN_OFF, SIZES),
            with_rc(inflate, rc))
    add("inflate_batch/one_dict", lambda e: e.eng.inflate_batch(e.data(), IN_OFF, SIZES, zdicts=one_dict), inflate)
    add("inflate_batch/dict_list",
        lambda e: e.eng.inflate_batch(e.data(), IN_OFF, SIZES, zdicts=two_dicts, dict_of=dict_of), inflate)
    add("inflate_batch/dict_unchecked",
        lambda e: e.eng.inflate_batch(e.data(), IN_OFF, SIZES, check=False, zdicts=one_dict), with_rc(inflate, E.E_CORRUPT))

    sizes = {"inflate_batch": [dict(streams, out=0)], "inflate_batch_dict": [dict(streams, out=0)]}
    family("inflate_sizes", lambda e, d: e.eng.inflate_sizes(d, IN_OFF), sizes, "inflate_batch", tolerated=PER_STREAM,
           empty=lambda e: e.eng.inflate_sizes(e.data(0), [0]))
    add("inflate_sizes/dict_list", lambda e: e.eng.inflate_sizes(e.data(), IN_OFF, zdicts=two_dicts, dict_of=dict_of),
        sizes)
    add("inflate_sizes/lax_tensor",  # no assertion on a tensor here: one that is not contiguous uint8 goes through
        lambda e: e.eng.inflate_sizes(e.data()[::2], [0, 100]), sizes, device=True)

    pieces = {"inflate_spliced": [streams],
              "inflate_spliced_framed": [dict(streams, member_status=0, member_err_off=-1)]}
    bits = [0, 180, 370, 555]
    for check in (True, False):
        family("inflate_spliced" + ("" if check else "/unchecked"),
               lambda e, d, check=check, **k: e.eng.inflate_spliced(d, 70, bits, SIZES, check=check, **k), pieces,
               "inflate_spliced", tolerated=() if check else PER_STREAM, outs=100 if check else None, out_cap=False,
               need=60, empty=lambda e, check=check: e.eng.inflate_spliced(e.data(0), 0, [0], [], check=check))
        family("inflate_spliced_framed" + ("" if check else "/unchecked"),
               lambda e, d, check=check, **k: e.eng.inflate_spliced_framed(d, 70, "zlib", bits, SIZES, check=check, **k),
               pieces, "inflate_spliced_framed", tolerated=() if check else PER_STREAM, outs=100 if check else None,
               out_cap=False, need=60,
               empty=lambda e, check=check: e.eng.inflate_spliced_framed(e.data(20), 20, "gzip", [80], [], check=check))
    add("inflate_spliced_framed/member_status",
        lambda e: e.eng.inflate_spliced_framed(e.data(), 70, "gzip", bits, SIZES, check=False),
        {"inflate_spliced_framed": [dict(failing, member_status=E.E_CORRUPT, member_err_off=66, rc=E.E_CORRUPT)]})

    read = {"inflate_batch_framed": [dict(streams, dict_used=[E.NO_DICT, 0, 1])]}
    sized = {"inflate_batch_framed": [{"out_len": SIZES, "status": [0, 0, 0]}, dict(streams, dict_used=[E.NO_DICT] * 3)]}
    family("inflate_batch_framed/sizes_given",
           lambda e, d, **k: e.eng.inflate_batch_framed(d, IN_OFF, "zlib", out_sizes=SIZES, **k), read,
           "inflate_batch_framed", tolerated=PER_STREAM, outs=100, out_cap=False, need=60,
           empty=lambda e: e.eng.inflate_batch_framed(e.data(0), [0], "zlib", out_sizes=[]))
    family("inflate_batch_framed/zlib_sized_by_a_pass", lambda e, d, **k: e.eng.inflate_batch_framed(d, IN_OFF, "zlib", **k),
           sized, "inflate_batch_framed", outs=100, out_cap=False, need=60,
           empty=lambda e: e.eng.inflate_batch_framed(e.data(0), [0], "zlib"))
    add("inflate_batch_framed/zlib_pass_fails", lambda e: e.eng.inflate_batch_framed(e.data(), IN_OFF, "zlib"),
        {"inflate_batch_framed": [{"out_len": [10, 3, 30], "status": [0, -4, 0], "rc": E.E_CORRUPT},
                                  dict(failing, rc=E.E_CORRUPT)]})
    for dev in (False, True):
        add("inflate_batch_framed/gzip" + ("/dev" if dev else ""),
            lambda e: e.eng.inflate_batch_framed(e.members(SIZES), IN_OFF, "gzip"), read, device=dev)
    add("inflate_batch_framed/gzip_short_member",
        lambda e: e.eng.inflate_batch_framed(e.members(SIZES), [0, 50, 60, 200], "gzip"), read)
    add("inflate_batch_framed/gzip_all_short", lambda e: e.eng.inflate_batch_framed(e.data(30), [0, 10, 20, 30], "gzip"),
        read)
    add("inflate_batch_framed/gzip_empty", lambda e: e.eng.inflate_batch_framed(e.data(0), [0], "gzip"), read)
    add("inflate_batch_framed/one_dict",
        lambda e: e.eng.inflate_batch_framed(e.data(), IN_OFF, "zlib", out_sizes=SIZES, zdicts=one_dict), read)
    add("inflate_batch_framed/dict_list",
        lambda e: e.eng.inflate_batch_framed(e.data(), IN_OFF, "zlib", out_sizes=SIZES, zdicts=two_dicts), read)
    add("inflate_batch_framed/gzip_ignores_dicts",
        lambda e: e.eng.inflate_batch_framed(e.members(SIZES), IN_OFF, "gzip", zdicts=one_dict), read)

    # ---- streams in pieces
    def written(e):
        w = e.eng.open_stream(compat_go=True)
        first = w.write(e.data(device=False))
        last = w.close(b"tail")
        w.free()
        return first, last
    add("stream_writer", written, {"stream_write": [{"out": 44, "out_len": 44}, {"out": 9, "out_len": 9}]})
    add("stream_writer/empty_tail", lambda e: e.eng.open_stream().close(), {"stream_write": [{"out": 5, "out_len": 5}]})
    add("stream_writer/array_tail", lambda e: e.eng.open_stream().close(e.data(device=False)),
        {"stream_write": [{"out": 5, "out_len": 5}]})
    add("stream_writer/open_raises", lambda e: e.eng.open_stream(), {"stream_open": [{"rc": BAD}]})
    add("stream_writer/write_raises", written, {"stream_write": [{"rc": E.E_INVALID}]})

    def fed(e):
        r = e.eng.open_inflate_stream(zdict=b"z" * 30)
        a = r.feed(e.data(device=False), room=64)
        state = (r.pending_input, r.total_in, r.err_off)
        b = r.feed(b"more", final=True, room=0)
        c = r.feed(b"")
        state2 = (r.pending_input, r.total_in, r.err_off)
        r.reset()
        r.reset(np.frombuffer(b"y" * 8, dtype=np.uint8))
        r.free()
        r.free()
        return a, state, b, c, state2
    add("stream_reader", fed, {"inflate_stream_read": [
        {"out": 64, "out_len": 64, "in_used": 150}, {"out": 0, "in_used": 54, "out_len": 0, "rc": 1},
        {"rc": E.E_CORRUPT, "err_off": 12}]})
    add("stream_reader/no_dict", lambda e: e.eng.open_inflate_stream(b"").feed(e.data(device=False), final=True),
        {"inflate_stream_read": [{"out": 10, "out_len": 10, "in_used": 200, "rc": E.E_UNEXPECTED_EOF}]})
    add("stream_reader/open_raises", lambda e: e.eng.open_inflate_stream(), {"inflate_stream_open": [{"rc": BAD}]})
    add("stream_reader/reset_raises", lambda e: e.eng.open_inflate_stream(b"dict"), {"inflate_stream_reset": [{"rc": BAD}]})
    add("stream_reader/read_raises", lambda e: e.eng.open_inflate_stream().feed(b"abc"),
        {"inflate_stream_read": [{"rc": E.E_OUT_TOO_SMALL}]})

    # ---- BGZF
    bgzf_w = {"bgzf_write": [{"out": 80, "out_len": 80, "member_off": [0, 52]}]}
    family("bgzf_write", lambda e, d, **k: e.eng.bgzf_write(d, **k), bgzf_w, "bgzf_write", outs=400, bytes_ok=True)
    add("bgzf_write/empty", lambda e: e.eng.bgzf_write(e.data(0)), {"bgzf_write": [{"out": 28, "out_len": 28, "member_off": [0]}]})
    add("bgzf_write/index", lambda e: e.eng.bgzf_write(e.data(), block_bytes=64, compat_go=True, index=True),
        {"bgzf_write": [{"out": 80, "out_len": 80, "member_off": [0, 10, 20, 30, 52]}]})
    add("bgzf_write/index/dev", lambda e: e.eng.bgzf_write(e.data(), index=True), bgzf_w, device=True)
    add("bgzf_write/bad_block_bytes", lambda e: e.eng.bgzf_write(e.data(), block_bytes=70000), bgzf_w)
    add("bgzf_write/tiny_out_cap", lambda e: e.eng.bgzf_write(e.data(), out_cap=3), with_rc(bgzf_w, E.E_OUT_TOO_SMALL))

    counts = {"n_members": 2, "out_bytes": 100, "eof_marker": 1, "n_candidates": 7}
    filled = dict(counts, member_off=[0, 90, 172], out_off=[0, 40, 100])
    for kind, idx_ok in (("bgzf", (E.E_CORRUPT, E.E_OUT_TOO_SMALL)),
                         ("gzip", (E.E_CORRUPT, E.E_UNEXPECTED_EOF, E.E_TOO_LARGE, E.E_OUT_TOO_SMALL))):
        index = lambda e, d, kind=kind, **k: getattr(e.eng, kind + "_index")(d, **k)
        ientry, rentry = kind + "_index", kind + "_read"
        family(ientry, index, {ientry: [counts, filled]}, ientry, bytes_ok=True,
               tolerated=idx_ok, single=lambda e, d, index=index: index(e, d, index_cap=3),
               empty=lambda e, index=index: index(e, e.data(0)))
        add(ientry + "/query", lambda e, index=index: index(e, e.data(), query=True), {ientry: [counts]})
        add(ientry + "/query/dev", lambda e, index=index: index(e, e.data(), query=True), {ientry: [counts]}, device=True)
        for rc in idx_ok:
            broken = dict(counts, rc=rc, err_off=90, n_members=1)
            add("%s/query_status%d" % (ientry, rc), lambda e, index=index: index(e, e.data(), query=True), {ientry: [broken]})
            add("%s/sized_by_query_status%d" % (ientry, rc), lambda e, index=index: index(e, e.data()),
                {ientry: [broken, dict(broken, member_off=[0, 90], out_off=[0, 40])]})
        add(ientry + "/cap_too_small", lambda e, index=index: index(e, e.data(), index_cap=2),
            {ientry: [dict(filled, rc=E.E_OUT_TOO_SMALL)]})
        add(ientry + "/cap_larger", lambda e, index=index: index(e, e.data(), index_cap=9), {ientry: [filled]})
        add(ientry + "/cap_zero", lambda e, index=index: index(e, e.data(), index_cap=0),
            {ientry: [dict(counts, rc=E.E_OUT_TOO_SMALL)]})

        got = {"out": 100, "out_len": 100, "n_members": 2, "bad_member": 2, "eof_marker": 1}
        rd = lambda e, d, kind=kind, **k: getattr(e.eng, kind + "_read")(d, **k)
        family(rentry, rd, {ientry: [counts], rentry: [got]}, rentry, bytes_ok=True,
               tolerated=PER_STREAM + ((E.E_TOO_LARGE,) if kind == "gzip" else ()),
               single=lambda e, d, rd=rd: rd(e, d, out=e.out(120)), outs=120, empty=lambda e, rd=rd: rd(e, e.data(0)))
        add(rentry + "/query_fails", lambda e, rd=rd: rd(e, e.data()),
            {ientry: [dict(rc=E.E_CORRUPT, n_members=1, out_bytes=40, err_off=90)],
             rentry: [dict(rc=E.E_CORRUPT, n_members=1, bad_member=1, err_off=90)]})
        add(rentry + "/query_raises", lambda e, rd=rd: rd(e, e.data()), {ientry: [{"rc": BAD}]})

    rng = {"bgzf_read_ranges": [{"rc": E.E_OUT_TOO_SMALL, "out_off": [0, 5, 25], "n_members": 2},
                                {"out": 25, "out_off": [0, 5, 25], "range_status": [0, 0], "n_members": 2,
                                 "n_decoded": 1, "bad_member": 2}]}
    ranges = lambda e, d, **k: e.eng.bgzf_read_ranges(d, [0, 10], [5, 30], **k)
    with_out = lambda e, d: ranges(e, d, out=e.out(64))
    family("bgzf_read_ranges", ranges, rng, "bgzf_read_ranges", tolerated=PER_STREAM, single=with_out, outs=64,
           bytes_ok=True, empty=lambda e: e.eng.bgzf_read_ranges(e.data(), [], []))
    add("bgzf_read_ranges/virtual", lambda e: e.eng.bgzf_read_ranges(e.data(), [1 << 16], [(90 << 16) | 7], virtual=True),
        {"bgzf_read_ranges": [{"rc": E.E_OUT_TOO_SMALL, "out_off": [0, 47]}, {"out": 47, "out_off": [0, 47]}]})
    add("bgzf_read_ranges/nothing_to_deliver", lambda e: ranges(e, e.data()),
        {"bgzf_read_ranges": [{"out_off": [0, 0, 0], "n_members": 2}]})
    add("bgzf_read_ranges/nothing_to_deliver/dev", lambda e: ranges(e, e.data()),
        {"bgzf_read_ranges": [{"out_off": [0, 0, 0], "n_members": 2}]}, device=True)
    add("bgzf_read_ranges/malformed_chain", lambda e: ranges(e, e.data()),
        {"bgzf_read_ranges": [{"rc": E.E_CORRUPT, "out_off": [0, 5, 25], "n_members": 1, "bad_member": 1, "err_off": 90}]})
    add("bgzf_read_ranges/invalid_range", lambda e: with_out(e, e.data()),
        {"bgzf_read_ranges": [{"rc": E.E_INVALID, "out": 5, "out_off": [0, 5, 5], "range_status": [0, E.E_INVALID]}]})
    add("bgzf_read_ranges/invalid_call", lambda e: with_out(e, e.data()),
        {"bgzf_read_ranges": [{"rc": E.E_INVALID, "range_status": [0, 0]}]})
    add("bgzf_read_ranges/invalid_no_ranges", lambda e: e.eng.bgzf_read_ranges(e.data(), [], [], out=e.out(16)),
        {"bgzf_read_ranges": [{"rc": E.E_INVALID}]})
    add("bgzf_read_ranges/shapes_differ", lambda e: e.eng.bgzf_read_ranges(e.data(), [0, 1], [5]))
    add("bgzf_read_ranges/two_dimensional", lambda e: e.eng.bgzf_read_ranges(e.data(), [[0]], [[5]]))

    # ---- one long stream
    one_counts = {"n_units": 3, "out_bytes": 900, "n_candidates": 11, "status": 0}
    one_filled = dict(one_counts, unit_bit=[0, 500, 900, 1500], out_off=[0, 300, 600, 900])
    oidx = lambda e, d, **k: e.eng.inflate_one_index(d, **k)
    family("inflate_one_index", oidx, {"inflate_one_index": [one_filled]}, "inflate_one_index", bytes_ok=True,
           tolerated=(E.E_CORRUPT, E.E_UNEXPECTED_EOF, E.E_TOO_LARGE, E.E_OUT_TOO_SMALL),
           empty=lambda e: oidx(e, e.data(0)))
    for wrap in ("raw", "zlib"):
        add("inflate_one_index/" + wrap, lambda e, wrap=wrap: oidx(e, e.data(), wrap=wrap), {"inflate_one_index": [one_filled]})
    add("inflate_one_index/unknown_wrap", lambda e: oidx(e, e.data(), wrap="lzma"))
    add("inflate_one_index/query", lambda e: oidx(e, e.data(), query=True), {"inflate_one_index": [one_counts]})
    add("inflate_one_index/query/dev", lambda e: oidx(e, e.data(), query=True), {"inflate_one_index": [one_counts]}, device=True)
    add("inflate_one_index/query_status", lambda e: oidx(e, e.data(), query=True),
        {"inflate_one_index": [dict(one_counts, rc=E.E_CORRUPT, status=E.E_CORRUPT, err_off=33)]})
    many = dict(n_units=100, out_bytes=5000, n_candidates=300)
    add("inflate_one_index/second_sizing_call", lambda e: oidx(e, e.data()),
        {"inflate_one_index": [dict(many, rc=E.E_OUT_TOO_SMALL),
                               dict(many, unit_bit=list(range(0, 808, 8)), out_off=list(range(0, 5050, 50)))]})
    add("inflate_one_index/second_call_too_small_again", lambda e: oidx(e, e.data()),
        {"inflate_one_index": [dict(many, rc=E.E_OUT_TOO_SMALL), dict(many, n_units=200, rc=E.E_OUT_TOO_SMALL)]})
    add("inflate_one_index/cap_too_small", lambda e: oidx(e, e.data(), index_cap=2),
        {"inflate_one_index": [dict(one_filled, rc=E.E_OUT_TOO_SMALL)]})
    add("inflate_one_index/cap_larger", lambda e: oidx(e, e.data(), index_cap=10), {"inflate_one_index": [one_filled]})
    add("inflate_one_index/good_prefix", lambda e: oidx(e, e.data(), index_cap=10),
        {"inflate_one_index": [dict(one_filled, rc=E.E_CORRUPT, status=E.E_CORRUPT, err_off=190)]})

    done = {"out": 120, "out_len": 120, "status": 0, "n_units": 3, "n_candidates": 11}
    one = lambda e, d, **k: e.eng.inflate_one(d, wrap="zlib", **k)
    family("inflate_one", one, {"inflate_one": [dict(done, rc=E.E_OUT_TOO_SMALL, out=0), done]}, "inflate_one",
           tolerated=PER_STREAM + (E.E_TOO_LARGE,), single=lambda e, d: one(e, d, out=e.out(150)), outs=150,
           bytes_ok=True)
    for dev in (False, True):
        tag = "/dev" if dev else ""
        add("inflate_one/hint_right" + tag, lambda e: e.eng.inflate_one(e.data(tail=120)), {"inflate_one": [done]}, device=dev)
        add("inflate_one/hint_too_small" + tag, lambda e: e.eng.inflate_one(e.data(tail=120)),
            {"inflate_one": [dict(done, rc=E.E_OUT_TOO_SMALL, out=0, out_len=500), dict(done, out=500, out_len=500)]},
            device=dev)
        add("inflate_one/nothing_to_deliver" + tag, lambda e: e.eng.inflate_one(e.data(0), wrap="raw"),
            {"inflate_one": [dict(rc=E.E_UNEXPECTED_EOF, status=E.E_UNEXPECTED_EOF)]}, device=dev)
    add("inflate_one/hint_right_but_corrupt", lambda e: e.eng.inflate_one(e.data(tail=120)),
        {"inflate_one": [dict(done, rc=E.E_CORRUPT, status=E.E_CORRUPT, err_off=200, out=100, out_len=100)]})
    add("inflate_one/hint_small_slot_overrun", lambda e: e.eng.inflate_one(e.data(tail=120)),
        {"inflate_one": [dict(done, rc=E.E_OUT_TOO_SMALL, out_len=120)]})
    add("inflate_one/hint_absurd", lambda e: e.eng.inflate_one(e.data(tail=1032 * 200 + 1)),
        {"inflate_one": [dict(done, rc=E.E_OUT_TOO_SMALL, out=0), done]})
    add("inflate_one/hint_zero", lambda e: e.eng.inflate_one(e.data(tail=0)), {"inflate_one": [dict(done, out=0, out_len=0)]})
    add("inflate_one/too_short_for_a_hint", lambda e: e.eng.inflate_one(e.data(17, tail=5)),
        {"inflate_one": [dict(rc=E.E_CORRUPT, status=E.E_CORRUPT, err_off=0)]})
    add("inflate_one/hint_ignored_with_out", lambda e: e.eng.inflate_one(e.data(tail=120), out=e.out(150), out_cap=130),
        {"inflate_one": [done]})
    add("inflate_one/unknown_wrap", lambda e: e.eng.inflate_one(e.data(), wrap="lzma"))

    # ---- ZIP
    names = ["a", b"bb", "c.txt"]
    zip_w = {"zip_write": [{"out": 150, "out_len": 150, "entry_off": [0, 40, 90, 130]}]}
    family("zip_write", lambda e, d, **k: e.eng.zip_write(d, IN_OFF, names, **k), zip_w, "zip_write", outs=600,
           bytes_ok=True)
    add("zip_write/empty", lambda e: e.eng.zip_write(e.data(0), [0], []), {"zip_write": [{"out": 22, "out_len": 22, "entry_off": [0]}]})
    add("zip_write/index", lambda e: e.eng.zip_write(e.data(), IN_OFF, names, compat_go=True, index=True), zip_w)
    add("zip_write/index/dev", lambda e: e.eng.zip_write(e.data(), IN_OFF, names, index=True), zip_w, device=True)
    add("zip_write/names_differ", lambda e: e.eng.zip_write(e.data(), IN_OFF, names[:2]), zip_w)
    add("zip_write/empty_name", lambda e: e.eng.zip_write(e.data(), IN_OFF, ["a", "", "c"]), zip_w)

    # (name_off, header_off, data_off, comp_size, size, crc32, name_len, method, flags, reserved, status, reserved2):
    # the names are data[30:31] and data[60:62]; byte 61 of the pattern is not UTF-8 after byte 60
    entries = [(30, 0, 31, 20, 10, 0xAABBCCDD, 1, 8, 0, 0, 0, 0), (60, 51, 62, 25, 20, 0x11223344, 2, 0, 0x800, 0, 0, 0)]
    zcount = {"n_entries": 2, "out_bytes": 30}
    zfill = dict(zcount, entries=entries, out_off=[0, 10, 30])
    zidx = {"zip_index": [zcount, zfill]}
    family("zip_index", lambda e, d: e.eng.zip_index(d), zidx, "zip_index", tolerated=(E.E_CORRUPT,), bytes_ok=True,
           empty=lambda e: e.eng.zip_index(e.data(0)))
    add("zip_index/no_entries", lambda e: e.eng.zip_index(e.data()), {"zip_index": [{"n_entries": 0, "out_off": [0]}]})
    add("zip_index/fill_fails", lambda e: e.eng.zip_index(e.data()), {"zip_index": [zcount, dict(zfill, rc=E.E_CORRUPT)]})

    def named(e, k):
        return [PATTERN[30:31].tobytes().decode(), PATTERN[60:62].tobytes()][k]
    zgot = {"out": 30, "out_off": [0, 10, 30], "out_len": [10, 20], "status": [0, 0], "err_off": [-1, -1], "n_entries": 2}
    zquery = dict(zgot, rc=E.E_OUT_TOO_SMALL, out=0)
    zall = {"zip_index": [zcount], "zip_read": [zquery, zgot]}
    zrd = lambda e, d, **k: e.eng.zip_read(d, **k)
    family("zip_read", zrd, zall, "zip_read", bytes_ok=True, outs=64, single=lambda e, d: zrd(e, d, out=e.out(64)),
           tolerated=PER_STREAM + (E.E_TOO_LARGE, E.E_UNSUPPORTED), empty=lambda e: zrd(e, e.data(0)))
    add("zip_read/index_fails", lambda e: zrd(e, e.data()), {"zip_index": [dict(rc=E.E_CORRUPT, n_entries=1, err_off=44)]})
    add("zip_read/index_fails/with_out", lambda e: zrd(e, e.data(), out=e.out(64)),
        {"zip_index": [dict(rc=E.E_CORRUPT, n_entries=1, err_off=44)]})
    add("zip_read/index_raises", lambda e: zrd(e, e.data()), {"zip_index": [{"rc": BAD}]})
    add("zip_read/nothing_to_deliver", lambda e: zrd(e, e.data()),
        {"zip_index": [zcount], "zip_read": [dict(zgot, rc=E.E_CORRUPT, out=0, archive_err_off=12)]})
    three = dict(out=40, out_off=[0, 20, 30, 50], out_len=[20, 10, 20], status=[0, 0, 0], err_off=[-1] * 3, n_entries=2)
    three = {"zip_index": [zcount, zfill], "zip_read": [dict(three, rc=E.E_OUT_TOO_SMALL, out=0), three]}
    for dev in (False, True):
        tag = "/dev" if dev else ""
        add("zip_read/by_number" + tag, lambda e: zrd(e, e.data(), select=[1, 0, np.uint32(1)]), three, device=dev)
        add("zip_read/by_name" + tag, lambda e: zrd(e, e.data(), select=[named(e, 1), 0, named(e, 1)]), three, device=dev)
    add("zip_read/by_number/out", lambda e: zrd(e, e.data(), select=(1, 0, 1), out=e.out(64), out_cap=60), three)
    add("zip_read/by_name/out", lambda e: zrd(e, e.data(), select=[named(e, 0).encode(), 1, 1], out=e.out(64)), three)
    add("zip_read/no_such_name", lambda e: zrd(e, e.data(), select=["nowhere"]), three)
    add("zip_read/by_name_index_fails", lambda e: zrd(e, e.data(), select=["a"], out=e.out(64)),
        {"zip_index": [dict(rc=E.E_CORRUPT, n_entries=1, err_off=44)]})
    add("zip_read/select_nothing", lambda e: zrd(e, e.data(), select=[]), {"zip_read": [dict(n_entries=2, out_off=[0])]})


build_scenarios()


def run(name):
    fn, script, device = SCENARIOS[name]
    env = Env(script, device)
    eng = env.eng
    try:
        res = {"ret": serialise(fn(env), env.lib)}
    except engine.FlateError as e:
        res = {"raises": "FlateError", "code": e.code, "msg": str(e)}
    except (ValueError, KeyError, AssertionError) as e:
        res = {"raises": type(e).__name__, "msg": "" if isinstance(e, AssertionError) else str(e)}
    for attr in ("last_framed_read", "last_member_err_off"):
        if hasattr(eng, attr):
            res[attr] = serialise(getattr(eng, attr), env.lib)
    res = json.loads(json.dumps({"trace": env.lib.trace, **res}))
    eng._ctx = None  # nothing to destroy
    return res


def run_all():
    return {name: run(name) for name in SCENARIOS}


if __name__ == "__main__":
    got = run_all()
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in got.items()) + "\n}\n")
    print("%d scenarios, %d calls -> %s" % (len(got), sum(len(v["trace"]) for v in got.values()), FIXTURE))
