"""Host-side handle of the MI355X batch DEFLATE engine (thin wrapper over the C ABI).

The C ABI (include/flate_hip.h) is the product boundary; this module only marshals
numpy / torch buffers into it.  PyTorch is used for device memory and streams only.

Every method resolves its buffers through the same few helpers: _in_buf for the
input, _out_buf for the output and the capacity the library is told, _stream_results for the per-stream tables,
FlateEngine._tolerate for the statuses a method hands back instead of raising, _query_then_fill for the index
calls and _read_into for the calls that size their output by a query.
"""
import collections
import ctypes as C
import os
import zlib

import numpy as np

from . import _lib

DEVICE_PTRS = 0x1
COMPAT_GO = 0x2
LZ_SERIAL = 0x4
SIZE_ONLY = 0x8
NO_DICT = 0xFFFFFFFF  # FLATE_HIP_NO_DICT: a stream of flate_hip_inflate_batch_dict without a dictionary

# status codes (include/flate_hip.h)
E_INVALID, E_OUT_TOO_SMALL, E_CORRUPT, E_UNEXPECTED_EOF, E_INTERNAL = -1, -2, -4, -7, -8
E_TOO_LARGE, E_UNSUPPORTED = -6, -10
# what a call returns when some stream, member or entry failed: the caller reads the verdicts, nothing is raised
PER_STREAM = (E_OUT_TOO_SMALL, E_CORRUPT, E_UNEXPECTED_EOF)
# ... and the index calls, whose chain can also break at a member or unit beyond the size limit
PER_CHAIN = PER_STREAM + (E_TOO_LARGE,)

CHECKSUM_ADLER32, CHECKSUM_CRC32 = 1, 2
CHECKSUMS = {"adler32": CHECKSUM_ADLER32, "crc32": CHECKSUM_CRC32}
WRAP_RAW, WRAP_ZLIB, WRAP_GZIP = 0, 1, 2  # FLATE_HIP_WRAP_*
WRAPS = {"raw": WRAP_RAW, "zlib": WRAP_ZLIB, "gzip": WRAP_GZIP}
ZLIB_HEADER = bytes([0x78, 0x01])  # CM = 8, CINFO = 7 (32 KiB window), FLEVEL = 0 (fastest), FCHECK (RFC 1950 2.2)
GZIP_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255])  # no name / time, XFL = 4 (fastest), OS unknown (RFC 1952 2.3)

SYNTH_RAMP, SYNTH_TEXT, SYNTH_RAND, SYNTH_ZERO = 0, 1, 2, 3
SYNTH_KINDS = {"ramp": SYNTH_RAMP, "text": SYNTH_TEXT, "rand": SYNTH_RAND, "zero": SYNTH_ZERO}
SEED_TEXT = 0x5EED0001
SEED_RAND = 0x5EED0002

STAGES = ("lz77_match", "huff_pack", "checksum", "inflate")

MAX_STORE_BLOCK_SIZE = 65535
MATCH_CAP_PER_CHUNK = 16384

BGZF_BLOCK_DEFAULT = 65280  # FLATE_HIP_BGZF_BLOCK_DEFAULT
BGZF_MEMBER_MAX = 65536
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BgzfIndex = collections.namedtuple("BgzfIndex", "rc n_members out_bytes eof_marker err_off member_off out_off")
BgzfRead = collections.namedtuple("BgzfRead", "rc out_len n_members bad_member err_off eof_marker")
BgzfRanges = collections.namedtuple("BgzfRanges", "rc out_off range_status n_members n_decoded bad_member err_off")
GZIP_MEMBER_MAX = (1 << 28) - 1  # the option "gzip_member_max": its default and its maximum
GzipIndex = collections.namedtuple("GzipIndex", "rc n_members out_bytes n_candidates err_off member_off out_off")
OneRead = collections.namedtuple("OneRead", "rc out_len status err_off n_units n_candidates")
OneIndex = collections.namedtuple("OneIndex", "rc n_units out_bytes n_candidates status err_off unit_bit out_off")
GzipRead = collections.namedtuple("GzipRead", "rc out_len n_members bad_member err_off")
SEEK_SPAN_DEFAULT = 1 << 20  # FLATE_HIP_SEEK_SPAN_DEFAULT
SEEK_SPAN_NONE = (1 << 64) - 1  # FLATE_HIP_SEEK_SPAN_NONE: unit 0 is the only point
SeekIndex = collections.namedtuple("SeekIndex", "rc index windows n_units n_points out_bytes status err_off")
OneRanges = collections.namedtuple("OneRanges", "rc out_off range_status n_decoded bad_unit")
SEEK_PACK_COMPRESS, SEEK_PACK_SPARSE = 1, 2  # FLATE_HIP_SEEK_PACK_*
SeekPack = collections.namedtuple("SeekPack", "rc pack_index packed packed_bytes kept_bytes")
SeekUnpack = collections.namedtuple("SeekUnpack", "rc windows_bytes bad_block")
GzFileIndex = collections.namedtuple("GzFileIndex", "rc n_units n_members out_bytes n_candidates status bad_member err_off "
                                     "stream_err_off unit_bit out_off member_off member_unit")
GzFileRead = collections.namedtuple("GzFileRead", "rc out_len n_members n_units n_candidates status bad_member err_off "
                                    "stream_err_off")
GzFileSeekIndex = collections.namedtuple("GzFileSeekIndex", "rc index windows n_units n_members n_points out_bytes "
                                         "n_candidates status bad_member err_off stream_err_off")

# flate_hip_zip_entry, as numpy sees it (64 bytes)
ZIP_ENTRY = np.dtype([("name_off", "<u8"), ("header_off", "<u8"), ("data_off", "<u8"), ("comp_size", "<u8"), ("size", "<u8"),
                      ("crc32", "<u4"), ("name_len", "<u2"), ("method", "<u2"), ("flags", "<u2"), ("reserved", "<u2"),
                      ("status", "<i4"), ("reserved2", "<u4")], align=True)
assert ZIP_ENTRY.itemsize == 64
ZipIndex = collections.namedtuple("ZipIndex", "rc n_entries out_bytes err_off entries out_off names")
ZipRead = collections.namedtuple("ZipRead", "rc out_off out_len status err_off n_entries archive_err_off")


class FlateError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("flate_hip error %d: %s" % (code, msg))
        self.code = code


def build_id():
    """Source hash compiled into the loaded library (see build.source_hash)."""
    return _lib.load().flate_hip_build_id().decode()


def deflate_bound(n):
    return int(_lib.load().flate_hip_deflate_bound(int(n)))


def _wrap_code(wrap):
    """FLATE_HIP_WRAP_* of the framed methods' wrap argument ("zlib", "raw"; anything else has always meant gzip)."""
    return WRAPS.get(wrap, WRAP_GZIP)


def frame_overhead(wrap, with_dict=False):
    """Bytes a zlib / gzip member adds around its raw stream (flate_hip_frame_overhead)."""
    return int(_lib.load().flate_hip_frame_overhead(_wrap_code(wrap) if isinstance(wrap, str) else int(wrap),
                                                    1 if with_dict else 0))


def bgzf_bound(n, block_bytes=0):
    """Room that always holds the BGZF file of n input bytes (flate_hip_bgzf_bound; 0: block_bytes is refused)."""
    return int(_lib.load().flate_hip_bgzf_bound(int(n), int(block_bytes)))


def _zip_names(names):
    """A list of str / bytes -> (the names back to back as numpy uint8, name_off as numpy uint64)."""
    raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), off


def zip_bound(in_off, names):
    """Room that always holds the ZIP archive of these entries (flate_hip_zip_bound; 0: a name would be refused)."""
    in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
    _, name_off = _zip_names(names)
    return int(_lib.load().flate_hip_zip_bound(in_off.ctypes.data, len(names), name_off.ctypes.data))


def synth(kind, n_streams, stream_len, seed=None, first_stream=0, nthreads=None):
    """Synthetic benchmark input: n_streams streams of stream_len bytes, back to back."""
    k = SYNTH_KINDS[kind] if isinstance(kind, str) else int(kind)
    if seed is None:
        seed = SEED_RAND if k == SYNTH_RAND else SEED_TEXT
    if nthreads is None:
        nthreads = min(16, os.cpu_count() or 1)
    out = np.empty(int(n_streams) * int(stream_len), dtype=np.uint8)
    rc = _lib.load().flate_hip_synth_fill(k, seed, first_stream, n_streams, stream_len,
                                          out.ctypes.data, nthreads)
    if rc != 0:
        raise FlateError(rc, "synth_fill")
    return out


def uniform_offsets(n_streams, stream_len):
    return (np.arange(n_streams + 1, dtype=np.uint64) * np.uint64(stream_len))


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _check_out(out, data, need, what):
    """A caller-supplied output buffer must be uint8, contiguous, on the same side (and device) as
    the input and hold at least `need` bytes: the kernels bound their writes by the slot table,
    not by the real size of `out`."""
    if _is_torch(data):
        import torch
        ok = _is_torch(out) and out.dtype == torch.uint8 and out.is_contiguous() and \
            out.device == data.device and out.numel() >= need
    else:
        ok = isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and \
            out.size >= need
    if not ok:
        raise FlateError(E_INVALID, "%s: out must be a contiguous uint8 buffer of >= %d bytes on the "
                                    "same device as the input" % (what, need))


def _in_buf(data, accept_bytes=False, lax=False, null_if_empty=False):
    """(data, pointer, bytes, device) of a call's input: a numpy uint8 array (made contiguous; with accept_bytes also
    bytes / bytearray) or a torch uint8 CUDA tensor, which must be contiguous (lax: checksum_batch and inflate_sizes
    have never asserted that).  null_if_empty: the single-buffer calls hand the library NULL for no input at all;
    the batch calls, whose offset table says that there is none, hand it the buffer's address whatever its size."""
    device = _is_torch(data)
    if device:
        if not lax:
            import torch
            assert data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()
        ptr, nbytes = data.data_ptr(), data.numel()
    else:
        if accept_bytes and isinstance(data, (bytes, bytearray)):
            data = np.frombuffer(data, dtype=np.uint8)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        ptr, nbytes = data.ctypes.data, data.size
    return data, (None if null_if_empty and not nbytes else ptr), nbytes, device


def _out_buf(out, data, size, out_cap, need, what, floor=16):
    """(out, pointer, capacity) of a call's output.  out=None: room for `size` bytes (at least `floor`) on the side
    of `data` -- zeroed on the host, torch.empty on the device; otherwise the caller's buffer, which _check_out
    wants to be of data's kind and of at least `need` bytes.  The capacity is what the library is told: the
    buffer's size, cut to out_cap where the method has one and the caller gave it.  (deflate_batch and
    deflate_spliced pass out_cap=None: they have always told the library the whole buffer.  The inflate calls take
    no capacity at all: their slot table bounds every write, which is why `need` is that table's end for them.)"""
    device = _is_torch(data)
    if out is not None:
        _check_out(out, data, need, what)
    elif device:
        import torch
        out = torch.empty(max(int(size), floor), dtype=torch.uint8, device=data.device)
    else:
        out = np.zeros(max(int(size), floor), dtype=np.uint8)
    room = out.numel() if device else out.size
    return out, (out.data_ptr() if device else out.ctypes.data), room if out_cap is None else min(int(out_cap), room)


def _host_bytes(x):
    """The bytes of a (small) piece of the input, wherever it is."""
    return (x.cpu().numpy() if _is_torch(x) else x).tobytes()


def _no_bytes(data):
    """An empty buffer of data's kind."""
    return data[:0] if _is_torch(data) else np.zeros(0, dtype=np.uint8)


def _offsets(off):
    """(the offset table as contiguous numpy uint64, the number of streams it describes)."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    return off, off.size - 1


def _slots(out_sizes, n):
    """out_off[n + 1]: the slots of out_sizes back to back."""
    out_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.asarray(out_sizes, dtype=np.uint64), out=out_off[1:])
    return out_off


def _deflate_room(in_off):
    """Room that always holds the raw streams of a batch: the sum of deflate_bound over its stream lengths."""
    lens = in_off[1:] - in_off[:-1]
    return int(sum(deflate_bound(int(l)) * int(c) for l, c in zip(*np.unique(lens, return_counts=True))))


def _stream_results(n, pad=True):
    """(out_len, status, err_off) for the library to fill.  pad: one entry even for an empty batch, so that the
    pointers are never those of empty arrays; the caller returns [:n]."""
    m = max(n, 1) if pad else n
    return np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.int32), np.full(m, -1, dtype=np.int64)


def _file_result(out, out_len, device, index, table):
    """What bgzf_write and zip_write return: the file as bytes (host) or (out, out_len) (device), then the table."""
    res = (out, out_len) if device else (bytes(out[:out_len]),)
    if index:
        res = res + (table,)
    return res if len(res) > 1 else res[0]


def _query_then_fill(call, found, result, index_cap, query, prefix, guess=None):
    """The protocol of the index calls.  call(cap, a_ptr, b_ptr) -> rc fills two uint64 tables of cap entries;
    found() is the count the last call reported, its tables have found() + 1 entries; result(rc, a, b) builds what
    the method returns.  query: the counts alone.  index_cap=None: sized by a query first -- or, with `guess`, by
    that guess, and by the count only if the guess was too small (where the discovery is the whole cost of a call).
    prefix: a broken chain still delivers the tables of the good entries in front (whenever they fit); without it
    the tables come with rc 0 only, and a query that fails is the answer."""
    if query:
        return result(call(0, None, None), None, None)
    if index_cap is not None:
        caps = [int(index_cap)]
    elif guess is not None:
        caps = [guess, None]
    else:
        rc = call(0, None, None)
        if rc != 0 and not prefix:
            return result(rc, None, None)
        caps = [None]
    for cap in caps:
        cap = found() + 1 if cap is None else cap
        a = np.zeros(max(cap, 1), dtype=np.uint64)
        b = np.zeros(max(cap, 1), dtype=np.uint64)
        rc = call(cap, a.ctypes.data, b.ctypes.data)
        k = found() + 1
        if (k <= cap) if prefix else (rc == 0):
            a, b = a[:k], b[:k]
            return result(rc, a, b) if guess is None else result(rc, a.copy(), b.copy())  # (a guess can be far too large)
    return result(rc, None, None)


def _read_into(out, data, out_cap, what, call, size):
    """The calls that deliver bytes into `out`: call(out_ptr, cap) -> the method's result.  out=None: size() ->
    (bytes needed, None) first, or (0, the result) when the query is the answer already and there is nothing to
    deliver; then room for that.  Otherwise the caller's buffer, its capacity cut to out_cap.  One call."""
    need, done = size() if out is None else (0, None)
    out, ptr, cap = _out_buf(out, data, need, out_cap, 0, what)
    return out, (call(ptr, cap) if done is None else done)


class OneSeekCalls:
    """The seek index of one long stream: the two methods FlateEngine inherits.  They stand in a class of their own so
    that their marshalling has its own recorded scenarios (tests/engine_trace_seek.py) beside the ones of the methods
    that were there before (tests/engine_trace.py)."""

    def inflate_one_seek_index(self, data, wrap="gzip", span=0):
        """The seek index of ONE long stream (flate_hip_inflate_one_seek_index) -> SeekIndex(rc, index, windows, n_units,
        n_points, out_bytes, status, err_off).  index: numpy uint64, the self-describing words the header documents;
        windows: n_points - 1 blocks of 32768 bytes, numpy for host data, a torch CUDA tensor for device data.  span: a
        point per that many bytes of output (0: 1 MiB; SEEK_SPAN_NONE: no windows, the cached discovery).  status is
        inflate_one's without the trailer; a stream that fails has no index (index and windows are None).  Sized by
        a guess and one retry, not by a query first: the discovery is most of the cost.  Other failures raise
        FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        iw, wb, nu, npts = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        ob, nc, st, eo = C.c_uint64(0), C.c_uint32(0), C.c_int32(0), C.c_int64(-1)
        # a unit per 256 bytes of input is more than zlib writes; the windows of a stream that inflates fourfold
        words = 16 + 2 * (n // 256 + 64) + 64
        # (and never more points than units)
        room = 0 if span == SEEK_SPAN_NONE else min(4 * n // (span or SEEK_SPAN_DEFAULT) + 4, n // 256 + 64) * 32768
        for _ in range(2):
            index = np.zeros(words, dtype=np.uint64)
            windows, w_ptr, _ = _out_buf(None, data, room, None, 0, "inflate_one_seek_index", floor=1)
            rc = self._tolerate(self._L.flate_hip_inflate_one_seek_index(
                self._ctx, in_ptr, n, WRAPS[wrap], span, index.ctypes.data, words, C.byref(iw), w_ptr, room,
                C.byref(wb), C.byref(nu), C.byref(npts), C.byref(ob), C.byref(nc), C.byref(st), C.byref(eo),
                self._flags(False, False, device)), *PER_CHAIN)
            if rc != E_OUT_TOO_SMALL:
                break
            words, room = int(iw.value), int(wb.value)
        ok = rc == 0
        return SeekIndex(rc, index[:int(iw.value)].copy() if ok else None, windows[:int(wb.value)] if ok else None,
                         int(nu.value), int(npts.value), int(ob.value), int(st.value), int(eo.value))

    def inflate_one_ranges(self, data, seek_index, begin, end, out=None, out_cap=None, wrap="gzip"):
        """Random access into ONE long stream through its seek index (flate_hip_inflate_one_ranges): the bytes of the
        ranges [begin[r], end[r]) of what the stream inflates to, back to back in out; only the units from the seek
        point in front of a range up to its end are decoded.  seek_index: what inflate_one_seek_index returned (its
        windows on the side of data), or an (index, windows) pair.  Returns (out, OneRanges(rc, out_off, range_status,
        n_decoded, bad_unit)): range r is out[out_off[r]:out_off[r + 1]].  rc 0; -4 with every range_status -4: not
        the stream the index was built from; -2 with out_off[-1] > capacity: out too small, nothing decoded; else the
        first decoded unit the index does not fit, in bad_unit.  out=None: sized by the size query first.  An index
        that is refused, begin[r] > end[r] and other refusals raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        index, windows = (seek_index.index, seek_index.windows) if isinstance(seek_index, SeekIndex) else seek_index
        index = np.ascontiguousarray(index, dtype=np.uint64)
        if windows is None or (windows.numel() if _is_torch(windows) else windows.size) == 0:
            w_ptr, wb = None, 0
        else:
            windows, w_ptr, wb, w_dev = _in_buf(windows)
            if w_dev != device:
                raise FlateError(E_INVALID, "inflate_one_ranges: the windows must be on the side of the data")
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        end = np.ascontiguousarray(end, dtype=np.uint64)
        if begin.ndim != 1 or begin.shape != end.shape:
            raise FlateError(E_INVALID, "inflate_one_ranges: begin and end must be one-dimensional and of one length")
        nr = begin.size
        out_off = np.zeros(nr + 1, dtype=np.uint64)
        status = np.zeros(max(nr, 1), dtype=np.int32)
        nd, bad = C.c_uint32(0), C.c_uint32(0)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_inflate_one_ranges(
                self._ctx, in_ptr, n, WRAPS[wrap], index.ctypes.data, index.size, w_ptr, wb, begin.ctypes.data,
                end.ctypes.data, nr, out_ptr, cap, out_off.ctypes.data, status.ctypes.data, C.byref(nd), C.byref(bad),
                self._flags(False, False, device)), *PER_CHAIN)
            return OneRanges(rc, out_off, status[:nr], int(nd.value), int(bad.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (int(out_off[nr]), None) if q.rc == E_OUT_TOO_SMALL else (0, q)

        return _read_into(out, data, out_cap, "inflate_one_ranges", call, size)


class SeekPackCalls:
    """The packed windows of the seek index of one long stream: the three methods FlateEngine inherits.  They stand in a
    class of their own so that their marshalling has its own recorded scenarios (tests/engine_trace_seek_pack.py)."""

    def seek_windows_pack(self, seek_index, data=None, sparse=True, wrap="gzip", out=None, out_cap=None):
        """The windows of a seek index, packed (flate_hip_seek_windows_pack) -> SeekPack(rc, pack_index, packed,
        packed_bytes, kept_bytes).  Every block becomes one raw DEFLATE stream, a block of zeros no bytes at all; with
        sparse the bytes that its segment never reads become zero first, for which the stream `data` is walked (without
        sparse data may be None: only its length, taken from the index, is told).  seek_index: what
        inflate_one_seek_index returned, or an (index, windows) pair; packed lies on the side of the windows.  rc 0; -4:
        data is not the stream the index was built from; -2 with packed_bytes the bytes needed: out too small, nothing
        usable written.  out=None: room for the bound.  Refusals raise FlateError."""
        index, windows = (seek_index.index, seek_index.windows) if isinstance(seek_index, SeekIndex) else seek_index
        index = np.ascontiguousarray(index, dtype=np.uint64)
        mode = SEEK_PACK_COMPRESS | (SEEK_PACK_SPARSE if sparse else 0)
        n_blocks = max(int(index[9]) - 1, 0) if index.size >= 16 else 0
        if windows is None or (windows.numel() if _is_torch(windows) else windows.size) == 0:
            windows, w_ptr, wb, device = np.zeros(0, dtype=np.uint8), None, 0, data is not None and _is_torch(data)
        else:
            windows, w_ptr, wb, device = _in_buf(windows)
        if data is None:
            in_ptr, n = None, int(index[3]) if index.size >= 16 else 0
        else:
            data, in_ptr, n, d_dev = _in_buf(data, accept_bytes=True, null_if_empty=True)
            if d_dev != device and wb:
                raise FlateError(E_INVALID, "seek_windows_pack: the windows must be on the side of the data")
        side = windows if wb or data is None else data
        words = 17 + n_blocks
        pack_index = np.zeros(words, dtype=np.uint64)
        bound = int(self._L.flate_hip_seek_windows_pack_bound(n_blocks))
        out, out_ptr, cap = _out_buf(out, side, bound, out_cap, 0, "seek_windows_pack")
        pw, pb, kb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self._tolerate(self._L.flate_hip_seek_windows_pack(
            self._ctx, in_ptr, n, WRAPS[wrap], index.ctypes.data, index.size, w_ptr, wb, mode, pack_index.ctypes.data,
            words, C.byref(pw), out_ptr, cap, C.byref(pb), C.byref(kb), self._flags(False, False, device)),
            E_OUT_TOO_SMALL, E_CORRUPT)
        ok = rc == 0
        return SeekPack(rc, pack_index if ok else None, out[:int(pb.value)] if ok else None, int(pb.value), int(kb.value))

    def seek_windows_unpack(self, pack, out=None, out_cap=None):
        """All blocks of packed windows in the raw layout (flate_hip_seek_windows_unpack) -> (windows,
        SeekUnpack(rc, windows_bytes, bad_block)): the sparsified windows, or the original ones of a pack without
        sparse -- what the unchanged inflate_one_ranges takes.  pack: what seek_windows_pack returned, or a
        (pack_index, packed) pair.  rc 0; -4 with bad_block the first block that does not inflate to 32768 bytes; -2:
        out too small.  Refusals raise FlateError."""
        pack_index, packed = (pack.pack_index, pack.packed) if isinstance(pack, SeekPack) else pack
        pack_index = np.ascontiguousarray(pack_index, dtype=np.uint64)
        packed, p_ptr, pb, device = _in_buf(packed, null_if_empty=True)
        need = (int(pack_index[3]) if pack_index.size >= 17 else 0) * 32768
        out, out_ptr, cap = _out_buf(out, packed, need, out_cap, 0, "seek_windows_unpack", floor=1)
        wb, bad = C.c_uint64(0), C.c_uint32(0)
        rc = self._tolerate(self._L.flate_hip_seek_windows_unpack(
            self._ctx, pack_index.ctypes.data, pack_index.size, p_ptr, pb, out_ptr, cap, C.byref(wb), C.byref(bad),
            self._flags(False, False, device)), E_OUT_TOO_SMALL, E_CORRUPT)
        return out[:int(wb.value)] if rc == 0 else out, SeekUnpack(rc, int(wb.value), int(bad.value))

    def inflate_one_ranges_packed(self, data, index, pack, begin, end, out=None, out_cap=None, wrap="gzip"):
        """inflate_one_ranges through PACKED windows (flate_hip_inflate_one_ranges_packed): only the blocks of the
        selected points are inflated, into scratch that grows with the selection.  index: the seek index's words (or a
        SeekIndex); pack: what seek_windows_pack returned, or a (pack_index, packed) pair, packed on the side of data.
        Returns (out, OneRanges) as inflate_one_ranges does; a block that does not inflate makes its point's unit the
        bad unit with status -4."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        index = np.ascontiguousarray(index.index if isinstance(index, SeekIndex) else index, dtype=np.uint64)
        pack_index, packed = (pack.pack_index, pack.packed) if isinstance(pack, SeekPack) else pack
        pack_index = np.ascontiguousarray(pack_index, dtype=np.uint64)
        if packed is None or (packed.numel() if _is_torch(packed) else packed.size) == 0:
            p_ptr, pb = None, 0
        else:
            packed, p_ptr, pb, p_dev = _in_buf(packed)
            if p_dev != device:
                raise FlateError(E_INVALID, "inflate_one_ranges_packed: the packed windows must be on the side of the data")
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        end = np.ascontiguousarray(end, dtype=np.uint64)
        if begin.ndim != 1 or begin.shape != end.shape:
            raise FlateError(E_INVALID, "inflate_one_ranges_packed: begin and end must be one-dimensional and of one length")
        nr = begin.size
        out_off = np.zeros(nr + 1, dtype=np.uint64)
        status = np.zeros(max(nr, 1), dtype=np.int32)
        nd, bad = C.c_uint32(0), C.c_uint32(0)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_inflate_one_ranges_packed(
                self._ctx, in_ptr, n, WRAPS[wrap], index.ctypes.data, index.size, pack_index.ctypes.data, pack_index.size,
                p_ptr, pb, begin.ctypes.data, end.ctypes.data, nr, out_ptr, cap, out_off.ctypes.data, status.ctypes.data,
                C.byref(nd), C.byref(bad), self._flags(False, False, device)), *PER_CHAIN)
            return OneRanges(rc, out_off, status[:nr], int(nd.value), int(bad.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (int(out_off[nr]), None) if q.rc == E_OUT_TOO_SMALL else (0, q)

        return _read_into(out, data, out_cap, "inflate_one_ranges_packed", call, size)


class GzFileCalls:
    """A gzip file of any members, long ones included: the two methods FlateEngine inherits.  They stand in a class of
    their own so that their marshalling has its own recorded scenarios (tests/engine_trace_gzfile.py) beside the ones
    of the methods that were there before."""

    def gzfile_index(self, data, index_cap=None, member_cap=None, query=False):
        """Where the units and the members of a gzip file start (one member or many, long or short) and where their
        output goes, found on the GPU from the file's bits (flate_hip_gzfile_index) -> GzFileIndex(rc, n_units,
        n_members, out_bytes, n_candidates, status, bad_member, err_off, stream_err_off, unit_bit, out_off, member_off,
        member_unit).  unit_bit (numpy uint64[n_units + 1], bits counted from the FILE's first byte) and out_off as
        inflate_one_index has them, per member; member_off (file offsets, the last entry len(data)) and member_unit
        (every member's first unit, the last entry n_units).  status 0, or the walk's: -4, -7 or -6 in member
        bad_member, which starts at err_off (or where no member can start), at stream_err_off of its raw stream; the
        arrays then hold the good prefix.  query=True: only the counts (the arrays are None).  index_cap / member_cap:
        the arrays' sizes (default: a unit per 256 bytes and a member per 4096 bytes of input, and a second call only
        if the file has more; given and too small: rc -2, that pair None).  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        nu, nm, ob, nc = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        st, bad, eo, seo = C.c_int32(0), C.c_uint32(0), C.c_int64(-1), C.c_int64(-1)

        def call(ucap, ub, oo, mcap, mo, mu):
            return self._tolerate(self._L.flate_hip_gzfile_index(
                self._ctx, in_ptr, n, ucap, ub, oo, mcap, mo, mu, C.byref(nu), C.byref(nm), C.byref(ob), C.byref(nc),
                C.byref(st), C.byref(bad), C.byref(eo), C.byref(seo), self._flags(False, False, device)), *PER_CHAIN)

        def result(rc, ub=None, oo=None, mo=None, mu=None):
            return GzFileIndex(rc, int(nu.value), int(nm.value), int(ob.value), int(nc.value), int(st.value),
                               int(bad.value), int(eo.value), int(seo.value), ub, oo, mo, mu)

        if query:
            return result(call(0, None, None, 0, None, None))
        # no query first: the discovery is the whole cost of the call
        ucap = n // 256 + 64 if index_cap is None else int(index_cap)
        mcap = n // 4096 + 64 if member_cap is None else int(member_cap)
        for _ in range(2):
            t = [np.zeros(max(c, 1), dtype=np.uint64) for c in (ucap, ucap, mcap, mcap)]
            rc = call(ucap, t[0].ctypes.data, t[1].ctypes.data, mcap, t[2].ctypes.data, t[3].ctypes.data)
            ku, km = int(nu.value) + 1, int(nm.value) + 1
            short_u, short_m = ku > ucap and index_cap is None, km > mcap and member_cap is None
            if not (short_u or short_m):
                break
            ucap, mcap = (ku if short_u else ucap), (km if short_m else mcap)
        u_ok, m_ok = ku <= ucap, km <= mcap
        return result(rc, t[0][:ku].copy() if u_ok else None, t[1][:ku].copy() if u_ok else None,
                      t[2][:km].copy() if m_ok else None, t[3][:km].copy() if m_ok else None)

    def gzfile_read(self, data, out=None, out_cap=None):
        """A gzip file of any members back into its bytes by one call, what zcat gives (flate_hip_gzfile_read): every
        member cut into units that are decoded in parallel, every member's CRC-32 and ISIZE checked on the GPU.  For
        files of many small members gzip_read is faster -- or set_option("gzfile_serial_max", 1 << 20), which decodes
        short members whole here (gzfile_last_route); for exactly one member inflate_one is the same work.  Returns
        (out, GzFileRead(rc, out_len, n_members, n_units, n_candidates, status, bad_member, err_off, stream_err_off));
        the bytes are out[:out_len] (numpy for host data, a torch CUDA tensor for device data).  status 0; a chain
        that breaks: gzfile_index's words, the good members in front and the failing member's bytes in front of its
        failure delivered; a wrong trailer: -4 with bad_member, err_off its file offset and stream_err_off its length,
        everything delivered.  rc -2 with out_len > capacity: out too small, nothing decoded.  out=None: sized by the
        size query first.  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        ol, nm, nu, nc = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        st, bad, eo, seo = C.c_int32(0), C.c_uint32(0), C.c_int64(-1), C.c_int64(-1)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_gzfile_read(
                self._ctx, in_ptr, n, out_ptr, cap, C.byref(ol), C.byref(nm), C.byref(nu), C.byref(nc), C.byref(st),
                C.byref(bad), C.byref(eo), C.byref(seo), self._flags(False, False, device)), *PER_CHAIN)
            return GzFileRead(rc, int(ol.value), int(nm.value), int(nu.value), int(nc.value), int(st.value),
                              int(bad.value), int(eo.value), int(seo.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (q.out_len, None) if q.rc == E_OUT_TOO_SMALL else (0, q)

        return _read_into(out, data, out_cap, "gzfile_read", call, size)


class GzFileSerialCalls:
    """gzfile_index / gzfile_read with the option "gzfile_serial_max": the method FlateEngine inherits.  It stands in a
    class of its own so that its marshalling has its own recorded scenarios (tests/engine_trace_gzfile_serial.py) beside
    the ones of the methods that were there before."""

    def gzfile_last_route(self):
        """What the last gzfile_index or gzfile_read on this engine did with the option "gzfile_serial_max"
        (flate_hip_gzfile_last_route): (serial_members, unit_members, find_from) -- the discovery's good members that
        were taken WHOLE (one unit each, decoded by the batch decoders), its other good members (cut into units), and
        the file offset the bit-offset search started at: len(data) = no search ran; 0 with the option at 0.  Bytes and
        verdicts are identical by design, so this is how to see which path ran."""
        sm, um, ff = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self._L.flate_hip_gzfile_last_route(self._ctx, C.byref(sm), C.byref(um), C.byref(ff)))
        return int(sm.value), int(um.value), int(ff.value)


class GzFileSeekCalls:
    """The seek index of a gzip file of any members: the two methods FlateEngine inherits.  They stand in a class of
    their own so that their marshalling has its own recorded scenarios (tests/engine_trace_gzfile_seek.py) beside the
    ones of the methods that were there before."""

    def gzfile_seek_index(self, data, span=0):
        """The seek index of a gzip file of ANY members (flate_hip_gzfile_seek_index) -> GzFileSeekIndex(rc, index,
        windows, n_units, n_members, n_points, out_bytes, n_candidates, status, bad_member, err_off, stream_err_off).
        index: numpy uint64, the self-describing words the header documents; windows: n_points - n_members blocks of
        32768 bytes (a point that starts a member has none), numpy for host data, a torch CUDA tensor for device data.
        span: a point per that many bytes of output besides every member start (0: 1 MiB; SEEK_SPAN_NONE: the member
        starts alone, no windows).  status and the three words behind it are gzfile_index's, trailers are not judged; a
        file that fails has no index (index and windows are None).  Sized by a guess and one retry, not by a query
        first: the discovery is most of the cost.  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        iw, wb, nu, nm, npts = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        ob, nc, st = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
        bad, eo, seo = C.c_uint32(0), C.c_int64(-1), C.c_int64(-1)
        # a unit per 256 bytes and a member per 4096 bytes of input; the windows of a file that inflates fourfold
        words = 16 + 2 * (n // 256 + 64) + 2 * (n // 4096 + 64) + 64
        room = 0 if span == SEEK_SPAN_NONE else min(4 * n // (span or SEEK_SPAN_DEFAULT) + 4, n // 256 + 64) * 32768
        for _ in range(2):
            index = np.zeros(words, dtype=np.uint64)
            windows, w_ptr, _ = _out_buf(None, data, room, None, 0, "gzfile_seek_index", floor=1)
            rc = self._tolerate(self._L.flate_hip_gzfile_seek_index(
                self._ctx, in_ptr, n, span, index.ctypes.data, words, C.byref(iw), w_ptr, room, C.byref(wb),
                C.byref(nu), C.byref(nm), C.byref(npts), C.byref(ob), C.byref(nc), C.byref(st), C.byref(bad),
                C.byref(eo), C.byref(seo), self._flags(False, False, device)), *PER_CHAIN)
            if rc != E_OUT_TOO_SMALL:
                break
            words, room = int(iw.value), int(wb.value)
        ok = rc == 0
        return GzFileSeekIndex(rc, index[:int(iw.value)].copy() if ok else None,
                               windows[:int(wb.value)] if ok else None, int(nu.value), int(nm.value), int(npts.value),
                               int(ob.value), int(nc.value), int(st.value), int(bad.value), int(eo.value),
                               int(seo.value))

    def gzfile_ranges(self, data, seek_index, begin, end, out=None, out_cap=None):
        """Random access into a gzip file of any members through its seek index (flate_hip_gzfile_ranges): the bytes of
        the ranges [begin[r], end[r]) of what zcat gives, back to back in out; a range may cross members; only the
        units from the seek point in front of a range up to its end are decoded.  seek_index: what gzfile_seek_index
        returned (its windows on the side of data), or an (index, windows) pair.  Returns (out, OneRanges(rc, out_off,
        range_status, n_decoded, bad_unit)): range r is out[out_off[r]:out_off[r + 1]].  rc 0; -4 with every
        range_status -4: some member's header is not where the index has it; -2 with out_off[-1] > capacity: out too
        small, nothing decoded; else the first decoded unit the index does not fit, in bad_unit.  out=None: sized by
        the size query first.  An index that is refused, begin[r] > end[r] and other refusals raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        index, windows = (seek_index.index, seek_index.windows) if isinstance(seek_index, GzFileSeekIndex) else seek_index
        index = np.ascontiguousarray(index, dtype=np.uint64)
        if windows is None or (windows.numel() if _is_torch(windows) else windows.size) == 0:
            w_ptr, wb = None, 0
        else:
            windows, w_ptr, wb, w_dev = _in_buf(windows)
            if w_dev != device:
                raise FlateError(E_INVALID, "gzfile_ranges: the windows must be on the side of the data")
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        end = np.ascontiguousarray(end, dtype=np.uint64)
        if begin.ndim != 1 or begin.shape != end.shape:
            raise FlateError(E_INVALID, "gzfile_ranges: begin and end must be one-dimensional and of one length")
        nr = begin.size
        out_off = np.zeros(nr + 1, dtype=np.uint64)
        status = np.zeros(max(nr, 1), dtype=np.int32)
        nd, bad = C.c_uint32(0), C.c_uint32(0)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_gzfile_ranges(
                self._ctx, in_ptr, n, index.ctypes.data, index.size, w_ptr, wb, begin.ctypes.data, end.ctypes.data, nr,
                out_ptr, cap, out_off.ctypes.data, status.ctypes.data, C.byref(nd), C.byref(bad),
                self._flags(False, False, device)), *PER_CHAIN)
            return OneRanges(rc, out_off, status[:nr], int(nd.value), int(bad.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (int(out_off[nr]), None) if q.rc == E_OUT_TOO_SMALL else (0, q)

        return _read_into(out, data, out_cap, "gzfile_ranges", call, size)


class ZipUnitsCalls:
    """ZIP reads with the option "zip_unit_min": the method FlateEngine inherits.  It stands in a class of its own so
    that its marshalling has its own recorded scenarios (tests/engine_trace_zip_units.py) beside the ones of the methods
    that were there before."""

    def zip_last_route(self):
        """What the last zip_read on this engine did with the option "zip_unit_min" (flate_hip_zip_last_route):
        (unit_entries, fallback_entries, n_units, n_candidates) -- the selection slots served by units, the slots that
        qualified by size but went to the batch decoders, the units on the path, FIND's candidates.  All zero with the
        option at 0: results are identical by design, so this is how to see which path ran."""
        w = [C.c_uint32(0) for _ in range(4)]
        self._check(self._L.flate_hip_zip_last_route(self._ctx, *[C.byref(x) for x in w]))
        return tuple(int(x.value) for x in w)


class GroupedCalls:
    """Grouped splice: the method FlateEngine inherits.  It stands in a class of its own so that its marshalling has its
    own recorded scenarios (tests/engine_trace_grouped.py) beside the ones of the methods that were there before."""

    def deflate_grouped_framed(self, data, in_off, group_off, wrap, compat_go=False, out=None, out_cap=None, index=False):
        """Several spliced members in one call (flate_hip_deflate_fast_grouped_framed): the pieces
        data[in_off[i]:in_off[i+1]] are compressed on their own, in parallel; group g = the pieces
        group_off[g] .. group_off[g+1] - 1 becomes ONE zlib stream, gzip member or ("raw") bare DEFLATE stream, what
        deflate_spliced_framed writes for those pieces, and the members lie back to back.  group_off starts at 0, ends
        at the number of pieces and is strictly increasing (an empty member is one piece of zero bytes).
        data: numpy uint8 (host; returns (exactly the members' bytes, out_off[n_groups+1])) or a torch uint8 CUDA tensor
        (returns (out tensor, out_off as numpy)).  index=True adds bit_off, numpy uint64[n_pieces + n_groups]: group g's
        index is bit_off[group_off[g] + g : group_off[g+1] + g + 1], counted from the first byte of the member's raw
        stream -- inflate_spliced_framed takes a member and this slice as they are."""
        in_off, n = _offsets(in_off)
        group_off = np.ascontiguousarray(group_off, dtype=np.uint32)
        n_groups = group_off.size - 1
        w = _wrap_code(wrap)
        data, in_ptr, _, device = _in_buf(data)
        if out_cap is None and out is None:
            out_cap = _deflate_room(in_off) + 16 + max(n_groups, 0) * (5 + frame_overhead(wrap))
        out, out_ptr, cap = _out_buf(out, data, out_cap, out_cap, 0, "deflate_grouped_framed")
        out_off = np.zeros(max(n_groups, 0) + 1, dtype=np.uint64)
        bit_off = np.zeros(max(n + n_groups, 1), dtype=np.uint64)
        self._check(self._L.flate_hip_deflate_fast_grouped_framed(
            self._ctx, in_ptr, in_off.ctypes.data, n, group_off.ctypes.data, max(n_groups, 0), w, out_ptr, cap,
            out_off.ctypes.data, bit_off.ctypes.data if index else None, self._flags(compat_go, False, device)))
        res = (out if device else out[:int(out_off[-1])]), out_off
        return res + (bit_off[:n + n_groups],) if index else res

    def zip_write_last_route(self):
        """What the last zip_write on this engine did with the option "zip_piece_bytes"
        (flate_hip_zip_write_last_route): (long_entries, n_pieces) -- the entries written from more than one piece and
        the pieces of the whole call.  (0, 0) on the unchanged route: the option at 0, or no entry longer than it."""
        w = [C.c_uint32(0) for _ in range(2)]
        self._check(self._L.flate_hip_zip_write_last_route(self._ctx, *[C.byref(x) for x in w]))
        return tuple(int(x.value) for x in w)


class OnePartsCalls:
    """One long stream read in parts: the method FlateEngine inherits.  It stands in a class of its own so that its
    marshalling has its own recorded scenarios (tests/engine_trace_one_parts.py) beside the ones of the methods that
    were there before (tests/engine_trace.py)."""

    def open_one_reader(self, wrap="gzip", device=False):
        """ONE long stream ("raw", "zlib" or "gzip") read in parts through bounded buffers at inflate_one's speed
        (flate_hip_one_reader_*): see OneReader.  device: every part and every output is a torch CUDA tensor."""
        return OneReader(self, wrap, device)


class GzFilePartsCalls:
    """A gzip file of any members read in parts: the method FlateEngine inherits.  It stands in a class of its own so
    that its marshalling has its own recorded scenarios (tests/engine_trace_gzfile_parts.py) beside the ones of the
    methods that were there before (tests/engine_trace.py)."""

    def open_gzfile_reader(self, device=False, serial_max=0):
        """A gzip FILE of any members read in parts through bounded buffers at gzfile_read's speed
        (flate_hip_gzfile_reader_*): see GzFileReader.  device: every part and every output is a torch CUDA tensor.
        serial_max: GzFileReader.set_serial_max on the fresh handle (0, the default: no call is made)."""
        r = GzFileReader(self, device)
        if serial_max:
            try:
                r.set_serial_max(serial_max)
            except Exception:
                r.close()
                raise
        return r


class OneWriterCalls:
    """One long stream written in parts: the method FlateEngine inherits.  It stands in a class of its own so that its
    marshalling has its own recorded scenarios (tests/engine_trace_one_writer.py) beside the ones of the methods that
    were there before (tests/engine_trace.py)."""

    def open_one_writer(self, wrap="gzip", piece_bytes=0, device=False, compat_go=False):
        """ONE long stream ("raw", "zlib" or "gzip") written in parts through bounded buffers at deflate_spliced_framed's
        speed (flate_hip_one_writer_*): see OneWriter.  piece_bytes: the bytes of a piece (0: 65535).  device: every
        part and every output is a torch CUDA tensor."""
        return OneWriter(self, wrap, piece_bytes, device, compat_go)


class BgzfPartsCalls:
    """A BGZF file read and written in parts: the methods FlateEngine inherits.  They stand in a class of their own so
    that their marshalling has its own recorded scenarios (tests/engine_trace_bgzf_parts.py) beside the ones of the
    methods that were there before (tests/engine_trace.py)."""

    def open_bgzf_reader(self, device=False):
        """A BGZF file read in parts through bounded buffers at bgzf_read's speed (flate_hip_bgzf_reader_*): see
        BgzfReader.  device: every part and every output is a torch CUDA tensor."""
        return BgzfReader(self, device)

    def open_bgzf_writer(self, block_bytes=0, device=False, compat_go=False):
        """A BGZF file written in parts through bounded buffers at bgzf_write's speed (flate_hip_bgzf_writer_*): see
        BgzfWriter.  block_bytes: as bgzf_write's (0: 65280).  device: every part and every output is a torch CUDA
        tensor."""
        return BgzfWriter(self, block_bytes, device, compat_go)


class FlateEngine(OneSeekCalls, SeekPackCalls, GzFileCalls, GzFileSerialCalls, GzFileSeekCalls, ZipUnitsCalls, GroupedCalls, OnePartsCalls,
                  OneWriterCalls, GzFilePartsCalls, BgzfPartsCalls):
    """One engine = one flate_hip_ctx = one GPU + one HIP stream."""

    def __init__(self, device=0):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._L.flate_hip_init(int(device), C.byref(self._ctx))
        if rc != 0:
            raise FlateError(rc, self._L.flate_hip_strerror(rc).decode())
        self.device = int(device)

    def close(self):
        if self._ctx:
            self._L.flate_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self._L.flate_hip_strerror(rc).decode()
            extra = self._L.flate_hip_last_hip_error(self._ctx).decode()
            raise FlateError(rc, msg + (" [" + extra + "]" if extra else ""))

    def _tolerate(self, rc, *allowed):
        """rc, if it is 0 or one of the statuses this call hands back to its caller; anything else raises."""
        if rc not in allowed:
            self._check(rc)
        return rc

    def use_stream(self, hip_stream_ptr):
        """Launch on the given hipStream_t (int address), e.g. torch.cuda.current_stream().cuda_stream."""
        self._check(self._L.flate_hip_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or None)))

    def host_register(self, arr):
        """Page-lock a host buffer the caller keeps across calls (flate_hip_host_register): the copies of
        the host-pointer calls then run at the link's rate.  Returns a context manager that
        unregisters on exit (or call .close())."""
        a = np.ascontiguousarray(arr)
        assert a is arr or np.shares_memory(a, arr), "host_register needs a contiguous array"
        self._check(self._L.flate_hip_host_register(self._ctx, a.ctypes.data, a.nbytes))
        eng = self

        class _Reg:
            def __init__(self):
                self.ptr = a.ctypes.data

            def close(self):
                if self.ptr:
                    eng._check(eng._L.flate_hip_host_unregister(eng._ctx, self.ptr))
                    self.ptr = None

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                self.close()

        return _Reg()

    def set_option(self, name, value):
        """Launch-geometry knobs (guest_blocks, resident_blocks, guest_min_streams)."""
        self._check(self._L.flate_hip_set_option(self._ctx, name.encode(), int(value)))

    def set_profiling(self, on=True):
        self._check(self._L.flate_hip_set_profiling(self._ctx, 1 if on else 0))

    def last_resident_share(self):
        """(streams the LDS-table blocks took, streams queued) of the last persistent match-finder launch."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.flate_hip_last_resident_share(self._ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_timing(self):
        ms = (C.c_float * len(STAGES))()
        self._check(self._L.flate_hip_last_timing(self._ctx, ms, len(STAGES)))
        return {STAGES[i]: float(ms[i]) for i in range(len(STAGES))}

    @staticmethod
    def _flags(compat_go, lz_serial, device):
        return (COMPAT_GO if compat_go else 0) | (LZ_SERIAL if lz_serial else 0) | \
               (DEVICE_PTRS if device else 0)

    def deflate_batch(self, data, in_off, out=None, out_cap=None, compat_go=False, lz_serial=False,
                      zdicts=None, dict_of=None):
        """Compress independent streams: stream i = data[in_off[i]:in_off[i+1]] with fresh-Writer
        semantics.  data: numpy uint8 array (host) or torch uint8 CUDA tensor (device).
        zdicts: preset dictionaries as HISTORY (flate_hip_deflate_fast_batch_dict) -- one bytes-like object or a
        list of them; dict_of[i] = the dictionary of stream i or NO_DICT (None: every stream uses the first), the
        argument shapes of inflate_batch.  Such a stream can only be read with the same dictionary
        (inflate_batch(..., zdicts=), zlib.decompressobj(-15, zdict=)); compat_go=True is the mode in which
        matches extend into the dictionary; payloads under 128 bytes get nothing from it (include/flate_hip.h).
        Returns (out, out_off): out has the same kind as data, out_off is numpy uint64[n+1]."""
        in_off, n = _offsets(in_off)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        data, in_ptr, _, device = _in_buf(data)
        if out_cap is None and out is None:
            out_cap = _deflate_room(in_off)
        out, out_ptr, cap = _out_buf(out, data, out_cap, None, 1, "deflate_batch")
        flags = self._flags(compat_go, lz_serial, device)
        if zdicts is None:
            rc = self._L.flate_hip_deflate_fast_batch(self._ctx, in_ptr, in_off.ctypes.data, n, out_ptr,
                                                      cap, out_off.ctypes.data, flags)
        else:
            dk = _DictArgs(zdicts, dict_of, n, device)
            rc = self._L.flate_hip_deflate_fast_batch_dict(self._ctx, in_ptr, in_off.ctypes.data, n, dk.ptr,
                                                           dk.off_ptr, dk.n_dicts, dk.of_ptr, out_ptr, cap,
                                                           out_off.ctypes.data, flags)
        self._check(rc)
        return out, out_off

    def checksum_batch(self, data, in_off, kind="adler32"):
        """Adler-32 (RFC 1950) or CRC-32 (RFC 1952) of every stream data[in_off[i]:in_off[i+1]] -> numpy uint32[n]
        (flate_hip_checksum_batch; numpy data = host pointers, torch CUDA tensor = device pointers)."""
        in_off, n = _offsets(in_off)
        sums = np.zeros(max(n, 1), dtype=np.uint32)
        data, ptr, nbytes, device = _in_buf(data, lax=True)
        if not device and not nbytes:
            ptr = None  # (only here, and only for host data, does a batch call say NULL for no bytes)
        self._check(self._L.flate_hip_checksum_batch(self._ctx, ptr, in_off.ctypes.data, n, CHECKSUMS[kind],
                                                     sums.ctypes.data, self._flags(False, False, device)))
        return sums[:n]

    def deflate_batch_framed(self, data, in_off, wrap, compat_go=False, zdicts=None, dict_of=None, out=None,
                             out_cap=None):
        """The streams of a batch as zlib (RFC 1950) or gzip (RFC 1952) members: the raw DEFLATE streams of
        deflate_batch between the container's header and its trailer -- Adler-32, or CRC-32 and the length --
        written in place on the GPU by one call (flate_hip_deflate_fast_batch_framed; wrap "raw" is deflate_batch).
        data: numpy uint8 (host; returns (exactly the members' bytes, off[n+1])) or a torch uint8 CUDA tensor (data
        and result stay on the device; returns (out tensor, off[n+1] as numpy), the members in out[:off[-1]]).
        zdicts / dict_of (zlib only; as in deflate_batch): a member written with a dictionary carries FDICT and
        the dictionary's Adler-32 as DICTID (RFC 1950 2.2), so that inflate_batch_framed(..., zdicts=) and
        zlib.decompressobj(zdict=) find it; the trailer stays the payload's checksum.  (gzip has no preset
        dictionaries: ValueError.)"""
        in_off, n = _offsets(in_off)
        w = _wrap_code(wrap)
        if zdicts is not None and w == WRAP_GZIP:
            raise ValueError("preset dictionaries exist in the zlib container only")
        data, in_ptr, _, device = _in_buf(data)
        if out_cap is None and out is None:
            out_cap = _deflate_room(in_off) + n * frame_overhead(wrap, zdicts is not None)
        out, out_ptr, cap = _out_buf(out, data, out_cap, out_cap, 0, "deflate_batch_framed")
        out_off = np.zeros(n + 1, dtype=np.uint64)
        dk = _DictArgs(zdicts, dict_of, n, device)
        self._check(self._L.flate_hip_deflate_fast_batch_framed(
            self._ctx, in_ptr, in_off.ctypes.data, n, w, dk.ptr, dk.off_ptr, dk.n_dicts, dk.of_ptr, out_ptr, cap,
            out_off.ctypes.data, self._flags(compat_go, False, device)))
        return (out if device else out[:int(out_off[-1])]), out_off

    def deflate_spliced_framed(self, data, in_off, wrap, compat_go=False, out=None, out_cap=None, index=False):
        """The whole batch as ONE zlib stream or ONE gzip member: the spliced DEFLATE stream of deflate_spliced
        (every input stream compressed on its own, in parallel, joined at bit granularity) between the
        container's header and the checksum of ALL the input -- what `gzip -d` / zlib.decompress turn back
        into the concatenated input; one call, framed on the GPU (flate_hip_deflate_fast_spliced_framed).
        Host data: returns bytes.  A torch CUDA tensor, or index=True: returns (out, out_len, bit_off[n+1]) as
        deflate_spliced does, bit_off counted from the raw stream's first byte (out[2:] zlib, out[10:] gzip)."""
        in_off, n = _offsets(in_off)
        w = _wrap_code(wrap)
        data, in_ptr, _, device = _in_buf(data)
        if out_cap is None and out is None:
            out_cap = _deflate_room(in_off) + 16 + frame_overhead(wrap)
        out, out_ptr, cap = _out_buf(out, data, out_cap, out_cap, 0, "deflate_spliced_framed")
        bit_off = np.zeros(n + 1, dtype=np.uint64)
        out_len = C.c_uint64(0)
        self._check(self._L.flate_hip_deflate_fast_spliced_framed(
            self._ctx, in_ptr, in_off.ctypes.data, n, w, out_ptr, cap, C.byref(out_len), bit_off.ctypes.data,
            self._flags(compat_go, False, device)))
        if device or index:
            return out, int(out_len.value), bit_off
        return bytes(out[:int(out_len.value)])

    def inflate_batch_framed(self, data, in_off, wrap, out_sizes=None, zdicts=None, out=None):
        """The reverse: zlib or gzip members -> (out, out_off, out_len, status[n]), parsed, decoded and checked against
        their trailers on the GPU by one call (flate_hip_inflate_batch_framed); status -4 (FLATE_HIP_E_CORRUPT) also
        for a bad header, a checksum or (gzip) a length that does not match, -7 for a raw stream that ends before
        its final block does.  data: numpy uint8 (host) or a torch uint8 CUDA tensor (data and result stay on the
        device).  zlib members carry no size: out_sizes (or a size-only pass of the same call) supplies it; gzip's
        ISIZE is used as the slot size.  zdicts (zlib): one preset dictionary or a list of them; a member with
        FDICT is decoded with the first one whose Adler-32 is its DICTID (RFC 1950 2.2) -- none matches, or no
        zdicts: the member is corrupt.  The details (err_off, the dictionary every member chose) are kept in
        self.last_framed_read = (err_off, dict_used)."""
        in_off, n = _offsets(in_off)
        w = _wrap_code(wrap)
        data, in_ptr, _, device = _in_buf(data)
        dk = _DictArgs(zdicts if w == WRAP_ZLIB else None, None, n, device)
        out_len, status, err_off = _stream_results(n)
        dict_used = np.full(max(n, 1), NO_DICT, dtype=np.uint32)

        def call(out_ptr, off_ptr, flags):
            self._tolerate(self._L.flate_hip_inflate_batch_framed(
                self._ctx, in_ptr, in_off.ctypes.data, n, w, dk.ptr, dk.off_ptr, dk.n_dicts, out_ptr, off_ptr,
                out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, dict_used.ctypes.data,
                flags | self._flags(False, False, device)), *PER_STREAM)

        if out_sizes is None:
            if w == WRAP_GZIP:
                out_sizes = _gzip_isizes(data, in_off)
            else:
                call(None, None, SIZE_ONLY)
                out_sizes = out_len[:n].copy()
        out_off = _slots(out_sizes, n)
        out, out_ptr, _ = _out_buf(out, data, out_off[-1], None, int(out_off[-1]), "inflate_batch_framed")
        call(out_ptr, out_off.ctypes.data, 0)
        self.last_framed_read = (err_off[:n], dict_used[:n])
        return out, out_off, out_len[:n], status[:n]

    def bgzf_write(self, data, block_bytes=0, compat_go=False, out=None, index=False, out_cap=None):
        """data as ONE BGZF file (the blocked gzip of the SAM/BAM specification; flate_hip_bgzf_write): a member of
        its own for every block_bytes of input (0: 65280, what bgzip cuts at; at most 65535), each with its size in
        a 'BC' extra subfield, then the 28-byte EOF marker -- a .gz file that gzip -d, gzip.decompress and every
        BGZF reader turn back into data, written on the GPU by one call.  data: numpy uint8 / bytes (host; returns
        the file as bytes) or a torch uint8 CUDA tensor (data and file stay on the device; returns (out, out_len),
        the file in out[:out_len]).  index=True: member_off (numpy uint64[n_blocks + 1]) is appended to the result.
        A block that compresses to more than 65536 bytes: FlateError(E_TOO_LARGE) naming it."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        if out_cap is None and out is None:
            out_cap = bgzf_bound(n, block_bytes)
            if out_cap == 0:
                raise FlateError(E_INVALID, "bgzf_write: block_bytes must be 0 or 1 .. 65535")
        out, out_ptr, cap = _out_buf(out, data, out_cap, out_cap, 0, "bgzf_write", floor=32)
        bb = int(block_bytes) if block_bytes else BGZF_BLOCK_DEFAULT
        member_off = np.zeros((n + bb - 1) // max(bb, 1) + 1, dtype=np.uint64)
        out_len = C.c_uint64(0)
        self._check(self._L.flate_hip_bgzf_write(self._ctx, in_ptr, n, int(block_bytes), out_ptr, cap,
                                                 C.byref(out_len), member_off.ctypes.data,
                                                 self._flags(compat_go, False, device)))
        return _file_result(out, int(out_len.value), device, index, member_off)

    def bgzf_index(self, data, index_cap=None, query=False):
        """Where the members of a BGZF file start and where their output goes, found on the GPU from the file's bytes
        (flate_hip_bgzf_index) -> BgzfIndex(rc, n_members, out_bytes, eof_marker, err_off, member_off, out_off).
        rc 0: member_off / out_off (numpy uint64[n_members + 1]) are what inflate_batch_framed(..., "gzip") takes as
        in_off / the cumulative out_sizes.  rc -4 (FLATE_HIP_E_CORRUPT): no member could be read at err_off, behind
        n_members good ones.  query=True: only the counts (the arrays are None); index_cap: the arrays' size (default:
        what a query says is needed; too small: rc -2).  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        nm, ob, eof, eo = C.c_uint32(0), C.c_uint64(0), C.c_int(0), C.c_int64(-1)

        def call(cap, a, b):
            return self._tolerate(self._L.flate_hip_bgzf_index(
                self._ctx, in_ptr, n, cap, a, b, C.byref(nm), C.byref(ob), C.byref(eof), C.byref(eo),
                self._flags(False, False, device)), E_CORRUPT, E_OUT_TOO_SMALL)

        def result(rc, a, b):
            return BgzfIndex(rc, int(nm.value), int(ob.value), int(eof.value), int(eo.value), a, b)

        return _query_then_fill(call, lambda: int(nm.value), result, index_cap, query, prefix=False)

    def bgzf_read(self, data, out=None, out_cap=None):
        """A BGZF file -- bgzf_write's, bgzip's, htslib's -- back into its bytes by one call (flate_hip_bgzf_read):
        member discovery, decode and the check of every member's CRC-32 and ISIZE on the GPU, no side index.
        Returns (out, BgzfRead(rc, out_len, n_members, bad_member, err_off, eof_marker)); the bytes are out[:out_len]
        (numpy for host data, a torch CUDA tensor for device data).  rc 0; -4 with bad_member == n_members: a
        malformed chain at err_off (nothing decoded); otherwise the first failing member's status (-4 header, CRC or
        ISIZE; -7 raw stream cut short; -2 more output than ISIZE) with its index and file offset, all other members
        delivered; -2 with out_len > capacity: out too small, nothing decoded.  out=None: sized by a query of the
        index first.  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        ol, nm, bad, eo, eof = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_int64(-1), C.c_int(0)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_bgzf_read(
                self._ctx, in_ptr, n, out_ptr, cap, C.byref(ol), C.byref(nm), C.byref(bad), C.byref(eo), C.byref(eof),
                self._flags(False, False, device)), *PER_STREAM)
            return BgzfRead(rc, int(ol.value), int(nm.value), int(bad.value), int(eo.value), int(eof.value))

        return _read_into(out, data, out_cap, "bgzf_read", call,
                          lambda: (self.bgzf_index(data, query=True).out_bytes, None))

    def gzip_index(self, data, index_cap=None, query=False):
        """Where the members of a plain multi-member gzip file (cat a.gz b.gz, rotated logs, WARC records) start and
        where their output goes, found on the GPU from the file's bytes (flate_hip_gzip_index) -> GzipIndex(rc,
        n_members, out_bytes, n_candidates, err_off, member_off, out_off).  rc 0: member_off / out_off (numpy
        uint64[n_members + 1]) are what inflate_batch_framed(..., "gzip") takes as in_off / the cumulative out_sizes.
        A broken chain: rc -4 (no member can start at err_off), -7 (the stream at err_off is cut short) or -6 (the
        member at err_off has more than "gzip_member_max" bytes, or inflates to 4 GiB or more), behind n_members good
        ones, whose index the arrays still hold.  n_candidates: the offsets decoded speculatively.  query=True: only the
        counts (the arrays are None); index_cap: the arrays' size (default: what a query says is needed; too small: rc
        -2, the arrays None).  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        nm, ob, nc, eo = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_int64(-1)

        def call(cap, a, b):
            return self._tolerate(self._L.flate_hip_gzip_index(
                self._ctx, in_ptr, n, cap, a, b, C.byref(nm), C.byref(ob), C.byref(nc), C.byref(eo),
                self._flags(False, False, device)), *PER_CHAIN)

        def result(rc, a, b):
            return GzipIndex(rc, int(nm.value), int(ob.value), int(nc.value), int(eo.value), a, b)

        return _query_then_fill(call, lambda: int(nm.value), result, index_cap, query, prefix=True)

    def inflate_one_index(self, data, wrap="gzip", index_cap=None, query=False):
        """Where the units of ONE long stream ("raw", "zlib" or "gzip": what gzip, zlib or pigz write, one member, many
        blocks) start and where their output goes, found on the GPU from the stream's bits
        (flate_hip_inflate_one_index) -> OneIndex(rc, n_units, out_bytes, n_candidates, status, err_off, unit_bit,
        out_off).  A unit starts at bit 0 of the raw stream and at every dynamic-Huffman block header the serial decode
        reaches (after set_option("one_stored_units", 1): at every stored block header too, so that incompressible
        data is many units); unit_bit (numpy uint64[n_units + 1], bits counted from the raw stream's first byte, the last entry the
        bit behind the final block) and out_off (the exclusive prefix sum of what the units inflate to).  status: 0, or
        what the serial decoder says of the stream without looking at its history or its trailer: -4 (at err_off,
        counted from the raw stream's first byte; a bad container header: 0), -7, or -6 for a unit whose input spans
        "one_unit_max" bytes or more; the arrays then hold the good units in front.  n_candidates: the bit offsets
        decoded speculatively.  query=True: only the counts (the arrays are None); index_cap: the arrays' size (default: a
        unit per 256 bytes of input, and a second call only if the stream has more; given and too small: rc -2, the
        arrays None).  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        nu, ob, nc, st, eo = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0), C.c_int32(0), C.c_int64(-1)

        def call(cap, a, b):
            return self._tolerate(self._L.flate_hip_inflate_one_index(
                self._ctx, in_ptr, n, WRAPS[wrap], cap, a, b, C.byref(nu), C.byref(ob), C.byref(nc), C.byref(st),
                C.byref(eo), self._flags(False, False, device)), *PER_CHAIN)

        def result(rc, a, b):
            return OneIndex(rc, int(nu.value), int(ob.value), int(nc.value), int(st.value), int(eo.value), a, b)

        # no query first: the discovery is the whole cost of the call.  A unit per 256 bytes of input is more than
        # zlib writes at its smallest memLevel; a stream that has more takes a second call, sized from the count.
        return _query_then_fill(call, lambda: int(nu.value), result, index_cap, query, prefix=True,
                                guess=n // 256 + 64)

    def inflate_one(self, data, wrap="gzip", out=None, out_cap=None):
        """ONE long stream ("raw", "zlib" or "gzip": one member, many blocks) back into its bytes, its blocks found and
        decoded in parallel on the GPU and its trailer checked there (flate_hip_inflate_one).  Returns (out, OneRead(rc,
        out_len, status, err_off, n_units, n_candidates)); the bytes are out[:out_len] (numpy for host data, a torch
        CUDA tensor for device data).  status is the serial decoder's: 0; -4 at err_off (counted from the raw stream's
        first byte; a bad header: 0; a trailer that does not match: len(data)); -7; -6 for a unit beyond
        "one_unit_max"; the bytes in front of an error are delivered.  rc -2 with out_len > capacity: out too small,
        nothing decoded.  out=None: sized from a gzip member's ISIZE, else (or if that was too little) by a query
        first.  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        ol, st, eo, nu, nc = C.c_uint64(0), C.c_int32(0), C.c_int64(-1), C.c_uint32(0), C.c_uint32(0)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_inflate_one(
                self._ctx, in_ptr, n, WRAPS[wrap], out_ptr, cap, C.byref(ol), C.byref(st), C.byref(eo), C.byref(nu),
                C.byref(nc), self._flags(False, False, device)), *PER_CHAIN)
            return OneRead(rc, int(ol.value), int(st.value), int(eo.value), int(nu.value), int(nc.value))

        if out is None:
            # a gzip member says in its last four bytes what it inflates to (mod 2^32): room for that, and the one
            # call is the decode -- no discovery spent on a size query.  A trailer that is wrong only costs the
            # second call the query would have cost anyway.  (DEFLATE expands at most 1032 times.)
            hint = 0
            if wrap == "gzip" and n >= 18:
                hint = int.from_bytes(_host_bytes(data[n - 4:n]), "little")
                if hint > 1032 * n:
                    hint = 0
            if hint:
                room, ptr, _ = _out_buf(None, data, hint, None, 0, "inflate_one")
                q = call(ptr, hint)
                if not (q.rc == E_OUT_TOO_SMALL and q.out_len > hint):
                    return room, q
            else:
                q = call(None, 0)
                if q.rc != E_OUT_TOO_SMALL:  # nothing to deliver: an empty stream, or a verdict without bytes
                    return _no_bytes(data), q
        return _read_into(out, data, out_cap, "inflate_one", call, lambda: (q.out_len, None))

    def gzip_read(self, data, out=None, out_cap=None):
        """A plain multi-member gzip file back into its bytes by one call (flate_hip_gzip_read): member discovery,
        decode and the check of every member's CRC-32 and ISIZE on the GPU, no side index.  Returns (out, GzipRead(rc,
        out_len, n_members, bad_member, err_off)); the bytes are out[:out_len] (numpy for host data, a torch CUDA tensor
        for device data).  rc 0; a broken chain (bad_member == n_members): gzip_index's rc at err_off, nothing decoded;
        otherwise the first failing member's status (-4 CRC or ISIZE, -2 more output than the slot) with its index and
        file offset, all other members delivered; -2 with out_len > capacity: out too small, nothing decoded.
        out=None: sized by a query of the index first.  Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        ol, nm, bad, eo = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_int64(-1)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_gzip_read(
                self._ctx, in_ptr, n, out_ptr, cap, C.byref(ol), C.byref(nm), C.byref(bad), C.byref(eo),
                self._flags(False, False, device)), *PER_CHAIN)
            return GzipRead(rc, int(ol.value), int(nm.value), int(bad.value), int(eo.value))

        return _read_into(out, data, out_cap, "gzip_read", call,
                          lambda: (self.gzip_index(data, query=True).out_bytes, None))

    def bgzf_read_ranges(self, data, begin, end, virtual=False, out=None, out_cap=None):
        """Random access into a BGZF file (flate_hip_bgzf_read_ranges): the bytes of the ranges [begin[r], end[r]) --
        positions in the file's uncompressed bytes, or (virtual=True) BGZF virtual offsets coffset << 16 | uoffset as
        BAM, tabix and CSI indexes store them -- back to back in out.  Only the members the ranges touch are decoded
        and verified, each once; the chain is validated whole.  data: numpy uint8 / bytes, or a torch uint8 CUDA tensor
        (the bytes then stay on the device).  Returns (out, BgzfRanges(rc, out_off, range_status, n_members, n_decoded,
        bad_member, err_off)): range r is out[out_off[r]:out_off[r + 1]].  rc 0; -1: some range had an invalid virtual
        offset (range_status[r] == -1, zero bytes; the others are delivered); -4 with bad_member == n_members: a
        malformed chain; -2 with out_off[-1] > capacity: out too small, nothing decoded; else the first failing touched
        member's status with its index and file offset.  out=None: sized by the size query first.  begin[r] > end[r]
        and other refusals raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        end = np.ascontiguousarray(end, dtype=np.uint64)
        if begin.ndim != 1 or begin.shape != end.shape:
            raise FlateError(E_INVALID, "bgzf_read_ranges: begin and end must be one-dimensional and of one length")
        nr = begin.size
        out_off = np.zeros(nr + 1, dtype=np.uint64)
        status = np.zeros(max(nr, 1), dtype=np.int32)
        nm, nd, bad, eo = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int64(-1)

        def call(out_ptr, cap):
            rc = self._L.flate_hip_bgzf_read_ranges(self._ctx, in_ptr, n, 1 if virtual else 0, begin.ctypes.data,
                                                    end.ctypes.data, nr, out_ptr, cap, out_off.ctypes.data,
                                                    status.ctypes.data, C.byref(nm), C.byref(nd), C.byref(bad),
                                                    C.byref(eo), self._flags(False, False, device))
            # (E_INVALID is a verdict only where some range carries it; otherwise the call itself was refused)
            invalid_range = rc == E_INVALID and nr and (status[:nr] == E_INVALID).any()
            self._tolerate(rc, *PER_STREAM + ((E_INVALID,) if invalid_range else ()))
            return BgzfRanges(rc, out_off, status[:nr], int(nm.value), int(nd.value), int(bad.value), int(eo.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (int(out_off[nr]), None) if q.rc == E_OUT_TOO_SMALL else (0, q)  # else: nothing to deliver, or a malformed chain

        return _read_into(out, data, out_cap, "bgzf_read_ranges", call, size)

    def zip_write(self, data, in_off, names, compat_go=False, out=None, out_cap=None, index=False):
        """The entries data[in_off[i]:in_off[i + 1]], named names[i] (str or UTF-8 bytes), as ONE ZIP archive that
        zipfile, unzip and every other reader open (flate_hip_zip_write): each entry's data is the raw stream
        deflate_batch gives for it, local headers, central directory and end records are written on the GPU.  data:
        numpy uint8 / bytes (returns the archive as bytes) or a torch uint8 CUDA tensor (returns (out, out_len), the
        archive in out[:out_len] on the device).  index=True: entry_off (numpy uint64[n + 1], the local headers and
        the directory's offset) is appended to the result."""
        data, in_ptr, _, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        in_off, n = _offsets(in_off)
        if n != len(names):
            raise FlateError(E_INVALID, "zip_write: one name per entry")
        name_bytes, name_off = _zip_names(names)
        if out_cap is None and out is None:
            out_cap = int(self._L.flate_hip_zip_bound(in_off.ctypes.data, n, name_off.ctypes.data))
            if out_cap == 0:
                raise FlateError(E_INVALID, "zip_write: a name must have 1 .. 65535 bytes and in_off must not decrease")
        out, out_ptr, cap = _out_buf(out, data, out_cap, out_cap, 0, "zip_write", floor=32)
        entry_off = np.zeros(n + 1, dtype=np.uint64)
        out_len = C.c_uint64(0)
        self._check(self._L.flate_hip_zip_write(self._ctx, in_ptr, in_off.ctypes.data, n, name_bytes.ctypes.data,
                                                name_off.ctypes.data, out_ptr, cap, C.byref(out_len),
                                                entry_off.ctypes.data, self._flags(compat_go, False, device)))
        return _file_result(out, int(out_len.value), device, index, entry_off)

    def _zip_count(self, in_ptr, n, flags):
        """The counting call of flate_hip_zip_index -> (rc: 0 or E_CORRUPT, n_entries, out_bytes, err_off)."""
        ne, ob, eo = C.c_uint32(0), C.c_uint64(0), C.c_int64(-1)
        rc = self._tolerate(self._L.flate_hip_zip_index(self._ctx, in_ptr, n, 0, None, None, C.byref(ne), C.byref(ob),
                                                        C.byref(eo), flags), E_CORRUPT)
        return rc, int(ne.value), int(ob.value), int(eo.value)

    def zip_index(self, data):
        """The entries of a ZIP archive, found on the GPU from the archive's bytes (flate_hip_zip_index) ->
        ZipIndex(rc, n_entries, out_bytes, err_off, entries, out_off, names).  rc 0: entries is a numpy structured
        array (ZIP_ENTRY: name_off, header_off, data_off, comp_size, size, crc32, name_len, method, flags, status),
        out_off (numpy uint64[n + 1]) where each entry's bytes go when all are read, names the entries' names (str;
        bytes where a name is not UTF-8).  rc -4 (FLATE_HIP_E_CORRUPT): a malformed archive at err_off behind
        n_entries good records; the arrays are None.  data: numpy uint8 / bytes, or a torch uint8 CUDA tensor.
        Other failures raise FlateError."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        flags = self._flags(False, False, device)
        rc, cnt, _, err = self._zip_count(in_ptr, n, flags)
        if rc != 0:
            return ZipIndex(rc, cnt, 0, err, None, None, None)
        entries = np.zeros(max(cnt, 1), dtype=ZIP_ENTRY)
        out_off = np.zeros(cnt + 1, dtype=np.uint64)
        ne, ob, eo = C.c_uint32(0), C.c_uint64(0), C.c_int64(-1)
        self._check(self._L.flate_hip_zip_index(self._ctx, in_ptr, n, cnt, entries.ctypes.data, out_off.ctypes.data,
                                                C.byref(ne), C.byref(ob), C.byref(eo), flags))
        entries = entries[:cnt]
        names = []
        if cnt:
            lo = int(entries["name_off"].min())
            hi = int((entries["name_off"] + entries["name_len"]).max())
            blob = _host_bytes(data[lo:hi])
            for e in entries:
                raw = blob[int(e["name_off"]) - lo:int(e["name_off"]) - lo + int(e["name_len"])]
                try:
                    names.append(raw.decode("utf-8"))
                except UnicodeDecodeError:
                    names.append(raw)
        return ZipIndex(0, cnt, int(ob.value), -1, entries, out_off, names)

    def zip_read(self, data, select=None, out=None, out_cap=None):
        """Entries of a ZIP archive back into their bytes by one call (flate_hip_zip_read): discovery, decode
        (deflate through the batch decoders, stored through a copy kernel) and the check of every entry's size and
        CRC-32 on the GPU.  select: entry numbers or names (a list in any order, duplicates allowed; names cost an index
        call first), None = every entry.  Returns (out, ZipRead(rc, out_off, out_len, status, err_off, n_entries,
        archive_err_off)): selected entry j is out[out_off[j]:out_off[j] + out_len[j]] (numpy for host data, a torch
        CUDA tensor for device data).  rc 0; -4 with archive_err_off >= 0: a malformed archive, nothing decoded; -2
        with out_off[-1] > capacity: out too small, nothing decoded; otherwise the first non-zero entry status, all other
        entries delivered.  out=None: sized by the size query first.  A name that is not in the archive raises KeyError;
        other failures raise FlateError.  After set_option("zip_unit_min", v) with v >= 1 a deflated entry of at least v
        compressed bytes (an .npz array, one large CSV) is decoded in parallel through units, with the same results;
        zip_last_route() says which path ran."""
        data, in_ptr, n, device = _in_buf(data, accept_bytes=True, null_if_empty=True)
        flags = self._flags(False, False, device)
        sel = None
        if select is not None:
            select = list(select)
            if any(not isinstance(x, (int, np.integer)) for x in select):
                ix = self.zip_index(data)
                if ix.rc != 0:
                    return out, ZipRead(ix.rc, None, None, None, None, ix.n_entries, ix.err_off)
                where = {}
                for k, name in enumerate(ix.names):
                    where.setdefault(name, k)

                def number(x):
                    if isinstance(x, (int, np.integer)):
                        return int(x)
                    if isinstance(x, (bytes, bytearray)):
                        try:
                            x = bytes(x).decode("utf-8")
                        except UnicodeDecodeError:
                            x = bytes(x)
                    return where[x]

                select = [number(x) for x in select]
            sel = np.ascontiguousarray(select, dtype=np.uint32)
            ns = sel.size
        else:
            rc, ns, _, err = self._zip_count(in_ptr, n, flags)
            if rc != 0:
                return out, ZipRead(rc, None, None, None, None, ns, err)
        out_off = np.zeros(ns + 1, dtype=np.uint64)
        out_len, status, err_off = _stream_results(ns)
        ne, aeo = C.c_uint32(0), C.c_int64(-1)

        def call(out_ptr, cap):
            rc = self._tolerate(self._L.flate_hip_zip_read(
                self._ctx, in_ptr, n, sel.ctypes.data if sel is not None else None, ns if sel is not None else 0, ns,
                out_ptr, cap, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data,
                C.byref(ne), C.byref(aeo), flags), *PER_CHAIN, E_UNSUPPORTED)
            return ZipRead(rc, out_off, out_len[:ns], status[:ns], err_off[:ns], int(ne.value), int(aeo.value))

        def size():  # the size query: nothing is decoded
            q = call(None, 0)
            return (int(out_off[ns]), None) if q.rc == E_OUT_TOO_SMALL else (0, q)

        return _read_into(out, data, out_cap, "zip_read", call, size)

    def _inflate_call(self, in_ptr, in_off, n, zdicts, dict_of, device, out_ptr, off_ptr, results, flags, allowed):
        """flate_hip_inflate_batch, or with zdicts flate_hip_inflate_batch_dict, into results = (out_len, status,
        err_off)."""
        tail = (out_ptr, off_ptr) + tuple(r.ctypes.data for r in results) + (flags | self._flags(False, False, device),)
        if zdicts is None:
            rc = self._L.flate_hip_inflate_batch(self._ctx, in_ptr, in_off.ctypes.data, n, *tail)
        else:
            dk = _DictArgs(zdicts, dict_of, n, device)
            rc = self._L.flate_hip_inflate_batch_dict(self._ctx, in_ptr, in_off.ctypes.data, n, dk.ptr, dk.off_ptr,
                                                      dk.n_dicts, dk.of_ptr, *tail)
        self._tolerate(rc, *allowed)

    def inflate_batch(self, data, in_off, out_sizes, out=None, check=True, zdicts=None, dict_of=None):
        """Decompress independent DEFLATE streams (&Reader::new + read to EOF each).
        out_sizes[i] = capacity reserved for stream i's output (its exact size if known).
        zdicts: preset dictionaries (&Reader::new_dict, flate_hip_inflate_batch_dict) -- one bytes-like object or
        a list of them; dict_of[i] = the dictionary of stream i or NO_DICT (None: every stream uses the first).
        Returns (out, out_off, out_len, status, err_off); with check=True a failing stream raises."""
        in_off, n = _offsets(in_off)
        out_off = _slots(out_sizes, n)
        results = _stream_results(n, pad=False)  # (this call alone returns its tables unpadded and whole)
        data, in_ptr, _, device = _in_buf(data)
        out, out_ptr, _ = _out_buf(out, data, out_off[-1], None, int(out_off[-1]), "inflate")
        self._inflate_call(in_ptr, in_off, n, zdicts, dict_of, device, out_ptr, out_off.ctypes.data, results, 0,
                           () if check else PER_STREAM)
        return (out, out_off) + results

    def inflate_sizes(self, data, in_off, zdicts=None, dict_of=None):
        """Decode without storing (FLATE_HIP_SIZE_ONLY): returns (out_len, status, err_off) -- the size
        every stream inflates to (up to its error, if any).  Host or device input; zdicts / dict_of as in
        inflate_batch."""
        in_off, n = _offsets(in_off)
        results = _stream_results(n)
        data, in_ptr, _, device = _in_buf(data, lax=True)
        self._inflate_call(in_ptr, in_off, n, zdicts, dict_of, device, None, None, results, SIZE_ONLY, PER_STREAM)
        return tuple(r[:n] for r in results)

    def open_inflate_stream(self, zdict=None):
        """One long DEFLATE stream decoded in pieces (see StreamReader); zdict: a preset dictionary
        (&Reader::new_dict, inflate.mbt:315-317)."""
        return StreamReader(self, zdict)

    def open_stream(self, compat_go=False):
        """One stream written in pieces (flate_hip_stream_*): see StreamWriter."""
        return StreamWriter(self, compat_go)

    def deflate_spliced(self, data, in_off, out=None, compat_go=False):
        """Compress the streams as deflate_batch does, but into ONE legal DEFLATE stream that
        inflates to the concatenation of the inputs.
        Returns (out, out_len, bit_off[N+1]): bit_off[i] = bit position of stream i's first block."""
        in_off, n = _offsets(in_off)
        bit_off = np.zeros(n + 1, dtype=np.uint64)
        out_len = C.c_uint64(0)
        data, in_ptr, _, device = _in_buf(data)
        out, out_ptr, cap = _out_buf(out, data, _deflate_room(in_off) + 16, None, 8, "deflate_spliced")
        self._check(self._L.flate_hip_deflate_fast_spliced(
            self._ctx, in_ptr, in_off.ctypes.data, n, out_ptr, cap, C.byref(out_len),
            bit_off.ctypes.data, self._flags(compat_go, False, device)))
        return out, int(out_len.value), bit_off

    def inflate_spliced(self, data, nbytes, bit_off, out_sizes, out=None, check=True):
        """Decompress ONE spliced DEFLATE stream data[:nbytes] in parallel from its index:
        piece i starts at bit bit_off[i].  Returns (out, out_off, out_len, status, err_off)."""
        bit_off, n = _offsets(bit_off)
        out_off = _slots(out_sizes, n)
        out_len, status, err_off = _stream_results(n)
        data, in_ptr, _, device = _in_buf(data)
        out, out_ptr, _ = _out_buf(out, data, out_off[-1], None, int(out_off[-1]), "inflate")
        self._tolerate(self._L.flate_hip_inflate_spliced(
            self._ctx, in_ptr, int(nbytes), bit_off.ctypes.data, n, out_ptr, out_off.ctypes.data, out_len.ctypes.data,
            status.ctypes.data, err_off.ctypes.data, self._flags(False, False, device)),
            0, *(() if check else PER_STREAM))
        return out, out_off, out_len[:n], status[:n], err_off[:n]

    def inflate_spliced_framed(self, data, nbytes, wrap, bit_off, out_sizes, out=None, check=True):
        """The reverse of deflate_spliced_framed: ONE zlib stream or gzip member data[:nbytes] around a spliced
        stream, decoded in parallel from its index and checked against its trailer on the GPU by one call
        (flate_hip_inflate_spliced_framed).  bit_off is counted from the raw stream's first byte, as
        deflate_spliced_framed returns it: the header (also a foreign one with FNAME / FEXTRA) is measured on the
        device.  out_sizes[i] = capacity of piece i's slot.  data: numpy uint8 or a torch uint8 CUDA tensor.
        An index of one entry -- what the writer returns for no input at all -- is one piece of size 0 at bit 0: the
        closing block and the trailer of nothing are still checked.
        Returns (out, out_off, out_len, status, err_off, member_status); member_status is the first non-zero piece
        status, or -4 for a bad header (every piece -4) or a checksum / ISIZE that does not match what the pieces
        produced (every piece 0), else 0.  With check=True a non-zero member status raises FlateError."""
        bit_off, n = _offsets(bit_off)
        out_sizes = np.asarray(out_sizes, dtype=np.uint64)
        if n == 0:
            bit_off, n = np.array([bit_off[0], bit_off[0]], dtype=np.uint64), 1
            out_sizes = np.zeros(1, dtype=np.uint64)
        out_off = _slots(out_sizes, n)
        out_len, status, err_off = _stream_results(n)
        member_status, member_err = C.c_int32(0), C.c_int64(-1)
        data, in_ptr, _, device = _in_buf(data)
        out, out_ptr, _ = _out_buf(out, data, out_off[-1], None, int(out_off[-1]), "inflate_spliced_framed")
        self._tolerate(self._L.flate_hip_inflate_spliced_framed(
            self._ctx, in_ptr, int(nbytes), _wrap_code(wrap), bit_off.ctypes.data, n, out_ptr, out_off.ctypes.data,
            out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, C.byref(member_status),
            C.byref(member_err), self._flags(False, False, device)), *(() if check else PER_STREAM))
        self.last_member_err_off = int(member_err.value)
        return out, out_off, out_len[:n], status[:n], err_off[:n], int(member_status.value)

    def lz77_matches(self, data, in_off, compat_go=False, lz_serial=False):
        """Match finder only.  Returns a list over LZ77 chunks (stream order) of
        (pos uint32[], tok uint32[]) and the per-stream chunk counts."""
        in_off, n = _offsets(in_off)
        data, in_ptr, _, _ = _in_buf(np.asarray(data))
        n_chunks, cap = C.c_uint32(0), C.c_uint64(0)
        flags = self._flags(compat_go, lz_serial, False)
        self._check(self._L.flate_hip_lz77_matches(self._ctx, in_ptr, in_off.ctypes.data, n,
                                                   flags, C.byref(n_chunks), C.byref(cap),
                                                   None, None, None))
        nc = n_chunks.value
        nmatch = np.zeros(max(nc, 1), dtype=np.uint32)
        rec_off = np.zeros(nc + 1, dtype=np.uint64)
        recs = np.zeros((max(cap.value, 1), 2), dtype=np.uint32)
        self._check(self._L.flate_hip_lz77_matches(self._ctx, in_ptr, in_off.ctypes.data, n,
                                                   flags, C.byref(n_chunks), C.byref(cap),
                                                   nmatch.ctypes.data, rec_off.ctypes.data,
                                                   recs.ctypes.data))
        out = []
        for c in range(nc):
            r = recs[int(rec_off[c]):int(rec_off[c]) + int(nmatch[c])]
            out.append((r[:, 0].copy(), r[:, 1].copy()))
        return out


def _piece(x):
    """(a piece of a stream as contiguous numpy uint8 -- bytes-like or an array, None = nothing; its pointer, NULL for
    no bytes; its size)."""
    if not isinstance(x, np.ndarray):
        x = np.frombuffer(bytes(x if x is not None else b""), dtype=np.uint8)
    x, ptr, nbytes, _ = _in_buf(x, null_if_empty=True)
    return x, ptr, nbytes


class StreamWriter:
    """Writer::write as the reference behaves for ONE long stream: every write() of whole
    65535-byte windows returns the compressed bytes that are complete so far; close(tail) ends the
    stream.  The concatenation equals deflate_batch of the whole stream, bit for bit."""
    WINDOW = MAX_STORE_BLOCK_SIZE

    def __init__(self, eng, compat_go=False):
        self._eng, self._L = eng, eng._L
        self._st = C.c_void_p()
        eng._check(self._L.flate_hip_stream_open(eng._ctx, COMPAT_GO if compat_go else 0, C.byref(self._st)))

    def _write(self, piece, final):
        piece, ptr, nbytes = _piece(piece)
        out, out_ptr, cap = _out_buf(None, piece, self._L.flate_hip_stream_bound(nbytes), None, 0, "write", floor=0)
        n = C.c_uint64(0)
        self._eng._check(self._L.flate_hip_stream_write(self._st, ptr, nbytes, 1 if final else 0, out_ptr, cap,
                                                        C.byref(n)))
        return out[:int(n.value)]

    def write(self, piece):
        """piece: a multiple of 65535 bytes.  Returns the output bytes finished by it."""
        return self._write(piece, False)

    def close(self, tail=b""):
        """The rest of the stream (any length) and Writer::close.  Returns the last output bytes."""
        out = self._write(tail, True)
        self.free()
        return out

    def free(self):
        if self._st:
            self._L.flate_hip_stream_free(self._st)
            self._st = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StreamReader:
    """Decompressor::read as the reference behaves for ONE long stream (flate_hip_inflate_stream_*): the
    caller feeds pieces of the compressed stream and takes pieces of output; the decoder's state rests
    on the device in between.  `feed(piece, final, room)` returns (out bytes, status): status 0 = go on,
    1 = end of stream, < 0 = the stream's error (err_off holds corrupt_input_error's offset)."""

    def __init__(self, eng, zdict=None):
        self._eng, self._L = eng, eng._L
        self._st = C.c_void_p()
        eng._check(self._L.flate_hip_inflate_stream_open(eng._ctx, C.byref(self._st)))
        self._rest = np.zeros(0, dtype=np.uint8)  # bytes a call reported as unused
        self.err_off = -1
        self.total_in = 0
        if zdict is not None and len(zdict):
            self.reset(zdict)

    def reset(self, zdict=None):
        """Decompressor::reset(r, dict) (inflate.mbt:862-884): a fresh decoder on the same handle, with the
        last 32768 bytes of zdict as history that has already been read."""
        _, ptr, nbytes = _piece(zdict)
        self._eng._check(self._L.flate_hip_inflate_stream_reset(self._st, ptr, nbytes))
        self._rest = np.zeros(0, dtype=np.uint8)
        self.err_off = -1
        self.total_in = 0

    def feed(self, piece, final=False, room=1 << 20):
        piece, _, _ = _piece(piece)
        buf, ptr, nbytes = _piece(np.concatenate([self._rest, piece]) if self._rest.size else piece)
        out, out_ptr, cap = _out_buf(None, buf, room, room, 0, "feed", floor=1)
        used, n, eo = C.c_uint64(0), C.c_uint64(0), C.c_int64(-1)
        rc = self._eng._tolerate(self._L.flate_hip_inflate_stream_read(
            self._st, ptr, nbytes, 1 if final else 0, out_ptr, cap, C.byref(used), C.byref(n), C.byref(eo)),
            1, E_CORRUPT, E_UNEXPECTED_EOF)  # (1: the end of the stream)
        self._rest = buf[int(used.value):].copy()
        self.total_in += int(used.value)
        self.err_off = int(eo.value)
        return out[:int(n.value)], rc

    @property
    def pending_input(self):
        return int(self._rest.size)

    def free(self):
        if self._st:
            self._L.flate_hip_inflate_stream_free(self._st)
            self._st = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


OnePartRead = collections.namedtuple("OnePartRead", "rc out_len err_off n_units")


class OneReader:
    """flate_hip_inflate_one on a stream the caller holds a part at a time (flate_hip_one_reader_*): every read() decodes
    the units that lie whole inside the part, in parallel, and the handle carries the bit where the next unit starts,
    the 32 KiB window and the running checksum.  read(part, final, out, out_cap) -> (in_used, out, OnePartRead(rc,
    out_len, err_off, n_units)): `part` BEGINS with the bytes the last read left unused (part[in_used:], then new
    bytes); the bytes are out[:out_len]; rc 0 = go on, 1 = the end of the stream (trailer checked), -2 = not even the
    first unit fits (out_len: its size; nothing changed), -4 / -7 / -6 = the stream's error, sticky.  out=None: room
    for out_cap bytes (default: four times the part, 64 KiB at least), and with no out_cap a first unit that does not
    fit gets a second call with room for it.  The unit rule and "one_unit_max" are the engine's at open."""

    def __init__(self, eng, wrap="gzip", device=False):
        self._eng, self._L = eng, eng._L
        self._device = bool(device)
        self._h = C.c_void_p()
        eng._check(self._L.flate_hip_one_reader_open(eng._ctx, WRAPS[wrap], eng._flags(False, False, self._device),
                                                     C.byref(self._h)))

    def read(self, part, final=False, out=None, out_cap=None):
        part, in_ptr, n, device = _in_buf(part, accept_bytes=True, null_if_empty=True)
        if device != self._device:
            raise FlateError(E_INVALID, "OneReader.read: the part is not on the side the reader was opened for")
        used, ol, eo, nu = C.c_uint64(0), C.c_uint64(0), C.c_int64(-1), C.c_uint32(0)

        def call(out_ptr, cap):
            rc = self._eng._tolerate(self._L.flate_hip_one_reader_read(
                self._h, in_ptr, n, 1 if final else 0, out_ptr, cap, C.byref(used), C.byref(ol), C.byref(eo),
                C.byref(nu)), 1, *PER_CHAIN)  # (1: the end of the stream)
            return OnePartRead(rc, int(ol.value), int(eo.value), int(nu.value))

        size = max(4 * n, 1 << 16) if out_cap is None else int(out_cap)
        buf, ptr, cap = _out_buf(out, part, size, out_cap, 0, "OneReader.read", floor=1)
        res = call(ptr, cap)
        if res.rc == E_OUT_TOO_SMALL and out is None and out_cap is None:
            buf, ptr, cap = _out_buf(None, part, res.out_len, None, 0, "OneReader.read", floor=1)
            res = call(ptr, cap)
        return int(used.value), (buf[:0] if res.rc == E_OUT_TOO_SMALL else buf[:res.out_len]), res

    def reset(self):
        """A fresh stream on the same handle: same wrap, same side, same options."""
        self._eng._check(self._L.flate_hip_one_reader_reset(self._h))

    def close(self):
        if self._h:
            self._L.flate_hip_one_reader_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GzFilePartRead = collections.namedtuple("GzFilePartRead", "rc out_len n_members n_units bad_member err_off stream_err_off")


class GzFileReader:
    """flate_hip_gzfile_read on a file the caller holds a part at a time (flate_hip_gzfile_reader_*): every read()
    decodes the units that lie whole inside the part, across the members in it, judges the trailers of the members that
    end among them, and the handle carries where the file stands.  read(part, final, out, out_cap) -> (in_used, out,
    GzFilePartRead(rc, out_len, n_members, n_units, bad_member, err_off, stream_err_off)): `part` BEGINS with the bytes
    the last read left unused; the bytes are out[:out_len]; rc 0 = go on, 1 = the end of the file, -2 = not even the
    first unit fits (out_len: its size; nothing changed), -4 / -7 / -6 = the file's error, sticky, with the three words
    counted over the FILE.  out=None behaves as OneReader's.  The unit rule and "one_unit_max" are the engine's at
    open; the engine's option "gzfile_serial_max" is not used: the reader has a setting of its own.
    set_serial_max(S), on a fresh reader (behind open or reset, before a read has consumed a byte; reset keeps it): with
    S >= 1 a member that lies whole inside a part, fits in S bytes, decodes cleanly and inflates to at most out_cap
    bytes is ONE unit, decoded with all other such members of the read by one batch of the batch decoders -- no
    bit-offset search, no symbolic pass; every other member, and the member continued from the last part, is cut into
    units as with S = 0.  A member that the part cuts but that could still fit in S bytes ends the read in front of its
    header (in_used is the header's offset) so that the next part takes it whole; if it is the part's first member it
    is read through units, so no part needs a minimum size.  Bytes, verdicts and the sum of in_used are the same for
    every S; n_units and in_used of a single read depend on it.  last_route() -> (serial_members, open_stop, find_from)
    of the last read that ran a discovery: the whole members among the units it delivered, whether its chain ended in
    front of a member that more bytes could make whole, and the part offset the bit-offset search started at
    (len(part): none ran; 0 with S = 0)."""

    def __init__(self, eng, device=False):
        self._eng, self._L = eng, eng._L
        self._device = bool(device)
        self._h = C.c_void_p()
        eng._check(self._L.flate_hip_gzfile_reader_open(eng._ctx, eng._flags(False, False, self._device), C.byref(self._h)))

    def read(self, part, final=False, out=None, out_cap=None):
        part, in_ptr, n, device = _in_buf(part, accept_bytes=True, null_if_empty=True)
        if device != self._device:
            raise FlateError(E_INVALID, "GzFileReader.read: the part is not on the side the reader was opened for")
        used, ol = C.c_uint64(0), C.c_uint64(0)
        nm, nu, bm = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0xffffffff)
        eo, so = C.c_int64(-1), C.c_int64(-1)

        def call(out_ptr, cap):
            rc = self._eng._tolerate(self._L.flate_hip_gzfile_reader_read(
                self._h, in_ptr, n, 1 if final else 0, out_ptr, cap, C.byref(used), C.byref(ol), C.byref(nm),
                C.byref(nu), C.byref(bm), C.byref(eo), C.byref(so)), 1, *PER_CHAIN)  # (1: the end of the file)
            return GzFilePartRead(rc, int(ol.value), int(nm.value), int(nu.value), int(bm.value), int(eo.value),
                                  int(so.value))

        size = max(4 * n, 1 << 16) if out_cap is None else int(out_cap)
        buf, ptr, cap = _out_buf(out, part, size, out_cap, 0, "GzFileReader.read", floor=1)
        res = call(ptr, cap)
        if res.rc == E_OUT_TOO_SMALL and out is None and out_cap is None:
            buf, ptr, cap = _out_buf(None, part, res.out_len, None, 0, "GzFileReader.read", floor=1)
            res = call(ptr, cap)
        return int(used.value), (buf[:0] if res.rc == E_OUT_TOO_SMALL else buf[:res.out_len]), res

    def reset(self):
        """A fresh file on the same handle: same side, same options."""
        self._eng._check(self._L.flate_hip_gzfile_reader_reset(self._h))

    def set_serial_max(self, serial_max):
        """Members of at most serial_max bytes that lie whole inside a part are decoded whole (0: none; at most
        2^28 - 1).  Only on a fresh reader: FlateError(E_INVALID) otherwise."""
        self._eng._check(self._L.flate_hip_gzfile_reader_set_serial_max(self._h, int(serial_max)))

    def last_route(self):
        """(serial_members, open_stop, find_from) of the last read that ran a discovery (the class docstring)."""
        sm, os_, ff = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self._eng._check(self._L.flate_hip_gzfile_reader_last_route(self._h, C.byref(sm), C.byref(os_), C.byref(ff)))
        return int(sm.value), int(os_.value), int(ff.value)

    def close(self):
        if self._h:
            self._L.flate_hip_gzfile_reader_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


OnePartWrite = collections.namedtuple("OnePartWrite", "rc out_len n_pieces bit_off")


def one_writer_bound(in_len, piece_bytes=0):
    """Room that holds any OneWriter.write of at most in_len bytes (flate_hip_one_writer_bound)."""
    return int(_lib.load().flate_hip_one_writer_bound(int(in_len), int(piece_bytes)))


class OneWriter:
    """deflate_spliced_framed for a stream the caller holds a part at a time (flate_hip_one_writer_*): every write()
    compresses the whole pieces of piece_bytes bytes that the part holds, in parallel, and the handle carries the last
    incomplete byte, the running checksum and the lengths on the device.  The concatenation of what the writes return
    is, byte for byte, deflate_spliced_framed of the whole input cut every piece_bytes bytes, whatever the parts.
    write(part, final, out, out_cap, index) -> (in_used, out, OnePartWrite(rc, out_len, n_pieces, bit_off)): `part`
    BEGINS with the bytes the last write left unused (part[in_used:], then new bytes); the bytes are out[:out_len]; rc 0
    = go on, 1 = the stream is finished (final=True: closing block and trailer written), -2 = out_cap is too small
    (out_len: the bytes needed; nothing changed).  index=True: bit_off holds the start bits of the n_pieces pieces,
    counted from the raw stream's first byte, and on a final write one entry more, where the closing block starts; else
    None.  out=None: room for out_cap bytes (default: the part and an eighth), and with no out_cap a call that does
    not fit gets a second call with room for it."""

    def __init__(self, eng, wrap="gzip", piece_bytes=0, device=False, compat_go=False):
        self._eng, self._L = eng, eng._L
        self._device = bool(device)
        self.piece_bytes = int(piece_bytes) or MAX_STORE_BLOCK_SIZE
        self._h = C.c_void_p()
        eng._check(self._L.flate_hip_one_writer_open(eng._ctx, WRAPS[wrap], int(piece_bytes),
                                                     eng._flags(compat_go, False, self._device), C.byref(self._h)))

    def write(self, part, final=False, out=None, out_cap=None, index=False):
        if part is None and self._device:
            import torch
            part = torch.empty(0, dtype=torch.uint8, device="cuda:%d" % self._eng.device)
        part, in_ptr, n, device = _in_buf(b"" if part is None else part, accept_bytes=True, null_if_empty=True)
        if device != self._device:
            raise FlateError(E_INVALID, "OneWriter.write: the part is not on the side the writer was opened for")
        used, ol, npc = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        bit_off = np.zeros(n // self.piece_bytes + 2, dtype=np.uint64)

        def call(out_ptr, cap):
            rc = self._eng._tolerate(self._L.flate_hip_one_writer_write(
                self._h, in_ptr, n, 1 if final else 0, out_ptr, cap, C.byref(used), C.byref(ol),
                bit_off.ctypes.data if index else None, C.byref(npc)), 1, E_OUT_TOO_SMALL)  # (1: the stream is finished)
            k = int(npc.value)
            return OnePartWrite(rc, int(ol.value), k, bit_off[:k + (1 if rc == 1 else 0)] if index and rc >= 0 else None)

        size = n + n // 8 + 4096 if out_cap is None else int(out_cap)
        buf, ptr, cap = _out_buf(out, part, size, out_cap, 0, "OneWriter.write", floor=1)
        res = call(ptr, cap)
        if res.rc == E_OUT_TOO_SMALL and out is None and out_cap is None:
            buf, ptr, cap = _out_buf(None, part, res.out_len, None, 0, "OneWriter.write", floor=1)
            res = call(ptr, cap)
        return int(used.value), (buf[:0] if res.rc == E_OUT_TOO_SMALL else buf[:res.out_len]), res

    def reset(self):
        """A fresh stream on the same handle: same wrap, same piece size, same side, same flags."""
        self._eng._check(self._L.flate_hip_one_writer_reset(self._h))

    def close(self):
        if self._h:
            self._L.flate_hip_one_writer_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BgzfPartRead = collections.namedtuple("BgzfPartRead", "rc out_len n_members bad_member err_off eof_marker member_off out_off")


class BgzfReader:
    """bgzf_read on a file the caller holds a part at a time (flate_hip_bgzf_reader_*): every read() decodes the members
    that lie whole inside the part and fit the room, and the handle carries where the file stands (a few host words:
    any other call of the engine may run between two reads).  read(part, final, out, out_cap, index) -> (in_used, out,
    BgzfPartRead(rc, out_len, n_members, bad_member, err_off, eof_marker, member_off, out_off)): `part` BEGINS with the
    bytes the last read left unused (a member the part cuts is left unused); the bytes are out[:out_len]; rc 0 = go on,
    1 = the end of the file, -2 with bad_member 0xffffffff = not even the first member fits (out_len: its size; nothing
    changed), anything else below 0 = the file's error, sticky, behind the good members in front of it, with bad_member
    and err_off counted over the FILE.  A part of at least 65536 bytes, or a final one, always makes progress or gives
    a verdict.  index: False, True (room for every member the part can hold) or a number of entries; member_off and
    out_off then hold the n_members + 1 FILE offsets of the delivered members, compressed and uncompressed, and a
    smaller room clips the read as out_cap does; else None.  out=None behaves as OneReader's."""

    def __init__(self, eng, device=False):
        self._eng, self._L = eng, eng._L
        self._device = bool(device)
        self._h = C.c_void_p()
        eng._check(self._L.flate_hip_bgzf_reader_open(eng._ctx, eng._flags(False, False, self._device), C.byref(self._h)))

    def read(self, part, final=False, out=None, out_cap=None, index=False):
        part, in_ptr, n, device = _in_buf(part, accept_bytes=True, null_if_empty=True)
        if device != self._device:
            raise FlateError(E_INVALID, "BgzfReader.read: the part is not on the side the reader was opened for")
        used, ol = C.c_uint64(0), C.c_uint64(0)
        nm, bm, eo, em = C.c_uint32(0), C.c_uint32(0xffffffff), C.c_int64(-1), C.c_int(0)
        with_index = index is not False and index is not None
        index_cap = (n // 28 + 2) if index is True else int(index) if with_index else 0
        moff = np.zeros(max(index_cap, 1), dtype=np.uint64) if with_index else None
        ooff = np.zeros(max(index_cap, 1), dtype=np.uint64) if with_index else None

        def call(out_ptr, cap):
            rc = self._eng._tolerate(self._L.flate_hip_bgzf_reader_read(
                self._h, in_ptr, n, 1 if final else 0, out_ptr, cap, C.byref(used), C.byref(ol), index_cap,
                moff.ctypes.data if with_index else None, ooff.ctypes.data if with_index else None, C.byref(nm),
                C.byref(bm), C.byref(eo), C.byref(em)), 1, E_UNSUPPORTED, *PER_CHAIN)  # (1: the end of the file)
            k = int(nm.value)
            return BgzfPartRead(rc, int(ol.value), k, int(bm.value), int(eo.value), int(em.value),
                                moff[:k + 1].copy() if with_index else None, ooff[:k + 1].copy() if with_index else None)

        size = max(4 * n, 1 << 16) if out_cap is None else int(out_cap)
        buf, ptr, cap = _out_buf(out, part, size, out_cap, 0, "BgzfReader.read", floor=1)
        res = call(ptr, cap)
        if res.rc == E_OUT_TOO_SMALL and res.bad_member == 0xffffffff and out is None and out_cap is None:
            buf, ptr, cap = _out_buf(None, part, res.out_len, None, 0, "BgzfReader.read", floor=1)
            res = call(ptr, cap)
        repeatable = res.rc == E_OUT_TOO_SMALL and res.bad_member == 0xffffffff
        return int(used.value), (buf[:0] if repeatable else buf[:res.out_len]), res

    def reset(self):
        """A fresh file on the same handle: same side."""
        self._eng._check(self._L.flate_hip_bgzf_reader_reset(self._h))

    def close(self):
        if self._h:
            self._L.flate_hip_bgzf_reader_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BgzfPartWrite = collections.namedtuple("BgzfPartWrite", "rc out_len n_blocks member_off")


def bgzf_writer_bound(in_len, block_bytes=0):
    """Room that holds any BgzfWriter.write of at most in_len bytes (flate_hip_bgzf_writer_bound; 0: block_bytes is
    refused)."""
    return int(_lib.load().flate_hip_bgzf_writer_bound(int(in_len), int(block_bytes)))


class BgzfWriter:
    """bgzf_write for an input the caller holds a part at a time (flate_hip_bgzf_writer_*): every write() compresses
    the whole blocks of block_bytes bytes that the part holds, and only the final one ends with the EOF marker.  The
    concatenation of what the writes return is, byte for byte, bgzf_write of the whole input, whatever the parts.
    write(part, final, out, out_cap, index) -> (in_used, out, BgzfPartWrite(rc, out_len, n_blocks, member_off)): `part`
    BEGINS with the bytes the last write left unused; the bytes are out[:out_len]; rc 0 = go on, 1 = the file is
    finished, -2 = out_cap is too small, -6 = a block that 65536 bytes cannot express (both: nothing changed).
    index=True: member_off holds the n_blocks + 1 FILE offsets of the members written and of what follows them (the
    next member, or the marker); else None.  out=None: room for bgzf_writer_bound of the part."""

    def __init__(self, eng, block_bytes=0, device=False, compat_go=False):
        self._eng, self._L = eng, eng._L
        self._device = bool(device)
        self.block_bytes = int(block_bytes) or BGZF_BLOCK_DEFAULT
        self._bb = int(block_bytes)
        self._h = C.c_void_p()
        eng._check(self._L.flate_hip_bgzf_writer_open(eng._ctx, int(block_bytes), eng._flags(compat_go, False, self._device),
                                                      C.byref(self._h)))

    def write(self, part, final=False, out=None, out_cap=None, index=False):
        if part is None and self._device:
            import torch
            part = torch.empty(0, dtype=torch.uint8, device="cuda:%d" % self._eng.device)
        part, in_ptr, n, device = _in_buf(b"" if part is None else part, accept_bytes=True, null_if_empty=True)
        if device != self._device:
            raise FlateError(E_INVALID, "BgzfWriter.write: the part is not on the side the writer was opened for")
        used, ol, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        member_off = np.zeros(n // self.block_bytes + 2, dtype=np.uint64)
        size = bgzf_writer_bound(n, self._bb) if out_cap is None else int(out_cap)
        buf, ptr, cap = _out_buf(out, part, size, out_cap, 0, "BgzfWriter.write", floor=1)
        rc = self._eng._tolerate(self._L.flate_hip_bgzf_writer_write(
            self._h, in_ptr, n, 1 if final else 0, ptr, cap, C.byref(used), C.byref(ol),
            member_off.ctypes.data if index else None, C.byref(nb)), 1, E_OUT_TOO_SMALL, E_TOO_LARGE)  # (1: finished)
        k = int(nb.value)
        res = BgzfPartWrite(rc, int(ol.value), k, member_off[:k + 1] if index and rc >= 0 else None)
        return int(used.value), buf[:res.out_len], res

    def reset(self):
        """A fresh file on the same handle: same block size, same side, same flags."""
        self._eng._check(self._L.flate_hip_bgzf_writer_reset(self._h))

    def close(self):
        if self._h:
            self._L.flate_hip_bgzf_writer_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _gzip_isizes(data, in_off):
    """ISIZE (RFC 1952 2.3.1: the last four bytes, little endian) of every gzip member data[in_off[i]:in_off[i+1]],
    gathered in one indexing step (host or device data); a member of fewer than 18 bytes cannot be one: 0."""
    lens = (in_off[1:] - in_off[:-1]).astype(np.int64)
    ok = lens >= 18
    at = np.where(ok, in_off[1:].astype(np.int64) - 4, 0)
    idx = at[:, None] + np.arange(4, dtype=np.int64)[None, :]
    if not ok.any():
        return np.zeros(lens.size, dtype=np.uint64)
    if _is_torch(data):
        import torch
        b = data[torch.from_numpy(idx.reshape(-1)).to(data.device)].cpu().numpy().reshape(-1, 4)
    else:
        b = data[idx.reshape(-1)].reshape(-1, 4)
    v = b.astype(np.uint64) @ np.array([1, 1 << 8, 1 << 16, 1 << 24], dtype=np.uint64)
    return np.where(ok, v, 0).astype(np.uint64)


def _dict_list(zdicts):
    """zdicts as a list of dictionaries: one bytes-like object (or 1-D tensor) is a list of one."""
    if isinstance(zdicts, (bytes, bytearray, memoryview, np.ndarray)) or _is_torch(zdicts):
        return [zdicts]
    return list(zdicts)


class _DictArgs:
    """The dictionary arguments of flate_hip_inflate_batch_dict (kept alive as long as this object): the
    dictionaries packed into one buffer (on the device when the call's pointers are), dict_off, dict_of.
    zdicts=None: the arguments of a call without dictionaries (NULL, NULL, 0, NULL)."""

    def __init__(self, zdicts, dict_of, n, device):
        self.buf = self.off = self.of = self.ptr = self.off_ptr = self.of_ptr = None
        self.n_dicts = 0
        if zdicts is None:
            return
        if device and _is_torch(zdicts):  # one dictionary already on the device
            import torch
            assert zdicts.dtype == torch.uint8 and zdicts.is_cuda and zdicts.is_contiguous()
            self.buf = zdicts
            lens = [zdicts.numel()]
        else:
            parts = [np.frombuffer(bytes(d), dtype=np.uint8) if not _is_torch(d) else d.cpu().numpy()
                     for d in _dict_list(zdicts)]
            lens = [p.size for p in parts]
            self.buf = np.concatenate(parts + [np.zeros(16, np.uint8)])
            if device:
                import torch
                self.buf = torch.from_numpy(self.buf).cuda()
        self.off = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(np.asarray(lens, dtype=np.uint64), out=self.off[1:])
        self.n_dicts = len(lens)
        self.ptr = self.buf.data_ptr() if _is_torch(self.buf) else self.buf.ctypes.data
        self.off_ptr = self.off.ctypes.data
        if dict_of is not None:
            self.of = np.ascontiguousarray(dict_of, dtype=np.uint32)
            assert self.of.size == n
            self.of_ptr = self.of.ctypes.data


def zlib_dict_ids(zdicts):
    """{Adler-32 of the whole dictionary (a zlib DICTID, RFC 1950 2.2): index} of preset dictionaries."""
    ids = {}
    for j, d in enumerate(_dict_list(zdicts)):
        ids.setdefault(zlib.adler32(bytes(d.cpu().numpy() if _is_torch(d) else d)), j)
    return ids


def zlib_dict_header(zdict):
    """The six header bytes of a zlib member written with preset dictionary `zdict`: CMF / FLG of ZLIB_HEADER with
    FDICT set and FCHECK recomputed, then DICTID = the dictionary's Adler-32, big endian (RFC 1950 2.2)."""
    cmf, flg = ZLIB_HEADER[0], (ZLIB_HEADER[1] & 0xC0) | 0x20
    flg |= 31 - ((cmf << 8) | flg) % 31
    d = zdict.cpu().numpy() if _is_torch(zdict) else zdict
    return bytes([cmf, flg]) + zlib.adler32(bytes(d)).to_bytes(4, "big")


def zlib_member_header(m, ids):
    """(header bytes, trailer bytes, dictionary) of one zlib member: the dictionary is NO_DICT, or with FDICT
    the index its DICTID has in ids (zlib_dict_ids); (-1, 0, NO_DICT) = not valid -- also FDICT without ids or
    with a DICTID that is not there."""
    h, t = parse_container_header(m, "zlib", fdict=ids is not None)
    if h != 6:
        return h, t, NO_DICT
    j = ids.get(int.from_bytes(bytes(m[2:6]), "big"))
    return (-1, 0, NO_DICT) if j is None else (h, t, j)


def parse_container_header(m, wrap, fdict=False):
    """(header bytes, trailer bytes) of one zlib / gzip member, or (-1, 0) if its header is not valid
    (RFC 1950 2.2: CM = 8, window <= 32 KiB, FCHECK, no preset dictionary unless fdict -- then FDICT gives a
    6-byte header, DICTID in bytes 2-5; RFC 1952 2.3: magic, CM = 8, reserved flag bits zero, the optional
    fields skipped)."""
    m = bytes(m[:min(len(m), 70000)])
    if wrap == "zlib":
        if len(m) < 2 or (m[0] & 15) != 8 or (m[0] >> 4) > 7 or ((m[0] << 8) | m[1]) % 31:
            return -1, 0
        if m[1] & 0x20:
            return (6, 4) if fdict and len(m) >= 6 else (-1, 0)
        return 2, 4
    if len(m) < 10 or m[0] != 0x1f or m[1] != 0x8b or m[2] != 8 or (m[3] & 0xe0):
        return -1, 0
    flg, p = m[3], 10
    if flg & 4:  # FEXTRA
        if len(m) < p + 2:
            return -1, 0
        p += 2 + int.from_bytes(m[p:p + 2], "little")
    for bit in (8, 16):  # FNAME, FCOMMENT: zero-terminated
        if flg & bit:
            z = m.find(b"\0", p)
            if z < 0:
                return -1, 0
            p = z + 1
    if flg & 2:  # FHCRC
        p += 2
    return (p, 8) if p <= len(m) else (-1, 0)


def lz_chunks(stream_len):
    """(start, length) of the LZ77 chunks of one stream (Compressor::enc_speed policy)."""
    full, r = divmod(int(stream_len), MAX_STORE_BLOCK_SIZE)
    ch = [(i * MAX_STORE_BLOCK_SIZE, MAX_STORE_BLOCK_SIZE) for i in range(full)]
    if r >= 128:
        ch.append((full * MAX_STORE_BLOCK_SIZE, r))
    return ch


def tokens_from_matches(chunk_bytes, pos, tok):
    """Expand match records into the reference's token array (token.mbt:69,76)."""
    src = np.frombuffer(bytes(chunk_bytes), dtype=np.uint8) if not isinstance(chunk_bytes, np.ndarray) \
        else chunk_bytes
    n = src.size
    pos = pos.astype(np.int64)
    lens = ((tok >> 22) & 0xFF).astype(np.int64) + 3
    covered = np.zeros(n + 1, dtype=np.int64)
    np.add.at(covered, pos, 1)
    np.add.at(covered, np.minimum(pos + lens, n), -1)
    inside = np.cumsum(covered[:n]) > 0
    is_start = np.zeros(n, dtype=bool)
    is_start[pos] = True
    keep = (~inside) | is_start
    vals = src.astype(np.uint32)
    vals[pos] = tok
    return vals[keep]
