"""The expected bytes of deflate with a preset dictionary as HISTORY (flate_hip_deflate_fast_batch_dict), computed
on the CPU from the oracle's exported functions: a fresh DeflateFast runs encode() over the dictionary's last
32768 bytes and its tokens are dropped, then the payload goes through the Compressor driver as it is
(65535-byte windows, enc_speed's size policy deflate.mbt:236-277, close).  Nothing under oracle/ changes: this
file only declares prototypes of functions the oracle library already exports.

TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from oracle import pyoracle

WINDOW = pyoracle.MAX_STORE_BLOCK_SIZE
DICT_MAX = 32768


class _Sink(C.Structure):  # orc_sink
    _fields_ = [("p", C.c_void_p), ("len", C.c_size_t), ("cap", C.c_size_t), ("err", C.c_int)]


_ready = False


def _lib():
    global _ready
    L = pyoracle.lib()
    if not _ready:
        vp = C.c_void_p
        L.orc_bw_init.argtypes = [vp, vp, C.c_int]
        L.orc_bw_flush.argtypes = [vp]
        L.orc_bw_write_stored_header.argtypes = [vp, C.c_int, C.c_int]
        L.orc_bw_write_bytes.argtypes = [vp, vp, C.c_int]
        for name in ("orc_bw_init", "orc_bw_flush", "orc_bw_write_stored_header", "orc_bw_write_bytes"):
            getattr(L, name).restype = None
        L.orc_bw_write_block_dynamic.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int]
        L.orc_bw_write_block_dynamic.restype = C.c_int
        L.orc_bw_write_block_huff.argtypes = [vp, C.c_int, vp, C.c_int]
        L.orc_bw_write_block_huff.restype = C.c_int
        L.orc_df_new.restype = C.c_void_p
        _ready = True
    return L


def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def deflate_dict(data, zdict=None, compat=pyoracle.COMPAT_MOONBIT):
    """Raw DEFLATE bytes of `data` written by a Writer that has seen `zdict` (None / empty: no dictionary)."""
    L = _lib()
    src = _u8(data)
    d = _u8(zdict)[-DICT_MAX:] if zdict is not None and len(zdict) else np.zeros(0, np.uint8)
    cap = int(L.orc_deflate_bound(src.size)) + 64
    out = np.empty(cap, dtype=np.uint8)
    sink = _Sink(out.ctypes.data, 0, cap, 0)
    bw = np.zeros(1 << 16, dtype=np.uint8)  # an orc_bit_writer (opaque, a few KiB)
    toks = np.empty(WINDOW + 2, dtype=np.uint32)  # (room for the end-of-block token)
    L.orc_bw_init(bw.ctypes.data, C.addressof(sink), compat)
    e = C.c_void_p(L.orc_df_new(compat))
    try:
        if d.size:
            L.orc_df_encode(e, toks.ctypes.data, 0, d.ctypes.data, d.size)  # tokens dropped
        for s in range(0, src.size, WINDOW):
            w = np.ascontiguousarray(src[s:s + WINDOW])
            n = w.size
            if n < WINDOW and n < 128:
                if n <= 16:
                    L.orc_bw_write_stored_header(bw.ctypes.data, n, 0)
                    L.orc_bw_write_bytes(bw.ctypes.data, w.ctypes.data, n)
                else:
                    L.orc_bw_write_block_huff(bw.ctypes.data, 0, w.ctypes.data, n)
                L.orc_df_reset(e)
                continue
            nt = L.orc_df_encode(e, toks.ctypes.data, 0, w.ctypes.data, n)
            if nt > n - (n >> 4):
                L.orc_bw_write_block_huff(bw.ctypes.data, 0, w.ctypes.data, n)
            else:
                L.orc_bw_write_block_dynamic(bw.ctypes.data, toks.ctypes.data, nt, 0, w.ctypes.data, n)
        L.orc_bw_write_stored_header(bw.ctypes.data, 0, 1)
        L.orc_bw_flush(bw.ctypes.data)
    finally:
        L.orc_df_free(e)
    assert sink.err == 0, "the reference writer overflowed its sink"
    return out[:sink.len].tobytes()
