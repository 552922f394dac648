"""ctypes loader of libflate_hip.so.  There is no fallback: a missing library is an error."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# FLATE_HIP_LIB: developer override to A/B an experimental build of the same library
LIB_PATH = os.environ.get("FLATE_HIP_LIB") or os.path.join(HERE, "lib", "libflate_hip.so")


def _signatures():
    """Every symbol include/flate_hip.h declares: name -> (restype, argtypes).  vp stands for every pointer to a buffer
    or a table (the wrapper passes addresses); the typed pointers are the scalars a call writes (ctypes.byref)."""
    i, i32, i64, u32, u64, f32, sz, vp, s = (C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t,
                                            C.c_void_p, C.c_char_p)
    ip, i32p, i64p, u32p, u64p, f32p, vpp = (C.POINTER(t) for t in (i, i32, i64, u32, u64, f32, vp))
    return {
        "flate_hip_init": (i, [i, vpp]),
        "flate_hip_destroy": (None, [vp]),
        "flate_hip_set_stream": (i, [vp, vp]),
        "flate_hip_set_option": (i, [vp, s, i64]),
        "flate_hip_strerror": (s, [i]),
        "flate_hip_last_hip_error": (s, [vp]),
        "flate_hip_deflate_bound": (sz, [sz]),
        "flate_hip_deflate_fast_batch": (i, [vp, vp, vp, u32, vp, u64, vp, u32]),
        "flate_hip_lz77_matches": (i, [vp, vp, vp, u32, u32, u32p, u64p, vp, vp, vp]),
        "flate_hip_inflate_batch": (i, [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32]),
        "flate_hip_deflate_fast_spliced": (i, [vp, vp, vp, u32, vp, u64, vp, vp, u32]),
        "flate_hip_inflate_spliced": (i, [vp, vp, u64, vp, u32, vp, vp, vp, vp, vp, u32]),
        "flate_hip_set_profiling": (i, [vp, i]),
        "flate_hip_last_resident_share": (i, [vp, u32p, u32p]),
        "flate_hip_last_timing": (i, [vp, f32p, i]),
        "flate_hip_stage_name": (s, [i]),
        "flate_hip_synth_fill": (i, [i, u64, u64, u32, u64, vp, i]),
        "flate_hip_build_id": (s, []),
        "flate_hip_comm_unique_id": (i, [vp]),
        "flate_hip_comm_init": (i, [vp, vp, i, i, vpp]),
        "flate_hip_comm_wrap": (i, [vp, vp, i, i, vpp]),
        "flate_hip_comm_destroy": (None, [vp]),
        "flate_hip_comm_plan": (i, [vp, u64p, u32p]),
        "flate_hip_comm_set_plan": (i, [vp, u64, u32]),
        "flate_hip_gather_layout": (i, [u32, vp, u64, u32, u64p, vp, u64p]),
        "flate_hip_gather_compressed": (i, [vp, vp, u64, vp, u32, vp, u64, vp, vp, u64, u64p, u32]),
        "flate_hip_gather_begin": (i, [vp, vp, u64, vp, u32, vp, u64]),
        "flate_hip_gather_end": (i, [vp, vp, vp, u64, u64p]),
        "flate_hip_stream_open": (i, [vp, u32, vpp]),
        "flate_hip_stream_bound": (sz, [sz]),
        "flate_hip_stream_write": (i, [vp, vp, u64, i, vp, u64, u64p]),
        "flate_hip_stream_free": (None, [vp]),
        "flate_hip_host_register": (i, [vp, vp, sz]),
        "flate_hip_host_unregister": (i, [vp, vp]),
        "flate_hip_host_alloc": (i, [vp, sz, vpp]),
        "flate_hip_host_free": (i, [vp, vp]),
        "flate_hip_inflate_stream_open": (i, [vp, vpp]),
        "flate_hip_inflate_stream_read": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, i64p]),
        "flate_hip_inflate_stream_free": (None, [vp]),
        "flate_hip_inflate_stream_reset": (i, [vp, vp, u64]),
        "flate_hip_checksum_batch": (i, [vp, vp, vp, u32, u32, vp, u32]),
        "flate_hip_inflate_batch_dict": (i, [vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, u32]),
        "flate_hip_deflate_fast_batch_dict": (i, [vp, vp, vp, u32, vp, vp, u32, vp, vp, u64, vp, u32]),
        "flate_hip_frame_overhead": (sz, [u32, i]),
        "flate_hip_deflate_fast_batch_framed": (i, [vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, u64, vp, u32]),
        "flate_hip_deflate_fast_spliced_framed": (i, [vp, vp, vp, u32, u32, vp, u64, vp, vp, u32]),
        "flate_hip_inflate_batch_framed": (i, [vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, u32]),
        "flate_hip_inflate_spliced_framed": (i, [vp, vp, u64, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32]),
        "flate_hip_bgzf_bound": (sz, [u64, u32]),
        "flate_hip_bgzf_write": (i, [vp, vp, u64, u32, vp, u64, u64p, vp, u32]),
        "flate_hip_bgzf_index": (i, [vp, vp, u64, u64, vp, vp, u32p, u64p, ip, i64p, u32]),
        "flate_hip_bgzf_read": (i, [vp, vp, u64, vp, u64, u64p, u32p, u32p, i64p, ip, u32]),
        "flate_hip_bgzf_read_ranges": (i, [vp, vp, u64, u32, vp, vp, u32, vp, u64, vp, vp, u32p, u32p, u32p, i64p, u32]),
        "flate_hip_gzip_index": (i, [vp, vp, u64, u64, vp, vp, u32p, u64p, u32p, i64p, u32]),
        "flate_hip_gzip_read": (i, [vp, vp, u64, vp, u64, u64p, u32p, u32p, i64p, u32]),
        "flate_hip_inflate_one_index": (i, [vp, vp, u64, u32, u64, vp, vp, u32p, u64p, u32p, i32p, i64p, u32]),
        "flate_hip_inflate_one": (i, [vp, vp, u64, u32, vp, u64, u64p, i32p, i64p, u32p, u32p, u32]),
        "flate_hip_inflate_one_seek_index": (i, [vp, vp, u64, u32, u64, vp, u64, u64p, vp, u64, u64p, u32p, u32p, u64p,
                                                 u32p, i32p, i64p, u32]),
        "flate_hip_inflate_one_ranges": (i, [vp, vp, u64, u32, vp, u64, vp, u64, vp, vp, u32, vp, u64, vp, vp, u32p, u32p,
                                             u32]),
        "flate_hip_seek_windows_pack_bound": (sz, [u64]),
        "flate_hip_seek_windows_pack": (i, [vp, vp, u64, u32, vp, u64, vp, u64, u32, vp, u64, u64p, vp, u64, u64p, u64p, u32]),
        "flate_hip_seek_windows_unpack": (i, [vp, vp, u64, vp, u64, vp, u64, u64p, u32p, u32]),
        "flate_hip_inflate_one_ranges_packed": (i, [vp, vp, u64, u32, vp, u64, vp, u64, vp, u64, vp, vp, u32, vp, u64, vp, vp,
                                                    u32p, u32p, u32]),
        "flate_hip_gzfile_index": (i, [vp, vp, u64, u64, vp, vp, u64, vp, vp, u32p, u32p, u64p, u32p, i32p, u32p, i64p, i64p,
                                       u32]),
        "flate_hip_gzfile_read": (i, [vp, vp, u64, vp, u64, u64p, u32p, u32p, u32p, i32p, u32p, i64p, i64p, u32]),
        "flate_hip_gzfile_seek_index": (i, [vp, vp, u64, u64, vp, u64, u64p, vp, u64, u64p, u32p, u32p, u32p, u64p, u32p,
                                            i32p, u32p, i64p, i64p, u32]),
        "flate_hip_gzfile_ranges": (i, [vp, vp, u64, vp, u64, vp, u64, vp, vp, u32, vp, u64, vp, vp, u32p, u32p, u32]),
        "flate_hip_zip_bound": (sz, [vp, u32, vp]),
        "flate_hip_zip_write": (i, [vp, vp, vp, u32, vp, vp, vp, u64, u64p, vp, u32]),
        "flate_hip_zip_index": (i, [vp, vp, u64, u64, vp, vp, u32p, u64p, i64p, u32]),
        "flate_hip_zip_read": (i, [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp, vp, vp, u32p, i64p, u32]),
        "flate_hip_zip_last_route": (i, [vp, u32p, u32p, u32p, u32p]),
        "flate_hip_gzfile_last_route": (i, [vp, u32p, u32p, u64p]),
        "flate_hip_deflate_fast_grouped_framed": (i, [vp, vp, vp, u32, vp, u32, u32, vp, u64, vp, vp, u32]),
        "flate_hip_zip_write_last_route": (i, [vp, u32p, u32p]),
        "flate_hip_one_reader_open": (i, [vp, u32, u32, vpp]),
        "flate_hip_one_reader_read": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, i64p, u32p]),
        "flate_hip_one_reader_reset": (i, [vp]),
        "flate_hip_one_reader_free": (None, [vp]),
        "flate_hip_gzfile_reader_open": (i, [vp, u32, vpp]),
        "flate_hip_gzfile_reader_read": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, u32p, u32p, u32p, i64p, i64p]),
        "flate_hip_gzfile_reader_reset": (i, [vp]),
        "flate_hip_gzfile_reader_free": (None, [vp]),
        "flate_hip_gzfile_reader_set_serial_max": (i, [vp, u64]),
        "flate_hip_gzfile_reader_last_route": (i, [vp, u32p, u32p, u64p]),
        "flate_hip_one_writer_bound": (sz, [sz, sz]),
        "flate_hip_one_writer_open": (i, [vp, u32, u64, u32, vpp]),
        "flate_hip_one_writer_write": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, vp, u32p]),
        "flate_hip_one_writer_reset": (i, [vp]),
        "flate_hip_one_writer_free": (None, [vp]),
        "flate_hip_bgzf_reader_open": (i, [vp, u32, vpp]),
        "flate_hip_bgzf_reader_read": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, u64, vp, vp, u32p, u32p, i64p, ip]),
        "flate_hip_bgzf_reader_reset": (i, [vp]),
        "flate_hip_bgzf_reader_free": (None, [vp]),
        "flate_hip_bgzf_writer_bound": (sz, [u64, u32]),
        "flate_hip_bgzf_writer_open": (i, [vp, u32, u32, vpp]),
        "flate_hip_bgzf_writer_write": (i, [vp, vp, u64, i, vp, u64, u64p, u64p, vp, u32p]),
        "flate_hip_bgzf_writer_reset": (i, [vp]),
        "flate_hip_bgzf_writer_free": (None, [vp]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

# What a developer's FLATE_HIP_LIB build of an older tree may lack; the product library may not.  (A call of one that is
# missing fails with ctypes' AttributeError for the symbol.)
MAY_BE_MISSING = [
    "flate_hip_checksum_batch", "flate_hip_frame_overhead", "flate_hip_deflate_fast_batch_framed",
    "flate_hip_deflate_fast_spliced_framed", "flate_hip_inflate_batch_framed", "flate_hip_inflate_spliced_framed",
    "flate_hip_bgzf_bound", "flate_hip_bgzf_write", "flate_hip_bgzf_index", "flate_hip_bgzf_read",
    "flate_hip_bgzf_read_ranges", "flate_hip_gzip_index", "flate_hip_gzip_read", "flate_hip_inflate_one_index",
    "flate_hip_inflate_one", "flate_hip_inflate_one_seek_index", "flate_hip_inflate_one_ranges",
    "flate_hip_gzfile_index", "flate_hip_gzfile_read", "flate_hip_gzfile_seek_index", "flate_hip_gzfile_ranges",
    "flate_hip_zip_bound", "flate_hip_zip_write", "flate_hip_zip_index", "flate_hip_zip_read",
    "flate_hip_zip_last_route", "flate_hip_gzfile_last_route", "flate_hip_deflate_fast_grouped_framed",
    "flate_hip_zip_write_last_route", "flate_hip_one_reader_open", "flate_hip_one_reader_read",
    "flate_hip_one_reader_reset", "flate_hip_one_reader_free", "flate_hip_one_writer_bound",
    "flate_hip_one_writer_open", "flate_hip_one_writer_write", "flate_hip_one_writer_reset",
    "flate_hip_one_writer_free", "flate_hip_seek_windows_pack_bound", "flate_hip_seek_windows_pack",
    "flate_hip_seek_windows_unpack", "flate_hip_inflate_one_ranges_packed", "flate_hip_gzfile_reader_open",
    "flate_hip_gzfile_reader_read", "flate_hip_gzfile_reader_reset", "flate_hip_gzfile_reader_free",
    "flate_hip_gzfile_reader_set_serial_max", "flate_hip_gzfile_reader_last_route", "flate_hip_bgzf_reader_open",
    "flate_hip_bgzf_reader_read", "flate_hip_bgzf_reader_reset", "flate_hip_bgzf_reader_free",
    "flate_hip_bgzf_writer_bound", "flate_hip_bgzf_writer_open", "flate_hip_bgzf_writer_write",
    "flate_hip_bgzf_writer_reset", "flate_hip_bgzf_writer_free",
]

_lib = None


class FlateLibraryMissing(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FlateLibraryMissing(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). This package has no CPU fallback." % LIB_PATH)
    try:
        import torch  # noqa: F401  (load torch's HIP runtime first so both share one libamdhip64)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in MAY_BE_MISSING and os.environ.get("FLATE_HIP_LIB") is not None and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L
