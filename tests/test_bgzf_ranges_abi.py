"""CPU-side checks of flate_hip_bgzf_read_ranges: the symbol is there and listed, the call refuses a missing ctx
before it touches a device -- and the Python model itself (tests/bgzf_range_ref.py) delivers what gzip's own reader
slices out of the corpus.  (GPU compute: tests/test_gpu_bgzf_ranges.py; the rule: tests/test_bgzf_range_model.py.)"""
import ctypes as C
import gzip
import importlib

import pytest

import bgzf_range_ref as model
import bgzf_ref as ref
from util import flate

NAME = "flate_hip_bgzf_read_ranges"


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_library_exports_the_call(lib):
    assert hasattr(lib, NAME)


def test_the_call_is_listed_in_exports():
    assert NAME in importlib.import_module("moonbit-flate_amd._lib").EXPORTS


def test_the_call_refuses_a_missing_ctx_before_it_touches_a_device(lib):
    buf = (C.c_uint8 * 64)(*ref.EOF)
    out = (C.c_uint8 * 256)()
    lo, hi, off = (C.c_uint64 * 2)(0, 0), (C.c_uint64 * 2)(0, 0), (C.c_uint64 * 3)()
    st = (C.c_int32 * 2)()
    nm, nd, bad, eo = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int64()
    for flags in (0, 1):
        for kind in (0, 1):
            assert lib.flate_hip_bgzf_read_ranges(None, buf, 28, kind, lo, hi, 2, out, 256, off, st, C.byref(nm),
                                                  C.byref(nd), C.byref(bad), C.byref(eo), flags) == -1


def test_the_model_delivers_what_gzip_slices(lib):
    for what, f in ref.index_corpus():
        w = ref.Walk(f)
        if w.rc or any(what == x[0] for x in ref.failing_files()):
            continue
        U = gzip.decompress(f) if f else b""
        ranges = model.byte_edge_ranges(w)
        R = model.read_ranges(f, model.POS_BYTES, [b for b, _ in ranges], [e for _, e in ranges])
        assert R.rc == 0 and R.n_members == w.n_members, what
        for r, (b, e) in enumerate(ranges):
            assert R.data[R.out_off[r]:R.out_off[r + 1]] == U[b:e], (what, b, e)
        # the virtual kind: the valid ranges deliver the same slices, the invalid ones nothing
        ranges = model.virtual_edge_ranges(f, w)
        R = model.read_ranges(f, model.POS_VIRTUAL, [b for b, _ in ranges], [e for _, e in ranges])
        for r, (b, e) in enumerate(ranges):
            pb, pe = model.virtual_pos(b, w), model.virtual_pos(e, w)
            if pb is None or pe is None:
                assert R.range_status[r] == -1 and R.out_off[r] == R.out_off[r + 1], (what, b, e)
            else:
                assert R.range_status[r] == 0 and R.data[R.out_off[r]:R.out_off[r + 1]] == U[pb:pe], (what, b, e)
        assert R.rc == (-1 if -1 in R.range_status else 0), what


def test_the_model_follows_the_order_of_the_verdict():
    what, f, err_off, n_good = ref.malformed_files()[1]
    R = model.read_ranges(f, model.POS_BYTES, [0, 5], [3, 9], out_cap=0)
    assert (R.rc, R.err_off, R.bad_member, R.out_off, R.range_status) == (-4, err_off, n_good, [0, 0, 0], [-4, -4])
    assert model.read_ranges(f, model.POS_BYTES, [5], [3]).rc == -1       # refused before the chain is looked at
    assert model.read_ranges(f, model.POS_BYTES, [], []).rc == 0          # nothing is read
    good = ref.header_files()[0][1]
    R = model.read_ranges(good, model.POS_BYTES, [0, 5], [3, 9], out_cap=6)
    assert (R.rc, R.out_off, R.data) == (-2, [0, 3, 7], b"")
    what, f, rc, bad = ref.failing_files()[4]  # two failures: the first is reported
    w = ref.Walk(f)
    R = model.read_ranges(f, model.POS_BYTES, [0, w.out_off[2]], [w.out_bytes, w.out_bytes], status={1: rc, 2: -4})
    assert (R.rc, R.bad_member, R.err_off, R.range_status, R.n_decoded) == (rc, 1, w.member_off[1], [rc, -4], 3)
