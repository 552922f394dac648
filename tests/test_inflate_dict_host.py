"""CPU-side checks of batch inflate with preset dictionaries (flate_hip_inflate_batch_dict): the export, its
argument checks (all made before the context or a device is touched), and the zlib FDICT header parsing of
inflate_batch_framed.  The decoding itself is tested on the GPU (test_gpu_inflate_dict.py)."""
import ctypes as C
import importlib
import os
import re
import zlib

import numpy as np
import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
engine = importlib.import_module("moonbit-flate_amd.engine")


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_export_is_declared_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    assert re.search(r"\bint flate_hip_inflate_batch_dict\s*\(", hdr)
    assert re.search(r"#define FLATE_HIP_NO_DICT 0xffffffffu", hdr)
    assert "flate_hip_inflate_batch_dict" in importlib.import_module("moonbit-flate_amd._lib").EXPORTS
    assert hasattr(lib, "flate_hip_inflate_batch_dict")
    assert flate.NO_DICT == 0xFFFFFFFF


def _call(lib, ctx, dicts=b"abcdef", dict_off=(0, 3, 6), dict_of=(0, 1), n=2, flags=0):
    in_buf = np.zeros(64, np.uint8)
    in_off = np.array([0, 8, 16][:n + 1], np.uint64)
    out = np.zeros(64, np.uint8)
    out_off = np.array([0, 16, 32][:n + 1], np.uint64)
    out_len = np.zeros(max(n, 1), np.uint64)
    status = np.zeros(max(n, 1), np.int32)
    err = np.zeros(max(n, 1), np.int64)
    d = np.frombuffer(dicts, np.uint8).copy() if dicts is not None else None
    doff = np.array(dict_off, np.uint64) if dict_off is not None else None
    dof = np.array(dict_of, np.uint32) if dict_of is not None else None
    n_dicts = len(dict_off) - 1 if dict_off is not None else 0
    return lib.flate_hip_inflate_batch_dict(
        ctx, in_buf.ctypes.data, in_off.ctypes.data, n, d.ctypes.data if d is not None else None,
        doff.ctypes.data if doff is not None else None, n_dicts, dof.ctypes.data if dof is not None else None,
        out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, err.ctypes.data, flags)


def test_argument_checks_without_a_device(lib):
    assert _call(lib, None) == -1  # no context
    # a context that is never touched: every one of these tables is refused before the library looks at it
    fake = C.create_string_buffer(4096)
    ctx = C.addressof(fake)
    assert _call(lib, ctx, dict_off=(0, 4, 3)) == -1                  # dict_off not monotone
    assert _call(lib, ctx, dict_of=(0, 2)) == -1                      # dict_of beyond n_dicts
    assert _call(lib, ctx, dict_of=(7, flate.NO_DICT)) == -1
    assert _call(lib, ctx, dict_off=(0,), dict_of=None) == -1         # dict_of == NULL, no dictionaries
    assert _call(lib, ctx, dicts=None) == -1                          # dicts == NULL, non-empty dictionaries


def test_fdict_header_parsing():
    d = b"a preset dictionary " * 10
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, d)
    member = co.compress(b"some data") + co.flush()
    assert member[1] & 0x20
    assert engine.parse_container_header(member, "zlib") == (-1, 0)              # as before: refused
    assert engine.parse_container_header(member, "zlib", fdict=True) == (6, 4)    # DICTID follows
    assert int.from_bytes(member[2:6], "big") == zlib.adler32(d)
    plain = zlib.compress(b"some data")
    assert engine.parse_container_header(plain, "zlib", fdict=True) == (2, 4)
    assert engine.parse_container_header(member[:5], "zlib", fdict=True) == (-1, 0)


def test_dictionary_arguments_packing():
    a, b = b"first", b"second dictionary"
    dk = engine._DictArgs([a, b, b""], [1, engine.NO_DICT, 0, 2], 4, False)
    assert dk.n_dicts == 3 and list(dk.off) == [0, 5, 5 + len(b), 5 + len(b)]
    assert bytes(dk.buf[:5 + len(b)]) == a + b
    assert list(dk.of) == [1, 0xFFFFFFFF, 0, 2]
    one = engine._DictArgs(a, None, 4, False)
    assert one.n_dicts == 1 and one.of_ptr is None and list(one.off) == [0, 5]


def test_dictid_selects_the_dictionary():
    dicts = [b"first dictionary " * 4, b"second dictionary " * 9]
    ids = engine.zlib_dict_ids(dicts)
    members = []
    for d in dicts + [b"a third one"]:
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, d)
        members.append(co.compress(b"payload") + co.flush())
    assert engine.zlib_member_header(members[0], ids) == (6, 4, 0)
    assert engine.zlib_member_header(members[1], ids) == (6, 4, 1)
    assert engine.zlib_member_header(members[2], ids) == (-1, 0, engine.NO_DICT)    # no match: corrupt
    assert engine.zlib_member_header(members[1], None) == (-1, 0, engine.NO_DICT)   # no zdicts: corrupt
    assert engine.zlib_member_header(zlib.compress(b"x"), ids) == (2, 4, engine.NO_DICT)
