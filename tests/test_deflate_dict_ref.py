"""CPU checks of deflate with preset dictionaries as history: the reference helper (tests/deflate_dict_ref.py) that
the GPU tests compare against, and the export and argument checks of flate_hip_deflate_fast_batch_dict (all made
before the context or a device is touched).  The encoding itself is tested on the GPU (test_gpu_deflate_dict.py)."""
import ctypes as C
import importlib
import os
import re
import zlib

import numpy as np
import pytest

from deflate_dict_ref import deflate_dict
from test_gpu_deflate_dict import DICT_LENS, KINDS, PAYLOAD_LENS, _matrix, kind_bytes, words
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
engine = importlib.import_module("moonbit-flate_amd.engine")
MODES = [0, 1]  # oracle.COMPAT_MOONBIT, oracle.COMPAT_GO


def unzip(comp, zdict):
    d = zlib.decompressobj(-15, zdict=zdict[-32768:]) if zdict else zlib.decompressobj(-15)
    out = d.decompress(comp)
    assert d.eof and d.unused_data == b""
    return out


@pytest.mark.parametrize("compat", MODES)
def test_without_a_dictionary_the_helper_is_the_oracle(oracle, compat):
    for k, n in enumerate(PAYLOAD_LENS):
        for kind in (KINDS[k % len(KINDS)], "text"):
            p = words(5 + k, n) if kind == "text" else kind_bytes(kind, n, 40 + k)
            want = oracle.deflate(p, compat=compat)
            assert deflate_dict(p, None, compat) == want, (n, kind)
            assert deflate_dict(p, b"", compat) == want, (n, kind)


@pytest.mark.parametrize("compat", MODES)
def test_zlib_reads_every_case_of_the_gpu_matrix(compat):
    for k, (pl, dl) in enumerate(_matrix()):
        kind = KINDS[k % len(KINDS)]
        d = words(900 + dl % 97, dl) if kind == "text" else kind_bytes(kind, dl, 77)
        p = words(100 + k, pl) if kind == "text" else kind_bytes(kind, pl, 1000 + k)
        comp = deflate_dict(p, d, compat)
        assert unzip(comp, d) == p, (pl, dl, kind)
        assert len(comp) <= flate.deflate_bound(pl), (pl, dl, kind, len(comp))


@pytest.mark.parametrize("compat", MODES)
def test_short_dictionaries_change_nothing_and_long_ones_are_cut(oracle, compat):
    p = words(3, 4096)
    plain = oracle.deflate(p, compat=compat)
    for dl in (0, 1, 16):  # DeflateFast::encode's small-input path (deflate-fast.mbt:136-140)
        assert deflate_dict(p, words(4, dl), compat) == plain, dl
    assert deflate_dict(p, words(4, 17), compat) is not None
    big = words(6, 100000)
    assert deflate_dict(p, big, compat) == deflate_dict(p, big[-32768:], compat)
    assert deflate_dict(p, big, compat) != deflate_dict(p, big[:32768], compat)


def test_the_dictionary_pays_in_go_mode_only(oracle):
    d, p = words(8, 32768), words(9, 4096)
    plain = len(oracle.deflate(p, compat=1))
    assert len(deflate_dict(p, d, 1)) < plain          # matches extend into the dictionary
    # MoonBit rules: `prev` is empty, a candidate in the dictionary is a match of exactly four bytes
    assert unzip(deflate_dict(p, d, 0), d) == p
    assert len(deflate_dict(d[-300:] + p, d, 1)) < len(deflate_dict(d[-300:] + p, d, 0))
    # payloads under 128 bytes never reach the match finder (deflate.mbt:243)
    small = d[:127]
    assert deflate_dict(small, d, 1) == oracle.deflate(small, compat=1)


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_export_is_declared_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    assert re.search(r"\bint flate_hip_deflate_fast_batch_dict\s*\(", hdr)
    assert "flate_hip_deflate_fast_batch_dict" in importlib.import_module("moonbit-flate_amd._lib").EXPORTS
    assert hasattr(lib, "flate_hip_deflate_fast_batch_dict")


def _call(lib, ctx, dicts=b"abcdef" * 10, dict_off=(0, 30, 60), dict_of=(0, 1), n=2, flags=0, in_off=(0, 200, 400),
          out_off=True, out=True):
    in_buf = np.zeros(512, np.uint8)
    ioff = np.array(in_off[:n + 1], np.uint64)
    obuf = np.zeros(4096, np.uint8)
    ooff = np.zeros(n + 1, np.uint64)
    d = np.frombuffer(dicts, np.uint8).copy() if dicts is not None else None
    doff = np.array(dict_off, np.uint64) if dict_off is not None else None
    dof = np.array(dict_of, np.uint32) if dict_of is not None else None
    n_dicts = len(dict_off) - 1 if dict_off is not None else 0
    return lib.flate_hip_deflate_fast_batch_dict(
        ctx, in_buf.ctypes.data, ioff.ctypes.data, n, d.ctypes.data if d is not None else None,
        doff.ctypes.data if doff is not None else None, n_dicts, dof.ctypes.data if dof is not None else None,
        obuf.ctypes.data if out else None, 4096, ooff.ctypes.data if out_off else None, flags)


def test_argument_checks_without_a_device(lib):
    assert _call(lib, None) == -1  # a null context
    # a context that is never touched: every one of these is refused before the library looks at it
    fake = C.create_string_buffer(4096)
    ctx = C.addressof(fake)
    assert _call(lib, ctx, out_off=False) == -1
    assert _call(lib, ctx, out=False) == -1
    assert _call(lib, ctx, dict_off=(0, 40, 30)) == -1                # dict_off not monotone
    assert _call(lib, ctx, dict_of=(0, 2)) == -1                      # dict_of beyond n_dicts
    assert _call(lib, ctx, dict_of=(7, flate.NO_DICT)) == -1
    assert _call(lib, ctx, dict_off=(0,), dict_of=None) == -1         # dict_of == NULL, no dictionaries
    assert _call(lib, ctx, dict_off=None) == -1                       # n_dicts == 0 but dict_of names some
    assert _call(lib, ctx, dicts=None) == -1                          # non-empty dictionaries without bytes
    assert _call(lib, ctx, flags=0x4) == -1                           # FLATE_HIP_LZ_SERIAL with a real dictionary
    assert _call(lib, ctx, in_off=(0, 300, 200)) == -1                # in_off not monotone (a dictionary in use)


def test_zlib_dict_header():
    d = words(12, 5000)
    h = engine.zlib_dict_header(d)
    assert len(h) == 6 and h[0] == engine.ZLIB_HEADER[0] and (h[1] & 0x20) and ((h[0] << 8) | h[1]) % 31 == 0
    assert (h[1] & 0xC0) == (engine.ZLIB_HEADER[1] & 0xC0)
    assert int.from_bytes(h[2:], "big") == zlib.adler32(d)
    # CPython's zlib accepts the header and asks for exactly this dictionary
    body = deflate_dict(b"payload " * 40, d, 1)
    member = h + body + zlib.adler32(b"payload " * 40).to_bytes(4, "big")
    o = zlib.decompressobj(zdict=d)
    assert o.decompress(member) == b"payload " * 40 and o.eof
    ids = engine.zlib_dict_ids([d])
    assert engine.zlib_member_header(member, ids) == (6, 4, 0)
