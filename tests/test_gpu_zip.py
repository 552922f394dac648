"""ZIP archives on the GPU: flate_hip_zip_write, flate_hip_zip_index and flate_hip_zip_read.  Every expectation comes
from the CPU: tests/zip_ref.py (the writer around the raw call's own streams, the serial reader, the corpora) and
Python's zipfile as an independent reader and writer."""
import ctypes as C
import io
import zipfile
import zlib

import numpy as np
import pytest

import zip_ref as ref
from util import flate, force_inflate_config

pytestmark = pytest.mark.gpu

DEVICE_PTRS, COMPAT_GO = 1, 2
GUARD = 0xA5
ENTRY = np.dtype(ref.ENTRY_DTYPE, align=True)  # (64 bytes, as the C struct)
assert ENTRY.itemsize == 64


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["wave_per_stream", "lane_per_stream", "speculative_wave_small_batch"])
def decoder_eng(request):
    e = force_inflate_config(flate.FlateEngine(0), request.param)
    yield e
    e.close()


def on_device(b, shift=0, pad=64):
    """bytes -> (keep-alive tensor, device pointer of the first byte) at the given byte alignment."""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\0" * shift + bytes(b) + b"\0" * pad, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


# ---- write ----

def write_entries():
    """(names, datas): 0 .. 70 000 bytes of text, random and zero bytes under names of 1, 2, 255 and 300 bytes, so
    that members start at every alignment (computed once per call site, never changed)."""
    names, datas = [], []
    for k, (n, fill) in enumerate((n, f) for n in (0, 1, 17, 127, 128, 4096, 65535, 65536, 70000) for f in ("text", "rand", "zero")):
        datas.append({"text": ref._text, "rand": ref._rand}.get(fill, lambda n, s: bytes(n))(n, k))
        names.append([chr(ord("a") + k // 4), chr(0xe0 + k // 4), "%03d" % k + "x" * 252, "%02d" % k + "☃" * 99 + "y"][k % 4])
    assert sorted({len(n.encode()) for n in names}) == [1, 2, 255, 300]
    return names, datas


def pack(datas):
    off = np.zeros(len(datas) + 1, np.uint64)
    np.cumsum([len(d) for d in datas], out=off[1:])
    return np.frombuffer(b"".join(datas) or b"\0", np.uint8).copy(), off


def zwrite(eng, names, datas, compat=0, device=False, cap=None, out_shift=0, want_off=True):
    """One flate_hip_zip_write call through ctypes -> (rc, archive bytes, entry_off); the guard bytes around the
    capacity must have stayed what they were."""
    src, in_off = pack(datas)
    name_bytes, name_off = flate.engine._zip_names(names)
    n = len(datas)
    if cap is None:
        cap = eng._L.flate_hip_zip_bound(in_off.ctypes.data, n, name_off.ctypes.data)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    eoff = np.full(n + 1, 7, np.uint64)
    out_len = C.c_uint64(0)
    flags = (COMPAT_GO if compat else 0) | (DEVICE_PTRS if device else 0)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(src).cuda(), torch.from_numpy(obuf).cuda()
        in_ptr, out_ptr = d_in.data_ptr(), d_out.data_ptr() + out_shift
    else:
        in_ptr, out_ptr = src.ctypes.data, obuf.ctypes.data + out_shift
    rc = eng._L.flate_hip_zip_write(eng._ctx, in_ptr, in_off.ctypes.data, n, name_bytes.ctypes.data, name_off.ctypes.data,
                                    out_ptr, cap, C.byref(out_len), eoff.ctypes.data if want_off else None, flags)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, obuf[out_shift:out_shift + int(out_len.value)].tobytes(), eoff


def expected_archive(eng, names, datas, compat):
    """zip_ref's archive around the raw call's own streams."""
    src, in_off = pack(datas)
    out, out_off = eng.deflate_batch(src, in_off, compat_go=bool(compat))
    raws = [out[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(len(datas))]
    return ref.write_archive(raws, [n.encode() for n in names], [zlib.crc32(d) for d in datas], [len(d) for d in datas])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("compat", [0, 1])
def test_write_equals_the_reference_and_zipfile_reads_it(eng, compat, device):
    names, datas = write_entries()
    want, want_off = expected_archive(eng, names, datas, compat)
    assert want[want_off[0] + 30 + len(names[0].encode()):want_off[1]] == b"\x01\x00\x00\xff\xff"  # the empty entry
    rc, got, eoff = zwrite(eng, names, datas, compat, device, out_shift=3 if device else 0)
    assert rc == 0 and got == want and eoff.tolist() == want_off
    z = zipfile.ZipFile(io.BytesIO(got))
    assert z.namelist() == names and z.testzip() is None
    assert [z.read(n) for n in names] == datas
    # the exact total is enough to the byte; one byte less is refused by the scan
    rc, got, _ = zwrite(eng, names, datas, compat, device, cap=len(want), want_off=False)
    assert rc == 0 and got == want
    rc, _, _ = zwrite(eng, names, datas, compat, device, cap=len(want) - 1)
    assert rc == ref.OUT_TOO_SMALL


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_write_no_entries_and_one_entry(eng, device):
    rc, got, eoff = zwrite(eng, [], [], device=device, cap=22)
    assert rc == 0 and got == ref.write_archive([], [], [], [])[0] and eoff.tolist() == [0]
    assert zipfile.ZipFile(io.BytesIO(got)).namelist() == []
    assert zwrite(eng, [], [], device=device, cap=21)[0] == ref.OUT_TOO_SMALL
    rc, got, _ = zwrite(eng, ["only"], [b"one entry " * 30], device=device)
    assert rc == 0 and got == expected_archive(eng, ["only"], [b"one entry " * 30], 0)[0]


def test_write_refusals(eng):
    assert zwrite(eng, [""], [b"x"], cap=200)[0] == -1
    assert zwrite(eng, ["n" * 65536], [b"x"], cap=200000)[0] == -1
    src, in_off = pack([b"x"])
    nb, no = flate.engine._zip_names(["a"])
    out, ol = np.zeros(200, np.uint8), C.c_uint64(0)
    call = lambda flags: eng._L.flate_hip_zip_write(eng._ctx, src.ctypes.data, in_off.ctypes.data, 1, nb.ctypes.data, no.ctypes.data,
                                                    out.ctypes.data, 200, C.byref(ol), None, flags)
    assert call(8) == -1 and call(4) == -1 and call(0) == 0
    assert eng._L.flate_hip_strerror(-10).startswith(b"ZIP")


@pytest.mark.parametrize("n", [65534, 65535, 65536, 70000])
def test_write_many_tiny_entries(eng, n):
    names = ["e%d" % i for i in range(n)]
    datas = [b"abc"[:i % 4] for i in range(n)]
    rc, got, eoff = zwrite(eng, names, datas, device=True)
    assert rc == 0
    ix = ref.Index(got)
    assert (ix.rc, ix.n_entries, ix.end.zip64) == (0, n, 1 if n >= 65535 else 0)
    assert (b"PK\6\6" in got[-120:]) == (n >= 65535)
    z = zipfile.ZipFile(io.BytesIO(got))
    assert len(z.namelist()) == n
    for i in (0, 1, 2, 3, n // 2, n - 2, n - 1):
        assert z.read(names[i]) == datas[i]
    want, want_off = expected_archive(eng, names, datas, 0)
    assert got == want and eoff.tolist() == want_off


# ---- index ----

def zindex(eng, f, device=False, shift=0, cap=None):
    """flate_hip_zip_index through ctypes: the count query, then the arrays -> (rc, n, out_bytes, err_off, entries,
    out_off)."""
    keep, ptr = on_device(f, shift) if device else (np.frombuffer(bytes(f) or b"\0", np.uint8).copy(), None)
    if not device:
        ptr = keep.ctypes.data
    flags = DEVICE_PTRS if device else 0
    ne, ob, eo = C.c_uint32(9), C.c_uint64(9), C.c_int64(9)
    rc = eng._L.flate_hip_zip_index(eng._ctx, ptr, len(f), 0, None, None, C.byref(ne), C.byref(ob), C.byref(eo), flags)
    if rc != 0:
        return rc, ne.value, ob.value, eo.value, None, None
    n = ne.value if cap is None else cap
    ent, ooff = np.zeros(n + 1, ENTRY), np.full(n + 2, 7, np.uint64)
    rc = eng._L.flate_hip_zip_index(eng._ctx, ptr, len(f), n, ent.ctypes.data, ooff.ctypes.data, C.byref(ne), C.byref(ob),
                                    C.byref(eo), flags)
    assert ooff[n + 1] == 7 and ent[n]["size"] == 0
    return rc, ne.value, ob.value, eo.value, ent[:n], ooff[:n + 1]


def entries_of(ent):
    return [ref.Entry(*(int(e[k]) for k in ref.Entry._fields)) for e in ent]


def check_index(eng, what, f, device=False, shift=0):
    ix = ref.Index(f)
    rc, n, ob, eo, ent, ooff = zindex(eng, f, device, shift)
    assert (rc, n, eo) == (ix.rc, ix.n_entries, ix.err_off), what
    if ix.rc == 0:
        assert ob == ix.out_bytes and ooff.tolist() == ix.out_off and entries_of(ent) == ix.entries, what
    return ix


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_index_equals_the_reference(eng, device):
    for k, (what, f) in enumerate(ref.zipfile_corpus()):
        check_index(eng, what, f, device, shift=k % 16)  # (the 70 000-entry archives: several tiles, 17 doubling rounds)


def test_index_of_hostile_archives(eng):
    for k, (what, f) in enumerate(ref.hostile_corpus()):
        if what.startswith("truncated") and k % 7 and len(f) > 40:  # (every 7th truncation, and every short one)
            continue
        check_index(eng, what, f, device=True, shift=(3 * k) % 16)


def test_index_too_small_and_at_every_alignment(eng):
    f = dict(ref.zipfile_corpus(big=False))["mixed"]
    ix = ref.Index(f)
    rc, n, ob, _, _, _ = zindex(eng, f, cap=ix.n_entries - 1)
    assert (rc, n, ob) == (ref.OUT_TOO_SMALL, ix.n_entries, ix.out_bytes)
    for shift in range(16):
        check_index(eng, "shift %d" % shift, f, device=True, shift=shift)


def test_index_of_a_directory_full_of_decoys(eng):
    # names that are themselves well-formed central records: more candidates than entries, none on the chain
    decoy = ref.central_record(b"d", 0, 0, 0, 0)
    datas = [b"payload %d" % i for i in range(40)]
    raws = []
    for d in datas:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raws.append(c.compress(d) + c.flush())
    f, _ = ref.write_archive(raws, [decoy + b"%d" % i for i in range(40)], [zlib.crc32(d) for d in datas], [len(d) for d in datas])
    ix = check_index(eng, "decoys", f, device=True, shift=5)
    assert (ix.rc, ix.n_entries) == (0, 40) and f.count(b"PK\1\2") >= 80


# ---- read ----

def zread(eng, f, sel=None, device=False, shift=0, out_shift=0, cap=None, n_cap=None, query=False):
    """flate_hip_zip_read through ctypes -> (rc, out image, out_off, out_len, status, err_off, n_entries,
    archive_err_off).  The output is prefilled with the guard pattern; with device pointers nothing outside
    out[0, out_off[n_sel]) may have changed."""
    ix = ref.Index(f)
    ns = len(sel) if sel is not None else ix.n_entries
    if n_cap is None:
        n_cap = ns
    if cap is None:
        cap = 0 if query else sum(ix.entries[j].size for j in (sel if sel is not None else range(ns))
                                  if j < ix.n_entries and ix.entries[j].status == 0) if ix.rc == 0 else 64
    obuf = np.full(out_shift + cap + 256, GUARD, np.uint8)
    ooff = np.full(n_cap + 2, 7, np.uint64)
    olen, st, eo = np.full(n_cap + 1, 7, np.uint64), np.full(n_cap + 1, 7, np.int32), np.full(n_cap + 1, 7, np.int64)
    selv = np.asarray(sel, np.uint32) if sel is not None else None
    ne, aeo = C.c_uint32(9), C.c_int64(9)
    if device:
        import torch
        keep, in_ptr = on_device(f, shift)
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        keep = np.frombuffer(bytes(f) or b"\0", np.uint8).copy()
        in_ptr, out_ptr = keep.ctypes.data, obuf.ctypes.data + out_shift
    rc = eng._L.flate_hip_zip_read(eng._ctx, in_ptr, len(f), selv.ctypes.data if sel is not None else None,
                                   ns if sel is not None else 0, n_cap, None if query else out_ptr, cap, ooff.ctypes.data,
                                   olen.ctypes.data, st.ctypes.data, eo.ctypes.data, C.byref(ne), C.byref(aeo),
                                   DEVICE_PTRS if device else 0)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert ooff[n_cap + 1] == 7 and olen[n_cap] == 7 and st[n_cap] == 7 and eo[n_cap] == 7
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, obuf[out_shift:], ooff, olen, st, eo, ne.value, aeo.value


def check_read(eng, what, f, sel=None, device=False, shift=0, out_shift=0):
    """One read against zip_ref.read_entry for every selected entry: status, err_off where the rule states it,
    length, bytes; failing and empty entries leave their slot (and everything else) as it was."""
    ix = ref.Index(f)
    assert ix.rc == 0, what
    chosen = list(sel) if sel is not None else list(range(ix.n_entries))
    rc, out, ooff, olen, st, eo, ne, aeo = zread(eng, f, sel, device, shift, out_shift)
    assert (ne, aeo) == (ix.n_entries, -1), what
    at, first = 0, 0
    for j, k in enumerate(chosen):
        e = ix.entries[k]
        want_st, want_eo, want = ref.read_entry(f, e)
        assert int(ooff[j]) == at and int(st[j]) == want_st, (what, j, k, int(st[j]), want_st)
        if want_eo is not None:
            assert int(eo[j]) == want_eo, (what, j, int(eo[j]), want_eo)
        slot = e.size if e.status == 0 else 0
        if want_st == 0:
            assert int(olen[j]) == len(want) and out[at:at + slot].tobytes() == want, (what, j)
        elif e.status != 0:
            assert int(olen[j]) == 0
        first = first or want_st
        at += slot
    assert int(ooff[len(chosen)]) == at and rc == first, (what, rc, first)
    assert (out[at:] == GUARD).all(), what
    return out, ooff, st


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_read_equals_zipfile(decoder_eng, device):
    for k, (what, f) in enumerate(ref.zipfile_corpus(big=False)):
        out, ooff, st = check_read(decoder_eng, what, f, device=device, shift=k % 16, out_shift=(5 * k + 3) % 16 if device else 0)
        z = zipfile.ZipFile(io.BytesIO(f))
        for j, zi in enumerate(z.infolist()):
            assert out[int(ooff[j]):int(ooff[j + 1])].tobytes() == z.read(zi), (what, j)
        assert (st[:len(z.infolist())] == 0).all()


def test_read_70000_entries(eng):
    f = ref.many(70000)
    out, ooff, st = check_read(eng, "70000 entries", f, device=True, shift=9)
    assert (st[:70000] == 0).all() and int(ooff[70000]) == sum(i % 4 for i in range(70000))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_our_own_archives_round_trip(decoder_eng, device):
    names, datas = write_entries()
    for compat in (0, 1):
        rc, f, _ = zwrite(decoder_eng, names, datas, compat, device)
        assert rc == 0
        out, ooff, st = check_read(decoder_eng, "own", f, device=device, shift=7)
        assert [out[int(ooff[j]):int(ooff[j + 1])].tobytes() for j in range(len(datas))] == datas


def test_read_selections_and_the_size_query(eng):
    f = dict(ref.zipfile_corpus(big=False))["mixed"]
    ix = ref.Index(f)
    n = ix.n_entries
    for sel in ([1, 4, 6], list(range(n))[::-1], [2, 2, 0, 7, 2], [], [5]):
        check_read(eng, "sel %r" % sel, f, sel=sel, device=True, shift=3, out_shift=1)
        check_read(eng, "sel %r" % sel, f, sel=sel)
    # the size query: out_off fully written, nothing decoded
    rc, _, ooff, _, _, _, ne, _ = zread(eng, f, query=True)
    assert (rc, ne, ooff[:n + 1].tolist()) == (ref.OUT_TOO_SMALL, n, ix.out_off)
    rc, out, ooff, _, _, _, _, _ = zread(eng, f, sel=[6, 1], device=True, cap=ix.entries[6].size + ix.entries[1].size - 1)
    assert rc == ref.OUT_TOO_SMALL and int(ooff[2]) == ix.entries[6].size + ix.entries[1].size and (out == GUARD).all()
    # refusals before decoding
    assert zread(eng, f, sel=[0, n], device=True)[0] == -1
    assert zread(eng, f, sel=[0, 1], n_cap=1, cap=1 << 17)[0] == -1
    assert zread(eng, f, n_cap=n - 1, cap=1 << 20)[0] == ref.OUT_TOO_SMALL
    assert zread(eng, dict(ref.zipfile_corpus(big=False))["empty archive"], device=True)[0] == 0


def test_read_damaged_entries(decoder_eng):
    for k, (what, f, bad, status, err_off) in enumerate(ref.entry_cases()):
        for device in (False, True):
            out, ooff, st = check_read(decoder_eng, what, f, device=device, shift=k, out_shift=k + 1 if device else 0)
            assert [int(s) for s in st[:3]] == [status if i == bad else 0 for i in range(3)], what
        check_read(decoder_eng, what, f, sel=[2, bad, 1, bad], device=True)


def test_read_of_a_malformed_archive_writes_nothing(eng):
    for k, (what, f) in enumerate(ref.hostile_corpus()):
        ix = ref.Index(f)
        if ix.rc == 0 or (what.startswith("truncated") and k % 11):
            continue
        rc, out, ooff, _, _, _, ne, aeo = zread(eng, f, device=True, shift=k % 16, cap=64, n_cap=4)
        assert (rc, ne, aeo) == (ix.rc, ix.n_entries, ix.err_off), what
        assert (out == GUARD).all() and int(ooff[0]) == 0, what


def test_slots_with_guard_entries(decoder_eng):
    """Nothing outside out[0, out_off[n_sel]) changes, and inside it nothing outside the entries that deliver: guard
    entries (empty, stored, failing) stand between and around the real ones, the buffer is prefilled, and every
    selected entry's slot is compared byte for byte with what it must hold -- the guard pattern for failing ones."""
    real = [("t%d" % i, ref._text(n, i)) for i, n in enumerate((1, 15, 16, 17, 255, 257, 4097, 70001))]
    items = [("g0", b"")]
    for k, it in enumerate(real):
        items += [it, ("g%d" % (k + 1), b"" if k % 2 else b"guard")]
    f = ref._zf(items, zipfile.ZIP_DEFLATED, 6, mixed=False)
    ix = ref.Index(f)
    # damage every second guard entry: an index status, an empty slot
    for e in ix.entries[2::4]:
        f = ref._patch(f, e.header_off, "<B", 0x51)
    for out_shift in (0, 1, 15):
        out, ooff, st = check_read(decoder_eng, "slots", f, device=True, shift=out_shift, out_shift=out_shift)
        assert sorted(set(int(s) for s in st[:len(items)])) == [ref.CORRUPT, 0]


# ---- the layer above ----

def test_engine_methods(eng):
    import torch
    names, datas = write_entries()
    src, in_off = pack(datas)
    f = eng.zip_write(src, in_off, names)
    d_out, d_len, eoff = eng.zip_write(torch.from_numpy(src).cuda(), in_off, names, index=True)
    assert d_out[:d_len].cpu().numpy().tobytes() == f and int(eoff[-1]) == ref.Index(f).end.cd_off
    assert flate.zip_bound(in_off, names) >= len(f)
    for arc in (f, torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()):
        ix = eng.zip_index(arc)
        assert ix.rc == 0 and ix.names == names and ix.entries["size"].tolist() == [len(d) for d in datas]
        out, r = eng.zip_read(arc)
        host = out.cpu().numpy() if hasattr(out, "cpu") else out
        assert r.rc == 0 and [host[int(r.out_off[j]):int(r.out_off[j + 1])].tobytes() for j in range(len(datas))] == datas
        out, r = eng.zip_read(arc, select=[names[5], 3, names[26].encode()])
        host = out.cpu().numpy() if hasattr(out, "cpu") else out
        assert r.rc == 0 and [host[int(r.out_off[j]):int(r.out_off[j + 1])].tobytes() for j in range(3)] == [datas[5], datas[3], datas[26]]
    bad = eng.zip_index(f[:-1])
    assert (bad.rc, bad.err_off, bad.entries) == (ref.CORRUPT, len(f) - 1, None)
    assert eng.zip_read(f[:-1])[1].rc == ref.CORRUPT
    with pytest.raises(KeyError):
        eng.zip_read(f, select=["no such entry"])
