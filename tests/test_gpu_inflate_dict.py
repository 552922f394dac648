"""GPU parity tests of the batch inflater with preset dictionaries (flate_hip_inflate_batch_dict:
&Reader::new_dict, inflate.mbt:315-317; DictDecoder::new, dict-decoder.mbt:40-60) against the oracle's
orc_inflate_stream_dict, on every decoder and build."""
import functools
import zlib

import numpy as np
import pytest

from util import INFLATE_CONFIGS, flate, force_inflate_config

pytestmark = pytest.mark.gpu

NO_DICT = flate.NO_DICT


@pytest.fixture(scope="module", params=INFLATE_CONFIGS)
def eng(request):
    """Every decoder (util.INFLATE_CONFIGS, as tests/test_gpu_inflate.py forces them) has a dictionary build: all
    must pass."""
    flate.build()
    e = force_inflate_config(flate.FlateEngine(0), request.param)
    yield e
    e.close()


def words(seed, n):
    return flate.synth("text", 1, n, seed=seed).tobytes() if n else b""


def zdeflate(data, zdict, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, zdict) if zdict else \
        zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def _pack(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.array([len(b) for b in blobs], dtype=np.uint64), out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0" * 8, dtype=np.uint8).copy(), off


def _check(oracle, blobs, caps, dicts, dict_of, res):
    """Stream by stream, on every status: status, error offset, out_len and the bytes delivered."""
    out, ooff, olen, status, err = res
    for i, bl in enumerate(blobs):
        j = 0 if dict_of is None else int(dict_of[i])
        d = None if j == NO_DICT else dicts[j]
        rc, want, used, eoff = oracle.inflate(bl, caps[i], full=True, zdict=d)
        want_status = {0: 0, oracle.E_CORRUPT: -4, oracle.E_UNEXPECTED_EOF: -7, oracle.E_OUT_TOO_SMALL: -2}[rc]
        assert int(status[i]) == want_status, (i, int(status[i]), rc)
        assert int(err[i]) == eoff, (i, int(err[i]), eoff)
        assert int(olen[i]) == len(want), (i, rc, int(olen[i]), len(want))
        assert bytes(out[int(ooff[i]):int(ooff[i]) + int(olen[i])]) == want, (i, rc)


# ---- a fixed-Huffman DEFLATE writer for hand-made edge copies (RFC 1951 3.2.5-3.2.6) ----
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
          4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_block(tokens):
    """One final fixed-Huffman block: tokens are ints (literals) or (length, distance) pairs."""
    bits = []

    def put(v, n):  # LSB first
        bits.extend((v >> k) & 1 for k in range(n))

    def code(c, n):  # Huffman codes MSB first
        bits.extend((c >> (n - 1 - k)) & 1 for k in range(n))

    def sym(s):
        if s < 144:
            code(0x30 + s, 8)
        elif s < 256:
            code(0x190 + s - 144, 9)
        elif s < 280:
            code(s - 256, 7)
        else:
            code(0xC0 + s - 280, 8)

    put(1, 1)
    put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            sym(t)
            continue
        ln, dist = t
        li = max(k for k in range(29) if _LBASE[k] <= ln)
        sym(257 + li)
        put(ln - _LBASE[li], _LEXT[li])
        di = max(k for k in range(30) if _DBASE[k] <= dist)
        code(di, 5)
        put(dist - _DBASE[di], _DEXT[di])
    sym(256)
    bits.extend([0] * (-len(bits) % 8))
    return bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


@functools.lru_cache(maxsize=None)
def _variety():
    """Streams from zlib at levels 1 / 6 / 9 with four strategies, and stored blocks, for eight dictionary lengths
    (40000: only its tail is history); data that shares its vocabulary with the dictionary."""
    dlens = [1, 7, 15, 16, 17, 1000, 32768, 40000]
    dicts = [words(100 + k, n) for k, n in enumerate(dlens)]
    blobs, caps, dict_of = [], [], []
    for j, d in enumerate(dicts):
        data = d[-3000:] + words(200 + j, 6000) + d[:2000] + d[-20:] * 3 + d[len(d) // 2:len(d) // 2 + 500]
        runs = [(lv, st) for lv in (1, 6, 9)
                for st in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY)] + [(0, 0)]
        for lv, st in runs:
            blobs.append(zdeflate(data, d, lv, st))
            caps.append(len(data))
            dict_of.append(j)
    return dicts, blobs, caps, dict_of


def test_dictionary_variety_matches_oracle(eng, oracle):
    dicts, blobs, caps, dict_of = _variety()
    data, off = _pack(blobs)
    res = eng.inflate_batch(data, off, caps, check=False, zdicts=dicts, dict_of=dict_of)
    assert (res[3] == 0).all()
    _check(oracle, blobs, caps, dicts, dict_of, res)


def test_one_shared_dictionary(eng, oracle):
    d = words(5, 32768)
    srcs = [d[-k * 997 % 30000:][:4000] + words(300 + k, 3000 + 500 * k) for k in range(24)]
    blobs = [zdeflate(s, d, 1 + k % 9) for k, s in enumerate(srcs)]
    data, off = _pack(blobs)
    caps = [len(s) for s in srcs]
    res = eng.inflate_batch(data, off, caps, check=False, zdicts=d)
    assert (res[3] == 0).all()
    _check(oracle, blobs, caps, [d], None, res)


def test_mixed_dictionary_none_and_empty_in_one_batch(eng, oracle):
    dicts = [words(7, 5000), b"", words(8, 20000)]
    blobs, caps, dict_of = [], [], []
    for k in range(30):
        j = [0, 1, 2, NO_DICT][k % 4]
        d = b"" if j == NO_DICT else dicts[j]
        s = d[-2000:] + words(400 + k, 4000) + d[:500]
        blobs.append(zdeflate(s, d, 6))
        caps.append(len(s))
        dict_of.append(j)
    data, off = _pack(blobs)
    res = eng.inflate_batch(data, off, caps, check=False, zdicts=dicts, dict_of=dict_of)
    assert (res[3] == 0).all()
    _check(oracle, blobs, caps, dicts, dict_of, res)


def test_edge_copies(eng, oracle):
    """Hand-made copies at the dictionary's edges: one that starts in the dictionary and runs into the output, an
    overlapping one (dist < len) whose source is all dictionary, dist == dict_len + produced exactly, dist == 32768
    with a 40000-byte dictionary, and the same one byte too far (corrupt)."""
    d1000, d40000 = words(9, 1000), words(10, 40000)
    lit = list(b"head")
    cases = [
        (d1000, [(40, 20)] + lit),                       # starts in the dictionary, runs into the output
        (d1000, [(100, 7)]),                             # overlapping, source in the dictionary
        (d1000, [(258, 600), (30, 300)]),                # second copy: source 300 back from 258 produced
        (d1000, lit + [(10, 1004)]),                     # dist == dict_len + produced
        (d1000, lit + [(10, 1005)]),                     # one past the history: corrupt
        (d40000, [(258, 32768)] + lit + [(3, 32768)]),   # dist == 32768, dictionary longer than the window
        (d40000, lit * 10 + [(16, 32768), (17, 32767)]),
        (d1000, [(3, 1)] * 5 + [(16, 16), (17, 17), (15, 15), (16, 1000)]),  # 16-byte chunk edges
        (words(11, 16), [(16, 16), (16, 16), (258, 1)]),
    ]
    blobs = [fixed_block(t) for _, t in cases]
    dicts = [d for d, _ in cases]
    caps = [4096] * len(cases)
    data, off = _pack(blobs)
    res = eng.inflate_batch(data, off, caps, check=False, zdicts=dicts, dict_of=list(range(len(cases))))
    assert int(res[3][4]) == -4
    _check(oracle, blobs, caps, dicts, list(range(len(cases))), res)


def test_errors_match_oracle(eng, oracle):
    """A missing, too short or wrong dictionary, truncated input, an output slot that is too small."""
    d = words(12, 20000)
    s = d[-5000:] + words(13, 8000) + d[:3000]
    good = zdeflate(s, d, 6)
    other = words(14, 20000)
    dicts = [d, d[-1000:], other, d[:5000]]
    blobs, caps, dict_of = [], [], []
    for j in (NO_DICT, 1, 2, 3):  # none, too short, wrong, wrong and short
        blobs.append(good)
        caps.append(len(s))
        dict_of.append(j)
    for cut in (1, 10, len(good) // 2, len(good) - 1):  # truncated
        blobs.append(good[:cut])
        caps.append(len(s))
        dict_of.append(0)
    for cap in (1, 100, 4999, 5000, len(s) - 1):  # slot too small
        blobs.append(good)
        caps.append(cap)
        dict_of.append(0)
    data, off = _pack(blobs)
    res = eng.inflate_batch(data, off, caps, check=False, zdicts=dicts, dict_of=dict_of)
    assert int(res[3][0]) == -4 and int(res[3][1]) == -4
    assert int(res[3][5]) == -7
    _check(oracle, blobs, caps, dicts, dict_of, res)


def test_size_only_sizes(eng, oracle):
    dicts, blobs, caps, dict_of = _variety()
    blobs = blobs + [blobs[3][:len(blobs[3]) // 2]]
    dict_of = dict_of + [dict_of[3]]
    data, off = _pack(blobs)
    olen, status, err = eng.inflate_sizes(data, off, zdicts=dicts, dict_of=dict_of)
    for i, bl in enumerate(blobs):
        rc, want, used, eoff = oracle.inflate(bl, 1 << 20, full=True, zdict=dicts[dict_of[i]])
        assert int(status[i]) == {0: 0, oracle.E_CORRUPT: -4, oracle.E_UNEXPECTED_EOF: -7}[rc], i
        assert int(err[i]) == eoff
        assert int(olen[i]) == len(want), (i, rc)  # (up to the error, if any)


def test_device_pointers_with_dictionaries_on_the_device(eng, oracle):
    import torch
    dicts, blobs, caps, dict_of = _variety()
    data, off = _pack(blobs)
    d_data = torch.from_numpy(data).cuda()
    res = eng.inflate_batch(d_data, off, caps, check=False, zdicts=dicts, dict_of=dict_of)
    out = res[0].cpu().numpy()
    _check(oracle, blobs, caps, dicts, dict_of, (out,) + tuple(res[1:]))
    # one dictionary that is itself a device tensor
    d = dicts[6]
    sel = [i for i in range(len(blobs)) if dict_of[i] == 6]
    data, off = _pack([blobs[i] for i in sel])
    res = eng.inflate_batch(torch.from_numpy(data).cuda(), off, [caps[i] for i in sel], check=False,
                            zdicts=torch.from_numpy(np.frombuffer(d, np.uint8).copy()).cuda())
    _check(oracle, [blobs[i] for i in sel], [caps[i] for i in sel], [d], None, (res[0].cpu().numpy(),) + tuple(res[1:]))


def test_no_dictionary_call_is_the_plain_call(eng):
    dicts, blobs, caps, _ = _variety()
    blobs = blobs[:20] + [b"\x03\x00", blobs[5][:50]]
    data, off = _pack(blobs)
    caps = caps[:20] + [10, 10]
    plain = eng.inflate_batch(data, off, caps, check=False)
    for zd, of in ((dicts, [NO_DICT] * len(blobs)), ([b""], None), ([b"", dicts[3]], [0] * len(blobs))):
        got = eng.inflate_batch(data, off, caps, check=False, zdicts=zd, dict_of=of)
        for a, b in zip(plain, got):
            assert np.array_equal(np.asarray(a), np.asarray(b))


def test_zlib_fdict_round_trip(eng):
    dicts = [words(20, 3000), words(21, 32768), words(22, 50000)]
    members, want = [], []
    for k in range(12):
        j = k % 4
        s = words(500 + k, 5000) + (dicts[j][-4000:] if j < 3 else b"")
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, dicts[j]) if j < 3 else zlib.compressobj(6)
        members.append(co.compress(s) + co.flush())
        want.append(s)
    data, off = _pack(members)
    out, ooff, olen, status = eng.inflate_batch_framed(data, off, "zlib", zdicts=dicts)
    assert (status == 0).all(), status
    for i, m in enumerate(members):
        j = i % 4
        dz = zlib.decompressobj(zdict=dicts[j]) if j < 3 else zlib.decompressobj()
        assert bytes(out[int(ooff[i]):int(ooff[i]) + int(olen[i])]) == dz.decompress(m) == want[i]
    # a dictionary that is not there, and no dictionaries at all: FDICT members are corrupt
    _, _, _, st = eng.inflate_batch_framed(data, off, "zlib", zdicts=dicts[:1])
    assert [int(x) for x in st] == [0 if k % 4 in (0, 3) else -4 for k in range(12)]
    _, _, _, st = eng.inflate_batch_framed(data, off, "zlib")
    assert [int(x) for x in st] == [0 if k % 4 == 3 else -4 for k in range(12)]


def test_host_pipeline_with_dictionaries_across_groups(oracle):
    """A host-pointer batch of >= 64 MiB takes the pipelined path; dict_of spans its groups."""
    flate.build()
    e = flate.FlateEngine(0)
    try:
        e.set_option("host_pipeline_groups", 4)
        e.set_option("host_pipeline_group_streams", 64)
        dicts = [words(30 + j, 32768) for j in range(3)]
        n, blen = 1100, 65536
        src = flate.synth("text", n, blen, seed=31)
        blobs, dict_of = [], []
        for i in range(n):
            j = (i * 7) % 4
            s = bytes(src[i * blen:(i + 1) * blen])
            if j < 3:
                s = dicts[j][-9000:] + s[9000:]
            blobs.append(zdeflate(s, dicts[j] if j < 3 else b"", 1))
            dict_of.append(j if j < 3 else NO_DICT)
        data, off = _pack(blobs)
        out, ooff, olen, status, err = e.inflate_batch(data, off, [blen] * n, check=False, zdicts=dicts, dict_of=dict_of)
        assert (status == 0).all() and (olen == blen).all()
        for i in range(0, n, 37):
            d = dicts[dict_of[i]] if dict_of[i] != NO_DICT else None
            assert bytes(out[int(ooff[i]):int(ooff[i + 1])]) == oracle.inflate(blobs[i], blen, zdict=d), i
    finally:
        e.close()


def test_large_batch_on_default_options(oracle):
    """>= 45056 streams on the default options: the 64-lane decoder with its output row."""
    flate.build()
    e = flate.FlateEngine(0)
    try:
        d = words(40, 32768)
        n = 45056
        rng = np.random.default_rng(41)
        starts = rng.integers(0, 32768 - 200, n)
        blobs, caps = [], []
        for i in range(n):
            s = d[int(starts[i]):int(starts[i]) + 150] + bytes([i & 255, 32]) + d[int(starts[i]) // 2:][:60]
            blobs.append(zdeflate(s, d, 1 + i % 9))
            caps.append(len(s))
        data, off = _pack(blobs)
        res = e.inflate_batch(data, off, caps, check=False, zdicts=d)
        assert (res[3] == 0).all()
        sel = list(range(0, n, 97)) + [n - 1]
        _check(oracle, [blobs[i] for i in sel], [caps[i] for i in sel], [d], None, _subset(res, sel))
    finally:
        e.close()


def _subset(res, sel):
    out, ooff, olen, status, err = res
    parts = [np.asarray(out[int(ooff[i]):int(ooff[i + 1])]) for i in sel]
    o = np.zeros(len(sel) + 1, np.uint64)
    np.cumsum([p.size for p in parts], out=o[1:])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8), o, olen[sel], status[sel], err[sel])
