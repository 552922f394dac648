"""GPU parity tests of batch deflate with preset dictionaries as history (flate_hip_deflate_fast_batch_dict): every
output is compared BYTE FOR BYTE with tests/deflate_dict_ref.py (the oracle's DeflateFast run over the dictionary,
tokens dropped, then the unchanged Compressor driver), then decoded with the same dictionary by the GPU inflater
and by zlib on the CPU.  Both compat modes."""
import zlib

import numpy as np
import pytest

from deflate_dict_ref import deflate_dict
from util import flate, make_streams

pytestmark = pytest.mark.gpu

NO_DICT = flate.NO_DICT
PAYLOAD_LENS = [0, 1, 16, 17, 127, 128, 129, 1000, 4096, 65534, 65535, 65536, 65552, 131070, 200000]
DICT_LENS = [0, 1, 16, 17, 18, 300, 4096, 32767, 32768, 32769, 100000]
KINDS = ["text", "ramp", "zero", "rand", "low", "period", "runs"]
MODES = [False, True]  # compat_go


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def words(seed, n):
    return flate.synth("text", 1, n, seed=seed).tobytes() if n else b""


def kind_bytes(kind, n, seed):
    if n == 0:
        return b""
    data, off = make_streams([(kind, n)], seed=seed)
    return data[:n].tobytes()


def _pack(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.array([len(b) for b in blobs], dtype=np.uint64), out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0" * 16, dtype=np.uint8).copy(), off


def zlib_inflate(comp, zdict):
    d = zlib.decompressobj(-15, zdict=zdict[-32768:]) if zdict else zlib.decompressobj(-15)
    out = d.decompress(bytes(comp))
    assert d.eof and d.unused_data == b""
    return out


def run_batch(eng, payloads, dicts, dict_of, compat_go, device=False):
    """Compress the batch, compare every stream with the reference helper, decode it on the GPU and with zlib."""
    data, off = _pack(payloads)
    if device:
        import torch
        out, ooff = eng.deflate_batch(torch.from_numpy(data).cuda(), off, compat_go=compat_go, zdicts=dicts,
                                      dict_of=dict_of)
        out = out.cpu().numpy()
    else:
        out, ooff = eng.deflate_batch(data, off, compat_go=compat_go, zdicts=dicts, dict_of=dict_of)
    comps = []
    for i, p in enumerate(payloads):
        j = 0 if dict_of is None else int(dict_of[i])
        d = b"" if j == NO_DICT else dicts[j]
        got = bytes(out[int(ooff[i]):int(ooff[i + 1])])
        want = deflate_dict(p, d, 1 if compat_go else 0)
        assert got == want, "stream %d (payload %d bytes, dictionary %d bytes, compat_go=%s): %d bytes, reference %d" \
            % (i, len(p), len(d), compat_go, len(got), len(want))
        assert len(got) <= flate.deflate_bound(len(p))
        assert zlib_inflate(got, d) == p, (i, len(p), len(d))
        comps.append(got)
    cdata, coff = _pack(comps)
    back, boff, blen, status, _ = eng.inflate_batch(cdata, coff, [len(p) for p in payloads], zdicts=dicts,
                                                    dict_of=dict_of)
    assert (status == 0).all()
    for i, p in enumerate(payloads):
        assert int(blen[i]) == len(p) and bytes(back[int(boff[i]):int(boff[i]) + len(p)]) == p, i
    return comps


def _matrix():
    """Every length of one axis against three of the other (32768 and 17 among them), kinds rotating."""
    cases = set()
    for pl in PAYLOAD_LENS:
        for dl in (17, 4096, 32768):
            cases.add((pl, dl))
    for dl in DICT_LENS:
        for pl in (128, 4096, 65552):
            cases.add((pl, dl))
    return sorted(cases)


@pytest.mark.parametrize("compat_go", MODES)
def test_length_matrix_matches_the_reference(eng, compat_go):
    cases = _matrix()
    dict_lens = sorted({dl for _, dl in cases})
    # a dictionary per length and kind: the kind's generator with another seed, so that payload and dictionary
    # share their statistics (text: the same vocabulary)
    dicts, index = [], {}
    payloads, dict_of = [], []
    for k, (pl, dl) in enumerate(cases):
        kind = KINDS[k % len(KINDS)]
        if (kind, dl) not in index:
            index[(kind, dl)] = len(dicts)
            dicts.append(words(900 + dl % 97, dl) if kind == "text" else kind_bytes(kind, dl, 77))
        payloads.append(words(100 + k, pl) if kind == "text" else kind_bytes(kind, pl, 1000 + k))
        dict_of.append(index[(kind, dl)])
    assert len(dict_lens) == len(DICT_LENS)
    run_batch(eng, payloads, dicts, dict_of, compat_go)


@pytest.mark.parametrize("compat_go", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_with_a_full_dictionary(eng, kind, compat_go):
    d = words(41, 32768) if kind == "text" else kind_bytes(kind, 32768, 5)
    payloads = [words(42, n) if kind == "text" else kind_bytes(kind, n, 6 + n) for n in (1000, 4096, 65536, 131070)]
    run_batch(eng, payloads, [d], None, compat_go)


@pytest.mark.parametrize("compat_go", MODES)
def test_hard_cases(eng, compat_go):
    rng = np.random.default_rng(9)
    d = words(7, 32768)
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = []  # (payload, dictionary)
    cases.append((d, d))                                             # the payload is the dictionary
    cont = words(8, 5000)
    cases.append(((d + cont)[-5300:], d))                            # starts as the dictionary's last 300 bytes and
    # ... goes on: with the dictionary d + cont[:k] a match begins in the dictionary and crosses into the payload
    full = words(11, 40000)
    cases.append((full[32768 - 300:], full[:32768]))                 # payload = last 300 bytes of dict + continuation
    cases.append((full[32768:32768 + 4000], full[:32768]))           # the continuation alone
    # matches only at distance exactly 32768 (accepted) and 32769 (refused) from the dictionary's far end
    far = noise(64)
    d_far = far + noise(32768 - 64)
    cases.append((far + noise(200), d_far))                          # payload[0:64] = dict[0:64]: distance 32768
    cases.append((noise(1) + far + noise(200), d_far))               # one further on: 32769, out of reach
    cases.append((bytes(5000), bytes(32768)))                        # zeros after zeros: distance-1 runs over the border
    cases.append((bytes(70000), bytes(300)))
    # a second window whose matches reach into the first window but no longer into the dictionary
    w1 = noise(65535)
    cases.append((w1 + w1[40000:60000] + d[:3000], d))
    cases.append((w1[:40000] + d[1000:9000] + w1[40000:65535] + w1[50000:65535] + d[1000:9000], d))
    dicts = []
    dict_of = []
    for p, dd in cases:
        if dd not in dicts:
            dicts.append(dd)
        dict_of.append(dicts.index(dd))
    run_batch(eng, [p for p, _ in cases], dicts, dict_of, compat_go)


@pytest.mark.parametrize("compat_go", MODES)
def test_mixed_dictionaries_in_shuffled_order(eng, compat_go):
    rng = np.random.default_rng(3)
    dicts = [words(21, 32768), words(22, 900), words(23, 50000), b""]
    payloads, dict_of = [], []
    for k in range(60):
        j = [0, 1, 2, NO_DICT, 3][k % 5]
        n = [4096, 300, 65536, 100, 131070, 2000][k % 6]
        payloads.append(words(300 + k, n))
        dict_of.append(j)
    order = rng.permutation(len(payloads))
    run_batch(eng, [payloads[i] for i in order], dicts, [dict_of[i] for i in order], compat_go)


@pytest.mark.parametrize("compat_go", MODES)
def test_large_batch_takes_lds_table_and_guest_blocks(eng, compat_go):
    """More than guest_min (5 x CUs) streams with a dictionary: the persistent launch, LDS-table and guest blocks
    side by side, device pointers; checked against the reference on a sample, decoded in full."""
    import torch
    n = 5 * 256 + 700
    dicts = [words(31, 32768), words(32, 5000)]
    lens = [4096, 1500, 65535 + 3000, 130, 9000]
    payloads = [words(4000 + i, lens[i % len(lens)]) for i in range(n)]
    dict_of = np.array([i % 2 for i in range(n)], dtype=np.uint32)
    data, off = _pack(payloads)
    out, ooff = eng.deflate_batch(torch.from_numpy(data).cuda(), off, compat_go=compat_go, zdicts=dicts, dict_of=dict_of)
    host = out.cpu().numpy()
    for i in list(range(0, n, 37)) + [n - 1]:
        got = bytes(host[int(ooff[i]):int(ooff[i + 1])])
        assert got == deflate_dict(payloads[i], dicts[int(dict_of[i])], 1 if compat_go else 0), i
    sizes = [len(p) for p in payloads]
    back, boff, blen, status, _ = eng.inflate_batch(out, ooff, sizes, zdicts=dicts, dict_of=dict_of)
    assert (status == 0).all() and (blen == np.array(sizes, dtype=np.uint64)).all()
    assert bytes(back[:int(boff[-1])].cpu().numpy()) == b"".join(payloads)
    # the same batch through host pointers gives the same bytes
    out2, ooff2 = eng.deflate_batch(data, off, compat_go=compat_go, zdicts=dicts, dict_of=dict_of)
    assert (ooff2 == ooff).all() and bytes(out2[:int(ooff2[-1])]) == bytes(host[:int(ooff[-1])])


def test_small_batch_on_device_pointers(eng):
    payloads = [words(500 + i, 3000 + 900 * i) for i in range(40)]
    run_batch(eng, payloads, [words(51, 20000)], None, True, device=True)


def test_out_cap_too_small(eng):
    payloads = [words(600 + i, 4096) for i in range(8)]
    data, off = _pack(payloads)
    with pytest.raises(flate.FlateError) as e:
        eng.deflate_batch(data, off, out=np.empty(64, np.uint8), compat_go=True, zdicts=words(61, 32768))
    assert e.value.code == -2  # FLATE_HIP_E_OUT_TOO_SMALL


def _raw_call(eng, **kw):
    """flate_hip_deflate_fast_batch_dict with one argument replaced (the rest valid)."""
    L = eng._L
    data = np.frombuffer(words(70, 600) * 2 + b"\0" * 16, dtype=np.uint8).copy()
    in_off = np.array([0, 600, 1200], dtype=np.uint64)
    dicts = np.frombuffer(words(71, 500) + b"\0" * 16, dtype=np.uint8).copy()
    dict_off = np.array([0, 200, 500], dtype=np.uint64)
    dict_of = np.array([1, NO_DICT], dtype=np.uint32)
    out = np.zeros(8192, dtype=np.uint8)
    out_off = np.zeros(3, dtype=np.uint64)
    a = dict(ctx=eng._ctx, inp=data.ctypes.data, in_off=in_off.ctypes.data, n=2, dicts=dicts.ctypes.data,
             dict_off=dict_off.ctypes.data, n_dicts=2, dict_of=dict_of.ctypes.data, out=out.ctypes.data, cap=8192,
             out_off=out_off.ctypes.data, flags=0)
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        a[k] = v
    return L.flate_hip_deflate_fast_batch_dict(a["ctx"], a["inp"], a["in_off"], a["n"], a["dicts"], a["dict_off"],
                                               a["n_dicts"], a["dict_of"], a["out"], a["cap"], a["out_off"], a["flags"])


def test_invalid_arguments(eng):
    assert _raw_call(eng) == 0
    assert _raw_call(eng, ctx=None) == -1
    assert _raw_call(eng, in_off=None) == -1
    assert _raw_call(eng, out_off=None) == -1
    assert _raw_call(eng, inp=None) == -1
    assert _raw_call(eng, out=None) == -1
    assert _raw_call(eng, in_off=np.array([0, 700, 600], dtype=np.uint64)) == -1       # offsets run backwards
    assert _raw_call(eng, dict_off=None) == -1                                         # dictionaries without offsets
    assert _raw_call(eng, n_dicts=0, dict_of=None) == -1                               # "dictionary 0" of none
    assert _raw_call(eng, dict_off=np.array([0, 300, 200], dtype=np.uint64)) == -1     # offsets run backwards
    assert _raw_call(eng, dicts=None) == -1                                            # bytes missing
    assert _raw_call(eng, dict_of=np.array([2, 0], dtype=np.uint32)) == -1             # no such dictionary
    assert _raw_call(eng, flags=0x4) == -1                                             # FLATE_HIP_LZ_SERIAL + dictionary
    # (the serial kernel with dictionaries that are all too short to matter: the plain call, which has it)
    assert _raw_call(eng, flags=0x4, dict_off=np.array([0, 3, 16], dtype=np.uint64)) == 0
    assert _raw_call(eng, dict_of=None) == 0                                           # everyone uses dictionary 0
    assert _raw_call(eng, n=0) == 0


@pytest.mark.parametrize("compat_go", MODES)
def test_dictionaries_under_17_bytes_are_the_plain_call(eng, compat_go):
    payloads = [words(800 + i, n) for i, n in enumerate([0, 100, 128, 4096, 65536, 140000])]
    data, off = _pack(payloads)
    plain, poff = eng.deflate_batch(data, off, compat_go=compat_go)
    dicts = [words(81, 16), b"x", b""]
    got, goff = eng.deflate_batch(data, off, compat_go=compat_go, zdicts=dicts,
                                  dict_of=[0, 1, 2, NO_DICT, 0, 1])
    assert (goff == poff).all() and bytes(got[:int(goff[-1])]) == bytes(plain[:int(poff[-1])])


def test_framed_zlib_members_with_fdict(eng):
    dicts = [words(91, 32768), words(92, 700)]
    payloads = [words(950 + i, n) for i, n in enumerate([4096, 50, 70000, 0, 3000])]
    dict_of = [0, 1, 0, NO_DICT, 1]
    data, off = _pack(payloads)
    out, ooff = eng.deflate_batch_framed(data, off, "zlib", compat_go=True, zdicts=dicts, dict_of=dict_of)
    members = []
    for i, p in enumerate(payloads):
        m = bytes(out[int(ooff[i]):int(ooff[i + 1])])
        members.append(m)
        j = dict_of[i]
        if j == NO_DICT:
            assert not (m[1] & 0x20) and zlib.decompress(m) == p
            continue
        assert (m[1] & 0x20) and ((m[0] << 8) | m[1]) % 31 == 0
        assert int.from_bytes(m[2:6], "big") == zlib.adler32(dicts[j])
        d = zlib.decompressobj(zdict=dicts[j])
        assert d.decompress(m) == p and d.eof
        with pytest.raises(zlib.error):
            zlib.decompressobj().decompress(m)  # it needs its dictionary
    mdata, moff = _pack(members)
    back, boff, blen, status = eng.inflate_batch_framed(mdata, moff, "zlib", zdicts=dicts)
    assert (status == 0).all()
    for i, p in enumerate(payloads):
        assert bytes(back[int(boff[i]):int(boff[i]) + int(blen[i])]) == p
