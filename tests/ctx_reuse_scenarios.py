"""A table of single ABI calls with fixed small input, for the tests that reuse one flate_hip_ctx across families
(tests/test_ctx_reuse_scenarios.py on the CPU, tests/test_gpu_ctx_reuse.py on the GPU).  No tests in here.

A Scenario is one call: `run(eng, device)` makes it through FlateEngine (or eng._L where the wrapper hides an
argument) and returns a canonical tuple -- the rc of the call, every result word, every index or size array up to its
count, the delivered bytes; `expected` is the same tuple computed ONLY from the CPU references of tests/ and from
zlib / zipfile / gzip, never from a GPU run, once per session (bind(oracle) hands the session's oracle in).

Per family there are three good scenarios: X, its dirty twin X' (same API, same counts, other bytes: every per-item
size and offset differs from X at the same index and, where the call has per-item verdicts that a CPU reference can
state, at least one of them differs) and its big twin X+ (three to four times the counts, so that stale words lie BEHIND
X's arrays).  The read families add one scenario per failure class: CORRUPT in a middle item, UNEXPECTED_EOF, a capacity
one byte short, an index capacity too small, a refused argument.

Words the tuples do not state exactly, and why:
 * n_candidates of the inflate_one / seek / gzfile calls is canonicalised to `n_candidates >= n_units`: its exact value
   needs a bit-by-bit rule scan in Python over the whole stream (one_ref.candidates, small streams only); gzip_index
   states it exactly (gzip_ref.Walk has it).
 * the bytes of a member, entry or range whose status is not 0 are unspecified by the contract; both sides zero them.
 * lz77_matches takes host pointers only; its device runs are host runs.
The inflate_one / seek / gzfile streams are built as one_ref.good_streams() builds its memLevel-1 entry, from a shorter
text: the 300 000-byte entry has 230 units and no four-fold twin of it stays near the size these tests may have."""
import gzip
import io
import struct
import zipfile
import zlib
import ctypes as C

import numpy as np

import bgzf_range_ref as brr
import bgzf_ref as bg
import deflate_corpus as dc
import framed_read_ref as fr
import gzfile_ref as gf
import gzip_ref as gz
import lz77_corpus
import one_ref
import seek_ref as sk
import zip_ref
from deflate_dict_ref import deflate_dict
from util import STATUS_OF_ORACLE, flate, make_streams, raw_inflate

engine = flate.engine
NO_DICT = engine.NO_DICT
NONE32 = 0xffffffff
INVALID, OUT_TOO_SMALL, CORRUPT, UNEXPECTED_EOF = -1, -2, -4, -7
FAIL_CLASSES = ("corrupt", "eof", "capacity", "index_cap", "invalid")
DEVICE_PTRS = 1

_oracle = None


def bind(oracle):
    """The session's oracle (the conftest fixture): every `expected` is computed with it, once."""
    global _oracle
    _oracle = oracle


class Scenario:
    def __init__(self, name, family, role, build, call, fail=None, host_only=False):
        self.name, self.family, self.role, self.fail, self.host_only = name, family, role, fail, host_only
        self._build, self._call, self._data = build, call, None

    @property
    def data(self):
        if self._data is None:
            assert _oracle is not None, "ctx_reuse_scenarios.bind(oracle) first"
            self._data = self._build(_oracle)
        return self._data

    @property
    def expected(self):
        return self.data["expected"]

    def run(self, eng, device):
        return self._call(eng, self.data, bool(device) and not self.host_only)

    def __repr__(self):
        return self.name


# ---- marshalling ----

class Rc:
    """The rc of the last ABI call a wrapper method made (the wrappers hand back or raise it, but do not return it)."""

    def __init__(self, eng):
        self.eng, self.last = eng, None

    def __enter__(self):
        eng, cls = self.eng, type(self.eng)

        def check(rc):
            self.last = rc
            cls._check(eng, rc)

        def tolerate(rc, *allowed):
            self.last = rc
            if rc not in allowed:
                cls._check(eng, rc)
            return rc

        eng._check, eng._tolerate = check, tolerate
        return self

    def __exit__(self, *exc):
        del self.eng._check, self.eng._tolerate
        return False

    @property
    def rc(self):
        assert self.last is not None, "the wrapper method handed no rc to _check / _tolerate: Rc has to follow engine.py"
        return self.last


def refused(eng, fn):
    """The code of the FlateError fn() raises, or the rc it returns."""
    try:
        return int(fn())
    except flate.FlateError as e:
        return int(e.code)


def arr(b, pad=8):
    """bytes -> numpy uint8 with a few bytes behind (the batch calls are handed the buffer whatever its size)."""
    if isinstance(b, np.ndarray):
        return b
    return np.frombuffer(bytes(b) + b"\0" * pad, np.uint8).copy()


def dev(a, device):
    if not device:
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def view(a, n):
    """The first n bytes of a numpy array or a torch tensor: the single-buffer calls take their input's length from
    the buffer, which arr() has made a few bytes longer."""
    return a[:n]


def B(x, n=None, lo=0):
    if x is None:
        return b""
    x = x[lo:] if n is None else x[lo:lo + int(n)]
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    return (x.cpu().numpy() if engine._is_torch(x) else np.asarray(x)).tobytes()


def T(a):
    return None if a is None else tuple(int(v) for v in a)


def cum(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(np.asarray(lens, np.uint64), out=off[1:])
    return off


def blank(b, spans):
    b = bytearray(b)
    for lo, hi in spans:
        b[lo:hi] = bytes(hi - lo)
    return bytes(b)


def streams(specs, seed):
    data, off = make_streams(specs, seed=seed)
    return arr(data[:int(off[-1])].tobytes()), off, [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(specs))]


def meta(counts, sizes, offs, status=None):
    """counts: a tuple; sizes / offs: lists of per-item lists (offsets without the leading 0 that every table starts
    with); status: the per-item verdict words, None where the call has none."""
    return dict(counts=tuple(int(c) for c in counts), sizes=[[int(v) for v in s] for s in sizes],
                offs=[[int(v) for v in o] for o in offs], status=None if status is None else [int(v) for v in status])


def lens_of(off):
    return [int(b) - int(a) for a, b in zip(off, off[1:])]


def invalid_of(build):
    """The scenario's input with the expectation of a refused call."""
    def b(o):
        d = dict(build(o))
        d["expected"] = (INVALID,)
        return d
    return b


TABLE = []
FAMILIES = {}   # family -> {"X": ..., "dirty": ..., "big": ..., "more": [...], "fail": {class: scenario}}


def add(name, family, role, build, call, fail=None, host_only=False):
    # a refusal is made with host pointers, in the form the family's own tests have proven to be refused before any HIP
    # call (zip_read's is proven with device pointers too)
    host_only = host_only or (fail == "invalid" and family != "zip_read")
    s = Scenario(name, family, role, build, call, fail, host_only)
    TABLE.append(s)
    f = FAMILIES.setdefault(family, {"more": [], "fail": {}})
    if role in ("X", "dirty", "big"):
        assert role not in f, (family, role)
        f[role] = s
    elif role == "fail":
        f["fail"][fail] = s
    else:
        f["more"].append(s)
    return s


def twins(family, builds, call, **kw):
    for role, tag in (("X", "x"), ("dirty", "dirty"), ("big", "big")):
        add("%s/%s" % (family, tag), family, role, builds[role], call, **kw)


# ---- the encoders ----

ENC = {"X": ([("text", 0), ("rand", 1), ("text", 300), ("text", 65536), ("period", 70000)], 41),
       "dirty": ([("text", 5), ("text", 0), ("low", 280), ("runs", 65537), ("text", 69000)], 42),
       "big": ([("text", 0), ("rand", 1), ("text", 300), ("text", 65536), ("period", 70000), ("text", 16), ("rand", 17),
                ("low", 127), ("text", 128), ("runs", 1000), ("zero", 2000), ("ramp", 3000), ("text", 4096),
                ("period", 5000), ("text", 66000), ("rand", 9), ("text", 200), ("low", 700), ("text", 40000),
                ("rand", 65535)], 43)}
DICT_OF = [0, 1, NO_DICT, 0, 1]


def enc_dicts(n0=3000, n1=17):
    return [flate.synth("text", 1, n0, seed=31).tobytes(), flate.synth("text", 1, n1, seed=33).tobytes()]


def enc_result(data, off, parts, outs, **extra):
    ooff = cum([len(x) for x in outs])
    d = dict(data=data, off=off, expected=(0, T(ooff), b"".join(outs)),
             meta=meta((len(parts),), [lens_of(off), lens_of(ooff)], [off[1:], ooff[1:]]))
    d.update(extra)
    return d


def b_deflate(role, go):
    def build(o):
        data, off, parts = streams(*ENC[role])
        outs = [o.deflate(np.frombuffer(p, np.uint8), compat=int(go)) for p in parts]
        return enc_result(data, off, parts, outs, proof=[(raw_inflate(x), p) for x, p in zip(outs, parts)])
    return build


def c_deflate(go):
    def call(eng, d, device):
        with Rc(eng) as r:
            out, ooff = eng.deflate_batch(dev(d["data"], device), d["off"], compat_go=go)
        return (r.rc, T(ooff), B(out, ooff[-1]))
    return call


for _go, _fam in ((False, "deflate_batch"), (True, "deflate_batch_go")):
    twins(_fam, {r: b_deflate(r, _go) for r in ENC}, c_deflate(_go))
# enough streams for two groups of a host-pointer batch: each group runs on a lane, a sub-context with scratch of its own
ENC["many"] = ([(("text", "low", "runs", "rand")[k % 4], (k * 7) % 90) for k in range(4100)], 45)
add("deflate_batch/many_streams", "deflate_batch", "more", b_deflate("many", False), c_deflate(False))


def dict_of_for(n):
    return (DICT_OF * (n // 5 + 1))[:n]


def unzdict(x, d):
    z = zlib.decompressobj(-15, zdict=d) if d else zlib.decompressobj(-15)
    return z.decompress(x)


def b_deflate_dict(role):
    def build(o):
        data, off, parts = streams(*ENC[role])
        dicts, of = enc_dicts(), dict_of_for(len(parts))
        ds = [dicts[j] if j != NO_DICT else None for j in of]
        outs = [deflate_dict(p, d, 0) for p, d in zip(parts, ds)]
        return enc_result(data, off, parts, outs, dicts=dicts, dict_of=of,
                          proof=[(unzdict(x, d), p) for x, d, p in zip(outs, ds, parts)])
    return build


def c_deflate_dict(eng, d, device):
    with Rc(eng) as r:
        out, ooff = eng.deflate_batch(dev(d["data"], device), d["off"], zdicts=d["dicts"], dict_of=d["dict_of"])
    return (r.rc, T(ooff), B(out, ooff[-1]))


twins("deflate_batch_dict", {r: b_deflate_dict(r) for r in ENC}, c_deflate_dict)

LZ = {"X": ([("text", 300), ("period", 5000), ("text", 70000)], 51),
      "dirty": ([("low", 280), ("text", 4000), ("runs", 69000)], 52),
      "big": ([("text", 300), ("period", 5000), ("text", 70000), ("low", 128), ("text", 1000), ("runs", 2000),
               ("text", 131), ("rand", 400), ("text", 66000), ("zero", 900), ("text", 3000), ("ramp", 700)], 53)}


def b_lz77(role):
    def build(o):
        data, off, parts = streams(*LZ[role])
        chunks = [np.frombuffer(p[s:s + n], np.uint8) for p in parts for s, n in flate.lz_chunks(len(p))]
        toks = tuple(t.astype(np.uint32).tobytes() for p in parts for t in lz77_corpus.oracle_tokens(o, p, False))
        assert len(toks) == len(chunks)
        return dict(data=data, off=off, chunks=chunks, expected=(0, len(chunks), toks), proof=None,
                    meta=meta((len(parts), len(chunks)), [lens_of(off)], [off[1:]]))
    return build


def c_lz77(eng, d, device):
    with Rc(eng) as r:
        got = eng.lz77_matches(d["data"], d["off"])
    return (r.rc, len(got), tuple(flate.tokens_from_matches(c, pos, tok).astype(np.uint32).tobytes()
                                    for c, (pos, tok) in zip(d["chunks"], got)))


twins("lz77_matches", {r: b_lz77(r) for r in LZ}, c_lz77, host_only=True)


def b_spliced(role, wrap):
    def build(o):
        data, off, parts = streams(*ENC[role])
        raw, bit_off = o.deflate_spliced(data[:int(off[-1])], off)
        whole = b"".join(parts)
        if wrap is None:
            f, back = raw, raw_inflate(raw)
        else:
            f = o.frame(o.FRAME_ZLIB if wrap == "zlib" else o.FRAME_GZIP, raw, whole)
            back = zlib.decompress(f) if wrap == "zlib" else gzip.decompress(f)
        return dict(data=data, off=off, expected=(0, len(f), T(bit_off), f), proof=[(back, whole)],
                    meta=meta((len(parts),), [lens_of(off), lens_of(bit_off)], [off[1:], bit_off[1:]]))
    return build


def c_spliced(wrap):
    def call(eng, d, device):
        with Rc(eng) as r:
            if wrap is None:
                out, n, bit_off = eng.deflate_spliced(dev(d["data"], device), d["off"])
            else:
                out, n, bit_off = eng.deflate_spliced_framed(dev(d["data"], device), d["off"], wrap, index=True)
        return (r.rc, n, T(bit_off), B(out, n))
    return call


for _wrap, _fam in ((None, "deflate_spliced"), ("zlib", "deflate_spliced_zlib"), ("gzip", "deflate_spliced_gzip")):
    twins(_fam, {r: b_spliced(r, _wrap) for r in ENC}, c_spliced(_wrap))

SMALL = ([("text", 200), ("rand", 1), ("text", 300), ("low", 700), ("period", 900)], 44)


def b_framed(spec, wrap, dict_sizes=None):
    def build(o):
        data, off, parts = streams(*spec)
        if dict_sizes is None:
            dicts = of = None
            ds = [None] * len(parts)
        else:
            dicts, of = enc_dicts(*dict_sizes), dict_of_for(len(parts))
            ds = [dicts[j] if j != NO_DICT else None for j in of]
        kind = o.FRAME_ZLIB if wrap == "zlib" else o.FRAME_GZIP
        outs = [o.frame(kind, o.deflate(np.frombuffer(p, np.uint8)), p) if d is None else
                engine.zlib_dict_header(d) + deflate_dict(p, d, 0) + zlib.adler32(p).to_bytes(4, "big")
                for p, d in zip(parts, ds)]
        if wrap == "gzip":
            back = [gzip.decompress(m) for m in outs]
        else:
            back = [(zlib.decompressobj(zdict=d) if d else zlib.decompressobj()).decompress(m) for m, d in zip(outs, ds)]
        return enc_result(data, off, parts, outs, dicts=dicts, dict_of=of, proof=list(zip(back, parts)),
                          dict_bytes=sum(len(x) for x in dicts or []))
    return build


def c_framed(wrap):
    def call(eng, d, device):
        with Rc(eng) as r:
            out, ooff = eng.deflate_batch_framed(dev(d["data"], device), d["off"], wrap, zdicts=d["dicts"],
                                                 dict_of=d["dict_of"])
        return (r.rc, T(ooff), B(out, ooff[-1]))
    return call


twins("deflate_framed_zlib_dict", {r: b_framed(ENC[r], "zlib", (3000, 17)) for r in ENC}, c_framed("zlib"))
# (the other way round: the dictionaries are larger in total than the streams, so the call's two checksum runs swap sizes)
add("deflate_framed_zlib_dict/large_dicts", "deflate_framed_zlib_dict", "more", b_framed(SMALL, "zlib", (3000, 40000)),
    c_framed("zlib"))
twins("deflate_framed_gzip", {r: b_framed(ENC[r], "gzip") for r in ENC}, c_framed("gzip"))

CK = {"X": [0, 1, 65535, 65536, 65537, 200000], "dirty": [3, 0, 65534, 65537, 65538, 199999],
      "big": [0, 1, 65535, 65536, 65537, 100000] + [(977 * k) % 5000 for k in range(18)]}


def b_checksum(role, kind):
    def build(o):
        lens = CK[role]
        data = np.random.default_rng(60 + len(lens) + lens[0]).integers(0, 256, sum(lens) + 8, dtype=np.uint8)
        off = cum(lens)
        f = zlib.adler32 if kind == "adler32" else zlib.crc32
        sums = tuple(f(data[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(lens)))
        ref = tuple((o.adler32 if kind == "adler32" else o.crc32)(data[int(off[i]):int(off[i + 1])]) for i in range(len(lens)))
        return dict(data=data, off=off, expected=(0, sums), proof=[(ref, sums)],
                    meta=meta((len(lens),), [lens], [off[1:]]))
    return build


def c_checksum(kind):
    def call(eng, d, device):
        with Rc(eng) as r:
            sums = eng.checksum_batch(dev(d["data"], device), d["off"], kind)
        return (r.rc, T(sums))
    return call


for _kind in ("adler32", "crc32"):
    twins("checksum_" + _kind, {r: b_checksum(r, _kind) for r in CK}, c_checksum(_kind))


# ---- the batch decoders ----

def first_bad(status):
    return next((int(s) for s in status if s), 0)


def zraw(p, level=6, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(p) + c.flush()


_pool = []


def inflate_pool(o):
    """[(stream, cap, (status, err_off, bytes))]: the edge corpus without its dictionary and slot cases, then nine raw
    streams zlib wrote.  Computed once."""
    if not _pool:
        _pool.extend(_inflate_pool(o))
    return list(_pool)


def _inflate_pool(o):
    pool = [(c.data, c.cap) for c in dc.CASES if not c.zdict and c.cap >= len(c.out) and len(c.data) < 4000]
    t = gz.text(20000, seed=71)
    pool += [(zraw(t[a:b], lv), b - a) for a, b, lv in ((0, 3000, 6), (3000, 3700, 1), (3700, 9000, 9), (9000, 9100, 6),
                                                        (9100, 12000, 1), (12000, 12900, 9), (13000, 19000, 6),
                                                        (19000, 19400, 1), (19400, 20000, 9))]
    out = []
    for s, cap in pool:
        rc, got, _, eoff = o.inflate(s, cap, full=True)
        out.append((bytes(s), cap, (STATUS_OF_ORACLE[rc], eoff, got)))
    return out


def pick_inflate(o, role):
    pool = inflate_pool(o)
    corpus, foreign = pool[:-9], pool[-9:]
    x = corpus[0:36:3] + foreign[:3]
    if role == "X":
        return x
    if role == "big":
        return (x + corpus[1:36:3] + corpus[2:36:3] + foreign[3:] + corpus[36:51])[:60]
    # the dirty twin: at every index another stream, chosen so that every size and every running offset differs
    rest = [p for p in corpus[1:] + foreign[3:] if p not in x]
    out, sums, xs = [], [0, 0, 0], [0, 0, 0]
    for s, cap, (st, eo, got) in x:
        xs = [xs[0] + len(s), xs[1] + cap, xs[2] + len(got)]
        k = next(k for k, (s2, cap2, (st2, eo2, got2)) in enumerate(rest)
                 if len(s2) != len(s) and cap2 != cap and len(got2) != len(got) and sums[0] + len(s2) != xs[0]
                 and sums[1] + cap2 != xs[1] and (st2 != st or out))
        s2, cap2, v2 = rest.pop(k)
        sums = [sums[0] + len(s2), sums[1] + cap2, sums[2] + len(v2[2])]
        out.append((s2, cap2, v2))
    return out


def inflate_tuple(res):
    return (first_bad(v[0] for v in res), tuple(v[0] for v in res), tuple(v[1] for v in res),
            tuple(len(v[2]) for v in res), tuple(v[2] for v in res))


def spoiled_stream(o, spoil, zdict=None):
    """(stream, slot, (status, err_off, bytes)) of one raw stream zlib wrote, made to fail: its first block of the
    reserved type, its last 7 bytes missing, or its slot one byte short -- judged by the oracle."""
    p = gz.text(3000, seed=73)
    s, cap = zraw(p, 6, zdict), len(p)
    if spoil == "corrupt":
        s = bytes([s[0] | 0x06]) + s[1:]
    elif spoil == "eof":
        s = s[:-7]
    elif spoil == "capacity":
        cap -= 1
    rc, got, _, eoff = o.inflate(s, cap, full=True, zdict=zdict)
    want = {"corrupt": CORRUPT, "eof": UNEXPECTED_EOF, "capacity": OUT_TOO_SMALL}[spoil]
    assert STATUS_OF_ORACLE[rc] == want, (spoil, rc)
    return s, cap, (want, eoff, got)


def b_inflate(role, size_only=False, spoil=None):
    def build(o):
        picked = pick_inflate(o, role)
        if spoil:   # a middle stream that fails in the class's way
            picked[7] = spoiled_stream(o, spoil)
        off, caps = cum([len(s) for s, _, _ in picked]), [c for _, c, _ in picked]
        res = [v for _, _, v in picked]
        if size_only:  # no slot: the size every stream inflates to, up to its error
            res = []
            for s, _, _ in picked:
                rc, got, _, eoff = o.inflate(s, 1 << 20, full=True)
                res.append((STATUS_OF_ORACLE[rc], eoff, got))
        foreign = {p[0] for p in inflate_pool(o)[-9:]}   # (zlib reads what zlib wrote; the hand-built corpus is the oracle's)
        proof = [(raw_inflate(s), v[2]) for (s, _, _), v in zip(picked, res) if s in foreign and v[0] == 0]
        exp = inflate_tuple(res)
        return dict(data=arr(b"".join(s for s, _, _ in picked)), off=off, caps=caps, proof=proof,
                    expected=exp[:4] if size_only else exp,
                    meta=meta((len(picked),), [lens_of(off), caps, exp[3]], [off[1:], cum(caps)[1:]], exp[1]))
    return build


def delivered(out, ooff, olen):
    return tuple(B(out, olen[i], int(ooff[i])) for i in range(len(olen)))


def c_inflate(eng, d, device):
    with Rc(eng) as r:
        out, ooff, olen, status, err = eng.inflate_batch(dev(d["data"], device), d["off"], d["caps"], check=False)
    return (r.rc, T(status), T(err), T(olen), delivered(out, ooff, olen))


def c_inflate_sizes(eng, d, device):
    with Rc(eng) as r:
        olen, status, err = eng.inflate_sizes(dev(d["data"], device), d["off"])
    return (r.rc, T(status), T(err), T(olen))


twins("inflate_batch", {r: b_inflate(r) for r in ("X", "dirty", "big")}, c_inflate)


def b_inflate_many(o):
    """More streams than "inflate_simt_min_streams": the batch takes the lane-per-stream decoder by itself."""
    t = gz.text(60000, seed=72)
    ps = [t[23 * k:23 * k + (k * 13) % 120] for k in range(2100)]
    raws = [zraw(p, 1 + k % 9) for k, p in enumerate(ps)]
    raws[1000] = raws[1000][:-2]   # one stream in the middle cut short
    res = []
    for s, p in zip(raws, ps):
        rc, got, _, eoff = o.inflate(s, len(p), full=True)
        res.append((STATUS_OF_ORACLE[rc], eoff, got))
    assert res[1000][0] == UNEXPECTED_EOF
    return dict(data=arr(b"".join(raws)), off=cum([len(s) for s in raws]), caps=[len(p) for p in ps],
                expected=inflate_tuple(res), proof=[(raw_inflate(s), v[2]) for s, v in zip(raws, res) if v[0] == 0], meta=None)


add("inflate_batch/many_streams", "inflate_batch", "more", b_inflate_many, c_inflate)
twins("inflate_sizes", {r: b_inflate(r, True) for r in ("X", "dirty", "big")}, c_inflate_sizes)


def b_inflate_bad_args(o):
    d = b_inflate("X")(o)
    d["expected"] = (INVALID,)
    return d


def c_inflate_bad_args(eng, d, device):
    x, off = dev(d["data"], device), d["off"]
    n = off.size - 1
    ooff = cum(d["caps"])
    out = dev(np.zeros(int(ooff[-1]) + 8, np.uint8), device)
    st, eo = np.zeros(n, np.int32), np.zeros(n, np.int64)
    ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
    return (int(eng._L.flate_hip_inflate_batch(eng._ctx, ptr(x), off.ctypes.data, n, ptr(out), ooff.ctypes.data, None,
                                                st.ctypes.data, eo.ctypes.data, DEVICE_PTRS if device else 0)),)


add("inflate_batch/fail_invalid", "inflate_batch", "fail", b_inflate_bad_args, c_inflate_bad_args, fail="invalid")
for _cls in ("corrupt", "eof", "capacity"):
    add("inflate_batch/fail_" + _cls, "inflate_batch", "fail", b_inflate("X", spoil=_cls), c_inflate, fail=_cls)
for _cls in ("corrupt", "eof"):
    add("inflate_sizes/fail_" + _cls, "inflate_sizes", "fail", b_inflate("X", True, _cls), c_inflate_sizes, fail=_cls)


def c_inflate_sizes_bad_args(eng, d, device):
    x, off = d["data"], d["off"]
    n = off.size - 1
    st, eo = np.zeros(n, np.int32), np.zeros(n, np.int64)
    return (int(eng._L.flate_hip_inflate_batch(eng._ctx, x.ctypes.data, off.ctypes.data, n, None, None, None, st.ctypes.data,
                                                eo.ctypes.data, engine.SIZE_ONLY)),)


add("inflate_sizes/fail_invalid", "inflate_sizes", "fail", invalid_of(b_inflate("X", True)), c_inflate_sizes_bad_args,
    fail="invalid")

DICT_LENS = {"X": [2000, 300, 7000, 0, 5000, 900], "dirty": [1900, 310, 6000, 40, 5100, 800],
             "big": [2000, 300, 7000, 0, 5000, 900] + [(613 * k) % 4000 for k in range(18)]}


def b_inflate_dict(role, spoil=None):
    def build(o):
        lens = list(DICT_LENS[role])
        dicts = enc_dicts(3000, 500)
        of = [[0, 1, NO_DICT][k % 3] for k in range(len(lens))]
        t = gz.text(sum(lens) + 400, seed=80 + len(lens) + lens[0])
        ps, at = [], 0
        for n, j in zip(lens, of):
            ps.append(((dicts[j][-200:] if j != NO_DICT else b"") + t[at:at + n])[:n])
            at += n
        raws = [zraw(p, 6, dicts[j] if j != NO_DICT else None) for p, j in zip(ps, of)]
        caps = list(lens)
        if role == "dirty":
            raws[2] = raws[2][:len(raws[2]) // 2]  # cut short: -7, the bytes in front delivered
        res = []
        for s, p, j in zip(raws, ps, of):
            rc, got, _, eoff = o.inflate(s, len(p), full=True, zdict=dicts[j] if j != NO_DICT else None)
            res.append((STATUS_OF_ORACLE[rc], eoff, got))
        if spoil:   # stream 3, written with dictionary 0, fails in the class's way
            assert of[3] == 0
            raws[3], caps[3], res[3] = spoiled_stream(o, spoil, dicts[0])
        exp = inflate_tuple(res)
        off = cum([len(s) for s in raws])
        return dict(data=arr(b"".join(raws)), off=off, caps=caps, dicts=dicts, dict_of=of, expected=exp,
                    proof=[(unzdict(s, dicts[j] if j != NO_DICT else None), v[2])
                           for s, j, v in zip(raws, of, res) if v[0] == 0],
                    meta=meta((len(lens),), [lens_of(off), lens, exp[3]], [off[1:], cum(lens)[1:]], exp[1]))
    return build


def c_inflate_dict(eng, d, device):
    with Rc(eng) as r:
        out, ooff, olen, status, err = eng.inflate_batch(dev(d["data"], device), d["off"], d["caps"], check=False,
                                                         zdicts=d["dicts"], dict_of=d["dict_of"])
    return (r.rc, T(status), T(err), T(olen), delivered(out, ooff, olen))


twins("inflate_batch_dict", {r: b_inflate_dict(r) for r in DICT_LENS}, c_inflate_dict)
for _cls in ("corrupt", "eof", "capacity"):
    add("inflate_batch_dict/fail_" + _cls, "inflate_batch_dict", "fail", b_inflate_dict("X", _cls), c_inflate_dict, fail=_cls)


def c_inflate_dict_bad_args(eng, d, device):
    x, off = d["data"], d["off"]
    n = off.size - 1
    ooff = cum(d["caps"])
    out = np.zeros(int(ooff[-1]) + 8, np.uint8)
    st, eo = np.zeros(n, np.int32), np.zeros(n, np.int64)
    return (int(eng._L.flate_hip_inflate_batch_dict(eng._ctx, x.ctypes.data, off.ctypes.data, n, None, None, 0, None,
                                                     out.ctypes.data, ooff.ctypes.data, None, st.ctypes.data, eo.ctypes.data,
                                                     0)),)


add("inflate_batch_dict/fail_invalid", "inflate_batch_dict", "fail", invalid_of(b_inflate_dict("X")), c_inflate_dict_bad_args,
    fail="invalid")


def framed_payloads(role):
    if role == "X":
        return fr.make_payloads()
    if role == "dirty":
        data, off = make_streams([(fr.FILLS[(k + 2) % 7], n + 3) for k, n in enumerate(fr.LENGTHS)], seed=78)
    else:
        data, off = make_streams([(fr.FILLS[k % 7], (1117 * k) % 6000) for k in range(60)], seed=79)
    return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def b_inflate_framed(role, wrap, spoil=None):
    def build(o):
        ps = framed_payloads(role)
        ms = [fr.oracle_member(o, wrap, p) for p in ps]
        slots = [len(p) for p in ps]
        hl, tl = (2, 4) if wrap == "zlib" else (10, 8)
        if role == "dirty" or spoil == "corrupt":   # a flipped checksum bit: -4 at the member's end, all delivered
            b = bytearray(ms[7])
            b[len(b) - tl + 2] ^= 0x04
            ms[7] = bytes(b)
        if spoil == "eof":
            ms[7] = ms[7][:hl] + ms[7][hl:-tl][:-7] + ms[7][-tl:]
        if spoil == "capacity":
            slots[7] -= 1
        res = [fr.expected(o, m, wrap, s, None) for m, s in zip(ms, slots)]
        off = cum([len(m) for m in ms])
        exp = (first_bad(v[0] for v in res), tuple(v[0] for v in res), tuple(v[1] for v in res),
               tuple(len(v[2]) for v in res), tuple(v[3] for v in res), tuple(v[2] for v in res))
        rd = zlib.decompress if wrap == "zlib" else gzip.decompress
        return dict(data=arr(b"".join(ms)), off=off, slots=slots, expected=exp,
                    proof=[(rd(m), v[2]) for m, v in zip(ms, res) if v[0] == 0],
                    meta=meta((len(ms),), [lens_of(off), slots], [off[1:], cum(slots)[1:]], exp[1]))
    return build


def c_inflate_framed(wrap):
    def call(eng, d, device):
        with Rc(eng) as r:
            out, ooff, olen, status = eng.inflate_batch_framed(dev(d["data"], device), d["off"], wrap, out_sizes=d["slots"])
        err, used = eng.last_framed_read
        return (r.rc, T(status), T(err), T(olen), T(used), delivered(out, ooff, olen))
    return call


def c_inflate_framed_bad_wrap(eng, d, device):
    x, off = dev(d["data"], device), d["off"]
    n = off.size - 1
    ooff = cum(d["slots"])
    out = dev(np.zeros(int(ooff[-1]) + 8, np.uint8), device)
    ol, st, eo, used = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.uint32)
    ptr = (lambda a: a.data_ptr()) if device else (lambda a: a.ctypes.data)
    return (int(eng._L.flate_hip_inflate_batch_framed(
        eng._ctx, ptr(x), off.ctypes.data, n, 3, None, None, 0, ptr(out), ooff.ctypes.data, ol.ctypes.data, st.ctypes.data,
        eo.ctypes.data, used.ctypes.data, DEVICE_PTRS if device else 0)),)


for _wrap in ("zlib", "gzip"):
    _fam = "inflate_framed_" + _wrap
    twins(_fam, {r: b_inflate_framed(r, _wrap) for r in ("X", "dirty", "big")}, c_inflate_framed(_wrap))
    for _cls in ("corrupt", "eof", "capacity"):
        add("%s/fail_%s" % (_fam, _cls), _fam, "fail", b_inflate_framed("X", _wrap, _cls), c_inflate_framed(_wrap), fail=_cls)
    add(_fam + "/fail_invalid", _fam, "fail", invalid_of(b_inflate_framed("big", _wrap)), c_inflate_framed_bad_wrap,
        fail="invalid")


def spliced_specs(role):
    from spliced_framed_ref import SPECS
    if role == "X":
        return SPECS, 13
    if role == "dirty":
        return [(SPECS[(i + 1) % len(SPECS)][0], n - 3 if n > 3 else n + 1) for i, (_, n) in enumerate(SPECS)], 14
    kinds = ["text", "rand", "zero", "low", "period", "runs"]
    return [(kinds[k % 6], 0 if k % 7 == 3 else (733 * k) % 5000 + (66000 if k == 20 else 0)) for k in range(60)], 15


def b_inflate_spliced(role, wrap, spoil=None):
    """spoil, every verdict the oracle's on the raw stream read from its first byte: "trailer" (framed: every piece 0 and
    delivered, the member corrupt at its end); "eof": the raw stream's last byte missing, the last piece -7 with what a
    reader of the cut stream has in hand; "head": piece 0 starts with a block of the reserved type; "capacity": piece 0's
    slot one byte short.  (Pieces behind the first start at bit offsets the oracle cannot start from: the first and the
    last piece are the ones a CPU reference judges.)"""
    def build(o):
        from spliced_framed_ref import Member
        specs, seed = spliced_specs(role)
        m = Member(o, specs, wrap or "zlib", seed=seed)
        n = len(specs)
        raw, slots = m.raw, list(m.sizes)
        status, err, pieces = [0] * n, [-1] * n, list(m.pieces)
        ms, me = 0, -1
        if spoil == "eof":
            raw = raw[:-1]
            assert int(m.bit_off[-1]) <= 8 * len(raw)
            rc, got, _, eoff = o.inflate(raw, len(m.whole), full=True)
            assert rc == o.E_UNEXPECTED_EOF and got[:sum(m.sizes[:-1])] == b"".join(m.pieces[:-1])
            status[-1], pieces[-1] = UNEXPECTED_EOF, got[sum(m.sizes[:-1]):]
        elif spoil == "head":
            raw = bytes([raw[0] | 0x06]) + raw[1:]
            rc, got, _, eoff = o.inflate(raw, len(m.whole), full=True)
            assert rc == o.E_CORRUPT and got == b""
            status[0], err[0], pieces[0] = CORRUPT, eoff, b""
        elif spoil == "capacity":
            slots[0] -= 1
            rc, got, _, eoff = o.inflate(raw, slots[0], full=True)
            assert rc == o.E_OUT_TOO_SMALL
            status[0], err[0], pieces[0] = OUT_TOO_SMALL, eoff, got
        first = first_bad(status)
        olen = tuple(len(p) for p in pieces)
        if wrap is None:
            f = raw
            exp = (first, tuple(status), tuple(err), olen, tuple(pieces))
        else:
            f, ms = m.member[:m.hl] + raw + m.trailer, first
            if spoil == "trailer":
                b = bytearray(f)
                b[len(b) - m.tl + 1] ^= 0x10
                f, ms, me = bytes(b), CORRUPT, len(b)
            exp = (ms, tuple(status), tuple(err), olen, ms, me, tuple(pieces))
        if spoil:
            proof = []
        elif wrap is None:
            proof = [(raw_inflate(m.raw), m.whole)]
        else:
            proof = [((zlib.decompress if wrap == "zlib" else gzip.decompress)(m.member), m.whole)]
        return dict(data=arr(f), nbytes=len(f), bit_off=m.bit_off, sizes=slots, expected=exp, proof=proof,
                    meta=meta((n,), [lens_of(m.bit_off), m.sizes], [m.bit_off[1:], cum(m.sizes)[1:]],
                              status + ([] if wrap is None else [ms])))
    return build


def c_inflate_spliced(wrap):
    def call(eng, d, device):
        x = dev(d["data"], device)
        with Rc(eng) as r:
            if wrap is None:
                out, ooff, olen, status, err = eng.inflate_spliced(x, d["nbytes"], d["bit_off"], d["sizes"], check=False)
                return (r.rc, T(status), T(err), T(olen), delivered(out, ooff, olen))
            out, ooff, olen, status, err, ms = eng.inflate_spliced_framed(x, d["nbytes"], wrap, d["bit_off"], d["sizes"],
                                                                          check=False)
        return (r.rc, T(status), T(err), T(olen), ms, eng.last_member_err_off, delivered(out, ooff, olen))
    return call


def c_spliced_bad_args(wrap):
    """The raw call without its status array; the framed call with a wrap that does not exist."""
    def call(eng, d, device):
        x, bits = d["data"], np.ascontiguousarray(d["bit_off"], np.uint64)
        n = bits.size - 1
        ooff = cum(d["sizes"])
        out = np.zeros(int(ooff[-1]) + 16, np.uint8)
        olen, st, eo = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int64)
        if wrap is None:
            return (int(eng._L.flate_hip_inflate_spliced(eng._ctx, x.ctypes.data, d["nbytes"], bits.ctypes.data, n,
                                                          out.ctypes.data, ooff.ctypes.data, olen.ctypes.data, None,
                                                          eo.ctypes.data, 0)),)
        return (int(eng._L.flate_hip_inflate_spliced_framed(eng._ctx, x.ctypes.data, d["nbytes"], 3, bits.ctypes.data, n,
                                                             out.ctypes.data, ooff.ctypes.data, olen.ctypes.data,
                                                             st.ctypes.data, eo.ctypes.data, None, None, 0)),)
    return call


for _wrap, _fam in ((None, "inflate_spliced"), ("zlib", "inflate_spliced_zlib"), ("gzip", "inflate_spliced_gzip")):
    # the dirty twins: the raw call's last piece cut short, the framed calls' trailer wrong
    twins(_fam, {r: b_inflate_spliced(r, _wrap, ("trailer" if _wrap else "eof") if r == "dirty" else None)
                 for r in ("X", "dirty", "big")}, c_inflate_spliced(_wrap))
    for _cls, _spoil in (("corrupt", "head"), ("eof", "eof"), ("capacity", "capacity")):
        add("%s/fail_%s" % (_fam, _cls), _fam, "fail", b_inflate_spliced("X", _wrap, _spoil), c_inflate_spliced(_wrap), fail=_cls)
    if _wrap:
        add(_fam + "/wrong_trailer", _fam, "more_fail", b_inflate_spliced("X", _wrap, "trailer"), c_inflate_spliced(_wrap),
            fail="corrupt")
    add(_fam + "/fail_invalid", _fam, "fail", invalid_of(b_inflate_spliced("X", _wrap)), c_spliced_bad_args(_wrap), fail="invalid")


# ---- the files: one buffer in, one buffer out ----

def flip(f, at, bit=0x10):
    b = bytearray(f)
    b[at] ^= bit
    return bytes(b)


def own_out(d, device, n):
    """A caller's buffer of exactly n bytes (the capacity the library is told)."""
    return dev(np.zeros(max(n, 1), np.uint8), device)


BGZF = {"X": (18000, 4096, 9), "dirty": (17500, 4000, 10), "big": (20 * 4096 + 7, 4096, 11)}


def bgzf_file(o, role):
    n, bb, seed = BGZF[role]
    data = bg.text(n, seed=seed)
    f, moff = bg.build_file(o, data, bb)
    return data, bb, f, moff


def b_bgzf_write(role):
    def build(o):
        data, bb, f, moff = bgzf_file(o, role)
        return dict(data=arr(data, 0), bb=bb, expected=(0, len(f), T(moff), f), proof=[(gzip.decompress(f), data)],
                    meta=meta((len(moff) - 1,), [lens_of(moff)], [moff[1:]]))
    return build


def c_bgzf_write(eng, d, device):
    with Rc(eng) as r:
        res = eng.bgzf_write(dev(d["data"], device), block_bytes=d["bb"], index=True)
    out, n, moff = res if device else (res[0], len(res[0]), res[1])
    return (r.rc, n, T(moff), B(out, n))


twins("bgzf_write", {r: b_bgzf_write(r) for r in BGZF}, c_bgzf_write)


def bgzf_read_file(o, role, spoil=None):
    """(file, {bad member: status}); "corrupt": a flipped CRC in member 2, as failing_files() makes one (the dirty twins
    of the reads have it too)."""
    data, bb, f, moff = bgzf_file(o, role)
    bad = {}
    if spoil == "corrupt":
        f, bad = flip(f, int(moff[3]) - 6), {2: CORRUPT}
    if spoil == "eof":   # member 2's raw stream cut short, its BSIZE lowered with it
        m = f[int(moff[2]):int(moff[3])]
        cut = bg.wrap_raw(m[18:-8][:-9], gzip.decompress(m))
        f, bad = f[:int(moff[2])] + cut + f[int(moff[3]):], {2: UNEXPECTED_EOF}
    return f, bad


def bgzf_meta(w, bad=None):
    """The members in front of the EOF marker (28 bytes and no output in every file: a constant of the format)."""
    n = w.n_members - w.eof_marker
    return meta((w.n_members,), [lens_of(w.member_off)[:n], lens_of(w.out_off)[:n]], [w.member_off[1:], w.out_off[1:n + 1]],
                None if bad is None else [bad.get(i, 0) for i in range(w.n_members)])


def b_bgzf_index(role, cap_short=False, malformed=False):
    def build(o):
        f, _ = bgzf_read_file(o, role)
        w = bg.Walk(f)
        if malformed:   # cut inside member 2's header: no member can be read there, behind two good ones
            f = f[:w.member_off[2] + 7]
            w = bg.Walk(f)
            assert (w.rc, w.n_members) == (CORRUPT, 2)
            return dict(data=arr(f), n=len(f), cap=None, proof=[], meta=None,
                        expected=(CORRUPT, 2, 0, 0, w.err_off, None, None))
        exp = (0, w.n_members, w.out_bytes, w.eof_marker, w.err_off, T(w.member_off), T(w.out_off))
        if cap_short:
            exp = (OUT_TOO_SMALL, w.n_members, w.out_bytes) + (None, None)
        return dict(data=arr(f), n=len(f), cap=w.n_members if cap_short else None, expected=exp,
                    proof=[(len(gzip.decompress(f)), w.out_bytes)],
                    meta=bgzf_meta(w))
    return build


def c_bgzf_index(eng, d, device):
    with Rc(eng) as r:
        ix = eng.bgzf_index(view(dev(d["data"], device), d["n"]), index_cap=d["cap"])
    if d["cap"] is not None:
        return (r.rc, ix.n_members, ix.out_bytes, T(ix.member_off), T(ix.out_off))
    return (r.rc,) + tuple(ix[1:5]) + (T(ix.member_off), T(ix.out_off))


twins("bgzf_index", {r: b_bgzf_index(r) for r in BGZF}, c_bgzf_index)


def b_bgzf_markers(read):
    """Nothing but empty members, more than the discovery's arrays hold at first: the pass is repeated inside the call
    with arrays sized from the count -- on a new ctx the buffer grows twice in one call, on a used one not at all."""
    def build(o):
        f = bg.EOF * 6000
        w = bg.Walk(f)
        assert w.n_members == 6000 > 4096 + len(f) // 1024 and gzip.decompress(f) == b""
        if read:
            return dict(data=arr(f), n=len(f), cap=16, blank=[], proof=[(gzip.decompress(f), b"")], meta=None,
                        expected=(0, 0, 6000, NONE32, -1, 1, b""))
        return dict(data=arr(f), n=len(f), cap=None, proof=[(gzip.decompress(f), b"")], meta=None,
                    expected=(0, 6000, 0, 1, -1, T(w.member_off), T(w.out_off)))
    return build


add("bgzf_index/many_markers", "bgzf_index", "more", b_bgzf_markers(False), c_bgzf_index)
add("bgzf_index/fail_index_cap", "bgzf_index", "fail", b_bgzf_index("X", True), c_bgzf_index, fail="index_cap")
add("bgzf_index/fail_corrupt", "bgzf_index", "fail", b_bgzf_index("X", malformed=True), c_bgzf_index, fail="corrupt")


def c_one_array_without_the_other(name):
    """flate_hip_bgzf_index / flate_hip_gzip_index handed one of the two arrays: refused before any HIP call."""
    def call(eng, d, device):
        x, one = d["data"], np.zeros(64, np.uint64)
        nm, ob = C.c_uint32(0), C.c_uint64(0)
        return (int(getattr(eng._L, name)(eng._ctx, x.ctypes.data, d["n"], 4, one.ctypes.data, None, C.byref(nm),
                                          C.byref(ob), None, None, 0)),)
    return call


add("bgzf_index/fail_invalid", "bgzf_index", "fail", invalid_of(b_bgzf_index("X")),
    c_one_array_without_the_other("flate_hip_bgzf_index"), fail="invalid")


def b_bgzf_read(role, spoil=None):
    def build(o):
        f, bad = bgzf_read_file(o, role, "corrupt" if role == "dirty" else spoil)
        w = bg.Walk(f)
        if spoil == "malformed":  # a chain the walk cannot finish: nothing decoded
            f = f[:w.member_off[2] + 7]
            w = bg.Walk(f)
            exp = (CORRUPT, 0, w.n_members, w.n_members, w.err_off, 0, b"")
            return dict(data=arr(f), n=len(f), cap=8192, blank=[], expected=exp, proof=[],
                        meta=meta((w.n_members,), [[0]], [[0]], [CORRUPT]))
        parts = [gzip.decompress(m) if k not in bad else bytes(w.out_off[k + 1] - w.out_off[k])
                 for k, m in enumerate(w.members(f))]
        k = min(bad) if bad else None
        exp = (bad[k] if bad else 0, w.out_bytes, w.n_members, NONE32 if k is None else k,
               -1 if k is None else w.member_off[k], w.eof_marker, b"".join(parts))
        cap = w.out_bytes
        if spoil == "capacity":
            cap, exp = w.out_bytes - 1, (OUT_TOO_SMALL, w.out_bytes, w.n_members, NONE32, -1, w.eof_marker, b"")
        return dict(data=arr(f), n=len(f), cap=cap, blank=[(w.out_off[k], w.out_off[k + 1]) for k in bad], expected=exp,
                    proof=[] if bad or spoil else [(gzip.decompress(f), exp[6])],
                    meta=bgzf_meta(w, bad))
    return build


def read_bytes(out, r_out_len, d):
    """What a read delivered: out[:out_len] when it fits the capacity, the unspecified spans zeroed."""
    n = r_out_len if r_out_len <= d["cap"] else 0
    return blank(B(out, n), [(lo, hi) for lo, hi in d["blank"] if hi <= n])


def c_bgzf_read(eng, d, device):
    with Rc(eng) as r:
        out, q = eng.bgzf_read(view(dev(d["data"], device), d["n"]), out=own_out(d, device, d["cap"]), out_cap=d["cap"])
    n = q.out_len if q.rc != OUT_TOO_SMALL or q.bad_member != NONE32 else 0
    return (r.rc,) + tuple(q[1:]) + (read_bytes(out, n, d),)


twins("bgzf_read", {r: b_bgzf_read(r) for r in BGZF}, c_bgzf_read)
add("bgzf_read/many_markers", "bgzf_read", "more", b_bgzf_markers(True), c_bgzf_read)
for _cls, _spoil in (("corrupt", "corrupt"), ("eof", "eof"), ("capacity", "capacity")):
    add("bgzf_read/fail_" + _cls, "bgzf_read", "fail", b_bgzf_read("X", _spoil), c_bgzf_read, fail=_cls)
add("bgzf_read/fail_invalid", "bgzf_read", "fail", invalid_of(b_bgzf_read("X")),
    lambda eng, d, device: (int(eng._L.flate_hip_bgzf_read(eng._ctx, d["data"].ctypes.data, d["n"], d["data"].ctypes.data, 0,
                                                           None, None, None, None, None, 0)),), fail="invalid")
add("bgzf_read/malformed_chain", "bgzf_read", "more_fail", b_bgzf_read("X", "malformed"), c_bgzf_read, fail="corrupt")


def b_bgzf_ranges(role, virtual, spoil=None):
    def build(o):
        f, bad = bgzf_read_file(o, role, "corrupt" if role == "dirty" else spoil)
        w = bg.Walk(f)
        rs = brr.virtual_edge_ranges(f, w) if virtual else brr.byte_edge_ranges(w)
        if role == "big":
            rs = rs[:4 * len(b_bgzf_ranges("X", virtual)(o)["begin"])]
        if spoil == "invalid":
            rs = [(5, 4)]
        begin, end = [a for a, _ in rs], [b for _, b in rs]
        R = brr.read_ranges(f, brr.POS_VIRTUAL if virtual else brr.POS_BYTES, begin, end, status=bad)
        if spoil == "invalid":
            return dict(data=arr(f), n=len(f), begin=begin, end=end, virtual=virtual, cap=64, blank=[], expected=(INVALID,),
                        proof=[], meta=None)
        cap = R.out_off[-1]
        spans = [(R.out_off[i], R.out_off[i + 1]) for i in range(len(rs)) if not R.exact[i]]
        exp = (R.rc, T(R.out_off), T(R.range_status), R.n_members, R.n_decoded, R.bad_member, R.err_off, blank(R.data, spans))
        if spoil == "capacity":
            cap -= 1
            exp = (OUT_TOO_SMALL, T(R.out_off), None, R.n_members, None, None, None, b"")
        return dict(data=arr(f), n=len(f), begin=begin, end=end, virtual=virtual, cap=cap, blank=spans, expected=exp,
                    proof=None if virtual else [] if bad or spoil else
                    [(b"".join(gzip.decompress(f)[min(a, w.out_bytes):min(b, w.out_bytes)] for a, b in rs), exp[7])],
                    meta=bgzf_meta(w, bad))
    return build


def c_bgzf_ranges(eng, d, device):
    x = view(dev(d["data"], device), d["n"])
    if d["expected"] == (INVALID,):
        return (refused(eng, lambda: eng.bgzf_read_ranges(x, d["begin"], d["end"], virtual=d["virtual"],
                                                          out=own_out(d, device, 64))[1].rc),)
    with Rc(eng) as r:
        out, q = eng.bgzf_read_ranges(x, d["begin"], d["end"], virtual=d["virtual"], out=own_out(d, device, d["cap"]),
                                      out_cap=d["cap"])
    if int(q.out_off[-1]) > d["cap"]:   # too small: the layout, nothing decoded
        return (r.rc, T(q.out_off), None, q.n_members, None, None, None, b"")
    return (r.rc, T(q.out_off), T(q.range_status), q.n_members, q.n_decoded, q.bad_member, q.err_off,
            read_bytes(out, int(q.out_off[-1]), d))


for _virtual, _fam in ((False, "bgzf_ranges_bytes"), (True, "bgzf_ranges_virtual")):
    twins(_fam, {r: b_bgzf_ranges(r, _virtual) for r in BGZF}, c_bgzf_ranges)
    for _cls in ("corrupt", "eof", "capacity", "invalid"):
        add("%s/fail_%s" % (_fam, _cls), _fam, "fail", b_bgzf_ranges("X", _virtual, _cls), c_bgzf_ranges, fail=_cls)


def gzip_members(role):
    """[(member, plain)]: tiny_members(6) for X; the twins are built the same way from other sizes."""
    if role == "X":
        f, plain = gz.tiny_members(6)
        w = gz.Walk(f)
        return [(m, plain[w.out_off[i]:w.out_off[i + 1]]) for i, m in enumerate(w.members(f))]
    rng = np.random.default_rng(5 if role == "dirty" else 6)
    out = []
    for k in range(6 if role == "dirty" else 24):
        p = b"" if k % 4 == 2 else bytes(rng.integers(32, 127, (k * 11 + 3) % 43 + (50 if role == "dirty" else 0), dtype=np.uint8))
        out.append(((gz.fixed(p, flg=gz.FNAME, name=b"n%d" % k) if k % 3 == 0 else gz.stored(p)), p))
    return out


def gzip_file(role, spoil=None):
    ms = gzip_members(role)
    f, plain = b"".join(m for m, _ in ms), b"".join(p for _, p in ms)
    at = sum(len(m) for m, _ in ms[:3])  # the end of member 2
    bad = {}
    if spoil == "trailer":
        f, bad = flip(f, at - 8, 0x40), {2: CORRUPT}
    return f, plain, bad, at


def b_gzip_index(role, spoil=None):
    def build(o):
        f, plain, _, at = gzip_file(role)
        if spoil == "corrupt":   # member 3 starts with a block of the reserved type: the chain breaks in the middle
            hl = gz.header_len(f, at, len(f))
            f = f[:at + hl] + b"\x07" + f[at + hl + 1:]
        if spoil == "eof":
            f = f[:-9]
        w = gz.Walk(f)
        exp = (w.rc, w.n_members, w.out_bytes, w.n_candidates, w.err_off, T(w.member_off), T(w.out_off))
        cap = None
        if spoil == "index_cap":
            cap, exp = w.n_members, (OUT_TOO_SMALL, w.n_members, w.out_bytes, w.n_candidates, -1, None, None)
        return dict(data=arr(f), n=len(f), cap=cap, expected=exp, proof=[(len(gz.plain_of(f)), w.out_bytes)] if not w.rc else [],
                    meta=meta((w.n_members,), [lens_of(w.member_off), lens_of(w.out_off)], [w.member_off[1:], w.out_off[1:]]))
    return build


def c_gzip_index(eng, d, device):
    with Rc(eng) as r:
        ix = eng.gzip_index(view(dev(d["data"], device), d["n"]), index_cap=d["cap"])
    return (r.rc,) + tuple(ix[1:5]) + (T(ix.member_off), T(ix.out_off))


def b_gzip_read(role, spoil=None):
    def build(o):
        f, plain, bad, at = gzip_file(role, "trailer" if spoil == "corrupt" or role == "dirty" else None)
        if spoil == "eof":
            f = f[:-9]
        w = gz.Walk(f)
        if w.rc:   # a broken chain: the index call's verdict, nothing decoded
            exp = (w.rc, 0, w.n_members, w.n_members, w.err_off, b"")
            return dict(data=arr(f), n=len(f), cap=4096, blank=[], expected=exp, proof=[], meta=None)
        k = min(bad) if bad else None
        spans = [(w.out_off[k], w.out_off[k + 1]) for k in bad]
        exp = (bad[k] if bad else 0, w.out_bytes, w.n_members, NONE32 if k is None else k,
               -1 if k is None else w.member_off[k], blank(plain, spans))
        cap = w.out_bytes
        if spoil == "capacity":
            cap, exp = cap - 1, (OUT_TOO_SMALL, w.out_bytes, w.n_members, NONE32, -1, b"")
        return dict(data=arr(f), n=len(f), cap=cap, blank=spans, expected=exp,
                    proof=[] if bad or spoil else [(gz.plain_of(f), exp[5])],
                    meta=meta((w.n_members,), [lens_of(w.member_off), lens_of(w.out_off)], [w.member_off[1:], w.out_off[1:]],
                              [bad.get(i, 0) for i in range(w.n_members)]))
    return build


def c_gzip_read(eng, d, device):
    with Rc(eng) as r:
        out, q = eng.gzip_read(view(dev(d["data"], device), d["n"]), out=own_out(d, device, d["cap"]), out_cap=d["cap"])
    return (r.rc,) + tuple(q[1:]) + (read_bytes(out, q.out_len, d),)


def b_gzip_decoy(o):
    what, f, plain, more = gz.decoy_files()[0]
    w = gz.Walk(f)
    assert w.n_candidates > w.n_members
    return dict(data=arr(f), n=len(f), cap=len(plain), blank=[], proof=[(gz.plain_of(f), plain)], meta=None,
                expected=(0, w.out_bytes, w.n_members, NONE32, -1, plain))


def c_flags_refused(name, args_of):
    """A call refused for its flags before any HIP call: FLATE_HIP_SIZE_ONLY (8) where it has no meaning."""
    def call(eng, d, device):
        x = view(dev(d["data"], device), d["n"])
        ptr = x.data_ptr() if device else x.ctypes.data
        keep = [C.c_uint64(0), C.c_int32(0), np.zeros(64, np.uint8)]
        return (int(getattr(eng._L, name)(eng._ctx, ptr, d["n"], *args_of(keep), 8 | (DEVICE_PTRS if device else 0))),)
    return call


twins("gzip_index", {r: b_gzip_index(r) for r in ("X", "dirty", "big")}, c_gzip_index)
twins("gzip_read", {r: b_gzip_read(r) for r in ("X", "dirty", "big")}, c_gzip_read)
add("gzip_read/decoys", "gzip_read", "more", b_gzip_decoy, c_gzip_read)
for _cls in ("corrupt", "eof", "index_cap"):
    add("gzip_index/fail_" + _cls, "gzip_index", "fail", b_gzip_index("X", _cls), c_gzip_index, fail=_cls)
for _cls in ("corrupt", "eof", "capacity"):
    add("gzip_read/fail_" + _cls, "gzip_read", "fail", b_gzip_read("X", _cls), c_gzip_read, fail=_cls)
add("gzip_index/fail_invalid", "gzip_index", "fail", invalid_of(b_gzip_index("X")),
    c_one_array_without_the_other("flate_hip_gzip_index"), fail="invalid")
add("gzip_read/fail_invalid", "gzip_read", "fail", invalid_of(b_gzip_read("X")),
    c_flags_refused("flate_hip_gzip_read", lambda k: (k[2].ctypes.data, 64, C.byref(k[0]), None, None, None)), fail="invalid")


# ---- one long stream ----

ONE_TEXT = {"X": (9000, 21), "big": (45000, 22)}
_one_cache = {}


def one_stream(role):
    """(raw, plain, Walk).  The dirty twin: another text, cut where it has the unit count of X and another size in every
    unit."""
    if role in _one_cache:
        return _one_cache[role]
    if role != "dirty":
        n, seed = ONE_TEXT[role]
        plain = gz.text(n, seed=seed)
        raw = one_ref.deflate(plain, 6, mem=1)
        res = (raw, plain, one_ref.Walk(raw))
    else:
        wx, res = one_stream("X")[2], None
        for seed in (23, 24, 25, 26, 27):
            for n in range(8000, 11000, 150):
                plain = gz.text(n, seed=seed)
                raw = one_ref.deflate(plain, 6, mem=1)
                w = one_ref.Walk(raw)
                if w.n_units == wx.n_units and len(sk.points(w.out_off, one_span())) == len(sk.points(wx.out_off, one_span())) \
                        and all(a != b for a, b in zip(lens_of(w.out_off), lens_of(wx.out_off))) and \
                        all(a != b for a, b in zip(w.unit_bit[1:], wx.unit_bit[1:])) and \
                        all(a != b for a, b in zip(w.out_off[1:], wx.out_off[1:])):
                    res = (raw, plain, w)
                    break
            if res:
                break
        assert res, "no dirty twin of the one-stream scenario found"
    _one_cache[role] = res
    return res


def one_spoiled(role, spoil):
    """(raw, plain, Walk) of a stream that fails in a middle unit."""
    raw, plain, w = one_stream(role)
    if spoil == "corrupt":   # unit 3 starts with a block of the reserved type
        bit = w.unit_bit[3] + 1
        raw = raw[:bit >> 3] + bytes([raw[bit >> 3] | 1 << (bit & 7)]) + raw[(bit >> 3) + 1:]
    elif spoil == "eof":
        raw = raw[:(w.unit_bit[4] + w.unit_bit[5]) // 16]
    return raw, plain, one_ref.Walk(raw)


KIND = {"gzip": one_ref.GZIP, "zlib": one_ref.ZLIB}


def b_one_index(role, wrap="gzip", spoil=None):
    def build(o):
        raw, plain, w = one_spoiled(role, spoil)
        f = one_ref.wrap(raw, plain, KIND[wrap])
        exp = (w.status, w.n_units, w.out_bytes, True, w.status, w.err_off, T(w.unit_bit), T(w.out_off))
        cap = None
        if spoil == "index_cap":
            cap, exp = w.n_units, (OUT_TOO_SMALL, w.n_units, w.out_bytes, True, 0, -1, None, None)
        return dict(data=arr(f), n=len(f), wrap=wrap, cap=cap, expected=exp,
                    proof=[(len(zlib.decompress(raw, -15)), w.out_bytes)] if not w.status else [],
                    meta=meta((w.n_units,), [lens_of(w.unit_bit), lens_of(w.out_off)], [w.unit_bit[1:], w.out_off[1:]]))
    return build


def c_one_index(eng, d, device):
    with Rc(eng) as r:
        ix = eng.inflate_one_index(view(dev(d["data"], device), d["n"]), d["wrap"], index_cap=d["cap"])
    return (r.rc, ix.n_units, ix.out_bytes, ix.n_candidates >= ix.n_units, ix.status, ix.err_off, T(ix.unit_bit),
            T(ix.out_off))


def b_one(role, wrap="gzip", spoil=None):
    def build(o):
        raw, plain, w = one_spoiled(role, spoil)
        f = one_ref.wrap(raw, plain, KIND[wrap])
        got = plain[:w.out_len]
        exp = (w.status, w.out_len, w.status, w.err_off, w.n_units, True, got)
        cap = len(plain)
        if role == "dirty" or spoil == "trailer":   # a trailer that does not match: -4 at in_len, everything delivered
            f = flip(f, len(f) - (8 if wrap == "gzip" else 4) + 1)
            exp = (CORRUPT, len(plain), CORRUPT, len(f), w.n_units, True, plain)
        if spoil == "capacity":
            cap, exp = cap - 1, (OUT_TOO_SMALL, len(plain), None, None, w.n_units, True, b"")
        return dict(data=arr(f), n=len(f), wrap=wrap, cap=cap, blank=[], expected=exp,
                    proof=[(zlib.decompress(raw, -15), plain)] if not w.status else [],
                    meta=meta((w.n_units,), [lens_of(w.unit_bit), lens_of(w.out_off)], [w.unit_bit[1:], w.out_off[1:]],
                              [exp[2] or 0]))
    return build


def c_one(eng, d, device):
    with Rc(eng) as r:
        out, q = eng.inflate_one(view(dev(d["data"], device), d["n"]), d["wrap"], out=own_out(d, device, d["cap"]),
                                 out_cap=d["cap"])
    if q.rc == OUT_TOO_SMALL and q.out_len > d["cap"]:
        return (r.rc, q.out_len, None, None, q.n_units, q.n_candidates >= q.n_units, b"")
    return (r.rc, q.out_len, q.status, q.err_off, q.n_units, q.n_candidates >= q.n_units, read_bytes(out, q.out_len, d))


def c_one_bad_wrap(eng, d, device):
    x = view(dev(d["data"], device), d["n"])
    ol, st = C.c_uint64(0), C.c_int32(0)
    return (int(eng._L.flate_hip_inflate_one(eng._ctx, x.data_ptr() if device else x.ctypes.data, d["n"], 3, None, 0,
                                             C.byref(ol), C.byref(st), None, None, None, DEVICE_PTRS if device else 0)),)


twins("inflate_one_index", {r: b_one_index(r) for r in ("X", "dirty", "big")}, c_one_index)
twins("inflate_one", {r: b_one(r) for r in ("X", "dirty", "big")}, c_one)
add("inflate_one_index/zlib", "inflate_one_index", "more", b_one_index("X", "zlib"), c_one_index)
add("inflate_one/zlib", "inflate_one", "more", b_one("X", "zlib"), c_one)
for _cls in ("corrupt", "eof", "index_cap"):
    add("inflate_one_index/fail_" + _cls, "inflate_one_index", "fail", b_one_index("X", "gzip", _cls), c_one_index, fail=_cls)
for _cls in ("corrupt", "eof", "capacity"):
    add("inflate_one/fail_" + _cls, "inflate_one", "fail", b_one("X", "gzip", _cls), c_one, fail=_cls)
add("inflate_one/fail_invalid", "inflate_one", "fail", invalid_of(b_one("X")), c_one_bad_wrap, fail="invalid")


def one_span():
    """A seek point per quarter of what X inflates to, in every scenario: the twins' point counts follow their sizes."""
    return one_stream("X")[2].out_off[-1] // 4


def b_seek_index(role, spoil=None):
    def build(o):
        raw, plain, w = one_spoiled(role, spoil)
        f = one_ref.wrap(raw, plain, one_ref.GZIP)
        span = one_span()
        if w.status:   # a stream that fails has no index
            exp = (w.status, None, b"", w.status, w.err_off)
            return dict(data=arr(f), n=len(f), span=span, expected=exp, proof=[], meta=None)
        words = sk.index_words(w, plain, len(raw), one_ref.GZIP, span)
        pts = sk.points(w.out_off, span)
        assert len(pts) >= 3
        wins = sk.windows(plain, w.out_off, pts)
        exp = (0, T(words), wins, w.n_units, len(pts), len(plain), 0, -1)
        return dict(data=arr(f), n=len(f), span=span, expected=exp, proof=[(zlib.decompress(raw, -15), plain)],
                    meta=meta((w.n_units, len(pts)), [lens_of(w.unit_bit), lens_of(w.out_off)], [w.unit_bit[1:], w.out_off[1:]]))
    return build


def c_seek_index(eng, d, device):
    with Rc(eng) as r:
        s = eng.inflate_one_seek_index(view(dev(d["data"], device), d["n"]), "gzip", d["span"])
    if s.rc:
        return (r.rc, T(s.index), B(s.windows), s.status, s.err_off)
    return (r.rc, T(s.index), B(s.windows), s.n_units, s.n_points, s.out_bytes, s.status, s.err_off)


def b_seek_ranges(role, spoil=None):
    def build(o):
        raw, plain, w = one_stream(role)
        f = one_ref.wrap(raw, plain, one_ref.GZIP)
        span = one_span()
        words = np.array(sk.index_words(w, plain, len(raw), one_ref.GZIP, span), np.uint64)
        pts = sk.points(w.out_off, span)
        wins = sk.windows(plain, w.out_off, pts)
        rs = sk.edge_ranges(w.out_off, pts)
        if role == "big":
            wx = one_stream("X")[2]
            rs = rs[:4 * len(sk.edge_ranges(wx.out_off, sk.points(wx.out_off, span)))]
        if spoil == "invalid":
            rs = [(5, 4)]
        begin, end = [a for a, _ in rs], [b for _, b in rs]
        d = dict(data=arr(f), n=len(f), words=words, wins=arr(wins, 0), begin=begin, end=end, blank=[],
                 proof=[(zlib.decompress(raw, -15), plain)],
                 meta=meta((w.n_units, len(pts)), [lens_of(w.unit_bit), lens_of(w.out_off)], [w.unit_bit[1:], w.out_off[1:]]))
        if spoil == "invalid":
            return dict(d, cap=64, expected=(INVALID,))
        same = not (role == "dirty" or spoil == "corrupt")
        if not same:   # not the stream the index was built from: the trailer says so, every range -4
            f2 = one_ref.wrap(raw, plain[:-1] + bytes([plain[-1] ^ 1]), one_ref.GZIP)
            assert len(f2) == len(f)
            d["data"], d["proof"] = arr(f2), []
            d["meta"]["status"] = [CORRUPT]
        else:
            d["meta"]["status"] = [0]
        rc, off, st, nd, bad, data = sk.read(plain, w.out_off, pts, begin, end, same_stream=same)
        cap = off[-1]
        exp = (rc, T(off), T(st), nd, bad, b"".join(x for x in data if x is not None))
        if spoil == "capacity":
            cap -= 1
            rc, off, st, nd, bad, data = sk.read(plain, w.out_off, pts, begin, end, out_cap=cap)
            exp = (rc, T(off), None, None, None, b"")
        return dict(d, cap=cap, expected=exp)
    return build


def c_seek_ranges(eng, d, device):
    x, wins = view(dev(d["data"], device), d["n"]), dev(d["wins"], device)
    if d["expected"] == (INVALID,):
        return (refused(eng, lambda: eng.inflate_one_ranges(x, (d["words"], wins), d["begin"], d["end"],
                                                            out=own_out(d, device, 64))[1].rc),)
    with Rc(eng) as r:
        out, q = eng.inflate_one_ranges(x, (d["words"], wins), d["begin"], d["end"], out=own_out(d, device, d["cap"]),
                                        out_cap=d["cap"])
    if int(q.out_off[-1]) > d["cap"]:
        return (r.rc, T(q.out_off), None, None, None, b"")
    return (r.rc, T(q.out_off), T(q.range_status), q.n_decoded, q.bad_unit, read_bytes(out, int(q.out_off[-1]), d))


twins("seek_index", {r: b_seek_index(r) for r in ("X", "dirty", "big")}, c_seek_index)


def b_seek_index_short(spoil):
    def build(o):
        d = dict(b_seek_index("X")(o))
        _, words, wins, n_units, n_points, out_bytes, _, _ = d["expected"]
        counts = (len(words), len(wins), n_units, n_points, out_bytes, 0)
        d["words"], d["room"], d["wrap"] = len(words), len(wins), one_ref.GZIP
        if spoil == "index_cap":
            d["words"] -= 1
        elif spoil == "capacity":
            d["room"] -= 1
        else:
            d["wrap"] = 3
        d["expected"], d["proof"] = ((INVALID,) if spoil == "invalid" else (OUT_TOO_SMALL,) + counts), []
        return d
    return build


def c_seek_index_abi(eng, d, device):
    """flate_hip_inflate_one_seek_index itself (the wrapper sizes both arrays and retries): the counts of a build whose
    index or windows do not fit; nothing is written."""
    x = view(dev(d["data"], device), d["n"])
    index, wins = np.zeros(d["words"] + 1, np.uint64), dev(np.zeros(d["room"] + 1, np.uint8), device)
    iw, wb, nu, npt = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    ob, st = C.c_uint64(0), C.c_int32(0)
    rc = eng._L.flate_hip_inflate_one_seek_index(
        eng._ctx, x.data_ptr() if device else x.ctypes.data, d["n"], d["wrap"], d["span"], index.ctypes.data, d["words"],
        C.byref(iw), wins.data_ptr() if device else wins.ctypes.data, d["room"], C.byref(wb), C.byref(nu), C.byref(npt),
        C.byref(ob), None, C.byref(st), None, DEVICE_PTRS if device else 0)
    if rc == INVALID:
        return (INVALID,)
    return (int(rc), iw.value, wb.value, nu.value, npt.value, ob.value, st.value)


for _cls in ("index_cap", "capacity", "invalid"):
    add("seek_index/fail_" + _cls, "seek_index", "fail", b_seek_index_short(_cls), c_seek_index_abi, fail=_cls)
twins("seek_ranges", {r: b_seek_ranges(r) for r in ("X", "dirty", "big")}, c_seek_ranges)
for _cls in ("corrupt", "eof"):
    add("seek_index/fail_" + _cls, "seek_index", "fail", b_seek_index("X", _cls), c_seek_index, fail=_cls)
for _cls in ("corrupt", "capacity", "invalid"):
    add("seek_ranges/fail_" + _cls, "seek_ranges", "fail", b_seek_ranges("X", _cls), c_seek_ranges, fail=_cls)


# ---- a gzip file of any members ----

_gf_cache = {}


def gzfile_members(role):
    """[(member, plain)]: three_members() for X; the dirty twin has the same number of units in every member."""
    if role in _gf_cache:
        return _gf_cache[role]
    if role == "X":
        res = gf.three_members()
    elif role == "big":
        res = gf.phase_members()[:14]
    else:
        x = gf.three_members()
        wx = gf.Walk(b"".join(m for m, _ in x))
        want = wx.member_unit[2] - wx.member_unit[1]
        res = None
        for seed in (32, 33, 34, 35):
            t = gz.text(30000, seed=seed)
            for n in range(15000, 21000, 250):
                mid = t[2900:2900 + n]
                raw = one_ref.deflate(mid, 6, mem=1)
                if one_ref.Walk(raw).n_units != want:
                    continue
                ms = [(gz.member(t[:2900], 6, flg=gz.FNAME, name=b"1st"), t[:2900]), (gf.wrap(raw, mid), mid),
                      (gz.member(t[2900 + n:2900 + n + 8000], 9), t[2900 + n:2900 + n + 8000])]
                w = gf.Walk(b"".join(m for m, _ in ms))
                if w.member_unit == wx.member_unit and all(a != b for a, b in zip(lens_of(w.out_off), lens_of(wx.out_off))) \
                        and all(a != b for a, b in zip(w.unit_bit, wx.unit_bit)) and \
                        all(a != b for a, b in zip(w.out_off[1:], wx.out_off[1:])):
                    res = ms
                    break
            if res:
                break
        assert res, "no dirty twin of the gzip-file scenario found"
    _gf_cache[role] = res
    return res


def gzfile_bytes(role, spoil=None):
    ms = gzfile_members(role)
    f, plain = b"".join(m for m, _ in ms), b"".join(p for _, p in ms)
    w = gf.Walk(f)
    if spoil == "corrupt":   # the middle member's third unit starts with a block of the reserved type
        bit = w.unit_bit[w.member_unit[1] + 2] + 1
        f = f[:bit >> 3] + bytes([f[bit >> 3] | 1 << (bit & 7)]) + f[(bit >> 3) + 1:]
    if spoil == "eof":
        f = f[:w.member_off[2] + (len(f) - w.member_off[2]) // 2]
    return f, plain


def gf_meta(w, status=None):
    return meta((w.n_units, w.n_members), [lens_of(w.unit_bit), lens_of(w.out_off), lens_of(w.member_off)],
                [w.unit_bit, w.out_off[1:], w.member_off[1:]], status)


def b_gzfile_index(role, spoil=None):
    def build(o):
        f, plain = gzfile_bytes(role, spoil)
        w = gf.Walk(f)
        exp = (w.status,) + w.index_words() + (True, T(w.unit_bit), T(w.out_off), T(w.member_off), T(w.member_unit))
        cap = None
        if spoil == "index_cap":
            cap = w.n_units
            exp = (OUT_TOO_SMALL,) + w.index_words() + (True, None, None, T(w.member_off), T(w.member_unit))
        return dict(data=arr(f), n=len(f), cap=cap, expected=exp,
                    proof=[(sum(len(p) for p in gf.members_of(f)), w.out_bytes)] if not w.status else [], meta=gf_meta(w))
    return build


def c_gzfile_index(eng, d, device):
    with Rc(eng) as r:
        ix = eng.gzfile_index(view(dev(d["data"], device), d["n"]), index_cap=d["cap"])
    return (r.rc, ix.status, ix.n_units, ix.n_members, ix.out_bytes, ix.bad_member, ix.err_off, ix.stream_err_off,
            ix.n_candidates >= ix.n_units, T(ix.unit_bit), T(ix.out_off), T(ix.member_off), T(ix.member_unit))


def b_gzfile_read(role, spoil=None):
    def build(o):
        f, plain = gzfile_bytes(role, spoil)
        w = gf.Walk(f)
        verdict = (w.status, w.bad_member, w.err_off, w.stream_err_off)
        got = plain[:w.out_len]
        if role == "dirty" or spoil == "trailer":   # a wrong CRC-32 in member 1: -4, everything delivered
            f = flip(f, w.member_off[2] - 8, 0x40)
            verdict = (CORRUPT, 1, w.member_off[1], w.member_off[2] - w.member_off[1])
        exp = (verdict[0], len(got), w.n_members, w.n_units, True) + verdict + (got,)
        cap = len(plain)
        if spoil == "capacity":
            cap, exp = cap - 1, (OUT_TOO_SMALL, len(plain), w.n_members, w.n_units, True, None, None, None, None, b"")
        return dict(data=arr(f), n=len(f), cap=cap, blank=[], expected=exp,
                    proof=[(b"".join(gf.members_of(f)), plain)] if not verdict[0] else [],
                    meta=gf_meta(w, [verdict[0]]))
    return build


def c_gzfile_read(eng, d, device):
    with Rc(eng) as r:
        out, q = eng.gzfile_read(view(dev(d["data"], device), d["n"]), out=own_out(d, device, d["cap"]), out_cap=d["cap"])
    head = (r.rc, q.out_len, q.n_members, q.n_units, q.n_candidates >= q.n_units)
    if q.rc == OUT_TOO_SMALL and q.out_len > d["cap"]:
        return head + (None, None, None, None, b"")
    return head + (q.status, q.bad_member, q.err_off, q.stream_err_off, read_bytes(out, q.out_len, d))


def b_gzfile_tiny(o):
    f, plain = gf.tiny_file()
    w = gf.Walk(f)
    return dict(data=arr(f), n=len(f), cap=len(plain), blank=[], proof=[(b"".join(gf.members_of(f)), plain)], meta=None,
                expected=(0, len(plain), w.n_members, w.n_units, True, 0, NONE32, -1, -1, plain))


twins("gzfile_index", {r: b_gzfile_index(r) for r in ("X", "dirty", "big")}, c_gzfile_index)
twins("gzfile_read", {r: b_gzfile_read(r) for r in ("X", "dirty", "big")}, c_gzfile_read)
add("gzfile_read/tiny_file", "gzfile_read", "more", b_gzfile_tiny, c_gzfile_read)
for _cls in ("corrupt", "eof", "index_cap"):
    add("gzfile_index/fail_" + _cls, "gzfile_index", "fail", b_gzfile_index("X", _cls), c_gzfile_index, fail=_cls)
for _cls in ("corrupt", "eof", "capacity"):
    add("gzfile_read/fail_" + _cls, "gzfile_read", "fail", b_gzfile_read("X", _cls), c_gzfile_read, fail=_cls)
add("gzfile_read/fail_invalid", "gzfile_read", "fail", invalid_of(b_gzfile_read("X")),
    c_flags_refused("flate_hip_gzfile_read", lambda k: (k[2].ctypes.data, 64, C.byref(k[0]), None, None, None, C.byref(k[1]),
                                                        None, None, None)), fail="invalid")


# ---- ZIP ----

ZIP_ITEMS = {"X": [("a.txt", ("t", 3000, 1)), ("stored.bin", ("r", 400, 2)), ("empty", ("t", 0, 0)), ("dir/b.txt", ("t", 9000, 3)),
                   ("c", ("r", 70, 4))],
             "dirty": [("aa.txt", ("t", 2800, 5)), ("stored2.bin", ("r", 410, 6)), ("e", ("t", 7, 0)), ("dir/bb.txt", ("t", 9100, 7)),
                       ("cc", ("r", 0, 8))],
             "big": [("n%d" % k, ("tr"[k % 2], (911 * k) % 4000 if k % 5 else 0, 10 + k)) for k in range(20)]}


def zip_items(role):
    return [(name, (zip_ref._text if kind == "t" else zip_ref._rand)(n, seed)) for name, (kind, n, seed) in ZIP_ITEMS[role]]


def b_zip_write(role):
    def build(o):
        items = zip_items(role)
        datas = [d for _, d in items]
        raws = [o.deflate(np.frombuffer(d, np.uint8)) for d in datas]
        f, eoff = zip_ref.write_archive(raws, [n.encode() for n, _ in items], [zlib.crc32(d) for d in datas],
                                        [len(d) for d in datas])
        z = zipfile.ZipFile(io.BytesIO(f))
        off = cum([len(d) for d in datas])
        return dict(data=arr(b"".join(datas)), off=off, names=[n for n, _ in items], expected=(0, len(f), T(eoff), f),
                    proof=[([z.read(n) for n, _ in items], datas)],
                    meta=meta((len(items),), [lens_of(off), lens_of(eoff)], [off[1:], eoff[1:]]))
    return build


def c_zip_write(eng, d, device):
    with Rc(eng) as r:
        res = eng.zip_write(dev(d["data"], device), d["off"], d["names"], index=True)
    out, n, eoff = res if device else (res[0], len(res[0]), res[1])
    return (r.rc, n, T(eoff), B(out, n))


def zip_archive(role, spoil=None):
    """An archive zipfile wrote: deflated entries, the second one stored.  -> (archive, {bad entry: its Entry})."""
    items = zip_items(role)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k, (name, data) in enumerate(items):
            zi = zipfile.ZipInfo(name)
            zi.compress_type = zipfile.ZIP_STORED if k % 5 == 1 else zipfile.ZIP_DEFLATED
            z.writestr(zi, data, compresslevel=6)
    f = buf.getvalue()
    ix = zip_ref.Index(f)
    if role == "dirty" or spoil == "corrupt":   # entry 3's CRC-32 in the directory does not match its bytes
        f = flip(f, ix.entries[3].name_off - 46 + 16, 0x01)
    if spoil == "eof":   # entry 0's stream loses its end: the directory says so, the decoder finds it cut short
        e = ix.entries[0]
        at = e.name_off - 46
        f = f[:at + 20] + struct.pack("<I", e.comp_size - 4) + f[at + 24:]
    return f, items


def entries_tuple(entries):
    return tuple(tuple(int(getattr(e, k) if hasattr(e, "_fields") else e[k]) for k in zip_ref.Entry._fields) for e in entries)


def b_zip_index(role, spoil=None):
    def build(o):
        f, items = zip_archive(role)
        if spoil == "corrupt":   # the end record's directory offset points one byte off
            p = zip_ref.find_end(f)
            f = f[:p + 16] + struct.pack("<I", struct.unpack_from("<I", f, p + 16)[0] + 1) + f[p + 20:]
        ix = zip_ref.Index(f)
        if ix.rc:
            exp = (ix.rc, ix.n_entries, 0, ix.err_off, None, None, None)
        else:
            exp = (0, ix.n_entries, ix.out_bytes, -1, entries_tuple(ix.entries), T(ix.out_off),
                   tuple(n.decode() for n in ix.names))
        e = ix.entries
        return dict(data=arr(f), n=len(f), expected=exp,
                    proof=[(zipfile.ZipFile(io.BytesIO(f)).namelist(), [n for n, _ in items])] if not ix.rc else [],
                    meta=meta((len(e),), [[x.comp_size for x in e], [x.size for x in e]],
                              [[x.header_off for x in e][1:], ix.out_off[1:]]))
    return build


def c_zip_index(eng, d, device):
    with Rc(eng) as r:
        ix = eng.zip_index(view(dev(d["data"], device), d["n"]))
    return (r.rc, ix.n_entries, ix.out_bytes, ix.err_off,
            None if ix.entries is None else entries_tuple(ix.entries), T(ix.out_off),
            None if ix.names is None else tuple(ix.names))


def b_zip_read(role, select=None, spoil=None):
    def build(o):
        f, items = zip_archive(role, spoil)
        ix = zip_ref.Index(f)
        assert ix.rc == 0
        sel = list(range(ix.n_entries)) if select is None else select
        if spoil == "invalid":
            return dict(data=arr(f), n=len(f), select=[0, ix.n_entries], cap=64, blank=[], expected=(INVALID,), proof=[],
                        meta=None)
        res = [zip_ref.read_entry(f, ix.entries[j]) for j in sel]
        sizes = [ix.entries[j].size if ix.entries[j].status == 0 else 0 for j in sel]
        off = cum(sizes)
        spans = [(int(off[k]), int(off[k + 1])) for k, v in enumerate(res) if v[2] is None]
        body = b"".join(v[2] if v[2] is not None else bytes(sizes[k]) for k, v in enumerate(res))
        exp = (first_bad(v[0] for v in res), T(off), tuple(len(v[2]) if v[2] is not None else None for v in res),
               tuple(v[0] for v in res), tuple(v[1] for v in res), ix.n_entries, -1, body)
        cap = int(off[-1])
        if spoil == "capacity":
            cap, exp = cap - 1, (OUT_TOO_SMALL, T(off), None, None, None, ix.n_entries, -1, b"")
        z = zipfile.ZipFile(io.BytesIO(f))
        return dict(data=arr(f), n=len(f), select=select, cap=cap, blank=spans, expected=exp,
                    proof=[(z.read(z.infolist()[j]), v[2]) for j, v in zip(sel, res) if v[0] == 0],
                    meta=meta((len(sel),), [[ix.entries[j].comp_size for j in sel], sizes],
                              [[ix.entries[j].header_off for j in sel][1:], off[1:]], [v[0] for v in res]))
    return build


def c_zip_read(eng, d, device):
    x = view(dev(d["data"], device), d["n"])
    if d["expected"] == (INVALID,):
        return (refused(eng, lambda: eng.zip_read(x, select=d["select"], out=own_out(d, device, 64))[1].rc),)
    with Rc(eng) as r:
        out, q = eng.zip_read(x, select=d["select"], out=own_out(d, device, d["cap"]), out_cap=d["cap"])
    if int(q.out_off[-1]) > d["cap"]:
        return (r.rc, T(q.out_off), None, None, None, q.n_entries, q.archive_err_off, b"")
    want = d["expected"]
    olen = tuple(int(v) if want[2][k] is not None else None for k, v in enumerate(q.out_len))   # (unspecified where the decoder failed)
    err = tuple(int(v) if want[4][k] is not None else None for k, v in enumerate(q.err_off))
    return (r.rc, T(q.out_off), olen, T(q.status), err, q.n_entries, q.archive_err_off,
            read_bytes(out, int(q.out_off[-1]), d))


twins("zip_write", {r: b_zip_write(r) for r in ZIP_ITEMS}, c_zip_write)
twins("zip_index", {r: b_zip_index(r) for r in ZIP_ITEMS}, c_zip_index)
twins("zip_read", {r: b_zip_read(r) for r in ZIP_ITEMS}, c_zip_read)
add("zip_read/selection", "zip_read", "more", b_zip_read("X", [4, 1, 1, 2, 0]), c_zip_read)
def b_zip_index_short(spoil):
    def build(o):
        d = dict(b_zip_index("X")(o))
        ix = zip_ref.Index(bytes(d["data"][:d["n"]]))
        d["expected"], d["proof"] = ((INVALID,) if spoil == "invalid" else (OUT_TOO_SMALL, ix.n_entries, ix.out_bytes)), []
        d["cap"], d["both"] = ix.n_entries - 1, spoil != "invalid"
        return d
    return build


def c_zip_index_abi(eng, d, device):
    """flate_hip_zip_index itself (the wrapper sizes the arrays from a count): arrays one entry short, or one array
    without the other."""
    x = view(dev(d["data"], device), d["n"])
    ent, ooff = np.zeros(d["cap"] + 1, engine.ZIP_ENTRY), np.zeros(d["cap"] + 2, np.uint64)
    ne, ob = C.c_uint32(0), C.c_uint64(0)
    rc = eng._L.flate_hip_zip_index(eng._ctx, x.data_ptr() if device else x.ctypes.data, d["n"], d["cap"], ent.ctypes.data,
                                    ooff.ctypes.data if d["both"] else None, C.byref(ne), C.byref(ob), None,
                                    DEVICE_PTRS if device else 0)
    return (INVALID,) if rc == INVALID else (int(rc), ne.value, ob.value)


for _cls in ("index_cap", "invalid"):
    add("zip_index/fail_" + _cls, "zip_index", "fail", b_zip_index_short(_cls), c_zip_index_abi, fail=_cls)
add("zip_index/fail_corrupt", "zip_index", "fail", b_zip_index("X", "corrupt"), c_zip_index, fail="corrupt")
for _cls in ("corrupt", "eof", "capacity", "invalid"):
    add("zip_read/fail_" + _cls, "zip_read", "fail", b_zip_read("X", None, _cls), c_zip_read, fail=_cls)


# ---- what the tests ask the table ----

# The read families: the calls that decode.  Each has a scenario of every failure class that can exist for it; the
# index calls have the classes an index has.
READ_FAMILIES = ["inflate_batch", "inflate_batch_dict", "inflate_sizes", "inflate_framed_zlib", "inflate_framed_gzip",
                 "inflate_spliced", "inflate_spliced_zlib", "inflate_spliced_gzip", "bgzf_read", "bgzf_ranges_bytes",
                 "bgzf_ranges_virtual", "gzip_read", "inflate_one", "seek_ranges", "gzfile_read", "zip_read"]
INDEX_FAMILIES = ["bgzf_index", "gzip_index", "inflate_one_index", "seek_index", "gzfile_index", "zip_index"]
READ_CLASSES = ("corrupt", "eof", "capacity", "invalid")
INDEX_CLASSES = ("corrupt", "index_cap")
# (family, class) pairs that cannot exist, each with its reason; nothing else may be missing
IMPOSSIBLE = {
    ("inflate_sizes", "capacity"): "the size-only pass has no output and no slots",
    ("seek_ranges", "eof"): "the index pins in_len, the raw stream's end and every unit's end bit, and the trailer must "
                            "match: a stream that ends early is refused as not the index's (the corrupt and the "
                            "invalid scenario), it never reaches a decoder that could run out of input",
}
# Families whose calls have no per-item verdict word at all, or none that a CPU reference states: the dirty twin differs
# in sizes and offsets only.
NO_STATUS = {f for f, v in FAMILIES.items() if f.startswith(("deflate_", "lz77", "checksum", "bgzf_write", "bgzf_index",
                                                            "gzip_index", "inflate_one_index", "seek_index",
                                                            "gzfile_index", "zip_write", "zip_index"))}
GOOD = [s for s in TABLE if s.role in ("X", "more")]
FAILS = [s for s in TABLE if s.fail]
BY_NAME = {s.name: s for s in TABLE}
assert len(BY_NAME) == len(TABLE)


# ---- seeded walks (3e) ----

SEEDS = (101, 202, 303)
WALK_LEN = 120
# The decoder configurations come last and are not undone: the library has no getter for the five "inflate_*" options
# they set, and a walk's engine ends with the walk.  The other options go back to the defaults the header documents.
OPTION_STEPS = [("one_round_units", 4), ("one_round_units", 4096), ("entropy_per_block", 0), ("entropy_per_block", 1),
                ("entropy_per_block", -1), ("gzip_member_max", 1 << 20), ("gzip_member_max", gz.MEMBER_MAX),
                ("inflate_config", "lane_per_stream"), ("inflate_config", "speculative_wave_small_batch")]
OPTION_DEFAULTS = {"one_round_units": 4096, "entropy_per_block": -1, "gzip_member_max": gz.MEMBER_MAX}
# the scenarios whose calls read an option: each runs directly behind every step of that option
OPTION_READERS = {"one_round_units": ["inflate_one/x", "gzfile_read/x", "seek_index/x", "seek_ranges/x"],
                  "entropy_per_block": ["deflate_batch/x", "deflate_framed_gzip/x", "zip_write/x", "bgzf_write/x"],
                  "gzip_member_max": ["gzip_index/x", "gzip_read/x"],
                  "inflate_config": ["inflate_batch/x", "inflate_framed_gzip/x", "inflate_spliced/x", "zip_read/x", "bgzf_read/x"]}


def apply_option(eng, name, value):
    """One option step of a walk.  "inflate_config": one of util.INFLATE_CONFIGS."""
    from util import force_inflate_config
    if name == "inflate_config":
        force_inflate_config(eng, value)
    else:
        eng.set_option(name, value)


def walk(seed, n_calls=WALK_LEN):
    """[("call", scenario name, device) | ("option", name, value)]: at least n_calls calls drawn from the table -- a
    shuffle of the whole table, so that a seed meets every scenario in an order of its own -- with the option steps at
    drawn places, in their order, each followed at once by the scenarios that read the option."""
    rng = np.random.default_rng(seed)
    names = [s.name for s in TABLE]
    order = []
    while len(order) < max(n_calls, len(names)):
        order += [names[i] for i in rng.permutation(len(names))]
    steps = [("call", name, bool(rng.integers(2))) for name in order[:max(n_calls, len(names))]]
    at = sorted(int(x) for x in rng.choice(np.arange(5, len(steps) - 5), len(OPTION_STEPS), replace=False))
    for k, pos in reversed(list(enumerate(at))):
        name, value = OPTION_STEPS[k]
        readers = [("call", r, bool(rng.integers(2))) for r in OPTION_READERS[name]]
        steps[pos:pos] = [("option", name, value)] + readers
    return steps
