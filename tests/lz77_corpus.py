"""Input BYTES that drive the match finder (lz77_stream, moonbit-flate_amd/csrc/lz77_kernels.hip) to the edges of its
hand-written machinery, and the rules that say which edge a case reached.

As tests/encode_corpus.py: a case is input data from a seeded generator and never states expected tokens; the
oracle (oracle/pyoracle.py, DeflateFast) is the only judge of those.  What a case is FOR is stated as a rule, and
every rule is detected from the oracle's tokens or from the counters and the event log of the extended host model
(tests/host_model/lz77_wave_model.cpp, model_lz77_ex: 16-bit modular slots, sweeps, the span cut and a shadow table
of absolute positions), never assumed from the generator.  REQUIRED_RULES names one witness case per rule;
tests/test_lz77_corpus.py fails when a witness does not reach its rule.

How a plant is made visible (deflate-fast.mbt:123-270): a position is entered in the table only when the scan
visits it, and after 32 misses the scan's stride grows, so incompressible filler skips planted bytes.  A run of one
byte value in front of a plant makes the scan dense again: the run's matches chain to its last byte, and the
position behind it is probed and inserted.  Its length is 3 x stride + 600 with stride = (positions since the last
match) / 32.  Whether a slot SURVIVED from a plant to its lookup is never assumed either: the generators ask the
model's shadow table (the LOG_OLD entries carry the slot's true age) and move to the next seed if it did not.

Edges that input bytes cannot reach, so no rule asks for them and the mutants that differ only there are listed
in EQUIVALENT_MUTANTS with the reasoning:
 * a candidate at W-5 .. W-1 of the previous window (the default mode's `cand + 4 < W` at its own edge): a window
   of n bytes inserts positions p with p + 1 <= s_limit = n - 15 only, so the last position a table slot can name is
   W - 16 of the window before, and `cand + 4 < W` and `cand < W` agree on every candidate there is.  The corpus
   plants candidates at W-16 (the last one possible) and W-17 instead.
 * `dist != 0` in the MULTI builds: a slot reads as distance 0 only if it names a position exactly 65536 behind
   the lookup, and no slot gets that old -- a sweep every kSweepEvery = 20480 positions turns everything older than
   32768 into a marker that is 36864 .. 36864 + 20480 + 4096 + 63 < 65536 behind every lookup before the next
   sweep.  The single-window builds' form of the same test (`old != 0`, the empty slot) is reachable and is covered.
"""
import ctypes as C
import os
import subprocess

import numpy as np

W = 65535
MOONBIT, GO = 0, 1
BOTH = (MOONBIT, GO)
K_SWEEP, K_SPAN, K_MARKER = 20480, 4096, 36864

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_SRC = os.path.join(HERE, "host_model", "lz77_wave_model.cpp")

# the model's stats_out (enum in lz77_wave_model.cpp)
(S_DENSE, S_SPARSE, S_EVENTS, S_DUP_EVALS, S_DISCARDED, S_SHADOW_DISAGREE, S_SWEEP_DENSE, S_SWEEP_SPARSE,
 S_SWEEP_FIRST_BATCH, S_SPAN_CUTS, S_MARKER_LOOKUPS, S_MARKER_MIN_DIST, S_MARKER_MAX_DIST, S_AGE_32768, S_AGE_32769,
 S_LIVE_OLD, S_REPLAYS, S_TAG_SKIPS, S_LOG_LOST, S_FAST, S_GENERAL, S_SPARSE_EVENTS, S_LOOKUPS, S_LOG_COUNT) = range(24)
NUM_STATS = 32
# the model's log kinds
(LOG_OLD, LOG_SWEEP, LOG_MATCH, LOG_SPANCUT, LOG_GROUP, LOG_REPLAY, LOG_SCAN_END, LOG_NEXT, LOG_TAG,
 LOG_GROUP_JUDGE) = range(1, 11)
PATH_FAST, PATH_GENERAL, PATH_SPARSE = 0, 1, 2

MUTANTS = {
    1: "in-range test dist < 32768",
    2: "in-range test dist <= 32769",
    3: "no sweep",
    4: "marker 32768 behind the sweep point",
    5: "no span cut",
    6: "dist != 0 / old != 0 test dropped",
    7: "same-slot group: earliest inserted member instead of the latest",
    8: "dense commit in reversed order",
    9: "sparse replay skipped",
    10: "have <= 16 takes the short path",
    11: "length cap 257",
    12: "length cap 259",
    13: "s_limit + 1",
    14: "s_limit - 1",
    15: "dense -> sparse hand-over at probe 48",
    16: "cand + 4 < W -> cand < W",
    17: "tag compare inverted for tag value 2",
}
# (see the module docstring: no input reaches the difference)
EQUIVALENT_MUTANTS = {
    16: "a table slot never names a position later than W - 16 of the previous window (s_limit = n - 15)",
}


def lz_chunks(n):
    """(start, length) of the windows that go through DeflateFast::encode (engine.lz_chunks restated)."""
    full, r = divmod(int(n), W)
    return [(i * W, W) for i in range(full)] + ([(full * W, r)] if r >= 128 else [])


# ---------------------------------------------------------------------------------------------------------------
# (a) the host model and the oracle

_models = {}


def model_lib(mutant=0):
    """The host model, built on demand (one shared library per mutant, beside the source)."""
    if mutant not in _models:
        lib = os.path.join(HERE, "host_model", "liblz77_wave_model%s.so" % ("_m%d" % mutant if mutant else ""))
        if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(MODEL_SRC):
            tmp = "%s.%d.tmp" % (lib, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DLZ_MODEL_MUTANT=%d" % mutant,
                                   MODEL_SRC, "-o", tmp])
            os.replace(tmp, lib)
        L = C.CDLL(lib)
        L.model_lz77_ex.argtypes = [C.c_void_p, C.c_uint64, C.c_int] + [C.c_void_p] * 5 + [C.c_uint32]
        L.model_lz77_ex.restype = C.c_int
        assert L.model_lz77_mutant() == mutant
        _models[mutant] = L
    return _models[mutant]


def tokens_from_matches(chunk, pos, tok):
    """engine.tokens_from_matches restated (this module needs no built library)."""
    n = chunk.size
    pos = pos.astype(np.int64)
    lens = ((tok >> 22) & 0xFF).astype(np.int64) + 3
    covered = np.zeros(n + 1, dtype=np.int64)
    np.add.at(covered, pos, 1)
    np.add.at(covered, np.minimum(pos + lens, n), -1)
    inside = np.cumsum(covered[:n]) > 0
    is_start = np.zeros(n, dtype=bool)
    is_start[pos] = True
    vals = chunk.astype(np.uint32)
    vals[pos] = tok
    return vals[(~inside) | is_start]


class Run:
    """One run of the model: tokens per chunk, stats, log (rows {kind, pos, a, b, c, d}), posmap."""


def run_model(data, go=False, tags=False, multi=False, mutant=0, log=True):
    sb = np.frombuffer(bytes(data), np.uint8)
    chunks = lz_chunks(sb.size)
    nch = max(len(chunks), 1)
    pad = np.concatenate([np.zeros(64, np.uint8), sb, np.zeros(64, np.uint8)])
    recs = np.zeros((nch * 16384, 2), np.uint32)
    nm = np.zeros(nch, np.uint32)
    stats = np.zeros(NUM_STATS, np.uint64)
    cap = 1 << 16 if log else 0
    lg = np.zeros((cap + 1, 6), np.uint32)
    posmap = np.zeros(sb.size + 64, np.uint8)
    flags = (1 if go else 0) | (2 if tags else 0) | (4 if multi else 0)
    got = model_lib(mutant).model_lz77_ex(pad.ctypes.data + 64, sb.size, flags, recs.ctypes.data, nm.ctypes.data,
                                          stats.ctypes.data, posmap.ctypes.data, lg.ctypes.data if log else None, cap)
    assert got == len(chunks)
    r = Run()
    r.tokens = []
    for k, (start, cn) in enumerate(chunks):
        rr = recs[k * 16384:k * 16384 + int(nm[k])]
        r.tokens.append(tokens_from_matches(sb[start:start + cn], rr[:, 0], rr[:, 1]))
    r.stats = stats.astype(np.int64)
    r.log = lg[:int(stats[S_LOG_COUNT])].astype(np.int64)
    r.log[:, 4] = r.log[:, 4].astype(np.int32)   # (the probe index may be -1)
    r.posmap = posmap[:sb.size]
    return r


def oracle_tokens(oracle, data, go):
    df = oracle.DeflateFast(GO if go else MOONBIT)
    sb = np.frombuffer(bytes(data), np.uint8)
    return [df.encode(sb[s:s + n]) for s, n in lz_chunks(sb.size)]


def matches_of(tokens, data_len):
    """The oracle's matches as rows (absolute position, length, distance)."""
    rows = []
    for (start, _), t in zip(lz_chunks(data_len), tokens):
        t = t.astype(np.int64)
        m = (t >> 30) == 1
        ln = np.where(m, ((t >> 22) & 0xFF) + 3, 1)
        pos = np.cumsum(ln) - ln + start
        rows.append(np.stack([pos[m], ln[m], (t[m] & 0x3FFFFF) + 1], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)


def same_tokens(a, b):
    return len(a) == len(b) and all(x.size == y.size and bool((x == y).all()) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------
# (b) building blocks

def scan_table():
    """Offset of probe e of a scan from its first probe (deflate-fast.mbt:178-187: step = skip >> 5)."""
    tab, skip, pos = [], 32, 0
    while pos <= 65535:
        tab.append(pos)
        st = skip >> 5
        pos += st
        skip += st
    return tab


SCAN = scan_table()


def lead_len(since):
    return 3 * (since // 32 + 1) + 600


class Buf:
    """Random (incompressible) bytes with plants written over them."""

    def __init__(self, n, seed):
        self.rng = np.random.default_rng(seed)
        self.a = self.rng.integers(0, 256, n, dtype=np.uint8)

    def key(self, n, avoid=()):
        while True:
            k = self.rng.integers(0, 256, n, dtype=np.uint8)
            if k[0] not in avoid and len(set(k[:4].tolist())) == min(4, n):
                return k

    def put(self, p, b):
        b = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
        self.a[p:p + b.size] = b
        return p + b.size

    def lead_in(self, p, byte, since):
        """A run of `byte` that ends exactly at p; the bytes around it are not `byte`."""
        n = min(lead_len(since), p)
        self.a[p - n:p] = byte
        if p - n > 0 and self.a[p - n - 1] == byte:
            self.a[p - n - 1] ^= 0x55
        return n

    def bytes(self):
        return self.a.tobytes()


def hash4(u):
    return ((int(u) * 0x1e35a7bd) & 0xFFFFFFFF) >> 18


def tag_of(u):
    return (((int(u) * 0x1e35a7bd) & 0xFFFFFFFF) >> 16) & 3


def colliding_pair(seed, same_tag):
    """Two different four-byte values with one table slot (brute force over hash4), their tags equal or not; the
    bytes of each all different, and none of them 0 or 255 (the run bytes of the generators)."""
    rng = np.random.default_rng(seed)
    while True:
        v = rng.integers(1, 255, (1 << 18, 4), dtype=np.uint8)
        u32 = v.view("<u4").ravel()
        prod = (u32.astype(np.uint64) * 0x1e35a7bd) & 0xFFFFFFFF
        h, t = prod >> 18, (prod >> 16) & 3
        order = np.argsort(h, kind="stable")
        hs = h[order]
        for i in np.nonzero(hs[1:] == hs[:-1])[0]:
            a, b = order[i], order[i + 1]
            if hs[i] not in (hash4(0), hash4(0xFFFFFFFF)) and (t[a] == t[b]) == same_tag and len(set(v[a].tolist())) == 4 and len(set(v[b].tolist())) == 4 \
                    and u32[a] != u32[b] and not set(v[a].tolist()) & set(v[b].tolist()):
                return v[a].copy(), v[b].copy()


# ---------------------------------------------------------------------------------------------------------------
# (c) the cases.  Every generator returns [(name, bytes)].

LADDER_D = [4, 5, 32767, 32768, 32769, 36863, 36864, 36865, 32768 + 20480 - 1, 32768 + 20480,
            32768 + 20480 + 4096 + 63, 57408, 61503, 65535, 65536, 65537, 98304]
PHASES = [0, 1, 20479, 9973]
RUN_A, RUN_B = 0, 255      # the bytes of the lead-in runs; keys and collision pairs avoid them
TAIL = 700                 # filler behind the last plant


def _ladder_geometry(d, phase, win):
    """p (first plant, p mod kSweepEvery == phase) and q = p + d in window `win`, both lead-ins inside the stream
    and the second one inside window `win`; None if no p fits."""
    for p in range(phase, 3 * W, K_SWEEP):
        q = p + d
        if q >= (win + 1) * W - TAIL:
            return None
        if p < lead_len(p % W) + 8 and p < 700:
            continue
        since = q - max(win * W, p + 24) if d > 64 else 0
        if q - lead_len(since) < win * W + 8 or (d > 64 and q - lead_len(since) < p + 40):
            continue
        return p, q, since
    return None


def ladder_stream(d, phase, win, seed, bait_k=None):
    """Key at p and again at p + d.  bait_k: the alias-bait form -- the second copy lies UNSCANNED in sparse filler
    and the lookup is a third copy at p + d + bait_k (d = 65536)."""
    g = _ladder_geometry(d, phase, win)
    if g is None:
        return None
    p, q, since = g
    look = q if bait_k is None else q + bait_k
    b = Buf(look + TAIL, seed)
    key = b.key(24, avoid=(RUN_A, RUN_B))
    b.lead_in(p, RUN_A, p % W)
    b.put(p, key[:min(24, d)])
    if bait_k is None:
        if d > 64:
            b.lead_in(q, RUN_B, since)
        b.put(q, key)
    else:
        # the lookup first (its lead-in may cover q for a small k), then the bait over it
        n = b.lead_in(look, RUN_B, look - max((look // W) * W, p + 24))
        b.put(look, key)
        if look - n <= q + 4:   # bait inside the lead-in: only four equal bytes can be both (see alias_bait)
            return None
        b.put(q, key[:4])
    return b.bytes(), p, q, look


def gen_ladder():
    out = []
    for d in LADDER_D:
        for win in (0, 1, 2):
            for phase in PHASES:
                for seed in range(40):
                    r = ladder_stream(d, phase, win, 1000 + seed)
                    if r is None:
                        break
                    data, p, q, _ = r
                    m = run_model(data, multi=True)
                    lg = m.log
                    hit = lg[(lg[:, 0] == LOG_OLD) & (lg[:, 1] == q) & (lg[:, 2] == d)]
                    if d >= 32767 and not hit.size:
                        continue    # the slot did not survive from p to q, or q was not looked up: next seed
                    if not (m.posmap[p] & 1 and m.posmap[q] & 2):
                        continue
                    out.append(("ladder_d%d_ph%d_w%d" % (d, phase, win), data))
                    break
    return out


def gen_alias_bait():
    """As the ladder at d = 65536, with the second copy of the key (the bait, four bytes) UNSCANNED at p + 65536 in
    the middle of sparse filler -- the model's posmap confirms that it is never inserted -- and the lookup k behind
    it: a table that missed a sweep still holds p + 1 = (p + 65536) + 1 mod 2^16 and would report a match of distance
    k where the reference emits literals.  k = 32768: the lookup has a lead-in run of its own.  k = 1, 4, 300: a run
    would cover the bait, so the lookup is a probe of the sparse scan as the model reports it, and the bait lies
    between two probes.  k = 1: five equal bytes x, the first unscanned; the key planted at p is x x x x."""
    out = []
    for phase in (1, 9973):
        for win in (1, 2):
            for seed in range(60):
                r = ladder_stream(65536, phase, win, 2000 + seed, bait_k=32768)
                if r is None:
                    break
                data, p, q, look = r
                m = run_model(data, multi=True)
                lg = m.log
                hit = lg[(lg[:, 0] == LOG_OLD) & (lg[:, 1] == look) & (lg[:, 2] == 65536 + 32768)]
                if not hit.size or m.posmap[q] & 1 or not m.posmap[p] & 1:
                    continue
                out.append(("alias_k32768_ph%d_w%d" % (phase, win), data))
                break
    for k in (1, 4, 300):
        for seed in range(400):
            rng = np.random.default_rng(3000 + seed)
            p = int(rng.integers(2000, 20000))
            b = Buf(p + 65536 + 3000, 3000 + seed)
            x = 77
            key = np.full(4, x, np.uint8) if k == 1 else b.key(4, avoid=(RUN_A, RUN_B))
            b.lead_in(p, RUN_A, p)
            b.put(p, key)
            m = run_model(b.bytes(), multi=True)
            bait = p + 65536
            look = bait + k
            # the lookup must be a probe of the sparse scan as it is, the bait and what lies around it not
            if not m.posmap[look] & 1 or m.posmap[bait - 3:min(look, bait + 4)].any() or m.posmap[look + 1:look + 4].any():
                continue
            if k == 1:
                b.put(bait, np.full(5, x, np.uint8))
            else:
                b.put(bait, key)
                b.put(look, key)
            data = b.bytes()
            m = run_model(data, multi=True)
            lg = m.log
            hit = lg[(lg[:, 0] == LOG_OLD) & (lg[:, 1] == look) & (lg[:, 2] == 65536 + k)]
            if not hit.size or m.posmap[bait] & 1 or not m.posmap[look] & 1:
                continue
            out.append(("alias_k%d_sparse" % k, data))
            break
    return out


def gen_span_twin():
    """The span cut's twin of the alias bait.  Window 0 is one scan without a match.  Without the cut the sparse
    batches hold 64 probes each, [47 + 64 j, 47 + 64 j + 64); the first of them that starts at or behind kSweepEvery
    sweeps at its first probe R and then reaches far beyond R + 28672, where a marker (36864 behind R) reads as
    distance (q - R - 28672) mod 2^16: in range.  The bait: the four bytes of such a probe q copied to R + 28672,
    which no scan visits.  A table that sweeps that late has also kept the empty-table fill beyond its time (the fill
    is a marker 36864 behind position 0, so it reads as position 28672 from there on unless a sweep in front of 28672
    has replaced it): the same four bytes are planted at 28672 too, unscanned as well."""
    out = []
    fill_alias = 65536 - K_MARKER
    for seed in range(50):
        n = W + 300
        b = Buf(n, 4000 + seed)
        starts = [SCAN[e] for e in range(47, len(SCAN), 64)]
        R = next(s for s in starts if s >= K_SWEEP)
        e0 = SCAN.index(R)
        probes = [SCAN[e] for e in range(e0, min(e0 + 64, len(SCAN))) if SCAN[e] > R + 28672 + 8 and SCAN[e] < W - 600]
        alias = R + 28672
        probes = [q for q in probes if q < fill_alias + 32768]
        if not probes or alias in SCAN or fill_alias in SCAN:
            continue
        q = probes[0]
        b.put(alias, b.a[q:q + 4].copy())
        b.put(fill_alias, b.a[q:q + 4].copy())
        data = b.bytes()
        m = run_model(data, multi=True)
        if m.posmap[alias] or m.posmap[fill_alias] or not m.posmap[q] & 1 or m.stats[S_SPAN_CUTS] == 0 \
                or m.stats[S_EVENTS] != 0:
            continue
        out.append(("span_cut_twin", data))
        break
    return out


LENGTHS = [4, 5, 6, 7, 8, 9, 10, 11, 15, 16, 17, 18, 19, 20, 21, 22, 23, 244, 245, 246, 247, 255, 256, 257, 258, 259, 300]


def length_key(b, T):
    """A key of T bytes.  Longer than 258: bytes 254 .. 257 repeat bytes 1 .. 4, so the scan through the key's first
    copy (it has a lead-in, and its probe 61 is byte 254) finds a match of 4 there that ends at byte 258: byte 258 is
    then probed and inserted, and a later match over the whole key, cut at 258, is continued from there."""
    key = b.key(T, avoid=(RUN_A, RUN_B))
    if T > 258:
        key[254:258] = key[1:5]
        if key[258] == key[5]:
            key[258] ^= 0x3c
    return key


def gen_lengths():
    """Total match lengths.  Dense: [run][K][x] ... [run][K][y] -- the runs' matches end at K, so the second K is the
    probe at s of a dense batch whose candidate is the first K (fast event below 16; general path from 16 on:
    extend_match with have = 16, so length 16 + 4 lane + o puts the first differing byte at offset o of that lane's
    dword).  Sparse: the second K sits on a probe of a sparse scan (have = 4: length 4 + 4 lane + o)."""
    out = []
    lead = lead_len(2000)
    for seed in range(20):
        b = Buf(len(LENGTHS) * (2 * lead + 2) + 2 * sum(LENGTHS) + 1200, 5000 + seed)
        at, second = 0, {}
        for T in LENGTHS:
            key = length_key(b, T)
            p1 = at + lead
            b.lead_in(p1, RUN_A, 2000)
            b.put(p1, key)
            p2 = p1 + T + 1 + lead
            b.lead_in(p2, RUN_B, 2000)
            b.put(p2, key)
            b.a[p2 + T] = int(b.a[p1 + T]) ^ 0x21
            second[T] = p2
            at = p2 + T + 1
        assert at + 300 <= W
        data = b.a[:at + 300].tobytes()
        lg = run_model(data).log
        found = {(pos, d >> 16) for _, pos, _, _, _, d in lg[lg[:, 0] == LOG_MATCH].tolist()}
        # (a chance collision can take a key's slot: every key must be found whole, the longest continued at 258)
        if all((second[T], min(T, 258)) in found for T in LENGTHS) and (second[300] + 258, 42) in found:
            out.append(("lengths_dense", data))
            break
    # sparse: one stream per group of lengths, each plant on a probe the model reports
    for gi in range(0, len(LENGTHS), 5):
        group = LENGTHS[gi:gi + 5]
        for seed in range(30):
            b = Buf(len(group) * 9500 + 3000, 5100 + 37 * gi + seed)
            at, ok = 700, True
            for T in group:
                b.lead_in(at, RUN_A, 2000)
                key = length_key(b, T)
                b.put(at, key)
                m = run_model(b.bytes())
                if not m.posmap[at] & 1:
                    ok = False
                    break
                cand = [q for q in range(at + T + 3000, at + T + 6000) if m.posmap[q] & 1]
                if not cand:
                    ok = False
                    break
                q = cand[0]
                b.put(q, key)
                b.a[q + T] = int(b.a[at + T]) ^ 0x21
                at = q + T + 1 + 900
            if not ok:
                continue
            data = b.a[:at].tobytes()
            m = run_model(data)
            lg = m.log
            got = set((lg[(lg[:, 0] == LOG_MATCH) & (lg[:, 2] == PATH_SPARSE)][:, 5] >> 16).tolist())
            if all(min(T, 258) in got for T in group):
                out.append(("lengths_sparse_%d" % group[0], data))
                break
    return out


SKIP_E = [0, 1, 31, 32, 33, 46, 47, 48, 58, 59, 66, 67, 68, 110, 111, 201, 240]


def gen_skip():
    """[run][K][gap][K]: the run's last match ends at the first K, which is probed (and inserted) as `the probe at
    s`; the scan then starts one byte on, and the second K lies on its probe e.  47 .. 110 are the lanes 0 .. 63 of
    the first sparse batch."""
    out = []
    b = Buf(60000, 6000)
    at = 700
    for e in SKIP_E:
        b.lead_in(at, RUN_A, 0 if at == 700 else 4000)
        key = b.key(8, avoid=(RUN_A, RUN_B))
        q = at + 1 + SCAN[e]
        if q < at + 8:      # the two copies overlap: bytes of period q - at
            key = np.resize(key[:q - at], 8 + q - at)
            key[-1] ^= 0x3c
        else:
            b.put(q, key)
        b.put(at, key)
        at = q + 8 + lead_len(4000) + 50
    out.append(("skip_schedule", b.a[:at].tobytes()))
    # a scan that runs into s_limit with nexist = 1, 63 and 64 lanes in its last sparse batch
    want = {1: None, 63: None, 64: None}
    for t in range(300, 5200):
        if all(v is not None for v in want.values()):
            break
        b = Buf(700 + 8 + t, 6100)
        b.lead_in(700, RUN_A, 0)
        b.put(700, b.key(8, avoid=(RUN_A, RUN_B)))
        data = b.bytes()
        lg = run_model(data).log
        end = lg[lg[:, 0] == LOG_SCAN_END]
        if end.shape[0] == 1:
            k = int(end[0, 2])
            if k in (1, 63) and want[k] is None and end[0, 3] == 0:
                want[k] = data
            if k == 64 and want[64] is None and end[0, 3] == 1:
                want[64] = data
    out += [("scan_end_nexist%d" % k, v) for k, v in want.items() if v is not None]
    return out


def gen_groups():
    """Same-slot groups inside one batch."""
    out = []
    b = Buf(12000, 7000)
    A = b.key(4, avoid=(RUN_A, RUN_B))
    sep = lambda n: b.key(n, avoid=(RUN_A, RUN_B, int(A[0])))
    at = 700
    b.lead_in(at, RUN_A, 0)
    # two and three lanes with equal bytes; the later A is found in the batch itself
    for x in (A, sep(5), A, sep(7), A, sep(9)):
        at = b.put(at, x)
    # ... and A again in a later batch: the slot must hold the LATEST of them
    at += 700
    b.lead_in(at, RUN_B, 700)
    for x in (A, sep(6), A, sep(6)):          # (and two lanes of this batch)
        at = b.put(at, x)
    out.append(("group_equal_bytes", b.a[:at + 300].tobytes()))

    U, V = colliding_pair(11, True)
    b = Buf(12000, 7001)
    at = 700
    b.lead_in(at, RUN_A, 0)
    # collision of different bytes: U, V, U in one batch -- the second U must NOT match (the slot holds V)
    for x in (U, b.key(5, avoid=(RUN_A, RUN_B)), V, b.key(7, avoid=(RUN_A, RUN_B)), U, b.key(6, avoid=(RUN_A, RUN_B))):
        at = b.put(at, x)
    # two lanes of a batch, different bytes
    U, V = colliding_pair(12, True)
    at += 700
    b.lead_in(at, RUN_B, 700)
    for x in (U, b.key(5, avoid=(RUN_A, RUN_B)), V, b.key(7, avoid=(RUN_A, RUN_B))):
        at = b.put(at, x)
    # U and V by turns, four times each in one batch: eight lanes, and every one of them finds the OTHER value as
    # the latest member of its group
    U, V = colliding_pair(13, False)
    at += 700
    b.lead_in(at, RUN_A, 700)
    for i in range(8):
        at = b.put(at, V if i & 1 else U)
        at = b.put(at, b.key(2, avoid=(RUN_A, RUN_B, int(U[0]), int(V[0]))))
    out.append(("group_collision", b.a[:at + 300].tobytes()))

    # eight and more lanes through a run, a group whose earlier member lies inside a match (not inserted), and a
    # group whose first member is the match lane (candidate from the table)
    b = Buf(14000, 7002)
    K = b.key(12, avoid=(RUN_A, RUN_B))
    at = 700
    b.lead_in(at, RUN_A, 0)
    at = b.put(at, K)                       # far copy: K[0:12], every four-gram inserted
    at += 700
    b.lead_in(at, RUN_B, 700)
    at = b.put(at, K)                       # match of 12 over K: K[3:7] inside it is not inserted
    at = b.put(at, b.key(3, avoid=(RUN_A, RUN_B, int(K[3]))))
    at = b.put(at, K[3:7])                  # same slot as the covered lane: judged against the table
    at = b.put(at, b.key(5, avoid=(RUN_A, RUN_B)))
    at += 700
    b.lead_in(at, RUN_A, 700)
    for x in (K[:4], b.key(5, avoid=(RUN_A, RUN_B)), K[:4], b.key(6, avoid=(RUN_A, RUN_B)), K[:4],
              b.key(6, avoid=(RUN_A, RUN_B))):
        at = b.put(at, x)                   # three lanes, the FIRST is a match through the table
    at += 100
    b.a[at:at + 90] = 33                    # a run inside one batch: a group of 60 lanes
    at += 90
    out.append(("group_mixed", b.a[:at + 300].tobytes()))

    # one sparse batch, two probes with equal bytes and nothing earlier: the replay finds the first as candidate
    for seed in range(20):
        b = Buf(9000, 7100 + seed)
        b.lead_in(700, RUN_A, 0)
        K = b.key(8, avoid=(RUN_A, RUN_B))
        b.put(700, b.key(8, avoid=(RUN_A, RUN_B)))
        q1, q2 = 701 + SCAN[70], 701 + SCAN[90]
        b.put(q1, K)
        b.put(q2, K)
        data = b.bytes()
        lg = run_model(data).log
        rp = lg[lg[:, 0] == LOG_REPLAY]
        if rp.size and rp[0, 3] == 1:
            out.append(("group_sparse_replay", data))
            break
    return out


def gen_tags():
    """Colliding four-byte values with equal and with different slot tags; the foreign value sits in the slot when
    the other is looked up (another batch), then the first again.  Single-window: those run with tags."""
    out = []
    for same in (True, False):
        U, V = colliding_pair(21 if same else 22, same)
        b = Buf(8000, 8000 + same)
        at = 700
        for x in (U, V, U, V):
            b.lead_in(at, RUN_A, 700)
            at = b.put(at, x)
            at = b.put(at, b.key(8, avoid=(RUN_A, RUN_B)))
            at += 760
        out.append(("tags_%s" % ("equal" if same else "different"), b.a[:at].tobytes()))
    # a stream that begins with X Y Z and later holds 0 X Y Z at a probed position whose slot is empty: an `old != 0`
    # test that is missing would take position -1 as the candidate
    b = Buf(3000, 8010)
    b.a[0:3] = (11, 22, 33)
    b.lead_in(1500, RUN_B, 1500)
    b.put(1500, bytes([0, 11, 22, 33, 44]))
    out.append(("empty_slot_first_bytes", b.bytes()))
    return out


def gen_start_lanes():
    """Short matches back to back (a four-letter alphabet): the next event of a dense batch starts at every lane."""
    rng = np.random.default_rng(9000)
    return [("start_lanes", rng.integers(0, 4, 6000, dtype=np.uint8).tobytes())]


def gen_window_edges():
    out = []
    # candidates at W-16 (the last position a window inserts) and W-17, looked up early in the next window
    for back in (16, 17, 40):
        for seed in range(30):
            b = Buf(W + 3000, 9100 + 10 * back + seed)
            c = W - back
            K = b.key(30, avoid=(RUN_A, RUN_B))
            b.lead_in(c, RUN_A, 60000)
            b.put(c, K)                       # runs over the window start
            q = W + 1000
            b.lead_in(q, RUN_B, 1000)
            b.put(q, K)
            data = b.bytes()
            m = run_model(data, multi=True)
            if m.posmap[c] & 1 and m.posmap[q] & 2:
                out.append(("edge_cand_W-%d" % back, data))
                break
    # a final window of exactly 128 bytes that holds a match
    b = Buf(W + 128, 9200)
    K = b.key(12, avoid=(RUN_A, RUN_B))
    b.put(W + 20, K)
    b.put(W + 50, K)
    out.append(("edge_last_window_128", b.bytes()))
    # matches that end at n - t, and a match cut by the end of the input
    for t in (0, 1, 14, 15, 16, 17):
        b = Buf(700 + 40 + 8 + 40 + t, 9300 + t)
        b.lead_in(700, RUN_A, 0)
        K = b.key(40, avoid=(RUN_A, RUN_B))
        b.put(700, K)
        b.put(700 + 48, K)
        if t:
            b.a[700 + 88] = int(b.a[700 + 40]) ^ 0x11
        out.append(("edge_match_ends_n-%d" % t, b.bytes()))
    # matches that START at s_limit - 1 (the last probe) and at s_limit (never probed)
    for t in (16, 15):
        b = Buf(700 + 8 + 20 + t, 9400 + t)
        b.lead_in(700, RUN_A, 0)
        K = b.key(8, avoid=(RUN_A, RUN_B))
        b.put(700, K)
        b.put(700 + 28, K)
        out.append(("edge_match_starts_n-%d" % t, b.bytes()))
    b = Buf(1200, 9500)
    b.a[1000:] = 99
    out.append(("edge_run_to_the_end", b.bytes()))
    return out


def gen_sweep_first_batch():
    """A sweep that falls due in a window's first dense batch (s = -1), and one inside a sparse scan: searched for."""
    out = []
    for seed in range(200):
        b = Buf(2 * W + 400, 9600 + seed)
        data = b.bytes()
        st = run_model(data, multi=True).stats
        if st[S_SWEEP_FIRST_BATCH] and st[S_SWEEP_SPARSE]:
            out.append(("sweep_first_batch", data))
            break
    return out


def gen_marker_at_sweep():
    """A sweep in a sparse scan is made at the batch's first probe R, and that probe then looks a marker up at its
    smallest distance, kMarkerBack.  The four bytes at R are copied to R - 32768, which no scan has visited: a marker
    written 32768 behind R instead would make that position a candidate."""
    out = []
    for seed in range(100):
        b = Buf(2 * W + 400, 9700 + seed)
        m = run_model(b.bytes(), multi=True)
        lg = m.log
        for _, R, where, _, _, _ in lg[lg[:, 0] == LOG_SWEEP].tolist():
            c = R - 32768
            if where == 1 and c > 8 and not m.posmap[c - 3:c + 4].any() and m.posmap[R] & 1:
                b.put(c, b.a[R:R + 4].copy())
                out.append(("marker_at_sweep_point", b.bytes()))
                return out
    return out


_cases = None


def _build_cases():
    out = []
    for g in (gen_ladder, gen_alias_bait, gen_span_twin, gen_lengths, gen_skip, gen_groups, gen_tags,
              gen_start_lanes, gen_window_edges, gen_sweep_first_batch, gen_marker_at_sweep):
        out += g()
    return out


def cases():
    global _cases
    if _cases is None:
        _cases = _build_cases()
    return _cases


# ---------------------------------------------------------------------------------------------------------------
# (d) facts and rules

def model_for(data, go=False, mutant=0, log=True):
    """The model as the kernel runs this stream: single-window streams with the plain table and slot tags (the guest
    blocks of single-window launches), longer ones with modular slots."""
    multi = len(data) > W
    return run_model(data, go=go, tags=not multi, multi=multi, mutant=mutant, log=log)


def facts(oracle, data):
    """The rules this input reaches: from the oracle's tokens (both modes) and the model's counters and log."""
    a = np.frombuffer(bytes(data), np.uint8)
    n = a.size
    mo = {go: matches_of(oracle_tokens(oracle, data, go), n) for go in BOTH}
    starts = {go: set(mo[go][:, 0].tolist()) for go in BOTH}
    m = model_for(data)
    lg, st = m.log, m.stats
    out = set()
    eq4 = lambda x, y: x >= 0 and y >= 0 and bytes(a[x:x + 4]) == bytes(a[y:y + 4])
    d0 = mo[MOONBIT]
    if (d0[:, 2] == 32768).any():
        out.add("dist_32768_accepted")
    for _, pos, age, b, dist, _ in lg[lg[:, 0] == LOG_OLD].tolist():
        if not eq4(pos, pos - age) or pos in starts[MOONBIT] or pos in starts[GO]:
            continue          # (only lookups of a planted key whose old copy the reference refuses)
        if age == 32769:
            out.add("dist_32769_refused")
        if age > 32768 and not b & 1:
            out.add("live_slot_age_%d" % age)
        if age > 32768 and b & 1:
            out.add("marker_slot_age_%d" % age)
        k = age - 65536
        if k > 0 and eq4(pos, pos - k) and not m.posmap[pos - k] & 1:
            out.add("alias_bait_k%d" % k)
    if len(data) > W:
        if 0 < st[S_MARKER_MIN_DIST] <= K_MARKER + 63:
            out.add("marker_lookup_small_distance")
        if st[S_MARKER_MAX_DIST] >= K_MARKER + K_SWEEP:
            out.add("marker_lookup_behind_the_due_point")
        # the largest: a marker is at most kMarkerBack + kSweepEvery - 1 behind the point where the next sweep falls
        # due, and a sparse batch that begins in front of that point reaches up to kSpanMax - 1 beyond it (a dense
        # one 63).  "Near" = within a sixteenth of the span of that.
        if st[S_MARKER_MAX_DIST] >= K_MARKER + K_SWEEP - 1 + K_SPAN - 1 - K_SPAN // 16:
            out.add("marker_lookup_near_the_largest_distance")
        if st[S_SWEEP_SPARSE]:
            out.add("sweep_in_sparse_scan")
        if st[S_SWEEP_FIRST_BATCH]:
            out.add("sweep_at_window_first_batch")
        if st[S_SPAN_CUTS]:
            out.add("span_cut")
        for _, R, where, _, _, _ in lg[lg[:, 0] == LOG_SWEEP].tolist():
            if where == 1 and eq4(R, R - 32768) and not m.posmap[R - 32768] & 1 and R not in starts[MOONBIT] \
                    and st[S_MARKER_MIN_DIST] == K_MARKER:
                out.add("marker_looked_up_at_the_sweep_point_with_bait")
    dist_at = {pos: dist for pos, _, dist in d0.tolist()}
    for _, pos, path, lane, e, d in lg[lg[:, 0] == LOG_MATCH].tolist():
        total = d >> 16
        pname = ("fast", "general", "sparse")[path]
        out.add("len_%d_%s" % (total, pname))
        # the cap: the bytes go on being equal behind a match of 258, and the reference continues at once
        dist = dist_at.get(pos)
        if total == 258 and dist is not None and pos + 258 < n and a[pos + 258] != a[pos + 258 - dist]:
            out.add("len_258_exact_" + pname)     # (not cut: the next byte differs)
        if total == 258 and dist is not None and pos + 258 < n and a[pos + 258] == a[pos + 258 - dist]:
            out.add("len_258_cut_" + pname)
            if dist_at.get(pos + 258) == dist and dist >= 258:   # (not a run: the source does not overlap)
                out.add("len_259plus_split_" + pname)
        out.add("probe_e%d_%s" % (e, "sparse" if path == PATH_SPARSE else "dense"))
        if path == PATH_SPARSE:
            out.add("sparse_match_lane_%d" % lane)
    for _, pos, k, full, _, _ in lg[lg[:, 0] == LOG_SCAN_END].tolist():
        out.add("scan_end_nexist_%d" % k if k != 64 or full else "scan_end_nexist_64_partial")
    group_last = {pos + last for _, pos, _, _, _, last in lg[lg[:, 0] == LOG_GROUP].tolist()}
    for _, pos, size, same, _, _ in lg[lg[:, 0] == LOG_GROUP].tolist():
        out.add("group_%s_%s" % (size if size < 8 else "8plus", "equal_bytes" if same else "collision"))
    for _, pos, ins, hit, fd, before in lg[lg[:, 0] == LOG_GROUP_JUDGE].tolist():
        if ins < before:
            out.add("group_member_not_inserted")
        if hit and before == 0:
            out.add("group_match_lane_first")
        if hit and ins >= 1:
            out.add("group_match_lane_later")
            if pos in group_last:
                out.add("group_match_lane_last")
        if ins >= 2:
            out.add("group_two_inserted_members")
        if not hit and ins >= 1:
            out.add("group_foreign_member_refused")
    for _, pos, f, mine, _, _ in lg[lg[:, 0] == LOG_REPLAY].tolist():
        if mine and f < 64:
            out.add("sparse_replay_candidate_from_batch")
    for _, pos, same, _, _, _ in lg[lg[:, 0] == LOG_TAG].tolist():
        out.add("tag_equal_foreign_value" if same else "tag_different_foreign_value")
    for _, pos, lane, kept, _, _ in lg[lg[:, 0] == LOG_NEXT].tolist():
        if 59 <= lane <= 63:
            out.add("next_start_lane_%d_%s" % (lane, "kept" if kept else "fresh"))
    # windows
    for go in BOTH:
        tag = "go" if go else "default"
        for pos, ln, dist in mo[go].tolist():
            w = (pos // W) * W
            c = pos - dist
            if c < w:
                out.add("cand_W-%d_%s_len%s" % (w - c, tag, ln if ln == 4 else "5plus") if w - c <= 40 else "cand_prev_window_" + tag)
                if c + ln > w:
                    out.add("source_runs_into_current_window_" + tag)
                if dist == 32768:
                    out.add("dist_32768_across_window_start_" + tag)
    last = lz_chunks(n)[-1] if lz_chunks(n) else (0, 0)
    if last[1] == 128 and (d0[:, 0] >= last[0]).any():
        out.add("last_window_128_holds_a_match")
    if n <= W and n >= 128:
        for pos, ln, dist in d0.tolist():
            if n - (pos + ln) in (0, 1, 14, 15, 16):
                out.add("match_ends_at_n-%d" % (n - pos - ln))
            if pos + ln == n and 4 < ln < 258:
                out.add("match_cut_by_end_of_input")
            if pos == n - 16:
                out.add("match_starts_at_s_limit-1")
        sl = n - 15
        first = bytes(a).find(bytes(a[sl:sl + 4]))
        if 0 <= first < sl and m.posmap[first] & 1 and sl not in starts[MOONBIT] and (d0[:, 0] + d0[:, 1] <= sl).all():
            out.add("match_refused_at_s_limit")
        for p in np.nonzero(m.posmap & 1)[0].tolist():
            if a[p] == 0 and bytes(a[p + 1:p + 4]) == bytes(a[0:3]) and p not in starts[MOONBIT] and 3 < p < 32768:
                if not (lg[(lg[:, 0] == LOG_TAG) & (lg[:, 1] == p)]).size:
                    out.add("empty_slot_lookup_of_0_and_first_bytes")
    return out


def coverage(oracle):
    """rule -> the cases that reach it."""
    cov = {}
    for name, data in cases():
        for r in facts(oracle, data):
            cov.setdefault(r, []).append(name)
    return cov


# rule -> the case built for it (its witness).  A fast event has tf < 16, so the lengths from 16 on exist on the
# general and the sparse path only; a length above 258 exists as a match of 258 that the reference continues at once.
REQUIRED_RULES = {
    "dist_32768_accepted": "ladder_d32768_ph0_w0",
    "dist_32769_refused": "ladder_d32769_ph0_w0",
    "live_slot_age_32769": "ladder_d32769_ph0_w0",
    "live_slot_age_36864": "ladder_d36864_ph0_w0",
    "live_slot_age_53247": "ladder_d53247_ph9973_w0",
    "live_slot_age_53248": "ladder_d53248_ph9973_w0",
    "marker_slot_age_36864": "ladder_d36864_ph9973_w1",
    "marker_slot_age_57408": "ladder_d57408_ph0_w1",
    "marker_slot_age_65535": "ladder_d65535_ph0_w1",
    "marker_slot_age_65536": "ladder_d65536_ph0_w1",
    "marker_slot_age_65537": "ladder_d65537_ph0_w1",
    "marker_slot_age_98304": "ladder_d98304_ph0_w1",
    "marker_lookup_small_distance": "sweep_first_batch",
    "marker_lookup_behind_the_due_point": "sweep_first_batch",
    "marker_lookup_near_the_largest_distance": "alias_k1_sparse",
    "sweep_in_sparse_scan": "sweep_first_batch",
    "sweep_at_window_first_batch": "sweep_first_batch",
    "span_cut": "span_cut_twin",
    "marker_looked_up_at_the_sweep_point_with_bait": "marker_at_sweep_point",
    "alias_bait_k1": "alias_k1_sparse",
    "alias_bait_k4": "alias_k4_sparse",
    "alias_bait_k300": "alias_k300_sparse",
    "alias_bait_k32768": "alias_k32768_ph1_w1",
    "cand_W-16_default_len4": "edge_cand_W-16",
    "cand_W-16_go_len5plus": "edge_cand_W-16",
    "cand_W-17_default_len4": "edge_cand_W-17",
    "source_runs_into_current_window_go": "edge_cand_W-16",
    "dist_32768_across_window_start_default": "ladder_d32768_ph0_w1",
    "dist_32768_across_window_start_go": "ladder_d32768_ph0_w1",
    "last_window_128_holds_a_match": "edge_last_window_128",
    "match_ends_at_n-0": "edge_match_ends_n-0",
    "match_ends_at_n-1": "edge_match_ends_n-1",
    "match_ends_at_n-14": "edge_match_ends_n-14",
    "match_ends_at_n-15": "edge_match_ends_n-15",
    "match_ends_at_n-16": "edge_match_ends_n-16",
    "match_cut_by_end_of_input": "edge_run_to_the_end",
    "match_starts_at_s_limit-1": "edge_match_starts_n-16",
    "match_refused_at_s_limit": "edge_match_starts_n-15",
    "empty_slot_lookup_of_0_and_first_bytes": "empty_slot_first_bytes",
    "group_2_equal_bytes": "group_equal_bytes",
    "group_3_equal_bytes": "group_equal_bytes",
    "group_8plus_equal_bytes": "group_mixed",
    "group_2_collision": "group_collision",
    "group_3_collision": "group_collision",
    "group_8plus_collision": "group_collision",
    "group_two_inserted_members": "group_collision",
    "group_foreign_member_refused": "group_collision",
    "group_member_not_inserted": "group_mixed",
    "group_match_lane_first": "group_mixed",
    "group_match_lane_later": "group_equal_bytes",
    "group_match_lane_last": "group_equal_bytes",
    "sparse_replay_candidate_from_batch": "group_sparse_replay",
    "tag_equal_foreign_value": "tags_equal",
    "tag_different_foreign_value": "tags_different",
    "next_start_lane_59_kept": "start_lanes",
    "next_start_lane_60_kept": "start_lanes",
    "next_start_lane_61_kept": "start_lanes",
    "next_start_lane_62_fresh": "start_lanes",
    "next_start_lane_63_fresh": "start_lanes",
    "scan_end_nexist_1": "scan_end_nexist1",
    "scan_end_nexist_63": "scan_end_nexist63",
    "scan_end_nexist_64": "scan_end_nexist64",
    "sparse_match_lane_0": "skip_schedule",
    "sparse_match_lane_63": "skip_schedule",
}
REQUIRED_RULES.update({"probe_e%d_%s" % (e, "dense" if e < 47 else "sparse"): "skip_schedule" for e in SKIP_E})
REQUIRED_RULES.update({"len_%d_fast" % t: "lengths_dense" for t in (4, 5, 6, 7, 8, 9, 10, 11, 15)})
REQUIRED_RULES.update({"len_%d_general" % t: "lengths_dense"
                       for t in (16, 17, 18, 19, 20, 21, 22, 23, 244, 245, 246, 247, 255, 256, 257, 258)})
REQUIRED_RULES.update({"len_258_exact_general": "lengths_dense", "len_258_cut_general": "lengths_dense",
                       "len_259plus_split_general": "lengths_dense", "len_258_exact_sparse": "lengths_sparse_247",
                       "len_258_cut_sparse": "lengths_sparse_259", "len_259plus_split_sparse": "lengths_sparse_259"})
REQUIRED_RULES.update({"len_%d_sparse" % t: "lengths_sparse_4" for t in (4, 5, 6, 7, 8)})
REQUIRED_RULES.update({"len_%d_sparse" % t: "lengths_sparse_9" for t in (9, 10, 11, 15, 16)})
REQUIRED_RULES.update({"len_%d_sparse" % t: "lengths_sparse_17" for t in (17, 18, 19, 20, 21)})
REQUIRED_RULES.update({"len_%d_sparse" % t: "lengths_sparse_22" for t in (22, 23, 244, 245, 246)})
REQUIRED_RULES.update({"len_%d_sparse" % t: "lengths_sparse_247" for t in (247, 255, 256, 257, 258)})


# The mutants that a single case kills, and that case: if it stopped killing, the table would lose the mutant.
PINNED_KILLERS = {4: "marker_at_sweep_point", 5: "span_cut_twin", 13: "edge_match_starts_n-15", 15: "skip_schedule"}


def kill_table(oracle, mutants=None):
    """mutant -> the cases whose tokens, from the model built with that fault, are not the oracle's (default mode and
    Go mode; a case counts once)."""
    table = {}
    want = {}
    for k in (mutants or sorted(MUTANTS)):
        killers = []
        for name, data in cases():
            for go in BOTH:
                if (name, go) not in want:
                    want[(name, go)] = oracle_tokens(oracle, data, go)
                if not same_tokens(model_for(data, go=bool(go), mutant=k, log=False).tokens, want[(name, go)]):
                    killers.append(name)
                    break
        table[k] = killers
    return table
