// lz77_wave_model.cpp -- TEST INFRASTRUCTURE.  Lane-accurate host model of the wave64
// match-finder kernel (moonbit-flate_amd/csrc/lz77_kernels.hip): every per-lane value is
// an array of 64, every ballot a 64-bit mask.  It lets the CPU test-suite fuzz the batch
// algorithm (dense multi-event batches + sparse scan batches + duplicate-slot handling)
// against the oracle without a GPU.  It follows the kernel, not the reference: the
// reference semantics it must reproduce are DeflateFast::encode, deflate-fast.mbt:123-270.
//
// Two table modes.  The plain one (model_lz77, flags bit 2 clear) keeps 32-bit absolute positions,
// slot = position + 1 and 0 = empty: what the kernel's single-window builds do.  The MULTI one (flags
// bit 2) is transcribed from lz77_stream<MULTI = true> with the same constants: slots hold
// (position + 1) mod 2^16, the empty table is filled with a marker, sweep() runs when the first
// position of a dense or sparse batch has reached the sweep clock, and a sparse batch is cut after
// kSpanMax positions (nexist / nall).  Beside the modular table the model keeps a SHADOW table of
// 32-bit absolute positions that is never swept; every lookup compares "in range" and the candidate
// position of the two and counts the disagreements (stats[5]; the tests assert zero).
//
// What it does not restate: the window-unit hand-over between blocks (uq_run: the table travels
// through memory, a guest rebuilds its tags), the dictionary builds' Hist reads and prime pass, and
// the stream writer's rebase.  One table serves all windows of a stream here.
//
// -DLZ_MODEL_MUTANT=k builds the model with ONE deliberate fault (list below).  The mutants exist
// only in this file: tests/test_lz77_corpus.py shows that for each of them some corpus case gives
// tokens that are not the oracle's, i.e. that the corpus would notice that fault in the kernel.
#include <cstdint>
#include <cstring>
#include <vector>

#ifndef LZ_MODEL_MUTANT
#define LZ_MODEL_MUTANT 0
#endif
//  1 in-range test `dist < 32768`            2 in-range test `dist <= 32769`
//  3 no sweep                                4 marker 32768 behind the sweep point
//  5 no span cut                             6 `dist != 0` / `old != 0` test dropped
//  7 same-slot group: EARLIEST inserted member instead of the latest
//  8 dense commit in reversed order          9 sparse replay skipped
// 10 `have <= 16` takes the short path      11 length cap 257          12 length cap 259
// 13 s_limit + 1                            14 s_limit - 1
// 15 dense -> sparse hand-over at probe 48  16 `cand + 4 < W` -> `cand < W`
// 17 tag compare inverted for tag value 2
#define MUT(k) (LZ_MODEL_MUTANT == (k))

namespace {

constexpr int kTableSize = 16384;
constexpr int kWin = 65535;
constexpr int kSmallLzMin = 128;
constexpr int kDenseKeep = 61;  // continue in the same dense batch while the next s-1 lane <= this
constexpr uint32_t kSweepEvery = 20480, kSpanMax = 4096, kMarkerBack = MUT(4) ? 32768 : 36864;
constexpr int kMaxLen = MUT(11) ? 257 : MUT(12) ? 259 : 258;
constexpr int kMargin = MUT(13) ? 14 : MUT(14) ? 16 : 15;  // s_limit = n - kMargin
constexpr int kNumStats = 32;

inline uint32_t ld32(const uint8_t *p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}
inline uint32_t hash4(uint32_t u) { return (u * 0x1e35a7bdu) >> 18; }
// the guest blocks' 2-bit slot tag (lz77_kernels.hip, tag_of): the two product bits below the slot index
inline uint32_t tag_of(uint32_t u) { return ((u * 0x1e35a7bdu) >> 16) & 3u; }
inline int ctz64(uint64_t m) { return m ? __builtin_ctzll(m) : 64; }
inline uint64_t below(int l) { return l >= 64 ? ~0ull : ((1ull << l) - 1); }  // lanes < l
inline uint64_t upto(int l) { return l >= 63 ? ~0ull : ((1ull << (l + 1)) - 1); }  // lanes <= l
inline bool in_range(uint32_t dist) {
  return MUT(1) ? dist < 32768u : MUT(2) ? dist <= 32769u : dist <= 32768u;
}

int scan_off(int e, int *step, const std::vector<uint32_t> &tab) {
  if (e < 32) { *step = 1; return e; }
  if (e < 48) { *step = 2; return 32 + 2 * (e - 32); }
  if (e < 59) { *step = 3; return 64 + 3 * (e - 48); }
  if (e < 67) { *step = 4; return 97 + 4 * (e - 59); }
  if (e + 1 >= (int)tab.size()) { *step = 1; return 1 << 24; }
  *step = (int)(tab[e + 1] - tab[e]);
  return (int)tab[e];
}

int common_prefix16(const uint8_t *a, const uint8_t *b) {
  int i = 0;
  while (i < 16 && a[i] == b[i]) ++i;
  return i;
}

struct Rec { uint32_t pos, tok; };

// stats_out of model_lz77_ex (the first five are model_lz77's)
enum {
  S_DENSE, S_SPARSE, S_EVENTS, S_DUP_EVALS, S_DISCARDED,
  S_SHADOW_DISAGREE,    // lookups where the modular table and the shadow differ in "in range" or in the candidate
  S_SWEEP_DENSE, S_SWEEP_SPARSE, S_SWEEP_FIRST_BATCH,  // sweeps by where they fell (first batch of a window: s == -1)
  S_SPAN_CUTS,          // sparse batches with nexist < nall
  S_MARKER_LOOKUPS, S_MARKER_MIN_DIST, S_MARKER_MAX_DIST,  // lookups of a marker-valued slot, their modular distance
  S_AGE_32768, S_AGE_32769,  // lookups whose slot's true age (shadow) is exactly that
  S_LIVE_OLD,           // lookups of a slot older than 32768 that no sweep has replaced yet
  S_REPLAYS,            // sparse batches replayed in order
  S_TAG_SKIPS,          // dense lookups the slot tag refused
  S_LOG_LOST,           // log entries that did not fit
  S_FAST, S_GENERAL, S_SPARSE_EVENTS,  // matches by path
  S_LOOKUPS,
  S_LOG_COUNT,          // log entries written
};

// log entries: six words {kind, absolute position, a, b, c, d}
enum {
  LOG_OLD = 1,      // lookup at pos whose slot's true age is >= 32767: a = age, b = 1 marker-valued | 2 in range (modular), c = modular distance
  LOG_SWEEP = 2,    // sweep at R = pos: a = 0 dense / 1 sparse, b = 1 if it is a window's first batch
  LOG_MATCH = 3,    // match at pos: a = path (0 fast, 1 general, 2 sparse), b = lane, c = probe index (-1: the probe at s), d = have | start lane << 8 | total << 16
  LOG_SPANCUT = 4,  // sparse batch at p0 = pos: a = nexist, b = nall, c = e_idx
  LOG_GROUP = 5,    // dense batch at B = pos: same-slot group, a = lanes, b = 1 if their four bytes are all equal, c = first lane, d = last lane
  LOG_REPLAY = 6,   // sparse replay at p0 = pos: a = match lane or 64, b = 1 if the candidate was inserted by an earlier lane of the batch
  LOG_SCAN_END = 7, // the scan ran into s_limit in a sparse batch at pos: a = nexist of the last batch that had lanes, b = 1 if that batch was full and the next one empty
  LOG_NEXT = 8,     // after a dense-batch match: a = lane of the next event start (s - 1 - B), b = 1 kept in the batch / 0 fresh batch
  LOG_TAG = 9,      // tagged dense lookup at pos with a FOREIGN value in the slot (other four bytes): a = 1 tags equal (slot read) / 0 different (read skipped)
  LOG_GROUP_JUDGE = 10,  // general path judged lane fd of a group: a = members already inserted, b = 1 match, c = lane fd, d = group lanes before fd
};

const uint8_t kZeros[512] = {0};

}  // namespace

// flags: bit 0 = compat_go; bit 1 = model the guest blocks' slot tags (a dense-batch lane whose own
// tag differs from its slot's skips the slot read: its candidate could not pass `cv == cand.val`);
// bit 2 = MULTI (16-bit modular slots, sweeps, span cut).
// The caller provides 64 readable bytes in front of `stream` and behind it (a mutant may look there).
// posmap (len bytes or null): bit 0 = the position was inserted, bit 1 = it was looked up.
extern "C" int model_lz77_ex(const uint8_t *stream, uint64_t len, int flags, uint32_t *recs_out,
                             uint32_t *chunk_nmatch, uint64_t *stats_out, uint8_t *posmap, uint32_t *log,
                             uint32_t log_cap) {
  const int compat_go = flags & 1;
  const bool use_tags = (flags & 2) != 0;
  const bool multi = (flags & 4) != 0;
  std::vector<uint32_t> table(kTableSize, 0), shadow(kTableSize, 0);
  std::vector<uint8_t> tags(kTableSize, 0), ismark(kTableSize, 0);
  std::vector<uint32_t> scantab;
  {
    uint32_t skip = 32, pos = 0;
    while (pos <= 65535) { scantab.push_back(pos); uint32_t st = skip >> 5; pos += st; skip += st; }
    scantab.push_back(1 << 24);
  }
  uint64_t st[kNumStats] = {0};
  st[S_MARKER_MIN_DIST] = ~0ull;
  uint32_t nlog = 0;
  auto logit = [&](uint32_t kind, uint32_t pos, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    if (!log) return;
    if (nlog >= log_cap) { st[S_LOG_LOST]++; return; }
    uint32_t *e = log + 6ull * nlog++;
    e[0] = kind; e[1] = pos; e[2] = a; e[3] = b; e[4] = c; e[5] = d;
  };
  // history bytes at absolute position `cand` (a mutant's candidate may lie in front of the stream)
  auto at = [&](uint32_t cand) -> const uint8_t * {
    const int32_t c = (int32_t)cand;
    return c < -64 ? kZeros : stream + c;
  };
  if (multi) {
    const uint32_t fill = (0u - kMarkerBack + 1u) & 0xffffu;
    for (int i = 0; i < kTableSize; ++i) { table[i] = fill; ismark[i] = 1; }
  }
  uint32_t next_sweep = kSweepEvery;
  auto sweep = [&](uint32_t R, int where, bool first_batch) {
    const uint32_t marker = (R - kMarkerBack + 1u) & 0xffffu;
    for (int i = 0; i < kTableSize; ++i) {
      const uint32_t d = (R + 1u - table[i]) & 0xffffu;
      if (d == 0 || d > 32768u) { table[i] = marker; ismark[i] = 1; }
    }
    next_sweep = R + kSweepEvery;
    st[where ? S_SWEEP_SPARSE : S_SWEEP_DENSE]++;
    if (first_batch) st[S_SWEEP_FIRST_BATCH]++;
    logit(LOG_SWEEP, R, (uint32_t)where, first_batch ? 1u : 0u, 0, 0);
  };
  struct Look { bool inr; uint32_t cand, old; };
  auto lookup = [&](uint32_t A1, uint32_t h) -> Look {
    Look k;
    k.old = table[h];
    const uint32_t dist = multi ? ((A1 - k.old) & 0xffffu) : (A1 - k.old);
    const bool nonzero = MUT(6) ? true : (multi ? dist != 0 : k.old != 0);
    k.inr = nonzero && in_range(dist);
    k.cand = A1 - 1u - dist;
    st[S_LOOKUPS]++;
    if (posmap) posmap[A1 - 1u] |= 2;
    const uint32_t so = shadow[h];
    const bool sinr = so != 0 && A1 - so <= 32768u;
    if (multi && (k.inr != sinr || (k.inr && k.cand != so - 1u))) st[S_SHADOW_DISAGREE]++;
    const uint32_t age = so ? A1 - so : 0;
    if (age == 32768u) st[S_AGE_32768]++;
    if (age == 32769u) st[S_AGE_32769]++;
    if (multi && ismark[h]) {
      st[S_MARKER_LOOKUPS]++;
      if (dist < st[S_MARKER_MIN_DIST]) st[S_MARKER_MIN_DIST] = dist;
      if (dist > st[S_MARKER_MAX_DIST]) st[S_MARKER_MAX_DIST] = dist;
    }
    if (age > 32768u && multi && !ismark[h]) st[S_LIVE_OLD]++;
    if (age >= 32767u) logit(LOG_OLD, A1 - 1u, age, (ismark[h] ? 1u : 0u) | (k.inr ? 2u : 0u), dist, 0);
    return k;
  };
  auto store = [&](uint32_t h, uint32_t A1, uint32_t cv) {
    table[h] = multi ? (A1 & 0xffffu) : A1;
    shadow[h] = A1;
    ismark[h] = 0;
    tags[h] = (uint8_t)tag_of(cv);
    if (posmap) posmap[A1 - 1u] |= 1;
  };

  const uint64_t full = len / kWin, r = len % kWin;
  const uint32_t nchunks = (uint32_t)(full + (r >= kSmallLzMin ? 1 : 0));
  uint64_t rec_base = 0;
  for (uint32_t c = 0; c < nchunks; ++c) {
    const uint32_t W = c * (uint32_t)kWin;
    const int n = (int)((len - W) < (uint64_t)kWin ? (len - W) : kWin);
    const uint8_t *src = stream + W;
    const int s_limit = n - kMargin;
    Rec *out = reinterpret_cast<Rec *>(recs_out) + rec_base;
    uint32_t nm = 0;

    int s = -1;          // POST state: re-insert s-1, probe s, scan from s+1 (chunk start: s = -1)
    bool sparse = false; // SPARSE state: continue the scan at (scan_base, e_idx)
    int scan_base = 0, e_idx = 0;
    bool done = false;
    int last_nexist = 0;

    // MoonBit: the previous window is empty
    auto cross = [&](uint32_t cand) { return !compat_go && (MUT(16) ? cand < W : cand + 4 < W); };
    auto extend = [&](int pf, uint32_t cand, int have) -> int {
      // total match length given `have` (>= 4) already verified bytes
      int limit = n - pf;
      if (limit > kMaxLen) limit = kMaxLen;
      if (cross(cand)) return 4;
      int l = have;
      const uint8_t *a = src + pf, *b = at(cand);
      while (l < limit && a[l] == b[l]) ++l;
      return l;
    };
    auto emit = [&](int pf, int total, uint32_t cand) {
      out[nm].pos = (uint32_t)pf;
      out[nm].tok = (1u << 30) | ((uint32_t)(total - 3) << 22) | ((W + (uint32_t)pf) - cand - 1);
      ++nm;
    };

    while (!done) {
      if (!sparse) {
        // ----------------------------- dense batch --------------------------------
        st[S_DENSE]++;
        const int B = s - 1;
        if (multi && !MUT(3)) {
          const uint32_t first = W + (uint32_t)(B < 0 ? 0 : B);
          if (first >= next_sweep) sweep(first, 0, B < 0);
        }
        int q[64];
        uint32_t cv[64], h[64], cand_abs[64], A1[64];
        uint8_t own[64][16];
        int mlen[64];
        uint64_t LD = 0, E1 = 0, E2 = 0, OK = 0, DUP = 0;
        for (int L = 0; L < 64; ++L) {
          q[L] = B + L;
          cv[L] = h[L] = cand_abs[L] = 0;
          mlen[L] = 0;
          A1[L] = W + (uint32_t)q[L] + 1;
          if (q[L] >= 0 && q[L] + 1 <= s_limit) E1 |= 1ull << L;
          if (q[L] >= 0 && q[L] + 2 <= s_limit) E2 |= 1ull << L;
        }
        LD = E1;
        for (int L = 0; L < 64; ++L) {
          if (!((LD >> L) & 1)) continue;
          memcpy(own[L], src + q[L], 16);
          cv[L] = ld32(src + q[L]);
          h[L] = hash4(cv[L]);
          bool maybe = true;
          if (use_tags) {
            const uint32_t mine = tag_of(cv[L]);
            maybe = tags[h[L]] == mine;
            if (MUT(17) && mine == 2u) maybe = !maybe;
            const uint32_t so = shadow[h[L]];
            if (so != 0 && A1[L] - so <= 32768u && ld32(at(so - 1u)) != cv[L])
              logit(LOG_TAG, A1[L] - 1u, tags[h[L]] == mine ? 1u : 0u, 0, 0, 0);
            if (!maybe) st[S_TAG_SKIPS]++;
          }
          if (!maybe) continue;
          const Look k = lookup(A1[L], h[L]);
          cand_abs[L] = k.cand;
          if (k.inr) {
            mlen[L] = common_prefix16(own[L], at(k.cand));
            if (mlen[L] >= 4) OK |= 1ull << L;
          }
        }
        // same-slot groups.  DUP as the LDS-table kernel finds it: of a two-lane group the later lane, of a
        // larger group every lane (the guests leave the first member out: it is judged the same either way).
        // FIRST2 = the first lanes of the two-lane groups: stats[3] goes on counting them as evaluations, as it
        // did when DUP held every lane of every group
        uint64_t FIRST2 = 0;
        for (int L = 0; L < 64; ++L) {
          if (!((LD >> L) & 1)) continue;
          uint64_t G = 0;
          for (int M = 0; M < 64; ++M)
            if (((LD >> M) & 1) && h[L] == h[M]) G |= 1ull << M;
          const int size = __builtin_popcountll(G);
          if (size < 2) continue;
          const int first = ctz64(G), last = 63 - __builtin_clzll(G);
          if (size == 2) { DUP |= 1ull << last; FIRST2 |= 1ull << first; }
          else DUP |= G;
          if (L == first) {
            bool same = true;
            for (int M = 0; M < 64; ++M)
              if (((G >> M) & 1) && cv[M] != cv[L]) same = false;
            logit(LOG_GROUP, W + (uint32_t)(B < 0 ? 0 : B), (uint32_t)size, same ? 1u : 0u, (uint32_t)first, (uint32_t)last);
          }
        }

        uint64_t INS = 0;
        int a = 0;
        bool batch_over = false;
        while (!batch_over) {
          // probe lanes of this event
          const uint64_t a_ins = (LD >> a) & 1 ? (1ull << a) : 0;
          uint64_t R = 0;
          int eidx[64];
          for (int L = 0; L < 64; ++L) eidx[L] = -2;
          if (a + 1 <= 63 && ((LD >> (a + 1)) & 1) && q[a + 1] >= 0) { R |= 1ull << (a + 1); eidx[a + 1] = -1; }
          bool scan_ended = false;
          int consumed = 0;
          {
            const int b = a + 2;
            for (int e = 0;; ++e) {
              int step;
              const int L = b + scan_off(e, &step, scantab);
              if (L > 63) break;
              const bool ex = step == 1 ? ((E1 >> L) & 1) : ((E2 >> L) & 1);
              if (!ex) { scan_ended = true; break; }
              R |= 1ull << L;
              eidx[L] = e;
              consumed = e + 1;
            }
          }
          uint64_t T = 0, rem = R;
          int f = 64;
          uint32_t cand = 0;
          int have = 0;
          bool fast = false;
          for (;;) {
            const int fv = ctz64(OK & rem & ~DUP), fd = ctz64(DUP & rem);
            if (fv < fd) {
              f = fv; cand = cand_abs[fv]; have = mlen[fv];
              // the kernel's fast event: no same-slot lane in front of the match lane and no extension needed
              if (rem == R) {
                const int tf = cross(cand) ? 4 : have;
                fast = MUT(10) ? tf <= 16 : tf < 16;
              }
              T |= rem & upto(fv);
              break;
            }
            if (fd == 64) { T |= rem; break; }
            st[S_DUP_EVALS]++;
            T |= rem & below(fd);
            uint64_t G = 0, Gall = 0;
            for (int L = 0; L < fd; ++L) {
              if (((LD >> L) & 1) && h[L] == h[fd]) Gall |= 1ull << L;
              if (((INS | T | a_ins) >> L) & 1 && h[L] == h[fd]) G |= 1ull << L;
            }
            bool v;
            uint32_t cnd;
            int ml;
            if (G) {
              const int i = MUT(7) ? ctz64(G) : 63 - __builtin_clzll(G);
              v = cv[i] == cv[fd];
              cnd = W + (uint32_t)q[i];
              ml = common_prefix16(own[fd], own[i]);
            } else {
              v = (OK >> fd) & 1;
              cnd = cand_abs[fd];
              ml = mlen[fd];
            }
            logit(LOG_GROUP_JUDGE, A1[fd] - 1u, (uint32_t)__builtin_popcountll(G), v ? 1u : 0u, (uint32_t)fd,
                  (uint32_t)__builtin_popcountll(Gall));
            T |= 1ull << fd;
            if (v) { f = fd; cand = cnd; have = ml; break; }
            rem &= ~upto(fd);
          }
          st[S_DUP_EVALS] += (uint64_t)__builtin_popcountll(FIRST2 & T);
          if (f == 64) {
            if (scan_ended) {
              INS |= T | a_ins;
              done = true;
            } else if (a == 0) {  // nothing in this whole batch: continue as a sparse scan
              INS |= T | a_ins;
              sparse = true;
              scan_base = s + 1;
              e_idx = MUT(15) ? consumed + 1 : consumed;
            } else {
              st[S_DISCARDED]++;  // partial event at the end of the batch: redo it in a new batch
            }
            batch_over = true;
          } else {
            INS |= T | a_ins;
            st[S_EVENTS]++;
            st[fast ? S_FAST : S_GENERAL]++;
            const int pf = q[f];
            const bool shortp = MUT(10) ? have <= 16 : have < 16;
            const int total = shortp ? (cross(cand) ? 4 : have) : extend(pf, cand, 16);
            logit(LOG_MATCH, W + (uint32_t)pf, fast ? 0u : 1u, (uint32_t)f, (uint32_t)eidx[f],
                  (uint32_t)have | ((uint32_t)a << 8) | ((uint32_t)total << 16));
            emit(pf, total, cand);
            s = pf + total;
            if (s >= s_limit) { done = true; batch_over = true; }
            else {
              a = s - 1 - B;
              logit(LOG_NEXT, W + (uint32_t)pf, (uint32_t)a, a > kDenseKeep ? 0u : 1u, 0, 0);
              if (a > kDenseKeep) batch_over = true;  // start a fresh dense batch at s
            }
          }
        }
        // commit the inserts in position order (later positions overwrite earlier ones)
        for (int k = 0; k < 64; ++k) {
          const int L = MUT(8) ? 63 - k : k;
          if ((INS >> L) & 1) store(h[L], A1[L], cv[L]);
        }
      } else {
        // ----------------------------- sparse batch -------------------------------
        st[S_SPARSE]++;
        int p[64], step[64];
        uint64_t EXall = 0, EX = 0;
        for (int L = 0; L < 64; ++L) {
          p[L] = scan_base + scan_off(e_idx + L, &step[L], scantab);
          if (p[L] + step[L] <= s_limit) EXall |= 1ull << L;
        }
        for (int L = 0; L < 64; ++L)  // MULTI: keep the batch within kSpanMax positions
          if (((EXall >> L) & 1) && (!multi || MUT(5) || (uint32_t)(p[L] - p[0]) < kSpanMax)) EX |= 1ull << L;
        const int nall = __builtin_popcountll(EXall), nexist = __builtin_popcountll(EX);
        if (nall == 0) {
          logit(LOG_SCAN_END, W + (uint32_t)p[0], (uint32_t)last_nexist, last_nexist == 64 ? 1u : 0u, 0, 0);
          done = true;
          break;
        }
        if (multi && !MUT(3) && W + (uint32_t)p[0] >= next_sweep) sweep(W + (uint32_t)p[0], 1, false);
        if (nexist < nall) {
          st[S_SPAN_CUTS]++;
          logit(LOG_SPANCUT, W + (uint32_t)p[0], (uint32_t)nexist, (uint32_t)nall, (uint32_t)e_idx, 0);
        }
        last_nexist = nexist;
        uint32_t cvs[64], hs[64], A1s[64], olds[64], cands[64];
        uint64_t V = 0;
        for (int L = 0; L < nexist; ++L) {
          cvs[L] = ld32(src + p[L]);
          hs[L] = hash4(cvs[L]);
          A1s[L] = W + (uint32_t)p[L] + 1;
          const Look k = lookup(A1s[L], hs[L]);
          olds[L] = k.old;
          cands[L] = k.cand;
          if (k.inr && ld32(at(k.cand)) == cvs[L]) V |= 1ull << L;
        }
        const int f0 = ctz64(V);
        const int lim = f0 < nexist - 1 ? f0 : nexist - 1;
        bool C = false;
        for (int L = 0; L <= lim && !C; ++L)
          for (int M = 0; M < L; ++M)
            if (hs[L] == hs[M]) { C = true; break; }
        if (MUT(9)) C = false;
        int f = f0;
        uint32_t cand = 0;
        if (!C) {
          for (int L = 0; L <= lim; ++L) store(hs[L], A1s[L], cvs[L]);
          if (f0 < 64) cand = cands[f0];
        } else {
          // two lanes of this batch share a slot: replay the batch in order
          st[S_REPLAYS]++;
          f = 64;
          bool from_batch = false;
          for (int e2 = 0; e2 < nexist; ++e2) {
            const uint32_t cur = table[hs[e2]];
            store(hs[e2], A1s[e2], cvs[e2]);
            bool v = false;
            uint32_t cnd = 0;
            bool mine = false;
            if (cur == olds[e2]) {
              v = (V >> e2) & 1;
              cnd = cands[e2];
            } else {  // candidate was inserted by an earlier lane of this batch
              for (int i = 0; i < nexist; ++i)
                if ((multi ? (A1s[i] & 0xffffu) : A1s[i]) == cur) {
                  v = cvs[i] == cvs[e2];
                  cnd = A1s[i] - 1u;
                  mine = true;
                  break;
                }
            }
            if (v) { f = e2; cand = cnd; from_batch = mine; break; }
          }
          logit(LOG_REPLAY, W + (uint32_t)p[0], (uint32_t)f, from_batch ? 1u : 0u, 0, 0);
        }
        if (f == 64) {
          if (nexist == nall && nall < 64) {  // the scan ran into s_limit
            logit(LOG_SCAN_END, W + (uint32_t)p[0], (uint32_t)nexist, 0, 0, 0);
            done = true;
            break;
          }
          e_idx += nexist;
          continue;
        }
        st[S_EVENTS]++;
        st[S_SPARSE_EVENTS]++;
        const int pf = p[f];
        const int total = extend(pf, cand, 4);
        logit(LOG_MATCH, W + (uint32_t)pf, 2u, (uint32_t)f, (uint32_t)(e_idx + f), 4u | ((uint32_t)total << 16));
        emit(pf, total, cand);
        s = pf + total;
        sparse = false;
        if (s >= s_limit) done = true;
      }
    }
    chunk_nmatch[c] = nm;
    rec_base += 16384;
  }
  if (st[S_MARKER_MIN_DIST] == ~0ull) st[S_MARKER_MIN_DIST] = 0;
  st[S_LOG_COUNT] = nlog;
  if (stats_out)
    for (int i = 0; i < kNumStats; ++i) stats_out[i] = st[i];
  return (int)nchunks;
}

// The entry point of tests/test_wave_model.py: the five counters {dense batches, sparse batches, events, same-slot
// evaluations, discarded partial events}.
extern "C" int model_lz77(const uint8_t *stream, uint64_t len, int flags, uint32_t *recs_out,
                          uint32_t *chunk_nmatch, uint64_t *stats_out) {
  uint64_t st[kNumStats];
  const int rc = model_lz77_ex(stream, len, flags, recs_out, chunk_nmatch, st, nullptr, nullptr, 0);
  if (stats_out)
    for (int i = 0; i < 5; ++i) stats_out[i] = st[i];
  return rc;
}

extern "C" int model_lz77_mutant(void) { return LZ_MODEL_MUTANT; }
