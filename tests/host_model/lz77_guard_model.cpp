// lz77_guard_model.cpp -- TEST INFRASTRUCTURE.  The progress guard of the wave64 match finder
// (moonbit-flate_amd/csrc/lz77_kernels.hip, lz77_stream) restated on the CPU, so that the rule can be shown never to
// fire on a healthy parser and always to fire on a stalled one BEFORE a kernel with that rule runs on a GPU: a guard
// that misses a stall leaves a wavefront spinning for ever.
//
// The parser is the batch algorithm of lz77_wave_model.cpp (dense multi-event batches, sparse scan batches, same-slot
// groups, both table modes, slot tags) without that file's instrumentation; tests/test_lz77_guard_model.py checks its
// tokens against the oracle too, so that "the guard never fires" is a statement about the kernel's algorithm.
//
// The guard, as the kernel has it:
//   dense : a batch found the parser at s0.  It made no progress if it ends with s == s0, not sparse and not done.
//           (One compare: every other way out of a dense batch raises s, turns sparse or ends the chunk.)
//   sparse: a batch that goes on adds nexist to e_idx; it made no progress if nexist == 0.  (nall == 0 ends the chunk
//           first, and lane 0 is always inside the span, so nall >= 1 gives nexist >= 1.)
// Beside it the model keeps the rule this one replaced -- a snapshot of (s, e_idx, sparse) compared at the head of
// every batch -- and counts the batches on which the two disagree (out[3]; the tests assert zero).
//
// stall_batch = k > 0 is the kernel's test hook (option debug_stall_batch): the k-th dense batch of every chunk
// forgets what it did and leaves the parser exactly as it found it, records and inserts included.
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int kTableSize = 16384;
constexpr int kWin = 65535;
constexpr int kSmallLzMin = 128;
constexpr int kDenseKeep = 61;
constexpr uint32_t kSweepEvery = 20480, kSpanMax = 4096, kMarkerBack = 36864;
constexpr int kMaxLen = 258;
constexpr int kMargin = 15;

inline uint32_t ld32(const uint8_t *p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}
inline uint32_t hash4(uint32_t u) { return (u * 0x1e35a7bdu) >> 18; }
inline uint32_t tag_of(uint32_t u) { return ((u * 0x1e35a7bdu) >> 16) & 3u; }
inline int ctz64(uint64_t m) { return m ? __builtin_ctzll(m) : 64; }
inline uint64_t below(int l) { return l >= 64 ? ~0ull : ((1ull << l) - 1); }
inline uint64_t upto(int l) { return l >= 63 ? ~0ull : ((1ull << (l + 1)) - 1); }

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

}  // namespace

// flags: bit 0 = compat_go, bit 1 = slot tags (guest blocks), bit 2 = MULTI (16-bit modular slots, sweeps, span cut).
// The caller provides 64 readable bytes behind `stream`.
// out[0] dense batches, out[1] sparse batches, out[2] chunks the guard abandoned, out[3] batches on which the guard
// and the snapshot rule it replaced disagree.  Returns the number of chunks.
extern "C" int guard_model_lz77(const uint8_t *stream, uint64_t len, int flags, uint32_t stall_batch, uint32_t *recs_out,
                                uint32_t *chunk_nmatch, uint64_t *out) {
  const int compat_go = flags & 1;
  const bool use_tags = (flags & 2) != 0;
  const bool multi = (flags & 4) != 0;
  std::vector<uint32_t> table(kTableSize, 0);
  std::vector<uint8_t> tags(kTableSize, 0);
  std::vector<uint32_t> scantab;
  {
    uint32_t skip = 32, pos = 0;
    while (pos <= 65535) { scantab.push_back(pos); uint32_t st = skip >> 5; pos += st; skip += st; }
    scantab.push_back(1 << 24);
  }
  uint64_t n_dense = 0, n_sparse = 0, n_fired = 0, n_disagree = 0;
  if (multi)
    for (int i = 0; i < kTableSize; ++i) table[i] = (0u - kMarkerBack + 1u) & 0xffffu;
  uint32_t next_sweep = kSweepEvery;
  auto sweep = [&](uint32_t R) {
    const uint32_t marker = (R - kMarkerBack + 1u) & 0xffffu;
    for (int i = 0; i < kTableSize; ++i) {
      const uint32_t d = (R + 1u - table[i]) & 0xffffu;
      if (d == 0 || d > 32768u) table[i] = marker;
    }
    next_sweep = R + kSweepEvery;
  };
  struct Look { bool inr; uint32_t cand, old; };
  auto lookup = [&](uint32_t A1, uint32_t h) -> Look {
    Look k;
    k.old = table[h];
    const uint32_t dist = multi ? ((A1 - k.old) & 0xffffu) : (A1 - k.old);
    k.inr = (multi ? dist != 0 : k.old != 0) && dist <= 32768u;
    k.cand = A1 - 1u - dist;
    return k;
  };
  auto store = [&](uint32_t h, uint32_t A1, uint32_t cv) {
    table[h] = multi ? (A1 & 0xffffu) : A1;
    tags[h] = (uint8_t)tag_of(cv);
  };

  const uint64_t full = len / kWin, r = len % kWin;
  const uint32_t nchunks = (uint32_t)(full + (r >= kSmallLzMin ? 1 : 0));
  for (uint32_t c = 0; c < nchunks; ++c) {
    const uint32_t W = c * (uint32_t)kWin;
    const int n = (int)((len - W) < (uint64_t)kWin ? (len - W) : kWin);
    const uint8_t *src = stream + W;
    const int s_limit = n - kMargin;
    Rec *recs = reinterpret_cast<Rec *>(recs_out) + (uint64_t)c * 16384;
    uint32_t nm = 0;

    int s = -1;
    bool sparse = false;
    int scan_base = 0, e_idx = 0;
    bool done = false;
    bool fired = false;

    auto cross = [&](uint32_t cand) { return !compat_go && cand + 4 < W; };
    auto extend = [&](int pf, uint32_t cand, int have) -> int {
      int limit = n - pf;
      if (limit > kMaxLen) limit = kMaxLen;
      if (cross(cand)) return 4;
      int l = have;
      const uint8_t *a = src + pf, *b = stream + cand;
      while (l < limit && a[l] == b[l]) ++l;
      return l;
    };
    auto emit = [&](int pf, int total, uint32_t cand) {
      recs[nm].pos = (uint32_t)pf;
      recs[nm].tok = (1u << 30) | ((uint32_t)(total - 3) << 22) | ((W + (uint32_t)pf) - cand - 1);
      ++nm;
    };

    int g_s = -2, g_e = -1;  // the snapshot rule this guard replaced
    bool g_sp = false;
    uint32_t dense_in_chunk = 0;
    bool moved = true;  // the guard's dense half, looked at before the next batch starts
    while (!done) {
      const bool old_rule = s == g_s && e_idx == g_e && sparse == g_sp;
      if (old_rule != !moved) ++n_disagree;
      if (!moved) {
        fired = true;
        break;
      }
      g_s = s, g_e = e_idx, g_sp = sparse;
      if (!sparse) {
        // ----------------------------- dense batch --------------------------------
        ++n_dense;
        const int s0 = s;
        const int e0 = e_idx;
        const uint32_t nm0 = nm;
        const int B = s - 1;
        if (multi) {
          const uint32_t first = W + (uint32_t)(B < 0 ? 0 : B);
          if (first >= next_sweep) sweep(first);
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
          if (use_tags && tags[h[L]] != tag_of(cv[L])) continue;
          const Look k = lookup(A1[L], h[L]);
          cand_abs[L] = k.cand;
          if (k.inr) {
            mlen[L] = common_prefix16(own[L], stream + k.cand);
            if (mlen[L] >= 4) OK |= 1ull << L;
          }
        }
        // same-slot groups: of a two-lane group the later lane, of a larger group every lane
        for (int L = 0; L < 64; ++L) {
          if (!((LD >> L) & 1)) continue;
          uint64_t G = 0;
          for (int M = 0; M < 64; ++M)
            if (((LD >> M) & 1) && h[L] == h[M]) G |= 1ull << M;
          const int size = __builtin_popcountll(G);
          if (size == 2) DUP |= 1ull << (63 - __builtin_clzll(G));
          else if (size > 2) DUP |= G;
        }

        uint64_t INS = 0;
        int a = 0;
        bool batch_over = false;
        while (!batch_over) {
          const uint64_t a_ins = (LD >> a) & 1 ? (1ull << a) : 0;
          uint64_t R = 0;
          if (a + 1 <= 63 && ((LD >> (a + 1)) & 1) && q[a + 1] >= 0) R |= 1ull << (a + 1);
          bool scan_ended = false;
          int consumed = 0;
          for (int e = 0;; ++e) {
            int step;
            const int L = a + 2 + scan_off(e, &step, scantab);
            if (L > 63) break;
            const bool ex = step == 1 ? ((E1 >> L) & 1) : ((E2 >> L) & 1);
            if (!ex) { scan_ended = true; break; }
            R |= 1ull << L;
            consumed = e + 1;
          }
          uint64_t T = 0, rem = R;
          int f = 64;
          uint32_t cand = 0;
          int have = 0;
          for (;;) {
            const int fv = ctz64(OK & rem & ~DUP), fd = ctz64(DUP & rem);
            if (fv < fd) {
              f = fv; cand = cand_abs[fv]; have = mlen[fv];
              T |= rem & upto(fv);
              break;
            }
            if (fd == 64) { T |= rem; break; }
            T |= rem & below(fd);
            uint64_t G = 0;
            for (int L = 0; L < fd; ++L)
              if (((INS | T | a_ins) >> L) & 1 && h[L] == h[fd]) G |= 1ull << L;
            bool v;
            uint32_t cnd;
            int ml;
            if (G) {
              const int i = 63 - __builtin_clzll(G);
              v = cv[i] == cv[fd];
              cnd = W + (uint32_t)q[i];
              ml = common_prefix16(own[fd], own[i]);
            } else {
              v = (OK >> fd) & 1;
              cnd = cand_abs[fd];
              ml = mlen[fd];
            }
            T |= 1ull << fd;
            if (v) { f = fd; cand = cnd; have = ml; break; }
            rem &= ~upto(fd);
          }
          if (f == 64) {
            if (scan_ended) {
              INS |= T | a_ins;
              done = true;
            } else if (a == 0) {  // nothing in this whole batch: continue as a sparse scan
              INS |= T | a_ins;
              sparse = true;
              scan_base = s + 1;
              e_idx = consumed;
            }  // else: partial event at the end of the batch, redone in a new batch
            batch_over = true;
          } else {
            INS |= T | a_ins;
            const int pf = q[f];
            const int total = have < 16 ? (cross(cand) ? 4 : have) : extend(pf, cand, 16);
            emit(pf, total, cand);
            s = pf + total;
            if (s >= s_limit) { done = true; batch_over = true; }
            else {
              a = s - 1 - B;
              if (a > kDenseKeep) batch_over = true;
            }
          }
        }
        // the test hook: this batch forgets what it did
        if (stall_batch != 0 && ++dense_in_chunk == stall_batch) {
          s = s0, e_idx = e0, sparse = false, done = false;
          nm = nm0;
          INS = 0;
        }
        for (int L = 0; L < 64; ++L)  // commit the inserts in position order
          if ((INS >> L) & 1) store(h[L], A1[L], cv[L]);
        moved = (s != s0) | sparse | done;  // ---- the guard's dense half ----
      } else {
        // ----------------------------- sparse batch -------------------------------
        ++n_sparse;
        int p[64], step[64];
        uint64_t EXall = 0, EX = 0;
        for (int L = 0; L < 64; ++L) {
          p[L] = scan_base + scan_off(e_idx + L, &step[L], scantab);
          if (p[L] + step[L] <= s_limit) EXall |= 1ull << L;
        }
        for (int L = 0; L < 64; ++L)
          if (((EXall >> L) & 1) && (!multi || (uint32_t)(p[L] - p[0]) < kSpanMax)) EX |= 1ull << L;
        const int nall = __builtin_popcountll(EXall), nexist = __builtin_popcountll(EX);
        if (nall == 0) break;
        if (multi && W + (uint32_t)p[0] >= next_sweep) sweep(W + (uint32_t)p[0]);
        uint32_t cvs[64], hs[64], A1s[64], olds[64], cands[64];
        uint64_t V = 0;
        for (int L = 0; L < nexist; ++L) {
          cvs[L] = ld32(src + p[L]);
          hs[L] = hash4(cvs[L]);
          A1s[L] = W + (uint32_t)p[L] + 1;
          const Look k = lookup(A1s[L], hs[L]);
          olds[L] = k.old;
          cands[L] = k.cand;
          if (k.inr && ld32(stream + k.cand) == cvs[L]) V |= 1ull << L;
        }
        const int f0 = ctz64(V);
        const int lim = f0 < nexist - 1 ? f0 : nexist - 1;
        bool C = false;
        for (int L = 0; L <= lim && !C; ++L)
          for (int M = 0; M < L; ++M)
            if (hs[L] == hs[M]) { C = true; break; }
        int f = f0;
        uint32_t cand = 0;
        if (!C) {
          for (int L = 0; L <= lim; ++L) store(hs[L], A1s[L], cvs[L]);
          if (f0 < 64) cand = cands[f0];
        } else {  // two lanes of this batch share a slot: replay the batch in order
          f = 64;
          for (int e2 = 0; e2 < nexist; ++e2) {
            const uint32_t cur = table[hs[e2]];
            store(hs[e2], A1s[e2], cvs[e2]);
            bool v = false;
            uint32_t cnd = 0;
            if (cur == olds[e2]) {
              v = (V >> e2) & 1;
              cnd = cands[e2];
            } else {
              for (int i = 0; i < nexist; ++i)
                if ((multi ? (A1s[i] & 0xffffu) : A1s[i]) == cur) {
                  v = cvs[i] == cvs[e2];
                  cnd = A1s[i] - 1u;
                  break;
                }
            }
            if (v) { f = e2; cand = cnd; break; }
          }
        }
        if (f == 64) {
          if (nexist == nall && nall < 64) break;  // the scan ran into s_limit
          if (nexist == 0) {  // ---- the guard's sparse half ----
            fired = true;
            break;
          }
          e_idx += nexist;
          continue;
        }
        const int pf = p[f];
        const int total = extend(pf, cand, 4);
        emit(pf, total, cand);
        s = pf + total;
        sparse = false;
        if (s >= s_limit) done = true;
      }
    }
    if (fired) ++n_fired;
    chunk_nmatch[c] = nm;
  }
  if (out) {
    out[0] = n_dense;
    out[1] = n_sparse;
    out[2] = n_fired;
    out[3] = n_disagree;
  }
  return (int)nchunks;
}
