// zip_kernels.hip -- ZIP archives on the device (flate_hip_zip_write / _index / _read; the format is zip_rule.h, the
// parameter blocks zip_kernels.h).  Every kernel equals the rule's serial functions on every input.
//
// WRITING (behind huff_code_kernel, around the pack kernels, as frame_kernels.hip does for zlib and gzip members):
//   zip_scan_kernel     one workgroup: the exclusive scan of 30 + name + raw size (scan_range of block_scan.h): the local
//                       header offsets, the payload offsets the pack kernels write at, k0, the directory's place and
//                       size in closed form, the total against out_cap (scan_sizes_kernel's status word)
//   zip_write_kernel    behind the pack kernel and the CRC-32s: thread i < n writes entry i's local header and its central
//                       record (whose place is zip_central_place), thread n the end records; byte stores, a header
//                       starts at any alignment
// READING, the end record:
//   zip_end_find_kernel one thread per offset of the tail window: signature and p + 22 + comment == in_len, atomic max
//   zip_end_read_kernel one thread: the rule at that offset (zip_end_read): n, the directory's range, or the verdict
// READING, the directory (the host knows its range by now): the skeleton of chain_walk.h (flate_kernels.h: THE
// DISCOVERY SKELETON) over tiles that count from cd_off, the candidates' offsets counted from cd_off too:
//   zip_dir_count_kernel / zip_dir_fill_kernel   the offset test: the signature in LDS, the record rule on the rare hit
//                       inside the directory; a hit stores cand_off and cand_total
//   zip_dir_scan_kernel the shared scan, and this format's own head
//   bgzf_link_kernel    (bgzf_kernels.hip) over the directory as a file of cd_size bytes: a record ends at cand_off +
//                       cand_total, the last one at cd_size
//   zip_entry_kernel    one thread per rank: the record and its local header -> the entry (zip_entry_make); the threads
//                       at rank n and at the chain's end write the archive's verdict
//   zip_out_scan_kernel one workgroup: out_off = the exclusive scan of size over the entries with status 0
// READING, around the decoders (one thread per selected entry, except the copy):
//   zip_prep_kernel     behind the decoders: stored entries and entries with an index status get their length and status
//   zip_copy_kernel     stored entries, one workgroup per piece of at most 64 KiB: 16-byte stores on the destination's
//                       grid, the source read at its own alignment, heads and tails byte by byte
//   zip_verdict_kernel  behind the CRC-32s of what was produced: the entry's verdict
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "zip_kernels.h"
#include "zip_rule.h"

namespace flate {

// ---- writing ----

__global__ __launch_bounds__(1024) void zip_scan_kernel(ZipWriteParams P) {
  __shared__ uint64_t wtot[16];
  __shared__ uint32_t k0_s;
  if (threadIdx.x == 0) k0_s = P.n;
  __syncthreads();
  const uint64_t sum = scan_range<16, uint64_t>(
      P.n, wtot, [&](uint32_t i) { return P.out_len[i] + kZipLocalLen + (P.name_off[i + 1] - P.name_off[i]); },
      [&](uint32_t i, uint64_t at, uint64_t) {
        P.entry_off[i] = at;
        P.payload_off[i] = at + kZipLocalLen + (P.name_off[i + 1] - P.name_off[i]);
        if (zip_central_has_extra(at)) atomicMin(&k0_s, i);
      });
  __syncthreads();  // (k0_s is final)
  if (threadIdx.x == 0) {
    P.entry_off[P.n] = sum;
    P.payload_off[P.n] = sum;
    ZipWriteHead h;
    h.cd_off = sum;
    h.k0 = k0_s, h.pad = 0;
    h.cd_size = zip_central_place(P.n, P.name_off[P.n] - P.name_off[0], k0_s);
    h.total = sum + h.cd_size + zip_end_len(P.n, sum, h.cd_size);
    *P.head = h;
    if (h.total > P.out_cap) *P.status = FLATE_HIP_E_OUT_TOO_SMALL;
  }
}

__global__ __launch_bounds__(256) void zip_write_kernel(ZipWriteParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (*P.status != 0 || i > P.n) return;  // (a status: the scan found the output too small -- nothing may be written)
  const ZipWriteHead h = *P.head;
  if (h.total > P.out_cap) return;  // (never: the scan has checked it)
  if (i == P.n) {
    zip_put_end(P.out + h.cd_off + h.cd_size, P.n, h.cd_off, h.cd_size);
    return;
  }
  const uint64_t at = P.entry_off[i];
  const uint32_t nl = (uint32_t)(P.name_off[i + 1] - P.name_off[i]);
  const uint8_t *name = P.names + P.name_off[i];
  uint32_t raw, size;
  if (P.group_off) {
    raw = (uint32_t)(P.entry_off[i + 1] - P.payload_off[i]);
    size = (uint32_t)(P.in_off[P.group_off[i + 1]] - P.in_off[P.group_off[i]]);
  } else {
    raw = (uint32_t)P.out_len[i], size = (uint32_t)(P.in_off[i + 1] - P.in_off[i]);
  }
  zip_put_local(P.out + at, name, nl, P.sums[i], raw, size);
  zip_put_central(P.out + h.cd_off + zip_central_place(i, P.name_off[i] - P.name_off[0], h.k0), name, nl, P.sums[i], raw, size, at);
}

// ---- reading: the end record ----

__global__ __launch_bounds__(256) void zip_end_find_kernel(const uint8_t *in, uint64_t in_len, ZipEndHead *head) {
  const uint64_t p = zip_tail_lo(in_len) + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (in_len < kZipEndLen || p > in_len - kZipEndLen) return;
  if (zip_end_candidate(in, in_len, p)) atomicMax((unsigned long long *)&head->end_p1, (unsigned long long)(p + 1u));
}

__global__ void zip_end_read_kernel(const uint8_t *in, uint64_t in_len, ZipEndHead *head) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ZipEndHead h = *head;
  h.n = h.cd_off = h.cd_size = h.rec_off = 0, h.zip64 = 0;
  h.rc = FLATE_HIP_E_CORRUPT, h.err_off = (int64_t)in_len;
  if (h.end_p1) {
    ZipEnd E;
    h.rc = zip_end_read(in, in_len, h.end_p1 - 1u, &E);
    h.err_off = h.rc ? (int64_t)(h.end_p1 - 1u) : -1;
    if (!h.rc) h.n = E.n, h.cd_off = E.cd_off, h.cd_size = E.cd_size, h.rec_off = E.rec_off, h.zip64 = E.zip64;
  }
  *head = h;
}

// ---- reading: the directory ----

namespace {

// the first tile's virtual position (virtual position = file offset + A: multiples of 16 are aligned addresses)
__device__ inline uint64_t tiles_base(const ZipDirParams &P, uint32_t A) { return (P.cd_off + A) & ~15ull; }

// this thread's 16 offsets: bit b of the result = a record can be read at virtual position v0 + 16 * tid + b (inside
// the directory); totals[k]: the length of the k-th of them (two signatures are 4 bytes apart: at most 4 in 16)
__device__ inline uint32_t test_offsets(const ZipDirParams &P, const uint8_t *lds, uint64_t v0, uint32_t A, uint32_t *totals) {
  uint32_t hits = 0, k = 0;
  const uint32_t at = 16u * threadIdx.x;
  const uint64_t cd_end = P.cd_off + P.cd_size;
  for (uint32_t b = 0; b < 16u; ++b) {
    if (!zip_sig(lds + at + b, 1, 2)) continue;
    const uint64_t v = v0 + at + b;
    if (v < A) continue;
    const uint64_t p = v - A;
    if (p < P.cd_off || p >= cd_end) continue;
    ZipCentral R;
    const uint32_t t = zip_central_read(P.C.in + p, cd_end - p, &R);
    if (t && k < 4u) hits |= 1u << b, totals[k++] = t;
  }
  return hits;
}

}  // namespace

__global__ __launch_bounds__(256) void zip_dir_count_kernel(ZipDirParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = tiles_base(P, A) + (uint64_t)blockIdx.x * kTileBytes;
  uint32_t totals[4];
  tile_count(P.C, L, v0, [&](const uint8_t *lds) { return (uint32_t)__popc(test_offsets(P, lds, v0, A, totals)); });
}

// One workgroup: tile_cnt becomes its exclusive scan (n_tiles + 1 entries); both heads are initialised.
__global__ __launch_bounds__(1024) void zip_dir_scan_kernel(ZipDirParams P) {
  __shared__ uint64_t wtot[16];
  tile_scan(P.C, wtot, 0);
  if (threadIdx.x == 0) {
    ZipDirHead h;  // (what stands when not even cd_off holds a record)
    h.out_bytes = 0, h.err_off = (int64_t)P.cd_off, h.n_entries = 0, h.rc = FLATE_HIP_E_CORRUPT;
    *P.head = h;
  }
}

__global__ __launch_bounds__(256) void zip_dir_fill_kernel(ZipDirParams P) {
  __shared__ TileLds L;
  const uint32_t A = tile_align(P.C.in);
  const uint64_t v0 = tiles_base(P, A) + (uint64_t)blockIdx.x * kTileBytes;
  uint32_t first, totals[4];
  if (!tile_fill_load(P.C, L, v0, false, &first)) return;
  const uint32_t hits = test_offsets(P, L.bytes, v0, A, totals);
  tile_put16(hits, tile_fill_at(L, first, (uint32_t)__popc(hits)), P.C.cap, [&](uint32_t i, uint32_t b, uint32_t k) {
    P.C.cand_off[i] = v0 + 16u * threadIdx.x + b - A - P.cd_off;
    P.cand_total[i] = totals[k];
  });
}

// One thread per rank of the chain from cd_off.  L = the chain's records; the serial walk reads min(L, n) of them and
// then stops: at the n-th record's end (which must be the directory's), or where the chain does.
__global__ __launch_bounds__(256) void zip_entry_kernel(ZipDirParams P) {
  const uint32_t nc = P.C.head->n_cand;
  if (nc > P.C.cap) return;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= P.C.path_len) return;  // (the last entry is a sink)
  const uint32_t c = P.C.path[r];
  if (c >= nc) return;
  const uint64_t off = P.cd_off + P.C.cand_off[c];
  const uint32_t total = P.cand_total[c];
  ZipDirHead *h = P.head;
  if (r == P.n) {  // a record where the directory should have ended: bytes left behind n records
    h->rc = FLATE_HIP_E_CORRUPT, h->err_off = (int64_t)off, h->n_entries = P.n;
    return;
  }
  if (r > P.n) return;
  if (r < P.ent_cap) {
    ZipCentral R;
    (void)zip_central_read(P.C.in + off, P.cd_off + P.cd_size - off, &R);  // (a candidate: it reads)
    zip_entry_make(P.C.in, P.cd_off, off, R, P.entries + r);
  }
  const uint32_t succ = P.C.path[r + 1u];  // (path_len >= cap + 2: r + 1 is inside the path)
  if (succ < nc) return;
  // the chain's last record, L = r + 1 <= n: one thread gets here
  h->n_entries = r + 1u;
  if (r + 1u == P.n && succ == nc) {
    h->rc = FLATE_HIP_OK, h->err_off = -1;
  } else {
    h->rc = FLATE_HIP_E_CORRUPT, h->err_off = (int64_t)(off + total);
  }
}

__global__ __launch_bounds__(1024) void zip_out_scan_kernel(ZipDirParams P) {
  __shared__ uint64_t wtot[16];
  if (P.C.head->n_cand > P.C.cap || P.head->rc != 0) return;  // (uniform)
  const uint32_t hi = P.head->n_entries;                    // (= n <= ent_cap)
  const uint64_t total = scan_range<16, uint64_t>(
      hi, wtot, [&](uint32_t i) { return P.entries[i].status == 0 ? P.entries[i].size : 0ull; },
      [&](uint32_t i, uint64_t before, uint64_t) { P.C.out_off[i] = before; });
  if (threadIdx.x == 0) {
    P.C.out_off[hi] = total;
    P.head->out_bytes = total;
  }
}

// ---- reading: around the decoders ----

// Behind the decoders (which ran over empty ranges for every entry that is not theirs): what the checksum plan and the
// verdict read for the others.
__global__ __launch_bounds__(256) void zip_prep_kernel(ZipReadParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_sel) return;
  const ZipSel s = P.sel[j];
  P.bad[j] = s.status != 0 ? 1u : 0u;
  if (s.status != 0) {
    P.out_len[j] = 0, P.status[j] = s.status, P.err_off[j] = -1;
  } else if (s.method == 0 || !P.decoded) {
    P.out_len[j] = s.method == 0 ? s.size : 0ull, P.status[j] = 0, P.err_off[j] = -1;
  }
}

// One workgroup per piece: out[dst, dst + len) = in[src, src + len).
__global__ __launch_bounds__(256) void zip_copy_kernel(ZipReadParams P) {
  const ZipCopyPiece pc = P.pieces[blockIdx.x];
  uint8_t *d = P.out + pc.dst;
  const uint8_t *s = P.in + pc.src;
  uint32_t head = (uint32_t)((16u - (reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
  if (head > pc.len) head = pc.len;
  const uint32_t chunks = (pc.len - head) / 16u, tail = head + 16u * chunks;
  if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
  for (uint32_t ch = threadIdx.x; ch < chunks; ch += 256u) {
    uint4 w;
    __builtin_memcpy(&w, s + head + 16u * ch, 16);  // (the source at its own alignment)
    *reinterpret_cast<uint4 *>(d + head + 16u * ch) = w;
  }
  if (threadIdx.x < pc.len - tail) d[tail + threadIdx.x] = s[tail + threadIdx.x];
}

__global__ __launch_bounds__(256) void zip_verdict_kernel(ZipReadParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_sel) return;
  const ZipSel s = P.sel[j];
  if (s.status != 0 || P.status[j] != 0) return;  // the index status (zip_prep_kernel), or the decoder's own
  if (P.out_len[j] != s.size || P.sums[j] != s.crc) {
    P.status[j] = FLATE_HIP_E_CORRUPT;
    P.err_off[j] = (int64_t)s.comp_size;
  }
}

}  // namespace flate
