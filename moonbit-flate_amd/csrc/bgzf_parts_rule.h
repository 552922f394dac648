// bgzf_parts_rule.h -- a BGZF file read and written in PARTS (flate_hip_bgzf_reader_* / flate_hip_bgzf_writer_*), what
// a call decides, written ONCE: plain C++17 without HIP, compiled into the kernels (bgzf_parts_kernels.hip), into the
// library's host code and into tests/host_model/bgzf_parts_rule_model.cpp, which compares it with
// tests/bgzf_parts_ref.py.
//
// A reader's call is flate_hip_bgzf_read's discovery over the part in[0, in_len) of the file.  Between two calls the
// reader stands at a member boundary, always: a member is at most 65536 bytes, so the bytes of a member that a part
// cuts are simply left unused.  This file holds the stop behind a part's last whole member, which members a call
// delivers, what the handle remembers, the result words of a failure counted over the FILE, the writer's block count
// and the arguments.
#pragma once

#include <stdint.h>

#include "bgzf_rule.h"

namespace flate {

// THE PART STOP.  p: the offset where the serial walk over in[0, in_len) finds no member (bgzf_member_total == 0);
// avail = in_len - p.  A member's total is at most kBgzfMemberMax, so behind that many bytes no continuation of the
// file can put a member at p; with fewer nothing is wrong yet.  The rule is coarse on purpose: no "could this prefix
// still become a header" test.  Every cut gives the same bytes and the same final verdict; a malformed file is only
// reported one call later.  A part of at least kBgzfMemberMax bytes, or a final one, therefore always makes progress
// (p > 0, or the call delivers) or gives a verdict.
constexpr uint32_t kBgzfPartBoundary = 0;  // avail == 0: the part ends where a member does
constexpr uint32_t kBgzfPartStop = 1;      // nothing is wrong yet: the next part begins at p
constexpr uint32_t kBgzfPartCorrupt = 2;   // no member can stand at p
BGZF_HD uint32_t bgzf_part_stop(uint64_t avail, bool final_in) {
  if (avail == 0) return kBgzfPartBoundary;
  if (final_in || avail >= (uint64_t)kBgzfMemberMax) return kBgzfPartCorrupt;
  return kBgzfPartStop;
}

// DELIVERY.  Of the n whole members in front of p a call delivers the longest prefix k whose output fits out_cap and
// whose k + 1 index entries fit index_cap (k_max = index_cap - 1, or 0xffffffff without arrays).  out_end: where member
// i's output ends, out_off[i + 1]; the sums rise, so "member i is delivered" is a prefix of the members.  Empty members
// are delivered as far as they go.
BGZF_HD bool bgzf_part_delivers(uint32_t i, uint64_t out_end, uint64_t out_cap, uint32_t k_max) {
  return out_end <= out_cap && i < k_max;
}
BGZF_HD uint32_t bgzf_part_k_max(bool with_index, uint64_t index_cap) {
  if (!with_index) return 0xffffffffu;
  return index_cap - 1u > 0xfffffffeull ? 0xffffffffu : (uint32_t)(index_cap - 1u);  // (index_cap >= 1: the arguments)
}

// ---- what the handle remembers: a few host words ----
struct BgzfPartsState {
  uint64_t consumed;    // file bytes used so far: the sum of *in_used
  uint64_t produced;    // output bytes delivered so far
  uint32_t members;     // members delivered so far
  uint32_t eof_marker;  // the last delivered member was the canonical marker
  int32_t status;       // sticky: 0, the file's end (1) or the file's error, with the two words below
  uint32_t bad_member;
  int64_t err_off;
};
inline BgzfPartsState bgzf_parts_fresh() { return BgzfPartsState{0, 0, 0, 0, 0, 0xffffffffu, -1}; }

// ---- what the discovery over a part found (the device's result words) ----
struct BgzfPartFound {
  uint32_t n;         // whole members in front of p
  uint32_t k;         // of them delivered (DELIVERY)
  uint32_t stop;      // THE PART STOP at p
  uint32_t eof_last;  // k >= 1: member k - 1 is the canonical marker
  uint64_t p;         // part-relative
  uint64_t in_end;    // member_off[k], part-relative: where the delivered members end
  uint64_t out_end;   // out_off[k]: what they inflate to
  uint64_t isize0;    // n >= 1: ISIZE of member 0
};

constexpr int kBgzfPartsOk = 0, kBgzfPartsEnd = 1, kBgzfPartsOutTooSmall = -2, kBgzfPartsCorrupt = -4, kBgzfPartsInvalid = -1;

// THE CALL, before any member is decoded: its status if every delivered member decodes, its words and the state
// behind it.  decode: members 0 .. k - 1 of the part are to be decoded into out[0, out_len).
struct BgzfPartCall {
  int status;         // kBgzfPartsOk: call again; kBgzfPartsEnd; kBgzfPartsOutTooSmall (repeatable); kBgzfPartsCorrupt (sticky)
  uint32_t decode;    // members to decode
  uint64_t in_used, out_len;
  BgzfPartsState next;
};
inline BgzfPartCall bgzf_parts_call(const BgzfPartsState &s, const BgzfPartFound &f, uint64_t in_len, bool final_in) {
  BgzfPartCall c{kBgzfPartsOk, f.k, f.in_end, f.out_end, s};
  if (f.k == 0 && f.n >= 1) {  // not even the first member fits: repeatable, nothing changes
    c.status = kBgzfPartsOutTooSmall, c.in_used = 0, c.out_len = f.isize0;
    return c;
  }
  BgzfPartsState &t = c.next;
  t.produced += f.out_end;
  t.members += f.k;
  if (f.k) t.eof_marker = f.eof_last;
  if (f.k == f.n && f.stop == kBgzfPartCorrupt) {  // the good members in front, then the file's error
    c.status = kBgzfPartsCorrupt, c.in_used = 0;
    t.status = kBgzfPartsCorrupt, t.bad_member = t.members, t.err_off = (int64_t)(s.consumed + f.p);
    return c;
  }
  t.consumed += f.in_end;
  if (final_in && f.k == f.n && f.in_end == in_len) c.status = t.status = kBgzfPartsEnd;
  return c;
}
// ... and behind the decode, when member j of the part (j < c.decode) is the first whose status is not 0: the members
// in front of it are delivered (out_off_j bytes), the file's error is sticky, nothing is used.
inline void bgzf_parts_fail(const BgzfPartsState &s, BgzfPartCall &c, uint32_t j, int status, uint64_t member_off_j,
                            uint64_t out_off_j, bool eof_before) {
  c.status = status, c.in_used = 0, c.out_len = out_off_j;
  c.next = s;
  c.next.produced += out_off_j;
  c.next.members += j;
  if (j) c.next.eof_marker = eof_before ? 1u : 0u;
  c.next.status = status, c.next.bad_member = s.members + j, c.next.err_off = (int64_t)(s.consumed + member_off_j);
}

// ---- the writer: the blocks a call compresses ----
// Not final: the whole blocks the part holds; final: everything, the last block as short as it is.
BGZF_HD uint64_t bgzf_writer_blocks(uint64_t in_len, uint32_t bb, bool final_in) {
  return in_len / bb + ((final_in && in_len % bb) ? 1u : 0u);
}
BGZF_HD uint64_t bgzf_writer_in_used(uint64_t in_len, uint32_t bb, bool final_in) {
  return final_in ? in_len : in_len / bb * bb;
}

// ---- the arguments (api_checks.h hands them on); bb: bgzf_block_bytes, 0 = refused ----
inline int bgzf_parts_reader_open_args(const void *ctx, uint32_t flags, uint32_t device_ptrs, const void *r) {
  return (!ctx || !r || (flags & ~device_ptrs)) ? kBgzfPartsInvalid : kBgzfPartsOk;
}
inline int bgzf_parts_reader_read_args(const void *r, const void *in, uint64_t in_len, const void *out, uint64_t out_cap,
                                       const void *in_used, const void *out_len, uint64_t index_cap, const void *member_off,
                                       const void *out_off) {
  if (!r || !in_used || !out_len || (in_len && !in) || (out_cap && !out)) return kBgzfPartsInvalid;
  if (!member_off != !out_off) return kBgzfPartsInvalid;
  if (member_off && index_cap == 0) return kBgzfPartsInvalid;
  return kBgzfPartsOk;
}
inline int bgzf_parts_writer_open_args(const void *ctx, uint32_t bb, uint32_t flags, uint32_t allowed, const void *w) {
  return (!ctx || !w || !bb || (flags & ~allowed)) ? kBgzfPartsInvalid : kBgzfPartsOk;
}
inline int bgzf_parts_writer_write_args(const void *w, const void *in, uint64_t in_len, const void *out, const void *in_used,
                                        const void *out_len, bool ended) {
  if (!w || !out || !in_used || !out_len || (in_len && !in) || ended) return kBgzfPartsInvalid;
  return kBgzfPartsOk;
}

}  // namespace flate
