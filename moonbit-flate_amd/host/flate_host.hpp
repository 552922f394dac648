// flate_host.hpp -- header-only C++ mirror of the reference's host API over the C ABI
// (include/flate_hip.h).  Names, argument meaning and error behaviour follow the reference:
//   Writer::new / write / close          writer.mbt:10,45,53
//   Compressor sticky errors             deflate.mbt:74,154-183,280-294
//   writer_closed_error                  deflate.mbt:154
//   &Reader::new / read / close, ioeof    inflate.mbt:305,382,410,19
//   corrupt_input_error                   inflate.mbt:38
// The reference is single-stream and synchronous: Compressor::write compresses every full
// 65535-byte window as soon as it is there and the sink sees the bytes (deflate.mbt:280-294,
// huffman-bit-writer.mbt:193-196).  Writer does the same through flate_hip_stream_write: write()
// calls are staged (the output is a function of the concatenated bytes only, deflate.mbt:222-229),
// and whenever `emit_windows` full windows are pending they are compressed and their finished bytes
// go to the sink -- memory stays bounded and output leaves before close().  BatchWriter (below) closes
// many Writers with one kernel pipeline -- the intended way to use the engine -- and a Writer built
// with chunk_bytes > 0 cuts ONE large stream into independent chunks that the GPU compresses in
// parallel and splices into one legal DEFLATE stream (different bytes than a single
// Writer would produce, same inflated result).
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "flate_hip.h"

namespace flate_host {

struct IOError {  // @io.IOError
  std::string msg;
  bool operator==(const IOError &o) const { return msg == o.msg; }
};
using Err = std::optional<IOError>;

inline const IOError &writer_closed_error() {  // deflate.mbt:154
  static const IOError e{"writer closed"};
  return e;
}

// &@io.Writer
struct ByteSink {
  virtual ~ByteSink() = default;
  virtual std::pair<int, Err> write(const uint8_t *p, size_t n) = 0;
};

// @io.Buffer used as in-memory sink
struct Buffer : ByteSink {
  std::vector<uint8_t> bytes;
  std::pair<int, Err> write(const uint8_t *p, size_t n) override {
    bytes.insert(bytes.end(), p, p + n);
    return {(int)n, std::nullopt};
  }
};

// One GPU context (flate_hip_ctx).  No GPU => construction reports the error; there is no CPU path.
class Engine {
 public:
  explicit Engine(int device = 0) { rc_ = flate_hip_init(device, &ctx_); }
  ~Engine() { flate_hip_destroy(ctx_); }
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;
  bool ok() const { return rc_ == 0; }
  int status() const { return rc_; }
  flate_hip_ctx *ctx() const { return ctx_; }
  // flate_hip_set_option: e.g. ("one_stored_units", 1) so that stored block headers start units too
  // ... or ("zip_unit_min", 1 << 20) so that flate_hip_zip_read decodes long entries in parallel through units
  int set_option(const char *name, int64_t value) { return flate_hip_set_option(ctx_, name, value); }
  // flate_hip_zip_last_route: what the last ZIP read on this engine did with "zip_unit_min"
  struct ZipRoute {
    uint32_t unit_entries = 0, fallback_entries = 0, n_units = 0, n_candidates = 0;
  };
  ZipRoute zip_last_route() const {
    ZipRoute r;
    (void)flate_hip_zip_last_route(ctx_, &r.unit_entries, &r.fallback_entries, &r.n_units, &r.n_candidates);
    return r;
  }
  // ... or ("gzfile_serial_max", 1 << 20) so that flate_hip_gzfile_index / _read take short members whole
  // flate_hip_gzfile_last_route: what the last index_gzfile / decompress_gzfile on this engine did with it
  struct GzFileRoute {
    uint32_t serial_members = 0, unit_members = 0;
    uint64_t find_from = 0;
  };
  GzFileRoute gzfile_last_route() const {
    GzFileRoute r;
    (void)flate_hip_gzfile_last_route(ctx_, &r.serial_members, &r.unit_members, &r.find_from);
    return r;
  }

 private:
  flate_hip_ctx *ctx_ = nullptr;
  int rc_ = 0;
};

inline Err make_error(const Engine &e, int rc) {
  std::string m = std::string("flate_hip: ") + flate_hip_strerror(rc);
  const char *h = e.ctx() ? flate_hip_last_hip_error(e.ctx()) : "";
  if (h && *h) m += std::string(" [") + h + "]";
  return IOError{m};
}

// Compress `streams` (each with fresh-Writer semantics) in one batch; out[i] = stream i's bytes.
inline Err compress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                          std::vector<std::vector<uint8_t>> &out, uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0);
  uint64_t cap = 16;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    cap += flate_hip_deflate_bound(streams[i].size());
  }
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const int rc = flate_hip_deflate_fast_batch(e.ctx(), in.data(), in_off.data(), n, buf.data(), cap,
                                              out_off.data(), flags);
  if (rc != 0) return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) out[i].assign(buf.begin() + out_off[i], buf.begin() + out_off[i + 1]);
  return std::nullopt;
}

// &Reader::new_dict(r, dict) (inflate.mbt:315-317) in batch form (flate_hip_inflate_batch_dict): dicts[j] is a
// preset dictionary (only its last 32768 bytes are history), dict_of[i] the dictionary of stream i or
// FLATE_HIP_NO_DICT; an empty dict_of: every stream uses dicts[0].  The encode side (compress_batch with a
// DictTable, BatchWriter) takes the same table: flate_hip_deflate_fast_batch_dict.
struct DictTable {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off;
  explicit DictTable(const std::vector<std::vector<uint8_t>> &dicts) : off(dicts.size() + 1, 0) {
    for (size_t j = 0; j < dicts.size(); ++j) off[j + 1] = off[j] + dicts[j].size();
    bytes.resize(off.back() + 16);
    for (size_t j = 0; j < dicts.size(); ++j) std::copy(dicts[j].begin(), dicts[j].end(), bytes.begin() + off[j]);
  }
};

// compress_batch with preset dictionaries as HISTORY (flate_hip_deflate_fast_batch_dict): stream i is written as
// if its Writer had seen dictionary dict_of[i] without producing output, and is read back by
// Reader::new_dict / decompress_batch with the same dictionary.  FLATE_HIP_COMPAT_GO is the mode in which
// matches extend into the dictionary (include/flate_hip.h).
inline Err compress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams, const DictTable &D,
                          const std::vector<uint32_t> &dict_of, std::vector<std::vector<uint8_t>> &out,
                          uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  if (!dict_of.empty() && dict_of.size() != n) return make_error(e, FLATE_HIP_E_INVALID);
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0);
  uint64_t cap = 16;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    cap += flate_hip_deflate_bound(streams[i].size());
  }
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const int rc = flate_hip_deflate_fast_batch_dict(e.ctx(), in.data(), in_off.data(), n, D.bytes.data(), D.off.data(),
                                                   (uint32_t)D.off.size() - 1, dict_of.empty() ? nullptr : dict_of.data(),
                                                   buf.data(), cap, out_off.data(), flags);
  if (rc != 0) return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) out[i].assign(buf.begin() + out_off[i], buf.begin() + out_off[i + 1]);
  return std::nullopt;
}

// The container formats around a raw stream (the reference has neither): zlib (RFC 1950: CMF, FLG,
// data, Adler-32 big endian) and gzip (RFC 1952: ten header bytes, data, CRC-32 and length little endian).
// Members are WRITTEN on the GPU (flate_hip_deflate_fast_batch_framed); reading them -- parsing the header, checking the
// trailer against flate_hip_checksum_batch -- is done here.
enum class Wrap { Raw, Zlib, Gzip };

inline Err checksum_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams, uint32_t kind,
                          std::vector<uint32_t> &sums) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  std::vector<uint64_t> in_off(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + streams[i].size();
  std::vector<uint8_t> in(in_off[n] + 1);
  for (uint32_t i = 0; i < n; ++i) std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  sums.assign(n, 0);
  const int rc = flate_hip_checksum_batch(e.ctx(), in.data(), in_off.data(), n, kind, sums.data(), 0);
  if (rc != 0) return make_error(e, rc);
  return std::nullopt;
}

inline uint32_t wrap_code(Wrap w) {
  return w == Wrap::Zlib ? FLATE_HIP_WRAP_ZLIB : w == Wrap::Gzip ? FLATE_HIP_WRAP_GZIP : FLATE_HIP_WRAP_RAW;
}

// compress_batch with every stream inside its container: ONE call (flate_hip_deflate_fast_batch_framed) -- the input
// crosses the link once, the checksums run on the device copy, headers and trailers are written there, and the
// members come back in one piece.  D (may be null; zlib only): preset dictionaries as in compress_batch with a
// DictTable; a member whose stream names one carries FDICT and the dictionary's Adler-32 as DICTID.
inline Err compress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams, const DictTable *D,
                          const std::vector<uint32_t> &dict_of, std::vector<std::vector<uint8_t>> &out, Wrap wrap,
                          uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  if (!dict_of.empty() && (!D || dict_of.size() != n)) return make_error(e, FLATE_HIP_E_INVALID);
  const uint32_t w = wrap_code(wrap);
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0);
  uint64_t cap = 16;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    cap += flate_hip_deflate_bound(streams[i].size()) + flate_hip_frame_overhead(w, D != nullptr);
  }
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const int rc = flate_hip_deflate_fast_batch_framed(
      e.ctx(), in.data(), in_off.data(), n, w, D ? D->bytes.data() : nullptr, D ? D->off.data() : nullptr,
      D ? (uint32_t)D->off.size() - 1 : 0u, dict_of.empty() ? nullptr : dict_of.data(), buf.data(), cap, out_off.data(),
      flags);
  if (rc != 0) return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) out[i].assign(buf.begin() + out_off[i], buf.begin() + out_off[i + 1]);
  return std::nullopt;
}
inline Err compress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                          std::vector<std::vector<uint8_t>> &out, Wrap wrap, uint32_t flags = 0) {
  return compress_batch(e, streams, nullptr, {}, out, wrap, flags);
}

inline Err compress_spliced(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                            std::vector<uint8_t> &out, std::vector<uint64_t> *bit_off, uint32_t flags);

// Writer (writer.mbt:2-15): write() appends to the stream, close() emits the DEFLATE bytes to the
// sink given at construction.  Sticky error rules of Compressor (deflate.mbt:157-183,280-294).
// chunk_bytes == 0 (default): the bytes a reference Writer produces, bit for bit.
// chunk_bytes  > 0 (opt-in): the stream is cut into independent chunks of that many
// bytes, each compressed as a fresh Writer would (no matches across chunk borders), all chunks in
// one GPU batch, and emitted as ONE spliced DEFLATE stream.  Any inflater reads it back to the
// same bytes, but it is NOT the byte sequence of a single Writer -- a one-wavefront stream gets no
// parallelism on the GPU, this mode does.
class Writer {
 public:
  static constexpr size_t kWindow = 65535;  // max_store_block_size, deflate-fast.mbt:46
  // emit_windows: full windows staged before they are compressed and handed to the sink (16 = 1 MiB)
  Writer(ByteSink &w, Engine &e, uint32_t flags = 0, size_t chunk_bytes = 0, size_t emit_windows = 16)
      : w_(w), e_(e), flags_(flags), chunk_(chunk_bytes), emit_(emit_windows ? emit_windows : 1) {}
  // Writer::new_dict(w, dict) (writer.mbt:25-31) AS THE REFERENCE BEHAVES: fill_window
  // (deflate.mbt:108-151) copies the last window_size = 32768 bytes of the dictionary into the input
  // window and sets window_end, i.e. they are unprocessed DATA -- the stream is the one Writer::new
  // produces when those bytes are written first (the reference's own test asserts exactly that
  // equality, deflate_test.mbt:12-35).  Go ignores the dictionary at this level.
  // (A dictionary as HISTORY, which the stream then needs to be read: BatchWriter with a DictTable.)
  static std::unique_ptr<Writer> new_dict(ByteSink &w, Engine &e, const uint8_t *dict, size_t n, uint32_t flags = 0) {
    std::unique_ptr<Writer> wr(new Writer(w, e, flags));
    constexpr size_t kDictWindow = 32768;  // window_size, deflate.mbt:12
    if (n > kDictWindow) {
      dict += n - kDictWindow;
      n = kDictWindow;
    }
    wr->pending_.assign(dict, dict + n);
    return wr;
  }
  ~Writer() { flate_hip_stream_free(st_); }
  Writer(const Writer &) = delete;
  Writer &operator=(const Writer &) = delete;

  std::pair<int, Err> write(const uint8_t *p, size_t n) {  // deflate.mbt:280-294
    if (err_) return {0, err_};
    pending_.insert(pending_.end(), p, p + n);
    if (chunk_ == 0 && !batch_member_ && pending_.size() >= emit_ * kWindow) {
      const size_t k = pending_.size() / kWindow * kWindow;  // every full window that is there
      if (Err er = feed(k, false)) {
        err_ = er;
        return {0, err_};
      }
    }
    return {(int)n, std::nullopt};
  }
  std::pair<int, Err> write(const std::vector<uint8_t> &b) { return write(b.data(), b.size()); }

  Err close() {  // deflate.mbt:157-183
    if (err_ && *err_ == writer_closed_error()) return std::nullopt;
    if (err_) return err_;
    Err er;
    if (chunk_ > 0 && pending_.size() > chunk_) {
      std::vector<std::vector<uint8_t>> parts;
      std::vector<uint8_t> one;
      for (size_t o = 0; o < pending_.size(); o += chunk_)
        parts.emplace_back(pending_.begin() + o, pending_.begin() + std::min(pending_.size(), o + chunk_));
      er = compress_spliced(e_, parts, one, nullptr, flags_);
      if (!er) {
        auto r = w_.write(one.data(), one.size());
        er = r.second;
      }
    } else {
      er = feed(pending_.size(), true);  // the rest (any length) + Writer::close's block
    }
    if (er) {
      err_ = er;
      return err_;
    }
    err_ = writer_closed_error();
    return std::nullopt;
  }
  // compressed bytes handed to the sink so far (before close(): the pieces already emitted)
  uint64_t emitted() const { return emitted_; }

 private:
  // compress the first n staged bytes as the stream's next piece and forward what is finished
  Err feed(size_t n, bool final) {
    if (!e_.ok()) return make_error(e_, e_.status());
    if (!st_) {
      const int rc = flate_hip_stream_open(e_.ctx(), flags_, &st_);
      if (rc != 0) return make_error(e_, rc);
    }
    std::vector<uint8_t> out(flate_hip_stream_bound(n));
    uint64_t len = 0;
    const int rc = flate_hip_stream_write(st_, pending_.data(), n, final ? 1 : 0, out.data(), out.size(), &len);
    if (rc != 0) return make_error(e_, rc);
    pending_.erase(pending_.begin(), pending_.begin() + n);
    emitted_ += len;
    auto r = w_.write(out.data(), len);
    return r.second;
  }
  ByteSink &w_;
  Engine &e_;
  uint32_t flags_;
  size_t chunk_, emit_;
  bool batch_member_ = false;  // closed by a BatchWriter: staged until close_all
  flate_hip_stream *st_ = nullptr;
  uint64_t emitted_ = 0;
  std::vector<uint8_t> pending_;
  Err err_;
  friend class BatchWriter;
};

// Many Writers closed by ONE kernel pipeline: every stream still gets the bytes of its own
// Writer::new / write / close (writer.mbt:10,45,53), but the GPU sees them as one batch.
//   BatchWriter bw(engine);  Writer &a = bw.add(sink_a);  Writer &b = bw.add(sink_b);
//   a.write(...); b.write(...);  bw.close_all();
class BatchWriter {
 public:
  explicit BatchWriter(Engine &e, uint32_t flags = 0) : e_(e), flags_(flags) {}
  // With preset dictionaries as history (flate_hip_deflate_fast_batch_dict): `dicts` must outlive the
  // BatchWriter; add(sink, j) gives a Writer dictionary j, add(sink) none.
  BatchWriter(Engine &e, const DictTable &dicts, uint32_t flags = 0) : e_(e), flags_(flags), dicts_(&dicts) {}
  Writer &add(ByteSink &sink, uint32_t dict = FLATE_HIP_NO_DICT) {
    ws_.emplace_back(new Writer(sink, e_, flags_));
    ws_.back()->batch_member_ = true;
    dict_of_.push_back(dict);
    return *ws_.back();
  }
  size_t size() const { return ws_.size(); }
  // close() of every Writer that is still open; returns the first error (each Writer keeps its
  // own sticky state exactly as a lone close() would leave it)
  Err close_all() {
    std::vector<std::vector<uint8_t>> in, out;
    std::vector<Writer *> open;
    std::vector<uint32_t> dict_of;
    for (size_t k = 0; k < ws_.size(); ++k)
      if (!ws_[k]->err_) {
        open.push_back(ws_[k].get());
        in.push_back(std::move(ws_[k]->pending_));
        dict_of.push_back(dict_of_[k]);
      }
    if (open.empty()) return std::nullopt;
    Err er = dicts_ ? compress_batch(e_, in, *dicts_, dict_of, out, flags_) : compress_batch(e_, in, out, flags_);
    Err first;
    for (size_t i = 0; i < open.size(); ++i) {
      Writer *w = open[i];
      if (er) {
        w->err_ = er;
      } else {
        auto r = w->w_.write(out[i].data(), out[i].size());
        w->err_ = r.second ? r.second : Err(writer_closed_error());
      }
      if (!first && w->err_ && !(*w->err_ == writer_closed_error())) first = w->err_;
    }
    return first;
  }

 private:
  Engine &e_;
  uint32_t flags_;
  const DictTable *dicts_ = nullptr;
  std::vector<uint32_t> dict_of_;  // per Writer
  std::vector<std::unique_ptr<Writer>> ws_;
};

// ---- spliced form (no reference counterpart): one DEFLATE stream for the batch ----
inline Err compress_spliced(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                            std::vector<uint8_t> &out, std::vector<uint64_t> *bit_off = nullptr,
                            uint32_t flags = 0);
inline Err compress_spliced(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                            std::vector<uint8_t> &out, std::vector<uint64_t> *bit_off, uint32_t flags) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  std::vector<uint64_t> in_off(n + 1, 0), bo(n + 1, 0);
  uint64_t cap = 16;
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    cap += flate_hip_deflate_bound(streams[i].size());
  }
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  uint64_t len = 0;
  const int rc = flate_hip_deflate_fast_spliced(e.ctx(), in.data(), in_off.data(), n, buf.data(), cap, &len,
                                                bo.data(), flags);
  if (rc != 0) return make_error(e, rc);
  out.assign(buf.begin(), buf.begin() + len);
  if (bit_off) *bit_off = bo;
  return std::nullopt;
}

// The whole batch as ONE zlib stream or ONE gzip member around the spliced stream, checksum and length over the
// concatenated input (flate_hip_deflate_fast_spliced_framed): what gzip -d / zlib's uncompress turn back into all the
// bytes.  bit_off counts from the raw stream's first byte, behind the 2 (zlib) or 10 (gzip) header bytes;
// decompress_spliced(..., Wrap) below takes the member and that index as they are.
inline Err compress_spliced(Engine &e, const std::vector<std::vector<uint8_t>> &streams, std::vector<uint8_t> &out,
                            Wrap wrap, std::vector<uint64_t> *bit_off = nullptr, uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  const uint32_t w = wrap_code(wrap);
  std::vector<uint64_t> in_off(n + 1, 0), bo(n + 1, 0);
  uint64_t cap = 16 + flate_hip_frame_overhead(w, 0);
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    cap += flate_hip_deflate_bound(streams[i].size());
  }
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  uint64_t len = 0;
  const int rc = flate_hip_deflate_fast_spliced_framed(e.ctx(), in.data(), in_off.data(), n, w, buf.data(), cap, &len,
                                                       bo.data(), flags);
  if (rc != 0) return make_error(e, rc);
  out.assign(buf.begin(), buf.begin() + len);
  if (bit_off) *bit_off = bo;
  return std::nullopt;
}

// Several spliced members in one call (flate_hip_deflate_fast_grouped_framed): groups[g] is the list of pieces of member
// g (at least one; an empty member is one empty piece), each compressed on its own and joined at bit granularity inside
// the member's header and trailer (Wrap::Raw: the bare streams).  members[g] receives member g; bit_off (may be null)
// receives per member its index, n_g + 1 entries counted from the raw stream's first byte: what
// decompress_spliced(..., Wrap) takes with the member as it is.
inline Err compress_grouped(Engine &e, const std::vector<std::vector<std::vector<uint8_t>>> &groups,
                            std::vector<std::vector<uint8_t>> &members, Wrap wrap,
                            std::vector<std::vector<uint64_t>> *bit_off = nullptr, uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n_groups = (uint32_t)groups.size();
  const uint32_t w = wrap_code(wrap);
  std::vector<uint32_t> group_off(n_groups + 1, 0);
  std::vector<uint64_t> in_off(1, 0);
  uint64_t cap = 16;
  for (uint32_t g = 0; g < n_groups; ++g) {
    for (const auto &p : groups[g]) {
      in_off.push_back(in_off.back() + p.size());
      cap += flate_hip_deflate_bound(p.size());
    }
    group_off[g + 1] = (uint32_t)(in_off.size() - 1);
    cap += 5 + flate_hip_frame_overhead(w, 0);
  }
  const uint32_t n = (uint32_t)(in_off.size() - 1);
  std::vector<uint8_t> in(in_off[n] + 1), buf(cap);
  uint32_t i = 0;
  for (const auto &grp : groups)
    for (const auto &p : grp) std::copy(p.begin(), p.end(), in.begin() + in_off[i++]);
  std::vector<uint64_t> out_off(n_groups + 1, 0), bo((size_t)n + n_groups + 1, 0);
  const int rc = flate_hip_deflate_fast_grouped_framed(e.ctx(), in.data(), in_off.data(), n, group_off.data(), n_groups, w,
                                                       buf.data(), cap, out_off.data(), bo.data(), flags);
  if (rc != 0) return make_error(e, rc);
  members.assign(n_groups, {});
  if (bit_off) bit_off->assign(n_groups, {});
  for (uint32_t g = 0; g < n_groups; ++g) {
    members[g].assign(buf.begin() + out_off[g], buf.begin() + out_off[g + 1]);
    if (bit_off) (*bit_off)[g].assign(bo.begin() + group_off[g] + g, bo.begin() + group_off[g + 1] + g + 1);
  }
  return std::nullopt;
}

// ---- decode side ---------------------------------------------------------------------------
// pub let ioeof (inflate.mbt:19) and the errors of the Decompressor (inflate.mbt:38,780-785)
inline const IOError &ioeof() {
  static const IOError e{"EOF"};
  return e;
}
inline IOError corrupt_input_error(long long off) {  // inflate.mbt:38-40
  return IOError{"flate: corrupt input before offset " + std::to_string(off)};
}
inline const IOError &err_unexpected_eof() {  // @io.err_unexpected_eof via no_eof, inflate.mbt:780-785
  static const IOError e{"unexpected EOF"};
  return e;
}

struct Inflated {
  std::vector<uint8_t> bytes;  // what was decoded (also in front of an error, as read() flushes it)
  Err err;                     // nullopt, corrupt_input_error(offset) or err_unexpected_eof
  int status = 0;              // the FLATE_HIP_E_* code behind err (0 = none)
};

// The size every stream inflates to, without storing anything (FLATE_HIP_SIZE_ONLY): what a Reader
// of a stream of unknown size runs first.  sizes[i] counts the bytes in front of an error, too.
inline Err inflate_sizes(Engine &e, const std::vector<std::vector<uint8_t>> &streams, std::vector<uint64_t> &sizes) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  std::vector<uint64_t> in_off(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + streams[i].size();
  std::vector<uint8_t> in(in_off[n] + 8);
  for (uint32_t i = 0; i < n; ++i) std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  sizes.assign(n + 1, 0);
  const int rc = flate_hip_inflate_batch(e.ctx(), in.data(), in_off.data(), n, nullptr, nullptr, sizes.data(),
                                         status.data(), err_off.data(), FLATE_HIP_SIZE_ONLY);
  sizes.resize(n);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF) return make_error(e, rc);
  return std::nullopt;
}

// Decode independent streams in one batch.  sizes[i] = capacity for stream i's output.
inline Err decompress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                            const std::vector<uint64_t> &sizes, std::vector<Inflated> &out) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0), out_len(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    out_off[i + 1] = out_off[i] + sizes[i];
  }
  std::vector<uint8_t> in(in_off[n] + 8), buf(out_off[n] + 8);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const int rc = flate_hip_inflate_batch(e.ctx(), in.data(), in_off.data(), n, buf.data(), out_off.data(),
                                         out_len.data(), status.data(), err_off.data(), 0);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF && rc != FLATE_HIP_E_OUT_TOO_SMALL)
    return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    out[i].bytes.assign(buf.begin() + out_off[i], buf.begin() + out_off[i] + out_len[i]);
    out[i].err = std::nullopt;
    out[i].status = status[i];
    if (status[i] == FLATE_HIP_E_CORRUPT) out[i].err = corrupt_input_error(err_off[i]);
    else if (status[i] == FLATE_HIP_E_UNEXPECTED_EOF) out[i].err = err_unexpected_eof();
    else if (status[i] != 0) out[i].err = make_error(e, status[i]);
  }
  return std::nullopt;
}

inline Err inflate_sizes(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                         const std::vector<std::vector<uint8_t>> &dicts, const std::vector<uint32_t> &dict_of,
                         std::vector<uint64_t> &sizes) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  if (!dict_of.empty() && dict_of.size() != n) return make_error(e, FLATE_HIP_E_INVALID);
  std::vector<uint64_t> in_off(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) in_off[i + 1] = in_off[i] + streams[i].size();
  std::vector<uint8_t> in(in_off[n] + 8);
  for (uint32_t i = 0; i < n; ++i) std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const DictTable D(dicts);
  sizes.assign(n + 1, 0);
  const int rc = flate_hip_inflate_batch_dict(e.ctx(), in.data(), in_off.data(), n, D.bytes.data(), D.off.data(),
                                              (uint32_t)dicts.size(), dict_of.empty() ? nullptr : dict_of.data(),
                                              nullptr, nullptr, sizes.data(), status.data(), err_off.data(),
                                              FLATE_HIP_SIZE_ONLY);
  sizes.resize(n);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF) return make_error(e, rc);
  return std::nullopt;
}

inline Err decompress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &streams,
                            const std::vector<uint64_t> &sizes, const std::vector<std::vector<uint8_t>> &dicts,
                            const std::vector<uint32_t> &dict_of, std::vector<Inflated> &out) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)streams.size();
  if (!dict_of.empty() && dict_of.size() != n) return make_error(e, FLATE_HIP_E_INVALID);
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0), out_len(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + streams[i].size();
    out_off[i + 1] = out_off[i] + sizes[i];
  }
  std::vector<uint8_t> in(in_off[n] + 8), buf(out_off[n] + 8);
  for (uint32_t i = 0; i < n; ++i)
    std::copy(streams[i].begin(), streams[i].end(), in.begin() + in_off[i]);
  const DictTable D(dicts);
  const int rc = flate_hip_inflate_batch_dict(e.ctx(), in.data(), in_off.data(), n, D.bytes.data(), D.off.data(),
                                              (uint32_t)dicts.size(), dict_of.empty() ? nullptr : dict_of.data(),
                                              buf.data(), out_off.data(), out_len.data(), status.data(),
                                              err_off.data(), 0);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF && rc != FLATE_HIP_E_OUT_TOO_SMALL)
    return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    out[i].bytes.assign(buf.begin() + out_off[i], buf.begin() + out_off[i] + out_len[i]);
    out[i].err = std::nullopt;
    out[i].status = status[i];
    if (status[i] == FLATE_HIP_E_CORRUPT) out[i].err = corrupt_input_error(err_off[i]);
    else if (status[i] == FLATE_HIP_E_UNEXPECTED_EOF) out[i].err = err_unexpected_eof();
    else if (status[i] != 0) out[i].err = make_error(e, status[i]);
  }
  return std::nullopt;
}

// header / trailer bytes of one zlib or gzip member, {-1, 0} if its header is not one (RFC 1950 2.2: CM = 8,
// window <= 32 KiB, FCHECK, no preset dictionary; RFC 1952 2.3: magic, CM = 8, reserved flag bits zero, the
// optional fields skipped)
inline std::pair<int, int> container_header(const std::vector<uint8_t> &m, Wrap wrap) {
  if (wrap == Wrap::Zlib) {
    if (m.size() < 2 || (m[0] & 15) != 8 || (m[0] >> 4) > 7 || ((m[0] << 8) | m[1]) % 31 || (m[1] & 0x20)) return {-1, 0};
    return {2, 4};
  }
  if (m.size() < 10 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || (m[3] & 0xe0)) return {-1, 0};
  const uint8_t flg = m[3];
  size_t p = 10;
  if (flg & 4) {  // FEXTRA
    if (m.size() < p + 2) return {-1, 0};
    p += 2 + (size_t)(m[p] | (m[p + 1] << 8));
  }
  for (int bit : {8, 16})  // FNAME, FCOMMENT: zero-terminated
    if (flg & bit) {
      while (p < m.size() && m[p]) ++p;
      if (p >= m.size()) return {-1, 0};
      ++p;
    }
  if (flg & 2) p += 2;  // FHCRC
  return p <= m.size() ? std::pair<int, int>{(int)p, 8} : std::pair<int, int>{-1, 0};
}

// decompress_batch for zlib / gzip members: ONE call of flate_hip_inflate_batch_framed -- the headers parsed, the raw
// streams decoded and the trailers checked against the checksums of what came out, all on the GPU; a bad header
// (corrupt_input_error(0)), a checksum or (gzip) a length that does not match (corrupt_input_error at the member's
// end).  sizes[i] = capacity for member i's output (gzip: 0 = its ISIZE).  dicts (zlib): preset dictionaries; a
// member with FDICT is decoded with the first one whose Adler-32 is its DICTID (RFC 1950 2.2), and is corrupt if
// none is; dict_used (may be null): the dictionary every member chose, or FLATE_HIP_NO_DICT.
inline Err decompress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &members, std::vector<uint64_t> sizes,
                            const std::vector<std::vector<uint8_t>> &dicts, std::vector<Inflated> &out, Wrap wrap,
                            std::vector<uint32_t> *dict_used = nullptr) {
  if (wrap == Wrap::Raw && dicts.empty()) return decompress_batch(e, members, sizes, out);
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)members.size();
  sizes.resize(n, 0);
  std::vector<uint64_t> in_off(n + 1, 0), out_off(n + 1, 0), out_len(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  std::vector<uint32_t> used(n + 1, FLATE_HIP_NO_DICT);
  for (uint32_t i = 0; i < n; ++i) {
    const std::vector<uint8_t> &m = members[i];
    if (wrap == Wrap::Gzip && sizes[i] == 0 && m.size() >= 18) {  // ISIZE: the member's last four bytes
      const uint8_t *t = m.data() + m.size() - 4;
      sizes[i] = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    }
    in_off[i + 1] = in_off[i] + m.size();
    out_off[i + 1] = out_off[i] + sizes[i];
  }
  std::vector<uint8_t> in(in_off[n] + 8), buf(out_off[n] + 8);
  for (uint32_t i = 0; i < n; ++i) std::copy(members[i].begin(), members[i].end(), in.begin() + in_off[i]);
  const DictTable D(dicts);
  const bool with = !dicts.empty();
  const int rc = flate_hip_inflate_batch_framed(e.ctx(), in.data(), in_off.data(), n, wrap_code(wrap),
                                                with ? D.bytes.data() : nullptr, with ? D.off.data() : nullptr,
                                                (uint32_t)dicts.size(), buf.data(), out_off.data(), out_len.data(),
                                                status.data(), err_off.data(), used.data(), 0);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF && rc != FLATE_HIP_E_OUT_TOO_SMALL)
    return make_error(e, rc);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    out[i].bytes.assign(buf.begin() + out_off[i], buf.begin() + out_off[i] + out_len[i]);
    out[i].err = std::nullopt;
    out[i].status = status[i];
    if (status[i] == FLATE_HIP_E_CORRUPT) out[i].err = corrupt_input_error(err_off[i]);
    else if (status[i] == FLATE_HIP_E_UNEXPECTED_EOF) out[i].err = err_unexpected_eof();
    else if (status[i] != 0) out[i].err = make_error(e, status[i]);
  }
  if (dict_used) dict_used->assign(used.begin(), used.begin() + n);
  return std::nullopt;
}

inline Err decompress_batch(Engine &e, const std::vector<std::vector<uint8_t>> &members, std::vector<uint64_t> sizes,
                            std::vector<Inflated> &out, Wrap wrap) {
  return decompress_batch(e, members, std::move(sizes), {}, out, wrap);
}

// &Reader (inflate.mbt:227-232): where a Decompressor pulls its input from
struct ByteSource {
  virtual ~ByteSource() = default;
  virtual std::pair<int, Err> read(uint8_t *p, size_t n) = 0;  // (0, ioeof) at the end
};
struct BytesReader : ByteSource {  // @io.Buffer used as source
  std::vector<uint8_t> bytes;
  size_t pos = 0;
  explicit BytesReader(std::vector<uint8_t> b) : bytes(std::move(b)) {}
  std::pair<int, Err> read(uint8_t *p, size_t n) override {
    if (pos == bytes.size()) return {0, ioeof()};
    const size_t k = std::min(n, bytes.size() - pos);
    std::copy(bytes.begin() + pos, bytes.begin() + pos + k, p);
    pos += k;
    return {(int)k, std::nullopt};
  }
};

// &Reader::new(r) -> Decompressor (inflate.mbt:305) with read (:382-405) and close (:410-415).
// As the reference's, this Reader holds a PIECE of the compressed stream and a piece of the output,
// never the whole of either (flate_hip_inflate_stream_*: the decoder's state -- window, tables of the
// block in progress, bit position, a copy that did not fit -- rests on the device between calls): a
// 10 GB stream needs the two pieces, not 10 GB.  The bytes and errors come out as the reference hands
// them out -- data first, the error (ioeof at a clean end) together with the last bytes, nothing but
// the error afterwards.  (size_hint is accepted for source compatibility and ignored: nothing has to
// be sized any more.)
class Reader {
 public:
  Reader(ByteSource &r, Engine &e, uint64_t size_hint = 0, size_t in_piece = 1u << 20, size_t out_piece = 1u << 20)
      : r_(&r), e_(e), in_piece_(in_piece < 4096 ? 4096 : in_piece), out_piece_(out_piece < 1 ? 1 : out_piece) {
    (void)size_hint;
  }
  // &Reader::new_dict(r, dict) (inflate.mbt:315-317): the stream decodes as if its output started with
  // `dict`, which has already been read (its last 32768 bytes are the history, dict-decoder.mbt:40-60)
  static std::unique_ptr<Reader> new_dict(ByteSource &r, Engine &e, std::vector<uint8_t> dict, size_t in_piece = 1u << 20,
                                          size_t out_piece = 1u << 20) {
    std::unique_ptr<Reader> rd(new Reader(r, e, 0, in_piece, out_piece));
    rd->dict_ = std::move(dict);
    return rd;
  }
  ~Reader() { flate_hip_inflate_stream_free(st_); }
  Reader(const Reader &) = delete;
  Reader &operator=(const Reader &) = delete;

  // Decompressor::reset(r, dict) (inflate.mbt:862-884): forget everything and decode the stream `r`
  // delivers next, with `dict` (may be empty) as its preset dictionary.
  void reset(ByteSource &r, std::vector<uint8_t> dict = {}) {
    r_ = &r;
    dict_ = std::move(dict);
    fresh_ = true;  // (the handle, if any, is reset in front of the next decode)
    in_.clear();
    src_end_ = false;
    data_.clear();
    pos_ = 0;
    err_ = std::nullopt;
  }

  // Decompressor::make_reader (inflate.mbt:857-860): the stream goes on from another source; nothing
  // else changes (bytes already pulled from the old source are used first).
  void make_reader(ByteSource &r) {
    r_ = &r;
    src_end_ = false;
  }
  // The reference pulls its source a byte at a time and stops at the end of the final block; this
  // Reader pulls a piece ahead.  What it pulled and did not use -- the bytes BEHIND the stream when the
  // source holds more than one payload -- is here (valid once read() has returned the stream's end).
  const std::vector<uint8_t> &unread() const { return in_; }

  std::pair<int, Err> read(uint8_t *p, size_t n) {
    for (;;) {
      if (pos_ < data_.size()) {  // :384-396
        const size_t k = std::min(n, data_.size() - pos_);
        std::copy(data_.begin() + pos_, data_.begin() + pos_ + k, p);
        pos_ += k;
        if (pos_ == data_.size()) return {(int)k, err_};
        return {(int)k, std::nullopt};
      }
      if (err_) return {0, err_};  // :397-400
      step();
    }
  }
  Err close() {  // :410-415
    if (err_ && *err_ == ioeof()) return std::nullopt;
    return err_;
  }
  // what this Reader holds at most: the two pieces (+ the decoder's 40 KiB on the device)
  size_t resident_bytes() const { return in_.capacity() + data_.capacity(); }

 private:
  // one call of the decoder: top the input piece up from the source, decode into the output piece
  void step() {
    if (!e_.ok()) {
      err_ = make_error(e_, e_.status());
      return;
    }
    if (!st_) {
      const int rc = flate_hip_inflate_stream_open(e_.ctx(), &st_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = !dict_.empty();
    }
    if (fresh_) {
      const int rc = flate_hip_inflate_stream_reset(st_, dict_.data(), dict_.size());
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    while (!src_end_ && in_.size() < in_piece_) {
      const size_t at = in_.size();
      in_.resize(in_piece_);
      auto r = r_->read(in_.data() + at, in_piece_ - at);
      in_.resize(at + (size_t)r.first);
      if (r.second) {
        if (!(*r.second == ioeof())) {  // the source's own error ends the stream (more_bits, :771-787)
          err_ = r.second;
          return;
        }
        src_end_ = true;
      }
    }
    data_.resize(out_piece_);
    pos_ = 0;
    uint64_t used = 0, got = 0;
    int64_t eoff = -1;
    const int rc = flate_hip_inflate_stream_read(st_, in_.data(), in_.size(), src_end_ ? 1 : 0, data_.data(),
                                                 out_piece_, &used, &got, &eoff);
    data_.resize((size_t)got);
    in_.erase(in_.begin(), in_.begin() + (size_t)used);
    if (rc == FLATE_HIP_STREAM_END) err_ = ioeof();
    else if (rc == FLATE_HIP_E_CORRUPT) err_ = corrupt_input_error(eoff);
    else if (rc == FLATE_HIP_E_UNEXPECTED_EOF) err_ = err_unexpected_eof();
    else if (rc != 0) err_ = make_error(e_, rc);
    else if (got == 0 && used == 0 && (src_end_ || in_.size() >= in_piece_))
      err_ = make_error(e_, FLATE_HIP_E_INTERNAL);  // (no progress although the decoder has what it may ask for)
  }
  ByteSource *r_;
  Engine &e_;
  size_t in_piece_, out_piece_;
  flate_hip_inflate_stream *st_ = nullptr;
  std::vector<uint8_t> dict_;  // preset dictionary of the stream being decoded (kept for nothing else)
  bool fresh_ = false;         // the handle must be reset before it decodes
  std::vector<uint8_t> in_;   // the bytes of the stream the decoder has not used yet
  bool src_end_ = false;
  std::vector<uint8_t> data_;  // decoded, not handed out yet (to_read, inflate.mbt:286)
  size_t pos_ = 0;
  Err err_;
};

// The same Reader over ONE LONG raw, zlib or gzip stream at flate_hip_inflate_one's speed (flate_hip_one_reader_*): every
// step decodes, in parallel, the units that lie whole inside the input piece, and the handle carries the bit where the
// next unit starts, the window and the running checksum.  It holds the two pieces and loops as Reader does; what differs
// is the grain -- a call delivers whole units -- so a piece grows where a unit needs it: the output piece to the size of a
// first unit that does not fit, the input piece (doubled) when it is full and holds no complete unit.  Bytes and errors
// come out as Reader's: data first, the error (ioeof at a clean end, the trailer checked) with the last bytes.
class OneReader {
 public:
  OneReader(ByteSource &r, Engine &e, Wrap wrap, size_t in_piece = 1u << 24, size_t out_piece = 1u << 26)
      : r_(&r), e_(e), wrap_(wrap), in_piece_(in_piece < 4096 ? 4096 : in_piece), out_piece_(out_piece < 1 ? 1 : out_piece) {}
  ~OneReader() { flate_hip_one_reader_free(h_); }
  OneReader(const OneReader &) = delete;
  OneReader &operator=(const OneReader &) = delete;

  // a fresh stream from `r` on the same handle: same wrap, and the unit rule and "one_unit_max" the engine had when the
  // handle was opened, which is in the first step that decodes
  void reset(ByteSource &r) {
    r_ = &r;
    fresh_ = true;
    in_.clear();
    src_end_ = false;
    len_ = 0;
    pos_ = 0;
    err_ = std::nullopt;
  }
  // what was pulled from the source and lies behind the stream (valid once read() has returned the stream's end)
  const std::vector<uint8_t> &unread() const { return in_; }

  std::pair<int, Err> read(uint8_t *p, size_t n) {
    for (;;) {
      if (pos_ < len_) {
        const size_t k = std::min(n, len_ - pos_);
        std::copy(data_.begin() + pos_, data_.begin() + pos_ + k, p);
        pos_ += k;
        if (pos_ == len_) return {(int)k, err_};
        return {(int)k, std::nullopt};
      }
      if (err_) return {0, err_};
      step();
    }
  }
  Err close() {
    if (err_ && *err_ == ioeof()) return std::nullopt;
    return err_;
  }
  size_t resident_bytes() const { return in_.capacity() + data_.capacity(); }
  uint64_t calls() const { return calls_; }

 private:
  void step() {
    if (!e_.ok()) {
      err_ = make_error(e_, e_.status());
      return;
    }
    if (!h_) {
      const int rc = flate_hip_one_reader_open(e_.ctx(), wrap_code(wrap_), 0, &h_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    if (fresh_) {
      const int rc = flate_hip_one_reader_reset(h_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    bool stalled = false;  // the source gave no byte and no error: decode what is here, do not ask again in this step
    while (!src_end_ && !stalled && in_.size() < in_piece_) {
      const size_t at = in_.size();
      in_.resize(in_piece_);
      auto r = r_->read(in_.data() + at, in_piece_ - at);
      in_.resize(at + (size_t)r.first);
      if (r.second) {
        if (!(*r.second == ioeof())) {
          err_ = r.second;
          return;
        }
        src_end_ = true;
      }
      stalled = r.first == 0 && !r.second;
    }
    if (data_.size() < out_piece_) data_.resize(out_piece_);  // (the piece is filled once, not per step)
    pos_ = 0;
    len_ = 0;
    uint64_t used = 0, got = 0;
    int64_t eoff = -1;
    ++calls_;
    const int rc = flate_hip_one_reader_read(h_, in_.data(), in_.size(), src_end_ ? 1 : 0, data_.data(), out_piece_, &used,
                                             &got, &eoff, nullptr);
    if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {  // not even the first unit fits: room for it, nothing has changed
      out_piece_ = (size_t)got;
      return;
    }
    len_ = (size_t)got;
    in_.erase(in_.begin(), in_.begin() + (size_t)used);
    if (rc == FLATE_HIP_STREAM_END) err_ = ioeof();
    else if (rc == FLATE_HIP_E_CORRUPT) err_ = corrupt_input_error(eoff);
    else if (rc == FLATE_HIP_E_UNEXPECTED_EOF) err_ = err_unexpected_eof();
    else if (rc != 0) err_ = make_error(e_, rc);
    else if (got == 0 && used == 0) {
      if (src_end_) err_ = make_error(e_, FLATE_HIP_E_INTERNAL);  // (no progress on the stream's last bytes)
      else if (stalled) err_ = IOError{"flate_host::OneReader: the source delivers neither bytes nor an error"};
      else if (in_.size() >= in_piece_) in_piece_ *= 2;           // a unit longer than the piece: it has to lie in it whole
    }
  }
  ByteSource *r_;
  Engine &e_;
  Wrap wrap_;
  size_t in_piece_, out_piece_;
  flate_hip_one_reader *h_ = nullptr;
  bool fresh_ = false;
  std::vector<uint8_t> in_;
  bool src_end_ = false;
  std::vector<uint8_t> data_;  // the output piece; its first len_ bytes are decoded and not all handed out yet
  size_t len_ = 0, pos_ = 0;
  uint64_t calls_ = 0;
  Err err_;
};

// The same Reader over a gzip FILE of any members at flate_hip_gzfile_read's speed (flate_hip_gzfile_reader_*): every
// step decodes, in parallel, the units that lie whole inside the input piece, across the members in it, and judges the
// trailers of the members that end among them; the handle carries where the file stands.  The pieces and the loop are
// OneReader's, and so is the grain: the output piece grows to a first unit that does not fit, the input piece (doubled)
// when it is full and holds no complete unit.  Bytes and errors come out as Reader's: data first, the error (ioeof at the
// file's end) with the last bytes; a corrupt file reports the member's FILE offset, and failure() holds the other words.
// set_serial_max(S) (flate_hip_gzfile_reader_set_serial_max): members of at most S bytes that lie whole inside an input
// piece are decoded whole, by one batch per step; only before the first step of a file, and reset keeps it.
class GzFileReader {
 public:
  struct Failure {
    uint32_t bad_member = 0xffffffffu;
    int64_t err_off = -1, stream_err_off = -1;
  };
  struct Route {  // flate_hip_gzfile_reader_last_route
    uint32_t serial_members = 0, open_stop = 0;
    uint64_t find_from = 0;
  };
  GzFileReader(ByteSource &r, Engine &e, size_t in_piece = 1u << 24, size_t out_piece = 1u << 26)
      : r_(&r), e_(e), in_piece_(in_piece < 4096 ? 4096 : in_piece), out_piece_(out_piece < 1 ? 1 : out_piece) {}
  ~GzFileReader() { flate_hip_gzfile_reader_free(h_); }
  GzFileReader(const GzFileReader &) = delete;
  GzFileReader &operator=(const GzFileReader &) = delete;

  // a fresh file from `r` on the same handle, with the unit rule and "one_unit_max" the engine had when the handle was
  // opened, which is in the first step that decodes
  void reset(ByteSource &r) {
    r_ = &r;
    fresh_ = true;
    in_.clear();
    src_end_ = false;
    len_ = 0;
    pos_ = 0;
    members_ = 0;
    serial_members_ = 0;
    begun_ = false;
    fail_ = Failure();
    err_ = std::nullopt;
  }

  // S = 0 .. 2^28 - 1, before the first step of the file (after construction or reset): false otherwise, and nothing
  // changes.  It reaches the handle in the first step that decodes.
  bool set_serial_max(uint64_t serial_max) {
    if (begun_ || serial_max > (1ull << 28) - 1) return false;
    serial_max_ = serial_max;
    serial_dirty_ = true;
    return true;
  }
  // what the last step's call did (zeros before the first)
  Route last_route() const {
    Route t;
    if (h_) (void)flate_hip_gzfile_reader_last_route(h_, &t.serial_members, &t.open_stop, &t.find_from);
    return t;
  }

  std::pair<int, Err> read(uint8_t *p, size_t n) {
    for (;;) {
      if (pos_ < len_) {
        const size_t k = std::min(n, len_ - pos_);
        std::copy(data_.begin() + pos_, data_.begin() + pos_ + k, p);
        pos_ += k;
        if (pos_ == len_) return {(int)k, err_};
        return {(int)k, std::nullopt};
      }
      if (err_) return {0, err_};
      step();
    }
  }
  Err close() {
    if (err_ && *err_ == ioeof()) return std::nullopt;
    return err_;
  }
  size_t resident_bytes() const { return in_.capacity() + data_.capacity(); }
  uint64_t calls() const { return calls_; }
  uint64_t members() const { return members_; }  // members whose trailers were judged good so far
  uint64_t serial_members() const { return serial_members_; }  // ... of which delivered whole (set_serial_max)
  const Failure &failure() const { return fail_; }

 private:
  void step() {
    if (!e_.ok()) {
      err_ = make_error(e_, e_.status());
      return;
    }
    if (!h_) {
      const int rc = flate_hip_gzfile_reader_open(e_.ctx(), 0, &h_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    if (fresh_) {
      const int rc = flate_hip_gzfile_reader_reset(h_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    if (serial_dirty_) {  // (the handle is fresh: nothing of this file has been decoded)
      const int rc = flate_hip_gzfile_reader_set_serial_max(h_, serial_max_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      serial_dirty_ = false;
    }
    begun_ = true;
    bool stalled = false;  // the source gave no byte and no error: decode what is here, do not ask again in this step
    while (!src_end_ && !stalled && in_.size() < in_piece_) {
      const size_t at = in_.size();
      in_.resize(in_piece_);
      auto r = r_->read(in_.data() + at, in_piece_ - at);
      in_.resize(at + (size_t)r.first);
      if (r.second) {
        if (!(*r.second == ioeof())) {
          err_ = r.second;
          return;
        }
        src_end_ = true;
      }
      stalled = r.first == 0 && !r.second;
    }
    if (data_.size() < out_piece_) data_.resize(out_piece_);  // (the piece is filled once, not per step)
    pos_ = 0;
    len_ = 0;
    uint64_t used = 0, got = 0;
    uint32_t members = 0;
    Failure f;
    ++calls_;
    const int rc = flate_hip_gzfile_reader_read(h_, in_.data(), in_.size(), src_end_ ? 1 : 0, data_.data(), out_piece_, &used,
                                                &got, &members, nullptr, &f.bad_member, &f.err_off, &f.stream_err_off);
    if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {  // not even the first unit fits: room for it, nothing has changed
      out_piece_ = (size_t)got;
      return;
    }
    len_ = (size_t)got;
    members_ += members;
    if (serial_max_ && (got || used)) serial_members_ += last_route().serial_members;
    in_.erase(in_.begin(), in_.begin() + (size_t)used);
    if (rc < 0) fail_ = f;
    if (rc == FLATE_HIP_STREAM_END) err_ = ioeof();
    else if (rc == FLATE_HIP_E_CORRUPT) err_ = corrupt_input_error(f.err_off);
    else if (rc == FLATE_HIP_E_UNEXPECTED_EOF) err_ = err_unexpected_eof();
    else if (rc != 0) err_ = make_error(e_, rc);
    else if (got == 0 && used == 0) {
      if (src_end_) err_ = make_error(e_, FLATE_HIP_E_INTERNAL);  // (no progress on the file's last bytes)
      else if (stalled) err_ = IOError{"flate_host::GzFileReader: the source delivers neither bytes nor an error"};
      else if (in_.size() >= in_piece_) in_piece_ *= 2;           // a unit longer than the piece: it has to lie in it whole
    }
  }
  ByteSource *r_;
  Engine &e_;
  size_t in_piece_, out_piece_;
  flate_hip_gzfile_reader *h_ = nullptr;
  bool fresh_ = false;
  std::vector<uint8_t> in_;
  bool src_end_ = false;
  std::vector<uint8_t> data_;  // the output piece; its first len_ bytes are decoded and not all handed out yet
  size_t len_ = 0, pos_ = 0;
  uint64_t calls_ = 0, members_ = 0, serial_members_ = 0;
  uint64_t serial_max_ = 0;
  bool serial_dirty_ = false, begun_ = false;
  Failure fail_;
  Err err_;
};

// A Writer (writer.mbt:45,53: write, close) over ONE LONG raw, zlib or gzip stream at the batch encoder's speed
// (flate_hip_one_writer_*): the stream is cut into independent pieces of piece_bytes bytes (0: 65535), every step
// compresses, in parallel, the whole pieces that are staged, and the handle carries the last incomplete byte, the running
// checksum and the lengths on the device.  write() stages the bytes and, once part_bytes of them are there, hands the
// whole pieces to the GPU and what they compress to -- whole bytes -- to the sink; the remainder below a piece stays
// staged on the host.  close() sends the final call: the last, shorter piece, the closing block and the trailer.  The
// sink sees the bytes of compress_spliced over the same pieces inside the container, whatever the sizes of the writes.
// Sticky errors as Writer's.
class OneWriter {
 public:
  OneWriter(ByteSink &w, Engine &e, Wrap wrap, uint64_t piece_bytes = 0, uint32_t flags = 0, size_t part_bytes = 1u << 26)
      : w_(&w), e_(e), wrap_(wrap), piece_(piece_bytes), flags_(flags & ~FLATE_HIP_DEVICE_PTRS) {
    const uint64_t P = piece_bytes ? piece_bytes : 65535u;
    part_ = part_bytes < P ? (size_t)P : part_bytes;
  }
  ~OneWriter() { flate_hip_one_writer_free(h_); }
  OneWriter(const OneWriter &) = delete;
  OneWriter &operator=(const OneWriter &) = delete;

  std::pair<int, Err> write(const uint8_t *p, size_t n) {
    if (err_) return {0, err_};
    pending_.insert(pending_.end(), p, p + n);
    if (pending_.size() >= part_) {
      if (Err er = feed(false)) {
        err_ = er;
        return {0, err_};
      }
    }
    return {(int)n, std::nullopt};
  }
  std::pair<int, Err> write(const std::vector<uint8_t> &b) { return write(b.data(), b.size()); }

  Err close() {
    if (err_ && *err_ == writer_closed_error()) return std::nullopt;
    if (err_) return err_;
    if (Err er = feed(true)) {
      err_ = er;
      return err_;
    }
    err_ = writer_closed_error();
    return std::nullopt;
  }
  // a fresh stream into `w` on the same handle: same wrap, same piece size, same flags (what is staged is dropped)
  Err reset(ByteSink &w) {
    w_ = &w;
    pending_.clear();
    err_ = std::nullopt;
    emitted_ = 0;
    if (h_) {
      const int rc = flate_hip_one_writer_reset(h_);
      if (rc != 0) err_ = make_error(e_, rc);
    }
    return err_;
  }
  // compressed bytes handed to the sink so far, the calls made, the pieces compressed
  uint64_t emitted() const { return emitted_; }
  uint64_t calls() const { return calls_; }
  uint64_t pieces() const { return pieces_; }
  size_t resident_bytes() const { return pending_.capacity() + out_.capacity(); }

 private:
  Err feed(bool final) {
    if (!e_.ok()) return make_error(e_, e_.status());
    if (!h_) {
      const int rc = flate_hip_one_writer_open(e_.ctx(), wrap_code(wrap_), piece_, flags_, &h_);
      if (rc != 0) return make_error(e_, rc);
    }
    const size_t room = flate_hip_one_writer_bound(pending_.size(), (size_t)piece_);
    if (out_.size() < room) out_.resize(room);
    uint64_t used = 0, len = 0;
    uint32_t k = 0;
    ++calls_;
    const int rc = flate_hip_one_writer_write(h_, pending_.data(), pending_.size(), final ? 1 : 0, out_.data(), out_.size(),
                                              &used, &len, nullptr, &k);
    if (rc != FLATE_HIP_OK && rc != FLATE_HIP_STREAM_END) return make_error(e_, rc);
    pending_.erase(pending_.begin(), pending_.begin() + (size_t)used);
    emitted_ += len;
    pieces_ += k;
    if (!len) return std::nullopt;
    auto r = w_->write(out_.data(), (size_t)len);
    return r.second;
  }
  ByteSink *w_;
  Engine &e_;
  Wrap wrap_;
  uint64_t piece_;
  uint32_t flags_;
  size_t part_;
  flate_hip_one_writer *h_ = nullptr;
  uint64_t emitted_ = 0, calls_ = 0, pieces_ = 0;
  std::vector<uint8_t> pending_, out_;
  Err err_;
};

// The same Reader over a BGZF file at flate_hip_bgzf_read's speed (flate_hip_bgzf_reader_*): every step decodes, in
// parallel, the members that lie whole inside the input piece and fit the output piece; the handle is a few host words.
// The pieces and the loop are GzFileReader's; the input piece never has to grow beyond 65536 bytes, the output piece
// grows to a first member that does not fit.  Bytes and errors come out as Reader's: data first -- the good members in
// front of a failure --, the error (ioeof at the file's end) with the last bytes; a corrupt file reports the FILE
// offset, and failure() holds the other word.
class BgzfReader {
 public:
  struct Failure {
    uint32_t bad_member = 0xffffffffu;
    int64_t err_off = -1;
  };
  BgzfReader(ByteSource &r, Engine &e, size_t in_piece = 1u << 24, size_t out_piece = 1u << 26)
      : r_(&r), e_(e), in_piece_(in_piece < FLATE_HIP_BGZF_MEMBER_MAX ? FLATE_HIP_BGZF_MEMBER_MAX : in_piece),
        out_piece_(out_piece < 1 ? 1 : out_piece) {}
  ~BgzfReader() { flate_hip_bgzf_reader_free(h_); }
  BgzfReader(const BgzfReader &) = delete;
  BgzfReader &operator=(const BgzfReader &) = delete;

  // a fresh file from `r` on the same handle
  void reset(ByteSource &r) {
    r_ = &r;
    fresh_ = true;
    in_.clear();
    src_end_ = false;
    len_ = 0;
    pos_ = 0;
    members_ = 0;
    eof_marker_ = false;
    fail_ = Failure();
    err_ = std::nullopt;
  }

  std::pair<int, Err> read(uint8_t *p, size_t n) {
    for (;;) {
      if (pos_ < len_) {
        const size_t k = std::min(n, len_ - pos_);
        std::copy(data_.begin() + pos_, data_.begin() + pos_ + k, p);
        pos_ += k;
        if (pos_ == len_) return {(int)k, err_};
        return {(int)k, std::nullopt};
      }
      if (err_) return {0, err_};
      step();
    }
  }
  Err close() {
    if (err_ && *err_ == ioeof()) return std::nullopt;
    return err_;
  }
  size_t resident_bytes() const { return in_.capacity() + data_.capacity(); }
  uint64_t calls() const { return calls_; }
  uint64_t members() const { return members_; }   // members delivered so far
  bool eof_marker() const { return eof_marker_; }  // the last of them is the canonical marker
  const Failure &failure() const { return fail_; }

 private:
  void step() {
    if (!e_.ok()) {
      err_ = make_error(e_, e_.status());
      return;
    }
    if (!h_) {
      const int rc = flate_hip_bgzf_reader_open(e_.ctx(), 0, &h_);
      if (rc != 0) {
        err_ = make_error(e_, rc);
        return;
      }
      fresh_ = false;
    }
    if (fresh_) {
      (void)flate_hip_bgzf_reader_reset(h_);
      fresh_ = false;
    }
    bool stalled = false;  // the source gave no byte and no error: decode what is here, do not ask again in this step
    while (!src_end_ && !stalled && in_.size() < in_piece_) {
      const size_t at = in_.size();
      in_.resize(in_piece_);
      auto r = r_->read(in_.data() + at, in_piece_ - at);
      in_.resize(at + (size_t)r.first);
      if (r.second) {
        if (!(*r.second == ioeof())) {
          err_ = r.second;
          return;
        }
        src_end_ = true;
      }
      stalled = r.first == 0 && !r.second;
    }
    if (data_.size() < out_piece_) data_.resize(out_piece_);  // (the piece is filled once, not per step)
    pos_ = 0;
    len_ = 0;
    uint64_t used = 0, got = 0;
    uint32_t members = 0;
    int marker = 0;
    Failure f;
    ++calls_;
    const int rc = flate_hip_bgzf_reader_read(h_, in_.data(), in_.size(), src_end_ ? 1 : 0, data_.data(), out_piece_, &used,
                                              &got, 0, nullptr, nullptr, &members, &f.bad_member, &f.err_off, &marker);
    if (rc == FLATE_HIP_E_OUT_TOO_SMALL && f.bad_member == 0xffffffffu) {  // not even the first member fits: room for it
      out_piece_ = (size_t)got;
      return;
    }
    len_ = (size_t)got;
    members_ += members;
    eof_marker_ = marker != 0;
    in_.erase(in_.begin(), in_.begin() + (size_t)used);
    if (rc < 0) fail_ = f;
    if (rc == FLATE_HIP_STREAM_END) err_ = ioeof();
    else if (rc == FLATE_HIP_E_CORRUPT) err_ = corrupt_input_error(f.err_off);
    else if (rc == FLATE_HIP_E_UNEXPECTED_EOF) err_ = err_unexpected_eof();
    else if (rc != 0) err_ = make_error(e_, rc);
    else if (members == 0 && used == 0) {
      // (a part of 65536 bytes or a final one always makes progress or gives a verdict: only a short part gets here)
      if (src_end_) err_ = make_error(e_, FLATE_HIP_E_INTERNAL);
      else if (stalled) err_ = IOError{"flate_host::BgzfReader: the source delivers neither bytes nor an error"};
    }
  }
  ByteSource *r_;
  Engine &e_;
  size_t in_piece_, out_piece_;
  flate_hip_bgzf_reader *h_ = nullptr;
  bool fresh_ = false;
  std::vector<uint8_t> in_;
  bool src_end_ = false;
  std::vector<uint8_t> data_;  // the output piece; its first len_ bytes are decoded and not all handed out yet
  size_t len_ = 0, pos_ = 0;
  uint64_t calls_ = 0, members_ = 0;
  bool eof_marker_ = false;
  Failure fail_;
  Err err_;
};

// A Writer (write, close) over a BGZF file at flate_hip_bgzf_write's speed (flate_hip_bgzf_writer_*): write() stages
// the bytes and, once part_bytes of them are there, hands the whole blocks to the GPU and their members to the sink; the
// remainder below a block stays staged on the host.  close() sends the final call: the last, shorter block and the EOF
// marker.  The sink sees the bytes of compress_bgzf, whatever the sizes of the writes.  Sticky errors as Writer's.
class BgzfWriter {
 public:
  BgzfWriter(ByteSink &w, Engine &e, uint32_t block_bytes = 0, uint32_t flags = 0, size_t part_bytes = 1u << 26)
      : w_(&w), e_(e), block_(block_bytes), flags_(flags & ~FLATE_HIP_DEVICE_PTRS) {
    const size_t bb = block_bytes ? block_bytes : FLATE_HIP_BGZF_BLOCK_DEFAULT;
    part_ = part_bytes < bb ? bb : part_bytes;
  }
  ~BgzfWriter() { flate_hip_bgzf_writer_free(h_); }
  BgzfWriter(const BgzfWriter &) = delete;
  BgzfWriter &operator=(const BgzfWriter &) = delete;

  std::pair<int, Err> write(const uint8_t *p, size_t n) {
    if (err_) return {0, err_};
    pending_.insert(pending_.end(), p, p + n);
    if (pending_.size() >= part_) {
      if (Err er = feed(false)) {
        err_ = er;
        return {0, err_};
      }
    }
    return {(int)n, std::nullopt};
  }
  std::pair<int, Err> write(const std::vector<uint8_t> &b) { return write(b.data(), b.size()); }

  Err close() {
    if (err_ && *err_ == writer_closed_error()) return std::nullopt;
    if (err_) return err_;
    if (Err er = feed(true)) {
      err_ = er;
      return err_;
    }
    err_ = writer_closed_error();
    return std::nullopt;
  }
  // a fresh file into `w` on the same handle: same block size, same flags (what is staged is dropped)
  Err reset(ByteSink &w) {
    w_ = &w;
    pending_.clear();
    err_ = std::nullopt;
    emitted_ = 0;
    if (h_) (void)flate_hip_bgzf_writer_reset(h_);
    return err_;
  }
  // compressed bytes handed to the sink so far, the calls made, the members written (the marker not counted)
  uint64_t emitted() const { return emitted_; }
  uint64_t calls() const { return calls_; }
  uint64_t blocks() const { return blocks_; }
  size_t resident_bytes() const { return pending_.capacity() + out_.capacity(); }

 private:
  Err feed(bool final) {
    if (!e_.ok()) return make_error(e_, e_.status());
    if (!h_) {
      const int rc = flate_hip_bgzf_writer_open(e_.ctx(), block_, flags_, &h_);
      if (rc != 0) return make_error(e_, rc);
    }
    const size_t room = flate_hip_bgzf_writer_bound(pending_.size(), block_);
    if (out_.size() < room) out_.resize(room);
    uint64_t used = 0, len = 0;
    uint32_t k = 0;
    ++calls_;
    const int rc = flate_hip_bgzf_writer_write(h_, pending_.data(), pending_.size(), final ? 1 : 0, out_.data(), out_.size(),
                                               &used, &len, nullptr, &k);
    if (rc != FLATE_HIP_OK && rc != FLATE_HIP_STREAM_END) return make_error(e_, rc);
    pending_.erase(pending_.begin(), pending_.begin() + (size_t)used);
    emitted_ += len;
    blocks_ += k;
    if (!len) return std::nullopt;
    auto r = w_->write(out_.data(), (size_t)len);
    return r.second;
  }
  ByteSink *w_;
  Engine &e_;
  uint32_t block_, flags_;
  size_t part_;
  flate_hip_bgzf_writer *h_ = nullptr;
  uint64_t emitted_ = 0, calls_ = 0, blocks_ = 0;
  std::vector<uint8_t> pending_, out_;
  Err err_;
};

// One spliced stream decoded in parallel from its index (flate_hip_inflate_spliced).
inline Err decompress_spliced(Engine &e, const std::vector<uint8_t> &stream, const std::vector<uint64_t> &bit_off,
                              const std::vector<uint64_t> &sizes, std::vector<uint8_t> &out) {
  if (!e.ok()) return make_error(e, e.status());
  const uint32_t n = (uint32_t)sizes.size();
  std::vector<uint64_t> out_off(n + 1, 0), out_len(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) out_off[i + 1] = out_off[i] + sizes[i];
  std::vector<uint8_t> in(stream);
  in.resize(in.size() + 8);
  out.assign(out_off[n] + 8, 0);
  const int rc = flate_hip_inflate_spliced(e.ctx(), in.data(), stream.size(), bit_off.data(), n, out.data(),
                                           out_off.data(), out_len.data(), status.data(), err_off.data(), 0);
  if (rc != 0) {
    for (uint32_t i = 0; i < n; ++i)
      if (status[i] == FLATE_HIP_E_CORRUPT) return corrupt_input_error(err_off[i]);
    return make_error(e, rc);
  }
  out.resize(out_off[n]);
  return std::nullopt;
}

// The same for ONE zlib stream or gzip member around the spliced stream -- what compress_spliced(..., Wrap) writes, or
// any other writer around the same raw stream: ONE call of flate_hip_inflate_spliced_framed, the header measured, the
// pieces decoded and the trailer checked against the checksum of their concatenation, all on the GPU.  bit_off is
// counted from the raw stream's first byte, as compress_spliced returns it; an index of one entry (no input at all)
// is one piece of size 0.  sizes[i] = capacity for piece i; out = what the pieces produced, one after another.
// Errors: a bad header is corrupt_input_error(0); a piece's own error is that piece's (its offset counted from the
// raw stream's first byte); a checksum or (gzip) a length that does not match is corrupt_input_error at the member's
// end -- `out` then still holds the bytes.  Wrap::Raw is the overload above.
inline Err decompress_spliced(Engine &e, const std::vector<uint8_t> &member, std::vector<uint64_t> bit_off,
                              std::vector<uint64_t> sizes, Wrap wrap, std::vector<uint8_t> &out) {
  if (wrap == Wrap::Raw) return decompress_spliced(e, member, bit_off, sizes, out);
  if (!e.ok()) return make_error(e, e.status());
  if (bit_off.size() == 1) {
    bit_off.push_back(bit_off[0]);
    sizes.assign(1, 0);
  }
  const uint32_t n = (uint32_t)sizes.size();
  if (bit_off.size() != (size_t)n + 1) return make_error(e, FLATE_HIP_E_INVALID);
  std::vector<uint64_t> out_off(n + 1, 0), out_len(n + 1, 0);
  std::vector<int32_t> status(n + 1, 0);
  std::vector<int64_t> err_off(n + 1, -1);
  for (uint32_t i = 0; i < n; ++i) out_off[i + 1] = out_off[i] + sizes[i];
  std::vector<uint8_t> in(member), buf(out_off[n] + 8);
  in.resize(in.size() + 8);
  int32_t member_status = 0;
  int64_t member_err_off = -1;
  const int rc = flate_hip_inflate_spliced_framed(e.ctx(), in.data(), member.size(), wrap_code(wrap), bit_off.data(), n,
                                                  buf.data(), out_off.data(), out_len.data(), status.data(),
                                                  err_off.data(), &member_status, &member_err_off, 0);
  if (rc != 0 && rc != FLATE_HIP_E_CORRUPT && rc != FLATE_HIP_E_UNEXPECTED_EOF && rc != FLATE_HIP_E_OUT_TOO_SMALL)
    return make_error(e, rc);
  out.clear();
  for (uint32_t i = 0; i < n; ++i)
    out.insert(out.end(), buf.begin() + out_off[i], buf.begin() + out_off[i] + std::min(out_len[i], sizes[i]));
  if (member_status == 0) return std::nullopt;
  if (member_err_off >= 0) return corrupt_input_error(member_err_off);  // the header (0) or the trailer (the member's end)
  for (uint32_t i = 0; i < n; ++i) {
    if (status[i] == FLATE_HIP_E_CORRUPT) return corrupt_input_error(err_off[i]);
    if (status[i] == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
    if (status[i] != 0) return make_error(e, status[i]);
  }
  return make_error(e, member_status);
}

// ---- BGZF files (the blocked gzip of the SAM/BAM specification) -----------------------------
// compress_bgzf: `data` as ONE .gz file that gzip -d, bgzip and htslib read -- a member per block_bytes of input (0:
// 65280), each with its size in a 'BC' extra subfield, then the 28-byte EOF marker; one call
// (flate_hip_bgzf_write), framed on the GPU.  member_off (may be null): where every member starts, the marker last.
// A block that compresses to more than 65536 bytes is FLATE_HIP_E_TOO_LARGE (the message names it).
inline Err compress_bgzf(Engine &e, const std::vector<uint8_t> &data, std::vector<uint8_t> &out, uint32_t block_bytes = 0,
                         std::vector<uint64_t> *member_off = nullptr, uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  const size_t cap = flate_hip_bgzf_bound(data.size(), block_bytes);
  if (!cap) return make_error(e, FLATE_HIP_E_INVALID);
  const uint32_t bb = block_bytes ? block_bytes : FLATE_HIP_BGZF_BLOCK_DEFAULT;
  std::vector<uint64_t> off((data.size() + bb - 1) / bb + 1, 0);
  std::vector<uint8_t> buf(cap);
  uint64_t len = 0;
  const int rc = flate_hip_bgzf_write(e.ctx(), data.data(), data.size(), block_bytes, buf.data(), cap, &len, off.data(),
                                      flags);
  if (rc != 0) return make_error(e, rc);
  out.assign(buf.begin(), buf.begin() + len);
  if (member_off) *member_off = off;
  return std::nullopt;
}

// What decompress_bgzf found beside the bytes.
struct BgzfInfo {
  uint32_t n_members = 0;
  uint32_t bad_member = 0xffffffffu;  // the first failing member, or (a malformed chain) the count of good ones
  int64_t err_off = -1;               // its file offset, or where no member could be read
  bool eof_marker = false;            // the file ends with the canonical empty member
  int status = 0;                     // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_bgzf: the reverse, for any BGZF file: member discovery, decoding and the check of every member's CRC-32
// and ISIZE on the GPU (flate_hip_bgzf_index for the size, flate_hip_bgzf_read for the bytes); no side index.
// Errors: a malformed chain is corrupt_input_error(the offset at which no member could be read), `out` empty; a
// failing member is corrupt_input_error(its file offset) or err_unexpected_eof -- `out` then still holds every other
// member's bytes.
inline Err decompress_bgzf(Engine &e, const std::vector<uint8_t> &file, std::vector<uint8_t> &out, BgzfInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  BgzfInfo I;
  uint64_t need = 0, len = 0;
  int eof = 0;
  int rc = flate_hip_bgzf_index(e.ctx(), file.data(), file.size(), 0, nullptr, nullptr, &I.n_members, &need, &eof,
                                &I.err_off, 0);
  out.clear();
  if (rc == 0) {
    std::vector<uint8_t> buf(need + 8);
    rc = flate_hip_bgzf_read(e.ctx(), file.data(), file.size(), buf.data(), need, &len, &I.n_members, &I.bad_member,
                             &I.err_off, &eof, 0);
    if (rc == 0 || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF || rc == FLATE_HIP_E_OUT_TOO_SMALL)
      out.assign(buf.begin(), buf.begin() + std::min(len, need));
  } else if (rc == FLATE_HIP_E_CORRUPT) {
    I.bad_member = I.n_members;
  }
  I.eof_marker = eof != 0;
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(I.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// ---- plain multi-member gzip files (cat a.gz b.gz, rotated logs, WARC records) ----------------
// What decompress_gzip found beside the bytes.
struct GzipInfo {
  uint32_t n_members = 0;
  uint32_t bad_member = 0xffffffffu;  // the first failing member, or (a broken chain) the count of good ones
  int64_t err_off = -1;               // its file offset, or where the chain broke
  uint32_t n_candidates = 0;          // offsets that were decoded speculatively
  int status = 0;                     // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_gzip: a .gz file of any number of members back into its bytes: member discovery, decoding and the check of
// every member's CRC-32 and ISIZE on the GPU (flate_hip_gzip_index for the size, flate_hip_gzip_read for the bytes); no
// side index.  Errors: a broken chain is corrupt_input_error(where no member can start), err_unexpected_eof (the last
// member is cut short) or FLATE_HIP_E_TOO_LARGE (a member beyond the option "gzip_member_max"), `out` empty; a failing
// member is corrupt_input_error(its file offset) -- `out` then still holds every other member's bytes.
inline Err decompress_gzip(Engine &e, const std::vector<uint8_t> &file, std::vector<uint8_t> &out, GzipInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  GzipInfo I;
  uint64_t need = 0, len = 0;
  int rc = flate_hip_gzip_index(e.ctx(), file.data(), file.size(), 0, nullptr, nullptr, &I.n_members, &need,
                                &I.n_candidates, &I.err_off, 0);
  out.clear();
  if (rc == 0) {
    std::vector<uint8_t> buf(need + 8);
    rc = flate_hip_gzip_read(e.ctx(), file.data(), file.size(), buf.data(), need, &len, &I.n_members, &I.bad_member,
                             &I.err_off, 0);
    if (rc == 0 || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF || rc == FLATE_HIP_E_OUT_TOO_SMALL)
      out.assign(buf.begin(), buf.begin() + std::min(len, need));
  } else if (rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF || rc == FLATE_HIP_E_TOO_LARGE) {
    I.bad_member = I.n_members;
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(I.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// ---- one long stream (one .gz, zlib or raw DEFLATE stream of many blocks) ----------------------
// What index_one found: the units of the stream -- bit 0 of the raw stream and every dynamic block header the serial
// decode reaches.
struct OneIndex {
  std::vector<uint64_t> unit_bit;  // n_units + 1: bits counted from the raw stream's first byte
  std::vector<uint64_t> out_off;   // n_units + 1: the exclusive prefix sum of what the units inflate to
  uint32_t n_units = 0;
  uint64_t out_bytes = 0;          // what the stream inflates to (0 unless status == 0)
  uint32_t n_candidates = 0;       // bit offsets that were decoded speculatively
  int64_t err_off = -1;            // counted from the raw stream's first byte
  int status = 0;                  // the FLATE_HIP_E_* code behind the error (0 = none)
};

// index_one: where the blocks of ONE long stream start and where their output goes, found on the GPU
// (flate_hip_inflate_one_index).  Errors: corrupt_input_error(err_off) for a bad container header (offset 0) or a block
// the decoder refuses, err_unexpected_eof for a stream that is cut short, FLATE_HIP_E_TOO_LARGE for a unit beyond the
// option "one_unit_max"; `ix` then holds the good units in front.
inline Err index_one(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, OneIndex &ix) {
  if (!e.ok()) return make_error(e, e.status());
  ix = OneIndex();
  int32_t st = 0;
  int rc = 0;
  // no query first: the discovery is the whole cost of the call.  A unit per 256 bytes of input is more than zlib
  // writes at its smallest memLevel; a stream that has more takes a second call, sized from the count.
  size_t cap = stream.size() / 256 + 64;
  for (int attempt = 0; attempt < 2; ++attempt) {
    ix.unit_bit.assign(cap, 0);
    ix.out_off.assign(cap, 0);
    rc = flate_hip_inflate_one_index(e.ctx(), stream.data(), stream.size(), wrap_code(wrap), cap, ix.unit_bit.data(),
                                     ix.out_off.data(), &ix.n_units, &ix.out_bytes, &ix.n_candidates, &st, &ix.err_off, 0);
    if ((size_t)ix.n_units + 1 <= cap) break;
    cap = (size_t)ix.n_units + 1;
  }
  ix.unit_bit.resize(std::min(cap, (size_t)ix.n_units + 1));
  ix.out_off.resize(ix.unit_bit.size());
  ix.status = rc;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(ix.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// What decompress_one found beside the bytes.
struct OneInfo {
  uint32_t n_units = 0;
  uint32_t n_candidates = 0;
  int64_t err_off = -1;  // counted from the raw stream's first byte; a trailer that does not match: the stream's size
  int status = 0;        // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_one: ONE long stream -- a .gz, zlib or raw DEFLATE stream of many blocks -- back into its bytes, its blocks
// found and decoded in parallel and its trailer checked on the GPU (flate_hip_inflate_one: one call with room for a
// gzip member's ISIZE; else, or if that was too little, a size query and the decode).  Errors are the serial
// decoder's: corrupt_input_error(err_off), err_unexpected_eof, FLATE_HIP_E_TOO_LARGE for a unit beyond the option
// "one_unit_max"; `out` then holds the bytes in front of the error.
inline Err decompress_one(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, std::vector<uint8_t> &out,
                          OneInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  OneInfo I;
  int32_t st = 0;
  uint64_t need = 0, len = 0;
  out.clear();
  // a gzip member says in its last four bytes what it inflates to (mod 2^32): with room for that the first call is
  // the decode, and no discovery is spent on a size query; a trailer that is wrong costs the second call the query
  // would have cost anyway.  (DEFLATE expands at most 1032 times.)
  const size_t n = stream.size();
  if (wrap == Wrap::Gzip && n >= 18) {
    need = (uint64_t)stream[n - 4] | ((uint64_t)stream[n - 3] << 8) | ((uint64_t)stream[n - 2] << 16) | ((uint64_t)stream[n - 1] << 24);
    if (need > 1032ull * n) need = 0;
  }
  std::vector<uint8_t> buf(need ? need + 8 : 0);
  uint64_t cap = need;
  int rc = flate_hip_inflate_one(e.ctx(), stream.data(), n, wrap_code(wrap), cap ? buf.data() : nullptr, cap, &len, &st,
                                 &I.err_off, &I.n_units, &I.n_candidates, 0);
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL && len > cap) {  // (len: the size needed)
    cap = len;
    buf.assign(cap + 8, 0);
    rc = flate_hip_inflate_one(e.ctx(), stream.data(), n, wrap_code(wrap), buf.data(), cap, &len, &st, &I.err_off,
                               &I.n_units, &I.n_candidates, 0);
  }
  if (cap && (rc == 0 || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF))
    out.assign(buf.begin(), buf.begin() + std::min(len, cap));
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(I.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// ---- a gzip file of any members, long ones included ----------------------------------------------
// What index_gzfile found: the units of every member and the members, bits counted from the FILE's first byte.
struct GzFileIndex {
  std::vector<uint64_t> unit_bit;     // n_units + 1
  std::vector<uint64_t> out_off;      // n_units + 1: the exclusive prefix sum of what the units inflate to
  std::vector<uint64_t> member_off;   // n_members + 1: file offsets; the last: the file's size
  std::vector<uint64_t> member_unit;  // n_members + 1: every member's first unit; the last: n_units
  uint32_t n_units = 0, n_members = 0;
  uint64_t out_bytes = 0;             // what the file inflates to (0 unless status == 0)
  uint32_t n_candidates = 0;
  uint32_t bad_member = 0xffffffffu;  // the member the chain broke in, or in front of which no member can start
  int64_t err_off = -1;               // where that member starts
  int64_t stream_err_off = -1;        // the serial decoder's offset, counted from that member's raw stream
  int status = 0;                     // the FLATE_HIP_E_* code behind the error (0 = none)
};

// index_gzfile: where the units and the members of a gzip file start and where their output goes, found on the GPU
// (flate_hip_gzfile_index; sized by a guess and one retry, as index_one).  Errors: corrupt_input_error(err_off) where
// no member can start or for a block the decoder refuses, err_unexpected_eof for a file that is cut short,
// FLATE_HIP_E_TOO_LARGE for a unit beyond the option "one_unit_max"; `ix` then holds the good prefix.
inline Err index_gzfile(Engine &e, const std::vector<uint8_t> &file, GzFileIndex &ix) {
  if (!e.ok()) return make_error(e, e.status());
  ix = GzFileIndex();
  int32_t st = 0;
  int rc = 0;
  size_t ucap = file.size() / 256 + 64, mcap = file.size() / 4096 + 64;
  for (int attempt = 0; attempt < 2; ++attempt) {
    ix.unit_bit.assign(ucap, 0);
    ix.out_off.assign(ucap, 0);
    ix.member_off.assign(mcap, 0);
    ix.member_unit.assign(mcap, 0);
    rc = flate_hip_gzfile_index(e.ctx(), file.data(), file.size(), ucap, ix.unit_bit.data(), ix.out_off.data(), mcap,
                                ix.member_off.data(), ix.member_unit.data(), &ix.n_units, &ix.n_members, &ix.out_bytes,
                                &ix.n_candidates, &st, &ix.bad_member, &ix.err_off, &ix.stream_err_off, 0);
    if ((size_t)ix.n_units + 1 <= ucap && (size_t)ix.n_members + 1 <= mcap) break;
    ucap = std::max(ucap, (size_t)ix.n_units + 1);
    mcap = std::max(mcap, (size_t)ix.n_members + 1);
  }
  ix.unit_bit.resize(std::min(ucap, (size_t)ix.n_units + 1));
  ix.out_off.resize(ix.unit_bit.size());
  ix.member_off.resize(std::min(mcap, (size_t)ix.n_members + 1));
  ix.member_unit.resize(ix.member_off.size());
  ix.status = rc;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(ix.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// What decompress_gzfile found beside the bytes.
struct GzFileInfo {
  uint32_t n_members = 0, n_units = 0, n_candidates = 0;
  uint32_t bad_member = 0xffffffffu;
  int64_t err_off = -1;         // the failing member's file offset
  int64_t stream_err_off = -1;  // inside its raw stream; a trailer that does not match: the member's length
  int status = 0;               // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_gzfile: a gzip file of any members back into its bytes, what zcat gives, every member cut into units that
// are decoded in parallel and every trailer checked on the GPU (flate_hip_gzfile_read: a size query, then the decode).
// Errors are the walk's: corrupt_input_error(err_off), err_unexpected_eof, FLATE_HIP_E_TOO_LARGE; `out` then holds the
// good members in front and the failing member's bytes in front of its failure (a wrong trailer: everything).
inline Err decompress_gzfile(Engine &e, const std::vector<uint8_t> &file, std::vector<uint8_t> &out,
                             GzFileInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  GzFileInfo I;
  int32_t st = 0;
  uint64_t len = 0;
  out.clear();
  auto call = [&](uint8_t *p, uint64_t cap) {
    return flate_hip_gzfile_read(e.ctx(), file.data(), file.size(), p, cap, &len, &I.n_members, &I.n_units,
                                 &I.n_candidates, &st, &I.bad_member, &I.err_off, &I.stream_err_off, 0);
  };
  int rc = call(nullptr, 0);
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL && len > 0) {  // (len: the size needed)
    const uint64_t cap = len;
    std::vector<uint8_t> buf(cap + 8, 0);
    rc = call(buf.data(), cap);
    if (rc == 0 || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF || rc == FLATE_HIP_E_TOO_LARGE)
      out.assign(buf.begin(), buf.begin() + std::min(len, cap));
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(I.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// What seek_index_one built: the seek index of ONE long stream, to keep beside the stream and hand to
// decompress_one_ranges.
struct OneSeekIndex {
  std::vector<uint64_t> index;   // the self-describing words (include/flate_hip.h documents the layout)
  std::vector<uint8_t> windows;  // n_points - 1 blocks of 32768 bytes
  uint32_t n_units = 0;
  uint32_t n_points = 0;
  uint64_t out_bytes = 0;        // what the stream inflates to
  uint32_t n_candidates = 0;
  int64_t err_off = -1;          // counted from the raw stream's first byte
  int status = 0;                // the FLATE_HIP_E_* code behind the error (0 = none)
};

// seek_index_one: the seek index of ONE long stream, a point per `span` bytes of output (0: 1 MiB;
// FLATE_HIP_SEEK_SPAN_NONE: no windows), built on the GPU (flate_hip_inflate_one_seek_index; sized by a guess and one
// retry, as index_one).  Errors are decompress_one's, except that the trailer is not judged; a stream that fails has
// no index.
inline Err seek_index_one(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, uint64_t span, OneSeekIndex &sx) {
  if (!e.ok()) return make_error(e, e.status());
  sx = OneSeekIndex();
  int32_t st = 0;
  int rc = 0;
  uint64_t words = 16 + 2 * (stream.size() / 256 + 64) + 64, bytes = 0, got_words = 0, got_bytes = 0;
  if (span != FLATE_HIP_SEEK_SPAN_NONE)
    bytes = std::min<uint64_t>(4 * (uint64_t)stream.size() / (span ? span : FLATE_HIP_SEEK_SPAN_DEFAULT) + 4,
                               stream.size() / 256 + 64) * FLATE_HIP_SEEK_WINDOW_BYTES;  // (never more points than units)
  for (int attempt = 0; attempt < 2; ++attempt) {
    sx.index.assign(words, 0);
    sx.windows.assign(bytes + 1, 0);
    rc = flate_hip_inflate_one_seek_index(e.ctx(), stream.data(), stream.size(), wrap_code(wrap), span, sx.index.data(), words,
                                          &got_words, sx.windows.data(), bytes, &got_bytes, &sx.n_units, &sx.n_points,
                                          &sx.out_bytes, &sx.n_candidates, &st, &sx.err_off, 0);
    if (rc != FLATE_HIP_E_OUT_TOO_SMALL) break;
    words = got_words, bytes = got_bytes;
  }
  sx.index.resize(rc == 0 ? got_words : 0);
  sx.windows.resize(rc == 0 ? got_bytes : 0);
  sx.status = rc;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(sx.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// One range of decompress_one_ranges: positions in what the stream inflates to; it reads short at the end.
struct OneRange {
  uint64_t begin = 0, end = 0;
};
// What decompress_one_ranges found beside the bytes.
struct OneRangesInfo {
  std::vector<uint64_t> out_off;      // n_ranges + 1: range r is out[out_off[r], out_off[r + 1])
  std::vector<int32_t> range_status;  // per range: 0, or the status of the first unit decoded for it that the index
                                      // does not fit
  uint32_t n_decoded = 0;             // the units decoded: from the seek point in front of a range up to its end
  uint32_t bad_unit = 0xffffffffu;    // the first unit the index does not fit
  int status = 0;                     // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_one_ranges: random access into ONE long stream through its seek index (flate_hip_inflate_one_ranges) --
// the bytes of `ranges` back to back in `out`; the size comes from the call's size query.  Errors:
// make_error(FLATE_HIP_E_INVALID) for an index that is not sound or not this stream's container and length,
// corrupt_input_error(-1) for a stream the index was not built from or does not fit (info->range_status says which
// ranges are exact all the same).
inline Err decompress_one_ranges(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, const OneSeekIndex &sx,
                                 const std::vector<OneRange> &ranges, std::vector<uint8_t> &out, OneRangesInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  OneRangesInfo I;
  const uint32_t nr = (uint32_t)ranges.size();
  std::vector<uint64_t> begin(nr), end(nr);
  for (uint32_t r = 0; r < nr; ++r) begin[r] = ranges[r].begin, end[r] = ranges[r].end;
  I.out_off.assign((size_t)nr + 1, 0);
  I.range_status.assign(nr, 0);
  out.clear();
  auto call = [&](uint8_t *buf, uint64_t cap) {
    return flate_hip_inflate_one_ranges(e.ctx(), stream.data(), stream.size(), wrap_code(wrap), sx.index.data(),
                                        sx.index.size(), sx.windows.empty() ? nullptr : sx.windows.data(), sx.windows.size(),
                                        begin.data(), end.data(), nr, buf, cap, I.out_off.data(), I.range_status.data(),
                                        &I.n_decoded, &I.bad_unit, 0);
  };
  int rc = call(nullptr, 0);  // the size query
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {
    const uint64_t need = I.out_off[nr];
    std::vector<uint8_t> buf(need + 8);
    rc = call(buf.data(), need);
    if (rc != FLATE_HIP_E_INVALID && rc != FLATE_HIP_E_HIP && rc != FLATE_HIP_E_INTERNAL)
      out.assign(buf.begin(), buf.begin() + std::min<uint64_t>(I.out_off[nr], need));
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(-1);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// What pack_seek_windows made of a seek index's windows: to keep beside the index in the windows' place.
struct SeekPack {
  std::vector<uint64_t> pack_index;  // the self-describing words (include/flate_hip.h documents the layout)
  std::vector<uint8_t> packed;       // every non-empty block as one raw DEFLATE stream, back to back
  uint64_t kept_bytes = 0;           // sparse: the window bytes some segment reads; else every byte
  int status = 0;                    // the FLATE_HIP_E_* code behind the error (0 = none)
};

// pack_seek_windows: the windows of sx, every block one raw DEFLATE stream and a block of zeros no bytes at all
// (flate_hip_seek_windows_pack); sparse: the bytes no segment reads become zero first, for which `stream` is walked
// (without sparse it is not read).  Errors: make_error(FLATE_HIP_E_INVALID) for an index that is not sound or not this
// stream's container and length, corrupt_input_error(-1) for a stream the index was not built from.
inline Err pack_seek_windows(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, const OneSeekIndex &sx, bool sparse,
                             SeekPack &pk) {
  if (!e.ok()) return make_error(e, e.status());
  pk = SeekPack();
  const uint64_t nb = sx.n_points ? sx.n_points - 1u : 0u;
  const uint64_t cap = flate_hip_seek_windows_pack_bound(nb);
  uint64_t words = 0, bytes = 0;
  pk.pack_index.assign(17 + nb, 0);
  pk.packed.assign(cap + 1, 0);
  const uint32_t mode = FLATE_HIP_SEEK_PACK_COMPRESS | (sparse ? FLATE_HIP_SEEK_PACK_SPARSE : 0u);
  const int rc = flate_hip_seek_windows_pack(e.ctx(), stream.data(), stream.size(), wrap_code(wrap), sx.index.data(),
                                             sx.index.size(), sx.windows.empty() ? nullptr : sx.windows.data(),
                                             sx.windows.size(), mode, pk.pack_index.data(), pk.pack_index.size(), &words,
                                             pk.packed.data(), cap, &bytes, &pk.kept_bytes, 0);
  pk.pack_index.resize(rc == 0 ? words : 0);
  pk.packed.resize(rc == 0 ? bytes : 0);
  pk.status = rc;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(-1);
  return make_error(e, rc);
}

// unpack_seek_windows: all blocks of pk in the raw layout (flate_hip_seek_windows_unpack): the sparsified windows, or
// the original ones of a pack without sparse -- what decompress_one_ranges takes as OneSeekIndex::windows.  Errors:
// corrupt_input_error(bad block) for a block that does not inflate to 32768 bytes.
inline Err unpack_seek_windows(Engine &e, const SeekPack &pk, std::vector<uint8_t> &windows) {
  if (!e.ok()) return make_error(e, e.status());
  const uint64_t need = pk.pack_index.size() > 3 ? pk.pack_index[3] * FLATE_HIP_SEEK_WINDOW_BYTES : 0;
  windows.assign(need + 1, 0);
  uint64_t bytes = 0;
  uint32_t bad = 0xffffffffu;
  const int rc = flate_hip_seek_windows_unpack(e.ctx(), pk.pack_index.data(), pk.pack_index.size(),
                                               pk.packed.empty() ? nullptr : pk.packed.data(), pk.packed.size(),
                                               windows.data(), need, &bytes, &bad, 0);
  windows.resize(rc == 0 || rc == FLATE_HIP_E_CORRUPT ? bytes : 0);
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error((int64_t)bad);
  return make_error(e, rc);
}

// decompress_one_ranges_packed: decompress_one_ranges through the PACKED windows of sx's index
// (flate_hip_inflate_one_ranges_packed; sx.windows is not read): only the blocks of the seek points the ranges need
// are inflated.  Errors are decompress_one_ranges's; a block that does not inflate is a unit the index does not fit.
inline Err decompress_one_ranges_packed(Engine &e, const std::vector<uint8_t> &stream, Wrap wrap, const OneSeekIndex &sx,
                                        const SeekPack &pk, const std::vector<OneRange> &ranges, std::vector<uint8_t> &out,
                                        OneRangesInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  OneRangesInfo I;
  const uint32_t nr = (uint32_t)ranges.size();
  std::vector<uint64_t> begin(nr), end(nr);
  for (uint32_t r = 0; r < nr; ++r) begin[r] = ranges[r].begin, end[r] = ranges[r].end;
  I.out_off.assign((size_t)nr + 1, 0);
  I.range_status.assign(nr, 0);
  out.clear();
  auto call = [&](uint8_t *buf, uint64_t cap) {
    return flate_hip_inflate_one_ranges_packed(e.ctx(), stream.data(), stream.size(), wrap_code(wrap), sx.index.data(),
                                               sx.index.size(), pk.pack_index.data(), pk.pack_index.size(),
                                               pk.packed.empty() ? nullptr : pk.packed.data(), pk.packed.size(), begin.data(),
                                               end.data(), nr, buf, cap, I.out_off.data(), I.range_status.data(),
                                               &I.n_decoded, &I.bad_unit, 0);
  };
  int rc = call(nullptr, 0);  // the size query
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {
    const uint64_t need = I.out_off[nr];
    std::vector<uint8_t> buf(need + 8);
    rc = call(buf.data(), need);
    if (rc != FLATE_HIP_E_INVALID && rc != FLATE_HIP_E_HIP && rc != FLATE_HIP_E_INTERNAL)
      out.assign(buf.begin(), buf.begin() + std::min<uint64_t>(I.out_off[nr], need));
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(-1);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// What seek_index_gzfile built: the seek index of a gzip file of ANY members, to keep beside the file and hand to
// decompress_gzfile_ranges.
struct GzFileSeekIndex {
  std::vector<uint64_t> index;   // the self-describing words (include/flate_hip.h documents the layout)
  std::vector<uint8_t> windows;  // n_points - n_members blocks of 32768 bytes: a point that starts a member has none
  uint32_t n_units = 0, n_members = 0, n_points = 0;
  uint64_t out_bytes = 0;        // what the file inflates to
  uint32_t n_candidates = 0;
  uint32_t bad_member = 0xffffffffu;
  int64_t err_off = -1;          // where the failing member starts, or where no member can start
  int64_t stream_err_off = -1;   // the serial decoder's offset, counted from that member's raw stream
  int status = 0;                // the FLATE_HIP_E_* code behind the error (0 = none)
};

// seek_index_gzfile: the seek index of a gzip file of any members: a point at every member's first unit and per `span`
// bytes of output (0: 1 MiB; FLATE_HIP_SEEK_SPAN_NONE: the member starts alone, no windows), built on the GPU
// (flate_hip_gzfile_seek_index; sized by a guess and one retry, as index_gzfile).  Errors are index_gzfile's and a
// distance in front of its member; trailers are not judged; a file that fails has no index.
inline Err seek_index_gzfile(Engine &e, const std::vector<uint8_t> &file, uint64_t span, GzFileSeekIndex &sx) {
  if (!e.ok()) return make_error(e, e.status());
  sx = GzFileSeekIndex();
  int32_t st = 0;
  int rc = 0;
  uint64_t words = 16 + 2 * (file.size() / 256 + 64) + 2 * (file.size() / 4096 + 64) + 64, bytes = 0, got_words = 0,
           got_bytes = 0;
  if (span != FLATE_HIP_SEEK_SPAN_NONE)
    bytes = std::min<uint64_t>(4 * (uint64_t)file.size() / (span ? span : FLATE_HIP_SEEK_SPAN_DEFAULT) + 4,
                               file.size() / 256 + 64) * FLATE_HIP_SEEK_WINDOW_BYTES;  // (never more points than units)
  for (int attempt = 0; attempt < 2; ++attempt) {
    sx.index.assign(words, 0);
    sx.windows.assign(bytes + 1, 0);
    rc = flate_hip_gzfile_seek_index(e.ctx(), file.data(), file.size(), span, sx.index.data(), words, &got_words,
                                     sx.windows.data(), bytes, &got_bytes, &sx.n_units, &sx.n_members, &sx.n_points,
                                     &sx.out_bytes, &sx.n_candidates, &st, &sx.bad_member, &sx.err_off, &sx.stream_err_off, 0);
    if (rc != FLATE_HIP_E_OUT_TOO_SMALL) break;
    words = got_words, bytes = got_bytes;
  }
  sx.index.resize(rc == 0 ? got_words : 0);
  sx.windows.resize(rc == 0 ? got_bytes : 0);
  sx.status = rc;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(sx.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// decompress_gzfile_ranges: random access into a gzip file of any members through its seek index
// (flate_hip_gzfile_ranges) -- the bytes of `ranges` of what zcat gives, back to back in `out`; a range may cross
// members; the size comes from the call's size query.  Errors: make_error(FLATE_HIP_E_INVALID) for an index that is
// not sound or not of this file's length, corrupt_input_error(-1) for a file whose members are not where the index has
// them or that the index does not fit (info->range_status says which ranges are exact all the same).
inline Err decompress_gzfile_ranges(Engine &e, const std::vector<uint8_t> &file, const GzFileSeekIndex &sx,
                                    const std::vector<OneRange> &ranges, std::vector<uint8_t> &out,
                                    OneRangesInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  OneRangesInfo I;
  const uint32_t nr = (uint32_t)ranges.size();
  std::vector<uint64_t> begin(nr), end(nr);
  for (uint32_t r = 0; r < nr; ++r) begin[r] = ranges[r].begin, end[r] = ranges[r].end;
  I.out_off.assign((size_t)nr + 1, 0);
  I.range_status.assign(nr, 0);
  out.clear();
  auto call = [&](uint8_t *buf, uint64_t cap) {
    return flate_hip_gzfile_ranges(e.ctx(), file.data(), file.size(), sx.index.data(), sx.index.size(),
                                   sx.windows.empty() ? nullptr : sx.windows.data(), sx.windows.size(), begin.data(),
                                   end.data(), nr, buf, cap, I.out_off.data(), I.range_status.data(), &I.n_decoded,
                                   &I.bad_unit, 0);
  };
  int rc = call(nullptr, 0);  // the size query
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {
    const uint64_t need = I.out_off[nr];
    std::vector<uint8_t> buf(need + 8);
    rc = call(buf.data(), need);
    if (rc != FLATE_HIP_E_INVALID && rc != FLATE_HIP_E_HIP && rc != FLATE_HIP_E_INTERNAL)
      out.assign(buf.begin(), buf.begin() + std::min<uint64_t>(I.out_off[nr], need));
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(-1);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// One range of decompress_bgzf_ranges: positions in the file's uncompressed bytes, or -- virtual_offsets -- BGZF
// virtual offsets (coffset << 16 | uoffset, as BAM, tabix and CSI indexes store them).
struct BgzfRange {
  uint64_t begin = 0, end = 0;
};
// What decompress_bgzf_ranges found beside the bytes.
struct BgzfRangesInfo {
  std::vector<uint64_t> out_off;      // n_ranges + 1: range r is out[out_off[r], out_off[r + 1])
  std::vector<int32_t> range_status;  // per range: 0, FLATE_HIP_E_INVALID (an invalid virtual offset: zero bytes), or
                                      // the status of the first failing member it touches
  uint32_t n_members = 0;
  uint32_t n_decoded = 0;             // the members the ranges touch: each decoded and verified once
  uint32_t bad_member = 0xffffffffu;  // the first failing member, or (a malformed chain) the count of good ones
  int64_t err_off = -1;
  int status = 0;                     // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_bgzf_ranges: random access into a BGZF file (flate_hip_bgzf_read_ranges) -- the bytes of `ranges` back to
// back in `out`; only the members they touch are decoded and verified, the chain is validated whole.  The size comes
// from the call's size query.  Errors: as decompress_bgzf; an invalid virtual offset is make_error(FLATE_HIP_E_INVALID)
// with every other range delivered (info->range_status says which).
inline Err decompress_bgzf_ranges(Engine &e, const std::vector<uint8_t> &file, const std::vector<BgzfRange> &ranges,
                                  std::vector<uint8_t> &out, BgzfRangesInfo *info = nullptr, bool virtual_offsets = false) {
  if (!e.ok()) return make_error(e, e.status());
  BgzfRangesInfo I;
  const uint32_t nr = (uint32_t)ranges.size();
  std::vector<uint64_t> begin(nr), end(nr);
  for (uint32_t r = 0; r < nr; ++r) begin[r] = ranges[r].begin, end[r] = ranges[r].end;
  I.out_off.assign((size_t)nr + 1, 0);
  I.range_status.assign(nr, 0);
  const uint32_t kind = virtual_offsets ? FLATE_HIP_BGZF_POS_VIRTUAL : FLATE_HIP_BGZF_POS_BYTES;
  out.clear();
  auto call = [&](uint8_t *buf, uint64_t cap) {
    return flate_hip_bgzf_read_ranges(e.ctx(), file.data(), file.size(), kind, begin.data(), end.data(), nr, buf, cap,
                                      I.out_off.data(), I.range_status.data(), &I.n_members, &I.n_decoded, &I.bad_member,
                                      &I.err_off, 0);
  };
  int rc = call(nullptr, 0);  // the size query
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL) {
    const uint64_t need = I.out_off[nr];
    std::vector<uint8_t> buf(need + 8);
    rc = call(buf.data(), need);
    if (rc == 0 || rc == FLATE_HIP_E_INVALID || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF)
      out.assign(buf.begin(), buf.begin() + std::min<uint64_t>(I.out_off[nr], need));
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(I.err_off);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

// ---- ZIP archives ----------------------------------------------------------------------------
// compress_zip: entries[i] under names[i] (UTF-8, 1 .. 65535 bytes each) as ONE archive that zipfile, unzip and
// every other reader open; one call (flate_hip_zip_write), headers and directory written on the GPU.  entry_off (may
// be null): the local header offsets and, last, where the directory starts.
inline Err compress_zip(Engine &e, const std::vector<std::vector<uint8_t>> &entries, const std::vector<std::string> &names,
                        std::vector<uint8_t> &out, std::vector<uint64_t> *entry_off = nullptr, uint32_t flags = 0) {
  if (!e.ok()) return make_error(e, e.status());
  if (entries.size() != names.size()) return make_error(e, FLATE_HIP_E_INVALID);
  const uint32_t n = (uint32_t)entries.size();
  std::vector<uint64_t> in_off(n + 1, 0), name_off(n + 1, 0), off(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    in_off[i + 1] = in_off[i] + entries[i].size();
    name_off[i + 1] = name_off[i] + names[i].size();
  }
  std::vector<uint8_t> in(in_off[n] + 1), nm(name_off[n] + 1);
  for (uint32_t i = 0; i < n; ++i) {
    std::copy(entries[i].begin(), entries[i].end(), in.begin() + in_off[i]);
    std::copy(names[i].begin(), names[i].end(), nm.begin() + name_off[i]);
  }
  const size_t cap = flate_hip_zip_bound(in_off.data(), n, name_off.data());
  if (!cap) return make_error(e, FLATE_HIP_E_INVALID);
  std::vector<uint8_t> buf(cap);
  uint64_t len = 0;
  const int rc = flate_hip_zip_write(e.ctx(), in.data(), in_off.data(), n, nm.data(), name_off.data(), buf.data(), cap, &len,
                                     off.data(), flags);
  if (rc != 0) return make_error(e, rc);
  out.assign(buf.begin(), buf.begin() + len);
  if (entry_off) *entry_off = off;
  return std::nullopt;
}

// What decompress_zip found beside the bytes.
struct ZipInfo {
  std::vector<std::string> names;            // every entry's name, as the directory has it
  std::vector<flate_hip_zip_entry> entries;  // the index
  std::vector<int32_t> entry_status;         // per entry: 0 or its FLATE_HIP_E_* code
  std::vector<int64_t> entry_err_off;
  uint32_t n_entries = 0;
  int64_t err_off = -1;                      // a malformed archive: where (flate_hip_zip_index)
  int status = 0;                            // the FLATE_HIP_E_* code behind the error (0 = none)
};

// decompress_zip: every entry of an archive: discovery, decoding (deflate and stored) and the check of every entry's
// size and CRC-32 on the GPU (flate_hip_zip_index for the names and sizes, flate_hip_zip_read for the bytes).  out[i] =
// entry i's bytes (empty for a failing entry).  Errors: a malformed archive is corrupt_input_error(where), `out` empty; a
// failing entry is corrupt_input_error(its header offset), err_unexpected_eof or make_error(its status) -- `out` then
// still holds every other entry (info->entry_status says which failed).
inline Err decompress_zip(Engine &e, const std::vector<uint8_t> &file, std::vector<std::vector<uint8_t>> &out,
                          ZipInfo *info = nullptr) {
  if (!e.ok()) return make_error(e, e.status());
  ZipInfo I;
  uint64_t need = 0;
  out.clear();
  int rc = flate_hip_zip_index(e.ctx(), file.data(), file.size(), 0, nullptr, nullptr, &I.n_entries, &need, &I.err_off, 0);
  int64_t where = I.err_off;
  if (rc == 0) {
    const uint32_t n = I.n_entries;
    I.entries.resize((size_t)n + 1);
    std::vector<uint64_t> out_off((size_t)n + 1, 0), out_len((size_t)n + 1, 0);
    I.entry_status.assign((size_t)n + 1, 0);
    I.entry_err_off.assign((size_t)n + 1, -1);
    rc = flate_hip_zip_index(e.ctx(), file.data(), file.size(), n, I.entries.data(), out_off.data(), &I.n_entries, &need,
                             &I.err_off, 0);
    if (rc == 0) {
      std::vector<uint8_t> buf(need + 8);
      rc = flate_hip_zip_read(e.ctx(), file.data(), file.size(), nullptr, 0, n, buf.data(), need, out_off.data(), out_len.data(),
                              I.entry_status.data(), I.entry_err_off.data(), &I.n_entries, &I.err_off, 0);
      if (I.err_off < 0) {  // (the archive itself is well-formed: rc is an entry's status)
        out.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
          const flate_hip_zip_entry &z = I.entries[i];
          I.names.emplace_back(file.begin() + z.name_off, file.begin() + z.name_off + z.name_len);
          if (I.entry_status[i] == 0) out[i].assign(buf.begin() + out_off[i], buf.begin() + out_off[i] + out_len[i]);
          else if (where < 0) where = (int64_t)z.header_off;
        }
      } else {
        where = I.err_off;
      }
    }
    I.entries.resize(n), I.entry_status.resize(n), I.entry_err_off.resize(n);
  }
  I.status = rc;
  if (info) *info = I;
  if (rc == 0) return std::nullopt;
  if (rc == FLATE_HIP_E_CORRUPT) return corrupt_input_error(where);
  if (rc == FLATE_HIP_E_UNEXPECTED_EOF) return err_unexpected_eof();
  return make_error(e, rc);
}

}  // namespace flate_host
