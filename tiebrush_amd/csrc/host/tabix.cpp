// tabix.cpp — see tabix.h
#include "tabix.h"

#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <thread>

#include "GSam.h"
#include "bgzf.h"
#include "tracks.h"

namespace tbh {

namespace {
const uint8_t kEofMember[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr size_t kMember = 0xff00;  // payload bytes of a member, as bgzip cuts them

int worker_count() { return std::max(1, std::min(cpu_budget(), 32)); }

// members of kMember payload bytes, the last one short; the members are independent, so ranges of them go to worker threads
bool deflate_slice(const uint8_t* src, size_t n, int threads, std::vector<uint8_t>& z) {
  z.clear();
  const size_t nmem = (n + kMember - 1) / kMember;
  const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)threads, nmem / 4));
  if (nt == 1) return bgzf_deflate_members(src, n, 6, z);
  std::vector<std::vector<uint8_t>> parts(nt);
  std::vector<char> ok(nt, 1);
  std::vector<std::thread> th;
  for (size_t t = 0; t < nt; ++t)
    th.emplace_back([&, t]() {
      const size_t a = nmem * t / nt * kMember, b = std::min(n, nmem * (t + 1) / nt * kMember);
      ok[t] = bgzf_deflate_members(src + a, b - a, 6, parts[t]) ? 1 : 0;
    });
  for (auto& x : th) x.join();
  for (size_t t = 0; t < nt; ++t) {
    if (!ok[t]) return false;
    z.insert(z.end(), parts[t].begin(), parts[t].end());
  }
  return true;
}
}  // namespace

TabixWriter::~TabixWriter() {
  if (f_) fclose(f_);
}

bool TabixWriter::open(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::string& head, std::string& err) {
  bool csi = false;
  for (uint32_t l : lens) csi = csi || (uint64_t)l > kBaiMaxRef;
  if (!(csi ? ix_.init_csi(names, lens, err) : ix_.init(names, lens, err))) return false;
  (void)unlink(path.c_str());
  (void)unlink((path + ".tbi").c_str());
  (void)unlink((path + ".csi").c_str());
  f_ = fopen(path.c_str(), "wb");
  if (!f_) {
    err = "cannot create " + path;
    return false;
  }
  path_ = path, head_ = head, names_ = names;
  off_ = runs_ = rows_ = text_ = 0, last_tid_ = -1, last_beg_ = 0;
  return true;
}

bool TabixWriter::add_run(const uint8_t* z, size_t n, const BaiChunk* chunks, size_t n_chunks, uint64_t lin_first, const uint64_t* lin, size_t n_lin, const BaiRef* refs,
                          size_t n_refs) {
  if (!f_) return false;
  ix_.add(off_, chunks, n_chunks, lin_first, lin, n_lin, refs, n_refs);
  if (n && fwrite(z, 1, n, f_) != n) return false;
  off_ += n, ++runs_;
  return true;
}

bool TabixWriter::add_text(const char* text, size_t n, std::vector<BaiRec>& recs, std::string& err) {
  if (!f_) {
    err = "the track is not open";
    return false;
  }
  for (size_t i = 0; i < recs.size(); ++i) {  // what tabix refuses too: the window table's rule needs the order
    const BaiRec& r = recs[i];
    if (r.tid < last_tid_ || (r.tid == last_tid_ && r.beg < last_beg_)) {
      err = "row " + std::to_string(rows_ + i) + " is out of order (the rows must be sorted by reference, then start)";
      return false;
    }
    last_tid_ = r.tid, last_beg_ = r.beg;
  }
  std::vector<uint8_t> z;
  if (!deflate_slice((const uint8_t*)text, n, worker_count(), z)) {
    err = "deflate failed";
    return false;
  }
  BaiPart part;
  if (!bai_member_voffsets(z.data(), z.size(), recs, err) || !bai_build_part(recs.data(), recs.size(), (uint64_t)z.size() << 16, ix_.ref_len(), part, err, ix_.depth())) {
    err = "rows from " + std::to_string(rows_) + " on: " + err;
    return false;
  }
  rows_ += recs.size(), text_ += n;
  if (!add_run(z.data(), z.size(), part.chunks.data(), part.chunks.size(), part.lin_first, part.lin.data(), part.lin.size(), part.refs.data(), part.refs.size())) {
    err = "cannot write " + path_;
    return false;
  }
  return true;
}

bool TabixWriter::close(std::string& err) {
  if (!f_) return true;
  const bool ok = fwrite(kEofMember, 1, sizeof(kEofMember), f_) == sizeof(kEofMember);
  const bool closed = fclose(f_) == 0;
  f_ = nullptr;
  if (!ok || !closed) {
    err = "cannot write " + path_;
    return false;
  }
  off_ += sizeof(kEofMember);
  const int32_t skip = head_.compare(0, 5, "track") == 0 ? 1 : 0;
  return ix_.write_tabix(path_ + (ix_.csi() ? ".csi" : ".tbi"), names_, skip, err);
}

void TabixWriter::discard() {
  if (!f_) return;
  fclose(f_);
  f_ = nullptr;
  (void)unlink(path_.c_str());
}

bool tabix_host_track(TabixWriter& w, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                      const std::function<int(uint32_t, char*, size_t)>& fmt, uint32_t slice_rows, int threads, std::string& err, bool with_head) {
  if (!slice_rows) slice_rows = 1u << 19;
  std::string text;
  std::vector<BaiRec> recs;
  bool first = true;
  for (uint32_t lo = 0; lo < n || (first && with_head); first = false) {
    const uint32_t hi = (uint32_t)std::min<uint64_t>(n, (uint64_t)lo + slice_rows), m = hi - lo;
    const size_t nt = m < 50000 ? 1 : (size_t)std::max(1, std::min(threads, 32));
    std::vector<std::string> parts(nt);
    std::vector<std::vector<uint32_t>> lens(nt);
    auto work = [&](size_t t) {
      const uint32_t a = lo + (uint32_t)((uint64_t)m * t / nt), b = lo + (uint32_t)((uint64_t)m * (t + 1) / nt);
      std::string& o = parts[t];
      o.reserve((size_t)(b - a) * 40);
      lens[t].reserve(b - a);
      char buf[1024];
      for (uint32_t i = a; i < b; ++i) {
        int len = fmt(i, buf, sizeof(buf));
        if (len < 0) len = 0;
        if ((size_t)len >= sizeof(buf)) {  // a very long reference name: format again into a buffer that fits
          std::vector<char> big((size_t)len + 1);
          len = fmt(i, big.data(), big.size());
          o.append(big.data(), (size_t)len);
        } else {
          o.append(buf, (size_t)len);
        }
        lens[t].push_back((uint32_t)len);
      }
    };
    if (nt == 1) {
      work(0);
    } else {
      std::vector<std::thread> th;
      for (size_t t = 0; t < nt; ++t) th.emplace_back(work, t);
      for (auto& x : th) x.join();
    }
    text.clear();
    if (first && with_head) text = w.head();
    recs.clear();
    recs.reserve(m);
    uint32_t i = lo;
    for (size_t t = 0; t < nt; ++t) {
      uint64_t o = text.size();
      for (uint32_t len : lens[t]) {
        recs.push_back(BaiRec{tid[i], start[i], std::max<int64_t>(end[i], (int64_t)start[i] + 1), o});
        o += len, ++i;
      }
      text += parts[t];
    }
    if (!text.empty() && !w.add_text(text.data(), text.size(), recs, err)) return false;
    lo = hi;
  }
  return true;
}

namespace {
static_assert(sizeof(BaiChunk) == sizeof(tbk_ix_chunk) && sizeof(BaiRef) == sizeof(tbk_ix_ref), "the part's arrays go to BaiIndex::add as they are");
struct TbxBridge {
  TabixWriter* w;
  bool failed = false;
  static int sink(void* user, const uint8_t* z, uint64_t n, const tbk_ix_part* p) {
    TbxBridge* b = (TbxBridge*)user;
    if (p && b->w->add_run(z, (size_t)n, (const BaiChunk*)p->chunks, p->n_chunks, p->lin_first, p->lin, (size_t)p->n_lin, (const BaiRef*)p->refs, p->n_refs)) return 0;
    b->failed = true;
    return 1;
  }
};
// TBK_DEBUG fmt_slice=BYTES (the device formatter's slice size) for the host path: BYTES / 32 rows a slice
uint32_t host_slice_rows() {
  const char* d = getenv("TBK_DEBUG");
  const char* p = d ? strstr(d, "fmt_slice=") : nullptr;
  if (!p) return 0;
  const unsigned long long b = strtoull(p + 10, nullptr, 0);
  return b ? (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>(b / 32, 1u << 30)) : 0;
}
}  // namespace

void set_track_names(const TrackApi& api, const std::vector<std::string>& names) {
  std::vector<uint64_t> off(names.size() + 1, 0);
  std::string blob;
  for (size_t t = 0; t < names.size(); ++t) blob += names[t], off[t + 1] = blob.size();
  const int rc = api.track_names(api.ctx, (uint32_t)names.size(), off.data(), blob.data());
  if (rc != 0) GError("Error: GPU track names failed: %s (%s)\n", api.strerror_(rc), api.last_error(api.ctx));
}

bool feed_tabix_track(TabixWriter& w, const tbk_track_rows& r, const std::vector<std::string>& names, const TrackApi& api, bool* names_set, bool with_head,
                      uint64_t* device_text_bytes) {
  uint64_t text_bytes = 0;
  bool done = false;
  std::string err;
  const std::string none;
  const std::string& head = with_head ? w.head() : none;
  const uint64_t runs_before = w.runs();
  if (!getenv("TBK_TRACK_HOST_FMT")) {
    if (!*names_set) set_track_names(api, names), *names_set = true;
    tbk_ix_opts ix;
    memset(&ix, 0, sizeof(ix));
    ix.n_ref = (uint32_t)w.index().ref_len().size(), ix.reserved = w.index().ix_format(), ix.ref_len = w.index().ref_len().data();
    TbxBridge b{&w};
    uint64_t out_bytes = 0;
    const int rc = api.track_bgzf(api.ctx, &r, head.data(), (uint32_t)head.size(), &ix, TbxBridge::sink, &b, &text_bytes, &out_bytes);
    if (rc == 0) {
      done = true;
    } else {  // (a refusal before the call's first run hands these rows to the host path; behind one the file is broken)
      if (b.failed || w.runs() != runs_before) GError("Error: writing %s failed (%s: %s)\n", w.path().c_str(), api.strerror_(rc), api.last_error(api.ctx));
      fprintf(stderr, "Warning: the device track writer refused %s (%s: %s); the host writer takes it\n", w.path().c_str(), api.strerror_(rc),
              api.last_error(api.ctx));
    }
  }
  if (!done) {
    std::function<int(uint32_t, char*, size_t)> fmt;
    if (r.kind == TBK_TRACK_COV)
      fmt = [&](uint32_t i, char* b, size_t cap) { return fmt_cov_line(b, cap, names[r.tid[i]].c_str(), r.start[i], r.end[i], r.val[i]); };
    else if (r.kind == TBK_TRACK_JUNC)
      fmt = [&](uint32_t i, char* b, size_t cap) {
        return fmt_junc_line(b, cap, names[r.tid[i]].c_str(), r.start[i], r.end[i], (int)(r.first_junc + (int64_t)i), r.val[i], (char)r.strand[i]);
      };
    else
      fmt = [&](uint32_t i, char* b, size_t cap) { return fmt_samp_line(b, cap, names[r.tid[i]].c_str(), r.start[i], r.end[i], r.count[i], r.heat[i]); };
    if (!tabix_host_track(w, r.n, r.tid, r.start, r.end, fmt, host_slice_rows(), worker_count(), err, with_head))
      GError("Error: writing %s failed (%s)\n", w.path().c_str(), err.c_str());
  }
  if (device_text_bytes) *device_text_bytes = text_bytes;
  return done;
}

void write_tabix_track(TabixWriter& w, const tbk_track_rows& r, const std::vector<std::string>& names, const TrackApi& api, bool* names_set) {
  const auto t0 = std::chrono::steady_clock::now();
  const char* kinds[3] = {"coverage", "junctions", "samples"};
  uint64_t text_bytes = 0;
  const bool done = feed_tabix_track(w, r, names, api, names_set, true, &text_bytes);
  const char* writer = done ? "device" : "host";
  std::string err;
  if (!w.close(err)) GError("Error: writing %s failed (%s)\n", w.path().c_str(), err.c_str());
  if (getenv("TBK_TIMING"))
    fprintf(stderr, "tabix phase ms: writer %s | %s | %u rows | %llu text bytes | %llu gz bytes | %.1f\n", writer, kinds[r.kind], r.n,
            (unsigned long long)(done ? text_bytes : w.text_bytes()), (unsigned long long)w.bytes(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

}  // namespace tbh
