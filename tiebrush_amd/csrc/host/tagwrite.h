// tagwrite.h — flushPData's tagging of one output record (/root/reference/src/tiebrush.cpp:506-525, GSam.h:300-305): the
// representative takes YC:f (always), YX:i (always, width by value) and YD:i (only when positive; an older YD is removed), then is
// framed for the BAM stream.  Shared by the single-GPU command line and the multi-rank writer (tbh_capi.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "bai.h"
#include "bam.h"

namespace tbh {

// appends `block_size | record + tags` of one group to `o`; `scratch` is a BamRec the caller keeps per thread
void append_tagged(const RecView& v, double yc, int64_t yx, int32_t yd, std::vector<uint8_t>& o, BamRec& scratch);

// the groups [g0, g1) of a run, tagged, framed and deflated into whole BGZF members appended to `members`; rec(g) hands out the
// representative of group g.  false when the deflate fails.
template <class RecOf>
bool tag_and_deflate(uint32_t g0, uint32_t g1, RecOf rec, const double* yc, const int64_t* yx, const int32_t* yd, int level, std::vector<uint8_t>& framed,
                     BamRec& scratch, std::vector<uint8_t>& members, std::vector<BaiRec>* ix_recs = nullptr);

}  // namespace tbh

#include "bgzf.h"
namespace tbh {
template <class RecOf>
bool tag_and_deflate(uint32_t g0, uint32_t g1, RecOf rec, const double* yc, const int64_t* yx, const int32_t* yd, int level, std::vector<uint8_t>& framed,
                     BamRec& scratch, std::vector<uint8_t>& members, std::vector<BaiRec>* ix_recs) {
  framed.clear();
  if (ix_recs) ix_recs->clear();
  for (uint32_t g = g0; g < g1; ++g) {
    const size_t at = framed.size();
    append_tagged(rec(g), yc[g], yx[g], yd[g], framed, scratch);
    if (ix_recs) {  // the output's index (bai.h): the record's span and where it starts in the slice's payload
      BaiRec r;
      if (!bai_rec_span(framed.data() + at + 4, framed.size() - at - 4, &r.tid, &r.beg, &r.end)) return false;
      r.vbeg = at;
      ix_recs->push_back(r);
    }
  }
  // BGZF members are independent deflate streams: the slice compresses itself, the writer only appends
  if (!bgzf_deflate_members(framed.data(), framed.size(), level, members)) return false;
  if (ix_recs) {
    std::string err;
    return bai_member_voffsets(members.data(), members.size(), *ix_recs, err);
  }
  return true;
}

// flushPData's tagging of the groups [0, n) (tiebrush.cpp:506-525): the groups are independent, so `threads` workers tag, frame and
// deflate slices of them (tag_and_deflate), taking the next slice as they come free (a static split leaves the cores that drew sparse
// regions idle).  The calling thread hands every slice's BGZF members to emit(data, size) in slice order, as soon as that slice and all
// earlier ones are out.  Slices: one when n < 4096 or per == 0, otherwise `per` groups each.  Slice ends are member ends: the rule
// fixes the output's bytes.  false when a deflate fails or emit returns false.  With slice_recs (the output's index, bai.h), slice k's
// records — span and virtual offset relative to the slice's first member — are in (*slice_recs)[k] when emit is called for it.
template <class RecOf, class Emit>
bool tag_deflate_ordered(uint32_t n, RecOf rec_of, const double* yc, const int64_t* yx, const int32_t* yd, int level, int threads, Emit emit,
                         uint32_t per = 16384, std::vector<std::vector<BaiRec>>* slice_recs = nullptr) {
  const int nt = n < 4096 ? 1 : std::max(1, threads);
  if (n < 4096 || per == 0) per = n ? n : 1;
  const uint32_t nsl = n ? (n + per - 1) / per : 0;
  std::vector<std::vector<uint8_t>> runs((size_t)nsl);
  if (slice_recs) slice_recs->assign((size_t)nsl, std::vector<BaiRec>());
  std::vector<std::atomic<int>> ready(nsl);  // (value-initialised: 0)
  std::atomic<uint32_t> next_slice{0};
  // the emitting thread sleeps until the slice it needs is out (no spinning beside fully subscribed workers); a worker that fails
  // says so here and the calling thread reports it once every worker has stopped
  std::mutex ready_m;
  std::condition_variable ready_cv;
  std::atomic<bool> failed{false};
  auto worker = [&]() {
    std::vector<uint8_t> o;
    o.reserve((size_t)per * 96);
    BamRec rr;
    for (;;) {
      const uint32_t sl = next_slice.fetch_add(1);
      if (sl >= nsl) break;
      // (after a failure: stop working, but let the emitter's wait for this slice end)
      const uint32_t g0 = sl * per;
      if (!failed.load() && !tag_and_deflate(g0, g0 + std::min(per, n - g0), rec_of, yc, yx, yd, level, o, rr, runs[(size_t)sl],
                                              slice_recs ? &(*slice_recs)[(size_t)sl] : nullptr))
        failed.store(true);
      std::lock_guard<std::mutex> lk(ready_m);
      ready[sl].store(1, std::memory_order_release);
      ready_cv.notify_all();
    }
  };
  std::vector<std::thread> th;
  if (nt > 1)
    for (int t = 0; t < nt; ++t) th.emplace_back(worker);
  else
    worker();
  for (uint32_t sl = 0; sl < nsl; ++sl) {
    if (!ready[sl].load(std::memory_order_acquire)) {
      std::unique_lock<std::mutex> lk(ready_m);
      ready_cv.wait(lk, [&] { return ready[sl].load(std::memory_order_acquire) != 0; });
    }
    if (failed.load()) break;
    if (!emit(runs[(size_t)sl].data(), runs[(size_t)sl].size())) {
      failed.store(true);
      break;
    }
    std::vector<uint8_t>().swap(runs[(size_t)sl]);
  }
  for (auto& x : th) x.join();
  return !failed.load();
}
}  // namespace tbh
