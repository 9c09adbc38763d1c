// bigwig.hip — the sections of a bigWig file built on the device (tbk_bigwig_build): what host/bigwig.cpp's BigWigWriter::close does
// with its rows on one core — the data sections, the zoom plan, the zoom records, and a compress2 call per section — as kernels.  The
// host writer is the specification, quirks included; the file's layout (header, chromosome tree, R-trees, summary) stays with it.
//
//   bw_check_k         a thread per row: the rules the host writer assumes (sorted by (tid, start), disjoint, end > start >= 0, tid known)
//                      and the covered bases (an integer sum: any order)
//   bw_chrom_first_k   a thread per chromosome: where its items begin (a binary search: the items are sorted), its sections
//   bw_sections_k      a thread per section: its chromosome, first item, count, R-tree key, and its cut in the payload run — a closed
//                      form, 24 s + 12 f for the data (s sections and f rows before it), 32 f for a zoom level: no scan of sizes
//   bw_pack_data_k     a block per data section: the 24-byte header and 12 bytes a row, as consecutive dwords
//   bw_zoom_count_k    a thread per row: the zoom records it opens at one reduction = the bins it touches, less one when its first bin is
//                      the previous row's last on the same chromosome
//   bw_zoom_fill_k     a thread per record: finds its opener in the scanned counts and walks the rows of its bin IN ROW ORDER — the
//                      sums are sequential float products and adds, the host's own order, so the floats are the host's bit for bit.
//                      The coarse levels are therefore a few long chains; that is the price of the contract (DESIGN.md 4h has the
//                      measurement), and it is not bought back with a tree or wave reduction.
// The records of a zoom level are their sections' payload as they lie (no header).  Every level's run goes through bgzdef.hip's
// deflater with zlib framing (tbk_zlib_sections) and out through two pinned slices, like tbk_format_track's text.
//
// Byte and integer work plus one float chain per record: no MFMA; the build is paced by the deflater (LDS round trips) and, at the
// coarsest levels, by the length of the longest chain.
#include <algorithm>
#include <vector>

#include "dev_common.hpp"
#include "tbk_internal.h"

namespace {

constexpr uint32_t BW_ITEMS = 1024;  // items per section (the host writer's ITEMS_PER_SLOT)
constexpr int BW_NT = 256;

enum : uint32_t { BW_ERR_TID = 1, BW_ERR_RANGE = 2, BW_ERR_ORDER = 4, BW_ERR_OVERLAP = 8 };

struct BwRows {
  uint32_t n;
  const int32_t *tid, *start, *end;
  const double* val;
};

// stat[0] |= the rules a row breaks; *covered += end - start
__global__ void __launch_bounds__(BW_NT) bw_check_k(BwRows R, uint32_t n_ref, uint32_t* stat, unsigned long long* covered) {
  const uint32_t i = blockIdx.x * BW_NT + threadIdx.x;
  uint32_t err = 0;
  unsigned long long w = 0;
  if (i < R.n) {
    const int32_t t = R.tid[i], s = R.start[i], e = R.end[i];
    if (t < 0 || (uint32_t)t >= n_ref) err |= BW_ERR_TID;
    if (s < 0 || e <= s) err |= BW_ERR_RANGE;
    if (i > 0) {
      const int32_t pt = R.tid[i - 1], ps = R.start[i - 1], pe = R.end[i - 1];
      if (pt > t || (pt == t && ps > s)) err |= BW_ERR_ORDER;
      else if (pt == t && pe > s) err |= BW_ERR_OVERLAP;
    }
    if (!err) w = (unsigned long long)(uint32_t)(e - s);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    err |= (uint32_t)__shfl_xor((int)err, d);
    w += (unsigned long long)__shfl_xor((long long)w, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (err) atomicOr(&stat[0], err);
    if (w) atomicAdd(covered, w);
  }
}

// first index in [0, n) whose key (key[idx * stride]) is >= t
__device__ __forceinline__ uint32_t bw_lower(const uint32_t* key, uint32_t stride, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (key[(size_t)mid * stride] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// first[t] (t <= n_ref) = the first item of chromosome t among n items sorted by chromosome; nsec[t] = its sections (0 for t == n_ref)
__global__ void __launch_bounds__(BW_NT) bw_chrom_first_k(const uint32_t* key, uint32_t stride, uint32_t n, uint32_t n_ref, uint32_t* first, uint32_t* nsec) {
  const uint32_t t = blockIdx.x * BW_NT + threadIdx.x;
  if (t > n_ref) return;
  const uint32_t a = bw_lower(key, stride, n, t);
  first[t] = a;
  uint32_t ns = 0;
  if (t < n_ref) {
    const uint32_t b = bw_lower(key, stride, n, t + 1);
    ns = (b - a + BW_ITEMS - 1) / BW_ITEMS;
  }
  nsec[t] = ns;
}

// section s: sec[s] = {chrom, start, end, count}, sec_first[s] = its first item, cut[s] = its first payload byte (cut[nsec] = the run's
// size).  item_words: 0 = data rows (start / end columns), 8 = zoom records (recs[8 i + 1], recs[8 i + 2])
__global__ void __launch_bounds__(BW_NT) bw_sections_k(uint32_t nsec, uint32_t n_items, uint32_t n_ref, const uint32_t* first, const uint32_t* secbase,
                                                       const int32_t* start, const int32_t* end, const uint32_t* recs, uint4* sec, uint32_t* sec_first,
                                                       uint64_t* cut) {
  const uint32_t s = blockIdx.x * BW_NT + threadIdx.x;
  if (s > nsec) return;
  const bool zoom = recs != nullptr;
  if (s == nsec) {
    cut[s] = zoom ? 32ull * n_items : 24ull * nsec + 12ull * n_items;
    return;
  }
  // the last chromosome whose base is <= s (the ones before it with the same base have no sections)
  uint32_t lo = 0, hi = n_ref + 1;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (secbase[mid] <= s) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t t = lo - 1;
  const uint32_t f = first[t] + (s - secbase[t]) * BW_ITEMS;
  const uint32_t cnt = min(BW_ITEMS, first[t + 1] - f);
  const uint32_t l = f + cnt - 1;
  uint4 v;
  v.x = t;
  v.y = zoom ? recs[(size_t)f * 8 + 1] : (uint32_t)start[f];
  v.z = zoom ? recs[(size_t)l * 8 + 2] : (uint32_t)end[l];
  v.w = cnt;
  sec[s] = v;
  sec_first[s] = f;
  cut[s] = zoom ? 32ull * f : 24ull * s + 12ull * f;
}

// the payload of data section blockIdx.x: chrom, start, end, itemStep 0, itemSpan 0, type 1 (bedGraph), 0, count; then start, end, value per row
__global__ void __launch_bounds__(BW_NT) bw_pack_data_k(BwRows R, const uint4* sec, const uint32_t* sec_first, const uint64_t* cut, uint32_t* out) {
  const uint32_t s = blockIdx.x;
  const uint4 h = sec[s];
  const uint32_t f = sec_first[s], cnt = h.w;
  uint32_t* o = out + (cut[s] >> 2);  // (24 s + 12 f: a multiple of 4)
  if (threadIdx.x < 6) {
    const uint32_t hw[6] = {h.x, h.y, h.z, 0u, 0u, 1u | cnt << 16};
    o[threadIdx.x] = hw[threadIdx.x];
  }
  o += 6;
  for (uint32_t w = threadIdx.x; w < 3 * cnt; w += BW_NT) {
    const uint32_t j = w / 3, c = w - 3 * j;
    uint32_t v;
    if (c == 0) v = (uint32_t)R.start[f + j];
    else if (c == 1) v = (uint32_t)R.end[f + j];
    else v = __float_as_uint((float)R.val[f + j]);
    o[w] = v;
  }
}

// opens[i] = the zoom records row i opens at reduction red (opens[n] = 0: the scan's last output is the level's record count)
__global__ void __launch_bounds__(BW_NT) bw_zoom_count_k(BwRows R, uint32_t red, uint32_t* opens) {
  const uint32_t i = blockIdx.x * BW_NT + threadIdx.x;
  if (i > R.n) return;
  uint32_t c = 0;
  if (i < R.n) {
    const uint32_t b0 = (uint32_t)R.start[i] / red, b1 = ((uint32_t)R.end[i] - 1u) / red;
    c = b1 - b0 + 1;
    if (i > 0 && R.tid[i - 1] == R.tid[i] && ((uint32_t)R.end[i - 1] - 1u) / red == b0) --c;
  }
  opens[i] = c;
}

// zoom record r of the level: {chrom, start, end, valid, min, max, sum, sum of squares}.  BigWigWriter::close's inner loop for one bin:
// the opener sets start, end = min(be, max(chromLen, hi)) and min = max = its value; every row of the bin, opener first, in row order,
// adds hi - lo to valid, its value to min / max (std::min / std::max's own comparisons) and val * w, val * val * w to the float sums.
__global__ void __launch_bounds__(BW_NT) bw_zoom_fill_k(BwRows R, uint32_t red, const uint64_t* ooff, uint32_t nrec, const uint32_t* ref_len, uint4* recs) {
  const uint32_t r = blockIdx.x * BW_NT + threadIdx.x;
  if (r >= nrec) return;
  // the opener: the last row whose offset is <= r (rows that open nothing share their successor's offset)
  uint32_t lo = 0, hi_ = R.n + 1;
  while (lo < hi_) {
    const uint32_t mid = lo + ((hi_ - lo) >> 1);
    if (ooff[mid] <= (uint64_t)r) lo = mid + 1;
    else hi_ = mid;
  }
  const uint32_t i = lo - 1;
  const int32_t t = R.tid[i];
  uint32_t b = (uint32_t)R.start[i] / red + (r - (uint32_t)ooff[i]);
  if (i > 0 && R.tid[i - 1] == t && ((uint32_t)R.end[i - 1] - 1u) / red == (uint32_t)R.start[i] / red) ++b;
  const uint64_t bs64 = (uint64_t)b * red, be64 = (uint64_t)(b + 1) * red;
  const uint32_t bs = (uint32_t)bs64, be = (uint32_t)(be64 < 0xFFFFFFFFull ? be64 : 0xFFFFFFFFull);
  uint32_t rec_end = 0, valid = 0;
  float mn = 0.f, mx = 0.f, sum = 0.f, sq = 0.f;
  for (uint32_t j = i; j < R.n; ++j) {
    if (R.tid[j] != t) break;
    const uint32_t s = (uint32_t)R.start[j], e = (uint32_t)R.end[j];
    if (s >= be) break;
    const float v = (float)R.val[j];
    const uint32_t l = max(bs, s), h = min(be, e);
    if (j == i) {
      rec_end = min(be, max(ref_len[t], h));
      mn = mx = v;
    }
    const float w = (float)(h - l);
    valid += h - l;
    mn = v < mn ? v : mn;
    mx = mx < v ? v : mx;
    sum += v * w;
    sq += v * v * w;
  }
  recs[(size_t)r * 2] = make_uint4((uint32_t)t, bs, rec_end, valid);
  recs[(size_t)r * 2 + 1] = make_uint4(__float_as_uint(mn), __float_as_uint(mx), __float_as_uint(sum), __float_as_uint(sq));
}

struct BwState {
  std::vector<tbk_bw_section> tab[1 + TBK_BW_MAX_ZOOM];
};

// One level: `n_items` items sorted by chromosome (key / stride: their chromosome column) -> sections, payload run, zlib streams, table,
// sink.  Data level: recs == nullptr, the payload is packed here; zoom level: the payload is the records.
int bw_level(tbk_ctx* ctx, const BwRows& R, uint32_t L, uint32_t n_items, const uint32_t* recs, uint32_t n_ref, tbk_bw_sink sink, void* user,
             tbk_bw_out* out, BwState* S) {
  const bool zoom = recs != nullptr;
  uint32_t* first = ws_alloc<uint32_t>(ctx, (size_t)n_ref + 1);
  uint32_t* nsecs = ws_alloc<uint32_t>(ctx, (size_t)n_ref + 1);
  uint32_t* secbase = ws_alloc<uint32_t>(ctx, (size_t)n_ref + 1);
  uint64_t* d_total = ws_alloc<uint64_t>(ctx, 1);
  if (!first || !nsecs || !secbase || !d_total) return TBK_ENOMEM;
  const uint32_t* key = zoom ? recs : (const uint32_t*)R.tid;
  TBK_LAUNCH(ctx, "bw_chrom_first_k", bw_chrom_first_k, cdiv((uint64_t)n_ref + 1, BW_NT), BW_NT, 0, key, zoom ? 8u : 1u, n_items, n_ref, first, nsecs);
  TBK_TRY(tbk_exscan_u32(ctx, nsecs, secbase, n_ref + 1, d_total));
  uint64_t nsec64 = 0;
  TBK_HIP(hipMemcpyAsync(&nsec64, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "bw_chrom_first_k"));
  if (nsec64 >= (1ull << 31)) return TBK_EUNSUPPORTED;
  const uint32_t nsec = (uint32_t)nsec64;
  uint4* d_sec = ws_alloc<uint4>(ctx, nsec);
  uint32_t* d_sec_first = ws_alloc<uint32_t>(ctx, nsec);
  uint64_t* d_cut = ws_alloc<uint64_t>(ctx, (size_t)nsec + 1);
  if (!d_sec || !d_sec_first || !d_cut) return TBK_ENOMEM;
  TBK_LAUNCH(ctx, "bw_sections_k", bw_sections_k, cdiv((uint64_t)nsec + 1, BW_NT), BW_NT, 0, nsec, n_items, n_ref, first, secbase, R.start, R.end, recs, d_sec,
             d_sec_first, d_cut);
  const uint8_t* payload = (const uint8_t*)recs;
  if (!zoom) {
    uint32_t* pay = ws_alloc<uint32_t>(ctx, 6 * (size_t)nsec + 3 * (size_t)n_items + 4);
    if (!pay) return TBK_ENOMEM;
    TBK_LAUNCH(ctx, "bw_pack_data_k", bw_pack_data_k, nsec, BW_NT, 0, R, d_sec, d_sec_first, d_cut, pay);
    payload = (const uint8_t*)pay;
  }
  TBK_TRY(tbk_check_launch(ctx, "bw_sections_k"));
  uint8_t* packed = nullptr;
  uint64_t total = 0;
  const uint64_t* d_zoff = nullptr;
  TBK_TRY(tbk_zlib_sections(ctx, payload, d_cut, nsec, &packed, &total, &d_zoff));
  // ---- the level's table (complete before its first byte goes out) ----
  std::vector<uint4> sec(nsec);
  std::vector<uint64_t> zoff((size_t)nsec + 1), cut((size_t)nsec + 1);
  TBK_HIP(hipMemcpyAsync(sec.data(), d_sec, (size_t)nsec * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(zoff.data(), d_zoff, zoff.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(cut.data(), d_cut, cut.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<tbk_bw_section>& tab = S->tab[L];
  tab.resize(nsec);
  uint32_t max_payload = 0;
  for (uint32_t s = 0; s < nsec; ++s) {
    tab[s] = tbk_bw_section{sec[s].x, sec[s].y, sec[s].z, 0, zoff[s], zoff[s + 1] - zoff[s]};
    max_payload = std::max(max_payload, (uint32_t)(cut[s + 1] - cut[s]));
  }
  tbk_bw_level& lv = out->level[L];
  lv.max_payload = max_payload;
  lv.n_sections = nsec;
  lv.bytes = total;
  lv.sections = tab.data();
  // ---- the bytes, in slices of whole sections: slice k + 1 is copied out while the sink takes slice k ----
  const uint64_t cap = ctx->dbg.fmt_slice ? ctx->dbg.fmt_slice : ((uint64_t)32 << 20);
  std::vector<uint32_t> sl{0};  // slice k = sections [sl[k], sl[k + 1])
  for (uint32_t s = 0; s < nsec;) {
    uint32_t e = s + 1;
    while (e < nsec && zoff[e + 1] - zoff[s] <= cap) ++e;
    sl.push_back(e);
    s = e;
  }
  const uint32_t ns = (uint32_t)sl.size() - 1;
  uint64_t slice_max = 0;
  for (uint32_t k = 0; k < ns; ++k) slice_max = std::max(slice_max, zoff[sl[k + 1]] - zoff[sl[k]]);
  TBK_TRY(tbk_pin_slices(ctx, slice_max));
  hipEvent_t ev[2] = {tbk_event(ctx), tbk_event(ctx)};
  if (!ev[0] || !ev[1]) return TBK_EHIP;
  int rc = 0;
  for (uint32_t k = 0; k <= ns && rc == 0; ++k) {
    if (k < ns) {
      TBK_HIP(hipMemcpyAsync(ctx->fmt_pin[k & 1], packed + zoff[sl[k]], zoff[sl[k + 1]] - zoff[sl[k]], hipMemcpyDeviceToHost, ctx->stream));
      TBK_HIP(hipEventRecord(ev[k & 1], ctx->stream));
    }
    if (k > 0) {
      const uint32_t p = k - 1;
      TBK_HIP(hipEventSynchronize(ev[p & 1]));
      if (sink(user, L, (const uint8_t*)ctx->fmt_pin[p & 1], zoff[sl[p + 1]] - zoff[sl[p]]) != 0) {
        ctx->last_error = "tbk_bigwig_build: the sink refused a slice";
        rc = TBK_EINVAL;
      }
    }
  }
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return rc;
}

}  // namespace

void tbk_bw_free(tbk_ctx* ctx) {
  delete (BwState*)ctx->bw;
  ctx->bw = nullptr;
}

int tbk_bigwig_device(tbk_ctx* ctx, const tbk_track_rows* rows, uint32_t n_ref, const uint32_t* ref_len, tbk_bw_sink sink, void* user, tbk_bw_out* out) {
  BwRows R{rows->n, rows->tid, rows->start, rows->end, rows->val};
  const uint32_t n = R.n;
  if (!ctx->bw) ctx->bw = new BwState();
  BwState* S = (BwState*)ctx->bw;
  for (auto& t : S->tab) t.clear();
  // ---- every row against the rules, before anything else is done with it ----
  uint32_t* stat = ws_alloc<uint32_t>(ctx, 4);
  unsigned long long* d_cov = ws_alloc<unsigned long long>(ctx, 1);
  uint32_t* d_len = ws_alloc<uint32_t>(ctx, (size_t)n_ref + 1);
  if (!stat || !d_cov || !d_len) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(stat, 0, 4 * sizeof(uint32_t), ctx->stream));
  TBK_HIP(hipMemsetAsync(d_cov, 0, sizeof(unsigned long long), ctx->stream));
  if (n_ref) TBK_HIP(hipMemcpyAsync(d_len, ref_len, (size_t)n_ref * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  TBK_LAUNCH(ctx, "bw_check_k", bw_check_k, cdiv(n, BW_NT), BW_NT, 0, R, n_ref, stat, d_cov);
  uint32_t errb = 0;
  unsigned long long covered = 0;
  TBK_HIP(hipMemcpyAsync(&errb, stat, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&covered, d_cov, sizeof(covered), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "bw_check_k"));
  if (errb) {
    ctx->last_error = (errb & BW_ERR_TID)     ? "tbk_bigwig_build: a row's reference index is outside [0, n_ref)"
                      : (errb & BW_ERR_RANGE) ? "tbk_bigwig_build: a row with a negative start or end <= start"
                      : (errb & BW_ERR_ORDER) ? "tbk_bigwig_build: rows not sorted by (tid, start)"
                                              : "tbk_bigwig_build: rows that overlap";
    return TBK_EINVAL;
  }
  // ---- the zoom plan (BigWigWriter::close): one count pass and one small read-back a level ----
  uint32_t* opens = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint64_t* ooff = ws_alloc<uint64_t>(ctx, (size_t)n + 1);
  uint64_t* d_total = ws_alloc<uint64_t>(ctx, 1);
  if (!opens || !ooff || !d_total) return TBK_ENOMEM;
  uint32_t nz = 0;
  uint32_t reds[TBK_BW_MAX_ZOOM];
  uint64_t nrecs[TBK_BW_MAX_ZOOM];
  uint64_t red = std::max<uint64_t>(32, 4 * (covered / n + 1));
  for (int z = 0; z < TBK_BW_MAX_ZOOM && red < (1ull << 31); ++z, red *= 4) {
    TBK_LAUNCH(ctx, "bw_zoom_count_k", bw_zoom_count_k, cdiv((uint64_t)n + 1, BW_NT), BW_NT, 0, R, (uint32_t)red, opens);
    TBK_TRY(tbk_exscan_u32_u64(ctx, opens, ooff, n + 1, d_total));
    uint64_t cnt = 0;
    TBK_HIP(hipMemcpyAsync(&cnt, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    TBK_TRY(tbk_check_launch(ctx, "bw_zoom_count_k"));
    if (z > 0 && cnt * 2 > nrecs[nz - 1]) break;  // no longer shrinking
    if (cnt >= (1ull << 31)) {
      ctx->last_error = "tbk_bigwig_build: a zoom level of 2^31 records or more";
      return TBK_EUNSUPPORTED;
    }
    reds[nz] = (uint32_t)red, nrecs[nz] = cnt, ++nz;
    if (cnt < 1000) break;
  }
  out->n_levels = 1 + nz;
  out->level[0].n_items = n;
  for (uint32_t z = 0; z < nz; ++z) out->level[1 + z].reduction = reds[z], out->level[1 + z].n_items = nrecs[z];
  // ---- the data, then the zoom levels ----
  TBK_TRY(bw_level(ctx, R, 0, n, nullptr, n_ref, sink, user, out, S));
  for (uint32_t z = 0; z < nz; ++z) {
    const uint32_t nrec = (uint32_t)nrecs[z];
    // (the level's offsets again: a count pass and a scan are cheaper than keeping n offsets per planned level)
    TBK_LAUNCH(ctx, "bw_zoom_count_k", bw_zoom_count_k, cdiv((uint64_t)n + 1, BW_NT), BW_NT, 0, R, reds[z], opens);
    TBK_TRY(tbk_exscan_u32_u64(ctx, opens, ooff, n + 1, d_total));
    uint4* recs = ws_alloc<uint4>(ctx, (size_t)nrec * 2);
    if (!recs) return TBK_ENOMEM;
    // (a name per level for the event timing: the coarsest level's few long chains are what the ordered float sums cost)
    static const char* const fill_name[TBK_BW_MAX_ZOOM] = {"bw_zoom_fill_k.z0", "bw_zoom_fill_k.z1", "bw_zoom_fill_k.z2", "bw_zoom_fill_k.z3",
                                                           "bw_zoom_fill_k.z4", "bw_zoom_fill_k.z5", "bw_zoom_fill_k.z6", "bw_zoom_fill_k.z7",
                                                           "bw_zoom_fill_k.z8", "bw_zoom_fill_k.z9"};
    TBK_LAUNCH(ctx, fill_name[z], bw_zoom_fill_k, cdiv(nrec, BW_NT), BW_NT, 0, R, reds[z], ooff, nrec, d_len, recs);
    TBK_TRY(tbk_check_launch(ctx, "bw_zoom_fill_k"));
    TBK_TRY(bw_level(ctx, R, 1 + z, nrec, (const uint32_t*)recs, n_ref, sink, user, out, S));
  }
  return 0;
}
