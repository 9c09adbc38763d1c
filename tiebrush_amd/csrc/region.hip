// region.hip — the device side of `tiecov -r` / `-R`: the records of a decoded tile that overlap a region table U
// as tiecov's input view (tbk_region_view, tbk_regions_view), and the rows of a coverage / sample call cut to U (tbk_cov_clip,
// tbk_sample_clip and their _regions forms); and of `tiebrush -r` / `-R`: the same records as a collapse tile
// (tbk_tile_region, tbk_tile_regions, at the end of this file).
//
// There is ONE path: a table of R sorted, disjoint intervals on the device.  A one-region entry builds the table of its one interval
// (which, unlike a caller's table, may be empty) and runs what the table entry runs; the two families differ in their extern "C"
// wrappers' argument checks and nowhere else.
//
// The reference has no region option (tiecov.cpp walks the whole file); the contract is that the rows equal the whole-file run's rows
// on the region, bit for bit.  These are bandwidth-trivial passes of one thread per record or row, each kernel a launch of its own
// (no hand-off between workgroups inside a launch); what can go wrong is at the edges: n = 0, the last partial wave, an end beyond 2^31.
//   rs_flag_k      keep[i] = the record overlaps any interval of U, by ONE bisection of U per record (the first interval that ends
//                  behind pos decides); rec_end by the index's rule (pos + the CIGAR's reference length over M D N = X, pos + 1 when
//                  that is 0); kcig[i] = the kept record's CIGAR count
//   two exclusive scans (tbk_exscan_u32) over keep and kcig, n + 1 elements each: the last ones are the totals
//   rv_scatter_k   the compacted tid / pos / flag / strand / yc / yx, the CSR cig_off and the gathered CIGAR words, in file order
//   clip_order_k   interval rows that are not sorted and disjoint are refused (they could overflow the scan below)
//   clip_mrange_k  interval rows are sorted and disjoint: the rows of an interval of U are one range, found by two bisections, a thread
//                  per interval: first[r], count[r]; a scan of the counts: off[r], m
//   clip_rows_k    a thread per OUTPUT row: its interval by a bisection of off, its source row, trimmed to that interval, into scratch
//                  (then copied over the caller's rows); one template for the coverage rows (val) and the sample rows (count, heat)
//   clip_mjflag_k / clip_jscat_k   junction rows are only sorted inside a bundle: keep flag (rs_flag_k's single probe of U), scan,
//                  scatter; rows are not trimmed
#include "dev_common.hpp"
#include "tbk_internal.h"

namespace {

constexpr int RG_NT = 256;

// the end of a record by the index's rule: pos + the reference length of its nc CIGAR words at cig + c0 over M D N = X, pos + 1 when that is 0
__device__ __forceinline__ int64_t rec_end_of(int64_t p, const uint32_t* __restrict__ cig, uint32_t c0, uint32_t nc) {
  int64_t rl = 0;
  for (uint32_t q = 0; q < nc; ++q) {
    const uint32_t w = cig[c0 + q];
    if ((0x18Du >> (w & 15u)) & 1u) rl += (int64_t)(w >> 4);
  }
  return p + (rl ? rl : 1);
}

// ---- a region table U on the device: R >= 1 sorted, disjoint, non-adjacent intervals in global memory; a caller's table
// has no empty interval, the table of a one-region entry may be one ----------------------------------------------------------------------
struct RegTab {
  uint32_t n;
  const int32_t* tid;
  const int64_t *beg, *end;
};
// the first interval with (tid, end) > (t, p) in lexicographic order (n: none).  U is disjoint and sorted, so its ends ascend with its
// begins: every interval before that one ends at or before p, every one behind it begins later than it does — [p, e) on t overlaps ANY
// interval exactly when that one lies on t and begins before e.  (The one empty interval [b, b): found when p < b, met when b < e.)
__device__ __forceinline__ uint32_t tab_probe(const RegTab& U, int32_t t, int64_t p) {
  uint32_t lo = 0, hi = U.n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    const int32_t mt = U.tid[m];
    if (mt > t || (mt == t && U.end[m] > p))
      hi = m;
    else
      lo = m + 1;
  }
  return lo;
}
__device__ __forceinline__ bool tab_overlaps(const RegTab& U, int32_t t, int64_t p, int64_t e) {
  const uint32_t r = tab_probe(U, t, p);
  return r < U.n && U.tid[r] == t && U.beg[r] < e;
}

// Records arrive in file order: the probes of a wave fall on a few neighbouring entries of the table, which stays in global memory.
__global__ __launch_bounds__(RG_NT) void rs_flag_k(uint32_t n, const int32_t* __restrict__ tid, const int32_t* __restrict__ pos,
                                                   const uint32_t* __restrict__ cig_off, const uint32_t* __restrict__ cig, RegTab U,
                                                   uint32_t* __restrict__ keep /* [n + 1] */, uint32_t* __restrict__ kcig /* [n + 1] */) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i > n) return;
  uint32_t k = 0, kc = 0;
  if (i < n) {
    const uint32_t c0 = cig_off[i], nc = cig_off[i + 1] - c0;
    const int64_t p = pos[i];
    const int32_t t = tid[i];
    const uint32_t r = tab_probe(U, t, p);
    // (the CIGAR is walked only for a record that starts before its candidate interval)
    if (r < U.n && U.tid[r] == t && (U.beg[r] <= p || U.beg[r] < rec_end_of(p, cig, c0, nc))) k = 1, kc = nc;
  }
  keep[i] = k;
  kcig[i] = kc;
}

struct RvOut {
  int32_t *tid, *pos;
  uint16_t* flag;
  uint8_t* strand;
  double* yc;
  int64_t* yx;
  uint32_t *cig_off, *cig;
};

__global__ __launch_bounds__(RG_NT) void rv_scatter_k(uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ koff /* [n + 1] */,
                                                      const uint32_t* __restrict__ coff /* [n + 1] */, const int32_t* __restrict__ tid,
                                                      const int32_t* __restrict__ pos, const uint16_t* __restrict__ flag, const uint8_t* __restrict__ strand,
                                                      const uint32_t* __restrict__ cig_off, const uint32_t* __restrict__ cig, const double* __restrict__ yc,
                                                      const int64_t* __restrict__ yx, const uint8_t* __restrict__ seen, RvOut O) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i > n) return;
  if (i == n) {  // the CSR's closing offset
    O.cig_off[koff[n]] = coff[n];
    return;
  }
  if (!keep[i]) return;
  const uint32_t o = koff[i], d = coff[i];
  const uint32_t sn = seen ? seen[i] : 3u;
  O.tid[o] = tid[i];
  O.pos[o] = pos[i];
  O.flag[o] = flag[i];
  O.strand[o] = strand[i];
  O.yc[o] = (yc && (sn & 1u)) ? yc[i] : 1.0;          // tiecov.cpp:482-485: YC absent -> 1.0, YX absent -> 1; a present YC:f:0 stays 0
  O.yx[o] = (yx && (sn & 2u)) ? yx[i] : (int64_t)1;
  O.cig_off[o] = d;
  const uint32_t c0 = cig_off[i], nc = cig_off[i + 1] - c0;
  for (uint32_t q = 0; q < nc; ++q) O.cig[d + q] = cig[c0 + q];
}

// ---- the clips: an interval row may come out once per interval of U that it meets, so the rows can grow (m <= n + R - 1) ----
// A thread per interval r of U: first[r] = the first row that ends behind beg on its reference (or lies on a later one), then the first
// row that starts at or behind end there (or lies on a later one): rows [first[r], first[r] + count[r]) meet interval r; count[R] = 0
// closes the scan.  The second bisection starts at the first one's result: first + count <= n whatever the rows' order.
__global__ __launch_bounds__(RG_NT) void clip_mrange_k(RegTab U, uint32_t n, const int32_t* __restrict__ tid, const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ endv, uint32_t* __restrict__ first /* [R] */,
                                                       uint32_t* __restrict__ count /* [R + 1] */) {
  const uint64_t r = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (r > U.n) return;
  if (r == U.n) {
    count[r] = 0;
    return;
  }
  const int32_t rtid = U.tid[r];
  const int64_t beg = U.beg[r], end = U.end[r];
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (tid[m] > rtid || (tid[m] == rtid && (int64_t)endv[m] > beg))
      hi = m;
    else
      lo = m + 1;
  }
  const uint32_t f = lo;
  hi = n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (tid[m] > rtid || (tid[m] == rtid && (int64_t)start[m] >= end))
      hi = m;
    else
      lo = m + 1;
  }
  first[r] = f;
  count[r] = lo - f;
}
// *bad = 1 when a row ends before it starts, lies on an earlier reference than its predecessor or starts before that one ends: rows that
// are sorted and disjoint give m <= n + R - 1, anything else could overflow the scan (*bad is zeroed before the launch; every writer
// stores the same 1)
__global__ __launch_bounds__(RG_NT) void clip_order_k(uint32_t n, const int32_t* __restrict__ tid, const int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ endv, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i >= n) return;
  if (endv[i] < start[i] || (i + 1 < n && (tid[i + 1] < tid[i] || (tid[i + 1] == tid[i] && start[i + 1] < endv[i])))) *bad = 1u;
}

__device__ __forceinline__ int32_t clip_lo(int32_t s, int64_t beg) { return (int64_t)s < beg ? (int32_t)beg : s; }
__device__ __forceinline__ int32_t clip_hi(int32_t e, int64_t end) { return (int64_t)e > end ? (int32_t)end : e; }

// Output row i: its interval r is the last one whose scanned offset is <= i (off[R] = m > i), its source row first[r] + (i - off[r]).
// The payload columns ride along: a (coverage: val; sample: count) and, where the rows have a second one, b (sample: heat; else NULL).
template <class A, class B>
__global__ __launch_bounds__(RG_NT) void clip_rows_k(uint32_t m, RegTab U, const uint32_t* __restrict__ off /* [R + 1] */, const uint32_t* __restrict__ first,
                                                     const int32_t* __restrict__ tid, const int32_t* __restrict__ start, const int32_t* __restrict__ endv,
                                                     const A* __restrict__ a, const B* __restrict__ b, int32_t* __restrict__ o_tid,
                                                     int32_t* __restrict__ o_start, int32_t* __restrict__ o_end, A* __restrict__ o_a, B* __restrict__ o_b) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i >= m) return;
  uint32_t lo = 0, hi = U.n;  // the first r in [0, R] with off[r] > i
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] > i)
      hi = mid;
    else
      lo = mid + 1;
  }
  const uint32_t r = lo - 1;  // (off[0] = 0 <= i: lo >= 1)
  const uint32_t s = first[r] + ((uint32_t)i - off[r]);
  o_tid[i] = tid[s];
  o_start[i] = clip_lo(start[s], U.beg[r]);
  o_end[i] = clip_hi(endv[s], U.end[r]);
  o_a[i] = a[s];
  if (b) o_b[i] = b[s];
}
// a junction row is kept when it overlaps any interval of U: rs_flag_k's one probe, with j_start / j_end
__global__ __launch_bounds__(RG_NT) void clip_mjflag_k(uint32_t n, const int32_t* __restrict__ tid, const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ endv, RegTab U, uint32_t* __restrict__ keep /* [n + 1] */) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i > n) return;
  keep[i] = (i < n && tab_overlaps(U, tid[i], (int64_t)start[i], (int64_t)endv[i])) ? 1u : 0u;
}

__global__ __launch_bounds__(RG_NT) void clip_jscat_k(uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ koff,
                                                      const int32_t* __restrict__ tid, const int32_t* __restrict__ start, const int32_t* __restrict__ endv,
                                                      const uint8_t* __restrict__ strand, const double* __restrict__ val, int32_t* __restrict__ o_tid,
                                                      int32_t* __restrict__ o_start, int32_t* __restrict__ o_end, uint8_t* __restrict__ o_strand,
                                                      double* __restrict__ o_val) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const uint32_t o = koff[i];
  o_tid[o] = tid[i];
  o_start[o] = start[i];
  o_end[o] = endv[i];
  o_strand[o] = strand[i];
  o_val[o] = val[i];
}

// rows of the caller (host or device) -> device pointers: a device array as it is, a host array through a copy into the arena
template <class T>
int rows_in(tbk_ctx* ctx, int mem, const T* p, size_t n, const T** d) {
  if (mem == TBK_MEM_DEVICE) {
    *d = p;
    return 0;
  }
  T* a = ws_alloc<T>(ctx, n);
  if (!a) return TBK_ENOMEM;
  TBK_HIP(hipMemcpyAsync(a, p, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  *d = a;
  return 0;
}
// m clipped rows from scratch back over the caller's array
template <class T>
int rows_out(tbk_ctx* ctx, int mem, T* dst, const T* scratch, size_t m) {
  if (!m) return 0;
  TBK_HIP(hipMemcpyAsync(dst, scratch, m * sizeof(T), mem == TBK_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

struct ProfEnd {
  tbk_ctx* c;
  ~ProfEnd() { tbk_prof_end_call(c); }
};

// a one-region entry's region; it may be empty (`-r` of a BEG behind the reference's end gives one)
bool region_ok(int32_t tid, int64_t beg, int64_t end) { return tid >= 0 && beg >= 0 && end >= beg; }
// a caller's table: sorted by (tid, beg), disjoint, non-empty, non-adjacent; n >= 1, tid >= 0, beg >= 0
bool regions_ok(const tbk_regions* U) {
  if (!U || U->n == 0 || !U->tid || !U->beg || !U->end) return false;
  for (uint32_t r = 0; r < U->n; ++r) {
    if (U->tid[r] < 0 || U->beg[r] < 0 || U->end[r] <= U->beg[r]) return false;
    if (r && (U->tid[r] < U->tid[r - 1] || (U->tid[r] == U->tid[r - 1] && U->beg[r] <= U->end[r - 1]))) return false;
  }
  return true;
}
// The implementations below take a table that its wrapper has checked (on the host, before anything is launched or changed).
size_t tab_bytes(const tbk_regions& U) { return (size_t)U.n * 32 + 4096; }  // (the table and, for the clips, first / count / off)

// the device form of U, uploaded once per call into the workspace (after the call's tbk_ws_reserve)
int tab_upload(tbk_ctx* ctx, const tbk_regions& U, RegTab* T) {
  int32_t* t = ws_alloc<int32_t>(ctx, U.n);
  int64_t *b = ws_alloc<int64_t>(ctx, U.n), *e = ws_alloc<int64_t>(ctx, U.n);
  if (!t || !b || !e) return TBK_ENOMEM;
  TBK_HIP(hipMemcpyAsync(t, U.tid, (size_t)U.n * 4, hipMemcpyHostToDevice, ctx->stream));
  TBK_HIP(hipMemcpyAsync(b, U.beg, (size_t)U.n * 8, hipMemcpyHostToDevice, ctx->stream));
  TBK_HIP(hipMemcpyAsync(e, U.end, (size_t)U.n * 8, hipMemcpyHostToDevice, ctx->stream));
  T->n = U.n, T->tid = t, T->beg = b, T->end = e;
  return 0;
}

// the opening of tbk_region_view and tbk_tile_region: keep / kcig of the tile's n records against U and their exclusive scans koff / coff,
// n + 1 elements each in the workspace (the last ones are the totals; the caller reads them with whatever else it scans)
struct Kept {
  uint32_t *keep, *kcig, *koff, *coff;
};
int flag_and_scan(tbk_ctx* ctx, const tbk_regions& U, uint32_t n, const int32_t* tid, const int32_t* pos, const uint32_t* cig_off, const uint32_t* cig, Kept* K) {
  K->keep = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  K->kcig = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  K->koff = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  K->coff = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  if (!K->keep || !K->kcig || !K->koff || !K->coff) return TBK_ENOMEM;
  RegTab T;
  TBK_TRY(tab_upload(ctx, U, &T));
  TBK_LAUNCH(ctx, "regions_flag", rs_flag_k, cdiv((uint64_t)n + 1, RG_NT), RG_NT, 0, n, tid, pos, cig_off, cig, T, K->keep, K->kcig);
  TBK_TRY(tbk_exscan_u32(ctx, K->keep, K->koff, n + 1, nullptr));
  TBK_TRY(tbk_exscan_u32(ctx, K->kcig, K->coff, n + 1, nullptr));
  return 0;
}

// interval rows against the table: *m output rows, row i from source row first[r] + (i - off[r]) of the interval r that off places it in
int clip_mrange(tbk_ctx* ctx, const RegTab& T, uint32_t n, const int32_t* d_tid, const int32_t* d_start, const int32_t* d_end, uint32_t** first, uint32_t** off,
                uint64_t* m) {
  const uint32_t R = T.n;
  uint32_t* count = ws_alloc<uint32_t>(ctx, (size_t)R + 1);
  uint32_t* bad = ws_alloc<uint32_t>(ctx, 1);
  *first = ws_alloc<uint32_t>(ctx, R);
  *off = ws_alloc<uint32_t>(ctx, (size_t)R + 1);
  if (!count || !bad || !*first || !*off) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(bad, 0, 4, ctx->stream));
  TBK_LAUNCH(ctx, "clip_order", clip_order_k, cdiv(n, RG_NT), RG_NT, 0, n, d_tid, d_start, d_end, bad);
  TBK_LAUNCH(ctx, "clip_mrange", clip_mrange_k, cdiv((uint64_t)R + 1, RG_NT), RG_NT, 0, T, n, d_tid, d_start, d_end, *first, count);
  uint32_t res[2] = {0, 0};
  // (a sum of counts beyond n + R - 1 needs rows that overlap or lie out of order, and those are refused here first)
  TBK_HIP(hipMemcpyAsync(&res[0], bad, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  if (res[0]) {
    ctx->last_error = "clip: interval rows are not sorted by reference and start, or overlap";
    return TBK_EINVAL;
  }
  TBK_TRY(tbk_exscan_u32(ctx, count, *off, R + 1, nullptr));
  TBK_HIP(hipMemcpyAsync(&res[1], *off + R, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  *m = res[1];
  if (*m > (uint64_t)n + R - 1) return TBK_EHIP;
  return 0;
}

// The interval rows of a clip, n >= 1 of them in the caller's arrays (mem HOST or DEVICE; cap elements each), cut to the table in place:
// *n_rows becomes the count that comes out.  When that exceeds cap nothing is written, *n_rows is the count needed and the call is
// TBK_E2BIG.  a and b are the payload columns (b NULL: the rows have one).
template <class A, class B>
int clip_intervals(tbk_ctx* ctx, const RegTab& T, int mem, uint32_t n, uint32_t cap, uint32_t* n_rows, int32_t* tid, int32_t* start, int32_t* end, A* a, B* b) {
  const int32_t *d_tid, *d_start, *d_end;
  const A* d_a;
  const B* d_b = nullptr;
  TBK_TRY(rows_in(ctx, mem, tid, n, &d_tid));
  TBK_TRY(rows_in(ctx, mem, start, n, &d_start));
  TBK_TRY(rows_in(ctx, mem, end, n, &d_end));
  TBK_TRY(rows_in(ctx, mem, a, n, &d_a));
  if (b) TBK_TRY(rows_in(ctx, mem, b, n, &d_b));
  uint32_t *first = nullptr, *off = nullptr;
  uint64_t m = 0;
  TBK_TRY(clip_mrange(ctx, T, n, d_tid, d_start, d_end, &first, &off, &m));
  *n_rows = (uint32_t)m;
  if (m > cap) return TBK_E2BIG;  // the rows grew beyond the caller's arrays
  if (!m) return 0;
  int32_t *s_tid = ws_alloc<int32_t>(ctx, m), *s_start = ws_alloc<int32_t>(ctx, m), *s_end = ws_alloc<int32_t>(ctx, m);
  A* s_a = ws_alloc<A>(ctx, m);
  B* s_b = b ? ws_alloc<B>(ctx, m) : nullptr;
  if (!s_tid || !s_start || !s_end || !s_a || (b && !s_b)) return TBK_ENOMEM;
  TBK_LAUNCH(ctx, "clip_rows", (clip_rows_k<A, B>), cdiv(m, RG_NT), RG_NT, 0, (uint32_t)m, T, off, first, d_tid, d_start, d_end, d_a, d_b, s_tid, s_start, s_end, s_a,
             s_b);
  TBK_TRY(rows_out(ctx, mem, tid, s_tid, m));
  TBK_TRY(rows_out(ctx, mem, start, s_start, m));
  TBK_TRY(rows_out(ctx, mem, end, s_end, m));
  TBK_TRY(rows_out(ctx, mem, a, s_a, m));
  if (b) TBK_TRY(rows_out(ctx, mem, b, s_b, m));
  return 0;
}

int region_view_impl(tbk_ctx* ctx, const tbk_soa_in* tile, const uint8_t* tag_seen, const tbk_regions& U, tbk_cov_in* view, uint32_t* n_kept) {
  if (!ctx || !tile || !view || !n_kept || tile->mem != TBK_MEM_DEVICE) return TBK_EINVAL;
  const uint32_t n = tile->n_records;
  if (n && (!tile->tid || !tile->pos || !tile->flag || !tile->strand || !tile->cig_off || (tile->n_cigar_ops && !tile->cig))) return TBK_EINVAL;
  if (n == UINT32_MAX) return TBK_E2BIG;
  TBK_HIP(hipSetDevice(ctx->device));
  memset(view, 0, sizeof(*view));
  view->mem = TBK_MEM_DEVICE;
  *n_kept = 0;
  ctx->view_prep.valid = false;  // (the context's view is about to change)
  if (n == 0) return 0;
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  TBK_TRY(tbk_ws_reserve(ctx, ((size_t)n + 1) * 16 + tab_bytes(U) + ((size_t)1 << 20)));
  Kept K;
  TBK_TRY(flag_and_scan(ctx, U, n, tile->tid, tile->pos, tile->cig_off, tile->cig, &K));
  uint32_t tot[2] = {0, 0};
  TBK_HIP(hipMemcpyAsync(&tot[0], K.koff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&tot[1], K.coff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  const size_t nk = tot[0], nc = tot[1];  // (nc < 2^32: a subset of the tile's CIGAR words, whose count is a uint32)
  if (nk == 0) return tbk_check_launch(ctx, "region_view");
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t need = al(nk * 4) * 2 + al(nk * 2) + al(nk) + al(nk * 8) * 2 + al((nk + 1) * 4) + al(nc * 4 + 4);
  if (need > ctx->d_view_cap) {
    if (ctx->d_view) (void)hipFree(ctx->d_view);
    ctx->d_view = nullptr;
    ctx->d_view_cap = 0;
    const size_t cap = need + need / 4;
    TBK_HIP(hipMalloc((void**)&ctx->d_view, cap));
    ctx->d_view_cap = cap;
  }
  char* p = ctx->d_view;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += al(bytes);
    return r;
  };
  RvOut O;
  O.tid = (int32_t*)take(nk * 4);
  O.pos = (int32_t*)take(nk * 4);
  O.flag = (uint16_t*)take(nk * 2);
  O.strand = (uint8_t*)take(nk);
  O.yc = (double*)take(nk * 8);
  O.yx = (int64_t*)take(nk * 8);
  O.cig_off = (uint32_t*)take((nk + 1) * 4);
  O.cig = (uint32_t*)take(nc * 4 + 4);
  TBK_LAUNCH(ctx, "region_scatter", rv_scatter_k, cdiv((uint64_t)n + 1, RG_NT), RG_NT, 0, n, K.keep, K.koff, K.coff, tile->tid, tile->pos, tile->flag, tile->strand,
             tile->cig_off, tile->cig, tile->yc_in, tile->yx_in, tag_seen, O);
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "region_view"));
  view->n_records = (uint32_t)nk;
  view->n_cigar_ops = (uint32_t)nc;
  view->tid = O.tid;
  view->pos = O.pos;
  view->flag = O.flag;
  view->cig_off = O.cig_off;
  view->cig = O.cig;
  view->yc = O.yc;
  view->strand = O.strand;
  view->yx = O.yx;
  *n_kept = (uint32_t)nk;
  return 0;
}

int cov_clip_impl(tbk_ctx* ctx, tbk_cov_out* rows, const tbk_regions& U) {
  if (!ctx || !rows || (rows->mem != TBK_MEM_HOST && rows->mem != TBK_MEM_DEVICE)) return TBK_EINVAL;
  const uint32_t ni = rows->cap_intervals ? rows->n_intervals : 0, nj = rows->cap_junctions ? rows->n_junctions : 0;
  if (ni > rows->cap_intervals || nj > rows->cap_junctions || ni == UINT32_MAX || nj == UINT32_MAX) return TBK_EINVAL;
  if (ni && (!rows->iv_tid || !rows->iv_start || !rows->iv_end || !rows->iv_val)) return TBK_EINVAL;
  if (nj && (!rows->j_tid || !rows->j_start || !rows->j_end || !rows->j_strand || !rows->j_val)) return TBK_EINVAL;
  if (!ni && !nj) return 0;
  const size_t R = U.n;
  if ((uint64_t)ni + R - 1 >= UINT32_MAX) return TBK_E2BIG;  // (the most rows that can come out)
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  const int mem = rows->mem;
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)ni * 48 + (ni ? R * 24 : 0) + tab_bytes(U) + (size_t)nj * 64 + ((size_t)1 << 20)));
  RegTab T;
  TBK_TRY(tab_upload(ctx, U, &T));
  // (on TBK_E2BIG no row is touched, junction rows included, and the count needed is left in n_intervals)
  if (ni) TBK_TRY(clip_intervals(ctx, T, mem, ni, rows->cap_intervals, &rows->n_intervals, rows->iv_tid, rows->iv_start, rows->iv_end, rows->iv_val, (float*)nullptr));
  if (nj) {
    const int32_t *d_tid, *d_start, *d_end;
    const uint8_t* d_strand;
    const double* d_val;
    TBK_TRY(rows_in(ctx, mem, rows->j_tid, nj, &d_tid));
    TBK_TRY(rows_in(ctx, mem, rows->j_start, nj, &d_start));
    TBK_TRY(rows_in(ctx, mem, rows->j_end, nj, &d_end));
    TBK_TRY(rows_in(ctx, mem, rows->j_strand, nj, &d_strand));
    TBK_TRY(rows_in(ctx, mem, rows->j_val, nj, &d_val));
    uint32_t* keep = ws_alloc<uint32_t>(ctx, (size_t)nj + 1);
    uint32_t* koff = ws_alloc<uint32_t>(ctx, (size_t)nj + 1);
    int32_t *s_tid = ws_alloc<int32_t>(ctx, nj), *s_start = ws_alloc<int32_t>(ctx, nj), *s_end = ws_alloc<int32_t>(ctx, nj);
    uint8_t* s_strand = ws_alloc<uint8_t>(ctx, nj);
    double* s_val = ws_alloc<double>(ctx, nj);
    if (!keep || !koff || !s_tid || !s_start || !s_end || !s_strand || !s_val) return TBK_ENOMEM;
    TBK_LAUNCH(ctx, "clip_mjunc", clip_mjflag_k, cdiv((uint64_t)nj + 1, RG_NT), RG_NT, 0, nj, d_tid, d_start, d_end, T, keep);
    TBK_TRY(tbk_exscan_u32(ctx, keep, koff, nj + 1, nullptr));
    TBK_LAUNCH(ctx, "clip_junc", clip_jscat_k, cdiv(nj, RG_NT), RG_NT, 0, nj, keep, koff, d_tid, d_start, d_end, d_strand, d_val, s_tid, s_start, s_end, s_strand,
               s_val);
    uint32_t m = 0;
    TBK_HIP(hipMemcpyAsync(&m, koff + nj, 4, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    if (m > nj) return TBK_EHIP;
    TBK_TRY(rows_out(ctx, mem, rows->j_tid, s_tid, m));
    TBK_TRY(rows_out(ctx, mem, rows->j_start, s_start, m));
    TBK_TRY(rows_out(ctx, mem, rows->j_end, s_end, m));
    TBK_TRY(rows_out(ctx, mem, rows->j_strand, s_strand, m));
    TBK_TRY(rows_out(ctx, mem, rows->j_val, s_val, m));
    rows->n_junctions = m;
  }
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return tbk_check_launch(ctx, "cov_clip");
}

int sample_clip_impl(tbk_ctx* ctx, tbk_sample_out* rows, const tbk_regions& U) {
  if (!ctx || !rows || (rows->mem != TBK_MEM_HOST && rows->mem != TBK_MEM_DEVICE)) return TBK_EINVAL;
  const uint32_t ni = rows->n_intervals;
  if (ni > rows->cap_intervals || ni == UINT32_MAX) return TBK_EINVAL;
  if (ni && (!rows->iv_tid || !rows->iv_start || !rows->iv_end || !rows->iv_count || !rows->iv_heat)) return TBK_EINVAL;
  if (!ni) return 0;
  const size_t R = U.n;
  if ((uint64_t)ni + R - 1 >= UINT32_MAX) return TBK_E2BIG;  // (as in cov_clip_impl)
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)ni * 56 + R * 24 + tab_bytes(U) + ((size_t)1 << 20)));
  RegTab T;
  TBK_TRY(tab_upload(ctx, U, &T));
  TBK_TRY(clip_intervals(ctx, T, rows->mem, ni, rows->cap_intervals, &rows->n_intervals, rows->iv_tid, rows->iv_start, rows->iv_end, rows->iv_count, rows->iv_heat));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return tbk_check_launch(ctx, "sample_clip");
}

}  // namespace

// The one-region entries: the table of the one interval [beg, end) on tid, on the stack.
extern "C" int tbk_region_view(tbk_ctx* ctx, const tbk_soa_in* tile, const uint8_t* tag_seen, int32_t tid, int64_t beg, int64_t end, tbk_cov_in* view,
                               uint32_t* n_kept) {
  if (!region_ok(tid, beg, end)) return TBK_EINVAL;
  return region_view_impl(ctx, tile, tag_seen, tbk_regions{1, &tid, &beg, &end}, view, n_kept);
}
extern "C" int tbk_cov_clip(tbk_ctx* ctx, tbk_cov_out* rows, int32_t tid, int64_t beg, int64_t end) {
  if (!region_ok(tid, beg, end)) return TBK_EINVAL;
  return cov_clip_impl(ctx, rows, tbk_regions{1, &tid, &beg, &end});
}
extern "C" int tbk_sample_clip(tbk_ctx* ctx, tbk_sample_out* rows, int32_t tid, int64_t beg, int64_t end) {
  if (!region_ok(tid, beg, end)) return TBK_EINVAL;
  return sample_clip_impl(ctx, rows, tbk_regions{1, &tid, &beg, &end});
}
// ---- the same for a caller's table ----
extern "C" int tbk_regions_view(tbk_ctx* ctx, const tbk_soa_in* tile, const uint8_t* tag_seen, const tbk_regions* regions, tbk_cov_in* view, uint32_t* n_kept) {
  if (!regions_ok(regions)) return TBK_EINVAL;
  return region_view_impl(ctx, tile, tag_seen, *regions, view, n_kept);
}
extern "C" int tbk_cov_clip_regions(tbk_ctx* ctx, tbk_cov_out* rows, const tbk_regions* regions) {
  if (!regions_ok(regions)) return TBK_EINVAL;
  return cov_clip_impl(ctx, rows, *regions);
}
extern "C" int tbk_sample_clip_regions(tbk_ctx* ctx, tbk_sample_out* rows, const tbk_regions* regions) {
  if (!regions_ok(regions)) return TBK_EINVAL;
  return sample_clip_impl(ctx, rows, *regions);
}

// ---- tbk_tile_region: the region's records of a decoded tile as a collapse tile -------------------------------------------
// The flags, the kept CIGAR counts and their scans are tbk_region_view's (flag_and_scan); what a collapse tile carries beyond tiecov's view —
// nh, mapq, yd_in, the MD and QNAME CSRs, qname_hash, the record-offset table behind tbk_bam_records and the encoders — moves in the same
// scatter pass.  (rv_scatter_k and rt_scatter_k stay two kernels: they carry different columns.)
//   rs_flag_k       keep / kcig as above
//   rt_lens_k       kmd[i] / kqn[i] = the kept record's MD / QNAME byte counts (only with those columns)
//   up to four exclusive scans (tbk_exscan_u32), n + 1 elements each
//   rt_scatter_k    a thread per record: the columns, the three CSR payloads and the record offset, file order kept
//   rt_fileoff_k    file_off_out[f] = the keep scan read at the old file_off[f]
namespace {

struct RtCols {
  int32_t *tid, *pos, *nh;
  uint16_t* flag;
  uint8_t *mapq, *strand;
  uint32_t *cig_off, *cig;
  double* yc;
  int64_t *yx, *yd;
  uint32_t* md_off;
  uint8_t *md, *md_has;
  uint64_t* qh;
  uint32_t* qn_off;
  uint8_t* qn;
  uint64_t* rec;
};

__global__ __launch_bounds__(RG_NT) void rt_lens_k(uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ md_off,
                                                   const uint32_t* __restrict__ qn_off, uint32_t* __restrict__ kmd /* [n + 1] or NULL */,
                                                   uint32_t* __restrict__ kqn /* [n + 1] or NULL */) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i > n) return;
  const bool k = i < n && keep[i];
  if (kmd) kmd[i] = k ? md_off[i + 1] - md_off[i] : 0u;
  if (kqn) kqn[i] = k ? qn_off[i + 1] - qn_off[i] : 0u;
}

__global__ __launch_bounds__(RG_NT) void rt_scatter_k(uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ koff /* [n + 1] */,
                                                      const uint32_t* __restrict__ coff, const uint32_t* __restrict__ moff, const uint32_t* __restrict__ qoff,
                                                      RtCols I, RtCols O) {
  const uint64_t i = (uint64_t)blockIdx.x * RG_NT + threadIdx.x;
  if (i > n) return;
  if (i == n) {  // the CSRs' closing offsets
    const uint32_t o = koff[n];
    O.cig_off[o] = coff[n];
    if (I.md_off) O.md_off[o] = moff[n];
    if (I.qn_off) O.qn_off[o] = qoff[n];
    return;
  }
  if (!keep[i]) return;
  const uint32_t o = koff[i];
  O.tid[o] = I.tid[i];
  O.pos[o] = I.pos[i];
  O.nh[o] = I.nh[i];
  O.flag[o] = I.flag[i];
  O.mapq[o] = I.mapq[i];
  O.strand[o] = I.strand[i];
  O.rec[o] = I.rec[i];
  if (I.yc) {
    O.yc[o] = I.yc[i];
    O.yx[o] = I.yx[i];
    O.yd[o] = I.yd[i];
  }
  {
    const uint32_t d = coff[i], c0 = I.cig_off[i], nc = I.cig_off[i + 1] - c0;
    O.cig_off[o] = d;
    for (uint32_t q = 0; q < nc; ++q) O.cig[d + q] = I.cig[c0 + q];
  }
  if (I.md_off) {
    const uint32_t d = moff[i], m0 = I.md_off[i], nm = I.md_off[i + 1] - m0;
    O.md_off[o] = d;
    O.md_has[o] = I.md_has[i];
    for (uint32_t q = 0; q < nm; ++q) O.md[d + q] = I.md[m0 + q];
  }
  if (I.qn_off) {
    const uint32_t d = qoff[i], q0 = I.qn_off[i], nq = I.qn_off[i + 1] - q0;
    O.qn_off[o] = d;
    O.qh[o] = I.qh[i];
    for (uint32_t q = 0; q < nq; ++q) O.qn[d + q] = I.qn[q0 + q];
  }
}

__global__ void rt_fileoff_k(uint32_t k1, const uint32_t* __restrict__ file_off, const uint32_t* __restrict__ koff, uint32_t* __restrict__ out) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < k1) out[f] = koff[file_off[f]];
}

template <class T>
T* rt_alloc(tbk_ctx* ctx, size_t n) {
  return (T*)tbk_bam_dev_alloc(ctx, (n ? n : 1) * sizeof(T));
}

int tile_region_impl(tbk_ctx* ctx, const tbk_soa_in* tile, const tbk_regions& U, tbk_soa_in* out, uint32_t* file_off_out, uint32_t* n_kept) {
  if (!ctx || !tile || !out || !file_off_out || !n_kept || tile->mem != TBK_MEM_DEVICE) return TBK_EINVAL;
  const uint32_t n = tile->n_records, k = tile->n_files;
  if (k == 0 || !tile->file_off || tile->prio_hi || tile->prio_lo) return TBK_EINVAL;
  if (tile->file_off[0] != 0 || tile->file_off[k] != n) return TBK_EINVAL;
  for (uint32_t f = 0; f < k; ++f)
    if (tile->file_off[f + 1] < tile->file_off[f]) return TBK_EINVAL;
  if (n == UINT32_MAX) return TBK_E2BIG;
  const bool has_y = tile->yc_in != nullptr, has_md = tile->md_off != nullptr, has_qn = tile->qname_off != nullptr;
  if (n) {
    if (!tbk_bam_dev_is_tile(ctx, tile)) {
      ctx->last_error = "tile_region: not the tile the last decode on this context returned";
      return TBK_EINVAL;
    }
    if (!tile->tid || !tile->pos || !tile->flag || !tile->mapq || !tile->strand || !tile->nh || !tile->cig_off || (tile->n_cigar_ops && !tile->cig) ||
        (has_y && (!tile->yx_in || !tile->yd_in)) || (has_md && !tile->md_has) || (has_qn && !tile->qname_hash))
      return TBK_EINVAL;
  }
  TBK_HIP(hipSetDevice(ctx->device));
  TBK_TRY(tbk_collapse_finish_yd(ctx));  // (a deferred YD stage may still read the tile)
  const tbk_soa_in in = *tile;           // (out may be the caller's input struct, file_off_out its file_off)
  const std::vector<uint32_t> fo_in(tile->file_off, tile->file_off + (size_t)k + 1);
  memset(out, 0, sizeof(*out));
  out->mem = TBK_MEM_DEVICE;
  out->n_files = k;
  out->file_off = file_off_out;
  out->tbmerged = in.tbmerged;
  for (uint32_t f = 0; f <= k; ++f) file_off_out[f] = 0;
  *n_kept = 0;
  ctx->view_prep.valid = false;
  if (n == 0) return 0;
  const uint8_t* d_inf = nullptr;
  const uint64_t* d_rec = nullptr;
  uint32_t n_rec = 0;
  if (!tbk_bam_dev_records(ctx, &d_inf, &d_rec, &n_rec) || n_rec != n) return TBK_EINVAL;
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  TBK_TRY(tbk_ws_reserve(ctx, ((size_t)n + 1) * 32 + ((size_t)k + 1) * 8 + tab_bytes(U) + ((size_t)1 << 20)));
  uint32_t *kmd = nullptr, *moff = nullptr, *kqn = nullptr, *qoff = nullptr;
  if (has_md) kmd = ws_alloc<uint32_t>(ctx, (size_t)n + 1), moff = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  if (has_qn) kqn = ws_alloc<uint32_t>(ctx, (size_t)n + 1), qoff = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint32_t* d_fo = ws_alloc<uint32_t>(ctx, (size_t)k + 1);
  uint32_t* d_fo_out = ws_alloc<uint32_t>(ctx, (size_t)k + 1);
  if ((has_md && (!kmd || !moff)) || (has_qn && (!kqn || !qoff)) || !d_fo || !d_fo_out) return TBK_ENOMEM;
  const uint32_t grid = cdiv((uint64_t)n + 1, RG_NT);
  TBK_HIP(hipMemcpyAsync(d_fo, fo_in.data(), ((size_t)k + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  Kept K;
  TBK_TRY(flag_and_scan(ctx, U, n, in.tid, in.pos, in.cig_off, in.cig, &K));
  const uint32_t *keep = K.keep, *koff = K.koff, *coff = K.coff;
  if (has_md || has_qn) {
    TBK_LAUNCH(ctx, "tile_region_lens", rt_lens_k, grid, RG_NT, 0, n, keep, in.md_off, in.qname_off, kmd, kqn);
    if (has_md) TBK_TRY(tbk_exscan_u32(ctx, kmd, moff, n + 1, nullptr));
    if (has_qn) TBK_TRY(tbk_exscan_u32(ctx, kqn, qoff, n + 1, nullptr));
  }
  uint32_t tot[4] = {0, 0, 0, 0};
  TBK_HIP(hipMemcpyAsync(&tot[0], koff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&tot[1], coff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (has_md) TBK_HIP(hipMemcpyAsync(&tot[2], moff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (has_qn) TBK_HIP(hipMemcpyAsync(&tot[3], qoff + n, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "tile_region"));
  const size_t nk = tot[0], nc = tot[1], nm = tot[2], nq = tot[3];  // (subsets of the tile's counts, which are uint32)
  if (nk > n || nc > in.n_cigar_ops) return TBK_EHIP;
  RtCols I{}, O{};
  I.tid = const_cast<int32_t*>(in.tid), I.pos = const_cast<int32_t*>(in.pos), I.nh = const_cast<int32_t*>(in.nh);
  I.flag = const_cast<uint16_t*>(in.flag), I.mapq = const_cast<uint8_t*>(in.mapq), I.strand = const_cast<uint8_t*>(in.strand);
  I.cig_off = const_cast<uint32_t*>(in.cig_off), I.cig = const_cast<uint32_t*>(in.cig);
  I.yc = const_cast<double*>(in.yc_in), I.yx = const_cast<int64_t*>(in.yx_in), I.yd = const_cast<int64_t*>(in.yd_in);
  I.md_off = const_cast<uint32_t*>(in.md_off), I.md = const_cast<uint8_t*>(in.md), I.md_has = const_cast<uint8_t*>(in.md_has);
  I.qh = const_cast<uint64_t*>(in.qname_hash), I.qn_off = const_cast<uint32_t*>(in.qname_off), I.qn = const_cast<uint8_t*>(in.qname);
  I.rec = const_cast<uint64_t*>(d_rec);
  O.tid = rt_alloc<int32_t>(ctx, nk), O.pos = rt_alloc<int32_t>(ctx, nk), O.nh = rt_alloc<int32_t>(ctx, nk);
  O.flag = rt_alloc<uint16_t>(ctx, nk), O.mapq = rt_alloc<uint8_t>(ctx, nk), O.strand = rt_alloc<uint8_t>(ctx, nk);
  O.cig_off = rt_alloc<uint32_t>(ctx, nk + 1), O.cig = rt_alloc<uint32_t>(ctx, nc);
  O.rec = rt_alloc<uint64_t>(ctx, nk);
  bool ok = O.tid && O.pos && O.nh && O.flag && O.mapq && O.strand && O.cig_off && O.cig && O.rec;
  if (has_y) {
    O.yc = rt_alloc<double>(ctx, nk), O.yx = rt_alloc<int64_t>(ctx, nk), O.yd = rt_alloc<int64_t>(ctx, nk);
    ok = ok && O.yc && O.yx && O.yd;
  }
  if (has_md) {
    O.md_off = rt_alloc<uint32_t>(ctx, nk + 1), O.md = rt_alloc<uint8_t>(ctx, nm), O.md_has = rt_alloc<uint8_t>(ctx, nk);
    ok = ok && O.md_off && O.md && O.md_has;
  }
  if (has_qn) {
    O.qn_off = rt_alloc<uint32_t>(ctx, nk + 1), O.qn = rt_alloc<uint8_t>(ctx, nq), O.qh = rt_alloc<uint64_t>(ctx, nk);
    ok = ok && O.qn_off && O.qn && O.qh;
  }
  if (!ok) {
    (void)hipGetLastError();
    return TBK_ENOMEM;
  }
  TBK_LAUNCH(ctx, "tile_region_scatter", rt_scatter_k, grid, RG_NT, 0, n, keep, koff, coff, moff, qoff, I, O);
  TBK_LAUNCH(ctx, "tile_region_fileoff", rt_fileoff_k, cdiv((uint64_t)k + 1, 256), 256, 0, k + 1, d_fo, koff, d_fo_out);
  TBK_HIP(hipMemcpyAsync(file_off_out, d_fo_out, ((size_t)k + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "tile_region"));
  tbk_bam_dev_compacted(ctx, O.rec, (uint32_t)nk, O.tid);
  out->n_records = (uint32_t)nk;
  out->n_cigar_ops = (uint32_t)nc;
  out->tid = O.tid, out->pos = O.pos, out->flag = O.flag, out->mapq = O.mapq, out->strand = O.strand, out->nh = O.nh;
  out->cig_off = O.cig_off, out->cig = O.cig;
  out->yc_in = O.yc, out->yx_in = O.yx, out->yd_in = O.yd;
  out->md_off = O.md_off, out->md = O.md, out->md_has = O.md_has;
  out->qname_hash = O.qh, out->qname_off = O.qn_off, out->qname = O.qn;
  *n_kept = (uint32_t)nk;
  return 0;
}

}  // namespace

extern "C" int tbk_tile_region(tbk_ctx* ctx, const tbk_soa_in* tile, int32_t tid, int64_t beg, int64_t end, tbk_soa_in* out, uint32_t* file_off_out,
                               uint32_t* n_kept) {
  if (!region_ok(tid, beg, end)) return TBK_EINVAL;
  return tile_region_impl(ctx, tile, tbk_regions{1, &tid, &beg, &end}, out, file_off_out, n_kept);
}
extern "C" int tbk_tile_regions(tbk_ctx* ctx, const tbk_soa_in* tile, const tbk_regions* regions, tbk_soa_in* out, uint32_t* file_off_out, uint32_t* n_kept) {
  if (!regions_ok(regions)) return TBK_EINVAL;
  return tile_region_impl(ctx, tile, *regions, out, file_off_out, n_kept);
}
