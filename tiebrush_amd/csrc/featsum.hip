// featsum.hip — tbk_cov_summary: the rows of a coverage call read against a list of features, what
// `tiecov --features BED --summary OUT` / `tiebrush --features BED --summary OUT` run.  Per feature [beg, end) on tid: the bases under a
// coverage row (covered), the sum of value x bases over them (sum), the largest row value (max) and the summed value of the junction rows
// that ARE the feature (junc: same tid, start and end, and the feature's strand; '.' takes every strand).
//
// The reference has no such option; the contract is stated against the rows themselves (include/tbk.h).  Interval rows are sorted by
// (tid, start) and disjoint, so the rows a feature meets are ONE run [lo, hi), found by two searches; only the run's first and last row can
// reach beyond the feature.  Junction rows are sorted by (tid, start, end, strand): the feature's rows are found by one search.
//   fs_order_k   *bad |= 1 for interval rows that are not sorted and disjoint, |= 2 for junction rows out of order (read back: TBK_EINVAL)
//   fs_tile_k    one wave per tile of FS_TILE interval rows: the tile's sum of val x len, its bases and its largest value, each lane its
//                rows in order and then a butterfly over the lanes — an order that depends on the tile alone
//   fs_feat_k    one wave per feature.  The searches are 64-ary: every lane probes one row and a ballot names the step, so a search over
//                2^24 rows is four rounds of one load each.  A run of up to FS_DIRECT rows is walked lane-strided, every row cut to the
//                feature.  A longer run: the rows up to the first tile boundary behind lo, the aggregates of the whole tiles, the rows of
//                the last tile, again lane-strided — a feature over a whole chromosome reads its tiles' aggregates, not its rows.  Lane 0
//                then adds the junction rows of the feature in row order.
// No floating-point atomics and no differences of prefix sums: a feature's sum is made of additions of its own rows' products alone, in an
// order fixed by (lo, hi), so two calls on the same inputs give the same bits; where every product and partial sum is representable (YC
// integral, the default) any order gives the same bits as well.
#include "dev_common.hpp"
#include "tbk_internal.h"

namespace {

constexpr int FS_NT = 256;             // threads of a block: four waves, a tile or a feature each
constexpr uint32_t FS_TILE = 256;      // interval rows per aggregate
constexpr uint32_t FS_DIRECT = 256;    // the longest run that is walked row by row

struct FsRows {
  uint32_t ni, nj;
  const int32_t *tid, *start, *end;
  const double* val;
  const int32_t *jtid, *jstart, *jend;
  const uint8_t* jstrand;
  const double* jval;
};
struct FsFeat {
  uint32_t n;
  const int32_t* tid;
  const int64_t *beg, *end;
  const uint8_t* strand;  // NULL: every feature is '.'
};
struct FsAgg {
  double *sum, *max;
  uint64_t* len;
};
struct FsOut {
  uint64_t* covered;
  double *sum, *max, *junc;
};

__global__ __launch_bounds__(FS_NT) void fs_order_k(FsRows R, uint32_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * FS_NT + threadIdx.x;
  if (i < R.ni) {
    const int32_t t = R.tid[i], e = R.end[i];
    if (e < R.start[i] || (i + 1 < R.ni && (R.tid[i + 1] < t || (R.tid[i + 1] == t && R.start[i + 1] < e)))) atomicOr(bad, 1u);
  }
  if (i + 1 < R.nj) {
    const int32_t t = R.jtid[i], t2 = R.jtid[i + 1], s = R.jstart[i], s2 = R.jstart[i + 1], e = R.jend[i], e2 = R.jend[i + 1];
    const bool ok = t2 > t || (t2 == t && (s2 > s || (s2 == s && (e2 > e || (e2 == e && R.jstrand[i + 1] >= R.jstrand[i])))));
    if (!ok) atomicOr(bad, 2u);
  }
}

// the lanes' partial (sum, bases, max) folded into every lane: a fixed butterfly
__device__ __forceinline__ void fs_fold(double& s, uint64_t& c, double& m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s += __shfl_xor(s, d, 64);
    c += __shfl_xor(c, d, 64);
    const double o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
}

__global__ __launch_bounds__(FS_NT) void fs_tile_k(FsRows R, uint32_t n_tiles, FsAgg A) {
  const uint32_t t = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;  // (a whole wave leaves: the shuffles below run in full waves)
  const uint64_t r0 = (uint64_t)t * FS_TILE, r1 = r0 + FS_TILE < R.ni ? r0 + FS_TILE : R.ni;
  double s = 0.0, m = -__builtin_inf();
  uint64_t c = 0;
  for (uint64_t i = r0 + lane_id(); i < r1; i += WAVE) {
    const int64_t len = (int64_t)R.end[i] - (int64_t)R.start[i];
    const double v = R.val[i];
    s += v * (double)len;
    c += (uint64_t)len;
    m = v > m ? v : m;
  }
  fs_fold(s, c, m);
  if (lane_id() == 0) A.sum[t] = s, A.len[t] = c, A.max[t] = m;
}

// The first index in [lo, n) at which the monotone predicate holds (n: nowhere), found by the whole wave: up to 64 probes a round.
// Invariant: the answer lies in [lo, hi], and hi == n or pred(hi) is known.  Every probe is an index below n.
template <class P>
__device__ __forceinline__ uint32_t fs_search(uint32_t lo, uint32_t n, P pred) {
  uint32_t hi = n;
  const uint32_t lane = lane_id();
  while (hi - lo > WAVE) {
    const uint32_t step = (hi - lo + WAVE - 1) / WAVE;  // lane k probes the last index of the k-th stretch of `step`
    const uint64_t idx = (uint64_t)lo + (uint64_t)(lane + 1) * step - 1;
    const bool p = idx >= hi || pred((uint32_t)idx);
    const unsigned long long found = __ballot(p);
    if (!found) {  // (lane 63 probed hi - 1, the last index, and it fails too: the answer is hi)
      lo = hi;
      break;
    }
    const uint32_t k = (uint32_t)__builtin_ctzll(found);
    const uint64_t top = (uint64_t)lo + (uint64_t)(k + 1) * step - 1;
    lo += k * step;
    hi = top < hi ? (uint32_t)top : hi;
  }
  const uint32_t idx = lo + lane;
  const unsigned long long b = __ballot(idx < hi && pred(idx));
  return b ? lo + (uint32_t)__builtin_ctzll(b) : hi;
}

__global__ __launch_bounds__(FS_NT) void fs_feat_k(FsRows R, FsFeat F, FsAgg A, FsOut O) {
  const uint32_t f = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (f >= F.n) return;  // (whole waves, as above)
  const uint32_t lane = lane_id();
  const int32_t ft = F.tid[f];
  const int64_t fb = F.beg[f], fe = F.end[f];
  if (O.covered) {
    double s = 0.0, m = -__builtin_inf();
    uint64_t c = 0;
    if (R.ni) {
      // lo: the first row that ends behind the feature's begin on its reference (or lies on a later one); hi: the first one from there
      // that starts at or behind its end
      const uint32_t lo = fs_search(0, R.ni, [&](uint32_t i) { const int32_t t = R.tid[i]; return t > ft || (t == ft && (int64_t)R.end[i] > fb); });
      const uint32_t hi = fs_search(lo, R.ni, [&](uint32_t i) { const int32_t t = R.tid[i]; return t > ft || (t == ft && (int64_t)R.start[i] >= fe); });
      auto rows = [&](uint32_t a, uint32_t b) {  // rows [a, b) cut to the feature
        for (uint32_t i = a + lane; i < b; i += WAVE) {
          const int64_t rs = R.start[i], re = R.end[i];
          const int64_t len = (re < fe ? re : fe) - (rs > fb ? rs : fb);
          const double v = R.val[i];
          s += v * (double)len;
          c += (uint64_t)len;
          m = v > m ? v : m;
        }
      };
      if (hi - lo <= FS_DIRECT) {
        rows(lo, hi);
      } else {
        // whole tiles never hold the run's first or last row, the two that may reach beyond the feature
        const uint32_t t0 = lo / FS_TILE + 1, t1 = (hi - 1) / FS_TILE;
        rows(lo, t0 * FS_TILE);
        for (uint32_t t = t0 + lane; t < t1; t += WAVE) {
          s += A.sum[t];
          c += A.len[t];
          const double v = A.max[t];
          m = v > m ? v : m;
        }
        rows(t1 * FS_TILE, hi);
      }
      fs_fold(s, c, m);
    }
    if (lane == 0) O.covered[f] = c, O.sum[f] = s, O.max[f] = c ? m : 0.0;
  }
  if (O.junc) {
    double j = 0.0;
    if (R.nj) {
      uint32_t i = fs_search(0, R.nj, [&](uint32_t k) {
        const int32_t t = R.jtid[k];
        if (t != ft) return t > ft;
        const int64_t js = R.jstart[k];
        return js > fb || (js == fb && (int64_t)R.jend[k] >= fe);
      });
      const uint8_t want = F.strand ? F.strand[f] : (uint8_t)'.';
      if (lane == 0)
        for (; i < R.nj && R.jtid[i] == ft && (int64_t)R.jstart[i] == fb && (int64_t)R.jend[i] == fe; ++i)
          if (want == '.' || R.jstrand[i] == want) j += R.jval[i];
    }
    if (lane == 0) O.junc[f] = j;
  }
}

struct ProfEnd {
  tbk_ctx* c;
  ~ProfEnd() { tbk_prof_end_call(c); }
};

// an array of the caller (host or device) as a device pointer: a device array as it is, a host array through a copy into the arena
template <class T>
int fs_in(tbk_ctx* ctx, int mem, const T* p, size_t n, const T** d) {
  if (mem == TBK_MEM_DEVICE || !n) {
    *d = p;
    return 0;
  }
  T* a = ws_alloc<T>(ctx, n);
  if (!a) return TBK_ENOMEM;
  TBK_HIP(hipMemcpyAsync(a, p, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  *d = a;
  return 0;
}
// an output column: the caller's device array, or scratch that fs_back copies to the caller's host array
template <class T>
int fs_col(tbk_ctx* ctx, int mem, T* p, size_t n, T** d) {
  *d = mem == TBK_MEM_DEVICE ? p : ws_alloc<T>(ctx, n);
  return *d ? 0 : TBK_ENOMEM;
}
template <class T>
int fs_back(tbk_ctx* ctx, int mem, T* dst, const T* d, size_t n) {
  if (mem == TBK_MEM_HOST) TBK_HIP(hipMemcpyAsync(dst, d, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

}  // namespace

extern "C" int tbk_cov_summary(tbk_ctx* ctx, const tbk_cov_out* rows, const tbk_features* F, tbk_feat_out* out) {
  if (!ctx || !rows || !F || !out) return TBK_EINVAL;
  if ((rows->mem != TBK_MEM_HOST && rows->mem != TBK_MEM_DEVICE) || (out->mem != TBK_MEM_HOST && out->mem != TBK_MEM_DEVICE)) return TBK_EINVAL;
  const bool want_cov = rows->cap_intervals != 0, want_junc = rows->cap_junctions != 0;
  const uint32_t ni = want_cov ? rows->n_intervals : 0, nj = want_junc ? rows->n_junctions : 0;
  if (ni > rows->cap_intervals || nj > rows->cap_junctions || ni == UINT32_MAX || nj == UINT32_MAX) return TBK_EINVAL;
  if (ni && (!rows->iv_tid || !rows->iv_start || !rows->iv_end || !rows->iv_val)) return TBK_EINVAL;
  if (nj && (!rows->j_tid || !rows->j_start || !rows->j_end || !rows->j_strand || !rows->j_val)) return TBK_EINVAL;
  const uint32_t n = F->n;
  if (n == 0 || !F->tid || !F->beg || !F->end) return TBK_EINVAL;
  if (want_cov && (!out->covered || !out->sum || !out->max)) return TBK_EINVAL;
  if (want_junc && !out->junc) return TBK_EINVAL;
  for (uint32_t f = 0; f < n; ++f) {
    if (F->tid[f] < 0 || F->beg[f] < 0 || F->end[f] <= F->beg[f]) return TBK_EINVAL;
    if (F->strand && F->strand[f] != '+' && F->strand[f] != '-' && F->strand[f] != '.') return TBK_EINVAL;
  }
  if (!want_cov && !want_junc) return 0;
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  const uint32_t n_tiles = ni > FS_DIRECT ? cdiv(ni, FS_TILE) : 0;  // (no run is longer than FS_DIRECT rows otherwise)
  TBK_TRY(tbk_ws_reserve(ctx, (rows->mem == TBK_MEM_HOST ? (size_t)ni * 20 + (size_t)nj * 21 : 0) + (size_t)n * (21 + 32) + (size_t)n_tiles * 24 + ((size_t)1 << 20)));
  FsRows R{};
  R.ni = ni, R.nj = nj;
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_tid, ni, &R.tid));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_start, ni, &R.start));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_end, ni, &R.end));
  TBK_TRY(fs_in(ctx, rows->mem, (const double*)rows->iv_val, ni, &R.val));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->j_tid, nj, &R.jtid));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->j_start, nj, &R.jstart));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->j_end, nj, &R.jend));
  TBK_TRY(fs_in(ctx, rows->mem, (const uint8_t*)rows->j_strand, nj, &R.jstrand));
  TBK_TRY(fs_in(ctx, rows->mem, (const double*)rows->j_val, nj, &R.jval));
  if (ni || nj) {
    uint32_t* bad = ws_alloc<uint32_t>(ctx, 1);
    if (!bad) return TBK_ENOMEM;
    TBK_HIP(hipMemsetAsync(bad, 0, 4, ctx->stream));
    TBK_LAUNCH(ctx, "featsum_order", fs_order_k, cdiv(ni > nj ? ni : nj, FS_NT), FS_NT, 0, R, bad);
    uint32_t res = 0;
    TBK_HIP(hipMemcpyAsync(&res, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    if (res) {
      ctx->last_error = (res & 1u) ? "summary: interval rows are not sorted by reference and start, or overlap"
                                   : "summary: junction rows are not sorted by reference, start, end and strand";
      return TBK_EINVAL;
    }
  }
  FsFeat D{};
  D.n = n;
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->tid, n, &D.tid));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->beg, n, &D.beg));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->end, n, &D.end));
  if (F->strand) TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->strand, n, &D.strand));
  FsAgg A{};
  if (n_tiles) {
    A.sum = ws_alloc<double>(ctx, n_tiles), A.max = ws_alloc<double>(ctx, n_tiles), A.len = ws_alloc<uint64_t>(ctx, n_tiles);
    if (!A.sum || !A.max || !A.len) return TBK_ENOMEM;
    TBK_LAUNCH(ctx, "featsum_tiles", fs_tile_k, cdiv(n_tiles, FS_NT / WAVE), FS_NT, 0, R, n_tiles, A);
  }
  FsOut O{};
  if (want_cov) {
    TBK_TRY(fs_col(ctx, out->mem, out->covered, n, &O.covered));
    TBK_TRY(fs_col(ctx, out->mem, out->sum, n, &O.sum));
    TBK_TRY(fs_col(ctx, out->mem, out->max, n, &O.max));
  }
  if (want_junc) TBK_TRY(fs_col(ctx, out->mem, out->junc, n, &O.junc));
  TBK_LAUNCH(ctx, "featsum_features", fs_feat_k, cdiv(n, FS_NT / WAVE), FS_NT, 0, R, D, A, O);
  if (want_cov) {
    TBK_TRY(fs_back(ctx, out->mem, out->covered, O.covered, n));
    TBK_TRY(fs_back(ctx, out->mem, out->sum, O.sum, n));
    TBK_TRY(fs_back(ctx, out->mem, out->max, O.max, n));
  }
  if (want_junc) TBK_TRY(fs_back(ctx, out->mem, out->junc, O.junc, n));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return tbk_check_launch(ctx, "cov_summary");
}
