// depththr.hip — tbk_cov_thresholds: the rows of a coverage call read against features and up to 16 thresholds, what
// `--depth-summary OUT` and `--feature-depth OUT` of tiecov / tiebrush run.  Per feature [beg, end) on tid and threshold T: the bases of
// the feature under an interval row whose value is >= T (ge), and the bases under any row (covered).
//
// The rows a feature meets are one run [lo, hi), found as tbk_cov_summary finds it (featsum_common.hpp: the 64-ary searches, the tile
// constants); only the run's first and last row can reach beyond the feature.
//   dt_tile_k    one wave per tile of FS_TILE interval rows, run only when there are more than FS_DIRECT rows: per threshold the tile's
//                bases with val >= T, 16 uint64 per tile, tile-major
//   dt_feat_k    one wave per feature.  A run of up to FS_DIRECT rows is walked lane-strided, every row cut to the feature.  A longer
//                run: the rows up to the first tile boundary behind lo, the aggregates of the whole tiles, the rows of the last tile.
//                The lanes' counts are folded by a butterfly.
// The thresholds travel in the kernel arguments (DtThr: uniform scalar loads; the slots behind n_thr hold +inf, which no finite value
// reaches).  The sixteen counters are named registers (DT_EACH), updated by straight-line code: no array is indexed at run time.  The
// counts are 64-bit integers: no atomics, no floating-point accumulation, exact in any order.
#include "featsum_common.hpp"

#include <math.h>

namespace {

constexpr uint32_t DT_MAX = TBK_MAX_THRESHOLDS;  // the register budget: 16 counters of 64 bits are 32 VGPRs
static_assert(DT_MAX == 16, "DT_EACH names sixteen counters");

struct DtThr {
  double t[DT_MAX];
};
struct DtOut {
  uint32_t n_thr;
  uint64_t *covered, *ge;  // covered may be NULL; ge [n][n_thr]
};

#define DT_EACH(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

// the sixteen counters of a lane and the bases under any row
struct DtCnt {
#define DT_DECL(k) uint64_t c##k = 0;
  DT_EACH(DT_DECL)
#undef DT_DECL
  uint64_t all = 0;
  // `len` bases at value v
  __device__ __forceinline__ void row(const DtThr& P, double v, uint64_t len) {
#define DT_ROW(k) c##k += v >= P.t[k] ? len : 0;
    DT_EACH(DT_ROW)
#undef DT_ROW
    all += len;
  }
  // a whole tile's sixteen counts
  __device__ __forceinline__ void tile(const uint64_t* __restrict__ a) {
#define DT_TILE(k) c##k += a[k];
    DT_EACH(DT_TILE)
#undef DT_TILE
  }
  // the lanes' counts folded into every lane: a fixed butterfly
  __device__ __forceinline__ void fold() {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#define DT_FOLD(k) c##k += __shfl_xor(c##k, d, 64);
      DT_EACH(DT_FOLD)
#undef DT_FOLD
      all += __shfl_xor(all, d, 64);
    }
  }
  // the first n counts to o[0 .. n)
  __device__ __forceinline__ void store(uint64_t* __restrict__ o, uint32_t n) const {
#define DT_STORE(k) \
  if (k < n) o[k] = c##k;
    DT_EACH(DT_STORE)
#undef DT_STORE
  }
};

__global__ __launch_bounds__(FS_NT) void dt_tile_k(FsRows R, uint32_t n_tiles, DtThr P, uint64_t* __restrict__ agg, uint64_t* __restrict__ agg_all) {
  const uint32_t t = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;  // (a whole wave leaves: the shuffles below run in full waves)
  const uint64_t r0 = (uint64_t)t * FS_TILE, r1 = r0 + FS_TILE < R.ni ? r0 + FS_TILE : R.ni;
  DtCnt C;
  for (uint64_t i = r0 + lane_id(); i < r1; i += WAVE) C.row(P, R.val[i], (uint64_t)((int64_t)R.end[i] - (int64_t)R.start[i]));
  C.fold();
  if (lane_id() == 0) C.store(agg + (size_t)t * DT_MAX, DT_MAX), agg_all[t] = C.all;
}

__global__ __launch_bounds__(FS_NT) void dt_feat_k(FsRows R, FsFeat F, DtThr P, const uint64_t* __restrict__ agg, const uint64_t* __restrict__ agg_all, DtOut O) {
  const uint32_t f = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (f >= F.n) return;  // (whole waves, as above)
  const uint32_t lane = lane_id();
  const int32_t ft = F.tid[f];
  const int64_t fb = F.beg[f], fe = F.end[f];
  DtCnt C;
  if (R.ni) {
    // lo: the first row that ends behind the feature's begin on its reference (or lies on a later one); hi: the first one from there
    // that starts at or behind its end
    const uint32_t lo = fs_search(0, R.ni, [&](uint32_t i) { const int32_t t = R.tid[i]; return t > ft || (t == ft && (int64_t)R.end[i] > fb); });
    const uint32_t hi = fs_search(lo, R.ni, [&](uint32_t i) { const int32_t t = R.tid[i]; return t > ft || (t == ft && (int64_t)R.start[i] >= fe); });
    auto rows = [&](uint32_t a, uint32_t b) {  // rows [a, b) cut to the feature
      for (uint32_t i = a + lane; i < b; i += WAVE) {
        const int64_t rs = R.start[i], re = R.end[i];
        C.row(P, R.val[i], (uint64_t)((re < fe ? re : fe) - (rs > fb ? rs : fb)));
      }
    };
    if (hi - lo <= FS_DIRECT) {
      rows(lo, hi);
    } else {
      // whole tiles never hold the run's first or last row, the two that may reach beyond the feature (n_tiles > t1: hi <= ni)
      const uint32_t t0 = lo / FS_TILE + 1, t1 = (hi - 1) / FS_TILE;
      rows(lo, t0 * FS_TILE);
      for (uint32_t t = t0 + lane; t < t1; t += WAVE) C.tile(agg + (size_t)t * DT_MAX), C.all += agg_all[t];
      rows(t1 * FS_TILE, hi);
    }
    C.fold();
  }
  if (lane == 0) {
    C.store(O.ge + (size_t)f * O.n_thr, O.n_thr);
    if (O.covered) O.covered[f] = C.all;
  }
}

}  // namespace

extern "C" int tbk_cov_thresholds(tbk_ctx* ctx, const tbk_cov_out* rows, const tbk_features* F, const double* thr, uint32_t n_thr, tbk_thr_out* out) {
  if (!ctx || !rows || !F || !out) return TBK_EINVAL;
  if ((rows->mem != TBK_MEM_HOST && rows->mem != TBK_MEM_DEVICE) || (out->mem != TBK_MEM_HOST && out->mem != TBK_MEM_DEVICE)) return TBK_EINVAL;
  const uint32_t ni = rows->n_intervals;
  if (ni > rows->cap_intervals || ni == UINT32_MAX) return TBK_EINVAL;
  if (ni && (!rows->iv_tid || !rows->iv_start || !rows->iv_end || !rows->iv_val)) return TBK_EINVAL;
  const uint32_t n = F->n;
  if (n == 0 || !F->tid || !F->beg || !F->end || !out->ge) return TBK_EINVAL;
  for (uint32_t f = 0; f < n; ++f) {
    if (F->tid[f] < 0 || F->beg[f] < 0 || F->end[f] <= F->beg[f]) return TBK_EINVAL;
    if (F->strand && F->strand[f] != '+' && F->strand[f] != '-' && F->strand[f] != '.') return TBK_EINVAL;
  }
  if (!thr || n_thr < 1 || n_thr > DT_MAX) return ctx->last_error = "thresholds: between 1 and 16 of them", TBK_EINVAL;
  DtThr P;
  for (uint32_t k = 0; k < DT_MAX; ++k) P.t[k] = __builtin_inf();
  for (uint32_t k = 0; k < n_thr; ++k) {
    if (!isfinite(thr[k]) || !(thr[k] > 0.0)) return ctx->last_error = "thresholds: every threshold is finite and > 0", TBK_EINVAL;
    if (k && !(thr[k] > thr[k - 1])) return ctx->last_error = "thresholds: strictly ascending", TBK_EINVAL;
    P.t[k] = thr[k];
  }
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  const uint32_t n_tiles = ni > FS_DIRECT ? cdiv(ni, FS_TILE) : 0;  // (no run is longer than FS_DIRECT rows otherwise)
  const size_t n_ge = (size_t)n * n_thr;
  TBK_TRY(tbk_ws_reserve(ctx, (rows->mem == TBK_MEM_HOST ? (size_t)ni * 20 : 0) + (size_t)n * 20 + (n_ge + n) * 8 + (size_t)n_tiles * (DT_MAX + 1) * 8 + ((size_t)1 << 20)));
  FsRows R{};
  R.ni = ni;
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_tid, ni, &R.tid));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_start, ni, &R.start));
  TBK_TRY(fs_in(ctx, rows->mem, (const int32_t*)rows->iv_end, ni, &R.end));
  TBK_TRY(fs_in(ctx, rows->mem, (const double*)rows->iv_val, ni, &R.val));
  TBK_TRY(fs_check_order(ctx, R, "thresholds"));
  FsFeat D{};
  D.n = n;
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->tid, n, &D.tid));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->beg, n, &D.beg));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, F->end, n, &D.end));
  uint64_t *agg = nullptr, *agg_all = nullptr;
  if (n_tiles) {
    agg = ws_alloc<uint64_t>(ctx, (size_t)n_tiles * DT_MAX), agg_all = ws_alloc<uint64_t>(ctx, n_tiles);
    if (!agg || !agg_all) return TBK_ENOMEM;
    TBK_LAUNCH(ctx, "depththr_tiles", dt_tile_k, cdiv(n_tiles, FS_NT / WAVE), FS_NT, 0, R, n_tiles, P, agg, agg_all);
  }
  DtOut O{};
  O.n_thr = n_thr;
  TBK_TRY(fs_col(ctx, out->mem, out->ge, n_ge, &O.ge));
  if (out->covered) TBK_TRY(fs_col(ctx, out->mem, out->covered, n, &O.covered));
  TBK_LAUNCH(ctx, "depththr_features", dt_feat_k, cdiv(n, FS_NT / WAVE), FS_NT, 0, R, D, P, agg, agg_all, O);
  TBK_TRY(fs_back(ctx, out->mem, out->ge, O.ge, n_ge));
  if (out->covered) TBK_TRY(fs_back(ctx, out->mem, out->covered, O.covered, n));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return tbk_check_launch(ctx, "cov_thresholds");
}
