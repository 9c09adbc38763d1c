// featsum.hip — tbk_cov_summary: the rows of a coverage call read against a list of features, what
// `tiecov --features BED --summary OUT` / `tiebrush --features BED --summary OUT` run.  Per feature [beg, end) on tid: the bases under a
// coverage row (covered), the sum of value x bases over them (sum), the largest row value (max) and the summed value of the junction rows
// that ARE the feature (junc: same tid, start and end, and the feature's strand; '.' takes every strand).
//
// The reference has no such option; the contract is stated against the rows themselves (include/tbk.h).  Interval rows are sorted by
// (tid, start) and disjoint, so the rows a feature meets are ONE run [lo, hi), found by two searches; only the run's first and last row can
// reach beyond the feature.  Junction rows are sorted by (tid, start, end, strand): the feature's rows are found by one search.
// (fs_order_k, the searches, the fold and the tile constants are shared with tbk_cov_thresholds: featsum_common.hpp)
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
#include "featsum_common.hpp"

namespace {

// (the two constants are featsum_common.hpp's; tests/test_feature_model_cpu.py reads their values off this line to hold its mirrors to them)
static_assert(FS_TILE == 256 && FS_DIRECT == 256, "constexpr uint32_t FS_TILE = 256; constexpr uint32_t FS_DIRECT = 256;");

struct FsAgg {
  double *sum, *max;
  uint64_t* len;
};
struct FsOut {
  uint64_t* covered;
  double *sum, *max, *junc;
};

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
  TBK_TRY(fs_check_order(ctx, R, "summary"));
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
