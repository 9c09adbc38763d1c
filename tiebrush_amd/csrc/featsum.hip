// featsum.hip — tbk_cov_summary: the rows of a coverage call read against a list of features, what
// `tiecov --features BED --summary OUT` / `tiebrush --features BED --summary OUT` run.  Per feature [beg, end) on tid: the bases under a
// coverage row (covered), the sum of value x bases over them (sum), the largest row value (max) and the summed value of the junction rows
// that ARE the feature (junc: same tid, start and end, and the feature's strand; '.' takes every strand).
//
// The reference has no such option; the contract is stated against the rows themselves (include/tbk.h).  Interval rows are sorted by
// (tid, start) and disjoint, so the rows a feature meets are ONE run [lo, hi), found by two searches; only the run's first and last row can
// reach beyond the feature.  Junction rows are sorted by (tid, start, end, strand): the feature's rows are found by one search.
// (fs_order_k, the searches, the fold and the tile constants are shared with tbk_cov_thresholds, the run walk and the junction lookup of
// fs_feat_k with tbk_tx_summary: featsum_common.hpp)
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

struct FsOut {
  uint64_t* covered;
  double *sum, *max, *junc;
};

__global__ __launch_bounds__(FS_NT) void fs_feat_k(FsRows R, FsFeat F, FsAgg A, FsOut O) {
  const uint32_t f = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (f >= F.n) return;  // (whole waves, as above)
  const uint32_t lane = lane_id();
  const int32_t ft = F.tid[f];
  const int64_t fb = F.beg[f], fe = F.end[f];
  if (O.covered) {
    double s = 0.0, m = 0.0;
    uint64_t c = 0;
    if (R.ni) fs_cov_part(R, A, ft, fb, fe, s, c, m);
    if (lane == 0) O.covered[f] = c, O.sum[f] = s, O.max[f] = c ? m : 0.0;
  }
  if (O.junc) {
    const double j = R.nj ? fs_junc_part(R, ft, fb, fe, F.strand ? F.strand[f] : (uint8_t)'.') : 0.0;
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
