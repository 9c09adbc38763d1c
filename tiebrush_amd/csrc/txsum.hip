// txsum.hip — tbk_tx_summary: the rows of a coverage call read against transcripts, what `tiecov --gtf FILE --transcripts
// OUT` / `tiebrush --gtf FILE --transcripts OUT` run.  A transcript is a run of exons (CSR: tx_off into ex_beg / ex_end, ascending, with
// at least one base between two of them); the introns are implied: [ex_end[e], ex_beg[e + 1]) behind every exon but the transcript's
// last.  Per exon: tbk_cov_summary's covered, sum and max of the exon on the transcript's reference.  Per intron: tbk_cov_summary's junc
// under the transcript's strand.  Per transcript: the fold of its parts (include/tbk.h).
//
// Two passes, so that a transcript of 300 exons does not serialise 600 searches on one wave while its neighbours have one exon:
//   tx_part_k   one wave per EXON: fs_cov_part for the exon and, unless the exon is its transcript's last, fs_junc_part for the intron
//               behind it — the very functions fs_feat_k calls (featsum_common.hpp), on the aggregates of the same fs_tile_k, so a
//               part has the bits tbk_cov_summary gives the exon or the intron as a feature.  Whether an exon is the last one comes from
//               ex_tx (the exon's transcript, filled by the host from tx_off) and tx_off: the wave of a last exon never reads
//               ex_beg[e + 1], a word that does not exist behind the table's very last exon.
//   tx_fold_k   one wave per transcript: lane k adds parts k, k + 64, ... of the transcript in that order, then a butterfly over the
//               lanes — an order that depends on the transcript's exon count alone.
// No floating-point atomics and no differences of prefix sums: two calls on the same inputs give the same bits, and where every product
// and partial sum is representable (YC integral, the default) any order gives the same bits as well.
#include "featsum_common.hpp"

namespace {

struct TxTab {
  uint32_t n_tx, n_exon;
  const uint32_t *tx_off, *ex_tx;  // [n_tx + 1], [n_exon]
  const int32_t* tid;              // [n_tx]
  const uint8_t* strand;           // [n_tx]; NULL: every transcript is '.'
  const int64_t *ex_beg, *ex_end;  // [n_exon]
};
struct TxParts {  // [n_exon]; the coverage three or in_junc NULL: that half is not computed
  uint64_t* covered;
  double *sum, *max, *in_junc;
};
struct TxOut {  // [n_tx]; NULL as in TxParts
  uint64_t* covered;
  double *sum, *max;
  uint32_t* exons_hit;
  uint32_t* introns_hit;
  double *junc_min, *junc_sum;
};

__global__ __launch_bounds__(FS_NT) void tx_part_k(FsRows R, TxTab T, FsAgg A, TxParts P) {
  const uint32_t e = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (e >= T.n_exon) return;  // (whole waves, as above)
  const uint32_t lane = lane_id();
  const uint32_t t = T.ex_tx[e];
  const int32_t ft = T.tid[t];
  const int64_t fb = T.ex_beg[e], fe = T.ex_end[e];
  if (P.covered) {
    double s = 0.0, m = 0.0;
    uint64_t c = 0;
    if (R.ni) fs_cov_part(R, A, ft, fb, fe, s, c, m);
    if (lane == 0) P.covered[e] = c, P.sum[e] = s, P.max[e] = c ? m : 0.0;
  }
  if (P.in_junc) {
    double j = 0.0;
    // (e is the wave's own: the branch is uniform, and only an exon with a successor in its transcript reads ex_beg[e + 1])
    if (R.nj && e + 1 != T.tx_off[t + 1]) j = fs_junc_part(R, ft, fe, T.ex_beg[e + 1], T.strand ? T.strand[t] : (uint8_t)'.');
    if (lane == 0) P.in_junc[e] = j;
  }
}

__global__ __launch_bounds__(FS_NT) void tx_fold_k(TxTab T, TxParts P, TxOut O) {
  const uint32_t t = blockIdx.x * (FS_NT / WAVE) + (threadIdx.x >> 6);
  if (t >= T.n_tx) return;  // (whole waves)
  const uint32_t lane = lane_id();
  const uint32_t e0 = T.tx_off[t], e1 = T.tx_off[t + 1];
  if (O.covered) {
    double s = 0.0, m = -__builtin_inf();
    uint64_t c = 0;
    uint32_t hit = 0;
    for (uint32_t e = e0 + lane; e < e1; e += WAVE) {
      const uint64_t ec = P.covered[e];
      s += P.sum[e];
      c += ec;
      if (ec) {
        const double v = P.max[e];
        m = v > m ? v : m;
        ++hit;
      }
    }
    fs_fold(s, c, m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hit += __shfl_xor(hit, d, 64);
    if (lane == 0) O.covered[t] = c, O.sum[t] = s, O.max[t] = c ? m : 0.0, O.exons_hit[t] = hit;
  }
  if (O.junc_sum) {
    double js = 0.0, jm = __builtin_inf();
    uint32_t hit = 0;
    for (uint32_t e = e0 + lane; e + 1 < e1; e += WAVE) {  // (the intron behind every exon but the last)
      const double j = P.in_junc[e];
      js += j;
      jm = j < jm ? j : jm;
      hit += j > 0.0 ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      js += __shfl_xor(js, d, 64);
      const double o = __shfl_xor(jm, d, 64);
      jm = o < jm ? o : jm;
      hit += __shfl_xor(hit, d, 64);
    }
    if (lane == 0) O.junc_sum[t] = js, O.junc_min[t] = e1 - e0 > 1 ? jm : 0.0, O.introns_hit[t] = hit;
  }
}

}  // namespace

extern "C" int tbk_tx_summary(tbk_ctx* ctx, const tbk_cov_out* rows, const tbk_transcripts* X, tbk_tx_out* out) {
  if (!ctx || !rows || !X || !out) return TBK_EINVAL;
  if ((rows->mem != TBK_MEM_HOST && rows->mem != TBK_MEM_DEVICE) || (out->mem != TBK_MEM_HOST && out->mem != TBK_MEM_DEVICE)) return TBK_EINVAL;
  const bool want_cov = rows->cap_intervals != 0, want_junc = rows->cap_junctions != 0;
  const uint32_t ni = want_cov ? rows->n_intervals : 0, nj = want_junc ? rows->n_junctions : 0;
  if (ni > rows->cap_intervals || nj > rows->cap_junctions || ni == UINT32_MAX || nj == UINT32_MAX) return TBK_EINVAL;
  if (ni && (!rows->iv_tid || !rows->iv_start || !rows->iv_end || !rows->iv_val)) return TBK_EINVAL;
  if (nj && (!rows->j_tid || !rows->j_start || !rows->j_end || !rows->j_strand || !rows->j_val)) return TBK_EINVAL;
  const uint32_t n_tx = X->n_tx, n_ex = X->n_exon;
  if (n_tx == 0 || n_ex == 0 || n_ex == UINT32_MAX || !X->tx_off || !X->tid || !X->ex_beg || !X->ex_end) return TBK_EINVAL;
  if (want_cov && (!out->covered || !out->sum || !out->max || !out->exons_hit)) return TBK_EINVAL;
  if (want_junc && (!out->introns_hit || !out->junc_min || !out->junc_sum)) return TBK_EINVAL;
  const int n_parts = (out->ex_covered ? 1 : 0) + (out->ex_sum ? 1 : 0) + (out->ex_max ? 1 : 0);
  if (n_parts != 0 && n_parts != 3) return ctx->last_error = "transcripts: ex_covered, ex_sum and ex_max are given together or not at all", TBK_EINVAL;
  if (X->tx_off[0] != 0 || X->tx_off[n_tx] != n_ex) return ctx->last_error = "transcripts: tx_off does not run from 0 to n_exon", TBK_EINVAL;
  for (uint32_t t = 0; t < n_tx; ++t) {
    const uint32_t e0 = X->tx_off[t], e1 = X->tx_off[t + 1];
    if (e1 <= e0 || e1 > n_ex) return ctx->last_error = "transcripts: tx_off is not strictly ascending (a transcript without an exon?)", TBK_EINVAL;
    if (X->tid[t] < 0) return TBK_EINVAL;
    if (X->strand && X->strand[t] != '+' && X->strand[t] != '-' && X->strand[t] != '.') return TBK_EINVAL;
    for (uint32_t e = e0; e < e1; ++e) {
      if (X->ex_beg[e] < 0 || X->ex_end[e] <= X->ex_beg[e]) return TBK_EINVAL;
      if (e > e0 && X->ex_beg[e] <= X->ex_end[e - 1])
        return ctx->last_error = "transcripts: the exons of a transcript are ascending with at least one base between them", TBK_EINVAL;
    }
  }
  if (!want_cov && !want_junc) return 0;
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  const uint32_t n_tiles = ni > FS_DIRECT ? cdiv(ni, FS_TILE) : 0;  // (no run is longer than FS_DIRECT rows otherwise)
  TBK_TRY(tbk_ws_reserve(ctx, (rows->mem == TBK_MEM_HOST ? (size_t)ni * 20 + (size_t)nj * 21 : 0) + (size_t)n_ex * (20 + 32) + (size_t)n_tx * (9 + 4 + 48) +
                                  (size_t)n_tiles * 24 + ((size_t)1 << 20)));
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
  TBK_TRY(fs_check_order(ctx, R, "transcripts"));
  // (the copies below are asynchronous: the map lives until the synchronise at the end of the call)
  std::vector<uint32_t> ex_tx(n_ex);
  for (uint32_t t = 0; t < n_tx; ++t)
    for (uint32_t e = X->tx_off[t]; e < X->tx_off[t + 1]; ++e) ex_tx[e] = t;
  TxTab T{};
  T.n_tx = n_tx, T.n_exon = n_ex;
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, X->tx_off, (size_t)n_tx + 1, &T.tx_off));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, (const uint32_t*)ex_tx.data(), n_ex, &T.ex_tx));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, X->tid, n_tx, &T.tid));
  if (X->strand) TBK_TRY(fs_in(ctx, TBK_MEM_HOST, X->strand, n_tx, &T.strand));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, X->ex_beg, n_ex, &T.ex_beg));
  TBK_TRY(fs_in(ctx, TBK_MEM_HOST, X->ex_end, n_ex, &T.ex_end));
  FsAgg A{};
  if (n_tiles) {
    A.sum = ws_alloc<double>(ctx, n_tiles), A.max = ws_alloc<double>(ctx, n_tiles), A.len = ws_alloc<uint64_t>(ctx, n_tiles);
    if (!A.sum || !A.max || !A.len) return TBK_ENOMEM;
    TBK_LAUNCH(ctx, "txsum_tiles", fs_tile_k, cdiv(n_tiles, FS_NT / WAVE), FS_NT, 0, R, n_tiles, A);
  }
  // the parts: the caller's arrays where given (device memory as they are), arena scratch otherwise
  const bool give_parts = n_parts == 3 && want_cov, give_junc = out->in_junc && want_junc;
  TxParts P{};
  if (want_cov) {
    TBK_TRY(fs_col(ctx, give_parts ? out->mem : TBK_MEM_HOST, out->ex_covered, n_ex, &P.covered));
    TBK_TRY(fs_col(ctx, give_parts ? out->mem : TBK_MEM_HOST, out->ex_sum, n_ex, &P.sum));
    TBK_TRY(fs_col(ctx, give_parts ? out->mem : TBK_MEM_HOST, out->ex_max, n_ex, &P.max));
  }
  if (want_junc) TBK_TRY(fs_col(ctx, give_junc ? out->mem : TBK_MEM_HOST, out->in_junc, n_ex, &P.in_junc));
  TBK_LAUNCH(ctx, "txsum_parts", tx_part_k, cdiv(n_ex, FS_NT / WAVE), FS_NT, 0, R, T, A, P);
  TxOut O{};
  if (want_cov) {
    TBK_TRY(fs_col(ctx, out->mem, out->covered, n_tx, &O.covered));
    TBK_TRY(fs_col(ctx, out->mem, out->sum, n_tx, &O.sum));
    TBK_TRY(fs_col(ctx, out->mem, out->max, n_tx, &O.max));
    TBK_TRY(fs_col(ctx, out->mem, out->exons_hit, n_tx, &O.exons_hit));
  }
  if (want_junc) {
    TBK_TRY(fs_col(ctx, out->mem, out->introns_hit, n_tx, &O.introns_hit));
    TBK_TRY(fs_col(ctx, out->mem, out->junc_min, n_tx, &O.junc_min));
    TBK_TRY(fs_col(ctx, out->mem, out->junc_sum, n_tx, &O.junc_sum));
  }
  TBK_LAUNCH(ctx, "txsum_fold", tx_fold_k, cdiv(n_tx, FS_NT / WAVE), FS_NT, 0, T, P, O);
  if (want_cov) {
    TBK_TRY(fs_back(ctx, out->mem, out->covered, O.covered, n_tx));
    TBK_TRY(fs_back(ctx, out->mem, out->sum, O.sum, n_tx));
    TBK_TRY(fs_back(ctx, out->mem, out->max, O.max, n_tx));
    TBK_TRY(fs_back(ctx, out->mem, out->exons_hit, O.exons_hit, n_tx));
    if (give_parts) {
      TBK_TRY(fs_back(ctx, out->mem, out->ex_covered, P.covered, n_ex));
      TBK_TRY(fs_back(ctx, out->mem, out->ex_sum, P.sum, n_ex));
      TBK_TRY(fs_back(ctx, out->mem, out->ex_max, P.max, n_ex));
    }
  }
  if (want_junc) {
    TBK_TRY(fs_back(ctx, out->mem, out->introns_hit, O.introns_hit, n_tx));
    TBK_TRY(fs_back(ctx, out->mem, out->junc_min, O.junc_min, n_tx));
    TBK_TRY(fs_back(ctx, out->mem, out->junc_sum, O.junc_sum, n_tx));
    if (give_junc) TBK_TRY(fs_back(ctx, out->mem, out->in_junc, P.in_junc, n_ex));
  }
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return tbk_check_launch(ctx, "tx_summary");
}
