// stream.hip — tiecov over a record stream that arrives in tiles: tbk_cov_stream_push cuts the stream where tiecov itself
// cuts it, at the last bundle head, and hands out everything before that head as tiecov's input view; the records from the head on — the
// bundle that is still open — wait in the context (the carry) for the next tile.  The reference flushes coverage, sample rows and
// junctions per bundle (tiecov.cpp:435-499), so the rows of the views, one after the other, are the rows of the uncut stream.
//
//   st_ends_k    (a) a thread per record of the tile: its end by the coverage path's own rule (cov_prep_k: pos + walk_exons' length), its
//                reference with unmapped records masked out (INT32_MIN: the bundle monoid's "no record"), the flags and CIGAR counts of
//                the mapped records for the two rank scans
//   st_agg_k     (b) the bundle aggregate (cb_tiles.hpp: CbAgg / CbOp, cov.hip's monoid) of every block of CB_TILE records of carry ++ tile;
//                the block that finishes last turns them into the aggregates BEFORE every block (cb_spine_block)
//   st_heads_k   (b) the same walk again: every record knows whether it opens a bundle (cb_is_head, the rule cb_heads_k uses); a block that
//                holds a head raises ONE atomicMax of (index + 1) on a 32-bit word — integers only, the result does not depend on timing
//   two exclusive scans (tbk_exscan_u32) over the mapped flags and their CIGAR counts, n + 1 elements each
//   st_split_k   (c) a thread per record: a mapped record before the cut goes to the view, behind the carry; one from the cut on to the
//                OTHER carry buffer; cig_off is rebased on both sides
// The carry is a bundle prefix: it starts with a head and holds no other.  A block of the passes (b) covers records of the carry or of the
// tile, never both, so both columns are read from their aligned starts with 16-byte loads.  The old carry moves as whole columns
// (device-to-device copies) in front of the view or, when the tile brought no head, in front of the new carry: its offsets need no rebase.
#include "cb_tiles.hpp"
#include "tbk_internal.h"

namespace {

constexpr int ST_NT = 256;

struct StCols {
  int32_t *tid, *pos, *end;
  uint16_t* flag;
  uint8_t* strand;
  double* yc;
  int64_t* yx;
  uint32_t *cig_off, *cig;
};
struct StBuf {
  char* base = nullptr;
  size_t cap = 0;
  StCols c{};
};
struct TbkCovStream {
  StBuf carry[2], view;
  int cur = 0;  // carry[cur] holds the carry: n_carry records, c_cig CIGAR words
  uint32_t n_carry = 0, c_cig = 0;
  int32_t first_tid = -2, first_pos = 0;  // the carry's first record (-2: the carry is empty), for the caller's messages
};

// one column of carry ++ tile for the passes (b): tid (INT32_MIN: not a record), pos, end
struct StSrc {
  const int32_t *tid, *pos, *end;
  uint32_t n;
};

// (a)
__global__ __launch_bounds__(ST_NT) void st_ends_k(uint32_t n, const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, const uint16_t* __restrict__ flag,
                                                   const uint32_t* __restrict__ cig_off, const uint32_t* __restrict__ cig, int32_t* __restrict__ mtid,
                                                   int32_t* __restrict__ mpos, int32_t* __restrict__ end, uint32_t* __restrict__ keep /* [n + 1] */, uint32_t* __restrict__ kcig /* [n + 1] */) {
  const uint64_t i = (uint64_t)blockIdx.x * ST_NT + threadIdx.x;
  if (i > n) return;
  uint32_t k = 0, kc = 0;
  if (i < n) {
    const bool mapped = !(flag[i] & 0x4);
    const uint32_t c0 = cig_off[i], nc = cig_off[i + 1] - c0;
    int nex = 0;
    const int32_t p = pos[i];
    const int l = mapped ? walk_exons(p, cig + c0, nc, [](int, int) {}, &nex) : 0;
    mtid[i] = mapped ? tid[i] : INT32_MIN;
    mpos[i] = p;  // (a copy at an aligned start: the passes (b) read four records at a time, whatever the caller's column is aligned to)
    end[i] = p + l;  // (1-based inclusive, as cov_prep_k's A.end)
    k = mapped ? 1u : 0u;
    kc = mapped ? nc : 0u;
  }
  keep[i] = k;
  kcig[i] = kc;
}

// the column and the block in it that a block of the passes (b) walks: the first nbc blocks cover the carry, the others the tile
struct StBlock {
  StSrc s;
  uint32_t blk, gbase;
};
__device__ __forceinline__ StBlock st_block(const StSrc& C, const StSrc& T, uint32_t nbc) {
  return blockIdx.x < nbc ? StBlock{C, blockIdx.x, 0u} : StBlock{T, blockIdx.x - nbc, C.n};
}
__device__ __forceinline__ CbAgg st_elem(int32_t t, int32_t e) { return CbAgg{t, t, e, 1u}; }  // (t == INT32_MIN: CbOp's "no record")

// (b) first walk
__global__ __launch_bounds__(CB_NT) void st_agg_k(StSrc C, StSrc T, uint32_t nbc, uint4* __restrict__ part, uint32_t* __restrict__ done) {
  constexpr uint32_t NWV = CB_NT / 64;
  __shared__ CbAgg wl[CB_ROWS * NWV];
  const CbOp op{};
  const CbAgg none{0, INT32_MIN, INT32_MIN, 1u};
  const StBlock B = st_block(C, T, nbc);
  const uint32_t m = B.s.n;
#pragma unroll
  for (uint32_t r = 0; r < CB_ROWS; ++r) {
    const uint64_t i = (uint64_t)B.blk * CB_TILE + ((uint64_t)r * CB_NT + threadIdx.x) * 4u;
    int32_t t4[4], e4[4];
    cb_load4(B.s.tid, i, m, INT32_MIN, t4);
    cb_load4(B.s.end, i, m, 0, e4);
    CbAgg a = none;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < m) a = op(a, st_elem(t4[e], e4[e]));
    a = wave_incl_scan_op(a, op);
    if (lane_id() == 63) wl[r * NWV + (threadIdx.x >> 6)] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    CbAgg run = none;
#pragma unroll
    for (uint32_t q = 0; q < CB_ROWS * NWV; ++q) run = op(run, wl[q]);
    uint64_t* o = reinterpret_cast<uint64_t*>(part + blockIdx.x);
    cb_put(o, (uint64_t)(uint32_t)run.first_tid | ((uint64_t)(uint32_t)run.last_tid << 32));
    cb_put(o + 1, (uint64_t)(uint32_t)run.mx | ((uint64_t)run.whole << 32));
  }
  if (cb_last_block(done)) cb_spine_block<CB_NT>(part, gridDim.x, wl);
}

// (b) second walk: *head1 = 1 + the index in carry ++ tile of the last record that opens a bundle (0: there is no record)
__global__ __launch_bounds__(CB_NT) void st_heads_k(StSrc C, StSrc T, uint32_t nbc, const uint4* __restrict__ part, uint32_t* __restrict__ head1) {
  __shared__ CbAgg sm[CB_NT / 64], wl[CB_NT / 64];
  __shared__ uint32_t smx[CB_NT / 64];
  const CbOp op{};
  const CbAgg none{0, INT32_MIN, INT32_MIN, 1u};
  const StBlock B = st_block(C, T, nbc);
  const uint32_t m = B.s.n;
  const uint4 pv = part[blockIdx.x];
  CbAgg run{(int32_t)pv.x, (int32_t)pv.y, (int32_t)pv.z, pv.w};  // the records before the current row
  uint32_t best = 0;
#pragma unroll
  for (uint32_t r = 0; r < CB_ROWS; ++r) {
    const uint64_t i = (uint64_t)B.blk * CB_TILE + ((uint64_t)r * CB_NT + threadIdx.x) * 4u;
    int32_t t4[4], p4[4], e4[4];
    cb_load4(B.s.tid, i, m, INT32_MIN, t4);
    cb_load4(B.s.pos, i, m, 0, p4);
    cb_load4(B.s.end, i, m, 0, e4);
    CbAgg a = none;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i + e < m) a = op(a, st_elem(t4[e], e4[e]));
    CbAgg tot;
    const CbAgg inc = block_incl_scan_op(a, op, sm, &tot);
    // the aggregate of everything before this thread's first record: run (+) the threads before it in the row
    CbAgg ex = shfl_up_t(inc, 1);
    if (lane_id() == 63) wl[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0)
      ex = none;
    else if (lane_id() == 0)
      ex = wl[(threadIdx.x >> 6) - 1];
    CbAgg w = op(run, ex);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i + e < m && t4[e] != INT32_MIN) {
        if (cb_is_head(w, t4[e], p4[e] + 1)) best = B.gbase + (uint32_t)(i + e) + 1u;  // (rows and elements ascend: the last one stays)
        w = op(w, st_elem(t4[e], e4[e]));
      }
    }
    run = op(run, tot);
    __syncthreads();
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(best, d, 64);
    best = o > best ? o : best;
  }
  if (lane_id() == 0) smx[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (uint32_t q = 1; q < CB_NT / 64; ++q) best = smx[q] > best ? smx[q] : best;
    if (best) atomicMax(head1, best);
  }
}

// (c) V: the view, its records from v_rec and its CIGAR words from v_cig on (behind the carry, when that went there); K: the new carry
// likewise.  counts: [0] mapped records of the tile before the cut, [1] their CIGAR words, [2] / [3] the same for the whole tile.
__global__ __launch_bounds__(ST_NT) void st_split_k(uint32_t n, uint32_t cut, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ koff /* [n + 1] */,
                                                    const uint32_t* __restrict__ coff /* [n + 1] */, const int32_t* __restrict__ tid,
                                                    const int32_t* __restrict__ pos, const uint16_t* __restrict__ flag, const uint8_t* __restrict__ strand,
                                                    const uint32_t* __restrict__ cig_off, const uint32_t* __restrict__ cig, const double* __restrict__ yc,
                                                    const int64_t* __restrict__ yx, const uint8_t* __restrict__ seen, const int32_t* __restrict__ end, StCols V,
                                                    uint32_t v_rec, uint32_t v_cig, StCols K, uint32_t k_rec, uint32_t k_cig, uint32_t* __restrict__ counts) {
  const uint64_t i = (uint64_t)blockIdx.x * ST_NT + threadIdx.x;
  if (i > n) return;
  const uint32_t rc = koff[cut], cc = coff[cut];
  if (i == n) {  // the closing offsets of both CSRs, and what the host wants to know
    V.cig_off[v_rec + rc] = v_cig + cc;
    K.cig_off[k_rec + (koff[n] - rc)] = k_cig + (coff[n] - cc);
    counts[0] = rc, counts[1] = cc, counts[2] = koff[n], counts[3] = coff[n];
    return;
  }
  if (!keep[i]) return;
  const bool taken = i < cut;
  const StCols& O = taken ? V : K;
  const uint32_t o = taken ? v_rec + koff[i] : k_rec + (koff[i] - rc);
  const uint32_t d = taken ? v_cig + coff[i] : k_cig + (coff[i] - cc);
  const uint32_t sn = seen ? seen[i] : 3u;
  O.tid[o] = tid[i];
  O.pos[o] = pos[i];
  O.end[o] = end[i];
  O.flag[o] = flag[i];
  O.strand[o] = strand[i];
  O.yc[o] = (yc && (sn & 1u)) ? yc[i] : 1.0;  // tbk_region_view's rule (tiecov.cpp:482-485): YC absent -> 1.0, YX absent -> 1
  O.yx[o] = (yx && (sn & 2u)) ? yx[i] : (int64_t)1;
  O.cig_off[o] = d;
  const uint32_t c0 = cig_off[i], nc = cig_off[i + 1] - c0;
  for (uint32_t q = 0; q < nc; ++q) O.cig[d + q] = cig[c0 + q];
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t buf_bytes(size_t nr, size_t nw) { return al256(nr * 4) * 3 + al256(nr * 2) + al256(nr) + al256(nr * 8) * 2 + al256((nr + 1) * 4) + al256(nw * 4 + 4); }
// room for nr records and nw CIGAR words in a buffer whose content is dead: a larger one is allocated before the old one goes
int buf_ensure(tbk_ctx* ctx, StBuf* b, size_t nr, size_t nw) {
  const size_t need = buf_bytes(nr, nw);
  if (need > b->cap) {
    char* p = nullptr;
    const size_t cap = need + need / 4;
    if (hipMalloc((void**)&p, cap) != hipSuccess) {
      (void)hipGetLastError();  // (the refusal is reported, not left behind for the next launch check)
      ctx->last_error = "cov_stream: device allocation failed";
      return TBK_ENOMEM;
    }
    if (b->base) (void)hipFree(b->base);
    b->base = p;
    b->cap = cap;
  }
  char* p = b->base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += al256(bytes);
    return r;
  };
  b->c.tid = (int32_t*)take(nr * 4);
  b->c.pos = (int32_t*)take(nr * 4);
  b->c.end = (int32_t*)take(nr * 4);
  b->c.flag = (uint16_t*)take(nr * 2);
  b->c.strand = (uint8_t*)take(nr);
  b->c.yc = (double*)take(nr * 8);
  b->c.yx = (int64_t*)take(nr * 8);
  b->c.cig_off = (uint32_t*)take((nr + 1) * 4);
  b->c.cig = (uint32_t*)take(nw * 4 + 4);
  return 0;
}

struct ProfEnd {
  tbk_ctx* c;
  ~ProfEnd() { tbk_prof_end_call(c); }
};

template <class T>
int col_copy(tbk_ctx* ctx, T* dst, const T* src, size_t n) {
  if (n) TBK_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

}  // namespace

void tbk_cov_stream_free(tbk_ctx* ctx) {
  TbkCovStream* S = (TbkCovStream*)ctx->cov_stream;
  if (!S) return;
  for (StBuf* b : {&S->carry[0], &S->carry[1], &S->view})
    if (b->base) (void)hipFree(b->base);
  delete S;
  ctx->cov_stream = nullptr;
}

extern "C" int tbk_cov_stream_reset(tbk_ctx* ctx) {
  if (!ctx) return TBK_EINVAL;
  TbkCovStream* S = (TbkCovStream*)ctx->cov_stream;
  if (S) S->n_carry = S->c_cig = 0, S->first_tid = -2, S->first_pos = 0;  // (the buffers stay for the next stream)
  return 0;
}

extern "C" int tbk_cov_stream_push(tbk_ctx* ctx, const tbk_soa_in* tile, const uint8_t* tag_seen, int final, tbk_cov_in* view, tbk_cov_stream_info* info) {
  if (!ctx || !tile || !view || !info) return TBK_EINVAL;
  if (tile->mem != TBK_MEM_DEVICE) {
    ctx->last_error = "cov_stream: the tile must be in device memory";
    return TBK_EINVAL;
  }
  const uint32_t n = tile->n_records;
  if (n && (!tile->tid || !tile->pos || !tile->flag || !tile->strand || !tile->cig_off || (tile->n_cigar_ops && !tile->cig))) return TBK_EINVAL;
  TbkCovStream* S = (TbkCovStream*)ctx->cov_stream;
  const uint64_t nc = S ? S->n_carry : 0, cw = S ? S->c_cig : 0;
  // (n + 1 elements are scanned and the head's index travels as index + 1)
  if (nc + n > (uint64_t)UINT32_MAX - 1 || cw + tile->n_cigar_ops > (uint64_t)UINT32_MAX - 1 || (ctx->dbg.stream_cap && nc + n > ctx->dbg.stream_cap)) {
    // which bundle: the carry's first record, as the last push left it; without a carry the tile's first record, read here
    memset(info, 0, sizeof(*info));
    info->n_carry = (uint32_t)nc;
    info->first_tid = nc ? S->first_tid : -2;
    info->first_pos = nc ? S->first_pos : 0;
    if (!nc && n && hipSetDevice(ctx->device) == hipSuccess) {
      int32_t tp[2] = {-2, 0};
      if (hipMemcpy(&tp[0], tile->tid, 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(&tp[1], tile->pos, 4, hipMemcpyDeviceToHost) == hipSuccess)
        info->first_tid = tp[0], info->first_pos = tp[1];
      else
        (void)hipGetLastError();
    }
    ctx->last_error = "cov_stream: the open bundle and the tile exceed what one view can hold";
    return TBK_E2BIG;
  }
  TBK_HIP(hipSetDevice(ctx->device));
  if (!S) {
    S = new TbkCovStream();
    ctx->cov_stream = S;
  }
  memset(view, 0, sizeof(*view));
  view->mem = TBK_MEM_DEVICE;
  memset(info, 0, sizeof(*info));
  info->first_tid = -2;
  if (nc + n == 0) return 0;
  const size_t tot_rec = (size_t)(nc + n), tot_cig = (size_t)(cw + tile->n_cigar_ops);
  const uint32_t nbc = cdiv(nc, CB_TILE), nbt = cdiv(n, CB_TILE), nb = nbc + nbt;
  // Everything that can fail for want of memory comes first: the carry is not touched before it.  (The previous view dies here.)
  StBuf* const cur = &S->carry[S->cur];
  StBuf* const nxt = &S->carry[S->cur ^ 1];
  TBK_TRY(buf_ensure(ctx, &S->view, tot_rec, tot_cig));
  TBK_TRY(buf_ensure(ctx, nxt, tot_rec, tot_cig));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  TBK_TRY(tbk_ws_reserve(ctx, ((size_t)n + 1) * 28 + (size_t)nb * 16 + ((size_t)n >> 7) + ((size_t)2 << 20)));
  int32_t *mtid = ws_alloc<int32_t>(ctx, n), *mpos = ws_alloc<int32_t>(ctx, n), *tend = ws_alloc<int32_t>(ctx, n);
  uint32_t *keep = ws_alloc<uint32_t>(ctx, (size_t)n + 1), *kcig = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint32_t *koff = ws_alloc<uint32_t>(ctx, (size_t)n + 1), *coff = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint4* part = ws_alloc<uint4>(ctx, nb);
  uint32_t* sc = ws_alloc<uint32_t>(ctx, 8);  // [0] done, [1] head + 1, [4 .. 7] st_split_k's counts
  if (!mtid || !mpos || !tend || !keep || !kcig || !koff || !coff || !part || !sc) return TBK_ENOMEM;
  ctx->view_prep.valid = false;
  TBK_HIP(hipMemsetAsync(sc, 0, 32, ctx->stream));
  TBK_LAUNCH(ctx, "stream_ends", st_ends_k, cdiv((uint64_t)n + 1, ST_NT), ST_NT, 0, n, tile->tid, tile->pos, tile->flag, tile->cig_off, tile->cig, mtid, mpos, tend,
             keep, kcig);
  const StSrc C{cur->c.tid, cur->c.pos, cur->c.end, (uint32_t)nc}, T{mtid, mpos, tend, n};
  TBK_LAUNCH(ctx, "stream_heads", st_agg_k, nb, CB_NT, 0, C, T, nbc, part, sc);
  TBK_LAUNCH(ctx, "stream_heads", st_heads_k, nb, CB_NT, 0, C, T, nbc, part, sc + 1);
  TBK_TRY(tbk_exscan_u32(ctx, keep, koff, n + 1, nullptr));
  TBK_TRY(tbk_exscan_u32(ctx, kcig, coff, n + 1, nullptr));
  uint32_t head1 = 0;
  TBK_HIP(hipMemcpyAsync(&head1, sc + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "cov_stream_push"));
  // the cut: the last head when the tile holds it; a tile without a head adds to the open bundle and everything waits
  const bool head_in_tile = head1 && (uint64_t)head1 - 1 >= nc;
  const bool carry_to_view = final || head_in_tile;
  const uint32_t cut = final ? n : (head_in_tile ? (uint32_t)(head1 - 1 - nc) : 0u);
  const StCols& D = carry_to_view ? S->view.c : nxt->c;
  TBK_TRY(col_copy(ctx, D.tid, cur->c.tid, nc));
  TBK_TRY(col_copy(ctx, D.pos, cur->c.pos, nc));
  TBK_TRY(col_copy(ctx, D.end, cur->c.end, nc));
  TBK_TRY(col_copy(ctx, D.flag, cur->c.flag, nc));
  TBK_TRY(col_copy(ctx, D.strand, cur->c.strand, nc));
  TBK_TRY(col_copy(ctx, D.yc, cur->c.yc, nc));
  TBK_TRY(col_copy(ctx, D.yx, cur->c.yx, nc));
  TBK_TRY(col_copy(ctx, D.cig_off, cur->c.cig_off, nc));  // (st_split_k writes the closing offset)
  TBK_TRY(col_copy(ctx, D.cig, cur->c.cig, cw));
  const uint32_t v_rec = carry_to_view ? (uint32_t)nc : 0u, v_cig = carry_to_view ? (uint32_t)cw : 0u;
  const uint32_t k_rec = carry_to_view ? 0u : (uint32_t)nc, k_cig = carry_to_view ? 0u : (uint32_t)cw;
  TBK_LAUNCH(ctx, "stream_split", st_split_k, cdiv((uint64_t)n + 1, ST_NT), ST_NT, 0, n, cut, keep, koff, coff, tile->tid, tile->pos, tile->flag, tile->strand,
             tile->cig_off, tile->cig, tile->yc_in, tile->yx_in, tag_seen, tend, S->view.c, v_rec, v_cig, nxt->c, k_rec, k_cig, sc + 4);
  uint32_t cnt[4] = {0, 0, 0, 0};
  int32_t first[2] = {-2, 0};  // (the new carry's first record, should it hold one: its columns are complete in stream order)
  TBK_HIP(hipMemcpyAsync(cnt, sc + 4, 16, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&first[0], nxt->c.tid, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&first[1], nxt->c.pos, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "cov_stream_push"));
  if (cnt[0] > cnt[2] || cnt[1] > cnt[3] || cnt[2] > n || cnt[3] > tile->n_cigar_ops) return TBK_EHIP;
  S->cur ^= 1;
  S->n_carry = k_rec + (cnt[2] - cnt[0]);
  S->c_cig = k_cig + (cnt[3] - cnt[1]);
  S->first_tid = S->n_carry ? first[0] : -2;
  S->first_pos = S->n_carry ? first[1] : 0;
  view->n_records = v_rec + cnt[0];
  view->n_cigar_ops = v_cig + cnt[1];
  const StCols& V = S->view.c;
  view->tid = V.tid, view->pos = V.pos, view->flag = V.flag, view->cig_off = V.cig_off, view->cig = V.cig;
  view->yc = V.yc, view->strand = V.strand, view->yx = V.yx;
  info->n_view = view->n_records;
  info->n_carry = S->n_carry;
  info->n_taken = cnt[0];
  info->cut = cut;
  info->first_tid = S->first_tid, info->first_pos = S->first_pos;
  return 0;
}
