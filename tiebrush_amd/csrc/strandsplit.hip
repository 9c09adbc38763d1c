// strandsplit.hip — tbk_cov_split_strand: tiecov's input divided by splice strand into three complete inputs, what
// `--strand-cov PREFIX` of tiecov / tiebrush runs between a tile's view and the coverage chain.  A record's class is 0 for strand '+', 1
// for '-', 2 for every other byte; a record with flag bit 0x4 has no class and goes nowhere.
//
// A block owns SS_TILE consecutive records: SS_ROWS rows of SS_NT threads, so wave w of row r holds the 64 consecutive records of
// segment r * SS_NW + w, and the segments of a block ascend with the records.
//   ss_count_k    per block and class the records and their CIGAR words: a ballot on the class bit and its population count for the
//                 records, the lanes' word counts folded by a butterfly; six counters per block, counter-major.  It also checks what
//                 the scatter relies on — cig_off ascends and ends within n_cigar_ops — so a broken CSR is TBK_EINVAL, not a fault.
//   one exclusive scan (prims.hip) over the 6 * blocks + 1 counters: the difference to a counter row's first element is the block's base
//   ss_totals_k   the six totals, which the host reads to size the views
//   ss_scatter_k  the same ballots again: a record's rank in its segment is the population count of the ballot below its lane, its word
//                 offset there an inclusive wave scan less its own count; the segments' counts meet in LDS and are scanned by six
//                 threads.  Each record's columns go to block base + segment base + lane rank; yc travels as raw 64 bits.  CIGARs of up
//                 to SS_LANE_WORDS words are copied by their lane; longer ones one after the other by the whole wave, 64 words a step.
// No per-record array but the outputs is written.  The views live in one allocation of the context's (ctx->strand_split), apart from
// the arena and from the storage of every other view.
#include "dev_common.hpp"
#include "tbk_internal.h"

namespace {

constexpr int SS_NT = 256;
constexpr uint32_t SS_NW = SS_NT / WAVE;
constexpr uint32_t SS_ROWS = 4;
constexpr uint32_t SS_TILE = SS_NT * SS_ROWS;  // records of a block
constexpr uint32_t SS_SEG = SS_ROWS * SS_NW;   // its segments of 64 records
constexpr uint32_t SS_LANE_WORDS = 8;          // the longest CIGAR its own lane copies
constexpr uint32_t SS_NONE = 3;                // the class of a record that goes to no view

struct SsIn {
  uint32_t n, n_cigar_ops;
  const int32_t *tid, *pos;
  const uint16_t* flag;  // NULL: every record is mapped
  const uint8_t* strand;
  const uint32_t *cig_off, *cig;
  const uint64_t* yc;    // the doubles' bits; NULL: the views carry none
  const int64_t* yx;     // likewise
};
struct SsCols {
  int32_t *tid, *pos;
  uint8_t* strand;
  uint64_t* yc;
  int64_t* yx;
  uint32_t *cig_off, *cig;
};
struct SsOut {
  SsCols v[3];
};

// record i's class and, for a record of the input, its CIGAR range
__device__ __forceinline__ uint32_t ss_class(const SsIn& I, uint64_t i, uint32_t* c0, uint32_t* c1) {
  *c0 = *c1 = 0;
  if (i >= I.n) return SS_NONE;
  *c0 = I.cig_off[i], *c1 = I.cig_off[i + 1];
  if (I.flag && (I.flag[i] & 0x4)) return SS_NONE;
  const uint8_t s = I.strand[i];
  return s == '+' ? 0u : (s == '-' ? 1u : 2u);
}

// cnt[k * nb + b]: k < 3 the records of class k in block b, k >= 3 the CIGAR words of class k - 3; cnt[6 * nb] = 0 closes the scan
__global__ __launch_bounds__(SS_NT) void ss_count_k(SsIn I, uint32_t nb, uint32_t* __restrict__ cnt, uint32_t* __restrict__ bad) {
  __shared__ uint32_t sm[SS_NW][6];
  uint32_t rec[3] = {0, 0, 0}, wrd[3] = {0, 0, 0};
  bool broken = false;
#pragma unroll
  for (uint32_t r = 0; r < SS_ROWS; ++r) {
    const uint64_t i = (uint64_t)blockIdx.x * SS_TILE + r * SS_NT + threadIdx.x;
    uint32_t c0, c1;
    const uint32_t c = ss_class(I, i, &c0, &c1);
    broken |= c1 < c0 || c1 > I.n_cigar_ops;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      rec[k] += (uint32_t)__popcll(__ballot(c == k));
      wrd[k] += c == k ? c1 - c0 : 0u;
    }
  }
  if (broken) atomicOr(bad, 1u);
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) wrd[k] = wave_sum(wrd[k]);
  if (lane_id() == 0) {
    const uint32_t w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) sm[w][k] = rec[k], sm[w][3 + k] = wrd[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t w = 0; w < SS_NW; ++w) s += sm[w][threadIdx.x];
    cnt[(size_t)threadIdx.x * nb + blockIdx.x] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 6) cnt[(size_t)6 * nb] = 0;
}

// tot[k] = the sum of counter row k (base: the exclusive scan of cnt, 6 * nb + 1 elements)
__global__ void ss_totals_k(const uint64_t* __restrict__ base, uint32_t nb, uint64_t* __restrict__ tot) {
  const uint32_t k = threadIdx.x;
  if (k < 6) tot[k] = base[(size_t)(k + 1) * nb] - base[(size_t)k * nb];
}

__device__ __forceinline__ const SsCols& ss_view(const SsOut& O, uint32_t c) { return c == 0 ? O.v[0] : (c == 1 ? O.v[1] : O.v[2]); }

__global__ __launch_bounds__(SS_NT) void ss_scatter_k(SsIn I, uint32_t nb, const uint64_t* __restrict__ base, SsOut O) {
  __shared__ uint32_t seg[6][SS_SEG];  // row k: per segment the count of counter k, then the count of the segments before it
  __shared__ uint32_t blk[6];          // the block's bases
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t below = lanemask_lt();
  uint32_t cls[SS_ROWS], c0[SS_ROWS], nc[SS_ROWS], lrec[SS_ROWS], lwrd[SS_ROWS];
#pragma unroll
  for (uint32_t r = 0; r < SS_ROWS; ++r) {
    const uint64_t i = (uint64_t)blockIdx.x * SS_TILE + r * SS_NT + threadIdx.x;
    uint32_t c1;
    cls[r] = ss_class(I, i, &c0[r], &c1);
    nc[r] = c1 - c0[r];
    lrec[r] = lwrd[r] = 0;
    const uint32_t s = r * SS_NW + w;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      const bool mine = cls[r] == k;
      const uint64_t b = __ballot(mine);
      const uint32_t v = mine ? nc[r] : 0u;
      const uint32_t inc = wave_incl_sum(v);
      if (mine) lrec[r] = (uint32_t)__popcll(b & below), lwrd[r] = inc - v;
      if (lane == 63) seg[k][s] = (uint32_t)__popcll(b), seg[3 + k][s] = inc;
    }
  }
  if (threadIdx.x < 6) blk[threadIdx.x] = (uint32_t)(base[(size_t)threadIdx.x * nb + blockIdx.x] - base[(size_t)threadIdx.x * nb]);
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t s = 0; s < SS_SEG; ++s) {
      const uint32_t x = seg[threadIdx.x][s];
      seg[threadIdx.x][s] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < SS_ROWS; ++r) {
    const uint64_t i = (uint64_t)blockIdx.x * SS_TILE + r * SS_NT + threadIdx.x;
    const uint32_t s = r * SS_NW + w, c = cls[r];
    uint32_t d = 0;
    if (c < SS_NONE) {
      const SsCols& V = ss_view(O, c);
      const uint32_t o = blk[c] + seg[c][s] + lrec[r];
      d = blk[3 + c] + seg[3 + c][s] + lwrd[r];
      V.tid[o] = I.tid[i];
      V.pos[o] = I.pos[i];
      V.strand[o] = I.strand[i];
      if (I.yc) V.yc[o] = I.yc[i];
      if (I.yx) V.yx[o] = I.yx[i];
      V.cig_off[o] = d;
      if (nc[r] <= SS_LANE_WORDS)
        for (uint32_t q = 0; q < nc[r]; ++q) V.cig[d + q] = I.cig[c0[r] + q];
    }
    // the long CIGARs of the segment, one after the other, by the whole wave
    uint64_t todo = __ballot(c < SS_NONE && nc[r] > SS_LANE_WORDS);
    while (todo) {
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint32_t lc = __shfl(c, l, 64), src = __shfl(c0[r], l, 64), dst = __shfl(d, l, 64), m = __shfl(nc[r], l, 64);
      uint32_t* __restrict__ out = ss_view(O, lc).cig;
      for (uint32_t q = lane; q < m; q += WAVE) out[dst + q] = I.cig[src + q];
    }
  }
  // the closing offsets
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const uint32_t k = threadIdx.x;
    const uint64_t nr = base[(size_t)(k + 1) * nb] - base[(size_t)k * nb], nw = base[(size_t)(k + 4) * nb] - base[(size_t)(k + 3) * nb];
    ss_view(O, k).cig_off[nr] = (uint32_t)nw;
  }
}

struct TbkStrandSplit {
  char* base = nullptr;
  size_t cap = 0;
};

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t view_bytes(size_t nr, size_t nw) { return al256(nr * 4) * 2 + al256(nr) + al256(nr * 8) * 2 + al256((nr + 1) * 4) + al256(nw * 4 + 4); }

struct ProfEnd {
  tbk_ctx* c;
  ~ProfEnd() { tbk_prof_end_call(c); }
};

// a column of the input as a device pointer: a device column as it is, a host column through a copy into the arena
template <class T>
int col_in(tbk_ctx* ctx, int mem, const T* p, size_t n, const T** d) {
  *d = p;
  if (mem == TBK_MEM_DEVICE || !p || !n) return 0;
  T* a = ws_alloc<T>(ctx, n);
  if (!a) return TBK_ENOMEM;
  TBK_HIP(hipMemcpyAsync(a, p, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  *d = a;
  return 0;
}

}  // namespace

void tbk_strand_split_free(tbk_ctx* ctx) {
  TbkStrandSplit* S = (TbkStrandSplit*)ctx->strand_split;
  if (!S) return;
  if (S->base) (void)hipFree(S->base);
  delete S;
  ctx->strand_split = nullptr;
}

extern "C" int tbk_cov_split_strand(tbk_ctx* ctx, const tbk_cov_in* in, tbk_cov_in view[3]) {
  if (!ctx || !in || !view) return TBK_EINVAL;
  if (in->mem != TBK_MEM_HOST && in->mem != TBK_MEM_DEVICE) return TBK_EINVAL;
  const uint32_t n = in->n_records;
  // an input without records has no columns to speak of (a zeroed view, the columns of an empty table): three empty views, whatever the pointers
  if (n && !in->strand) return ctx->last_error = "cov_split_strand: the input carries no strand column", TBK_EINVAL;
  if (n && (!in->tid || !in->pos || !in->cig_off || (in->n_cigar_ops && !in->cig))) return TBK_EINVAL;  // (tbk_coverage_tile's rule)
  // the views of the last split are not an input of the next one: the scatter would write what it is reading, or read what was freed
  if (n && in->mem == TBK_MEM_DEVICE && ctx->strand_split) {
    const TbkStrandSplit* P = (const TbkStrandSplit*)ctx->strand_split;
    const char* t = (const char*)in->tid;
    if (P->base && t >= P->base && t < P->base + P->cap)
      return ctx->last_error = "cov_split_strand: the input is a view of the previous split (copy it, or split the original again)", TBK_EINVAL;
  }
  for (int s = 0; s < 3; ++s) {
    memset(&view[s], 0, sizeof(view[s]));
    view[s].mem = TBK_MEM_DEVICE;
  }
  if (n == 0) return 0;
  if (n == UINT32_MAX) return ctx->last_error = "cov_split_strand: more records than one call takes", TBK_E2BIG;  // (n + 1 offsets)
  TBK_HIP(hipSetDevice(ctx->device));
  tbk_prof_begin_call(ctx);
  ProfEnd prof_end{ctx};
  const uint32_t nb = cdiv(n, SS_TILE), nscan = 6 * nb + 1;
  const size_t nw_in = in->n_cigar_ops;
  const size_t up = in->mem == TBK_MEM_HOST ? (size_t)n * 27 + ((size_t)n + 1) * 4 + nw_in * 4 + 8 * 256 : 0;
  TBK_TRY(tbk_ws_reserve(ctx, up + (size_t)nscan * 12 + ((size_t)nscan >> 7) + ((size_t)1 << 20)));
  SsIn I{};
  I.n = n, I.n_cigar_ops = in->n_cigar_ops;
  TBK_TRY(col_in(ctx, in->mem, in->tid, n, &I.tid));
  TBK_TRY(col_in(ctx, in->mem, in->pos, n, &I.pos));
  TBK_TRY(col_in(ctx, in->mem, in->flag, n, &I.flag));
  TBK_TRY(col_in(ctx, in->mem, in->strand, n, &I.strand));
  TBK_TRY(col_in(ctx, in->mem, in->cig_off, (size_t)n + 1, &I.cig_off));
  TBK_TRY(col_in(ctx, in->mem, in->cig, nw_in, &I.cig));
  TBK_TRY(col_in(ctx, in->mem, (const uint64_t*)in->yc, n, &I.yc));
  TBK_TRY(col_in(ctx, in->mem, in->yx, n, &I.yx));
  uint32_t* cnt = ws_alloc<uint32_t>(ctx, nscan);
  uint64_t* base = ws_alloc<uint64_t>(ctx, nscan);
  uint64_t* tot = ws_alloc<uint64_t>(ctx, 8);  // [0 .. 5] the totals, [6] low word: the CSR check
  if (!cnt || !base || !tot) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(tot, 0, 64, ctx->stream));
  TBK_LAUNCH(ctx, "strand_count", ss_count_k, nb, SS_NT, 0, I, nb, cnt, (uint32_t*)(tot + 6));
  TBK_TRY(tbk_exscan_u32_u64(ctx, cnt, base, nscan, nullptr));
  TBK_LAUNCH(ctx, "strand_totals", ss_totals_k, 1, 64, 0, base, nb, tot);
  uint64_t h[7] = {0, 0, 0, 0, 0, 0, 0};
  TBK_HIP(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "cov_split_strand"));
  if (h[6]) return ctx->last_error = "cov_split_strand: cig_off does not ascend or runs past n_cigar_ops", TBK_EINVAL;
  if (h[0] + h[1] + h[2] > n || h[3] + h[4] + h[5] > nw_in) return TBK_EHIP;
  size_t need = 0;
  for (int s = 0; s < 3; ++s) need += view_bytes((size_t)h[s], (size_t)h[3 + s]);
  TbkStrandSplit* S = (TbkStrandSplit*)ctx->strand_split;
  if (!S) ctx->strand_split = S = new TbkStrandSplit();
  if (need > S->cap) {
    // (the previous views die here, whether or not the new buffer can be had)
    if (S->base) (void)hipFree(S->base);
    S->base = nullptr, S->cap = 0;
    const size_t cap = need + need / 4;
    char* p = nullptr;
    if (hipMalloc((void**)&p, cap) != hipSuccess) {
      (void)hipGetLastError();  // (the refusal is reported, not left behind for the next launch check)
      return ctx->last_error = "cov_split_strand: device allocation failed", TBK_ENOMEM;
    }
    S->base = p, S->cap = cap;
  }
  char* p = S->base;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += al256(bytes);
    return r;
  };
  SsOut O{};
  for (int s = 0; s < 3; ++s) {
    const size_t nr = (size_t)h[s], nw = (size_t)h[3 + s];
    SsCols& V = O.v[s];
    V.tid = (int32_t*)take(nr * 4);
    V.pos = (int32_t*)take(nr * 4);
    V.strand = (uint8_t*)take(nr);
    V.yc = (uint64_t*)take(nr * 8);
    V.yx = (int64_t*)take(nr * 8);
    V.cig_off = (uint32_t*)take((nr + 1) * 4);
    V.cig = (uint32_t*)take(nw * 4 + 4);
  }
  TBK_LAUNCH(ctx, "strand_scatter", ss_scatter_k, nb, SS_NT, 0, I, nb, base, O);
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  TBK_TRY(tbk_check_launch(ctx, "cov_split_strand"));
  for (int s = 0; s < 3; ++s) {
    const SsCols& V = O.v[s];
    view[s].n_records = (uint32_t)h[s];
    view[s].n_cigar_ops = (uint32_t)h[3 + s];
    view[s].tid = V.tid, view[s].pos = V.pos, view[s].cig_off = V.cig_off, view[s].cig = V.cig, view[s].strand = V.strand;
    view[s].yc = in->yc ? (const double*)V.yc : nullptr;
    view[s].yx = in->yx ? V.yx : nullptr;
  }
  return 0;
}
