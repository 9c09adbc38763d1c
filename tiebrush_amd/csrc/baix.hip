// baix.hip — the BAM index part of an encoded run (tbk_bam_encode_indexed, include/tbk.h; contract: DESIGN.md §4d): what htslib's
// hts_idx_push / hts_idx_finish make of a second pass over the written file, from what the encoder holds when its members are packed —
// the tagged records in the payload stream, their offsets (enc_plan_k's scan), the member cuts (enc_cuts_k) and the members'
// prefix-summed compressed sizes (bgz_gather_k's table).
//
//   ix_rec_k      16 lanes per record: refID / pos / l_read_name / n_cigar_op out of the record's first dwords in the payload stream (the
//                 records lie back to back there, whatever their source was: the lanes' loads coalesce), the CIGAR's reference length
//                 summed over the lanes; lane 0 bisects the cuts for the record's member -> (tid, bin), (tid, end), vbeg
//   tx_rec_k      the other front end (tbk_track_bgzf): one thread per row of a text track, the row's line in the place of the record
//   ix_head_k     run heads: a record whose (tid, bin) differs from its predecessor's; refIDs must not decrease
//   ix_runs_k     the runs compacted (tbk_exscan_u32 of the heads): sort key (tid, bin | beg), the run's end = the vbeg behind its last record
//   tbk_radix_sort128 of the runs by (tid, bin, beg); ix_mhead_k / ix_chunks_k merge neighbours of one bin that meet in one member
//   ix_lin_k      the linear table by a running maximum and a bisection per window: M[g] = max over the records up to g of (tid << 32 |
//                 end) (scan_op_run; refIDs do not decrease, so the maximum restarts by itself at every reference), and window w of
//                 reference t takes the vbeg of the first g with M[g] > (t << 32 | w << 14) — no atomics, one thread per window, the
//                 table's bytes are the same from run to run.  (The other form, one atomicMin per window a record touches plus a fill from
//                 the right, needs the same scan for the fill and 64-bit atomics on top.)
//   ix_refs_k     per reference between the run's first and last: its record range by two bisections in M
// tbk_ix_opts.reserved selects the bins: 0 the BAI's (depth 5, ends up to 2^29), k >= 1 a CSI's of depth k - 1 (ends up to 2^(14 + 3 (k - 1))).
// The runs, the chunks, the window table and the part are the same for both; the host's combiner turns the table into a CSI's loff per bin.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dev_common.hpp"
#include "scan_op.hpp"
#include "tbk_internal.h"

namespace {

constexpr uint32_t IX_E_RANGE = 8u, IX_E_UNSORTED = 16u, IX_E_MALFORMED = 32u;  // bits of ctx->d_err inside this call
constexpr uint64_t IX_MAX_END = 1ull << 29;                                      // what a BAI's bins and windows address
constexpr uint32_t IX_MAX_DEPTH = 6;                                             // CSI: 2^(14 + 3 * 6) covers every BAM length (< 2^31)

__device__ __forceinline__ uint32_t ix_rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
// UCSC binning (SAM specification 5.3; htslib hts_reg2bin(beg, end, 14, 5))
__device__ __forceinline__ uint32_t ix_reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
  return 0u;
}
// the same scheme with `depth` levels below bin 0 (CSI, min_shift 14; htslib hts_reg2bin(beg, end, 14, depth)); end <= 2^(14 + 3 * depth)
__device__ __forceinline__ uint32_t ix_reg2bin_depth(uint64_t beg, uint64_t end, uint32_t depth) {
  --end;
  uint32_t s = 14, t = ((1u << (3 * depth)) - 1u) / 7u;
  for (uint32_t l = depth; l > 0; --l) {
    if (beg >> s == end >> s) return t + (uint32_t)(beg >> s);
    s += 3, t -= 1u << (3 * (l - 1));
  }
  return 0u;
}

__global__ __launch_bounds__(256) void ix_rec_k(uint32_t n, const uint8_t* __restrict__ pay, const uint64_t* __restrict__ ooff, uint32_t nmem,
                                                const uint64_t* __restrict__ cut, const uint64_t* __restrict__ moff, uint64_t ztotal, uint32_t n_ref,
                                                const uint64_t* __restrict__ base, uint32_t fmt, uint64_t* __restrict__ key, uint64_t* __restrict__ tend,
                                                uint64_t* __restrict__ vbeg, uint32_t* __restrict__ err) {
  const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, sub = threadIdx.x & 15u;
  if (g > n) return;  // (the sixteen lanes of a record leave together)
  if (g == n) {
    if (sub == 0) vbeg[n] = ztotal << 16;
    return;
  }
  const uint64_t o = ooff[g];
  const uint64_t len = ooff[g + 1] - o;  // block_size field + record + tags
  const uint8_t* p = pay + o;
  // block_size | refID | pos | l_read_name, mapq, bin | n_cigar_op, flag | ... (36 bytes) | read_name | cigar
  uint32_t v = 0;
  const bool hdr_ok = len >= 36;
  if (hdr_ok && sub >= 1 && sub <= 4) v = ix_rd32(p + 4 * sub);
  const int32_t tid = (int32_t)__shfl(v, 1, 16), pos = (int32_t)__shfl(v, 2, 16);
  const uint32_t l_qname = (uint32_t)__shfl(v, 3, 16) & 0xffu, n_cig = (uint32_t)__shfl(v, 4, 16) & 0xffffu;
  const uint64_t cig0 = 36ull + l_qname;
  const bool ok = hdr_ok && cig0 + 4ull * n_cig <= len;
  unsigned long long rl = 0;
  if (ok)
    for (uint32_t i = sub; i < n_cig; i += 16) {
      const uint32_t c = ix_rd32(p + cig0 + 4ull * i);
      if ((0x18Du >> (c & 15u)) & 1u) rl += c >> 4;  // M D N = X consume the reference
    }
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) rl += __shfl_xor(rl, d, 16);
  if (sub != 0) return;
  uint32_t bad = ok ? 0u : IX_E_MALFORMED;
  // (64 bits up to the packing below: pos = 2^31 - 1 with 1M ends on 2^31, which still fits the low word of tid << 32 | end)
  const uint64_t end = (uint64_t)(uint32_t)pos + (rl ? rl : 1ull);
  const uint64_t max_end = fmt ? 1ull << (14 + 3 * (fmt - 1)) : IX_MAX_END;  // fmt: tbk_ix_opts.reserved (0 BAI, k CSI of depth k - 1)
  if (ok && (tid < 0 || (uint32_t)tid >= n_ref || pos < 0 || end > max_end)) bad |= IX_E_RANGE;
  if (!bad && ((end - 1) >> 14) >= base[tid + 1] - base[tid]) bad |= IX_E_RANGE;  // (ends behind its reference's last window)
  if (bad) {
    atomicOr(err, bad);
    key[g] = 0, tend[g] = 0;
  } else {
    key[g] = (uint64_t)(uint32_t)tid << 32 | (fmt ? ix_reg2bin_depth((uint64_t)(uint32_t)pos, end, fmt - 1) : ix_reg2bin((uint32_t)pos, (uint32_t)end));
    tend[g] = (uint64_t)(uint32_t)tid << 32 | end;
  }
  // the record's member: the last m < nmem with cut[m] <= o (an empty member shares its cut with the next one, which wins)
  uint32_t lo = 0, hi = nmem;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (cut[mid] <= o) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t m = lo ? lo - 1 : 0;  // (cut[0] == 0: lo >= 1)
  vbeg[g] = moff[m] << 16 | ((o - cut[m]) & 0xffffull);
}

// The front end of a track's index (tbk_track_bgzf): one thread per row of the run, the row in the place of ix_rec_k's
// record — beg = start, end = max(end, start + 1), the same bins; the line's offset in the run's text (its offset in the track's text,
// less the run's first line's, plus the header bytes before it) bisects the member cuts for its vbeg.  A row is compared with the row
// before it in the TRACK (not only in the run): tids must not decrease, starts must not decrease within a tid.
__global__ __launch_bounds__(256) void tx_rec_k(uint32_t n, uint32_t first, const int32_t* __restrict__ r_tid, const int32_t* __restrict__ r_start,
                                                const int32_t* __restrict__ r_end, const uint64_t* __restrict__ off, uint64_t text0, uint32_t nmem,
                                                const uint64_t* __restrict__ cut, const uint64_t* __restrict__ moff, uint64_t ztotal, uint32_t n_ref,
                                                const uint64_t* __restrict__ base, uint32_t fmt, uint64_t* __restrict__ key, uint64_t* __restrict__ tend,
                                                uint64_t* __restrict__ vbeg, uint32_t* __restrict__ err) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n) return;
  if (g == n) {
    vbeg[n] = ztotal << 16;
    return;
  }
  const uint32_t i = first + g;
  const int32_t tid = r_tid[i], beg = r_start[i];
  const int64_t e = max((int64_t)r_end[i], (int64_t)beg + 1);
  const uint64_t max_end = fmt ? 1ull << (14 + 3 * (fmt - 1)) : IX_MAX_END;  // fmt: tbk_ix_opts.reserved (0 BAI, k CSI of depth k - 1)
  uint32_t bad = 0;
  if (tid < 0 || (uint32_t)tid >= n_ref || beg < 0 || (uint64_t)e > max_end) bad |= IX_E_RANGE;
  const uint64_t end = (uint64_t)e;
  if (!bad && ((end - 1) >> 14) >= base[tid + 1] - base[tid]) bad |= IX_E_RANGE;  // (ends behind its reference's last window)
  if (i) {
    const int32_t tp = r_tid[i - 1];
    if (tp > tid || (tp == tid && r_start[i - 1] > beg)) bad |= IX_E_UNSORTED;
  }
  if (bad) {
    atomicOr(err, bad);
    key[g] = 0, tend[g] = 0;
  } else {
    key[g] = (uint64_t)(uint32_t)tid << 32 | (fmt ? ix_reg2bin_depth((uint64_t)(uint32_t)beg, end, fmt - 1) : ix_reg2bin((uint32_t)beg, (uint32_t)end));
    tend[g] = (uint64_t)(uint32_t)tid << 32 | end;
  }
  // the line's member: the last m < nmem with cut[m] <= o (row 0 lies behind the header)
  const uint64_t o = off[i] - off[first] + text0;
  uint32_t lo = 0, hi = nmem;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (cut[mid] <= o) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t m = lo ? lo - 1 : 0;  // (cut[0] == 0: lo >= 1)
  vbeg[g] = moff[m] << 16 | ((o - cut[m]) & 0xffffull);
}

__global__ __launch_bounds__(256) void ix_head_k(uint32_t n, const uint64_t* __restrict__ key, uint32_t* __restrict__ head, uint32_t* __restrict__ err) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n) return;
  if (g == n) {
    head[n] = 0;
    return;
  }
  const uint64_t k = key[g];
  uint32_t h = 1;
  if (g) {
    const uint64_t kp = key[g - 1];
    h = k != kp;
    if ((k >> 32) < (kp >> 32)) atomicOr(err, IX_E_UNSORTED);
  }
  head[g] = h;
}

struct IxMax {  // scan element: running maximum of a 64-bit word (two 32-bit halves)
  uint32_t h, l;
};
struct IxMaxOp {
  __device__ __forceinline__ IxMax operator()(const IxMax& a, const IxMax& b) const {
    const uint64_t x = ((uint64_t)a.h << 32) | a.l, y = ((uint64_t)b.h << 32) | b.l;
    return y > x ? b : a;
  }
};
struct IxMaxLoad {
  const uint64_t* tend;
  __device__ __forceinline__ IxMax operator()(uint32_t g) const {
    const uint64_t t = tend[g];
    return IxMax{(uint32_t)(t >> 32), (uint32_t)t};
  }
};
struct IxMaxStore {
  uint64_t* M;
  __device__ __forceinline__ void operator()(uint32_t g, const IxMax&, const IxMax& inc, const IxMax&) const { M[g] = ((uint64_t)inc.h << 32) | inc.l; }
};

// sc[5] = the run's first refID, sc[6] = M[n - 1] (its last refID and the farthest end there)
__global__ __launch_bounds__(256) void ix_runs_k(uint32_t n, const uint64_t* __restrict__ key, const uint64_t* __restrict__ vbeg, const uint32_t* __restrict__ head,
                                                 const uint32_t* __restrict__ ex, const uint64_t* __restrict__ M, uint64_t* __restrict__ hi, uint64_t* __restrict__ lo,
                                                 uint32_t* __restrict__ val, uint64_t* __restrict__ rend, uint64_t* __restrict__ sc) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint32_t h = head[g], r = ex[g] + h - 1;  // (head[0] == 1: r >= 0)
  if (h) hi[r] = key[g], lo[r] = vbeg[g], val[r] = r;
  if (head[g + 1] || g + 1 == n) rend[r] = vbeg[g + 1];
  if (g == 0) sc[5] = key[0] >> 32;
  if (g + 1 == n) sc[6] = M[g];
}

// sorted run j starts a chunk unless it continues its bin in the member where the chunk before it ends (htslib's compress_binning)
__global__ __launch_bounds__(256) void ix_mhead_k(uint32_t R, const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, const uint32_t* __restrict__ val,
                                                  const uint64_t* __restrict__ rend, uint64_t* __restrict__ esorted, uint32_t* __restrict__ mh) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > R) return;
  if (j == R) {
    mh[R] = 0;
    return;
  }
  esorted[j] = rend[val[j]];
  mh[j] = j == 0 || hi[j] != hi[j - 1] || (rend[val[j - 1]] >> 16) < (lo[j] >> 16);
}
__global__ __launch_bounds__(256) void ix_chunks_k(uint32_t R, const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ esorted,
                                                   const uint32_t* __restrict__ mh, const uint32_t* __restrict__ mex, tbk_ix_chunk* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  const uint32_t h = mh[j], c = mex[j] + h - 1;
  if (h) out[c].tid = (int32_t)(hi[j] >> 32), out[c].bin = (uint32_t)hi[j], out[c].beg = lo[j];
  if (mh[j + 1] || j + 1 == R) out[c].end = esorted[j];
}

// first g in [0, n) with M[g] > x (n: none); M does not decrease
__device__ __forceinline__ uint32_t ix_first_above(const uint64_t* __restrict__ M, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (M[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void ix_lin_k(uint64_t n_lin, uint64_t lin_first, uint32_t n_ref, const uint64_t* __restrict__ base, uint32_t n,
                                                const uint64_t* __restrict__ M, const uint64_t* __restrict__ vbeg, uint64_t* __restrict__ lin) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_lin) return;
  const uint64_t f = lin_first + i;
  uint32_t lo = 0, hi = n_ref;  // the last t < n_ref with base[t] <= f
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (base[mid] <= f) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t t = lo ? lo - 1 : 0, w = f - base[t];
  const uint32_t g = ix_first_above(M, n, t << 32 | w << 14);
  lin[i] = (g < n && (M[g] >> 32) == t) ? vbeg[g] : ~0ull;
}
__global__ __launch_bounds__(256) void ix_refs_k(uint32_t n_t, uint32_t tid_first, uint32_t n, const uint64_t* __restrict__ M, const uint64_t* __restrict__ vbeg,
                                                 tbk_ix_ref* __restrict__ refs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_t) return;
  const uint64_t t = (uint64_t)tid_first + i;
  const uint32_t a = t ? ix_first_above(M, n, (t << 32) - 1) : 0u, b = ix_first_above(M, n, ((t + 1) << 32) - 1);
  tbk_ix_ref r;
  r.tid = (int32_t)t, r.reserved = 0, r.n_records = b - a, r.first = b > a ? vbeg[a] : 0, r.last = b > a ? vbeg[b] : 0;
  refs[i] = r;
}

struct IxHost {  // the part's pinned host arrays: owned by the context
  uint8_t* p = nullptr;
  size_t cap = 0;
};
int ix_host(tbk_ctx* ctx, size_t bytes, uint8_t** out) {
  IxHost* H = (IxHost*)ctx->ix;
  if (!H) ctx->ix = H = new IxHost();
  if (bytes > H->cap) {
    if (H->p) (void)hipHostFree(H->p);
    H->p = nullptr, H->cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc((void**)&H->p, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return TBK_ENOMEM;
    }
    H->cap = want;
  }
  *out = H->p;
  return 0;
}

}  // namespace

void tbk_ix_free(tbk_ctx* ctx) {
  IxHost* H = (IxHost*)ctx->ix;
  if (!H) return;
  if (H->p) (void)hipHostFree(H->p);
  delete H;
  ctx->ix = nullptr;
}

int tbk_ix_check_opts(tbk_ctx* ctx, const tbk_ix_opts* ix) {
  if (!ix || (ix->n_ref && !ix->ref_len) || ix->n_ref >= (1u << 31)) return TBK_EINVAL;
  if (ix->reserved) {  // CSI of depth reserved - 1
    const uint32_t depth = ix->reserved - 1;
    if (depth > IX_MAX_DEPTH) {
      ctx->last_error = "bam_encode_indexed: CSI depth " + std::to_string(depth) + " is above " + std::to_string(IX_MAX_DEPTH);
      return TBK_EINVAL;
    }
    for (uint32_t t = 0; t < ix->n_ref; ++t)
      if (ix->ref_len[t] > (1ull << (14 + 3 * depth))) {
        ctx->last_error = "bam_encode_indexed: reference " + std::to_string(t) + " is longer than 2^" + std::to_string(14 + 3 * depth) + ": a CSI of depth " +
                          std::to_string(depth) + " cannot address it";
        return TBK_EINVAL;
      }
    return 0;
  }
  for (uint32_t t = 0; t < ix->n_ref; ++t)
    if (ix->ref_len[t] > IX_MAX_END) {
      ctx->last_error = "bam_encode_indexed: reference " + std::to_string(t) + " is longer than 2^29: a BAI cannot address it";
      return TBK_EINVAL;
    }
  return 0;
}

namespace {
// what a front end (ix_rec_k for records, tx_rec_k for track rows) fills and the back half reads
struct IxFront {
  uint32_t n = 0;
  std::vector<uint64_t> base;  // [n_ref + 1] flat window of every reference's window 0
  size_t base_bytes = 0;
  uint64_t *d_base = nullptr, *key = nullptr, *tend = nullptr, *M = nullptr, *vbeg = nullptr, *rend = nullptr;
  uint32_t *head = nullptr, *ex = nullptr;
  SortBufs sb;
};

// the front half up to the launch of the front end's kernel.  fresh_arena: the arena starts over (the encoder's path); else the arrays
// go behind what the arena holds
int ix_front(tbk_ctx* ctx, uint32_t n, const tbk_ix_opts* ix, bool fresh_arena, IxFront& F) {
  const uint32_t n_ref = ix->n_ref;
  hipStream_t st = ctx->stream;
  F.n = n;
  std::vector<uint64_t>& base = F.base;
  base.assign((size_t)n_ref + 1, 0);
  for (uint32_t t = 0; t < n_ref; ++t) base[t + 1] = base[t] + (((uint64_t)ix->ref_len[t] + 16383) >> 14);
  const size_t base_bytes = F.base_bytes = (((size_t)n_ref + 1) * 8 + 255) & ~(size_t)255;
  // (the encoder's kernels have run and its scans' partial sums are dead: the arena starts over)
  if (fresh_arena) TBK_TRY(tbk_ws_reserve(ctx, (size_t)n * 140 + base[n_ref] * 8 + (size_t)n_ref * 48 + tbk_radix_ws_bytes(n) + ((size_t)2 << 20)));
  uint8_t* hp;
  TBK_TRY(ix_host(ctx, base_bytes, &hp));
  memcpy(hp, base.data(), ((size_t)n_ref + 1) * 8);
  uint64_t* d_base = F.d_base = ws_alloc<uint64_t>(ctx, (size_t)n_ref + 1);
  uint64_t* key = F.key = ws_alloc<uint64_t>(ctx, n);
  uint64_t* tend = F.tend = ws_alloc<uint64_t>(ctx, n);
  uint64_t* M = F.M = ws_alloc<uint64_t>(ctx, n);
  uint64_t* vbeg = F.vbeg = ws_alloc<uint64_t>(ctx, (size_t)n + 1);
  uint32_t* head = F.head = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint32_t* ex = F.ex = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  SortBufs& sb = F.sb;
  sb.hi = ws_alloc<uint64_t>(ctx, n), sb.lo = ws_alloc<uint64_t>(ctx, n), sb.val = ws_alloc<uint32_t>(ctx, n);
  uint64_t* rend = F.rend = ws_alloc<uint64_t>(ctx, n);
  if (!d_base || !key || !tend || !M || !vbeg || !head || !ex || !sb.hi || !sb.lo || !sb.val || !rend) return TBK_ENOMEM;
  TBK_HIP(hipMemcpyAsync(d_base, hp, ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, st));
  uint64_t* sc = ctx->d_scalars;
  TBK_HIP(hipMemsetAsync(sc, 0, 16 * sizeof(uint64_t), st));
  return 0;
}

// the back half: everything from ix_head_k on.  track: the rows of tbk_track_bgzf stand in the records' place (the messages say so)
int ix_back(tbk_ctx* ctx, IxFront& F, const tbk_ix_opts* ix, uint64_t ztotal, bool track, tbk_ix_part* part) {
  const uint32_t n = F.n, n_ref = ix->n_ref;
  hipStream_t st = ctx->stream;
  const std::vector<uint64_t>& base = F.base;
  const size_t base_bytes = F.base_bytes;
  uint64_t *d_base = F.d_base, *key = F.key, *tend = F.tend, *M = F.M, *vbeg = F.vbeg, *rend = F.rend;
  uint32_t *head = F.head, *ex = F.ex;
  SortBufs& sb = F.sb;
  uint64_t* sc = ctx->d_scalars;
  uint8_t* hp;
  TBK_LAUNCH(ctx, "ix_head", ix_head_k, cdiv((uint64_t)n + 1, 256), 256, 0, n, key, head, ctx->d_err);
  TBK_TRY(tbk_exscan_u32(ctx, head, ex, n + 1, sc + 4));
  TBK_TRY((scan_op_run<IxMax, IxMaxOp, IxMaxLoad, IxMaxStore>(ctx, "ix_max_scan", n, IxMaxLoad{tend}, IxMaxStore{M}, IxMaxOp{}, IxMax{0u, 0u})));
  TBK_LAUNCH(ctx, "ix_runs", ix_runs_k, cdiv(n, 256), 256, 0, n, key, vbeg, head, ex, M, sb.hi, sb.lo, sb.val, rend, sc);
  uint32_t eb = 0;
  TBK_TRY(tbk_sync_err(ctx, &eb));  // (the run count sizes the sort, the reference range the two tables)
  if (eb) {
    if (track) {
      ctx->last_error = (eb & IX_E_RANGE) ? "track_bgzf: a row outside what the index addresses (tid not below n_ref, negative start, or an end beyond the "
                                            "format's reach or its reference's last window)"
                        : (eb & IX_E_UNSORTED) ? "track_bgzf: the rows are not sorted (a tid decreases, or a start decreases within a tid)"
                                               : "track_bgzf: device error";
      return (eb & (IX_E_RANGE | IX_E_UNSORTED)) ? TBK_EINVAL : TBK_EHIP;
    }
    ctx->last_error = (eb & IX_E_MALFORMED)  ? "bam_encode_indexed: a malformed record"
                      : (eb & IX_E_RANGE)    ? (ix->reserved ? "bam_encode_indexed: a record outside what the CSI addresses (refID not in the header, negative pos, or an end "
                                                               "beyond 2^(14 + 3 * depth) or its reference)"
                                                             : "bam_encode_indexed: a record outside what a BAI addresses (refID not in the header, negative pos, or an end beyond 2^29 "
                                                               "or its reference)")
                      : (eb & IX_E_UNSORTED) ? "bam_encode_indexed: the records' refIDs decrease"
                                             : "bam_encode_indexed: device error";
    return (eb & (IX_E_MALFORMED | IX_E_RANGE | IX_E_UNSORTED)) ? TBK_EINVAL : TBK_EHIP;
  }
  const uint32_t R = (uint32_t)ctx->h_scalars[4];
  const uint32_t tid_first = (uint32_t)ctx->h_scalars[5], tid_last = (uint32_t)(ctx->h_scalars[6] >> 32);
  const uint64_t max_end = ctx->h_scalars[6] & 0xffffffffull;
  if (R == 0 || R > n || tid_last >= n_ref || tid_first > tid_last || max_end == 0) {
    ctx->last_error = track ? "track_bgzf: inconsistent run table" : "bam_encode_indexed: inconsistent run table";
    return TBK_EHIP;
  }
  const uint32_t n_t = tid_last - tid_first + 1;
  const uint64_t lin_first = base[tid_first], n_lin = base[tid_last] + ((max_end - 1) >> 14) + 1 - lin_first;
  sb.hi2 = ws_alloc<uint64_t>(ctx, R), sb.lo2 = ws_alloc<uint64_t>(ctx, R), sb.val2 = ws_alloc<uint32_t>(ctx, R);
  uint64_t* esorted = ws_alloc<uint64_t>(ctx, R);
  uint32_t* mh = ws_alloc<uint32_t>(ctx, (size_t)R + 1);
  uint32_t* mex = ws_alloc<uint32_t>(ctx, (size_t)R + 1);
  tbk_ix_chunk* d_chunks = ws_alloc<tbk_ix_chunk>(ctx, R);
  uint64_t* d_lin = ws_alloc<uint64_t>(ctx, n_lin);
  tbk_ix_ref* d_refs = ws_alloc<tbk_ix_ref>(ctx, n_t);
  if (!sb.hi2 || !sb.lo2 || !sb.val2 || !esorted || !mh || !mex || !d_chunks || !d_lin || !d_refs) return TBK_ENOMEM;
  // the bits that can differ: refIDs below n_ref, bins below 2^16 (a CSI of depth 6: below (8^7 - 1) / 7 = 299593, 19 bits), virtual offsets
  // below the run's end (a shallow CSI keeps the BAI's 16 bin bits: the same passes)
  auto bits_below = [](uint64_t x) {
    uint64_t m = 0;
    while (m < x) m = m << 1 | 1;
    return m;
  };
  const uint64_t n_bins = ix->reserved ? ((1ull << (3 * ix->reserved)) - 1) / 7 : 37449;
  TBK_TRY(tbk_radix_sort128(ctx, &sb, R, bits_below(n_ref) << 32 | bits_below(n_bins) | 0xffffull, bits_below(ztotal) << 16 | 0xffffull, true));
  TBK_LAUNCH(ctx, "ix_mhead", ix_mhead_k, cdiv((uint64_t)R + 1, 256), 256, 0, R, sb.hi, sb.lo, sb.val, rend, esorted, mh);
  TBK_TRY(tbk_exscan_u32(ctx, mh, mex, R + 1, sc + 7));
  TBK_LAUNCH(ctx, "ix_chunks", ix_chunks_k, cdiv(R, 256), 256, 0, R, sb.hi, sb.lo, esorted, mh, mex, d_chunks);
  TBK_LAUNCH(ctx, "ix_lin", ix_lin_k, cdiv(n_lin, 256), 256, 0, n_lin, lin_first, n_ref, d_base, n, M, vbeg, d_lin);
  TBK_LAUNCH(ctx, "ix_refs", ix_refs_k, cdiv(n_t, 256), 256, 0, n_t, tid_first, n, M, vbeg, d_refs);
  // one download behind the members': at most R chunks (the merged count comes with the same synchronisation)
  const size_t ch_bytes = ((size_t)R * sizeof(tbk_ix_chunk) + 255) & ~(size_t)255, lin_bytes = ((size_t)n_lin * 8 + 255) & ~(size_t)255;
  TBK_TRY(ix_host(ctx, base_bytes + ch_bytes + lin_bytes + (size_t)n_t * sizeof(tbk_ix_ref), &hp));  // (the base table has been uploaded: d_base is read from now on)
  tbk_ix_chunk* h_chunks = (tbk_ix_chunk*)(hp + base_bytes);
  uint64_t* h_lin = (uint64_t*)(hp + base_bytes + ch_bytes);
  tbk_ix_ref* h_refs = (tbk_ix_ref*)(hp + base_bytes + ch_bytes + lin_bytes);
  TBK_HIP(hipMemcpyAsync(h_chunks, d_chunks, (size_t)R * sizeof(tbk_ix_chunk), hipMemcpyDeviceToHost, st));
  TBK_HIP(hipMemcpyAsync(h_lin, d_lin, (size_t)n_lin * 8, hipMemcpyDeviceToHost, st));
  TBK_HIP(hipMemcpyAsync(h_refs, d_refs, (size_t)n_t * sizeof(tbk_ix_ref), hipMemcpyDeviceToHost, st));
  if (ix->rec_vbeg) TBK_HIP(hipMemcpyAsync(ix->rec_vbeg, vbeg, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
  TBK_TRY(tbk_sync_err(ctx, &eb));
  if (eb) {
    ctx->last_error = track ? "track_bgzf: device error in the index kernels" : "bam_encode_indexed: device error in the index kernels";
    return TBK_EHIP;
  }
  uint32_t nr = 0;
  for (uint32_t i = 0; i < n_t; ++i)
    if (h_refs[i].n_records) h_refs[nr++] = h_refs[i];
  part->n_chunks = (uint32_t)ctx->h_scalars[7];
  part->n_refs = nr;
  part->n_lin = n_lin;
  part->lin_first = lin_first;
  part->chunks = h_chunks, part->lin = h_lin, part->refs = h_refs;
  return tbk_check_launch(ctx, track ? "track_bgzf" : "bam_encode_indexed");
}
}  // namespace

size_t tbk_ix_ws_bytes(uint32_t n, const tbk_ix_opts* ix) {
  uint64_t windows = 0;
  for (uint32_t t = 0; t < ix->n_ref; ++t) windows += ((uint64_t)ix->ref_len[t] + 16383) >> 14;
  return (size_t)n * 140 + windows * 8 + (size_t)ix->n_ref * 48 + tbk_radix_ws_bytes(n) + ((size_t)2 << 20);
}

int tbk_ix_build(tbk_ctx* ctx, const TbkIxIn& I, const tbk_ix_opts* ix, tbk_ix_part* part) {
  memset(part, 0, sizeof(*part));
  const uint32_t n = I.n, n_ref = ix->n_ref;
  if (n == 0) return 0;
  IxFront F;
  TBK_TRY(ix_front(ctx, n, ix, true, F));
  TBK_LAUNCH(ctx, "ix_rec", ix_rec_k, cdiv(((uint64_t)n + 1) * 16, 256), 256, 0, n, I.pay, I.ooff, I.nmem, I.cut, I.moff, I.ztotal, n_ref, F.d_base, ix->reserved, F.key, F.tend,
             F.vbeg, ctx->d_err);
  return ix_back(ctx, F, ix, I.ztotal, false, part);
}

int tbk_tx_build(tbk_ctx* ctx, const TbkTxIn& I, const tbk_ix_opts* ix, tbk_ix_part* part) {
  memset(part, 0, sizeof(*part));
  const uint32_t n = I.n, n_ref = ix->n_ref;
  if (n == 0) return 0;
  IxFront F;
  TBK_TRY(ix_front(ctx, n, ix, false, F));
  TBK_LAUNCH(ctx, "tx_rec", tx_rec_k, cdiv((uint64_t)n + 1, 256), 256, 0, n, I.first, I.tid, I.start, I.end, I.off, I.text0, I.nmem, I.cut, I.moff, I.ztotal, n_ref, F.d_base,
             ix->reserved, F.key, F.tend, F.vbeg, ctx->d_err);
  return ix_back(ctx, F, ix, I.ztotal, true, part);
}
