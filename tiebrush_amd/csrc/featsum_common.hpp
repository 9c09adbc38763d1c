// featsum_common.hpp — what the two readers of coverage rows against features share: tbk_cov_summary (featsum.hip) and
// tbk_cov_thresholds (depththr.hip, §4l) — and tbk_tx_summary (txsum.hip, §4m), which reads them against exons and introns.  The tile
// constants, the rows and features as kernels take them, the order check, the 64-ary search, the butterfly fold, the walk of one
// feature's run of rows and its junction lookup (fs_cov_part, fs_junc_part: what fs_feat_k and tx_part_k both call), and the host
// helpers that bring a caller's arrays to the device and the columns back.  Every translation unit gets its own copy (anonymous
// namespace): the kernels of one never call into the other.
#pragma once
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

// *bad |= 1 for interval rows that are not sorted and disjoint, |= 2 for junction rows out of order (read back: TBK_EINVAL)
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

// the aggregates fs_tile_k makes, one element per tile of FS_TILE interval rows
struct FsAgg {
  double *sum, *max;
  uint64_t* len;
};

// one wave per tile: each lane its rows in order, then the butterfly — an order that depends on the tile alone
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

// The coverage part of one feature [fb, fe) on ft, by the whole wave (R.ni > 0): the run [lo, hi) of its rows by two searches, a run of up
// to FS_DIRECT rows walked lane-strided with every row cut to the feature, a longer one as the rows up to the first tile boundary behind
// lo, the aggregates of the whole tiles and the rows of the last tile; then the butterfly.  Every lane returns the sum of val x bases,
// the bases and the largest value (-inf without a row).
__device__ __forceinline__ void fs_cov_part(const FsRows& R, const FsAgg& A, int32_t ft, int64_t fb, int64_t fe, double& s, uint64_t& c, double& m) {
  const uint32_t lane = lane_id();
  s = 0.0, m = -__builtin_inf(), c = 0;
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

// The junction rows that ARE [fb, fe) on ft under the strand `want` ('.': every strand), by the whole wave (R.nj > 0): one search, then
// lane 0 adds their values in row order.  Lane 0 returns the sum; the other lanes 0.
__device__ __forceinline__ double fs_junc_part(const FsRows& R, int32_t ft, int64_t fb, int64_t fe, uint8_t want) {
  uint32_t i = fs_search(0, R.nj, [&](uint32_t k) {
    const int32_t t = R.jtid[k];
    if (t != ft) return t > ft;
    const int64_t js = R.jstart[k];
    return js > fb || (js == fb && (int64_t)R.jend[k] >= fe);
  });
  double j = 0.0;
  if (lane_id() == 0)
    for (; i < R.nj && R.jtid[i] == ft && (int64_t)R.jstart[i] == fb && (int64_t)R.jend[i] == fe; ++i)
      if (want == '.' || R.jstrand[i] == want) j += R.jval[i];
  return j;
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

// the order check of the rows a call reads (interval rows alone with R.nj == 0): 0, or TBK_EINVAL with the sentence in last_error
inline int fs_check_order(tbk_ctx* ctx, const FsRows& R, const char* who) {
  if (!R.ni && !R.nj) return 0;
  uint32_t* bad = ws_alloc<uint32_t>(ctx, 1);
  if (!bad) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(bad, 0, 4, ctx->stream));
  TBK_LAUNCH(ctx, "featsum_order", fs_order_k, cdiv(R.ni > R.nj ? R.ni : R.nj, FS_NT), FS_NT, 0, R, bad);
  uint32_t res = 0;
  TBK_HIP(hipMemcpyAsync(&res, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  if (res) {
    ctx->last_error = std::string(who) + ((res & 1u) ? ": interval rows are not sorted by reference and start, or overlap"
                                                     : ": junction rows are not sorted by reference, start, end and strand");
    return TBK_EINVAL;
  }
  return 0;
}

}  // namespace
