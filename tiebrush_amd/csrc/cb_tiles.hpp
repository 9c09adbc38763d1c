// cb_tiles.hpp — the bundle monoid of tiecov's lean passes over 4096-record tiles and the hand-over of per-tile results to the block
// that finishes last (cov.hip: cb_agg_k, cl_heads_k; collapse.hip: the view builder, which folds the tile aggregates while it has
// every group's reference and end in registers).
#pragma once
#include "dev_common.hpp"
#include "scan_op.hpp"

struct CbAgg {
  int32_t first_tid, last_tid;  // last_tid == INT32_MIN: no record
  int32_t mx;                   // maximum end over the trailing records that share last_tid
  uint32_t whole;               // every record shares one tid
};
struct CbOp {
  __device__ __forceinline__ CbAgg operator()(const CbAgg& a, const CbAgg& b) const {
    if (b.last_tid == INT32_MIN) return a;
    if (a.last_tid == INT32_MIN) return b;
    CbAgg r;
    r.first_tid = a.first_tid;
    r.last_tid = b.last_tid;
    const bool joins = b.whole && b.first_tid == a.last_tid;
    r.mx = joins ? (a.mx > b.mx ? a.mx : b.mx) : b.mx;
    r.whole = joins ? a.whole : 0u;
    return r;
  }
};
// Whether a record on `tid` that starts at `start` (1-based) opens a bundle, given the aggregate of the records before it: the first
// record of a tid run, or a start beyond the running maximum of end over the run so far (tiecov.cpp:443).  The one statement of the
// rule for every walk that looks for heads (cov.hip: cb_heads_k, cl_heads_k; stream.hip: st_heads_k).
__device__ __forceinline__ bool cb_is_head(const CbAgg& before, int32_t tid, int32_t start) {
  return before.last_tid == INT32_MIN || tid != before.last_tid || start > before.mx;
}
constexpr uint32_t CB_NT = 256, CB_ROWS = 4, CB_TILE = CB_NT * 4 * CB_ROWS;
// four consecutive records of a thread from a column of m: one 16-byte load inside the column, element by element (`fill` behind it) at its end
__device__ __forceinline__ void cb_load4(const int32_t* __restrict__ a, uint64_t i, uint32_t m, int32_t fill, int32_t v[4]) {
  if (i + 3 < m) {
    const int4 q = *reinterpret_cast<const int4*>(a + i);  // (i is a multiple of 4, the arrays 256-byte aligned)
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < m ? a[i + e] : fill;
  }
}
template <class T, class Op>
__device__ __forceinline__ T wave_incl_scan_op(T v, Op op) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_t(v, d);
    if ((int)lane_id() >= d) v = op(o, v);
  }
  return v;
}
// True in every thread of the block that finishes last; `done` starts at zero.  What the blocks hand to the last one travels without
// fences: thread 0 writes its block's result with agent-scope stores (cb_put), waits for them to be acknowledged and counts the block;
// the last block reads the results with agent-scope loads (cb_get).  (A __threadfence per block writes back and invalidates L2: with
// 6 k blocks it made this pass — and the junction kernels beside it — five times slower.)
__device__ __forceinline__ void cb_put(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t cb_get(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint4 cb_get4(const uint4* p) {
  const uint64_t a = cb_get(reinterpret_cast<const uint64_t*>(p)), b = cb_get(reinterpret_cast<const uint64_t*>(p) + 1);
  return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}
__device__ __forceinline__ bool cb_last_block(uint32_t* __restrict__ done) {  // (called behind thread 0's cb_put's)
  __shared__ uint32_t s_last;
  if (threadIdx.x == 0) {
    // The block is counted BEHIND its results: they are write-through stores (agent scope), so what orders them before the counter is
    // the wait for their acknowledgement — stated explicitly: a workgroup-scope release fence compiles to no wait at all here (the
    // counter could pass the results, and the last block scan entries that were not there yet), an agent-scope release to an L2
    // write-back per block (buffer_wbl2: 0.37 -> 0.69 ms for the two passes, and the junction kernels beside them as much slower).
    __builtin_amdgcn_s_waitcnt(TBK_WAIT_VMCNT0);  // vmcnt(0): on gfx9 stores count there too
    __asm__ volatile("" ::: "memory");
    s_last = atomicAdd(done, 1u) == gridDim.x - 1u ? 1u : 0u;
  }
  __syncthreads();
  return s_last != 0u;
}
// The tile aggregates -> for every tile the aggregate of the tiles before it, by ONE block of NT threads: a slice of the tiles per
// thread with eight loads in flight at a time, the slices' aggregates by wave scans and one fold of the wave totals.  It runs in the
// block of cb_agg_k that finishes last (cb_last_block): as a kernel of its own between the passes — one block — it waited for a CU
// with room while the junction branch's grids filled the GPU (100-200 us of a 1.4 ms coverage call, whatever the streams' priorities).
template <uint32_t NT>
__device__ __forceinline__ void cb_spine_block(uint4* __restrict__ part, uint32_t ntiles, CbAgg* wl /* [NT / 64] */) {
  const CbOp op{};
  const CbAgg none{0, INT32_MIN, INT32_MIN, 1u};
  auto un = [](const uint4& v) { return CbAgg{(int32_t)v.x, (int32_t)v.y, (int32_t)v.z, v.w}; };
  auto pk = [](const CbAgg& a) { return make_uint4((uint32_t)a.first_tid, (uint32_t)a.last_tid, (uint32_t)a.mx, a.whole); };
  const uint4 none4 = pk(none);
  const uint32_t per = (ntiles + NT - 1u) / NT, i0 = threadIdx.x * per, i1 = i0 + per < ntiles ? i0 + per : ntiles;
  CbAgg a = none;
  for (uint32_t q0 = i0; q0 < i1; q0 += 8u) {
    uint4 v8[8];
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) v8[u] = q0 + u < i1 ? cb_get4(part + q0 + u) : none4;
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) a = op(a, un(v8[u]));
  }
  const CbAgg inc = wave_incl_scan_op(a, op);
  if (lane_id() == 63) wl[threadIdx.x >> 6] = inc;
  CbAgg run = shfl_up_t(inc, 1);
  __syncthreads();  // (every slice has been read: the writes below may begin)
  {
    CbAgg acc = none;
    const uint32_t wv = threadIdx.x >> 6;
    for (uint32_t q = 0; q < wv; ++q) acc = op(acc, wl[q]);
    run = lane_id() == 0 ? acc : op(acc, run);
  }
  for (uint32_t q0 = i0; q0 < i1; q0 += 8u) {
    uint4 v8[8];
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) v8[u] = q0 + u < i1 ? cb_get4(part + q0 + u) : none4;
#pragma unroll
    for (uint32_t u = 0; u < 8u; ++u) {
      if (q0 + u < i1) part[q0 + u] = pk(run);
      run = op(run, un(v8[u]));
    }
  }
}
