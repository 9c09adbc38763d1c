// prims_probe.hip — test infrastructure only: C entry points that run the library's device-wide primitives (the exclusive scans, the
// two radix sorts, the run sort, the scan engine in its three forms and the two-scan kernel) on a context made by tbk_create, with
// nothing else around them, so that tests/test_gpu_prims.py can put them on their own edges and compare with numpy.
// Built by tiebrush_amd/csrc/Makefile into tiebrush_amd/_build/libtbk_probe.so, linked against libtbk.so; libtbk.so neither knows
// of it nor exports anything for it (the primitives are ordinary C++ symbols of the library already).
//
// Every entry: reserve the arena, run the primitive on ctx->stream, synchronise that stream, return the primitive's status (and the
// device error word where the primitive can raise one).  All pointers are device memory unless a name ends in _host.
#include "dev_common.hpp"
#include "tbk_internal.h"
#include "scan_op.hpp"
#include "rx_w64.hpp"

namespace {
// the brackets of an API call for the per-kernel event timing: tbk_kernel_times then names what a probe call launched, and how often
struct Call {
  tbk_ctx* ctx;
  explicit Call(tbk_ctx* c) : ctx(c) { tbk_prof_begin_call(c); }
  ~Call() { tbk_prof_end_call(ctx); }
};
int clear_derr(tbk_ctx* ctx) {
  TBK_HIP(hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), ctx->stream));
  return 0;
}
int sync(tbk_ctx* ctx) {
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---- the scan engine's test operator ---------------------------------------------------------------------------------------
// A segmented sum over a POD of W 32-bit words: word 0 is a head flag, the others are W - 1 independent sums mod 2^32.
//   op(l, r) = r.flag ? r : {l.flag, l.s[k] + r.s[k]}
// Associative, not commutative (a flipped operand order anywhere gives another result) and exact.
// Widths: 2, and 5.  so_single_k / so_down_k keep a tile of SO_LDS = 2304 elements in static LDS: 2304 * 4 * W bytes, plus two
// arrays of 4 elements and a carry: W = 5 takes 46 080 + 184 bytes of the 65 536 a block may have (W = 7 would be the last
// that fits, at 64 512 + 256, and leaves the compiler nothing); a published value of 5 words is 5 granules that arrive one by one.
template <int W>
struct Seg {
  uint32_t flag;
  uint32_t s[W - 1];
};
template <int W>
struct SegOp {
  __device__ __forceinline__ Seg<W> operator()(const Seg<W>& l, const Seg<W>& r) const {
    if (r.flag) return r;
    Seg<W> o;
    o.flag = l.flag;
#pragma unroll
    for (int k = 0; k < W - 1; ++k) o.s[k] = l.s[k] + r.s[k];
    return o;
  }
};
template <int W>
__host__ __device__ __forceinline__ Seg<W> seg_ident() {
  Seg<W> z;
  z.flag = 0;
  for (int k = 0; k < W - 1; ++k) z.s[k] = 0;
  return z;
}
constexpr uint32_t PROBE_MAX_DELAY = 1000000u;  // 10 ms of the 100 MHz clock: three orders of magnitude below SO_SPIN_TICKS

// values are planar: word k of element i is value[k * n + i]; so are the outputs (word 0 = the flag, word k + 1 = sum k)
template <int W>
struct SegLoad {
  const uint32_t* flag;
  const uint32_t* value;
  uint32_t n, delay_index, delay_ticks;
  __device__ __forceinline__ Seg<W> operator()(uint32_t i) const {
    Seg<W> r;
    r.flag = flag[i] ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < W - 1; ++k) r.s[k] = value[(size_t)k * n + i];
    if (delay_ticks != 0 && i == delay_index) {  // a bounded wait of this one lane: the tile's aggregate is published that much later
      const unsigned long long t0 = wall_clock64();
      for (uint32_t it = 0; it < (1u << 22) && wall_clock64() - t0 < (unsigned long long)delay_ticks; ++it) __builtin_amdgcn_s_sleep(8);
    }
    return r;
  }
};
template <int W>
__device__ __forceinline__ void seg_put(uint32_t* out, uint32_t n, uint32_t i, const Seg<W>& v) {
  out[i] = v.flag;
#pragma unroll
  for (int k = 0; k < W - 1; ++k) out[(size_t)(k + 1) * n + i] = v.s[k];
}
template <int W>
struct SegStore {
  uint32_t *elem, *inc, *exc;
  uint32_t n;
  __device__ __forceinline__ void operator()(uint32_t i, const Seg<W>& e, const Seg<W>& in, const Seg<W>& ex) const {
    seg_put<W>(elem, n, i, e);
    seg_put<W>(inc, n, i, in);
    seg_put<W>(exc, n, i, ex);
  }
};

template <int W>
int run_scan(tbk_ctx* ctx, const uint32_t* flag, const uint32_t* value, uint32_t n, uint32_t delay_index, uint32_t delay_ticks, uint32_t* out_elem,
             uint32_t* out_inc, uint32_t* out_exc) {
  SegLoad<W> ld{flag, value, n, delay_index, delay_ticks};
  SegStore<W> st{out_elem, out_inc, out_exc, n};
  return scan_op_run<Seg<W>, SegOp<W>, SegLoad<W>, SegStore<W>>(ctx, "probe_scan", n, ld, st, SegOp<W>{}, seg_ident<W>(), false);
}

// ---- the two-scan kernel: first scan Seg<3>, second scan a count -------------------------------------------------------------
constexpr int W2S = 3;
struct TwoAux {
  const uint32_t* value;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return value[i]; }
};
struct TwoSecond {  // depends on the first scan's exclusive prefix: a wrong first prefix changes the second scan
  __device__ __forceinline__ uint32_t operator()(uint32_t i, const Seg<W2S>&, const Seg<W2S>&, const Seg<W2S>& ex, uint32_t) const {
    return (ex.s[0] + i) % 3u == 0u ? 1u : 0u;
  }
};
struct TwoStore {
  uint32_t *inc, *exc, *term, *before;
  uint32_t n;
  __device__ __forceinline__ void operator()(uint32_t i, const Seg<W2S>&, const Seg<W2S>& in, const Seg<W2S>& ex, uint32_t t, uint32_t tb, uint32_t) const {
    seg_put<W2S>(inc, n, i, in);
    seg_put<W2S>(exc, n, i, ex);
    term[i] = t;
    before[i] = tb;
  }
};
template <int E>
int run_scan_two(tbk_ctx* ctx, const uint32_t* flag, const uint32_t* value, uint32_t n, uint32_t* out_inc, uint32_t* out_exc, uint32_t* out_term,
                 uint32_t* out_before) {
  SegLoad<W2S> ld{flag, value, n, 0u, 0u};
  TwoStore st{out_inc, out_exc, out_term, out_before, n};
  return scan_two_run<E, Seg<W2S>, SegOp<W2S>, uint32_t, SoPlusU32, SegLoad<W2S>, TwoAux, TwoSecond, TwoStore>(
      ctx, "probe_scan_two", n, ld, TwoAux{value}, TwoSecond{}, st, SegOp<W2S>{}, seg_ident<W2S>(), SoPlusU32{}, 0u);
}

// ---- the emit functor of tbk_radix_sort_w64_emit ------------------------------------------------------------------------------
// calls[g] counts the calls for final position g (calls[n]: calls with a position outside the array), word[g] is what it was given
struct ProbeEmit {
  uint32_t* calls;
  uint64_t* word;
  uint32_t n;
  __device__ __forceinline__ void operator()(uint32_t g, uint64_t w) const {
    if (g < n) {
      atomicAdd(&calls[g], 1u);
      word[g] = w;
    } else {
      atomicAdd(&calls[n], 1u);
    }
  }
};
}  // namespace

extern "C" {

int probe_exscan(tbk_ctx* ctx, const uint32_t* in, void* out, uint32_t n, int out_is_u64, uint64_t* total_or_null) {
  Call call(ctx);
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)cdiv(n, 2048) * 8 + 65536));
  const int rc = out_is_u64 ? tbk_exscan_u32_u64(ctx, in, (uint64_t*)out, n, total_or_null) : tbk_exscan_u32(ctx, in, (uint32_t*)out, n, total_or_null);
  TBK_TRY(sync(ctx));
  return rc;
}

// sorts (hi, lo, val) in place: the second side of the buffers lives here
int probe_radix128(tbk_ctx* ctx, uint64_t* hi, uint64_t* lo, uint32_t* val, uint32_t n, uint64_t only_hi, uint64_t only_lo, int exact) {
  Call call(ctx);
  TBK_TRY(tbk_ws_reserve(ctx, tbk_radix_ws_bytes(n) + 65536));
  char* side = nullptr;
  const size_t m = n ? n : 1;
  TBK_HIP(hipMalloc((void**)&side, m * 20));
  SortBufs b{hi, lo, val, (uint64_t*)side, (uint64_t*)(side + m * 8), (uint32_t*)(side + m * 16)};
  int rc = tbk_radix_sort128(ctx, &b, n, only_hi, only_lo, exact != 0);
  hipError_t e = hipSuccess;
  if (rc == 0 && b.hi != hi) {
    e = hipMemcpyAsync(hi, b.hi, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(lo, b.lo, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(val, b.val, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(side);
  if (rc == 0 && (e != hipSuccess || es != hipSuccess)) rc = TBK_EHIP;
  return rc;
}

// sorts w in place.  emit_calls [n + 1] (zeroed by the caller) and emit_word [n], both given or both null: with them the sort is
// tbk_radix_sort_w64_emit with ProbeEmit
int probe_radix_w64(tbk_ctx* ctx, uint64_t* w, uint32_t n, uint64_t mask, int exact, uint32_t* emit_calls, uint64_t* emit_word) {
  Call call(ctx);
  TBK_TRY(tbk_ws_reserve(ctx, tbk_radix_ws_bytes(n) + 65536));
  uint64_t* side = nullptr;
  TBK_HIP(hipMalloc((void**)&side, (size_t)(n ? n : 1) * 8));
  uint64_t *a = w, *a2 = side;
  int rc;
  if (emit_calls && emit_word)
    rc = tbk_radix_sort_w64_emit(ctx, &a, &a2, n, mask, exact != 0, ProbeEmit{emit_calls, emit_word, n});
  else
    rc = tbk_radix_sort_w64(ctx, &a, &a2, n, mask, exact != 0);
  hipError_t e = hipSuccess;
  if (rc == 0 && a != w) e = hipMemcpyAsync(w, a, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(side);
  if (rc == 0 && (e != hipSuccess || es != hipSuccess)) rc = TBK_EHIP;
  return rc;
}

// Both sides are the caller's (n_hi elements each).  err_out_host[0]: the device error word as it is (TBK_DERR_BIGBUCKET is 1 << 8),
// err_out_host[1]: 1 when the routine left its result side in (hi2, lo2, val2), 0 when in (hi, lo, val); the other side is then the
// phase-A output, which the fallback sorts again
int probe_sort_runs(tbk_ctx* ctx, uint64_t* hi, uint64_t* lo, uint32_t* val, uint32_t n_hi, const uint32_t* run_off, uint32_t nruns, uint32_t* err_out_host,
                    uint64_t* hi2, uint64_t* lo2, uint32_t* val2) {
  Call call(ctx);
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)n_hi / 256 + 65536));
  uint32_t* nbig = ws_alloc<uint32_t>(ctx, 1);
  if (!nbig) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(nbig, 0, sizeof(uint32_t), ctx->stream));
  TBK_TRY(clear_derr(ctx));
  SortBufs b{hi, lo, val, hi2, lo2, val2};
  const int rc = tbk_sort_runs(ctx, &b, n_hi, run_off, nruns, ctx->d_err, nbig);
  uint32_t bits = 0;
  TBK_TRY(tbk_sync_err(ctx, &bits));
  err_out_host[0] = bits;
  err_out_host[1] = b.hi == hi2 ? 1u : 0u;
  return rc;
}

// words: 2 or 5.  form: 0 = the default of a caller that passes single_pass = false, 1 = look-back, 2 = three launches.
// delay_ticks != 0: the lane that loads element delay_index waits that long (clamped to 10 ms) before its load returns
int probe_scan(tbk_ctx* ctx, const uint32_t* flag, const uint32_t* value, uint32_t n, int words, int form, uint32_t delay_index, uint32_t delay_ticks,
               uint32_t* out_elem, uint32_t* out_inc, uint32_t* out_exc, uint32_t* err_out_host) {
  Call call(ctx);
  if ((words != 2 && words != 5) || form < 0 || form > 2) return TBK_EINVAL;
  if (delay_ticks > PROBE_MAX_DELAY) delay_ticks = PROBE_MAX_DELAY;
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)cdiv(n, SO_TILE) * (size_t)words * 32 + 65536));
  TBK_TRY(clear_derr(ctx));
  const int saved = ctx->dbg.scan;
  ctx->dbg.scan = form;
  const int rc = words == 2 ? run_scan<2>(ctx, flag, value, n, delay_index, delay_ticks, out_elem, out_inc, out_exc)
                            : run_scan<5>(ctx, flag, value, n, delay_index, delay_ticks, out_elem, out_inc, out_exc);
  ctx->dbg.scan = saved;
  uint32_t bits = 0;
  TBK_TRY(tbk_sync_err(ctx, &bits));
  *err_out_host = bits;
  return rc;
}

// E: 4 or 8 (the library's two instantiations).  The first scan's value has 3 words (flag + 2 sums)
int probe_scan_two(tbk_ctx* ctx, const uint32_t* flag, const uint32_t* value, uint32_t n, int E, uint32_t* out_inc, uint32_t* out_exc, uint32_t* out_term,
                   uint32_t* out_before, uint32_t* err_out_host) {
  Call call(ctx);
  if (E != 4 && E != 8) return TBK_EINVAL;
  TBK_TRY(tbk_ws_reserve(ctx, (size_t)cdiv(n, 256u * (uint32_t)E) * 128 + 65536));
  TBK_TRY(clear_derr(ctx));
  const int rc = E == 4 ? run_scan_two<4>(ctx, flag, value, n, out_inc, out_exc, out_term, out_before)
                        : run_scan_two<8>(ctx, flag, value, n, out_inc, out_exc, out_term, out_before);
  uint32_t bits = 0;
  TBK_TRY(tbk_sync_err(ctx, &bits));
  *err_out_host = bits;
  return rc;
}

}  // extern "C"
