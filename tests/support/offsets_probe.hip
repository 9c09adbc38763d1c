// offsets_probe.hip — test infrastructure only: one C entry point that runs the raw form's offsets pass of the window path
// (wgroup.hip: wg_tidchunks_k, wg_offsets_stream_k<true> or wg_offsets_wave_k, wg_offsets_edges_k, wg_offsets_transpose_k) on hand-built
// records, runs and bounds, so that tests/test_gpu_offsets_pass.py can compare the matrix word for word with numpy
// (tests/offsets_model.py).  Built by tiebrush_amd/csrc/Makefile into tiebrush_amd/_build/libtbk_offsets_probe.so, linked against
// libtbk.so, which neither knows of it nor exports anything for it (tbk_wg_offsets_raw is an ordinary C++ symbol of the library).
// Which kernel runs is the context's debug state: wg_offsets=block, wg_og=N (tbk_set_debug).
#include "dev_common.hpp"
#include "tbk_internal.h"
#include "wgroup.h"

extern "C" {

// tid / pos [n], run_off [k + 1], W [nW] (sorted), off [(nW + 2) * k], wbase [nW + 2]: device memory; *err_out_host: the device error bits
int probe_offsets_raw(tbk_ctx* ctx, const int32_t* tid, const int32_t* pos, const uint32_t* run_off, uint32_t k, uint32_t n, const uint64_t* W,
                      uint32_t nW, uint32_t* off, uint32_t* wbase, uint32_t* err_out_host) {
  tbk_prof_begin_call(ctx);
  int rc = tbk_ws_reserve(ctx, ((size_t)nW + 2) * k * 4 + (size_t)n / 1024 + 65536);
  if (rc == 0 && hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), ctx->stream) != hipSuccess) rc = TBK_EHIP;
  if (rc == 0) rc = tbk_wg_offsets_raw(ctx, tid, pos, run_off, k, n, W, nW, off, wbase);
  uint32_t bits = 0;
  if (rc == 0) rc = tbk_sync_err(ctx, &bits);
  *err_out_host = bits;
  tbk_prof_end_call(ctx);
  return rc;
}

}  // extern "C"
