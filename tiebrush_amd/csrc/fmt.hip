// fmt.hip — the text of tiecov's three tracks, formatted on the device (tbk_format_track).
//
// What the reference's flushCoverage / CJunc::write / flushCoverage(pair) print with fprintf (tiecov.cpp:91-95, :237, :289):
//   coverage  "%s\t%d\t%d\t%.3f\n"
//   junction  "%s\t%d\t%d\tJUNC%08d\t%.3f\t%c\n"
//   sample    "%s\t%d\t%d\t%ld\t%f\n"          (the float heat promoted to double)
// Three passes: the length of every line (and a range check of its values), an exclusive scan of the lengths, then the bytes.  The
// bytes go out in slices of bounded size through two device buffers and two pinned host buffers: the device formats slice k + 1 while
// the caller's sink takes slice k.  tbk_track_bgzf cuts the same slices and keeps the text on the device: what leaves is BGZF members and
// their tabix index parts.
//
// %.3f / %f: the printed digits are those of the EXACT binary value rounded half to even, as glibc prints them.  No floating-point
// arithmetic is involved: v = m * 2^e with m < 2^53; the integer part is m >> -e (or m << e), the fraction's digits are
// (fraction bits * 10^k) >> -e in 128-bit integers, and the bits shifted out, compared with one half, decide the rounding.  A
// carry out of the fraction (999.9995 -> 1000.000) moves into the integer part.  Bound: finite values of magnitude below 2^63 (the
// integer part is a uint64); anything else makes the call return TBK_EUNSUPPORTED before the sink sees a byte.
#include <algorithm>

#include "dev_common.hpp"
#include "tbk_internal.h"

namespace {

constexpr int FMT_NT = 256;          // rows per block
constexpr uint32_t FMT_LDS = 16384;  // bytes of a block's lines staged in LDS (64 a line on average)

enum : uint32_t { FMT_ERR_RANGE = 1, FMT_ERR_TID = 2 };

struct Rows {
  int kind;
  uint32_t n;
  const int32_t *tid, *start, *end;
  const double* val;
  const uint8_t* strand;
  const int64_t* count;
  const float* heat;
  int64_t first_junc;
  const uint64_t* name_off;
  const char* names;
  uint32_t n_names;
};

__device__ __forceinline__ uint32_t ndig(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) v /= 10, ++d;
  return d;
}

// a byte sink: counts (WR false) or writes
template <bool WR>
struct Out {
  char* p;
  uint32_t n;
  __device__ __forceinline__ void put(char c) {
    if (WR) p[n] = c;
    ++n;
  }
  __device__ __forceinline__ void digits(uint64_t v, uint32_t nd) {  // exactly nd digits (leading zeros when v is shorter)
    if (WR)
      for (uint32_t k = 0; k < nd; ++k) p[n + nd - 1 - k] = (char)('0' + v % 10), v /= 10;
    n += nd;
  }
  // printf's %d / %ld, zero-padded to `width` like %08d (the sign counts towards the width)
  __device__ __forceinline__ void integer(int64_t x, uint32_t width = 0) {
    const bool neg = x < 0;
    const uint64_t a = neg ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
    if (neg) put('-');
    const uint32_t d = ndig(a), w = width > (neg ? 1u : 0u) ? width - (neg ? 1u : 0u) : 0u;
    digits(a, d > w ? d : w);
  }
  // printf's %.kf of the exact value; false: outside the bound
  __device__ __forceinline__ bool fixed(double v, uint32_t k, uint64_t pow10k) {
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    const uint64_t ab = bits & ~(1ull << 63);
    if (ab >= 0x43E0000000000000ull) return false;  // |v| >= 2^63, inf, nan
    const uint32_t ex = (uint32_t)(ab >> 52);
    const uint64_t m = ex ? ((ab & ((1ull << 52) - 1)) | (1ull << 52)) : ab;
    const int e = ex ? (int)ex - 1075 : -1074;
    uint64_t ip, q = 0;
    if (e >= 0) {
      ip = m << e;
    } else {
      const uint32_t s = (uint32_t)-e;
      ip = s < 64 ? m >> s : 0;
      const uint64_t fr = s < 64 ? m & ((1ull << s) - 1) : m;
      if (s < 74) {  // (s >= 74: fr * 10^k < 2^73 <= half, the fraction rounds to 0)
        const unsigned __int128 P = (unsigned __int128)fr * pow10k;
        q = (uint64_t)(P >> s);
        const unsigned __int128 rem = P - ((unsigned __int128)q << s), half = (unsigned __int128)1 << (s - 1);
        if (rem > half || (rem == half && (q & 1))) ++q;
        if (q == pow10k) q = 0, ++ip;
      }
    }
    if (bits >> 63) put('-');
    digits(ip, ndig(ip));
    put('.');
    digits(q, k);
    return true;
  }
};

// line i of the track; returns false when a value is outside the bound or the reference index has no name
template <bool WR>
__device__ __forceinline__ uint32_t emit(const Rows& R, uint32_t i, char* dst, uint32_t* err) {
  Out<WR> o{dst, 0};
  const int32_t t = R.tid[i];
  if (t < 0 || (uint32_t)t >= R.n_names) {
    *err |= FMT_ERR_TID;
    return 0;
  }
  const uint64_t a = R.name_off[t], b = R.name_off[t + 1];
  if (WR)
    for (uint64_t c = a; c < b; ++c) o.put(R.names[c]);
  else
    o.n += (uint32_t)(b - a);
  o.put('\t');
  o.integer(R.start[i]);
  o.put('\t');
  o.integer(R.end[i]);
  o.put('\t');
  bool ok;
  if (R.kind == TBK_TRACK_COV) {
    ok = o.fixed(R.val[i], 3, 1000);
  } else if (R.kind == TBK_TRACK_JUNC) {
    o.put('J'), o.put('U'), o.put('N'), o.put('C');
    o.integer((int32_t)(R.first_junc + (int64_t)i), 8);  // (int)i + 1 in the reference
    o.put('\t');
    ok = o.fixed(R.val[i], 3, 1000);
    o.put('\t');
    o.put((char)R.strand[i]);
  } else {
    o.integer(R.count[i]);
    o.put('\t');
    ok = o.fixed((double)R.heat[i], 6, 1000000);
  }
  o.put('\n');
  if (!ok) *err |= FMT_ERR_RANGE;
  return o.n;
}

// pass 1: lens[i], the longest line (stat[0]) and the error bits (stat[1])
__global__ void __launch_bounds__(FMT_NT) fmt_len_k(Rows R, uint32_t* lens, uint32_t* stat) {
  const uint32_t i = blockIdx.x * FMT_NT + threadIdx.x;
  uint32_t len = 0, err = 0;
  if (i < R.n) len = emit<false>(R, i, nullptr, &err);
  if (i < R.n) lens[i] = len;
  if (i == R.n) lens[i] = 0;  // (the scan runs over n + 1 entries: its last output is the total)
  // one atomic per wave
  uint32_t mx = len, er = err;
  for (int d = 32; d >= 1; d >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    er |= (uint32_t)__shfl_xor((int)er, d);
  }
  if (lane_id() == 0) {
    if (mx) atomicMax(&stat[0], mx);
    if (er) atomicOr(&stat[1], er);
  }
}

// pass 3: the bytes of rows [lo, hi) into out (offsets relative to off[lo]).  A block stages its lines in LDS and the block stores them
// as consecutive dwords (coalesced whatever the lines' lengths); a block whose lines do not fit writes each line from its own lane.
__global__ void __launch_bounds__(FMT_NT) fmt_write_k(Rows R, const uint64_t* off, uint32_t lo, uint32_t hi, char* out) {
  __shared__ uint32_t stage_w[FMT_LDS / 4];
  char* stage = (char*)stage_w;
  const uint32_t b_lo = lo + blockIdx.x * FMT_NT;
  const uint32_t b_hi = min(hi, b_lo + FMT_NT);
  const uint32_t i = b_lo + threadIdx.x;
  const uint64_t base = off[lo], b0 = off[b_lo];
  const uint64_t span = off[b_hi] - b0;
  uint32_t err = 0;
  char* dst = out + (b0 - base);
  if (span > FMT_LDS) {
    if (i < b_hi) (void)emit<true>(R, i, out + (off[i] - base), &err);
    return;
  }
  if (i < b_hi) (void)emit<true>(R, i, stage + (off[i] - b0), &err);
  __syncthreads();
  const uint32_t sp = (uint32_t)span;
  const uint32_t head = min(sp, (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3));
  const uint32_t nw = (sp - head) >> 2, tail0 = head + nw * 4;
  if (threadIdx.x < head) dst[threadIdx.x] = stage[threadIdx.x];
  uint32_t* dw = (uint32_t*)(dst + head);
  for (uint32_t w = threadIdx.x; w < nw; w += FMT_NT) {
    const uint32_t s = head + 4 * w;
    dw[w] = (uint32_t)(uint8_t)stage[s] | (uint32_t)(uint8_t)stage[s + 1] << 8 | (uint32_t)(uint8_t)stage[s + 2] << 16 |
            (uint32_t)(uint8_t)stage[s + 3] << 24;
  }
  if (tail0 + threadIdx.x < sp) dst[tail0 + threadIdx.x] = stage[tail0 + threadIdx.x];
}

__global__ void fmt_cuts_k(const uint64_t* off, uint32_t n, uint32_t rows, uint32_t ncut, uint64_t* cut) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ncut) cut[c] = off[min((uint64_t)n, (uint64_t)c * rows)];
}

}  // namespace

int tbk_pin_slices(tbk_ctx* ctx, size_t bytes) {
  if (ctx->fmt_pin_cap >= bytes) return 0;
  for (auto& p : ctx->fmt_pin)
    if (p) (void)hipHostFree(p), p = nullptr;
  ctx->fmt_pin_cap = 0;
  for (auto& p : ctx->fmt_pin)
    if (hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      ctx->last_error = "pinned staging allocation failed";
      return TBK_ENOMEM;
    }
  ctx->fmt_pin_cap = bytes;
  return 0;
}

namespace {
// What tbk_format_track and tbk_track_bgzf share: the lines' lengths and offsets, the range check, and the slices of whole lines.
struct FmtPlan {
  Rows R = {};
  uint64_t* off = nullptr;    // device [n + 1]: every line's offset in the track's text
  uint64_t total = 0;         // bytes of the text
  uint32_t per = 0, ns = 0;   // rows per slice, slices
  std::vector<uint64_t> cut;  // [ns + 1] the slices' first bytes
  uint64_t slice_max = 0;
};

int fmt_plan(tbk_ctx* ctx, const tbk_track_rows* rows, FmtPlan& P) {
  Rows& R = P.R;
  R.kind = rows->kind;
  R.n = rows->n;
  R.tid = rows->tid, R.start = rows->start, R.end = rows->end;
  R.val = rows->val, R.strand = rows->strand, R.count = rows->count, R.heat = rows->heat;
  R.first_junc = rows->first_junc;
  R.name_off = ctx->d_name_off, R.names = ctx->d_names, R.n_names = ctx->n_names;
  const uint32_t n = R.n;
  uint32_t* lens = ws_alloc<uint32_t>(ctx, (size_t)n + 1);
  uint64_t* off = P.off = ws_alloc<uint64_t>(ctx, (size_t)n + 1);
  uint32_t* stat = ws_alloc<uint32_t>(ctx, 4);
  uint64_t* d_total = ws_alloc<uint64_t>(ctx, 1);
  if (!lens || !off || !stat || !d_total) return TBK_ENOMEM;
  TBK_HIP(hipMemsetAsync(stat, 0, 4 * sizeof(uint32_t), ctx->stream));
  TBK_LAUNCH(ctx, "fmt_len_k", fmt_len_k, cdiv((uint64_t)n + 1, FMT_NT), FMT_NT, 0, R, lens, stat);
  TBK_TRY(tbk_check_launch(ctx, "fmt_len_k"));
  TBK_TRY(tbk_exscan_u32_u64(ctx, lens, off, n + 1, d_total));
  uint64_t hs[3] = {0, 0, 0};
  TBK_HIP(hipMemcpyAsync(&hs[0], stat, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipMemcpyAsync(&hs[1], d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t maxlen = (uint32_t)hs[0], errb = (uint32_t)(hs[0] >> 32);
  P.total = hs[1];
  if (errb & FMT_ERR_TID) {
    ctx->last_error = "a row's reference index has no name in the table (tbk_track_names)";
    return TBK_EINVAL;
  }
  if (errb & FMT_ERR_RANGE) {
    ctx->last_error = "a value outside the formatter's exact range (finite, magnitude below 2^63)";
    return TBK_EUNSUPPORTED;
  }
  // slices of whole lines, at most `cap` bytes each (a single line longer than that is a slice of its own)
  const uint64_t cap = std::max<uint64_t>(ctx->dbg.fmt_slice ? ctx->dbg.fmt_slice : ((uint64_t)32 << 20), maxlen);
  const uint32_t per = P.per = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(1, cap / std::max<uint32_t>(maxlen, 1)));
  const uint32_t ns = P.ns = cdiv(n, per);
  uint64_t* d_cut = ws_alloc<uint64_t>(ctx, (size_t)ns + 1);
  if (!d_cut) return TBK_ENOMEM;
  TBK_LAUNCH(ctx, "fmt_cuts_k", fmt_cuts_k, cdiv((uint64_t)ns + 1, 256), 256, 0, off, n, per, ns + 1, d_cut);
  TBK_TRY(tbk_check_launch(ctx, "fmt_cuts_k"));
  std::vector<uint64_t>& cut = P.cut;
  cut.assign((size_t)ns + 1, 0);
  TBK_HIP(hipMemcpyAsync(cut.data(), d_cut, cut.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  P.slice_max = 0;
  for (uint32_t s = 0; s < ns; ++s) P.slice_max = std::max(P.slice_max, cut[s + 1] - cut[s]);
  return 0;
}
}  // namespace

int tbk_format_device(tbk_ctx* ctx, const tbk_track_rows* rows, tbk_track_sink sink, void* user, uint64_t* out_bytes) {
  const uint32_t n = rows->n;
  if (out_bytes) *out_bytes = 0;
  if (n == 0) return 0;
  FmtPlan P;
  TBK_TRY(fmt_plan(ctx, rows, P));
  const Rows& R = P.R;
  const uint64_t* off = P.off;
  const uint64_t total = P.total, slice_max = P.slice_max;
  const uint32_t per = P.per, ns = P.ns;
  const std::vector<uint64_t>& cut = P.cut;
  char* dbuf[2] = {ws_alloc<char>(ctx, slice_max + 16), ns > 1 ? ws_alloc<char>(ctx, slice_max + 16) : nullptr};
  if (!dbuf[0] || (ns > 1 && !dbuf[1])) return TBK_ENOMEM;
  TBK_TRY(tbk_pin_slices(ctx, slice_max));
  hipEvent_t ev[2] = {tbk_event(ctx), tbk_event(ctx)};
  if (!ev[0] || !ev[1]) return TBK_EHIP;
  int rc = 0;
  for (uint32_t s = 0; s <= ns && rc == 0; ++s) {
    if (s < ns) {  // slice s: format, copy out
      const uint32_t lo = s * per, hi = std::min<uint64_t>(n, (uint64_t)lo + per);
      TBK_LAUNCH(ctx, "fmt_write_k", fmt_write_k, cdiv(hi - lo, FMT_NT), FMT_NT, 0, R, off, lo, hi, dbuf[s & 1]);
      TBK_TRY(tbk_check_launch(ctx, "fmt_write_k"));
      TBK_HIP(hipMemcpyAsync(ctx->fmt_pin[s & 1], dbuf[s & 1], cut[s + 1] - cut[s], hipMemcpyDeviceToHost, ctx->stream));
      TBK_HIP(hipEventRecord(ev[s & 1], ctx->stream));
    }
    if (s > 0) {  // ... while the sink takes slice s - 1
      const uint32_t p = s - 1;
      TBK_HIP(hipEventSynchronize(ev[p & 1]));
      if (sink(user, (const char*)ctx->fmt_pin[p & 1], cut[p + 1] - cut[p]) != 0) {
        ctx->last_error = "tbk_format_track: the sink refused a slice";
        rc = TBK_EINVAL;
      }
    }
  }
  TBK_HIP(hipStreamSynchronize(ctx->stream));
  if (out_bytes) *out_bytes = total;
  return rc;
}

// tbk_track_bgzf: the slices of tbk_format_track, but the text stays on the device — slice k is formatted into the text
// buffer (the header in front of row 0), deflated into a run of whole members (tbk_bgzf_run), indexed (tbk_tx_build: tx_rec_k and the
// BAM index's back half) and copied into one of two pinned buffers with its part; the context's sink thread takes it while the
// device works on slice k + 1.
int tbk_track_bgzf_device(tbk_ctx* ctx, const tbk_track_rows* rows, const char* head, uint32_t head_len, const tbk_ix_opts* ix, tbk_tbx_sink sink, void* user,
                          uint64_t* text_bytes, uint64_t* out_bytes) {
  const uint32_t n = rows->n;
  if (text_bytes) *text_bytes = 0;
  if (out_bytes) *out_bytes = 0;
  if (n == 0 && head_len == 0) return 0;
  FmtPlan P;
  if (n) TBK_TRY(fmt_plan(ctx, rows, P));  // (the range refusal comes from here: before any run)
  else P.ns = 1, P.cut.assign(2, 0);      // the header alone: one run
  const Rows& R = P.R;
  tbk_ix_opts ixo = {};
  if (ix) ixo = *ix, ixo.rec_vbeg = nullptr;
  const uint64_t text_max = P.slice_max + head_len;
  char* dtext = ws_alloc<char>(ctx, text_max + 64);
  if (!dtext) return TBK_ENOMEM;
  if (head_len) TBK_HIP(hipMemcpyAsync(dtext, head, head_len, hipMemcpyHostToDevice, ctx->stream));
  // a member that does not compress is stored: its payload and a few dozen bytes of framing
  TBK_TRY(tbk_pin_slices(ctx, text_max + (text_max / 0xff00 + 2) * 64));
  struct Slot {  // what the sink of a slice reads while the next slice is made
    tbk_ix_part part;
    std::vector<tbk_ix_chunk> chunks;
    std::vector<uint64_t> lin;
    std::vector<tbk_ix_ref> refs;
    uint64_t zbytes = 0;
  } slot[2];
  int sink_rc = 0;
  uint64_t zsum = 0;
  TbkWorker worker;  // (declared last: it is joined before the slots go)
  for (uint32_t s = 0; s < P.ns; ++s) {
    const size_t mark = ctx->ws_off;  // the slice's temporaries (deflater's scans, index arrays) go when the slice is done
    const uint32_t lo = s * P.per, hi = (uint32_t)std::min<uint64_t>(n, (uint64_t)lo + P.per);
    const uint64_t text0 = s == 0 ? head_len : 0, len = text0 + P.cut[s + 1] - P.cut[s];
    if (hi > lo) {
      TBK_LAUNCH(ctx, "fmt_write_k", fmt_write_k, cdiv(hi - lo, FMT_NT), FMT_NT, 0, R, P.off, lo, hi, dtext + text0);
      TBK_TRY(tbk_check_launch(ctx, "fmt_write_k"));
    }
    uint8_t* packed;
    uint64_t ztotal;
    uint32_t nmem;
    const uint64_t *d_cut, *d_moff;
    TBK_TRY(tbk_bgzf_run(ctx, (const uint8_t*)dtext, len, &packed, &ztotal, &nmem, &d_cut, &d_moff));
    if (ztotal > ctx->fmt_pin_cap) {
      ctx->last_error = "track_bgzf: a run larger than its text allows for";
      return TBK_EHIP;
    }
    Slot& S = slot[s & 1];  // (its last sink call, of slice s - 2, has returned: slice s - 1 was posted behind it)
    TBK_HIP(hipMemcpyAsync(ctx->fmt_pin[s & 1], packed, ztotal, hipMemcpyDeviceToHost, ctx->stream));
    S.zbytes = ztotal;
    if (ix) {  // (the index kernels run under the members' download; the build ends with a synchronisation)
      const TbkTxIn I{hi - lo, lo, R.tid, R.start, R.end, P.off, text0, nmem, d_cut, d_moff, ztotal};
      tbk_ix_part part;
      TBK_TRY(tbk_tx_build(ctx, I, &ixo, &part));
      S.chunks.assign(part.chunks, part.chunks + part.n_chunks);
      S.lin.assign(part.lin, part.lin + part.n_lin);
      S.refs.assign(part.refs, part.refs + part.n_refs);
      S.part = part;
      S.part.chunks = S.chunks.data(), S.part.lin = S.lin.data(), S.part.refs = S.refs.data();
    }
    TBK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->ws_off = mark;
    zsum += ztotal;
    worker.wait();  // slice s - 1 is with the sink since the device began this one
    if (sink_rc != 0) break;
    const uint8_t* zb = (const uint8_t*)ctx->fmt_pin[s & 1];
    const tbk_ix_part* pp = ix ? &S.part : nullptr;
    const uint64_t zn = S.zbytes;
    worker.post([=, &sink_rc]() { sink_rc = sink(user, zb, zn, pp); });
  }
  worker.wait();
  if (sink_rc != 0) {
    ctx->last_error = "tbk_track_bgzf: the sink refused a run";
    return TBK_EINVAL;
  }
  if (text_bytes) *text_bytes = P.total + head_len;
  if (out_bytes) *out_bytes = zsum;
  return 0;
}

int tbk_names_upload(tbk_ctx* ctx, uint32_t n_names, const uint64_t* off, const char* bytes) {
  if (ctx->d_names) (void)hipFree(ctx->d_names), ctx->d_names = nullptr;
  if (ctx->d_name_off) (void)hipFree(ctx->d_name_off), ctx->d_name_off = nullptr;
  ctx->n_names = 0;
  const uint64_t nb = off[n_names];
  TBK_HIP(hipMalloc((void**)&ctx->d_name_off, ((size_t)n_names + 1) * sizeof(uint64_t)));
  TBK_HIP(hipMalloc((void**)&ctx->d_names, nb ? nb : 1));
  TBK_HIP(hipMemcpy(ctx->d_name_off, off, ((size_t)n_names + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (nb) TBK_HIP(hipMemcpy(ctx->d_names, bytes, nb, hipMemcpyHostToDevice));
  ctx->n_names = n_names;
  return 0;
}
