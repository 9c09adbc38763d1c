// track_run_probe — test infrastructure (tests/test_track_run_cpu.py): tbh::run_tracks and tbh::CovRecs (tiebrush_amd/csrc/host/tracks.h)
// as a plain program, without HIP and without libtbk.so.  The device entry points of the TrackApi are host stubs that log every call
// with its capacities and arguments on stdout and answer from a script given on the command line.
//   track_run_probe run OUTDIR [key=value ...]
//       recs=N co=M        n_records / n_cigar_ops of the input (the stubs read no record; N > 0: the coverage and sample stubs give
//                          their canned rows, else none)
//       cov=1 junc=1 samp=1   the tracks to open: OUTDIR/c, OUTDIR/j, OUTDIR/s
//       tabix=1 bigwig=1 bw_device=1 summary=1 device_text=1   the options of the run (summary: two features into OUTDIR/OUT.tsv)
//       clip=R             a clip table of R intervals (R = 1: through the one-region entries)
//       e2big=K            the sample stub's first call answers TBK_E2BIG and says it needs K rows
//       fmt=marker|unsupported|sinkfail   what the format_track stub does
//       null=NAME[,NAME]   table entries left null: track_bgzf, bigwig_build, cov_summary
//       the last stdout line: "times host_tracks=H"
//   track_run_probe strand FILE.bam
//       CovRecs::append over the file's records (YC / YX with tiecov's defaults), one line per record:
//       tid pos flag strand yc yx cig_off n_cigar
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tiebrush_amd/csrc/host/GSam.h"
#include "../../tiebrush_amd/csrc/host/tracks.h"

namespace {
tbk_ctx* const kCtx = (tbk_ctx*)0x1000;  // (never dereferenced: every entry is a stub)
long g_e2big = 0;
int g_sample_calls = 0;
std::string g_fmt = "marker";

// the canned rows: three intervals, two junctions, two sample rows
const int32_t IV_TID[3] = {0, 0, 1}, IV_START[3] = {10, 20, 5}, IV_END[3] = {20, 35, 9};
const double IV_VAL[3] = {1.0, 2.5, 1234.0625};
const int32_t J_TID[2] = {0, 1}, J_START[2] = {20, 100}, J_END[2] = {300, 250};
const uint8_t J_STRAND[2] = {'+', '-'};
const double J_VAL[2] = {3.0, 0.5};
const int32_t S_TID[2] = {0, 1}, S_START[2] = {10, 5}, S_END[2] = {35, 9};
const int64_t S_COUNT[2] = {2, 1};
const float S_HEAT[2] = {0.25f, 1.0f};

int coverage_tile(tbk_ctx* ctx, const tbk_cov_in* in, tbk_cov_out* o) {
  printf("coverage_tile ctx=%d recs=%u co=%u cap_intervals=%u cap_junctions=%u\n", ctx == kCtx, in->n_records, in->n_cigar_ops, o->cap_intervals, o->cap_junctions);
  o->n_intervals = o->n_junctions = 0;
  if (!in->n_records) return 0;
  if (o->cap_intervals >= 3) {
    o->n_intervals = 3;
    for (int i = 0; i < 3; ++i) o->iv_tid[i] = IV_TID[i], o->iv_start[i] = IV_START[i], o->iv_end[i] = IV_END[i], o->iv_val[i] = IV_VAL[i];
  }
  if (o->cap_junctions >= 2) {
    o->n_junctions = 2;
    for (int i = 0; i < 2; ++i) o->j_tid[i] = J_TID[i], o->j_start[i] = J_START[i], o->j_end[i] = J_END[i], o->j_strand[i] = J_STRAND[i], o->j_val[i] = J_VAL[i];
  }
  return 0;
}
int sample_tile(tbk_ctx*, const tbk_cov_in* in, int32_t num_samples, tbk_sample_out* o) {
  printf("sample_tile call=%d num_samples=%d cap_intervals=%u\n", ++g_sample_calls, num_samples, o->cap_intervals);
  o->n_intervals = 0;
  if (g_e2big && g_sample_calls == 1) return o->n_intervals = (uint32_t)g_e2big, TBK_E2BIG;
  if (!in->n_records) return 0;
  if (o->cap_intervals < 2) return o->n_intervals = 2, TBK_E2BIG;
  o->n_intervals = 2;
  for (int i = 0; i < 2; ++i) o->iv_tid[i] = S_TID[i], o->iv_start[i] = S_START[i], o->iv_end[i] = S_END[i], o->iv_count[i] = S_COUNT[i], o->iv_heat[i] = S_HEAT[i];
  return 0;
}
int cov_clip(tbk_ctx*, tbk_cov_out* o, int32_t tid, int64_t beg, int64_t end) {
  return printf("cov_clip rows=%u tid=%d beg=%lld end=%lld\n", o->n_intervals, tid, (long long)beg, (long long)end), 0;
}
int cov_clip_regions(tbk_ctx*, tbk_cov_out* o, const tbk_regions* U) { return printf("cov_clip_regions rows=%u regions=%u\n", o->n_intervals, U->n), 0; }
int sample_clip(tbk_ctx*, tbk_sample_out* o, int32_t tid, int64_t beg, int64_t end) {
  return printf("sample_clip rows=%u tid=%d beg=%lld end=%lld\n", o->n_intervals, tid, (long long)beg, (long long)end), 0;
}
int sample_clip_regions(tbk_ctx*, tbk_sample_out* o, const tbk_regions* U) { return printf("sample_clip_regions rows=%u regions=%u\n", o->n_intervals, U->n), 0; }
int track_names(tbk_ctx*, uint32_t n, const uint64_t* off, const char* bytes) {
  return printf("track_names n=%u bytes=%.*s\n", n, (int)off[n], bytes), 0;
}
const char* g_last_error = "";
int format_track(tbk_ctx*, const tbk_track_rows* r, tbk_track_sink sink, void* user, uint64_t*) {
  printf("format_track kind=%d rows=%u fmt=%s\n", r->kind, r->n, g_fmt.c_str());
  if (g_fmt == "unsupported") return g_last_error = "a value outside the formatter's range", TBK_EUNSUPPORTED;
  if (g_fmt == "sinkfail") return g_last_error = "the sink refused a slice", TBK_EINVAL;
  char line[64];
  const int len = snprintf(line, sizeof(line), "MARKER kind=%d rows=%u\n", r->kind, r->n);
  return sink(user, line, (uint64_t)len);
}
int track_bgzf(tbk_ctx*, const tbk_track_rows* r, const char*, uint32_t head_len, const tbk_ix_opts* ix, tbk_tbx_sink, void*, uint64_t*, uint64_t*) {
  printf("track_bgzf kind=%d rows=%u head_len=%u n_ref=%u\n", r->kind, r->n, head_len, ix->n_ref);
  return g_last_error = "the stub writes no run", TBK_EUNSUPPORTED;  // (before its first run: the host path takes the track)
}
int bigwig_build(tbk_ctx*, const tbk_track_rows* r, uint32_t n_ref, const uint32_t*, tbk_bw_sink, void*, tbk_bw_out*) {
  printf("bigwig_build rows=%u n_ref=%u\n", r->n, n_ref);
  return g_last_error = "the stub builds no section", TBK_EUNSUPPORTED;
}
int cov_summary(tbk_ctx*, const tbk_cov_out* rows, const tbk_features* f, tbk_feat_out* o) {
  printf("cov_summary intervals=%u junctions=%u features=%u\n", rows->n_intervals, rows->n_junctions, f->n);
  for (uint32_t i = 0; i < f->n; ++i) o->covered[i] = 4 + i, o->sum[i] = 10.0 + i, o->max[i] = 2.5, o->junc[i] = (double)i;
  return 0;
}
const char* strerror_stub(int rc) { return rc == TBK_EUNSUPPORTED ? "unsupported" : rc == TBK_EINVAL ? "invalid" : "status"; }
const char* last_error(const tbk_ctx*) { return g_last_error; }

int run(int argc, char** argv) {
  const std::string dir = argv[0];
  long recs = 0, co = 0, clip_n = 0;
  bool cov = false, junc = false, samp = false, summary = false;
  tbh::TrackOptions topt;
  tbh::TrackRun run;
  std::string nulls;
  for (int a = 1; a < argc; ++a) {
    const char* eq = strchr(argv[a], '=');
    if (!eq) return fprintf(stderr, "bad argument: %s\n", argv[a]), 2;
    const std::string k(argv[a], (size_t)(eq - argv[a])), v(eq + 1);
    const long num = atol(v.c_str());
    if (k == "recs") recs = num;
    else if (k == "co") co = num;
    else if (k == "cov") cov = num;
    else if (k == "junc") junc = num;
    else if (k == "samp") samp = num;
    else if (k == "tabix") topt.tabix = num;
    else if (k == "bigwig") topt.bigwig = num;
    else if (k == "bw_device") topt.bw_device = num;
    else if (k == "summary") summary = num;
    else if (k == "device_text") run.device_text = num;
    else if (k == "clip") clip_n = num;
    else if (k == "e2big") g_e2big = num;
    else if (k == "fmt") g_fmt = v;
    else if (k == "null") nulls = "," + v + ",";
    else return fprintf(stderr, "unknown key: %s\n", argv[a]), 2;
  }
  tbh::TrackApi api;
  api.ctx = kCtx;
  api.coverage_tile = coverage_tile, api.sample_tile = sample_tile;
  api.cov_clip = cov_clip, api.cov_clip_regions = cov_clip_regions, api.sample_clip = sample_clip, api.sample_clip_regions = sample_clip_regions;
  api.track_names = track_names, api.format_track = format_track, api.strerror_ = strerror_stub, api.last_error = last_error;
  if (nulls.find(",track_bgzf,") == std::string::npos) api.track_bgzf = track_bgzf;
  if (nulls.find(",bigwig_build,") == std::string::npos) api.bigwig_build = bigwig_build;
  if (nulls.find(",cov_summary,") == std::string::npos) api.cov_summary = cov_summary;

  const std::vector<std::string> names = {"chr1", "chr2"};
  const std::vector<uint32_t> lens = {1000000, 500000};
  if (cov) topt.cov = dir + "/c";
  if (junc) topt.junc = dir + "/j";
  if (samp) topt.samp = dir + "/s";
  tbh::TrackFiles tf;
  tf.open(topt, names, lens);

  tbh::SummaryJob sj;
  if (summary) {
    sj.out = dir + "/OUT.tsv", sj.bed = "features.bed";
    tbh::FeatureTable& F = sj.F;
    F.tid = {0, 1}, F.beg = {10, 100}, F.end = {30, 250}, F.strand = {'+', '.'}, F.name = {"f0", "f1"}, F.line = {1, 2};
  }
  const int32_t rt[3] = {0, 0, 1};
  const int64_t rb[3] = {5, 100, 0}, re[3] = {40, 400, 300};
  tbk_regions regs;
  regs.n = (uint32_t)clip_n, regs.tid = rt, regs.beg = rb, regs.end = re;
  const tbh::TrackClip clip{&regs, clip_n == 1};
  tbk_cov_in in;
  memset(&in, 0, sizeof(in));
  in.mem = TBK_MEM_HOST, in.n_records = (uint32_t)recs, in.n_cigar_ops = (uint32_t)co;
  tbh::TrackTimes tt;
  run.clip = clip_n ? &clip : nullptr;
  run.num_samples = 3, run.bw_device = topt.bw_device, run.summary = &sj, run.times = &tt;
  tbh::run_tracks(api, in, names, tf, run);
  if (tf.cov || tf.junc || tf.samp || tf.cov_bw || tf.cov_tx.is_open() || tf.junc_tx.is_open() || tf.samp_tx.is_open()) return fprintf(stderr, "a track is still open\n"), 3;
  printf("times host_tracks=%d\n", tt.host_tracks);
  return 0;
}

int strand(const char* path) {
  tbh::BamFile bf;
  std::string err;
  if (!bf.load(path, err, 1)) return fprintf(stderr, "cannot read %s (%s)\n", path, err.c_str()), 2;
  tbh::CovRecs R;
  auto values = [](uint32_t, const tbh::RecView& v, double* yc, int64_t* yx) {
    const uint8_t* s = tbh::aux_get(v.aux_begin(), v.aux_end(), "YC");
    *yc = s ? tbh::aux2f(s) : 1.0;
    s = tbh::aux_get(v.aux_begin(), v.aux_end(), "YX");
    *yx = s ? tbh::aux2i(s) : 1;
  };
  // two appends, the second on three workers: the offsets go on from the first's
  const uint32_t n = (uint32_t)bf.n(), half = n / 2;
  if (!R.append(half, [&](uint32_t i) { return bf.rec(i); }, values, 1)) return 3;
  if (!R.append(n - half, [&](uint32_t i) { return bf.rec(half + i); }, values, 3)) return 3;
  const tbk_cov_in in = R.as_cov_in();
  if (in.n_records != n || in.n_cigar_ops != in.cig_off[n] || in.mem != TBK_MEM_HOST) return 4;
  for (uint32_t i = 0; i < n; ++i) {
    printf("%d %d %u %c %g %lld %u %u", in.tid[i], in.pos[i], in.flag[i], in.strand[i], in.yc[i], (long long)in.yx[i], in.cig_off[i], in.cig_off[i + 1] - in.cig_off[i]);
    for (uint32_t c = in.cig_off[i]; c < in.cig_off[i + 1]; ++c) printf(" %u", in.cig[c]);
    printf("\n");
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  if (argc >= 3 && !strcmp(argv[1], "run")) return run(argc - 2, argv + 2);
  if (argc == 3 && !strcmp(argv[1], "strand")) return strand(argv[2]);
  return fprintf(stderr, "usage: track_run_probe run OUTDIR [key=value ...] | strand FILE.bam\n"), 2;
}
