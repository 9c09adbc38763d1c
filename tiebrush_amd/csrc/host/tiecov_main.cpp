// tiecov — drop-in command line of the reference's coverage tool (/root/reference/src/tiecov.cpp:345-573).
// The per-record loop (:435-499: bundles, addCov, addJunction, addMean, flushes) is replaced by
// tbk_coverage_tile / tbk_sample_tile (HIP); BAM decode and text output stay on the host.
// With -r REGION (no counterpart in the reference) only the chunks the file's index names for the region are read, and
// they are inflated, decoded, filtered, summarised and cut to the region on the device (regions_main below).
// With -R FILE the same for the region table of a BED file, in one run: the chunks are merged over the whole table.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/tbk.h"
#include "GSam.h"
#include "args.h"
#include "bai_read.h"
#include "tracks.h"

#define VERSION "0.0.7"

static const char* USAGE =
    "TieCov v" VERSION " (MI355X build)\n"
    "Summarises a (TieBrush-collapsed) BAM file as BED-like tracks.\n"
    "\n"
    " usage: tiecov [-s out.sample] [-c out.coverage] [-j out.junctions] [--features BED --summary OUT.tsv] [-r REGION | -R FILE] input.bam\n"
    "\n"
    "  -h,--help    print this text and exit\n"
    "  --version    print the version and exit\n"
    "  -c PREFIX    per-base coverage as bedGraph (the YC tag weighs each alignment)\n"
    "  -j PREFIX    splice junctions as BED\n"
    "  -s PREFIX    estimated number of samples per position as bedGraph (needs @CO SAMPLE: header lines)\n"
    "  -W           write the coverage (-c) as a bigWig file (PREFIX.bigwig) instead of a bedGraph\n"
    "  --bigwig-writer host|device   with -W: who builds the file's sections and zoom levels — this core with zlib (host, the\n"
    "               default) or the GPU (device: the same payloads, compressed by the device's deflater)\n"
    "  --tabix      write every text track BGZF-compressed with its tabix index: PREFIX.bedgraph.gz / PREFIX.bed.gz and FILE.gz.tbi\n"
    "               beside each (FILE.gz.csi when a reference is longer than 2^29), what bgzip and tabix -p bed -S 1 make of the\n"
    "               plain tracks; compressed and indexed on the GPU (TBK_TRACK_HOST_FMT=1: on the cores).  With -W the coverage\n"
    "               stays the bigWig.  Not with -c - / stdout\n"
    "  -r,--region REGION   only the tracks of REGION: NAME, NAME:BEG or NAME:BEG-END (1-based, inclusive, commas allowed), read\n"
    "               through the file's index (input.bam.csi, input.bam.bai or input.bai; `tiebrush --index` / `--csi` write one)\n"
    "  -R,--regions-file FILE   the tracks of several regions in one run: FILE is BED (chrom start end, 0-based half-open; further\n"
    "               columns ignored), its intervals sorted and merged where they overlap or abut; read through the index like -r\n"
    "  --index-file PATH    the index to use with -r / -R\n"
    "  --features BED --summary OUT.tsv   per-feature coverage and junction support: one line of OUT.tsv per line of BED (chrom start\n"
    "               end [name [score [strand]]]; features may overlap, nest and repeat, nothing is merged): size, covered bases, sum,\n"
    "               mean0 = sum / size, mean = sum / covered, max of the coverage, and junc = the junction track's value for the feature\n"
    "               taken as an intron (same start and end; strand + - or, for '.', every strand).  Computed on the GPU from the rows of\n"
    "               -c / -j (TBK_SUMMARY_HOST=1: on this core).  With -r / -R every feature must lie inside one interval of the region\n"
    " At least one of -c / -j / -s / --summary is required.\n";

// ---- tiecov -r --------------------------------------------------------------------------------------------------------------------
// how often -r / --region is given (Args keeps the last value of a repeated option)
static int count_region_opts(int argc, char** argv) {
  static const char* const value_longs[] = {"index-file", "regions-file", "bigwig-writer", "features", "summary", nullptr};
  return count_value_option(argc, argv, "region", 'r', value_longs, "csjR");
}
static int count_regions_file_opts(int argc, char** argv) {
  static const char* const value_longs[] = {"index-file", "region", "bigwig-writer", "features", "summary", nullptr};
  return count_value_option(argc, argv, "regions-file", 'R', value_longs, "csjr");
}

// ---- what every run does with its records: the tracks -----------------------------------------------------------------------------
// file names and header lines: tracks.cpp (tiecov.cpp:365-402)
static void open_tracks(tbh::TrackFiles& tf, sam_hdr_t* hdr, const std::string& covfname, const std::string& jfname, const std::string& sfname, bool bigwig,
                        bool tabix) {
  std::vector<std::string> names;
  std::vector<uint32_t> lens;
  for (int t = 0; t < hdr->n_targets; ++t) {
    names.push_back(hdr->target_name[t]);
    lens.push_back(hdr->target_len[t]);
  }
  tf.open(covfname, jfname, sfname, bigwig, names, lens, tabix);
}

// the cut of a region run: the table, through the one-region entries (one: the table is the region itself, which may be empty) or the
// table entries
struct TrackClip {
  const tbk_regions* U;
  bool one;
};

// The rows of tbk_coverage_tile / tbk_sample_tile for `in` (host arrays, or a device view), cut to *clip where one is given, into the
// open files of tf.  An input of no records goes the same way: the calls give no rows and status 0.  With a summary job the coverage
// and junction rows are computed whatever tracks are open, and summarised before the cut.
static void write_tracks(tbk_ctx* ctx, sam_hdr_t* hdr, const tbk_cov_in& in, int num_samples, tbh::TrackFiles& tf, const TrackClip* clip, bool bw_device,
                         const tbh::SummaryJob& sj) {
  const size_t n = in.n_records, co = in.n_cigar_ops;
  const size_t extra = clip ? clip->U->n : 0;  // (a clip over a table of R intervals can grow the interval rows by R - 1: the arrays are sized with R added)
  FILE *coutf = tf.cov, *joutf = tf.junc, *soutf = tf.samp;
  const bool cov_bw = tf.cov_bw;
  // --tabix: a track's writer is open in the place of its FILE*
  const bool cov_tx = tf.cov_tx.is_open(), junc_tx = tf.junc_tx.is_open(), samp_tx = tf.samp_tx.is_open();
  tbh::TabixDevice txd;
  txd.ctx = ctx, txd.track_bgzf = tbk_track_bgzf, txd.track_names = tbk_track_names, txd.strerror_ = tbk_strerror, txd.last_error = tbk_last_error;
  auto tabix_rows = [](int kind, uint32_t nr, const int32_t* t, const int32_t* s, const int32_t* e) {
    tbk_track_rows r;
    memset(&r, 0, sizeof(r));
    r.mem = TBK_MEM_HOST, r.kind = kind, r.n = nr, r.tid = t, r.start = s, r.end = e, r.first_junc = 1;
    return r;
  };
  int rc = 0;
  if (coutf || cov_bw || joutf || cov_tx || junc_tx || sj.on()) {
    const size_t ci = (coutf || cov_bw || cov_tx || sj.on()) ? 2 * co + 2 * n + 16 + extra : 0, cj = (joutf || junc_tx || sj.on()) ? co + 16 : 0;
    std::vector<int32_t> it(ci ? ci : 1), is(ci ? ci : 1), ie(ci ? ci : 1), jt(cj ? cj : 1), js(cj ? cj : 1), je(cj ? cj : 1);
    std::vector<double> iv(ci ? ci : 1), jv(cj ? cj : 1);
    std::vector<uint8_t> jstr(cj ? cj : 1);
    tbk_cov_out o;
    memset(&o, 0, sizeof(o));
    o.mem = TBK_MEM_HOST;
    o.cap_intervals = (uint32_t)ci;
    o.iv_tid = it.data();
    o.iv_start = is.data();
    o.iv_end = ie.data();
    o.iv_val = iv.data();
    o.cap_junctions = (uint32_t)cj;
    o.j_tid = jt.data();
    o.j_start = js.data();
    o.j_end = je.data();
    o.j_strand = jstr.data();
    o.j_val = jv.data();
    rc = tbk_coverage_tile(ctx, &in, &o);
    if (rc == TBK_EFATALOP) GError("ERROR: unknown opcode in a CIGAR string (tiecov accepts M, I, D, N, S only)\n");
    if (rc != 0) GError("Error: GPU coverage failed: %s (%s)\n", tbk_strerror(rc), tbk_last_error(ctx));
    if (sj.on()) {
      tbh::SummaryDevice sd;
      sd.ctx = ctx, sd.summary = tbk_cov_summary, sd.strerror_ = tbk_strerror, sd.last_error = tbk_last_error;
      tbh::write_summary(sj, hdr->target_name, o, sd);
    }
    if (clip) {
      const tbk_regions* U = clip->U;
      rc = clip->one ? tbk_cov_clip(ctx, &o, U->tid[0], U->beg[0], U->end[0]) : tbk_cov_clip_regions(ctx, &o, U);
      if (rc != 0) GError("Error: GPU clip failed: %s (%s)\n", tbk_strerror(rc), tbk_last_error(ctx));
    }
    if (coutf) tbh::emit_cov_lines(coutf, hdr->target_name, o.n_intervals, it.data(), is.data(), ie.data(), iv.data());  // flushCoverage, tiecov.cpp:237
    if (cov_bw) {  // flushCoverage(bigWigFile_t*), tiecov.cpp:243-275: the same intervals, the value as a float
      tbh::BigWigDevice bd;
      bd.ctx = ctx, bd.build = tbk_bigwig_build, bd.strerror_ = tbk_strerror, bd.last_error = tbk_last_error;
      tf.write_bigwig(o.n_intervals, it.data(), is.data(), ie.data(), iv.data(), bw_device ? &bd : nullptr);
    }
    if (joutf)  // CJunc::write, tiecov.cpp:91-95 (numbered from 1)
      tbh::emit_junc_lines(joutf, hdr->target_name, o.n_junctions, jt.data(), js.data(), je.data(), jv.data(), jstr.data(), 1);
    if (cov_tx) {
      tbk_track_rows r = tabix_rows(TBK_TRACK_COV, o.n_intervals, it.data(), is.data(), ie.data());
      r.val = iv.data();
      tbh::write_tabix_track(tf.cov_tx, r, hdr->target_name, &txd);
    }
    if (junc_tx) {
      tbk_track_rows r = tabix_rows(TBK_TRACK_JUNC, o.n_junctions, jt.data(), js.data(), je.data());
      r.val = jv.data(), r.strand = jstr.data();
      tbh::write_tabix_track(tf.junc_tx, r, hdr->target_name, &txd);
    }
  }
  if (soutf || samp_tx) {
    // the value of the track changes only where an M segment starts or ends: at most 2 intervals per CIGAR operation + 2 per
    // record, as for the coverage track (not one per covered base); if a call still reports TBK_E2BIG it also reports the
    // count it needs, and the call is repeated with that
    size_t cs = 2 * co + 2 * n + 16 + extra;
    std::vector<int32_t> st, ss, se;
    std::vector<int64_t> sc;
    std::vector<float> sh;
    tbk_sample_out so;
    for (int attempt = 0; attempt < 2; ++attempt) {
      st.resize(cs);
      ss.resize(cs);
      se.resize(cs);
      sc.resize(cs);
      sh.resize(cs);
      memset(&so, 0, sizeof(so));
      so.mem = TBK_MEM_HOST;
      so.cap_intervals = (uint32_t)cs;
      so.iv_tid = st.data();
      so.iv_start = ss.data();
      so.iv_end = se.data();
      so.iv_count = sc.data();
      so.iv_heat = sh.data();
      rc = tbk_sample_tile(ctx, &in, num_samples, &so);
      if (rc != TBK_E2BIG) break;
      cs = (size_t)so.n_intervals + 16 + extra;
    }
    if (rc == TBK_EFATALOP) GError("ERROR: unknown opcode in a CIGAR string (tiecov accepts M, I, D, N, S only)\n");
    if (rc != 0) GError("Error: GPU sample track failed: %s (%s)\n", tbk_strerror(rc), tbk_last_error(ctx));
    if (clip) {
      const tbk_regions* U = clip->U;
      rc = clip->one ? tbk_sample_clip(ctx, &so, U->tid[0], U->beg[0], U->end[0]) : tbk_sample_clip_regions(ctx, &so, U);
      if (rc != 0) GError("Error: GPU clip failed: %s (%s)\n", tbk_strerror(rc), tbk_last_error(ctx));
    }
    if (soutf) tbh::emit_samp_lines(soutf, hdr->target_name, so.n_intervals, st.data(), ss.data(), se.data(), sc.data(), sh.data());  // flushCoverage(pair), tiecov.cpp:289
    if (samp_tx) {
      tbk_track_rows r = tabix_rows(TBK_TRACK_SAMPLE, so.n_intervals, st.data(), ss.data(), se.data());
      r.count = sc.data(), r.heat = sh.data();
      tbh::write_tabix_track(tf.samp_tx, r, hdr->target_name, &txd);
    }
  }
}

// The run of -r (one: U is the region itself, which may be empty, and goes through the one-region entries) and of -R (U is the
// normalised table of the BED file, through the table entries): every other statement is shared.
static int regions_main(sam_hdr_t* hdr, const std::string& infname, const tbh::RegionTable& U, bool one, const std::string& index_file,
                        const std::string& covfname, const std::string& jfname, const std::string& sfname, bool bigwig,
                        bool bw_device, bool tabix, const tbh::SummaryJob& sj, const std::chrono::steady_clock::time_point t0) {
  const bool timing = getenv("TBK_TIMING") != nullptr;
  auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  // every refusal comes before an output file exists
  std::string err;
  const uint32_t R = (uint32_t)U.n();
  tbk_regions regs;
  regs.n = R, regs.tid = U.tid.data(), regs.beg = U.beg.data(), regs.end = U.end.data();
  int num_samples = 0;
  if (!sfname.empty()) {
    num_samples = (int)hdr->co_samples().size();
    if (num_samples == 0) GError("Error: no sample lines found in header");
  }
  std::vector<tbh::IdxChunk> chunks;
  if (!tbh::index_query_regions_file(infname, index_file, U, chunks, err)) GError("Error: %s\n", err.c_str());
  if (!one && chunks.size() > 65535)
    GError("Error: the index names %zu chunks for the %u regions; the device decode takes 65535\n", chunks.size(), R);
  const double ms_index = ms();
  // the context comes up beside the file reads
  tbk_ctx* ctx = nullptr;
  const int dev = getenv("TBK_DEVICE") ? atoi(getenv("TBK_DEVICE")) : 0;
  int rc = 0;
  std::thread ctx_thread([&]() { rc = tbk_create(dev, &ctx); });
  std::vector<tbh::RegionSpan> spans;
  uint64_t bytes_read = 0;
  const bool read_ok = tbh::read_spans(infname, chunks, spans, &bytes_read, err);
  const double ms_read = ms();
  ctx_thread.join();
  if (!read_ok) GError("Error: %s\n", err.c_str());
  if (rc != 0) GError("Error: cannot use GPU %d (%s); this build has no CPU coverage path\n", dev, tbk_strerror(rc));
  const double ms_ctx = ms();
  const uint32_t k = (uint32_t)spans.size();
  std::vector<const uint8_t*> comp(k);
  std::vector<uint64_t> comp_bytes(k);
  std::vector<uint32_t> first_uoff(k), last_uoff(k), span_off(k + 1, 0);
  for (uint32_t i = 0; i < k; ++i) comp[i] = spans[i].z.data(), comp_bytes[i] = spans[i].z.size(), first_uoff[i] = spans[i].first_uoff, last_uoff[i] = spans[i].last_uoff;
  tbk_soa_in tile;
  const uint8_t* tag_seen = nullptr;
  rc = tbk_bam_decode_spans(ctx, k, comp.data(), comp_bytes.data(), first_uoff.data(), last_uoff.data(), hdr->n_targets, &tile, span_off.data(), &tag_seen);
  if (rc == TBK_E2BIG) GError("Error: input too large for one tile\n");
  if (rc != 0) GError("Error: could not decode the chunks of %s the index names (%s %s): is the index the file's own?\n", infname.c_str(), tbk_strerror(rc), tbk_last_error(ctx));
  tbk_cov_in in;
  uint32_t n_kept = 0;
  rc = one ? tbk_region_view(ctx, &tile, tag_seen, U.tid[0], U.beg[0], U.end[0], &in, &n_kept) : tbk_regions_view(ctx, &tile, tag_seen, &regs, &in, &n_kept);
  if (rc == TBK_E2BIG) GError("Error: input too large for one tile\n");
  if (rc != 0) GError("Error: GPU region filter failed: %s (%s)\n", tbk_strerror(rc), tbk_last_error(ctx));
  const double ms_decode = ms();
  // file names and header lines as without -r
  tbh::TrackFiles tf;
  open_tracks(tf, hdr, covfname, jfname, sfname, bigwig, tabix);
  const TrackClip clip{&regs, one};
  write_tracks(ctx, hdr, in, num_samples, tf, &clip, bw_device, sj);
  tf.close();
  if (timing)
    fprintf(stderr, "tiecov %s phases ms: %u regions | index %.1f | chunk reads %.1f (%llu bytes in %u chunks) | context up at %.1f | decode + filter %.1f (%u of %u records) | tracks %.1f\n",
            one ? "-r" : "-R", R, ms_index, ms_read - ms_index, (unsigned long long)bytes_read, k, ms_ctx, ms_decode - ms_ctx, n_kept, tile.n_records, ms() - ms_decode);
  tbk_destroy(ctx);
  return 0;
}

int main(int argc, char* argv[]) {
  Args args(argc, argv, "help;verbose;version;region=;regions-file=;index-file=;bigwig-writer=;features=;summary=;tabix;DVWhc:s:j:r:R:");
  if (!args.error().empty()) {
    GMessage("%s\n%s\n", USAGE, args.error().c_str());
    return 1;
  }
  if (args.getOpt('h') || args.getOpt("help")) {
    GMessage("%s", USAGE);
    return 1;  // the reference exits 1 here (tiecov.cpp:535-538)
  }
  if (args.getOpt("version")) {
    fprintf(stdout, "%s\n", VERSION);
    return 0;
  }
  const bool tabix = args.getOpt("tabix") != nullptr;
  if (tabix && !args.getOpt('c') && !args.getOpt('s') && !args.getOpt('j')) GError("Error: --tabix needs at least one of -c / -j / -s (it applies to their tracks)\n");
  if ((args.getOpt("summary") != nullptr) != (args.getOpt("features") != nullptr))
    GError("Error: --features BED and --summary OUT.tsv go together (%s is missing)\n", args.getOpt("summary") ? "--features" : "--summary");
  if (!args.getOpt('c') && !args.getOpt('s') && !args.getOpt('j') && !args.getOpt("summary")) {
    GMessage("%s", USAGE);
    GMessage("\nError: at least one of -c/-j/-s arguments required!\n");
    return 1;
  }
  const bool bigwig = args.getOpt('W') != nullptr;
  if (tabix && !bigwig && args.getOpt('c') && (strcmp(args.getOpt('c'), "-") == 0 || strcmp(args.getOpt('c'), "stdout") == 0))
    GError("Error: --tabix needs a coverage file (-c PREFIX, not -c %s): an index addresses file offsets, standard output has none\n", args.getOpt('c'));
  if (args.getOpt("bigwig-writer") && !(bigwig && args.getOpt('c'))) GError("Error: --bigwig-writer needs -W (and -c)\n");
  const bool bw_device = args.getOpt("bigwig-writer") && tbh::parse_bigwig_writer(args.getOpt("bigwig-writer"));
  if (args.getOpt("verbose") || args.getOpt('V')) {
    fprintf(stderr, "Running TieCov " VERSION ". Command line:\n");
    args.printCmdLine(stderr);
  }
  std::string covfname = args.getOpt('c') ? args.getOpt('c') : "";
  std::string jfname = args.getOpt('j') ? args.getOpt('j') : "";
  std::string sfname = args.getOpt('s') ? args.getOpt('s') : "";
  if (args.startNonOpt() == 0) {
    GMessage("%s", USAGE);
    GMessage("\nError: no input file provided!\n");
    return 1;
  }
  std::string infname = args.nextNonOpt();
  GSamReader samreader(infname.c_str(), SAM_QNAME | SAM_FLAG | SAM_RNAME | SAM_POS | SAM_CIGAR | SAM_AUX);
  sam_hdr_t* hdr = samreader.header();
  tbh::SummaryJob sj;  // (--features / --summary: refused, where they are, before any output file exists)
  if (args.getOpt('r') || args.getOpt("region") || args.getOpt('R') || args.getOpt("regions-file") || args.getOpt("index-file")) {
    const auto t0 = std::chrono::steady_clock::now();
    if (count_region_opts(argc, argv) > 1) GError("Error: -r / --region given more than once (one region per run)\n");
    if (count_regions_file_opts(argc, argv) > 1) GError("Error: -R / --regions-file given more than once (one file of regions per run)\n");
    const char* r = args.getOpt('r') ? args.getOpt('r') : args.getOpt("region");
    const char* rf = args.getOpt('R') ? args.getOpt('R') : args.getOpt("regions-file");
    if (r && rf) GError("Error: -R / --regions-file and -r / --region do not go together\n");
    if (!r && !rf) GError("Error: --index-file needs -r REGION\n");
    const std::string index_file = args.getOpt("index-file") ? args.getOpt("index-file") : "";
    std::string err;
    tbh::RegionTable U;
    if (rf) {
      if (!tbh::regions_from_bed_file(*hdr, rf, U, err)) GError("Error: -R: %s\n", err.c_str());
    } else {
      int32_t rtid = 0;
      int64_t beg = 0, end = 0;
      if (!tbh::parse_region(*hdr, r, &rtid, &beg, &end, err)) GError("Error: %s\n", err.c_str());
      U.add(rtid, beg, end);
    }
    sj.setup(args.getOpt("features"), args.getOpt("summary"), *hdr, &U);
    return regions_main(hdr, infname, U, rf == nullptr, index_file, covfname, jfname, sfname, bigwig, bw_device, tabix, sj, t0);
  }
  sj.setup(args.getOpt("features"), args.getOpt("summary"), *hdr, nullptr);
  // file names and header lines: tracks.cpp (tiecov.cpp:365-402)
  tbh::TrackFiles tf;
  open_tracks(tf, hdr, covfname, jfname, sfname, bigwig, tabix);
  int num_samples = 0;
  if (tf.samp || tf.samp_tx.is_open()) {  // load_sample_info (commons.h:47-71)
    num_samples = (int)hdr->co_samples().size();
    if (num_samples == 0) GError("Error: no sample lines found in header");
  }
  // the HIP runtime takes ~0.2 s to come up: do that on a helper thread while the input is decoded
  tbk_ctx* ctx = nullptr;
  int dev = getenv("TBK_DEVICE") ? atoi(getenv("TBK_DEVICE")) : 0;
  int rc = 0;
  std::thread ctx_thread([&]() { rc = tbk_create(dev, &ctx); });
  // ---- decode to SoA (tiecov.cpp:482-485 defaults: YC absent -> 1.0, YX absent -> 1)
  tbh::BamFile* bf = samreader.file();
  {  // (the reader opened the header only: its records are inflated on demand, and this decode takes the whole file)
    std::string err;
    if (!bf->load(infname, err, std::max(1, tbh::cpu_budget()))) GError("Error: could not read %s (%s)\n", infname.c_str(), err.c_str());
  }
  size_t n = bf->n();
  std::vector<int32_t> tid(n), pos(n);
  std::vector<uint16_t> flag(n);
  std::vector<uint32_t> cig_off(n + 1, 0), cig;
  std::vector<double> yc(n, 1.0);
  std::vector<int64_t> yx(n, 1);
  std::vector<uint8_t> strand(n, '.');
  // pass 1 (serial, cheap): CIGAR offsets; pass 2 (threads): fields + one aux scan per record
  uint64_t ops = 0;
  for (size_t i = 0; i < n; ++i) {
    if (ops >= (1ull << 32)) break;
    cig_off[i] = (uint32_t)ops;
    ops += bf->rec(i).n_cigar();
  }
  if (ops >= (1ull << 32) || n >= (1ull << 32)) GError("Error: input too large for one tile\n");
  cig.resize(ops);
  uint64_t co = ops;
  {
    unsigned hw = (unsigned)tbh::cpu_budget();
    size_t nt = std::max<size_t>(1, std::min<size_t>(hw ? hw : 4, 32));
    if (n < 100000) nt = 1;
    auto work = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i) {
        tbh::RecView v = bf->rec(i);
        tid[i] = v.tid();
        pos[i] = v.pos();
        flag[i] = v.flag();
        uint32_t o = cig_off[i];
        for (uint32_t c = 0; c < v.n_cigar(); ++c) cig[o + c] = v.cigar(c);
        const uint8_t *a = v.aux_begin(), *e = v.aux_end();
        if (const uint8_t* s = tbh::aux_get(a, e, "YC")) yc[i] = tbh::aux2f(s);
        if (const uint8_t* s = tbh::aux_get(a, e, "YX")) yx[i] = tbh::aux2i(s);
        char xs = 0, ts = 0;
        if (const uint8_t* s = tbh::aux_get(a, e, "XS")) xs = (*s == 'A' || *s == 'Z') ? (char)s[1] : 0;
        if (!xs)
          if (const uint8_t* s = tbh::aux_get(a, e, "ts")) ts = (*s == 'A' || *s == 'Z') ? (char)s[1] : 0;
        char c = xs;
        if (c == 0 && (ts == '+' || ts == '-')) c = (flag[i] & 0x10) ? (ts == '+' ? '-' : '+') : ts;
        strand[i] = (uint8_t)((c == '+' || c == '-') ? c : '.');
      }
    };
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
    for (auto& x : th) x.join();
  }
  cig_off[n] = (uint32_t)co;

  ctx_thread.join();
  if (rc != 0) GError("Error: cannot use GPU %d (%s); this build has no CPU coverage path\n", dev, tbk_strerror(rc));
  tbk_cov_in in;
  memset(&in, 0, sizeof(in));
  in.mem = TBK_MEM_HOST;
  in.n_records = (uint32_t)n;
  in.n_cigar_ops = (uint32_t)co;
  in.tid = tid.data();
  in.pos = pos.data();
  in.flag = flag.data();
  in.cig_off = cig_off.data();
  in.cig = cig.data();
  in.yc = yc.data();
  in.strand = strand.data();
  in.yx = yx.data();
  write_tracks(ctx, hdr, in, num_samples, tf, nullptr, bw_device, sj);
  tf.close();
  tbk_destroy(ctx);
  return 0;
}
