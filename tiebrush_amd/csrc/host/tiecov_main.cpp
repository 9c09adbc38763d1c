// tiecov — drop-in command line of the reference's coverage tool (/root/reference/src/tiecov.cpp:345-573).
// The per-record loop (:435-499: bundles, addCov, addJunction, addMean, flushes) is replaced by
// tbk_coverage_tile / tbk_sample_tile (HIP); BAM decode and text output stay on the host.
// With -r REGION (no counterpart in the reference) only the chunks the file's index names for the region are read, and
// they are inflated, decoded, filtered, summarised and cut to the region on the device (regions_main below).
// With -R FILE the same for the region table of a BED file, in one run: the chunks are merged over the whole table.
// With --stream the file is read in batches of whole BGZF members, decoded on the device and cut at bundle heads
// (stream_main below): host and device memory are bounded by the batch and the largest bundle, not by the file.
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
#include "bgzf.h"
#include "stream_read.h"
#include "tracks.h"

#define VERSION "0.0.7"

static const char* USAGE =
    "TieCov v" VERSION " (MI355X build)\n"
    "Summarises a (TieBrush-collapsed) BAM file as BED-like tracks.\n"
    "\n"
    " usage: tiecov [-s out.sample] [-c out.coverage] [-j out.junctions] [--features BED --summary OUT.tsv] [--thresholds T1,T2,.. --depth-summary OUT.tsv] [--gtf FILE --transcripts OUT.tsv] [--strand-cov PREFIX] [-r REGION | -R FILE] [--stream] input.bam\n"
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
    "  --thresholds T1,T2,...   1 to 16 depths, decimal numbers > 0 in strictly ascending order, for the two tables below: the column ge_T\n"
    "               counts the bases whose coverage is >= T (the name is ge_ and the number as given)\n"
    "  --depth-summary OUT.tsv   bases at depth per reference: one line per @SQ in header order and a line `total`, with length, covered\n"
    "               bases, sum, mean0 = sum / length, mean = sum / covered, max and the ge_T columns (none without --thresholds).\n"
    "               Computed on the GPU from the rows of -c (TBK_SUMMARY_HOST=1: on this core); goes with --stream; not with -r / -R\n"
    "  --feature-depth OUT.tsv   with --features BED and --thresholds: one line per line of BED with size, covered bases and the ge_T\n"
    "               columns.  With -r / -R every feature must lie inside one interval of the region; not with --stream\n"
    "  --gtf FILE --transcripts OUT.tsv   per-transcript support: FILE is GTF (only its `exon` lines are read; transcript_id required,\n"
    "               gene_id optional; GFF3 is not read), one line of OUT.tsv per transcript in the order of first appearance: its span, id,\n"
    "               gene, strand, exons, length (exonic bases), covered, sum, mean0 = sum / length, mean = sum / covered and max of the\n"
    "               coverage over its exons, exons_hit (exons with a covered base), introns, introns_hit (introns that are a junction of\n"
    "               the track on the transcript's strand; '.' takes every strand), junc_min and junc_sum over its introns' junction values.\n"
    "               Computed on the GPU from the rows of -c / -j (TBK_SUMMARY_HOST=1: on this core).  With -r / -R every transcript's\n"
    "               span must lie inside one interval of the region; not with --stream\n"
    "  --strand-cov PREFIX   the coverage of each splice strand (the XS tag, else minimap2's ts turned round on a reverse read) in a file\n"
    "               of its own: PREFIX.plus.bedgraph, PREFIX.minus.bedgraph and PREFIX.none.bedgraph (every other record), each the file -c\n"
    "               writes for a BAM of that strand's mapped records alone.  The records are divided on the GPU (TBK_SPLIT_HOST=1: on this\n"
    "               core).  -W makes them .bigwig, --tabix .bedgraph.gz with an index each; goes with every other output, -r / -R and\n"
    "               --stream; PREFIX cannot be - / stdout\n"
    "  --stream [--tile-bytes N]   read input.bam in batches of whole BGZF members of about N compressed bytes (plain bytes, or K / M / G;\n"
    "               default 64M; --tile-bytes alone implies --stream), decode them on the GPU and write the tracks bundle by bundle: the same\n"
    "               bytes as without it, with memory bounded by a batch and the largest bundle.  With -c (also - / stdout), -j, -s, -W,\n"
    "               --tabix, --depth-summary; not with -r / -R / --index-file, --features / --summary / --feature-depth, --gtf / --transcripts,\n"
    "               --bigwig-writer device,\n"
    "               or SAM text input\n"
    " At least one of -c / -j / -s / --summary / --depth-summary / --feature-depth / --transcripts / --strand-cov is required.\n";

// ---- tiecov -r --------------------------------------------------------------------------------------------------------------------
// how often -r / --region is given (Args keeps the last value of a repeated option)
static int count_region_opts(int argc, char** argv) {
  static const char* const value_longs[] = {"index-file", "regions-file", "bigwig-writer", "features", "summary", "tile-bytes", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", "strand-cov", nullptr};
  return count_value_option(argc, argv, "region", 'r', value_longs, "csjR");
}
static int count_regions_file_opts(int argc, char** argv) {
  static const char* const value_longs[] = {"index-file", "region", "bigwig-writer", "features", "summary", "tile-bytes", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", "strand-cov", nullptr};
  return count_value_option(argc, argv, "regions-file", 'R', value_longs, "csjr");
}
static int count_strand_cov_opts(int argc, char** argv) {
  static const char* const value_longs[] = {"index-file", "region", "regions-file", "bigwig-writer", "features", "summary", "tile-bytes", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", nullptr};
  return count_value_option(argc, argv, "strand-cov", 0, value_longs, "csjrR");
}

// ---- what every run does with its records: the tracks (tracks.cpp: run_tracks) ----------------------------------------------------
// file names and header lines: tracks.cpp (tiecov.cpp:365-402)
static void open_tracks(tbh::TrackFiles& tf, sam_hdr_t* hdr, const tbh::TrackOptions& o) { tf.open(o, hdr->target_name, hdr->target_len); }

// the device entry points for run_tracks: this binary links libtbk.so
static tbh::TrackApi linked_track_api(tbk_ctx* ctx) {
  tbh::TrackApi a;
  a.ctx = ctx;
  a.coverage_tile = tbk_coverage_tile, a.sample_tile = tbk_sample_tile;
  a.cov_clip = tbk_cov_clip, a.cov_clip_regions = tbk_cov_clip_regions, a.sample_clip = tbk_sample_clip, a.sample_clip_regions = tbk_sample_clip_regions;
  a.track_names = tbk_track_names, a.format_track = tbk_format_track, a.track_bgzf = tbk_track_bgzf, a.bigwig_build = tbk_bigwig_build;
  a.cov_summary = tbk_cov_summary, a.cov_thresholds = tbk_cov_thresholds, a.tx_summary = tbk_tx_summary, a.cov_split_strand = tbk_cov_split_strand;
  a.strerror_ = tbk_strerror, a.last_error = tbk_last_error;
  return a;
}

// The tracks of `in` into the open files of tf, and the files closed; the plain text stays on the host formatter.
static void write_run(tbk_ctx* ctx, sam_hdr_t* hdr, const tbk_cov_in& in, int num_samples, tbh::TrackFiles& tf, const tbh::TrackClip* clip, bool bw_device,
                      const tbh::SummaryJob& sj, const tbh::DepthJob& dj, const tbh::TxJob& xj) {
  tbh::TrackRun run;
  run.clip = clip, run.num_samples = num_samples, run.bw_device = bw_device, run.summary = &sj, run.depth = &dj, run.transcripts = &xj;
  tbh::run_tracks(linked_track_api(ctx), in, hdr->target_name, tf, run);
}

// The run of -r (one: U is the region itself, which may be empty, and goes through the one-region entries) and of -R (U is the
// normalised table of the BED file, through the table entries): every other statement is shared.
static int regions_main(sam_hdr_t* hdr, const std::string& infname, const tbh::RegionTable& U, bool one, const std::string& index_file,
                        const tbh::TrackOptions& topt, const tbh::SummaryJob& sj, const tbh::DepthJob& dj, const tbh::TxJob& xj, const std::chrono::steady_clock::time_point t0) {
  const bool timing = getenv("TBK_TIMING") != nullptr;
  auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  // every refusal comes before an output file exists
  std::string err;
  const uint32_t R = (uint32_t)U.n();
  tbk_regions regs;
  regs.n = R, regs.tid = U.tid.data(), regs.beg = U.beg.data(), regs.end = U.end.data();
  int num_samples = 0;
  if (!topt.samp.empty()) {
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
  open_tracks(tf, hdr, topt);
  const tbh::TrackClip clip{&regs, one};
  write_run(ctx, hdr, in, num_samples, tf, &clip, topt.bw_device, sj, dj, xj);
  if (timing)
    fprintf(stderr, "tiecov %s phases ms: %u regions | index %.1f | chunk reads %.1f (%llu bytes in %u chunks) | context up at %.1f | decode + filter %.1f (%u of %u records) | tracks %.1f\n",
            one ? "-r" : "-R", R, ms_index, ms_read - ms_index, (unsigned long long)bytes_read, k, ms_ctx, ms_decode - ms_ctx, n_kept, tile.n_records, ms() - ms_decode);
  tbk_destroy(ctx);
  return 0;
}

// ---- tiecov --stream -----------------------------------------------------------------------------------------------
// "N", "NK", "NM", "NG" -> bytes; false: not a size
static bool parse_size(const char* v, uint64_t* out) {
  char* e = nullptr;
  const unsigned long long n = strtoull(v, &e, 10);
  if (e == v || *v == '-') return false;
  uint64_t mul = 1;
  if (*e == 'K' || *e == 'k') mul = 1ull << 10, ++e;
  else if (*e == 'M' || *e == 'm') mul = 1ull << 20, ++e;
  else if (*e == 'G' || *e == 'g') mul = 1ull << 30, ++e;
  if (*e) return false;
  *out = (uint64_t)n * mul;
  return true;
}

// The whole file in batches: reader -> tbk_bam_decode_open -> tbk_cov_stream_push -> the rows of the view into the open files.  Every
// refusal of the option rules came before this; from the first file on, a failure removes what was written (standard output is what it is).
static int stream_main(sam_hdr_t* hdr, const std::string& infname, uint64_t tile_bytes, const tbh::TrackOptions& topt, const tbh::DepthJob& dj) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  auto ms_since = [](clock::time_point a) { return std::chrono::duration<double, std::milli>(clock::now() - a).count(); };
  int num_samples = 0;
  if (!topt.samp.empty()) {
    num_samples = (int)hdr->co_samples().size();
    if (num_samples == 0) GError("Error: no sample lines found in header");
  }
  tbk_ctx* ctx = nullptr;
  const int dev = getenv("TBK_DEVICE") ? atoi(getenv("TBK_DEVICE")) : 0;
  int rc = 0;
  std::thread ctx_thread([&]() { rc = tbk_create(dev, &ctx); });
  tbh::StreamReader rd;
  std::string err;
  const bool opened = rd.open(infname, tile_bytes, err);
  ctx_thread.join();
  if (!opened) GError("Error: %s\n", err.c_str());
  if (rc != 0) GError("Error: cannot use GPU %d (%s); this build has no CPU coverage path\n", dev, tbk_strerror(rc));
  tbh::TrackFiles tf;
  open_tracks(tf, hdr, topt);
  auto fail = [&](const std::string& msg) {
    tf.discard();
    GError("Error: %s\n", msg.c_str());
  };
  tbh::TrackRun run;
  run.num_samples = num_samples, run.depth = &dj;
  const tbh::TrackApi api = linked_track_api(ctx);
  tbh::TrackStream ts(api, hdr->target_name, tf, run);
  double ms_decode = 0, ms_push = 0, ms_tracks = 0;
  uint32_t largest_carry = 0;
  uint64_t n_batches = 0;
  bool ended = false;
  auto push = [&](const tbk_soa_in& tile, const uint8_t* seen, bool last) {
    tbk_cov_in view;
    tbk_cov_stream_info info;
    auto a = clock::now();
    const int prc = tbk_cov_stream_push(ctx, &tile, seen, last ? 1 : 0, &view, &info);
    ms_push += ms_since(a);
    if (prc == TBK_E2BIG) {  // (info names the first record of the bundle that did not fit)
      const bool known = info.first_tid >= 0 && info.first_tid < hdr->n_targets;
      fail("bundle too large for one tile: the bundle of " + infname + " that begins at " +
           (known ? hdr->target_name[(size_t)info.first_tid] + ":" + std::to_string((long long)info.first_pos + 1) : std::string("an unplaced record")) +
           " and the next batch exceed what one call can take");
    }
    if (prc != 0) fail(std::string("GPU stream cut failed: ") + tbk_strerror(prc) + " (" + tbk_last_error(ctx) + ")");
    largest_carry = std::max(largest_carry, info.n_carry);
    if (view.n_records == 0 && !last) return;  // (the open bundle goes on: nothing to write yet)
    if (view.n_records == 0) memset(&view, 0, sizeof(view)), view.mem = TBK_MEM_HOST;  // (no record at all: the empty input of a whole-file run)
    a = clock::now();
    ts.tile(view, last);
    ms_tracks += ms_since(a);
    ended = last;
  };
  tbh::StreamBatch b;
  while (rd.next(b, err)) {
    ++n_batches;
    tbk_soa_in tile;
    const uint8_t* seen = nullptr;
    uint64_t tail = 0;
    auto a = clock::now();
    rc = tbk_bam_decode_open(ctx, b.z.data(), b.z.size(), b.first_uoff, hdr->n_targets, &tile, &seen, &tail);
    ms_decode += ms_since(a);
    if (rc == TBK_E2BIG) fail("input too large for one tile (a batch of " + infname + " holds 2^32 records: use a smaller --tile-bytes)");
    if (rc != 0) fail("could not decode " + infname + " (" + tbk_strerror(rc) + " " + tbk_last_error(ctx) + ")");
    if (!rd.advance(b, tail, err)) fail(err);
    push(tile, seen, b.last);
  }
  if (!err.empty()) fail(err);
  if (!ended) {  // (the file ended on a batch's edge, or holds no record: what is still open goes out now)
    tbk_soa_in none;
    memset(&none, 0, sizeof(none));
    none.mem = TBK_MEM_DEVICE;
    push(none, nullptr, true);
  }
  ts.end();
  if (getenv("TBK_TIMING"))
    fprintf(stderr, "tiecov --stream phases ms: %llu batches of about %llu bytes (%llu tiles written) | %llu bytes read | %llu bytes inflated twice | largest carry %u records | decode %.1f | push %.1f | tracks %.1f | total %.1f\n",
            (unsigned long long)n_batches, (unsigned long long)tile_bytes, (unsigned long long)ts.tiles(), (unsigned long long)rd.bytes_read(),
            (unsigned long long)rd.reinflated(), largest_carry, ms_decode, ms_push, ms_tracks, ms_since(t0));
  tbk_destroy(ctx);
  return 0;
}

int main(int argc, char* argv[]) {
  Args args(argc, argv, "help;verbose;version;region=;regions-file=;index-file=;bigwig-writer=;features=;summary=;thresholds=;depth-summary=;feature-depth=;gtf=;transcripts=;strand-cov=;tabix;stream;tile-bytes=;DVWhc:s:j:r:R:");
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
  const char* strand_cov = args.getOpt("strand-cov");
  tbh::check_strand_cov(strand_cov, count_strand_cov_opts(argc, argv), 1);
  if (tabix && !args.getOpt('c') && !args.getOpt('s') && !args.getOpt('j') && !strand_cov) GError("Error: --tabix needs at least one of -c / -j / -s (it applies to their tracks)\n");
  // (--features serves --summary and --feature-depth: with neither, today's sentence)
  if (args.getOpt("summary") ? !args.getOpt("features") : (args.getOpt("features") && !args.getOpt("feature-depth")))
    GError("Error: --features BED and --summary OUT.tsv go together (%s is missing)\n", args.getOpt("summary") ? "--features" : "--summary");
  if (args.getOpt("transcripts") ? !args.getOpt("gtf") : args.getOpt("gtf") != nullptr)
    GError("Error: --gtf FILE and --transcripts OUT.tsv go together (%s is missing)\n", args.getOpt("transcripts") ? "--gtf" : "--transcripts");
  if (!args.getOpt('c') && !args.getOpt('s') && !args.getOpt('j') && !args.getOpt("summary") && !args.getOpt("depth-summary") && !args.getOpt("feature-depth") &&
      !args.getOpt("transcripts") && !strand_cov) {
    GMessage("%s", USAGE);
    GMessage("\nError: at least one of -c/-j/-s arguments required!\n");
    return 1;
  }
  const bool bigwig = args.getOpt('W') != nullptr;
  if (tabix && !bigwig && args.getOpt('c') && (strcmp(args.getOpt('c'), "-") == 0 || strcmp(args.getOpt('c'), "stdout") == 0))
    GError("Error: --tabix needs a coverage file (-c PREFIX, not -c %s): an index addresses file offsets, standard output has none\n", args.getOpt('c'));
  if (args.getOpt("bigwig-writer") && !(bigwig && (args.getOpt('c') || strand_cov))) GError("Error: --bigwig-writer needs -W (and -c)\n");
  tbh::TrackOptions topt;
  topt.bigwig = bigwig, topt.tabix = tabix;
  topt.bw_device = args.getOpt("bigwig-writer") && tbh::parse_bigwig_writer(args.getOpt("bigwig-writer"));
  if (args.getOpt("verbose") || args.getOpt('V')) {
    fprintf(stderr, "Running TieCov " VERSION ". Command line:\n");
    args.printCmdLine(stderr);
  }
  topt.cov = args.getOpt('c') ? args.getOpt('c') : "";
  topt.junc = args.getOpt('j') ? args.getOpt('j') : "";
  topt.samp = args.getOpt('s') ? args.getOpt('s') : "";
  topt.strand_cov = strand_cov ? strand_cov : "";
  if (args.startNonOpt() == 0) {
    GMessage("%s", USAGE);
    GMessage("\nError: no input file provided!\n");
    return 1;
  }
  std::string infname = args.nextNonOpt();
  // --stream: what it does not go with is refused here, before the input is opened and any file exists
  const bool stream = args.getOpt("stream") || args.getOpt("tile-bytes");
  uint64_t tile_bytes = (uint64_t)64 << 20;  // (the default is not measured yet: DESIGN.md 4k)
  if (stream) {
    if (args.getOpt("tile-bytes") && !parse_size(args.getOpt("tile-bytes"), &tile_bytes))
      GError("Error: --tile-bytes takes a size in bytes, or with a K / M / G suffix (got '%s')\n", args.getOpt("tile-bytes"));
    if (args.getOpt('r') || args.getOpt("region") || args.getOpt('R') || args.getOpt("regions-file") || args.getOpt("index-file"))
      GError("Error: --stream and -r / -R / --index-file do not go together (a region run reads only the region's chunks)\n");
    if (args.getOpt("features") || args.getOpt("summary"))
      GError("Error: --stream and --features / --summary do not go together (a feature across two tiles needs a carried partial sum)\n");
    if (args.getOpt("gtf") || args.getOpt("transcripts"))
      GError("Error: --stream and --gtf / --transcripts do not go together (a transcript can lie across the seam of two tiles)\n");
    if (topt.bw_device) GError("Error: --stream and --bigwig-writer device do not go together (the device writer takes all rows at once)\n");
    tbh::refuse_split_host_on_device(strand_cov, "--stream");
    if (!tbh::bgzf_probe(infname)) GError("Error: --stream needs a BAM file (BGZF); %s is SAM text or cannot be read\n", infname.c_str());
  }
  GSamReader samreader(infname.c_str(), SAM_QNAME | SAM_FLAG | SAM_RNAME | SAM_POS | SAM_CIGAR | SAM_AUX);
  sam_hdr_t* hdr = samreader.header();
  tbh::SummaryJob sj;  // (--features / --summary: refused, where they are, before any output file exists)
  tbh::DepthJob dj;    // (--thresholds / --depth-summary / --feature-depth: the same)
  tbh::TxJob xj;       // (--gtf / --transcripts: the same)
  const char* sum_features = args.getOpt("summary") ? args.getOpt("features") : nullptr;
  if (args.getOpt('r') || args.getOpt("region") || args.getOpt('R') || args.getOpt("regions-file") || args.getOpt("index-file")) {
    const auto t0 = std::chrono::steady_clock::now();
    tbh::refuse_split_host_on_device(strand_cov, "-r / -R");
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
    sj.setup(sum_features, args.getOpt("summary"), *hdr, &U);
    dj.setup(args.getOpt("thresholds"), args.getOpt("depth-summary"), args.getOpt("feature-depth"), args.getOpt("features"), *hdr, &U);
    xj.setup(args.getOpt("gtf"), args.getOpt("transcripts"), *hdr, &U);
    return regions_main(hdr, infname, U, rf == nullptr, index_file, topt, sj, dj, xj, t0);
  }
  dj.setup(args.getOpt("thresholds"), args.getOpt("depth-summary"), args.getOpt("feature-depth"), args.getOpt("features"), *hdr, nullptr);
  if (stream) return stream_main(hdr, infname, tile_bytes, topt, dj);
  sj.setup(sum_features, args.getOpt("summary"), *hdr, nullptr);
  xj.setup(args.getOpt("gtf"), args.getOpt("transcripts"), *hdr, nullptr);
  // file names and header lines: tracks.cpp (tiecov.cpp:365-402)
  tbh::TrackFiles tf;
  open_tracks(tf, hdr, topt);
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
  const size_t n = bf->n();
  if (n >= (1ull << 32)) GError("Error: input too large for one tile\n");
  const unsigned hw = (unsigned)tbh::cpu_budget();
  const int nt = n < 100000 ? 1 : (int)std::max<size_t>(1, std::min<size_t>(hw ? hw : 4, 32));
  tbh::CovRecs recs;
  const bool fits = recs.append((uint32_t)n, [&](uint32_t i) { return bf->rec(i); },
                                [](uint32_t, const tbh::RecView& v, double* yc, int64_t* yx) {
                                  const uint8_t *a = v.aux_begin(), *e = v.aux_end();
                                  const uint8_t* s = tbh::aux_get(a, e, "YC");
                                  *yc = s ? tbh::aux2f(s) : 1.0;
                                  s = tbh::aux_get(a, e, "YX");
                                  *yx = s ? tbh::aux2i(s) : 1;
                                },
                                nt);
  if (!fits) GError("Error: input too large for one tile\n");

  ctx_thread.join();
  if (rc != 0) GError("Error: cannot use GPU %d (%s); this build has no CPU coverage path\n", dev, tbk_strerror(rc));
  write_run(ctx, hdr, recs.as_cov_in(), num_samples, tf, nullptr, topt.bw_device, sj, dj, xj);
  tbk_destroy(ctx);
  return 0;
}
