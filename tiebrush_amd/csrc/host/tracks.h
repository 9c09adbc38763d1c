// tracks.h — tiecov's three track files, shared by the tiecov command line and by `tiebrush --cov / --junc / --samp`: file names and
// header lines (tiecov.cpp:365-402 and the openings around them), and the host formatter of the lines (flushCoverage :237,
// CJunc::write :91-95, flushCoverage(pair) :289).  The host formatter is what tiecov prints with, the reference the device formatter
// (tbk_format_track) is tested against, and the command line's fallback when the device formatter refuses a track.  And what both do
// with their records: the record table (CovRecs) and the one run from it to the closed files (run_tracks).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/tbk.h"
#include "bai_read.h"
#include "bigwig.h"
#include "bgzf.h"
#include "tabix.h"

namespace tbh {

// The device entry points of a track run, as a command line has them: tracks.cpp and tabix.cpp are linked without libtbk.so (tbh_tool,
// libtbh.so), tiecov links the library and tiebrush binds it at run time, so the calls travel as pointers.  An entry the library in use
// lacks is null (tiebrush: track_bgzf, bigwig_build, cov_summary, cov_thresholds, tx_summary may be; it never clips, and leaves the four clip entries null).
struct TrackApi {
  tbk_ctx* ctx = nullptr;
  decltype(&tbk_coverage_tile) coverage_tile = nullptr;
  decltype(&tbk_sample_tile) sample_tile = nullptr;
  decltype(&tbk_cov_clip) cov_clip = nullptr;
  decltype(&tbk_cov_clip_regions) cov_clip_regions = nullptr;
  decltype(&tbk_sample_clip) sample_clip = nullptr;
  decltype(&tbk_sample_clip_regions) sample_clip_regions = nullptr;
  decltype(&tbk_track_names) track_names = nullptr;
  decltype(&tbk_format_track) format_track = nullptr;
  decltype(&tbk_track_bgzf) track_bgzf = nullptr;
  decltype(&tbk_bigwig_build) bigwig_build = nullptr;
  decltype(&tbk_cov_summary) cov_summary = nullptr;
  decltype(&tbk_strerror) strerror_ = nullptr;
  decltype(&tbk_last_error) last_error = nullptr;
  decltype(&tbk_cov_thresholds) cov_thresholds = nullptr;
  decltype(&tbk_tx_summary) tx_summary = nullptr;
  decltype(&tbk_cov_split_strand) cov_split_strand = nullptr;  // (the last field: a table filled in field by field without it stays valid)
};

// The track options of a command line (tiecov -c / -j / -s / -W / --bigwig-writer / --tabix and tiebrush's long spellings of them; each
// main checks their rules in its own words).  An empty prefix: that track is not written.
struct TrackOptions {
  std::string cov, junc, samp;
  std::string strand_cov;  // --strand-cov PREFIX: the coverage of each splice strand in a file of its own
  bool bigwig = false, bw_device = false, tabix = false;
};
// `--strand-cov PREFIX` as both command lines refuse it, before any file exists: a prefix of - / stdout (three tracks do not share one
// standard output), the option given twice (`times`: how often the command line holds it), --ranks (`ranks` > 1).  Errors are fatal.
void check_strand_cov(const char* prefix, int times, int ranks);
// TBK_SPLIT_HOST=1 (anything but "0"): the records are divided by split_strand_host.  That loop reads host arrays, so a run whose records
// stay on the device (`what`: "-r / -R", "--stream") refuses the variable with --strand-cov — here, before any file exists (GError)
bool split_host_asked();
void refuse_split_host_on_device(const char* prefix, const char* what);
// "host" / "device" -> false / true; anything else is fatal (GError)
bool parse_bigwig_writer(const char* value);

// one coverage sink of --strand-cov: what the coverage track itself has
struct CovSink {
  FILE* f = nullptr;
  BigWigWriter bw;
  bool is_bw = false;
  TabixWriter tx;
  std::string name;
  bool on() const { return f || is_bw || tx.is_open(); }
};
extern const char* const kStrandSuffix[3];  // ".plus", ".minus", ".none": PREFIX<suffix>.bedgraph / .bigwig / .bedgraph.gz

// The open track files.  Coverage goes to stdout for "-" / "stdout", to PREFIX.bigwig with `bigwig`, else to PREFIX.bedgraph; junctions to PREFIX.bed; the sample counts to PREFIX.bedgraph.  Errors are fatal (GError).
// With `tabix` every text track is PREFIX.bedgraph.gz / PREFIX.bed.gz (BGZF) with its tabix index beside it (tabix.h): the track's
// TabixWriter is open in the place of its FILE*, and takes the header line with its first rows.
struct TrackFiles {
  FILE *cov = nullptr, *junc = nullptr, *samp = nullptr;
  BigWigWriter bw;
  bool cov_bw = false;
  std::vector<uint32_t> bw_lens;  // the chromosome lengths the bigWig was opened with
  std::string cov_name, junc_name, samp_name;  // (junc / samp: the plain files; a tabix track's name is its writer's)
  TabixWriter cov_tx, junc_tx, samp_tx;  // --tabix
  CovSink strand[3];  // --strand-cov: the records with splice strand '+', '-', and every other, each a coverage track under -c's rules
  bool strand_on() const { return strand[0].on() || strand[1].on() || strand[2].on(); }
  // write_bigwig for the sink of class s
  void write_strand_bigwig(int s, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const TrackApi* dev);
  void open(const TrackOptions& o, const std::vector<std::string>& names, const std::vector<uint32_t>& lens);
  void close_bigwig();  // (after every interval went to bw)
  // The coverage rows into the bigWig and the file closed (flushCoverage(bigWigFile_t*), tiecov.cpp:243-275: the value as a float).
  // dev == nullptr: the host producer.  Else the sections are dev->bigwig_build's; a refusal of that call other than a failed write
  // hands the file to the host producer (a line on stderr says so).  TBK_TIMING: a "bigwig phase" line on stderr for either.
  void write_bigwig(uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const TrackApi* dev);
  void close();
  void discard();  // a run that failed: every file closed and removed (standard output is what it is)
};

// Text output: the lines are independent, so slices of them are formatted by worker threads and written in order.
// fmt(i, buf, cap) is snprintf-like: it returns the line's length even when that is more than cap.
template <class F>
void emit_lines(FILE* f, uint32_t n, F fmt);

// the three formats, as the reference prints them
int fmt_cov_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, double val);
int fmt_junc_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, int number, double val, char strand);
int fmt_samp_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, int64_t count, float heat);

// whole tracks from row arrays (first_junc: the JUNC number of row 0)
void emit_cov_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                    const double* val);
void emit_junc_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                     const double* val, const uint8_t* strand, int64_t first_junc);
void emit_samp_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                     const int64_t* count, const float* heat);

void GErrorWrite();  // [[noreturn]]: "failed to write an output line"

// ---- `--features BED --summary OUT`: the rows of a coverage call read against features --------------------------------
// what tbk_cov_summary computes, one element per feature
struct FeatSummary {
  std::vector<uint64_t> covered;
  std::vector<double> sum, max, junc;
  void resize(size_t n) { covered.assign(n, 0), sum.assign(n, 0.0), max.assign(n, 0.0), junc.assign(n, 0.0); }
};
// The host summariser (TBK_SUMMARY_HOST=1, `tbh_tool summary`): plain loops over host rows, tbk_cov_summary's contract — interval rows
// sorted by (tid, start) and disjoint, junction rows sorted by (tid, start, end, strand); a feature's products are added in row order.
// want_cov / want_junc false: those columns stay zero.
void summarise_features(const FeatureTable& F, bool want_cov, uint32_t ni, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val,
                        bool want_junc, uint32_t nj, const int32_t* jtid, const int32_t* jstart, const int32_t* jend, const uint8_t* jstrand, const double* jval,
                        FeatSummary& S);
// the summary file: the header line, then one line per feature in the table's order; mean0 = sum / size, mean = sum / covered (0 when
// nothing is covered), in double.  false: the file cannot be created or written
bool write_summary_tsv(const std::string& path, const std::vector<std::string>& names, const FeatureTable& F, const FeatSummary& S, std::string& err);

// `--features BED --summary OUT` of a run: parsed (and refused) before any output file exists, written by write_summary
struct SummaryJob {
  std::string bed, out;
  FeatureTable F;
  bool on() const { return !out.empty(); }
  // The two options' rules and the BED file against the header (and, in a region run, against its normalised table U: every feature
  // wholly inside one interval).  Errors are fatal (GError) and name the line.
  void setup(const char* features_opt, const char* summary_opt, const BamHeader& hdr, const RegionTable* U);
};
// The summary of HOST rows (what tbk_coverage_tile wrote, before any clip) into job.out: api.cov_summary, or the host summariser with
// TBK_SUMMARY_HOST=1.  Errors are fatal; a missing tbk_cov_summary is one.  TBK_TIMING: a "summary phase ms" line.
void write_summary(const SummaryJob& job, const std::vector<std::string>& names, const tbk_cov_out& rows, const TrackApi& api);

// ---- `--thresholds T1,.. --depth-summary OUT` / `--feature-depth OUT`: bases at depth ----------------------------------
// "T1,T2,..": 1 to 16 decimal numbers, each parsed completely by strtod, finite, > 0, strictly ascending; text[k] is item k as given
// (the column's name is ge_<text>).  false: err names the offending item
bool parse_thresholds(const char* list, std::vector<double>& thr, std::vector<std::string>& text, std::string& err);
// The host form of tbk_cov_thresholds (TBK_SUMMARY_HOST=1, `tbh_tool depth`): a plain loop per feature over host rows sorted by
// (tid, start) and disjoint.  covered [n] (may be null), ge [n][n_thr] feature-major; the comparison val >= thr[k] on the doubles
void threshold_features(size_t n, const int32_t* ftid, const int64_t* fbeg, const int64_t* fend, uint32_t ni, const int32_t* tid, const int32_t* start,
                        const int32_t* end, const double* val, const double* thr, uint32_t n_thr, uint64_t* covered, uint64_t* ge);
// the per-reference table of a run: one element per @SQ in header order, added up over the tiles of a streamed run (the integers by
// integer addition, max by max, sum by double addition in tile order)
struct DepthTable {
  std::vector<uint64_t> covered, ge;  // ge [n_ref][n_thr]
  std::vector<double> sum, max;
  void resize(size_t n_ref, size_t n_thr) { covered.assign(n_ref, 0), ge.assign(n_ref * n_thr, 0), sum.assign(n_ref, 0.0), max.assign(n_ref, 0.0); }
};
// `#chrom length covered sum mean0 mean max ge_T1 ..`: one line per reference, then `total` (the integers added, the sums added in
// header order, the largest max; mean0 = sum / length and mean = sum / covered, 0 where the divisor is).  false: the file cannot be
// created or written (and is removed)
bool write_depth_tsv(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::vector<std::string>& thr_text,
                     const DepthTable& D, std::string& err);
// `#chrom start end name strand size covered ge_T1 ..`: one line per feature in the table's order
bool write_feature_depth_tsv(const std::string& path, const std::vector<std::string>& names, const FeatureTable& F, const std::vector<std::string>& thr_text,
                             const uint64_t* covered, const uint64_t* ge, std::string& err);

// the three options of a run: parsed (and refused) before a device is touched or any output file exists; the files are written by
// TrackStream::end, so a run that fails leaves neither
struct DepthJob {
  std::string summary_out, feature_out, bed;
  std::vector<double> thr;
  std::vector<std::string> thr_text;
  std::vector<uint32_t> lens;  // the references' lengths, header order
  FeatureTable F;              // --feature-depth
  bool per_ref() const { return !summary_out.empty(); }
  bool per_feature() const { return !feature_out.empty(); }
  bool on() const { return per_ref() || per_feature(); }
  // The options' rules (each refusal its own sentence), the threshold list, the BED file against the header and — in a region run,
  // which U != null says — the refusal of --depth-summary and every feature wholly inside one interval.  Errors are fatal (GError).
  void setup(const char* thresholds_opt, const char* depth_opt, const char* feature_depth_opt, const char* features_opt, const BamHeader& hdr, const RegionTable* U);
};

// ---- `--gtf FILE --transcripts OUT`: per-transcript support -----------------------------------------------------------
// what tbk_tx_summary computes: one element per transcript, and the parts per exon (in_junc: the intron BEHIND the exon, 0 for a last one)
struct TxSummary {
  std::vector<uint64_t> covered, ex_covered;
  std::vector<double> sum, max, junc_min, junc_sum, ex_sum, ex_max, in_junc;
  std::vector<uint32_t> exons_hit, introns_hit;
  void resize(size_t n_tx, size_t n_exon) {
    covered.assign(n_tx, 0), sum.assign(n_tx, 0.0), max.assign(n_tx, 0.0), junc_min.assign(n_tx, 0.0), junc_sum.assign(n_tx, 0.0);
    exons_hit.assign(n_tx, 0), introns_hit.assign(n_tx, 0);
    ex_covered.assign(n_exon, 0), ex_sum.assign(n_exon, 0.0), ex_max.assign(n_exon, 0.0), in_junc.assign(n_exon, 0.0);
  }
};
// The host summariser (TBK_SUMMARY_HOST=1, `tbh_tool transcripts`): tbk_tx_summary's contract by plain loops — summarise_features over
// the exons and over the introns, then a transcript's parts added in exon order.  want_cov / want_junc false: those columns stay zero.
void summarise_transcripts(const TranscriptTable& X, bool want_cov, uint32_t ni, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val,
                           bool want_junc, uint32_t nj, const int32_t* jtid, const int32_t* jstart, const int32_t* jend, const uint8_t* jstrand, const double* jval,
                           TxSummary& S);
// `#chrom start end transcript gene strand exons length covered sum mean0 mean max exons_hit introns introns_hit junc_min junc_sum`: one
// line per transcript in the table's order; start / end are the first exon's begin and the last exon's end, length the exonic bases,
// mean0 = sum / length, mean = sum / covered (0 when nothing is covered), in double.  false: the file cannot be created or written (and
// is removed)
bool write_transcripts_tsv(const std::string& path, const std::vector<std::string>& names, const TranscriptTable& X, const TxSummary& S, std::string& err);

// the two options of a run: parsed (and refused) before a device is touched or any output file exists; the file is written by
// TrackStream::end behind the closed tracks, so a run that fails leaves none
struct TxJob {
  std::string gtf, out;
  TranscriptTable X;
  bool on() const { return !out.empty(); }
  // The two options' rules and the GTF file against the header (and, in a region run, against its normalised table U: every
  // transcript's span wholly inside one interval).  Errors are fatal (GError) and name the line.
  void setup(const char* gtf_opt, const char* transcripts_opt, const BamHeader& hdr, const RegionTable* U);
};

// ---- what every run does with its records: the tracks -----------------------------------------------------------------------------
// The records of a run as tbk_coverage_tile / tbk_sample_tile read them (host arrays): tiecov's decode of its input, tiebrush's groups
// as they go into the output.
struct CovRecs {
  std::vector<int32_t> tid, pos;
  std::vector<uint16_t> flag;
  std::vector<uint32_t> cig_off{0}, cig;
  std::vector<double> yc;
  std::vector<int64_t> yx;
  std::vector<uint8_t> strand;
  tbk_cov_in as_cov_in() const;  // (an empty flag column travels as NULL: every record counts)
  // ng further records, rec(g) in file order: tid, pos, flag and the splice strand (bam.h) on `threads` workers, the CIGAR offsets by
  // one serial pass over the counts, then the operations on the workers again.  values(g, view, &yc, &yx) gives a record's weights.
  // false: the CIGAR operations of all records no longer fit 32 bits (the message is the caller's)
  bool append(uint32_t ng, const std::function<RecView(uint32_t)>& rec, const std::function<void(uint32_t, const RecView&, double*, int64_t*)>& values,
              int threads);
};

// tbk_cov_split_strand's rule by a plain loop over HOST arrays (TBK_SPLIT_HOST=1, libtbh's tbh_split_strand_host): out[0] the mapped
// records (flag bit 0x4 clear; no flag column: all) with strand '+', out[1] '-', out[2] every other byte, each in the input's order with
// its CIGAR CSR rebuilt from 0 and no flag column; yc / yx are copied where the input has them
void split_strand_host(const tbk_cov_in& in, CovRecs out[3]);

// the cut of a region run: the table, through the one-region entries (one: the table is the region itself, which may be empty) or the
// table entries
struct TrackClip {
  const tbk_regions* U;
  bool one;
};
// the figures of tiebrush's "tracks ms:" line
struct TrackTimes {
  double ms_cov = 0, ms_samp = 0, ms_text = 0;  // the coverage call, the sample call, text + write of every track
  int host_tracks = 0;                           // plain-text tracks that the host formatter wrote
};
struct TrackRun {
  const TrackClip* clip = nullptr;
  int num_samples = 0;
  bool bw_device = false;                // the bigWig's sections by api.bigwig_build
  const SummaryJob* summary = nullptr;   // (null, or a job that is not on: no summary)
  const DepthJob* depth = nullptr;       // (the same for --depth-summary / --feature-depth)
  const TxJob* transcripts = nullptr;    // (the same for --gtf / --transcripts)
  bool device_text = false;              // plain text by api.format_track (the names set up front), the host formatter where it refuses a track
  TrackTimes* times = nullptr;
};
// The rows of coverage_tile / sample_tile for `in` (host arrays, or a device view), cut to *run.clip where one is given, into the open
// files of tf, and the files closed.  An input of no records goes the same way: the calls give no rows and status 0.  With a summary
// or a transcripts job the coverage and junction rows are computed whatever tracks are open, and summarised before the cut (DESIGN.md
// 4j, 4m).  The
// reference names go to the context (track_names) at most once: up front with device_text, else before the first tabix track the
// device writes.  Errors are fatal (GError).
void run_tracks(const TrackApi& api, const tbk_cov_in& in, const std::vector<std::string>& names, TrackFiles& tf, const TrackRun& run);

// run_tracks in three steps, for a record stream that arrives in tiles cut at bundle heads: the rows of the tiles, one
// after the other, are the rows of the uncut stream, so every tile's lines are appended to the open files — the junction numbers run on,
// the bigWig's host writer collects the rows of every tile — and end() closes the files.  run_tracks is begin, ONE tile, end: the same
// calls in the same order, the same bytes.  A tabix track takes a tile's rows as further runs (feed_tabix_track: the header line with
// the first rows, one close in end()).  The summary, --feature-depth, --transcripts, a clip and the device bigWig writer take the rows
// of one tile and are refused (GError) in a run of several.  --depth-summary goes with any number of tiles: every row belongs to one tile, so a tile's
// table — over the references between its first and its last row — is added to the run's (DepthTable), and end() writes the file.
class TrackStream {
 public:
  TrackStream(const TrackApi& api, const std::vector<std::string>& names, TrackFiles& tf, const TrackRun& run);
  void tile(const tbk_cov_in& in, bool last);  // last: no tile follows
  void end();
  uint64_t n_bases() const { return n_bases_; }
  uint64_t span_bases() const { return span_bases_; }
  uint64_t tiles() const { return tiles_; }

 private:
  const TrackApi& api_;
  const std::vector<std::string>& names_;
  TrackFiles& tf_;
  const TrackRun& run_;
  int64_t first_junc_ = 1;
  uint64_t n_bases_ = 0, span_bases_ = 0, tiles_ = 0;
  bool names_set_ = false;  // the reference names are on the context
  bool tx_started_[6] = {false, false, false, false, false, false};  // --tabix in a run of several tiles: the track's writer (cov, junc, samp, the three strands) has its header line and first rows
  // --strand-cov: the figures of the "strand phase ms" line (TBK_TIMING), added up over the tiles
  double ms_split_ = 0, ms_strand_cov_ = 0, ms_strand_text_ = 0;
  uint64_t strand_records_[3] = {0, 0, 0};
  bool strand_host_ = false;
  DepthTable depth_;                 // --depth-summary: the run's table so far
  std::vector<uint64_t> fd_covered_, fd_ge_;  // --feature-depth: the one tile's columns, written by end()
  double ms_depth_ = 0;
  uint64_t depth_rows_ = 0;
  bool depth_host_ = false;
  void depth_tile(const tbk_cov_out& rows);
  TxSummary tx_;                     // --transcripts: the one tile's columns, written by end()
  double ms_tx_ = 0;
  bool tx_host_ = false;
  void tx_tile(const tbk_cov_out& rows);
  TrackTimes times_;
};

template <class F>
void emit_lines(FILE* f, uint32_t n, F fmt) {
  unsigned hw = (unsigned)cpu_budget();
  size_t nt = n < 50000 ? 1 : std::max<size_t>(1, std::min<size_t>(hw ? hw : 4, 32));
  std::vector<std::string> parts(nt);
  auto work = [&](size_t t) {
    const uint32_t lo = (uint32_t)((uint64_t)n * t / nt), hi = (uint32_t)((uint64_t)n * (t + 1) / nt);
    std::string& o = parts[t];
    o.reserve((size_t)(hi - lo) * 40);
    char b[1024];
    for (uint32_t i = lo; i < hi; ++i) {
      int len = fmt(i, b, sizeof(b));
      if (len < 0) len = 0;
      if ((size_t)len >= sizeof(b)) {  // a very long reference name: format again into a buffer that fits
        std::vector<char> big((size_t)len + 1);
        len = fmt(i, big.data(), big.size());
        o.append(big.data(), (size_t)len);
      } else {
        o.append(b, (size_t)len);
      }
    }
  };
  if (nt == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; ++t) th.emplace_back(work, t);
    for (auto& x : th) x.join();
  }
  for (auto& o : parts)
    if (!o.empty() && fwrite(o.data(), 1, o.size(), f) != o.size()) GErrorWrite();
}

}  // namespace tbh
