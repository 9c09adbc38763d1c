// tracks.h — tiecov's three track files, shared by the tiecov command line and by `tiebrush --cov / --junc / --samp`: file names and
// header lines (tiecov.cpp:365-402 and the openings around them), and the host formatter of the lines (flushCoverage :237,
// CJunc::write :91-95, flushCoverage(pair) :289).  The host formatter is what tiecov prints with, the reference the device formatter
// (tbk_format_track) is tested against, and the command line's fallback when the device formatter refuses a track.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <thread>
#include <vector>

#include "../../../include/tbk.h"
#include "bai_read.h"
#include "bigwig.h"
#include "bgzf.h"
#include "tabix.h"

namespace tbh {

// The open track files.  An empty prefix: that track is not written.  Coverage goes to stdout for "-" / "stdout", to PREFIX.bigwig
// with `bigwig`, else to PREFIX.bedgraph; junctions to PREFIX.bed; the sample counts to PREFIX.bedgraph.  Errors are fatal (GError).
// With `tabix` every text track is PREFIX.bedgraph.gz / PREFIX.bed.gz (BGZF) with its tabix index beside it (tabix.h): the track's
// TabixWriter is open in the place of its FILE*, and takes the header line with its first rows.
// The device section producer of the bigWig (--bigwig-writer device) as a command line has it: tiecov links libtbk.so, tiebrush binds it
// at run time, so the entry points travel as pointers.
struct BigWigDevice {
  tbk_ctx* ctx = nullptr;
  decltype(&tbk_bigwig_build) build = nullptr;
  decltype(&tbk_strerror) strerror_ = nullptr;
  decltype(&tbk_last_error) last_error = nullptr;
};
// "host" / "device" -> false / true; anything else is fatal (GError)
bool parse_bigwig_writer(const char* value);

struct TrackFiles {
  FILE *cov = nullptr, *junc = nullptr, *samp = nullptr;
  BigWigWriter bw;
  bool cov_bw = false;
  std::vector<uint32_t> bw_lens;  // the chromosome lengths the bigWig was opened with
  std::string cov_name;
  TabixWriter cov_tx, junc_tx, samp_tx;  // --tabix
  void open(std::string cov_prefix, std::string junc_prefix, std::string samp_prefix, bool bigwig, const std::vector<std::string>& names,
            const std::vector<uint32_t>& lens, bool tabix = false);
  void close_bigwig();  // (after every interval went to bw)
  // The coverage rows into the bigWig and the file closed (flushCoverage(bigWigFile_t*), tiecov.cpp:243-275: the value as a float).
  // dev == nullptr: the host producer.  Else the sections are tbk_bigwig_build's; a refusal of that call other than a failed write
  // hands the file to the host producer (a line on stderr says so).  TBK_TIMING: a "bigwig phase" line on stderr for either.
  void write_bigwig(uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const BigWigDevice* dev);
  void close();
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

// The device summariser as a command line has it (see BigWigDevice).  summary == nullptr: the library in use has no tbk_cov_summary.
struct SummaryDevice {
  tbk_ctx* ctx = nullptr;
  decltype(&tbk_cov_summary) summary = nullptr;
  decltype(&tbk_strerror) strerror_ = nullptr;
  decltype(&tbk_last_error) last_error = nullptr;
};
// `--features BED --summary OUT` of a run: parsed (and refused) before any output file exists, written by write_summary
struct SummaryJob {
  std::string bed, out;
  FeatureTable F;
  bool on() const { return !out.empty(); }
  // The two options' rules and the BED file against the header (and, in a region run, against its normalised table U: every feature
  // wholly inside one interval).  Errors are fatal (GError) and name the line.
  void setup(const char* features_opt, const char* summary_opt, const BamHeader& hdr, const RegionTable* U);
};
// The summary of HOST rows (what tbk_coverage_tile wrote, before any clip) into job.out: tbk_cov_summary through dev, or the host
// summariser with TBK_SUMMARY_HOST=1.  Errors are fatal; a missing tbk_cov_summary is one.  TBK_TIMING: a "summary phase ms" line.
void write_summary(const SummaryJob& job, const std::vector<std::string>& names, const tbk_cov_out& rows, const SummaryDevice& dev);

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
