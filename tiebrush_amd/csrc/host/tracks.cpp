// tracks.cpp — see tracks.h
#include "tracks.h"

#include <string.h>
#include <unistd.h>

#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>

#include "GSam.h"

namespace tbh {

static bool ends_with(const std::string& s, const char* suf) {
  size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

static const char* const kCovHead = "track type=bedGraph\n";
static const char* const kJuncHead = "track name=junctions\n";
static const char* const kSampHead =
    "track type=bedGraph name=\"Sample Count Heatmap\" description=\"Sample Count Heatmap\" visibility=full "
    "graphType=\"heatmap\" color=200,100,0 altColor=0,100,200\n";

// --tabix: PREFIX<ext>.gz, opened with the track's header line
static void open_tabix(TabixWriter& w, std::string prefix, const char* ext, const char* head, const std::vector<std::string>& names,
                       const std::vector<uint32_t>& lens) {
  if (ends_with(prefix, (std::string(ext) + ".gz").c_str())) prefix.resize(prefix.size() - 3);
  if (!ends_with(prefix, ext)) prefix += ext;
  prefix += ".gz";
  std::string err;
  if (!w.open(prefix, names, lens, head, err)) GError("Error creating file %s (%s)\n", prefix.c_str(), err.c_str());
}

const char* const kStrandSuffix[3] = {".plus", ".minus", ".none"};

bool split_host_asked() { return getenv("TBK_SPLIT_HOST") && strcmp(getenv("TBK_SPLIT_HOST"), "0") != 0; }

void refuse_split_host_on_device(const char* prefix, const char* what) {
  if (prefix && split_host_asked())
    GError("Error: TBK_SPLIT_HOST=1 divides host records; the records of a %s run are on the device (unset it, or run without %s)\n", what, what);
}

void check_strand_cov(const char* prefix, int times, int ranks) {
  if (!prefix) return;
  if (times > 1) GError("Error: --strand-cov given more than once (one prefix per run)\n");
  if (!*prefix || strcmp(prefix, "-") == 0 || strcmp(prefix, "stdout") == 0)
    GError("Error: --strand-cov needs a file prefix (not '%s'): its three tracks cannot share standard output\n", prefix);
  if (ranks > 1) GError("Error: --strand-cov and --ranks do not go together (the per-strand tracks are written by a single-rank run)\n");
}

void TrackFiles::open(const TrackOptions& o, const std::vector<std::string>& names, const std::vector<uint32_t>& lens) {
  std::string cov_prefix = o.cov, junc_prefix = o.junc, samp_prefix = o.samp;
  const bool bigwig = o.bigwig;
  for (int s = 0; s < 3 && !o.strand_cov.empty(); ++s) {  // --strand-cov: each file by the rules of -c below
    CovSink& k = strand[s];
    std::string prefix = o.strand_cov + kStrandSuffix[s];
    if (o.tabix && !bigwig) {
      open_tabix(k.tx, prefix, ".bedgraph", kCovHead, names, lens);
      k.name = k.tx.path();
    } else if (bigwig) {
      prefix += ".bigwig";
      std::string err;
      if (!k.bw.open(prefix, names, lens, err)) GError("Error creating file %s\n", prefix.c_str());
      k.is_bw = true;
      bw_lens = lens;
      k.name = prefix;
    } else {
      prefix += ".bedgraph";
      k.f = fopen(prefix.c_str(), "w");
      if (!k.f) GError("Error creating file %s\n", prefix.c_str());
      fprintf(k.f, "%s", kCovHead);
      k.name = prefix;
    }
  }
  if (o.tabix) {  // every text track; the coverage as a bigWig stays what it is below
    if (!cov_prefix.empty() && !bigwig && cov_prefix != "-" && cov_prefix != "stdout") open_tabix(cov_tx, cov_prefix, ".bedgraph", kCovHead, names, lens), cov_name = cov_tx.path(), cov_prefix.clear();
    if (!junc_prefix.empty()) open_tabix(junc_tx, junc_prefix, ".bed", kJuncHead, names, lens), junc_prefix.clear();
    if (!samp_prefix.empty()) open_tabix(samp_tx, samp_prefix, ".bedgraph", kSampHead, names, lens), samp_prefix.clear();
  }
  if (!cov_prefix.empty()) {
    if (cov_prefix == "-" || cov_prefix == "stdout") {
      cov = stdout;
    } else if (bigwig) {  // tiecov.cpp:365-402
      if (!ends_with(cov_prefix, ".bigwig")) cov_prefix += ".bigwig";
      std::string err;
      if (!bw.open(cov_prefix, names, lens, err)) GError("Error creating file %s\n", cov_prefix.c_str());
      cov_bw = true;
      bw_lens = lens;
    } else {
      if (!ends_with(cov_prefix, ".bedgraph")) cov_prefix += ".bedgraph";
      cov = fopen(cov_prefix.c_str(), "w");
      if (!cov) GError("Error creating file %s\n", cov_prefix.c_str());
      fprintf(cov, "%s", kCovHead);
    }
    cov_name = cov_prefix;
  }
  if (!junc_prefix.empty()) {
    if (!ends_with(junc_prefix, ".bed")) junc_prefix += ".bed";
    junc = fopen(junc_prefix.c_str(), "w");
    if (!junc) GError("Error creating file %s\n", junc_prefix.c_str());
    junc_name = junc_prefix;
    fprintf(junc, "%s", kJuncHead);
  }
  if (!samp_prefix.empty()) {
    if (!ends_with(samp_prefix, ".bedgraph")) samp_prefix += ".bedgraph";
    samp = fopen(samp_prefix.c_str(), "w");
    if (!samp) GError("Error creating file %s\n", samp_prefix.c_str());
    samp_name = samp_prefix;
    fprintf(samp, "%s", kSampHead);
  }
}

void TrackFiles::close_bigwig() {
  if (!cov_bw) return;
  std::string err;
  if (!bw.close(err)) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
  cov_bw = false;
}

// (a per-strand bigWig whose items are all in: --strand-cov -W over several tiles)
static void close_strand_bigwigs(TrackFiles& tf) {
  for (CovSink& k : tf.strand) {
    if (!k.is_bw) continue;
    std::string err;
    if (!k.bw.close(err)) GError("Error: writing %s failed (%s)\n", k.name.c_str(), err.c_str());
    k.is_bw = false;
  }
}

bool parse_bigwig_writer(const char* value) {
  const std::string v = value ? value : "";
  if (v == "device") return true;
  if (v != "host") GError("Error: --bigwig-writer takes host or device (got '%s')\n", v.c_str());
  return false;
}

namespace {
// tbk_bigwig_build's events -> the writer's feed: the plan at the first event, a level's table before its first byte
struct BwBridge {
  BigWigFeed* feed;
  const tbk_bw_out* out;
  bool planned = false, failed = false;
  int level = -1;
  bool advance(uint32_t to) {  // plan, and the tables of every level up to `to`
    if (!planned) {
      uint32_t red[TBK_BW_MAX_ZOOM];
      uint64_t items[1 + TBK_BW_MAX_ZOOM];
      const uint32_t nz = out->n_levels - 1;
      for (uint32_t L = 0; L <= nz; ++L) items[L] = out->level[L].n_items;
      for (uint32_t z = 0; z < nz; ++z) red[z] = out->level[1 + z].reduction;
      planned = true;
      if (!feed->plan(red, items, nz)) return false;
    }
    while (level < (int)to) {
      const tbk_bw_level& lv = out->level[++level];
      std::vector<BigWigSection> sec((size_t)lv.n_sections);
      for (size_t i = 0; i < sec.size(); ++i) {
        const tbk_bw_section& s = lv.sections[i];
        sec[i] = BigWigSection{s.chrom, s.start, s.end, s.offset, s.size};
      }
      if (!feed->level((uint32_t)level, sec.data(), sec.size(), lv.max_payload)) return false;
    }
    return true;
  }
  static int sink(void* user, uint32_t level, const uint8_t* bytes, uint64_t n) {
    BwBridge* b = (BwBridge*)user;
    if (b->advance(level) && b->feed->bytes(bytes, (size_t)n)) return 0;
    b->failed = true;
    return 1;
  }
};
}  // namespace

// one bigWig file: the rows into `bw` and the file closed (TrackFiles::write_bigwig for the coverage track and for a strand's)
static void write_bigwig_file(BigWigWriter& bw, bool& cov_bw, const std::string& cov_name, const std::vector<uint32_t>& bw_lens, uint32_t n, const int32_t* tid,
                              const int32_t* start, const int32_t* end, const double* val, const TrackApi* dev) {
  if (!cov_bw) return;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n; ++i) bw.add((uint32_t)tid[i], (uint32_t)start[i], (uint32_t)end[i], (float)val[i]);
  const char* writer = "host";
  std::string err;
  bool done = false;
  if (dev) {
    tbk_track_rows r;
    memset(&r, 0, sizeof(r));
    r.mem = TBK_MEM_HOST, r.kind = TBK_TRACK_COV, r.n = n, r.tid = tid, r.start = start, r.end = end, r.val = val;
    tbk_bw_out out;
    memset(&out, 0, sizeof(out));
    int rc = 0;
    bool write_failed = false;
    done = bw.close_with(
        [&](BigWigFeed& feed) {
          BwBridge b{&feed, &out};
          rc = dev->bigwig_build(dev->ctx, &r, (uint32_t)bw_lens.size(), bw_lens.data(), BwBridge::sink, &b, &out);
          if (rc == 0 && !b.advance(out.n_levels - 1)) b.failed = true;  // (levels without a byte: an empty data level)
          write_failed = b.failed;
          return rc == 0 && !b.failed;
        },
        err);
    if (done) {
      writer = "device";
    } else {
      if (write_failed || rc == 0) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
      fprintf(stderr, "Warning: the device bigWig writer refused %s (%s: %s); the host writer takes it\n", cov_name.c_str(), dev->strerror_(rc),
              dev->last_error(dev->ctx));
      if (!bw.restart(err)) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
    }
  }
  if (!done && !bw.close(err)) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
  cov_bw = false;
  if (getenv("TBK_TIMING"))
    fprintf(stderr, "bigwig phase ms: writer %s | %u rows | %.1f\n", writer, n,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

void TrackFiles::write_bigwig(uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const TrackApi* dev) {
  write_bigwig_file(bw, cov_bw, cov_name, bw_lens, n, tid, start, end, val, dev);
}
void TrackFiles::write_strand_bigwig(int s, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const TrackApi* dev) {
  write_bigwig_file(strand[s].bw, strand[s].is_bw, strand[s].name, bw_lens, n, tid, start, end, val, dev);
}

void TrackFiles::close() {
  close_bigwig();
  close_strand_bigwigs(*this);
  for (CovSink& k : strand) {
    if (k.f) fclose(k.f);
    k.f = nullptr;
  }
  if (cov && cov != stdout) fclose(cov);
  if (cov == stdout) fflush(stdout);
  if (junc) fclose(junc);
  if (samp) fclose(samp);
  cov = junc = samp = nullptr;
  for (TabixWriter* w : {&cov_tx, &junc_tx, &samp_tx, &strand[0].tx, &strand[1].tx, &strand[2].tx}) {  // (a track nobody wrote rows to: its header, the EOF member, an empty index)
    std::string err;
    if (!w->is_open()) continue;
    std::vector<BaiRec> none;
    if ((!w->head().empty() && !w->add_text(w->head().data(), w->head().size(), none, err)) || !w->close(err))
      GError("Error: writing %s failed (%s)\n", w->path().c_str(), err.c_str());
  }
}

void GErrorWrite() { GError("Error: failed to write an output line\n"); }

int fmt_cov_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, double val) {
  return snprintf(b, cap, "%s\t%d\t%d\t%.3f\n", name, start, end, val);
}
int fmt_junc_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, int number, double val, char strand) {
  return snprintf(b, cap, "%s\t%d\t%d\tJUNC%08d\t%.3f\t%c\n", name, start, end, number, val, strand);
}
int fmt_samp_line(char* b, size_t cap, const char* name, int32_t start, int32_t end, int64_t count, float heat) {
  return snprintf(b, cap, "%s\t%d\t%d\t%ld\t%f\n", name, start, end, (long)count, heat);
}

void emit_cov_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                    const double* val) {
  emit_lines(f, n, [&](uint32_t i, char* b, size_t cap) { return fmt_cov_line(b, cap, names[tid[i]].c_str(), start[i], end[i], val[i]); });
}
void emit_junc_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                     const double* val, const uint8_t* strand, int64_t first_junc) {
  emit_lines(f, n, [&](uint32_t i, char* b, size_t cap) {
    return fmt_junc_line(b, cap, names[tid[i]].c_str(), start[i], end[i], (int)(first_junc + (int64_t)i), val[i], (char)strand[i]);
  });
}
void emit_samp_lines(FILE* f, const std::vector<std::string>& names, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                     const int64_t* count, const float* heat) {
  emit_lines(f, n, [&](uint32_t i, char* b, size_t cap) { return fmt_samp_line(b, cap, names[tid[i]].c_str(), start[i], end[i], count[i], heat[i]); });
}

void summarise_features(const FeatureTable& F, bool want_cov, uint32_t ni, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val,
                        bool want_junc, uint32_t nj, const int32_t* jtid, const int32_t* jstart, const int32_t* jend, const uint8_t* jstrand, const double* jval,
                        FeatSummary& S) {
  S.resize(F.n());
  for (size_t f = 0; f < F.n(); ++f) {
    const int32_t ft = F.tid[f];
    const int64_t fb = F.beg[f], fe = F.end[f];
    if (want_cov && ni) {
      uint32_t lo = 0, hi = ni;  // the first row that ends behind the feature's begin on its reference, or lies on a later one
      while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (tid[m] > ft || (tid[m] == ft && (int64_t)end[m] > fb))
          hi = m;
        else
          lo = m + 1;
      }
      double s = 0.0, mx = 0.0;
      uint64_t c = 0;
      for (uint32_t i = lo; i < ni && tid[i] == ft && (int64_t)start[i] < fe; ++i) {
        const int64_t len = std::min<int64_t>(end[i], fe) - std::max<int64_t>(start[i], fb);
        s += val[i] * (double)len;
        c += (uint64_t)len;
        mx = (i == lo || val[i] > mx) ? val[i] : mx;
      }
      S.covered[f] = c, S.sum[f] = s, S.max[f] = c ? mx : 0.0;
    }
    if (want_junc && nj) {
      uint32_t lo = 0, hi = nj;  // the first junction row at or behind (tid, start, end)
      while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        const bool ge = jtid[m] != ft ? jtid[m] > ft : ((int64_t)jstart[m] != fb ? (int64_t)jstart[m] > fb : (int64_t)jend[m] >= fe);
        if (ge)
          hi = m;
        else
          lo = m + 1;
      }
      double j = 0.0;
      for (uint32_t i = lo; i < nj && jtid[i] == ft && (int64_t)jstart[i] == fb && (int64_t)jend[i] == fe; ++i)
        if (F.strand[f] == '.' || jstrand[i] == F.strand[f]) j += jval[i];
      S.junc[f] = j;
    }
  }
}

bool write_summary_tsv(const std::string& path, const std::vector<std::string>& names, const FeatureTable& F, const FeatSummary& S, std::string& err) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return err = "cannot create " + path, false;
  bool ok = fputs("#chrom\tstart\tend\tname\tstrand\tsize\tcovered\tsum\tmean0\tmean\tmax\tjunc\n", f) >= 0;
  for (size_t i = 0; ok && i < F.n(); ++i) {
    const int64_t size = F.end[i] - F.beg[i];
    const double mean0 = S.sum[i] / (double)size, mean = S.covered[i] ? S.sum[i] / (double)S.covered[i] : 0.0;
    ok = fprintf(f, "%s\t%lld\t%lld\t%s\t%c\t%lld\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\t%.3f\n", names[(size_t)F.tid[i]].c_str(), (long long)F.beg[i], (long long)F.end[i],
                 F.name[i].c_str(), (char)F.strand[i], (long long)size, (unsigned long long)S.covered[i], S.sum[i], mean0, mean, S.max[i], S.junc[i]) > 0;
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) err = "writing " + path + " failed";
  return ok;
}

void SummaryJob::setup(const char* features_opt, const char* summary_opt, const BamHeader& hdr, const RegionTable* U) {
  if (summary_opt && !features_opt) GError("Error: --summary needs --features BED (the features to summarise)\n");
  if (features_opt && !summary_opt) GError("Error: --features needs --summary OUT.tsv (the file to write)\n");
  if (!summary_opt) return;
  if (!*summary_opt || !*features_opt) GError("Error: --features / --summary need a file name\n");
  bed = features_opt, out = summary_opt;
  std::string err;
  if (!features_from_bed_file(hdr, bed, F, err)) GError("Error: --features: %s\n", err.c_str());
  // (outside the region's intervals the rows are incomplete; inside them they are the whole file's)
  if (U && !features_inside(F, *U, bed, err)) GError("Error: --features: %s\n", err.c_str());
}

void write_summary(const SummaryJob& job, const std::vector<std::string>& names, const tbk_cov_out& rows, const TrackApi& api) {
  const auto t0 = std::chrono::steady_clock::now();
  const FeatureTable& F = job.F;
  const bool host = getenv("TBK_SUMMARY_HOST") && strcmp(getenv("TBK_SUMMARY_HOST"), "0") != 0;
  FeatSummary S;
  if (host) {
    summarise_features(F, true, rows.n_intervals, rows.iv_tid, rows.iv_start, rows.iv_end, rows.iv_val, true, rows.n_junctions, rows.j_tid, rows.j_start,
                       rows.j_end, rows.j_strand, rows.j_val, S);
  } else {
    if (!api.cov_summary) GError("Error: --summary: the loaded libtbk.so has no tbk_cov_summary (an older build?)\n");
    S.resize(F.n());
    tbk_features f;
    f.n = (uint32_t)F.n(), f.tid = F.tid.data(), f.beg = F.beg.data(), f.end = F.end.data(), f.strand = F.strand.data();
    tbk_feat_out o;
    o.mem = TBK_MEM_HOST, o.covered = S.covered.data(), o.sum = S.sum.data(), o.max = S.max.data(), o.junc = S.junc.data();
    const int rc = api.cov_summary(api.ctx, &rows, &f, &o);
    if (rc != 0) GError("Error: GPU feature summary failed: %s (%s)\n", api.strerror_(rc), api.last_error(api.ctx));
  }
  std::string err;
  if (!write_summary_tsv(job.out, names, F, S, err)) GError("Error: --summary: %s\n", err.c_str());
  if (getenv("TBK_TIMING"))
    fprintf(stderr, "summary phase ms: %s | %zu features | %u interval rows | %u junction rows | %.1f\n", host ? "host" : "device", F.n(), rows.n_intervals,
            rows.n_junctions, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ---- bases at depth -------------------------------------------------------------------------------------------------
bool parse_thresholds(const char* list, std::vector<double>& thr, std::vector<std::string>& text, std::string& err) {
  thr.clear(), text.clear();
  const std::string all = list ? list : "";
  for (size_t a = 0;; ) {
    const size_t b = std::min(all.find(',', a), all.size());
    const std::string item = all.substr(a, b - a);
    if (thr.size() == TBK_MAX_THRESHOLDS) return err = "more than 16 thresholds (the 17th is '" + item + "')", false;
    char* e = nullptr;
    const double v = item.empty() ? 0.0 : strtod(item.c_str(), &e);
    // (strtod skips leading blanks and reads "inf", "nan" and hexadecimal forms: a decimal number starts with a digit, a point or a sign)
    if (item.empty() || !strchr("0123456789.+-", item[0]) || *e != 0 || item.find_first_of("xXnN") != std::string::npos)
      return err = "'" + item + "' is not a decimal number", false;
    if (!(v > 0.0) || v - v != 0.0) return err = "'" + item + "' is not a finite number above 0", false;
    if (!thr.empty() && !(v > thr.back())) return err = "'" + item + "' is not above the threshold before it ('" + text.back() + "'): the list is strictly ascending", false;
    thr.push_back(v), text.push_back(item);
    if (b == all.size()) return true;
    a = b + 1;
  }
}

void threshold_features(size_t n, const int32_t* ftid, const int64_t* fbeg, const int64_t* fend, uint32_t ni, const int32_t* tid, const int32_t* start,
                        const int32_t* end, const double* val, const double* thr, uint32_t n_thr, uint64_t* covered, uint64_t* ge) {
  for (size_t f = 0; f < n; ++f) {
    const int32_t ft = ftid[f];
    const int64_t fb = fbeg[f], fe = fend[f];
    uint32_t lo = 0, hi = ni;  // the first row that ends behind the feature's begin on its reference, or lies on a later one
    while (lo < hi) {
      const uint32_t m = lo + (hi - lo) / 2;
      if (tid[m] > ft || (tid[m] == ft && (int64_t)end[m] > fb))
        hi = m;
      else
        lo = m + 1;
    }
    uint64_t c = 0;
    uint64_t* g = ge + f * n_thr;
    for (uint32_t k = 0; k < n_thr; ++k) g[k] = 0;
    for (uint32_t i = lo; i < ni && tid[i] == ft && (int64_t)start[i] < fe; ++i) {
      const uint64_t len = (uint64_t)(std::min<int64_t>(end[i], fe) - std::max<int64_t>(start[i], fb));
      c += len;
      for (uint32_t k = 0; k < n_thr && val[i] >= thr[k]; ++k) g[k] += len;  // (ascending: the first threshold above the value ends the row)
    }
    if (covered) covered[f] = c;
  }
}

// a table file under write_summary's rules, with one more: a file that could not be written whole is removed
static bool write_table(const std::string& path, const std::string& text, std::string& err) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return err = "cannot create " + path, false;
  bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0) ok = false;
  if (!ok) (void)unlink(path.c_str()), err = "writing " + path + " failed";
  return ok;
}
static void append_fmt(std::string& o, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void append_fmt(std::string& o, const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(b, sizeof(b), fmt, ap);
  va_end(ap);
  o.append(b, (size_t)std::min<int>(std::max(n, 0), (int)sizeof(b) - 1));
}

bool write_depth_tsv(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::vector<std::string>& thr_text,
                     const DepthTable& D, std::string& err) {
  const size_t nt = thr_text.size();
  std::string o = "#chrom\tlength\tcovered\tsum\tmean0\tmean\tmax";
  for (const std::string& t : thr_text) o += "\tge_" + t;
  o += "\n";
  auto line = [&](const std::string& name, uint64_t len, uint64_t cov, double sum, double max, const uint64_t* ge) {
    o += name;
    append_fmt(o, "\t%llu\t%llu\t%.3f\t%.3f\t%.3f\t%.3f", (unsigned long long)len, (unsigned long long)cov, sum, len ? sum / (double)len : 0.0,
               cov ? sum / (double)cov : 0.0, max);
    for (size_t k = 0; k < nt; ++k) append_fmt(o, "\t%llu", (unsigned long long)ge[k]);
    o += "\n";
  };
  uint64_t t_len = 0, t_cov = 0;
  double t_sum = 0.0, t_max = 0.0;
  std::vector<uint64_t> t_ge(nt ? nt : 1, 0);
  for (size_t r = 0; r < names.size(); ++r) {
    line(names[r], lens[r], D.covered[r], D.sum[r], D.max[r], D.ge.data() + r * nt);
    t_len += lens[r], t_cov += D.covered[r], t_sum += D.sum[r], t_max = std::max(t_max, D.max[r]);
    for (size_t k = 0; k < nt; ++k) t_ge[k] += D.ge[r * nt + k];
  }
  line("total", t_len, t_cov, t_sum, t_max, t_ge.data());
  return write_table(path, o, err);
}

bool write_feature_depth_tsv(const std::string& path, const std::vector<std::string>& names, const FeatureTable& F, const std::vector<std::string>& thr_text,
                             const uint64_t* covered, const uint64_t* ge, std::string& err) {
  const size_t nt = thr_text.size();
  std::string o = "#chrom\tstart\tend\tname\tstrand\tsize\tcovered";
  for (const std::string& t : thr_text) o += "\tge_" + t;
  o += "\n";
  for (size_t i = 0; i < F.n(); ++i) {
    o += names[(size_t)F.tid[i]];
    append_fmt(o, "\t%lld\t%lld\t", (long long)F.beg[i], (long long)F.end[i]);
    o += F.name[i];
    append_fmt(o, "\t%c\t%lld\t%llu", (char)F.strand[i], (long long)(F.end[i] - F.beg[i]), (unsigned long long)covered[i]);
    for (size_t k = 0; k < nt; ++k) append_fmt(o, "\t%llu", (unsigned long long)ge[i * nt + k]);
    o += "\n";
  }
  return write_table(path, o, err);
}

void DepthJob::setup(const char* thresholds_opt, const char* depth_opt, const char* feature_depth_opt, const char* features_opt, const BamHeader& hdr,
                     const RegionTable* U) {
  if (!thresholds_opt && !depth_opt && !feature_depth_opt) return;
  std::string err;
  if (thresholds_opt && !parse_thresholds(thresholds_opt, thr, thr_text, err)) GError("Error: --thresholds: %s\n", err.c_str());
  if (thresholds_opt && !depth_opt && !feature_depth_opt)
    GError("Error: --thresholds needs --depth-summary OUT.tsv or --feature-depth OUT.tsv (the table its columns go to)\n");
  if (feature_depth_opt && !features_opt) GError("Error: --feature-depth needs --features BED (the features to count in)\n");
  if (feature_depth_opt && !thresholds_opt) GError("Error: --feature-depth needs --thresholds T1,T2,... (the depths to count)\n");
  if ((depth_opt && !*depth_opt) || (feature_depth_opt && (!*feature_depth_opt || !*features_opt))) GError("Error: --depth-summary / --feature-depth / --features need a file name\n");
  if (depth_opt && U) GError("Error: --depth-summary and -r / -R do not go together (outside the region's intervals the rows are incomplete)\n");
  lens = hdr.target_len;
  if (depth_opt) summary_out = depth_opt;
  if (feature_depth_opt) {
    feature_out = feature_depth_opt, bed = features_opt;
    if (!features_from_bed_file(hdr, bed, F, err)) GError("Error: --features: %s\n", err.c_str());
    if (U && !features_inside(F, *U, bed, err)) GError("Error: --features: %s\n", err.c_str());
  }
}

// ---- per-transcript support -------------------------------------------------------------------------------------------
void summarise_transcripts(const TranscriptTable& X, bool want_cov, uint32_t ni, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val,
                           bool want_junc, uint32_t nj, const int32_t* jtid, const int32_t* jstart, const int32_t* jend, const uint8_t* jstrand, const double* jval,
                           TxSummary& S) {
  const size_t n_tx = X.n_tx(), n_ex = X.n_exon();
  S.resize(n_tx, n_ex);
  if (want_cov) {  // the exons as features
    FeatureTable F;
    for (size_t t = 0; t < n_tx; ++t)
      for (uint32_t e = X.tx_off[t]; e < X.tx_off[t + 1]; ++e) F.tid.push_back(X.tid[t]), F.beg.push_back(X.ex_beg[e]), F.end.push_back(X.ex_end[e]), F.strand.push_back((uint8_t)'.');
    FeatSummary E;
    summarise_features(F, true, ni, tid, start, end, val, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, E);
    S.ex_covered = E.covered, S.ex_sum = E.sum, S.ex_max = E.max;
  }
  if (want_junc && n_ex > n_tx) {  // the introns as features
    FeatureTable F;
    std::vector<uint32_t> at;
    for (size_t t = 0; t < n_tx; ++t)
      for (uint32_t e = X.tx_off[t]; e + 1 < X.tx_off[t + 1]; ++e)
        F.tid.push_back(X.tid[t]), F.beg.push_back(X.ex_end[e]), F.end.push_back(X.ex_beg[e + 1]), F.strand.push_back(X.strand[t]), at.push_back(e);
    FeatSummary I;
    summarise_features(F, false, 0, nullptr, nullptr, nullptr, nullptr, true, nj, jtid, jstart, jend, jstrand, jval, I);
    for (size_t k = 0; k < at.size(); ++k) S.in_junc[at[k]] = I.junc[k];
  }
  for (size_t t = 0; t < n_tx; ++t) {
    const uint32_t e0 = X.tx_off[t], e1 = X.tx_off[t + 1];
    for (uint32_t e = e0; e < e1 && want_cov; ++e) {
      S.covered[t] += S.ex_covered[e], S.sum[t] += S.ex_sum[e];
      if (S.ex_covered[e]) S.max[t] = (S.exons_hit[t] == 0 || S.ex_max[e] > S.max[t]) ? S.ex_max[e] : S.max[t], ++S.exons_hit[t];
    }
    for (uint32_t e = e0; e + 1 < e1 && want_junc; ++e) {
      const double j = S.in_junc[e];
      S.junc_sum[t] += j, S.introns_hit[t] += j > 0.0;
      S.junc_min[t] = (e == e0 || j < S.junc_min[t]) ? j : S.junc_min[t];
    }
  }
}

bool write_transcripts_tsv(const std::string& path, const std::vector<std::string>& names, const TranscriptTable& X, const TxSummary& S, std::string& err) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) return err = "cannot create " + path, false;
  bool ok = fputs("#chrom\tstart\tend\ttranscript\tgene\tstrand\texons\tlength\tcovered\tsum\tmean0\tmean\tmax\texons_hit\tintrons\tintrons_hit\tjunc_min\tjunc_sum\n", f) >= 0;
  for (size_t t = 0; ok && t < X.n_tx(); ++t) {
    const uint32_t e0 = X.tx_off[t], e1 = X.tx_off[t + 1];
    int64_t length = 0;
    for (uint32_t e = e0; e < e1; ++e) length += X.ex_end[e] - X.ex_beg[e];
    const double mean0 = S.sum[t] / (double)length, mean = S.covered[t] ? S.sum[t] / (double)S.covered[t] : 0.0;
    ok = fprintf(f, "%s\t%lld\t%lld\t%s\t%s\t%c\t%u\t%lld\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\t%u\t%u\t%u\t%.3f\t%.3f\n", names[(size_t)X.tid[t]].c_str(), (long long)X.ex_beg[e0],
                 (long long)X.ex_end[e1 - 1], X.id[t].c_str(), X.gene[t].c_str(), (char)X.strand[t], e1 - e0, (long long)length, (unsigned long long)S.covered[t], S.sum[t],
                 mean0, mean, S.max[t], S.exons_hit[t], e1 - e0 - 1, S.introns_hit[t], S.junc_min[t], S.junc_sum[t]) > 0;
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) (void)unlink(path.c_str()), err = "writing " + path + " failed";
  return ok;
}

void TxJob::setup(const char* gtf_opt, const char* transcripts_opt, const BamHeader& hdr, const RegionTable* U) {
  if (transcripts_opt && !gtf_opt) GError("Error: --transcripts needs --gtf FILE (the annotation to summarise)\n");
  if (gtf_opt && !transcripts_opt) GError("Error: --gtf needs --transcripts OUT.tsv (the file to write)\n");
  if (!transcripts_opt) return;
  if (!*transcripts_opt || !*gtf_opt) GError("Error: --gtf / --transcripts need a file name\n");
  gtf = gtf_opt, out = transcripts_opt;
  std::string err;
  if (!transcripts_from_gtf_file(hdr, gtf, X, err)) GError("Error: --gtf: %s\n", err.c_str());
  // (outside the region's intervals the rows are incomplete, and a transcript's introns lie between its exons: the whole span)
  if (U && !features_inside(transcript_spans(X), *U, gtf, err)) GError("Error: --gtf: %s (a transcript's span, from its first exon to its last)\n", err.c_str());
}

// the one tile's rows (host, before any clip) into the run's transcript columns; the file is end()'s
void TrackStream::tx_tile(const tbk_cov_out& rows) {
  const auto t0 = std::chrono::steady_clock::now();
  const TranscriptTable& X = run_.transcripts->X;
  const TrackApi& api = api_;
  tx_host_ = getenv("TBK_SUMMARY_HOST") && strcmp(getenv("TBK_SUMMARY_HOST"), "0") != 0;
  if (tx_host_) {
    summarise_transcripts(X, true, rows.n_intervals, rows.iv_tid, rows.iv_start, rows.iv_end, rows.iv_val, true, rows.n_junctions, rows.j_tid, rows.j_start, rows.j_end,
                          rows.j_strand, rows.j_val, tx_);
  } else {
    if (!api.tx_summary) GError("Error: --transcripts: the loaded libtbk.so has no tbk_tx_summary (an older build?)\n");
    tx_.resize(X.n_tx(), X.n_exon());
    tbk_transcripts x;
    x.n_tx = (uint32_t)X.n_tx(), x.n_exon = (uint32_t)X.n_exon(), x.tx_off = X.tx_off.data(), x.tid = X.tid.data(), x.strand = X.strand.data();
    x.ex_beg = X.ex_beg.data(), x.ex_end = X.ex_end.data();
    tbk_tx_out o;
    memset(&o, 0, sizeof(o));
    o.mem = TBK_MEM_HOST, o.covered = tx_.covered.data(), o.sum = tx_.sum.data(), o.max = tx_.max.data(), o.exons_hit = tx_.exons_hit.data();
    o.introns_hit = tx_.introns_hit.data(), o.junc_min = tx_.junc_min.data(), o.junc_sum = tx_.junc_sum.data();
    const int rc = api.tx_summary(api.ctx, &rows, &x, &o);
    if (rc != 0) GError("Error: GPU transcript summary failed: %s (%s)\n", api.strerror_(rc), api.last_error(api.ctx));
  }
  ms_tx_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// one tile's rows (host, before any clip) into the run's depth tables
void TrackStream::depth_tile(const tbk_cov_out& rows) {
  const auto t0 = std::chrono::steady_clock::now();
  const DepthJob& job = *run_.depth;
  const TrackApi& api = api_;
  const bool host = getenv("TBK_SUMMARY_HOST") && strcmp(getenv("TBK_SUMMARY_HOST"), "0") != 0;
  const uint32_t nt = (uint32_t)job.thr.size(), ni = rows.n_intervals;
  if (!host && nt && !api.cov_thresholds) GError("Error: --thresholds: the loaded libtbk.so has no tbk_cov_thresholds (an older build?)\n");
  tbk_cov_out iv = rows;  // the interval rows alone
  iv.cap_junctions = 0, iv.n_junctions = 0;
  auto thresholds = [&](const FeatureTable& F, uint64_t* covered, uint64_t* ge) {
    if (host) return threshold_features(F.n(), F.tid.data(), F.beg.data(), F.end.data(), ni, rows.iv_tid, rows.iv_start, rows.iv_end, rows.iv_val, job.thr.data(), nt, covered, ge);
    tbk_features f;
    f.n = (uint32_t)F.n(), f.tid = F.tid.data(), f.beg = F.beg.data(), f.end = F.end.data(), f.strand = nullptr;
    tbk_thr_out o;
    o.mem = TBK_MEM_HOST, o.covered = covered, o.ge = ge;
    const int rc = api.cov_thresholds(api.ctx, &iv, &f, job.thr.data(), nt, &o);
    if (rc != 0) GError("Error: GPU depth thresholds failed: %s (%s)\n", api.strerror_(rc), api.last_error(api.ctx));
  };
  if (job.per_ref()) {
    const size_t n_ref = job.lens.size();
    if (depth_.covered.size() != n_ref) depth_.resize(n_ref, nt);
    FeatureTable F;  // a tile needs the references between its first and its last row's: [0, LN) of each (LN:0 has no base to count)
    if (ni)
      for (int32_t t = rows.iv_tid[0]; t <= rows.iv_tid[ni - 1]; ++t)
        if (t >= 0 && (size_t)t < n_ref && job.lens[(size_t)t]) F.tid.push_back(t), F.beg.push_back(0), F.end.push_back((int64_t)job.lens[(size_t)t]), F.strand.push_back((uint8_t)'.');
    if (F.n()) {
      FeatSummary S;
      if (host) {
        summarise_features(F, true, ni, rows.iv_tid, rows.iv_start, rows.iv_end, rows.iv_val, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, S);
      } else {
        if (!api.cov_summary) GError("Error: --depth-summary: the loaded libtbk.so has no tbk_cov_summary (an older build?)\n");
        S.resize(F.n());
        tbk_features f;
        f.n = (uint32_t)F.n(), f.tid = F.tid.data(), f.beg = F.beg.data(), f.end = F.end.data(), f.strand = nullptr;
        tbk_feat_out o;
        o.mem = TBK_MEM_HOST, o.covered = S.covered.data(), o.sum = S.sum.data(), o.max = S.max.data(), o.junc = nullptr;
        const int rc = api.cov_summary(api.ctx, &iv, &f, &o);
        if (rc != 0) GError("Error: GPU depth summary failed: %s (%s)\n", api.strerror_(rc), api.last_error(api.ctx));
      }
      std::vector<uint64_t> ge(F.n() * (size_t)nt + 1, 0);
      if (nt) thresholds(F, nullptr, ge.data());
      for (size_t i = 0; i < F.n(); ++i) {
        const size_t r = (size_t)F.tid[i];
        depth_.covered[r] += S.covered[i], depth_.sum[r] += S.sum[i], depth_.max[r] = std::max(depth_.max[r], S.max[i]);
        for (uint32_t k = 0; k < nt; ++k) depth_.ge[r * nt + k] += ge[i * nt + k];
      }
    }
  }
  if (job.per_feature()) {
    fd_covered_.assign(job.F.n(), 0), fd_ge_.assign(job.F.n() * (size_t)nt, 0);
    thresholds(job.F, fd_covered_.data(), fd_ge_.data());
  }
  depth_host_ = host, depth_rows_ += ni;
  ms_depth_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

tbk_cov_in CovRecs::as_cov_in() const {
  tbk_cov_in in;
  memset(&in, 0, sizeof(in));
  in.mem = TBK_MEM_HOST;
  in.n_records = (uint32_t)tid.size();
  in.n_cigar_ops = (uint32_t)cig.size();
  // A column without elements travels as NULL, said here and not left to what vector::data() gives for an empty vector: no records at
  // all (every column), or a part of split_strand_host, which has no flag column ("every record counts") and no yc / yx where its
  // input had none.  A table that append() filled has every column as long as tid, so nothing changes for it.
  auto col = [](const auto& v) { return v.empty() ? nullptr : v.data(); };
  in.tid = col(tid), in.pos = col(pos), in.flag = col(flag), in.cig_off = cig_off.data(), in.cig = col(cig);
  in.yc = col(yc), in.strand = col(strand), in.yx = col(yx);
  return in;
}

void split_strand_host(const tbk_cov_in& in, CovRecs out[3]) {
  for (int s = 0; s < 3; ++s) out[s] = CovRecs();
  for (size_t i = 0; i < in.n_records; ++i) {
    if (in.flag && (in.flag[i] & 0x4)) continue;
    const uint8_t st = in.strand[i];
    CovRecs& o = out[st == '+' ? 0 : (st == '-' ? 1 : 2)];
    o.tid.push_back(in.tid[i]), o.pos.push_back(in.pos[i]), o.strand.push_back(st);
    if (in.yc) o.yc.push_back(in.yc[i]);
    if (in.yx) o.yx.push_back(in.yx[i]);
    o.cig.insert(o.cig.end(), in.cig + in.cig_off[i], in.cig + in.cig_off[i + 1]);
    o.cig_off.push_back((uint32_t)o.cig.size());
  }
}

bool CovRecs::append(uint32_t ng, const std::function<RecView(uint32_t)>& rec, const std::function<void(uint32_t, const RecView&, double*, int64_t*)>& values,
                     int threads) {
  const size_t b = tid.size();
  tid.resize(b + ng), pos.resize(b + ng), flag.resize(b + ng), yc.resize(b + ng), yx.resize(b + ng), strand.resize(b + ng);
  cig_off.resize(b + ng + 1);
  const int T = std::max(1, threads);
  auto par = [&](const std::function<void(uint32_t, uint32_t)>& f) {
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(f, (uint32_t)((uint64_t)ng * t / T), (uint32_t)((uint64_t)ng * (t + 1) / T));
    f(0, (uint32_t)((uint64_t)ng / T));
    for (auto& x : th) x.join();
  };
  par([&](uint32_t lo, uint32_t hi) {
    for (uint32_t g = lo; g < hi; ++g) {
      const RecView v = rec(g);
      const size_t i = b + g;
      tid[i] = v.tid(), pos[i] = v.pos(), flag[i] = v.flag();
      cig_off[i + 1] = v.n_cigar();
      values(g, v, &yc[i], &yx[i]);
      strand[i] = (uint8_t)splice_strand(v);
    }
  });
  uint64_t ops = cig_off[b];
  for (size_t i = b; i < b + ng; ++i) {
    ops += cig_off[i + 1];
    if (ops >= (1ull << 32)) return false;
    cig_off[i + 1] = (uint32_t)ops;
  }
  cig.resize(ops);
  par([&](uint32_t lo, uint32_t hi) {
    for (uint32_t g = lo; g < hi; ++g) {
      const RecView v = rec(g);
      uint32_t* o = cig.data() + cig_off[b + g];
      for (uint32_t c = 0; c < v.n_cigar(); ++c) o[c] = v.cigar(c);
    }
  });
  return true;
}

static int fwrite_sink(void* user, const char* p, uint64_t n) { return fwrite(p, 1, n, (FILE*)user) == n ? 0 : 1; }

TrackStream::TrackStream(const TrackApi& api, const std::vector<std::string>& names, TrackFiles& tf, const TrackRun& run)
    : api_(api), names_(names), tf_(tf), run_(run) {
  // --tabix: a track's writer is open in the place of its FILE* (tabix.h)
  const bool host_fmt = getenv("TBK_TRACK_HOST_FMT") != nullptr;
  if ((tf.cov_tx.is_open() || tf.junc_tx.is_open() || tf.samp_tx.is_open() || tf.strand[0].tx.is_open()) && !host_fmt && !api.track_bgzf) GError("Error: --tabix: libtbk.so lacks tbk_track_bgzf\n");
  if (run.device_text) set_track_names(api, names), names_set_ = true;
}

void TrackStream::tile(const tbk_cov_in& in, bool last) {
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point a) { return std::chrono::duration<double, std::milli>(clock::now() - a).count(); };
  const TrackApi& api = api_;
  const std::vector<std::string>& names = names_;
  TrackFiles& tf = tf_;
  const TrackRun& run = run_;
  TrackTimes& times = times_;
  bool& names_set = names_set_;
  tbk_ctx* ctx = api.ctx;
  const size_t n = in.n_records, co = in.n_cigar_ops;
  const TrackClip* clip = run.clip;
  const size_t extra = clip ? clip->U->n : 0;  // (a clip over a table of R intervals can grow the interval rows by R - 1: the arrays are sized with R added)
  const bool summary = run.summary && run.summary->on();
  const bool depth = run.depth && run.depth->on();
  const bool txjob = run.transcripts && run.transcripts->on();
  const bool cov_tx =tf.cov_tx.is_open(), junc_tx = tf.junc_tx.is_open(), samp_tx = tf.samp_tx.is_open();
  const bool only = last && tiles_ == 0;  // the run's one tile: run_tracks
  // (the summary and a clip take every row of a track in one call: a run of several tiles does not have them)
  if (!only && (summary || txjob || clip || (depth && run.depth->per_feature()))) GError("Error: a summary and a region clip take the rows of one tile\n");
  ++tiles_;
  // a tabix track: the run's one tile as before (written and closed); a tile of several as further runs behind the writer's, the header
  // line with the first rows, the writer closed by end().  A tile without rows for a track writes nothing to it.
  auto tabix = [&](TabixWriter& w, const tbk_track_rows& r, int k) {
    if (only) return write_tabix_track(w, r, names, api, &names_set);
    if (!r.n) return;
    (void)feed_tabix_track(w, r, names, api, &names_set, !tx_started_[k], nullptr);
    tx_started_[k] = true;
  };
  // the text of one plain track: the device formatter, or false (then the caller's host formatter)
  auto device_text = [&](FILE* f, const tbk_track_rows& r) {
    if (!run.device_text) return ++times.host_tracks, false;
    const int rc = api.format_track(ctx, &r, fwrite_sink, f, nullptr);
    if (rc == TBK_EUNSUPPORTED) return ++times.host_tracks, false;
    if (rc == TBK_EINVAL && std::string(api.last_error(ctx)).find("sink") != std::string::npos) GErrorWrite();
    if (rc != 0) GError("Error: GPU track text failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    return true;
  };
  auto rows = [](int kind, uint32_t nr, const int32_t* t, const int32_t* s, const int32_t* e) {
    tbk_track_rows r;
    memset(&r, 0, sizeof(r));
    r.mem = TBK_MEM_HOST, r.kind = kind, r.n = nr, r.tid = t, r.start = s, r.end = e, r.first_junc = 1;
    return r;
  };
  int rc = 0;
  if (tf.cov || tf.cov_bw || tf.junc || cov_tx || junc_tx || summary || depth || txjob) {
    const size_t ci = (tf.cov || tf.cov_bw || cov_tx || summary || depth || txjob) ? 2 * co + 2 * n + 16 + extra : 0, cj = (tf.junc || junc_tx || summary || txjob) ? co + 16 : 0;
    std::vector<int32_t> it(ci ? ci : 1), is(ci ? ci : 1), ie(ci ? ci : 1), jt(cj ? cj : 1), js(cj ? cj : 1), je(cj ? cj : 1);
    std::vector<double> iv(ci ? ci : 1), jv(cj ? cj : 1);
    std::vector<uint8_t> jstr(cj ? cj : 1);
    tbk_cov_out o;
    memset(&o, 0, sizeof(o));
    o.mem = TBK_MEM_HOST;
    o.cap_intervals = (uint32_t)ci;
    o.iv_tid = it.data(), o.iv_start = is.data(), o.iv_end = ie.data(), o.iv_val = iv.data();
    o.cap_junctions = (uint32_t)cj;
    o.j_tid = jt.data(), o.j_start = js.data(), o.j_end = je.data(), o.j_strand = jstr.data(), o.j_val = jv.data();
    auto a = clock::now();
    rc = api.coverage_tile(ctx, &in, &o);
    times.ms_cov += ms_since(a);
    n_bases_ += o.n_bases, span_bases_ += o.span_bases;
    if (rc == TBK_EFATALOP) GError("ERROR: unknown opcode in a CIGAR string (tiecov accepts M, I, D, N, S only)\n");
    if (rc != 0) GError("Error: GPU coverage failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    if (summary) write_summary(*run.summary, names, o, api);
    if (depth) depth_tile(o);
    if (txjob) tx_tile(o);
    if (clip) {
      const tbk_regions* U = clip->U;
      rc = clip->one ? api.cov_clip(ctx, &o, U->tid[0], U->beg[0], U->end[0]) : api.cov_clip_regions(ctx, &o, U);
      if (rc != 0) GError("Error: GPU clip failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    }
    tbk_track_rows rcov = rows(TBK_TRACK_COV, o.n_intervals, it.data(), is.data(), ie.data());
    rcov.val = iv.data();
    tbk_track_rows rjunc = rows(TBK_TRACK_JUNC, o.n_junctions, jt.data(), js.data(), je.data());
    rjunc.val = jv.data(), rjunc.strand = jstr.data(), rjunc.first_junc = first_junc_;  // (JUNC%08d runs on over the tiles)
    if (tf.cov) {  // flushCoverage, tiecov.cpp:237
      a = clock::now();
      if (!device_text(tf.cov, rcov)) emit_cov_lines(tf.cov, names, o.n_intervals, it.data(), is.data(), ie.data(), iv.data());
      times.ms_text += ms_since(a);
    }
    if (tf.cov_bw) {  // flushCoverage(bigWigFile_t*), tiecov.cpp:243-275: the same intervals, the value as a float
      if (run.bw_device && !api.bigwig_build) GError("Error: --bigwig-writer device: libtbk.so lacks tbk_bigwig_build\n");
      if (only) {
        tf.write_bigwig(o.n_intervals, it.data(), is.data(), ie.data(), iv.data(), run.bw_device ? &api : nullptr);
      } else {  // the host writer keeps its items: the file is closed by end()
        if (run.bw_device) GError("Error: --bigwig-writer device takes the rows of one tile\n");
        for (uint32_t i = 0; i < o.n_intervals; ++i) tf.bw.add((uint32_t)it[i], (uint32_t)is[i], (uint32_t)ie[i], (float)iv[i]);
      }
    }
    if (tf.junc) {  // CJunc::write, tiecov.cpp:91-95 (numbered from 1)
      a = clock::now();
      if (!device_text(tf.junc, rjunc)) emit_junc_lines(tf.junc, names, o.n_junctions, jt.data(), js.data(), je.data(), jv.data(), jstr.data(), first_junc_);
      times.ms_text += ms_since(a);
    }
    first_junc_ += o.n_junctions;
    a = clock::now();
    if (cov_tx) tabix(tf.cov_tx, rcov, 0);
    if (junc_tx) tabix(tf.junc_tx, rjunc, 1);
    times.ms_text += ms_since(a);
  }
  if (tf.samp || samp_tx) {
    // the value of the track changes only where an M segment starts or ends: at most 2 intervals per CIGAR operation + 2 per
    // record, as for the coverage track (not one per covered base); if a call still reports TBK_E2BIG it also reports the
    // count it needs, and the call is repeated with that
    size_t cs = 2 * co + 2 * n + 16 + extra;
    std::vector<int32_t> st, ss, se;
    std::vector<int64_t> sc;
    std::vector<float> sh;
    tbk_sample_out so;
    auto a = clock::now();
    for (int attempt = 0; attempt < 2; ++attempt) {
      st.resize(cs), ss.resize(cs), se.resize(cs), sc.resize(cs), sh.resize(cs);
      memset(&so, 0, sizeof(so));
      so.mem = TBK_MEM_HOST;
      so.cap_intervals = (uint32_t)cs;
      so.iv_tid = st.data(), so.iv_start = ss.data(), so.iv_end = se.data(), so.iv_count = sc.data(), so.iv_heat = sh.data();
      rc = api.sample_tile(ctx, &in, run.num_samples, &so);
      if (rc != TBK_E2BIG) break;
      cs = (size_t)so.n_intervals + 16 + extra;
    }
    times.ms_samp += ms_since(a);
    if (rc == TBK_EFATALOP) GError("ERROR: unknown opcode in a CIGAR string (tiecov accepts M, I, D, N, S only)\n");
    if (rc != 0) GError("Error: GPU sample track failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    if (clip) {
      const tbk_regions* U = clip->U;
      rc = clip->one ? api.sample_clip(ctx, &so, U->tid[0], U->beg[0], U->end[0]) : api.sample_clip_regions(ctx, &so, U);
      if (rc != 0) GError("Error: GPU clip failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    }
    tbk_track_rows r = rows(TBK_TRACK_SAMPLE, so.n_intervals, st.data(), ss.data(), se.data());
    r.count = sc.data(), r.heat = sh.data();
    a = clock::now();
    if (samp_tx) tabix(tf.samp_tx, r, 2);
    else if (!device_text(tf.samp, r)) emit_samp_lines(tf.samp, names, so.n_intervals, st.data(), ss.data(), se.data(), sc.data(), sh.data());  // flushCoverage(pair), tiecov.cpp:289
    times.ms_text += ms_since(a);
  }
  if (tf.strand_on()) {
    // --strand-cov: the tile divided by splice strand, the coverage chain on each part (intervals only), the rows cut by
    // the run's clip and written as the coverage rows are.  A tile cut at a bundle head of the whole stream is cut at a bundle head of
    // each part, so a part's rows over the tiles are its rows over the uncut stream.  (n_bases_ / span_bases_ stay the whole tile's.)
    const bool host = split_host_asked();
    tbk_cov_in part[3];
    CovRecs hrec[3];
    auto a = clock::now();
    if (host) {
      // (the command lines refuse this before a file exists, refuse_split_host_on_device; a caller that did not: the files go with the run)
      if (in.mem != TBK_MEM_HOST && in.n_records) {
        tf.discard();
        GError("Error: TBK_SPLIT_HOST=1 divides host records; the records of this run are on the device\n");
      }
      split_strand_host(in, hrec);
      for (int s = 0; s < 3; ++s) part[s] = hrec[s].as_cov_in();
    } else {
      if (!api.cov_split_strand) GError("Error: --strand-cov: the loaded libtbk.so has no tbk_cov_split_strand (an older build?)\n");
      rc = api.cov_split_strand(ctx, &in, part);
      if (rc == TBK_E2BIG) GError("Error: input too large for one tile\n");
      if (rc != 0) GError("Error: GPU strand split failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
    }
    ms_split_ += ms_since(a);
    strand_host_ = host;
    for (int s = 0; s < 3; ++s) {
      CovSink& k = tf.strand[s];
      const size_t pn = part[s].n_records, pco = part[s].n_cigar_ops;
      strand_records_[s] += pn;
      const size_t ci = 2 * pco + 2 * pn + 16 + extra;
      std::vector<int32_t> it(ci), is(ci), ie(ci);
      std::vector<double> iv(ci);
      tbk_cov_out o;
      memset(&o, 0, sizeof(o));
      o.mem = TBK_MEM_HOST;
      o.cap_intervals = (uint32_t)ci;
      o.iv_tid = it.data(), o.iv_start = is.data(), o.iv_end = ie.data(), o.iv_val = iv.data();
      a = clock::now();
      rc = api.coverage_tile(ctx, &part[s], &o);
      if (rc == TBK_EFATALOP) GError("ERROR: unknown opcode in a CIGAR string (tiecov accepts M, I, D, N, S only)\n");
      if (rc != 0) GError("Error: GPU coverage failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
      if (clip) {
        const tbk_regions* U = clip->U;
        rc = clip->one ? api.cov_clip(ctx, &o, U->tid[0], U->beg[0], U->end[0]) : api.cov_clip_regions(ctx, &o, U);
        if (rc != 0) GError("Error: GPU clip failed: %s (%s)\n", api.strerror_(rc), api.last_error(ctx));
      }
      ms_strand_cov_ += ms_since(a);
      tbk_track_rows rcov = rows(TBK_TRACK_COV, o.n_intervals, it.data(), is.data(), ie.data());
      rcov.val = iv.data();
      a = clock::now();
      if (k.f && !device_text(k.f, rcov)) emit_cov_lines(k.f, names, o.n_intervals, it.data(), is.data(), ie.data(), iv.data());
      if (k.is_bw) {
        if (run.bw_device && !api.bigwig_build) GError("Error: --bigwig-writer device: libtbk.so lacks tbk_bigwig_build\n");
        if (only) {
          tf.write_strand_bigwig(s, o.n_intervals, it.data(), is.data(), ie.data(), iv.data(), run.bw_device ? &api : nullptr);
        } else {
          if (run.bw_device) GError("Error: --bigwig-writer device takes the rows of one tile\n");
          for (uint32_t i = 0; i < o.n_intervals; ++i) k.bw.add((uint32_t)it[i], (uint32_t)is[i], (uint32_t)ie[i], (float)iv[i]);
        }
      }
      if (k.tx.is_open()) tabix(k.tx, rcov, 3 + s);
      ms_strand_text_ += ms_since(a);
    }
  }
}

void TrackStream::end() {
  TabixWriter* const tx[6] = {&tf_.cov_tx, &tf_.junc_tx, &tf_.samp_tx, &tf_.strand[0].tx, &tf_.strand[1].tx, &tf_.strand[2].tx};
  for (int k = 0; k < 6; ++k) {  // (a writer that got rows tile by tile; one that got none is TrackFiles::close's: header, EOF member, empty index)
    std::string err;
    if (tx_started_[k] && !tx[k]->close(err)) GError("Error: writing %s failed (%s)\n", tx[k]->path().c_str(), err.c_str());
  }
  const bool strand_on = tf_.strand_on();
  tf_.close();
  if (strand_on && getenv("TBK_TIMING"))
    fprintf(stderr, "strand phase ms: %s | %llu+ %llu- %llu. records | %.1f | %.1f | %.1f\n", strand_host_ ? "host" : "device",
            (unsigned long long)strand_records_[0], (unsigned long long)strand_records_[1], (unsigned long long)strand_records_[2], ms_split_, ms_strand_cov_,
            ms_strand_text_);
  if (run_.depth && run_.depth->on()) {  // (behind the tracks: a run that failed before this left neither table)
    const auto t0 = std::chrono::steady_clock::now();
    const DepthJob& job = *run_.depth;
    std::string err;
    if (job.per_ref()) {
      if (depth_.covered.size() != job.lens.size()) depth_.resize(job.lens.size(), job.thr.size());  // (no tile at all)
      if (!write_depth_tsv(job.summary_out, names_, job.lens, job.thr_text, depth_, err)) GError("Error: --depth-summary: %s\n", err.c_str());
    }
    if (job.per_feature()) {
      if (fd_covered_.size() != job.F.n()) fd_covered_.assign(job.F.n(), 0), fd_ge_.assign(job.F.n() * job.thr.size(), 0);
      if (!write_feature_depth_tsv(job.feature_out, names_, job.F, job.thr_text, fd_covered_.data(), fd_ge_.data(), err)) {
        if (job.per_ref()) (void)unlink(job.summary_out.c_str());
        GError("Error: --feature-depth: %s\n", err.c_str());
      }
    }
    ms_depth_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (getenv("TBK_TIMING"))
      fprintf(stderr, "depth phase ms: %s | %zu references | %zu features | %zu thresholds | %llu interval rows in %llu tiles | %.1f\n", depth_host_ ? "host" : "device",
              job.per_ref() ? job.lens.size() : (size_t)0, job.F.n(), job.thr.size(), (unsigned long long)depth_rows_, (unsigned long long)tiles_, ms_depth_);
  }
  if (run_.transcripts && run_.transcripts->on()) {  // (behind the tracks and the depth tables: a run that failed before this left no file)
    const auto t0 = std::chrono::steady_clock::now();
    const TxJob& job = *run_.transcripts;
    if (tx_.covered.size() != job.X.n_tx()) tx_.resize(job.X.n_tx(), job.X.n_exon());  // (no tile at all)
    std::string err;
    if (!write_transcripts_tsv(job.out, names_, job.X, tx_, err)) {
      if (run_.depth && run_.depth->per_ref()) (void)unlink(run_.depth->summary_out.c_str());
      if (run_.depth && run_.depth->per_feature()) (void)unlink(run_.depth->feature_out.c_str());
      GError("Error: --transcripts: %s\n", err.c_str());
    }
    ms_tx_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (getenv("TBK_TIMING"))
      fprintf(stderr, "transcripts phase ms: %s | %zu transcripts, %zu exons | %.1f\n", tx_host_ ? "host" : "device", job.X.n_tx(), job.X.n_exon(), ms_tx_);
  }
  if (run_.times) *run_.times = times_;
}

void run_tracks(const TrackApi& api, const tbk_cov_in& in, const std::vector<std::string>& names, TrackFiles& tf, const TrackRun& run) {
  TrackStream s(api, names, tf, run);
  s.tile(in, true);
  s.end();
}

void TrackFiles::discard() {
  std::string err;
  if (cov_bw) (void)bw.close(err), cov_bw = false;
  if (cov && cov != stdout) fclose(cov);
  if (junc) fclose(junc);
  if (samp) fclose(samp);
  cov = junc = samp = nullptr;
  for (CovSink& k : strand) {
    if (k.is_bw) (void)k.bw.close(err), k.is_bw = false;
    if (k.f) fclose(k.f);
    k.f = nullptr;
  }
  for (TabixWriter* w : {&cov_tx, &junc_tx, &samp_tx, &strand[0].tx, &strand[1].tx, &strand[2].tx})
    if (w->is_open()) w->discard();
  for (const std::string* p : {&cov_name, &junc_name, &samp_name, &strand[0].name, &strand[1].name, &strand[2].name})
    if (!p->empty() && *p != "-" && *p != "stdout") (void)unlink(p->c_str());
}

}  // namespace tbh
