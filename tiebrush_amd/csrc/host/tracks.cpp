// tracks.cpp — see tracks.h
#include "tracks.h"

#include <string.h>

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

void TrackFiles::open(std::string cov_prefix, std::string junc_prefix, std::string samp_prefix, bool bigwig, const std::vector<std::string>& names,
                      const std::vector<uint32_t>& lens, bool tabix) {
  if (tabix) {  // every text track; the coverage as a bigWig stays what it is below
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
    fprintf(junc, "%s", kJuncHead);
  }
  if (!samp_prefix.empty()) {
    if (!ends_with(samp_prefix, ".bedgraph")) samp_prefix += ".bedgraph";
    samp = fopen(samp_prefix.c_str(), "w");
    if (!samp) GError("Error creating file %s\n", samp_prefix.c_str());
    fprintf(samp, "%s", kSampHead);
  }
}

void TrackFiles::close_bigwig() {
  if (!cov_bw) return;
  std::string err;
  if (!bw.close(err)) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
  cov_bw = false;
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

void TrackFiles::write_bigwig(uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end, const double* val, const BigWigDevice* dev) {
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
          rc = dev->build(dev->ctx, &r, (uint32_t)bw_lens.size(), bw_lens.data(), BwBridge::sink, &b, &out);
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

void TrackFiles::close() {
  close_bigwig();
  if (cov && cov != stdout) fclose(cov);
  if (cov == stdout) fflush(stdout);
  if (junc) fclose(junc);
  if (samp) fclose(samp);
  cov = junc = samp = nullptr;
  for (TabixWriter* w : {&cov_tx, &junc_tx, &samp_tx}) {  // (a track nobody wrote rows to: its header, the EOF member, an empty index)
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

void write_summary(const SummaryJob& job, const std::vector<std::string>& names, const tbk_cov_out& rows, const SummaryDevice& dev) {
  const auto t0 = std::chrono::steady_clock::now();
  const FeatureTable& F = job.F;
  const bool host = getenv("TBK_SUMMARY_HOST") && strcmp(getenv("TBK_SUMMARY_HOST"), "0") != 0;
  FeatSummary S;
  if (host) {
    summarise_features(F, true, rows.n_intervals, rows.iv_tid, rows.iv_start, rows.iv_end, rows.iv_val, true, rows.n_junctions, rows.j_tid, rows.j_start,
                       rows.j_end, rows.j_strand, rows.j_val, S);
  } else {
    if (!dev.summary) GError("Error: --summary: the loaded libtbk.so has no tbk_cov_summary (an older build?)\n");
    S.resize(F.n());
    tbk_features f;
    f.n = (uint32_t)F.n(), f.tid = F.tid.data(), f.beg = F.beg.data(), f.end = F.end.data(), f.strand = F.strand.data();
    tbk_feat_out o;
    o.mem = TBK_MEM_HOST, o.covered = S.covered.data(), o.sum = S.sum.data(), o.max = S.max.data(), o.junc = S.junc.data();
    const int rc = dev.summary(dev.ctx, &rows, &f, &o);
    if (rc != 0) GError("Error: GPU feature summary failed: %s (%s)\n", dev.strerror_(rc), dev.last_error(dev.ctx));
  }
  std::string err;
  if (!write_summary_tsv(job.out, names, F, S, err)) GError("Error: --summary: %s\n", err.c_str());
  if (getenv("TBK_TIMING"))
    fprintf(stderr, "summary phase ms: %s | %zu features | %u interval rows | %u junction rows | %.1f\n", host ? "host" : "device", F.n(), rows.n_intervals,
            rows.n_junctions, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

}  // namespace tbh
