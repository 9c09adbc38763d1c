// tracks.cpp — see tracks.h
#include "tracks.h"

#include <string.h>

#include <algorithm>

#include "GSam.h"

namespace tbh {

static bool ends_with(const std::string& s, const char* suf) {
  size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

void TrackFiles::open(std::string cov_prefix, std::string junc_prefix, std::string samp_prefix, bool bigwig, const std::vector<std::string>& names,
                      const std::vector<uint32_t>& lens) {
  if (!cov_prefix.empty()) {
    if (cov_prefix == "-" || cov_prefix == "stdout") {
      cov = stdout;
    } else if (bigwig) {  // tiecov.cpp:365-402
      if (!ends_with(cov_prefix, ".bigwig")) cov_prefix += ".bigwig";
      std::string err;
      if (!bw.open(cov_prefix, names, lens, err)) GError("Error creating file %s\n", cov_prefix.c_str());
      cov_bw = true;
    } else {
      if (!ends_with(cov_prefix, ".bedgraph")) cov_prefix += ".bedgraph";
      cov = fopen(cov_prefix.c_str(), "w");
      if (!cov) GError("Error creating file %s\n", cov_prefix.c_str());
      fprintf(cov, "track type=bedGraph\n");
    }
    cov_name = cov_prefix;
  }
  if (!junc_prefix.empty()) {
    if (!ends_with(junc_prefix, ".bed")) junc_prefix += ".bed";
    junc = fopen(junc_prefix.c_str(), "w");
    if (!junc) GError("Error creating file %s\n", junc_prefix.c_str());
    fprintf(junc, "track name=junctions\n");
  }
  if (!samp_prefix.empty()) {
    if (!ends_with(samp_prefix, ".bedgraph")) samp_prefix += ".bedgraph";
    samp = fopen(samp_prefix.c_str(), "w");
    if (!samp) GError("Error creating file %s\n", samp_prefix.c_str());
    fprintf(samp,
            "track type=bedGraph name=\"Sample Count Heatmap\" description=\"Sample Count Heatmap\" visibility=full "
            "graphType=\"heatmap\" color=200,100,0 altColor=0,100,200\n");
  }
}

void TrackFiles::close_bigwig() {
  if (!cov_bw) return;
  std::string err;
  if (!bw.close(err)) GError("Error: writing %s failed (%s)\n", cov_name.c_str(), err.c_str());
  cov_bw = false;
}

void TrackFiles::close() {
  close_bigwig();
  if (cov && cov != stdout) fclose(cov);
  if (cov == stdout) fflush(stdout);
  if (junc) fclose(junc);
  if (samp) fclose(samp);
  cov = junc = samp = nullptr;
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

}  // namespace tbh
