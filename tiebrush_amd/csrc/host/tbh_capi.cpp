// tbh_capi.cpp — libtbh.so: the C ABI of include/tbh_host.h over the host codec (tagging + BGZF deflate of a rank's slice of the
// output, the output header + concatenation of the ranks' parts).  No GPU code.
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "../../../include/tbh_host.h"
#include "GSam.h"
#include "bai.h"
#include "bai_read.h"
#include "bgzf.h"
#include "tagwrite.h"
#include "tmerge.h"
#include "tracks.h"

namespace {
thread_local std::string g_err;
int fail(const std::string& m) {
  g_err = m;
  return -1;
}
}  // namespace

extern "C" {

int tbh_abi_version(void) { return TBH_ABI_VERSION; }
const char* tbh_last_error(void) { return g_err.c_str(); }

int tbh_tag_deflate_part(const uint8_t* blob, const uint64_t* rec_off, const uint32_t* rec_len, uint32_t n, const double* yc, const int64_t* yx,
                         const int32_t* yd, int level, int threads, const char* out_path) {
  if (!out_path || (n && (!blob || !rec_off || !rec_len || !yc || !yx || !yd))) return fail("tbh_tag_deflate_part: null argument");
  int nt = threads > 0 ? threads : tbh::cpu_budget();
  if (nt > 128) nt = 128;
  auto rec = [&](uint32_t g) {
    tbh::RecView v;
    v.p = blob + rec_off[g];
    v.len = rec_len[g];
    return v;
  };
  FILE* f = fopen(out_path, "wb");
  if (!f) return fail(std::string("tbh_tag_deflate_part: cannot open ") + out_path);
  bool wrote = true;
  auto emit = [&](const uint8_t* p, size_t sz) { return wrote = fwrite(p, 1, sz, f) == sz; };
  const bool ok = tbh::tag_deflate_ordered(n, rec, yc, yx, yd, level, nt, emit);
  if (fclose(f) == 0 && ok) return 0;
  (void)unlink(out_path);  // (no half-written part is left behind)
  return fail(ok || !wrote ? std::string("tbh_tag_deflate_part: write failed on ") + out_path : std::string("tbh_tag_deflate_part: deflate failed"));
}

int tbh_write_bam_parts(const char* out_path, const char* version, int cmd_argc, const char* const* cmd_argv, int n_files, const char* const* files,
                        int n_parts, const char* const* parts, int remove_parts) {
  if (!out_path || !version || n_files <= 0 || !files || n_parts < 0 || (n_parts && !parts)) return fail("tbh_write_bam_parts: bad argument");
  // the header exactly as the single-GPU command line builds it: TInputFiles opens every input (header + first record), merges the
  // @SQ tables, lists the samples in @CO lines and adds its @PG line (tmerge.cpp: addSam)
  TInputFiles in;
  std::vector<char*> av;
  for (int i = 0; i < cmd_argc; ++i) av.push_back(const_cast<char*>(cmd_argv[i]));
  in.setup(version, cmd_argc, av.data());
  for (int i = 0; i < n_files; ++i) in.addFile(tbh_realpath(files[i]).c_str());
  in.start();
  // written beside the target and renamed when complete: a part that cannot be read must not leave a well-formed but truncated BAM
  const std::string tmp = std::string(out_path) + ".tmp";
  std::string bad;
  {
    GSamWriter out(tmp.c_str(), in.header(), GSamFile_BAM);
    std::vector<uint8_t> buf((size_t)8 << 20);
    for (int p = 0; p < n_parts && bad.empty(); ++p) {
      FILE* f = fopen(parts[p], "rb");
      if (!f) {
        bad = std::string("tbh_write_bam_parts: cannot open ") + parts[p];
        break;
      }
      size_t got;
      while ((got = fread(buf.data(), 1, buf.size(), f)) > 0) out.write_members(buf.data(), got);
      if (ferror(f)) bad = std::string("tbh_write_bam_parts: read failed on ") + parts[p];
      fclose(f);
    }
  }  // (closing the writer appends the EOF member)
  in.stop();
  if (bad.empty() && rename(tmp.c_str(), out_path) != 0) bad = std::string("tbh_write_bam_parts: cannot rename to ") + out_path;
  if (!bad.empty()) {
    (void)unlink(tmp.c_str());
    return fail(bad);
  }
  if (remove_parts)
    for (int p = 0; p < n_parts; ++p) (void)unlink(parts[p]);
  return 0;
}

int tbh_is_tiebrush(const char* path) {
  if (!path) return -1;
  tbh::BamFile bf;
  std::string err;
  if (!bf.open(path, err, 1)) {
    g_err = err;
    return -1;
  }
  return bf.hdr.is_tiebrush() ? 1 : 0;
}

int tbh_bai_index_file(const char* bam_path, const char* bai_path) {
  if (!bam_path) return fail("tbh_bai_index_file: null argument");
  std::string err;
  if (!tbh::bai_index_file(bam_path, bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai", err)) return fail("tbh_bai_index_file: " + err);
  return 0;
}
uint32_t tbh_bai_reg2bin(int64_t beg, int64_t end) { return tbh::bai_reg2bin(beg, end); }

int tbh_csi_index_file(const char* bam_path, const char* csi_path) {
  if (!bam_path) return fail("tbh_csi_index_file: null argument");
  std::string err;
  if (!tbh::bai_index_file(bam_path, csi_path ? std::string(csi_path) : std::string(bam_path) + ".csi", err, true)) return fail("tbh_csi_index_file: " + err);
  return 0;
}
int tbh_csi_depth(uint64_t max_len) { return tbh::csi_depth(max_len); }
uint32_t tbh_csi_reg2bin(int64_t beg, int64_t end, int depth) {
  return depth < 0 || depth > tbh::kCsiMaxDepth || beg < 0 || end <= beg || end > (1ll << (14 + 3 * depth)) ? UINT32_MAX : tbh::bai_reg2bin(beg, end, depth);
}


int64_t tbh_index_query(const char* bam_path, const char* index_path, int32_t tid, int64_t beg, int64_t end, uint64_t* chunk_beg, uint64_t* chunk_end,
                        uint64_t cap) {
  if (!bam_path || (cap && (!chunk_beg || !chunk_end))) return fail("tbh_index_query: null argument");
  std::string err;
  std::vector<tbh::IdxChunk> ch;
  if (!tbh::index_query_file(bam_path, index_path ? index_path : "", tid, beg, end, ch, err)) return fail("tbh_index_query: " + err);
  if (ch.size() <= cap)
    for (size_t i = 0; i < ch.size(); ++i) chunk_beg[i] = ch[i].beg, chunk_end[i] = ch[i].end;
  return (int64_t)ch.size();
}

int64_t tbh_regions_from_bed(const char* bam_path, const char* bed_path, int32_t* tid, int64_t* beg, int64_t* end, uint64_t cap) {
  if (!bam_path || !bed_path || (cap && (!tid || !beg || !end))) return fail("tbh_regions_from_bed: null argument");
  std::string err;
  tbh::BamFile bf;
  if (!bf.open(bam_path, err, 1)) return fail("tbh_regions_from_bed: " + err);
  tbh::RegionTable U;
  if (!tbh::regions_from_bed_file(bf.hdr, bed_path, U, err)) return fail("tbh_regions_from_bed: " + err);
  if (U.n() <= cap)
    for (size_t r = 0; r < U.n(); ++r) tid[r] = U.tid[r], beg[r] = U.beg[r], end[r] = U.end[r];
  return (int64_t)U.n();
}

int64_t tbh_index_query_regions(const char* bam_path, const char* index_path, uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end,
                                uint64_t* chunk_beg, uint64_t* chunk_end, uint64_t cap) {
  if (!bam_path || !n || !tid || !beg || !end || (cap && (!chunk_beg || !chunk_end))) return fail("tbh_index_query_regions: null argument or an empty table");
  tbh::RegionTable U;
  for (uint32_t r = 0; r < n; ++r) U.add(tid[r], beg[r], end[r]);
  std::string err;
  std::vector<tbh::IdxChunk> ch;
  if (!tbh::index_query_regions_file(bam_path, index_path ? index_path : "", U, ch, err)) return fail("tbh_index_query_regions: " + err);
  if (ch.size() <= cap)
    for (size_t i = 0; i < ch.size(); ++i) chunk_beg[i] = ch[i].beg, chunk_end[i] = ch[i].end;
  return (int64_t)ch.size();
}

int64_t tbh_features_from_bed(const char* bam_path, const char* bed_path, int32_t* tid, int64_t* beg, int64_t* end, uint8_t* strand, uint64_t* line,
                              uint64_t cap, char* names, uint64_t names_cap, uint64_t* names_bytes) {
  if (!bam_path || !bed_path || (cap && (!tid || !beg || !end || !strand || !line)) || (names_cap && !names)) return fail("tbh_features_from_bed: null argument");
  std::string err;
  tbh::BamFile bf;
  if (!bf.open(bam_path, err, 1)) return fail("tbh_features_from_bed: " + err);
  tbh::FeatureTable F;
  if (!tbh::features_from_bed_file(bf.hdr, bed_path, F, err)) return fail("tbh_features_from_bed: " + err);
  if (F.n() <= cap)
    for (size_t i = 0; i < F.n(); ++i) tid[i] = F.tid[i], beg[i] = F.beg[i], end[i] = F.end[i], strand[i] = F.strand[i], line[i] = F.line[i];
  uint64_t nb = 0;
  for (const std::string& s : F.name) nb += s.size() + 1;
  if (names_bytes) *names_bytes = nb;
  if (nb <= names_cap) {
    char* p = names;
    for (const std::string& s : F.name) memcpy(p, s.c_str(), s.size() + 1), p += s.size() + 1;
  }
  return (int64_t)F.n();
}

int tbh_cov_summary_host(uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end, const uint8_t* strand, int want_cov, uint32_t n_intervals,
                         const int32_t* iv_tid, const int32_t* iv_start, const int32_t* iv_end, const double* iv_val, int want_junc, uint32_t n_junctions,
                         const int32_t* j_tid, const int32_t* j_start, const int32_t* j_end, const uint8_t* j_strand, const double* j_val,
                         uint64_t* covered, double* sum, double* max, double* junc) {
  if (!n || !tid || !beg || !end || (want_cov && (!covered || !sum || !max)) || (want_junc && !junc)) return fail("tbh_cov_summary_host: null argument or no feature");
  if ((want_cov && n_intervals && (!iv_tid || !iv_start || !iv_end || !iv_val)) || (want_junc && n_junctions && (!j_tid || !j_start || !j_end || !j_strand || !j_val)))
    return fail("tbh_cov_summary_host: null rows");
  tbh::FeatureTable F;
  F.tid.assign(tid, tid + n), F.beg.assign(beg, beg + n), F.end.assign(end, end + n);
  if (strand) F.strand.assign(strand, strand + n);
  else F.strand.assign(n, (uint8_t)'.');
  tbh::FeatSummary S;
  tbh::summarise_features(F, want_cov != 0, n_intervals, iv_tid, iv_start, iv_end, iv_val, want_junc != 0, n_junctions, j_tid, j_start, j_end, j_strand, j_val, S);
  if (want_cov) memcpy(covered, S.covered.data(), (size_t)n * 8), memcpy(sum, S.sum.data(), (size_t)n * 8), memcpy(max, S.max.data(), (size_t)n * 8);
  if (want_junc) memcpy(junc, S.junc.data(), (size_t)n * 8);
  return 0;
}

int tbh_cov_thresholds_host(uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end, uint32_t n_intervals, const int32_t* iv_tid,
                            const int32_t* iv_start, const int32_t* iv_end, const double* iv_val, const double* thr, uint32_t n_thr, uint64_t* covered,
                            uint64_t* ge) {
  if (!n || !tid || !beg || !end || !thr || !ge) return fail("tbh_cov_thresholds_host: null argument or no feature");
  if (n_intervals && (!iv_tid || !iv_start || !iv_end || !iv_val)) return fail("tbh_cov_thresholds_host: null rows");
  if (n_thr < 1 || n_thr > TBK_MAX_THRESHOLDS) return fail("tbh_cov_thresholds_host: between 1 and 16 thresholds");
  for (uint32_t k = 0; k < n_thr; ++k)
    if (!(thr[k] > 0.0) || thr[k] - thr[k] != 0.0 || (k && !(thr[k] > thr[k - 1]))) return fail("tbh_cov_thresholds_host: thresholds are finite, > 0 and strictly ascending");
  tbh::threshold_features(n, tid, beg, end, n_intervals, iv_tid, iv_start, iv_end, iv_val, thr, n_thr, covered, ge);
  return 0;
}

int tbh_parse_thresholds(const char* list, double* thr, uint32_t cap) {
  if (!list || !thr || cap < TBK_MAX_THRESHOLDS) return (int)fail("tbh_parse_thresholds: null argument or room for fewer than 16");
  std::vector<double> v;
  std::vector<std::string> text;
  std::string err;
  if (!tbh::parse_thresholds(list, v, text, err)) return (int)fail("--thresholds: " + err);
  for (size_t k = 0; k < v.size(); ++k) thr[k] = v[k];
  return (int)v.size();
}

int64_t tbh_transcripts_from_gtf(const char* bam_path, const char* gtf_path, uint32_t* tx_off, int32_t* tid, uint8_t* strand, uint64_t* line, uint64_t tx_cap,
                                 int64_t* ex_beg, int64_t* ex_end, uint64_t ex_cap, uint64_t* n_exon, char* names, uint64_t names_cap, uint64_t* names_bytes) {
  if (!bam_path || !gtf_path || !n_exon || (tx_cap && (!tx_off || !tid || !strand || !line)) || (ex_cap && (!ex_beg || !ex_end)) || (names_cap && !names))
    return fail("tbh_transcripts_from_gtf: null argument");
  std::string err;
  tbh::BamFile bf;
  if (!bf.open(bam_path, err, 1)) return fail("tbh_transcripts_from_gtf: " + err);
  tbh::TranscriptTable X;
  if (!tbh::transcripts_from_gtf_file(bf.hdr, gtf_path, X, err)) return fail("tbh_transcripts_from_gtf: " + err);
  *n_exon = X.n_exon();
  if (X.n_tx() <= tx_cap) {
    memcpy(tx_off, X.tx_off.data(), (X.n_tx() + 1) * 4);
    for (size_t t = 0; t < X.n_tx(); ++t) tid[t] = X.tid[t], strand[t] = X.strand[t], line[t] = X.line[t];
  }
  if (X.n_exon() <= ex_cap) memcpy(ex_beg, X.ex_beg.data(), X.n_exon() * 8), memcpy(ex_end, X.ex_end.data(), X.n_exon() * 8);
  uint64_t nb = 0;
  for (size_t t = 0; t < X.n_tx(); ++t) nb += X.id[t].size() + X.gene[t].size() + 2;
  if (names_bytes) *names_bytes = nb;
  if (nb <= names_cap) {
    char* p = names;
    for (size_t t = 0; t < X.n_tx(); ++t)
      for (const std::string* s : {&X.id[t], &X.gene[t]}) memcpy(p, s->c_str(), s->size() + 1), p += s->size() + 1;
  }
  return (int64_t)X.n_tx();
}

int tbh_tx_summary_host(uint32_t n_tx, uint32_t n_exon, const uint32_t* tx_off, const int32_t* tid, const uint8_t* strand, const int64_t* ex_beg,
                        const int64_t* ex_end, int want_cov, uint32_t n_intervals, const int32_t* iv_tid, const int32_t* iv_start, const int32_t* iv_end,
                        const double* iv_val, int want_junc, uint32_t n_junctions, const int32_t* j_tid, const int32_t* j_start, const int32_t* j_end,
                        const uint8_t* j_strand, const double* j_val, uint64_t* covered, double* sum, double* max, uint32_t* exons_hit, uint32_t* introns_hit,
                        double* junc_min, double* junc_sum, uint64_t* ex_covered, double* ex_sum, double* ex_max, double* in_junc) {
  if (!n_tx || !n_exon || !tx_off || !tid || !ex_beg || !ex_end || (want_cov && (!covered || !sum || !max || !exons_hit)) ||
      (want_junc && (!introns_hit || !junc_min || !junc_sum)))
    return fail("tbh_tx_summary_host: null argument or no transcript");
  if ((want_cov && n_intervals && (!iv_tid || !iv_start || !iv_end || !iv_val)) || (want_junc && n_junctions && (!j_tid || !j_start || !j_end || !j_strand || !j_val)))
    return fail("tbh_tx_summary_host: null rows");
  if (tx_off[0] != 0 || tx_off[n_tx] != n_exon) return fail("tbh_tx_summary_host: tx_off does not run from 0 to n_exon");
  for (uint32_t t = 0; t < n_tx; ++t) {
    if (tx_off[t + 1] <= tx_off[t] || tx_off[t + 1] > n_exon || tid[t] < 0 || (strand && strand[t] != '+' && strand[t] != '-' && strand[t] != '.'))
      return fail("tbh_tx_summary_host: a transcript without an exon, a tid < 0 or a strand other than + - .");
    for (uint32_t e = tx_off[t]; e < tx_off[t + 1]; ++e)
      if (ex_beg[e] < 0 || ex_end[e] <= ex_beg[e] || (e > tx_off[t] && ex_beg[e] <= ex_end[e - 1]))
        return fail("tbh_tx_summary_host: the exons of a transcript are not empty, ascending and apart");
  }
  tbh::TranscriptTable X;
  X.tx_off.assign(tx_off, tx_off + n_tx + 1), X.tid.assign(tid, tid + n_tx), X.ex_beg.assign(ex_beg, ex_beg + n_exon), X.ex_end.assign(ex_end, ex_end + n_exon);
  if (strand) X.strand.assign(strand, strand + n_tx);
  else X.strand.assign(n_tx, (uint8_t)'.');
  tbh::TxSummary S;
  tbh::summarise_transcripts(X, want_cov != 0, n_intervals, iv_tid, iv_start, iv_end, iv_val, want_junc != 0, n_junctions, j_tid, j_start, j_end, j_strand, j_val, S);
  if (want_cov) {
    memcpy(covered, S.covered.data(), (size_t)n_tx * 8), memcpy(sum, S.sum.data(), (size_t)n_tx * 8), memcpy(max, S.max.data(), (size_t)n_tx * 8);
    memcpy(exons_hit, S.exons_hit.data(), (size_t)n_tx * 4);
    if (ex_covered) memcpy(ex_covered, S.ex_covered.data(), (size_t)n_exon * 8);
    if (ex_sum) memcpy(ex_sum, S.ex_sum.data(), (size_t)n_exon * 8);
    if (ex_max) memcpy(ex_max, S.ex_max.data(), (size_t)n_exon * 8);
  }
  if (want_junc) {
    memcpy(introns_hit, S.introns_hit.data(), (size_t)n_tx * 4), memcpy(junc_min, S.junc_min.data(), (size_t)n_tx * 8), memcpy(junc_sum, S.junc_sum.data(), (size_t)n_tx * 8);
    if (in_junc) memcpy(in_junc, S.in_junc.data(), (size_t)n_exon * 8);
  }
  return 0;
}

int tbh_split_strand_host(uint32_t n, uint32_t n_cigar_ops, const int32_t* tid, const int32_t* pos, const uint16_t* flag, const uint32_t* cig_off,
                          const uint32_t* cig, const double* yc, const uint8_t* strand, const int64_t* yx, uint32_t* n_rec, uint32_t* n_cig, int32_t* o_tid,
                          int32_t* o_pos, uint32_t* o_cig_off, uint32_t* o_cig, double* o_yc, uint8_t* o_strand, int64_t* o_yx) {
  if (!strand || !n_rec || !n_cig || !o_cig_off || (n && (!tid || !pos || !cig_off || !o_tid || !o_pos || !o_strand)) || (n_cigar_ops && (!cig || !o_cig)) ||
      (n && yc && !o_yc) || (n && yx && !o_yx))
    return fail("tbh_split_strand_host: null argument");
  tbk_cov_in in;
  memset(&in, 0, sizeof(in));
  in.mem = TBK_MEM_HOST, in.n_records = n, in.n_cigar_ops = n_cigar_ops;
  in.tid = tid, in.pos = pos, in.flag = flag, in.cig_off = cig_off, in.cig = cig, in.yc = yc, in.strand = strand, in.yx = yx;
  tbh::CovRecs out[3];
  tbh::split_strand_host(in, out);
  size_t r = 0, w = 0;
  for (int s = 0; s < 3; ++s) {
    const tbh::CovRecs& o = out[s];
    const size_t m = o.tid.size(), c = o.cig.size();
    n_rec[s] = (uint32_t)m, n_cig[s] = (uint32_t)c;
    if (m) {
      memcpy(o_tid + r, o.tid.data(), m * 4), memcpy(o_pos + r, o.pos.data(), m * 4), memcpy(o_strand + r, o.strand.data(), m);
      if (yc) memcpy(o_yc + r, o.yc.data(), m * 8);
      if (yx) memcpy(o_yx + r, o.yx.data(), m * 8);
    }
    memcpy(o_cig_off + r + s, o.cig_off.data(), (m + 1) * 4);
    if (c) memcpy(o_cig + w, o.cig.data(), c * 4);
    r += m, w += c;
  }
  return 0;
}

}  // extern "C"
