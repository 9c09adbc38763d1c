// tbh_tool — small test driver for the host-side codec and API mirror (used by tests/, CPU only):
//   cat IN.bam OUT.bam            decode with GSamReader, re-encode with GSamWriter
//   mergeorder IN1.bam IN2.bam..  print "fidx idx" of every record in TInputFiles::next() order
//   soa OUTDIR IN1.bam ...        dump the SoA tile arrays (one raw little-endian file per array)
//   tags IN.bam OUT.bam SPEC...   apply tag edits to every record: YC=f:2.5  YX=i:255  YD=i:0  YD=del
//   bai IN.bam                    write IN.bam.bai with the host index builder alone (bai.h: what `tiebrush --index` builds as it writes)
//   csi IN.bam                    write IN.bam.csi the same way (what `tiebrush --csi` builds: references beyond 2^29 included)
//   tabix IN.bam IN.bed OUT.gz    a bedGraph / BED track (a first line that begins with "track" is its header) as BGZF OUT.gz with its
//                                 tabix index OUT.gz.tbi / .csi by the host path alone (tabix.h: what `tiecov --tabix` writes; IN.bam
//                                 gives the reference names and lengths); rows out of order are refused with their line number
//   query IN.bam REGION [INDEX]   the chunks the index names for REGION (bai_read.h), one line "vbeg vend" in hex each, then the number of
//                                 records in the chunks and of those overlapping the region, by the host codec ("hit vbeg" per overlap)
//   rquery IN.bam REGIONS.bed [INDEX]   the same for the region table of a BED file: "regions R", a "region tid beg end"
//                                 line per interval of the normalised table, the chunks merged over the whole table, records, hits
//   mquery REGION THREADS IN1.bam ... / mrquery REGIONS.bed THREADS IN1.bam ...   the host plumbing of `tiebrush -r` / `-R`, per input
//   summary IN.bam COV.bedgraph JUNC.bed FEATURES.bed OUT.tsv   the per-feature summary of `tiecov --features --summary` from our own
//                                 plain tracks, by the host summariser alone ("-" for a track that is not there)
//   depth IN.bam COV.bedgraph THRESHOLDS OUT.tsv [FEATURES.bed]   the bases-at-depth table of `tiecov --thresholds --depth-summary` (per
//                                 reference; with FEATURES.bed the per-feature table of `--feature-depth`) from our own plain coverage
//                                 track, by the host loops alone (THRESHOLDS "-": no ge_ columns, per reference only)
//   batches IN.bam BYTES          the batches of whole BGZF members a streamed decode reads (stream_read.h): per batch its
//                                 member range, first_uoff, the range of whole records in it and the tail, both by the host codec
//   mkbam SOADIR PREFIX [LEVEL [THREADS]]   encode the raw SoA arrays of a synthetic tile (file_off, tid, pos, flag, mapq, strand,
//                                 nh, cig_off, cig as little-endian files + header.txt) as PREFIX<f>.bam, one per input file: the
//                                 records tiebrush_amd.synth.write_bams writes (SEQ '*', QNAME r<f>_<i>, NH:C / XS:A), files in parallel
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "GSam.h"
#include "bai.h"
#include "bai_read.h"
#include "bgzf.h"
#include "fastload.h"
#include "tmerge.h"
#include "bigwig.h"
#include "stream_read.h"
#include "tabix.h"
#include "tracks.h"

template <class T>
static bool slurp(const std::string& dir, const char* name, std::vector<T>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)sz / sizeof(T));
  const bool ok = v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
  fclose(f);
  return ok;
}
// UCSC binning scheme (SAM spec 5.3), as htslib's hts_reg2bin(beg, end, 14, 5)
static uint16_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint16_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint16_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint16_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint16_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint16_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
template <class T>
static void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  if (!f) GError("cannot write %s/%s\n", dir.c_str(), name);
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
  fclose(f);
}

// does the record overlap any interval of the table (brute force: the check is not the code under test)
static bool overlaps_any(const tbh::RegionTable& U, const tbh::BaiRec& r) {
  for (size_t q = 0; q < U.n(); ++q)
    if (r.tid == U.tid[q] && r.beg < U.end[q] && r.end > U.beg[q]) return true;
  return false;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::string cmd = argv[1];
  if (cmd == "cat" && argc == 4) {
    GSamReader rd(argv[2]);
    GSamWriter wr(argv[3], rd.header());
    GSamRecord r;
    while (rd.next(r)) wr.write(&r);
    return 0;
  }
  if (cmd == "mergeorder" && argc >= 3) {
    TInputFiles in;
    in.setup("test", 0, nullptr);
    for (int i = 2; i < argc; ++i) in.addFile(argv[i]);
    int k = in.start();
    std::vector<uint32_t> idx(k, 0);
    while (TInputRecord* r = in.next()) printf("%d %u\n", r->fidx, idx[r->fidx]++);
    return 0;
  }
  if (cmd == "soa" && argc >= 4) {
    TInputFiles in;
    in.setup("test", 0, nullptr);
    for (int i = 3; i < argc; ++i) in.addFile(argv[i]);
    in.start();
    TbkTile t;
    in.load_tile(t, true, true, 4);
    std::string d = argv[2];
    dump(d, "file_off", t.file_off);
    dump(d, "tbmerged", t.tbmerged);
    dump(d, "tid", t.tid);
    dump(d, "pos", t.pos);
    dump(d, "flag", t.flag);
    dump(d, "mapq", t.mapq);
    dump(d, "strand", t.strand);
    dump(d, "nh", t.nh);
    dump(d, "cig_off", t.cig_off);
    dump(d, "cig", t.cig);
    dump(d, "yc_in", t.yc_in);
    dump(d, "yx_in", t.yx_in);
    dump(d, "yd_in", t.yd_in);
    dump(d, "md_off", t.md_off);
    dump(d, "md", t.md);
    dump(d, "md_has", t.md_has);
    dump(d, "qname_hash", t.qname_hash);
    dump(d, "qname_off", t.qname_off);
    dump(d, "qname", t.qname);
    FILE* f = fopen((d + "/header.txt").c_str(), "w");
    fputs(in.header()->text.c_str(), f);
    fclose(f);
    return 0;
  }
  if (cmd == "fastsoa" && argc >= 4) {  // fastsoa OUTDIR IN1.bam ...: the tile of the whole-input loader (fastload.cpp), as `soa` dumps it
    std::vector<std::string> paths;
    std::vector<uint8_t> tb;
    for (int i = 3; i < argc; ++i) {
      paths.push_back(argv[i]);
      GSamReader rd(argv[i]);
      tb.push_back(rd.header()->is_tiebrush() ? 1 : 0);
    }
    tbh::FastTile t;
    bool fits = false;
    std::string err;
    if (!tbh::fast_load(paths, tb, argc > 3 ? 3 : 1, (size_t)1 << 40, t, &fits, err) || !fits) {
      fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    fprintf(stderr, "fastsoa: %zu of %zu inputs indexed by their members' own walks; ms read %.1f inflate %.1f index %.1f SoA %.1f\n", t.n_fused, t.in.size(), t.ms_read,
            t.ms_inflate, t.ms_index, t.ms_soa);
    const std::string d = argv[2];
    auto dumpp = [&](const char* name, const void* p, size_t bytes) {
      FILE* f = fopen((d + "/" + name).c_str(), "wb");
      if (!f) GError("cannot write %s/%s\n", d.c_str(), name);
      if (bytes) fwrite(p, 1, bytes, f);
      fclose(f);
    };
    dump(d, "file_off", t.file_off);
    dump(d, "tbmerged", t.tbmerged);
    dumpp("tid", t.tid, t.n * 4);
    dumpp("pos", t.pos, t.n * 4);
    dumpp("flag", t.flag, t.n * 2);
    dumpp("mapq", t.mapq, t.n);
    dumpp("strand", t.strand, t.n);
    dumpp("nh", t.nh, t.n * 4);
    dumpp("cig_off", t.cig_off, (t.n + 1) * 4);
    dumpp("cig", t.cig, t.n_cig * 4);
    dumpp("yc_in", t.yc_in, t.yc_in ? t.n * 8 : 0);
    dumpp("yx_in", t.yx_in, t.yx_in ? t.n * 8 : 0);
    dumpp("yd_in", t.yd_in, t.yd_in ? t.n * 8 : 0);
    // the raw records behind a few tile indices: first, last, and one from the middle of every file
    std::vector<uint8_t> recs;
    for (size_t f = 0; f + 1 < t.file_off.size(); ++f)
      for (uint32_t g : {t.file_off[f], (t.file_off[f] + t.file_off[f + 1]) / 2, t.file_off[f + 1] - 1}) {
        if (t.file_off[f] == t.file_off[f + 1]) continue;
        uint32_t len;
        const uint8_t* p = t.record(g, &len);
        recs.insert(recs.end(), (const uint8_t*)&g, (const uint8_t*)&g + 4);
        recs.insert(recs.end(), (const uint8_t*)&len, (const uint8_t*)&len + 4);
        recs.insert(recs.end(), p, p + len);
      }
    dump(d, "probe_records", recs);
    return 0;
  }
  if (cmd == "mkbam" && argc >= 4) {
    const std::string d = argv[2], prefix = argv[3];
    const int level = argc > 4 ? atoi(argv[4]) : 1;
    int threads = argc > 5 && atoi(argv[5]) > 0 ? atoi(argv[5]) : tbh::cpu_budget();
    // "seq": every record carries SEQ / QUAL of its query length and the aux tags of an aligner's output, about 250 bytes per
    // 100-bp read like the reference's fixtures (test/t1/t1s0.bam) — what BGZF inflate / deflate and the tagging really move
    const bool with_seq = argc > 6 && strcmp(argv[6], "seq") == 0;
    std::vector<uint32_t> file_off, cig_off, cig;
    std::vector<int32_t> tid, pos, nh;
    std::vector<uint16_t> flag;
    std::vector<uint8_t> mapq, strand;
    if (!slurp(d, "file_off", file_off) || !slurp(d, "tid", tid) || !slurp(d, "pos", pos) || !slurp(d, "flag", flag) || !slurp(d, "mapq", mapq) ||
        !slurp(d, "strand", strand) || !slurp(d, "nh", nh) || !slurp(d, "cig_off", cig_off) || !slurp(d, "cig", cig) || file_off.size() < 2)
      GError("mkbam: cannot read the SoA arrays in %s\n", d.c_str());
    std::string text;
    {
      FILE* f = fopen((d + "/header.txt").c_str(), "r");
      if (!f) GError("mkbam: no header.txt in %s\n", d.c_str());
      char buf[4096];
      size_t r;
      while ((r = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, r);
      fclose(f);
    }
    tbh::BamHeader hdr;
    hdr.text = text;
    for (const std::string& l : hdr.lines()) {
      if (l.compare(0, 3, "@SQ") != 0) continue;
      const size_t a = l.find("SN:"), b = l.find("LN:");
      if (a == std::string::npos || b == std::string::npos) continue;
      hdr.target_name.push_back(l.substr(a + 3, l.find('\t', a) - a - 3));
      hdr.target_len.push_back((uint32_t)atoll(l.c_str() + b + 3));
    }
    hdr.n_targets = (int32_t)hdr.target_name.size();
    const uint32_t k = (uint32_t)file_off.size() - 1;
    if (threads < 1) threads = 1;
    if ((uint32_t)threads > k) threads = (int)k;
    std::atomic<uint32_t> next{0};
    std::atomic<int> failed{0};
    auto work = [&]() {
      std::vector<uint8_t> buf;
      for (;;) {
        const uint32_t f = next.fetch_add(1);
        if (f >= k) return;
        tbh::BgzfWriter w;
        if (!w.open(prefix + std::to_string(f) + ".bam", level, 1)) {
          failed = 1;
          return;
        }
        // blocks as htslib cuts them: the header in blocks of its own (bam_hdr_write ends with a flush), and a new block whenever
        // the next record does not fit into the current one (bgzf_flush_try in bam_write1) — every block begins with a record
        std::vector<uint8_t> z;
        auto flush_block = [&]() {
          if (buf.empty()) return;
          z.clear();
          if (!tbh::bgzf_deflate_members(buf.data(), buf.size(), level, z) || !w.write_members(z.data(), z.size())) failed = 1;
          buf.clear();
        };
        buf.clear();
        hdr.serialize(buf);
        flush_block();
        for (uint32_t i = file_off[f]; i < file_off[f + 1]; ++i) {
          char nm[40];
          const int nl = snprintf(nm, sizeof(nm), "r%u_%u", f, i - file_off[f]) + 1;
          const uint32_t c0 = cig_off[i], nc = cig_off[i + 1] - c0;
          int64_t rl = 0, ql = 0;
          for (uint32_t q = 0; q < nc; ++q) {
            const uint32_t op = cig[c0 + q] & 0xF;
            if ((0x18Du >> op) & 1u) rl += cig[c0 + q] >> 4;
            if ((0x193u >> op) & 1u) ql += cig[c0 + q] >> 4;  // M I S = X consume the query
          }
          const bool has_nh = nh[i] != INT32_MIN, has_xs = strand[i] == '+' || strand[i] == '-';
          const uint32_t lseq = with_seq ? (uint32_t)ql : 0u;
          // AS XN XM XO XG NM as C-typed zeros, MD:Z:<ql>, YT:Z:UU — the tag set of the fixtures' aligner
          char md[16];
          const int mdl = with_seq ? snprintf(md, sizeof(md), "%lld", (long long)ql) + 1 : 0;
          const uint32_t extra = with_seq ? 6u * 4u + 3u + (uint32_t)mdl + 6u : 0u;
          const uint32_t body = 32 + (uint32_t)nl + 4 * nc + (lseq + 1) / 2 + lseq + extra + (has_nh ? 4u : 0u) + (has_xs ? 4u : 0u);
          if (buf.size() + 4 + (size_t)body > 0xff00) flush_block();
          const size_t o = buf.size();
          buf.resize(o + 4 + body);
          uint8_t* p = buf.data() + o;
          auto w32 = [&](size_t at, uint32_t v) { memcpy(p + at, &v, 4); };
          auto w16 = [&](size_t at, uint16_t v) { memcpy(p + at, &v, 2); };
          w32(0, body);
          w32(4, (uint32_t)tid[i]);
          w32(8, (uint32_t)pos[i]);
          p[12] = (uint8_t)nl;
          p[13] = mapq[i];
          w16(14, pos[i] >= 0 ? reg2bin(pos[i], pos[i] + (rl > 1 ? rl : 1)) : (uint16_t)4680);
          w16(16, (uint16_t)nc);
          w16(18, flag[i]);
          w32(20, lseq);                // l_seq
          w32(24, 0xFFFFFFFFu);         // next refID
          w32(28, 0xFFFFFFFFu);         // next pos
          w32(32, 0);                   // tlen
          memcpy(p + 36, nm, (size_t)nl);
          memcpy(p + 36 + nl, cig.data() + c0, 4 * (size_t)nc);
          uint8_t* a = p + 36 + nl + 4 * nc;
          if (with_seq) {
            uint64_t x = ((uint64_t)f << 40) ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull) ^ 0xD1B54A32D192ED03ull;  // (deterministic per record)
            auto rnd = [&]() {
              x ^= x << 13, x ^= x >> 7, x ^= x << 17;
              return x;
            };
            static const uint8_t nt[4] = {1, 2, 4, 8};  // A C G T
            for (uint32_t b = 0; b < (lseq + 1) / 2; ++b) {
              const uint64_t r = rnd();
              a[b] = (uint8_t)((nt[r & 3] << 4) | ((2 * b + 1 < lseq) ? nt[(r >> 2) & 3] : 0));
            }
            a += (lseq + 1) / 2;
            for (uint32_t b = 0; b < lseq; ++b) {  // Phred 40 with a dip every so often (a quality string deflates well, not to nothing)
              const uint64_t r = rnd();
              a[b] = (r & 15) == 0 ? (uint8_t)(20 + ((r >> 4) & 15)) : (uint8_t)40;
            }
            a += lseq;
            static const char* zt[6] = {"AS", "XN", "XM", "XO", "XG", "NM"};
            for (int z = 0; z < 6; ++z) {
              a[0] = (uint8_t)zt[z][0], a[1] = (uint8_t)zt[z][1], a[2] = 'C', a[3] = 0;
              a += 4;
            }
            a[0] = 'M', a[1] = 'D', a[2] = 'Z';
            memcpy(a + 3, md, (size_t)mdl);
            a += 3 + mdl;
            memcpy(a, "YTZUU", 6);
            a += 6;
          }
          if (has_nh) {
            a[0] = 'N', a[1] = 'H', a[2] = 'C', a[3] = (uint8_t)nh[i];
            a += 4;
          }
          if (has_xs) a[0] = 'X', a[1] = 'S', a[2] = 'A', a[3] = strand[i];
        }
        flush_block();
        if (!w.close()) failed = 1;
      }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t) th.emplace_back(work);
    for (auto& t : th) t.join();
    return failed ? 1 : 0;
  }
  if (cmd == "tiles" && argc >= 4) {  // tiles <target records> files...: one line per streamed tile = records taken from every input
    TInputFiles in;
    in.setup("test", 0, nullptr);
    for (int i = 3; i < argc; ++i) in.addFile(argv[i]);
    in.start();
    TInputFiles::TilePlan plan;
    while (in.next_tile(plan, (size_t)atoll(argv[2]), 4)) {
      size_t win = 0;
      for (auto fr : in.freaders) win += fr->samreader->file()->n();
      printf("%zu", win);  // records resident in the windows when the tile was cut
      for (size_t f = 0; f < plan.hi.size(); ++f) printf(" %zu", plan.hi[f]);
      printf("\n");
      in.release_tile(plan);
    }
    return 0;
  }
  if (cmd == "tags" && argc >= 5) {
    GSamReader rd(argv[2]);
    GSamWriter wr(argv[3], rd.header());
    GSamRecord r;
    while (rd.next(r)) {
      for (int i = 4; i < argc; ++i) {
        std::string s = argv[i];
        char tag[2] = {s[0], s[1]};
        std::string v = s.substr(3);
        if (v == "del")
          r.remove_tag(tag);
        else if (v[0] == 'f')
          r.add_double_tag(tag, atof(v.c_str() + 2));
        else
          r.add_int_tag(tag, atoll(v.c_str() + 2));
      }
      wr.write(&r);
    }
    return 0;
  }
  if (cmd == "bedgraph2bw" && argc == 5) {  // <alignment file: the chromosome list> <in.bedgraph> <out.bigwig>
    GSamReader rd(argv[2]);
    sam_hdr_t* hdr = rd.header();
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    for (int t = 0; t < hdr->n_targets; ++t) {
      names.push_back(hdr->target_name[t]);
      lens.push_back(hdr->target_len[t]);
    }
    tbh::BigWigWriter bw;
    std::string err;
    if (!bw.open(argv[4], names, lens, err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    FILE* f = fopen(argv[3], "r");
    if (!f) return 1;
    char line[4096], chrom[2048];
    while (fgets(line, sizeof(line), f)) {
      unsigned long a, b;
      double v;
      if (sscanf(line, "%2047s %lu %lu %lf", chrom, &a, &b, &v) != 4) continue;  // (track line)
      int tid = hdr->name2tid(chrom);
      if (tid < 0) return 1;
      bw.add((uint32_t)tid, (uint32_t)a, (uint32_t)b, (float)v);
    }
    fclose(f);
    if (!bw.close(err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  if (cmd == "tabix" && argc == 5) {  // <alignment file: names and lengths> <in.bedgraph|in.bed> <out.gz>
    GSamReader rd(argv[2]);
    sam_hdr_t* hdr = rd.header();
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    for (int t = 0; t < hdr->n_targets; ++t) {
      names.push_back(hdr->target_name[t]);
      lens.push_back(hdr->target_len[t]);
    }
    FILE* f = fopen(argv[3], "r");
    if (!f) {
      fprintf(stderr, "tbh_tool tabix: cannot open %s\n", argv[3]);
      return 1;
    }
    std::string text, head, err;
    {
      char buf[1 << 16];
      size_t got;
      while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
      fclose(f);
    }
    size_t p = 0;
    if (text.compare(0, 5, "track") == 0) {
      p = text.find('\n');
      p = p == std::string::npos ? text.size() : p + 1;
      head = text.substr(0, p);
    }
    tbh::TabixWriter w;
    if (!w.open(argv[4], names, lens, head, err)) {
      fprintf(stderr, "tbh_tool tabix: %s\n", err.c_str());
      return 1;
    }
    // slices of whole lines as the command lines' host path cuts them; the header rides with the first
    const size_t slice_rows = (size_t)1 << 19;
    std::vector<tbh::BaiRec> recs;
    size_t s0 = 0, line = head.empty() ? 0 : 1;
    int32_t last_tid = -1, last_beg = 0;
    auto flush = [&](size_t upto) {
      if (upto == s0) return true;
      for (tbh::BaiRec& r : recs) r.vbeg -= s0;
      const bool ok = w.add_text(text.data() + s0, upto - s0, recs, err);
      recs.clear(), s0 = upto;
      return ok;
    };
    bool ok = true;
    while (ok && p < text.size()) {
      size_t e = text.find('\n', p);
      e = e == std::string::npos ? text.size() : e + 1;
      ++line;
      const size_t t1 = text.find('\t', p);
      char* q = nullptr;
      long long a = 0, b = 0;
      bool good = t1 != std::string::npos && t1 < e;
      if (good) {
        a = strtoll(text.c_str() + t1 + 1, &q, 10);
        good = q != text.c_str() + t1 + 1 && *q == '\t';
      }
      if (good) {
        const char* q0 = q + 1;
        b = strtoll(q0, &q, 10);
        good = q != q0;
      }
      const int tid = good ? hdr->name2tid(text.substr(p, t1 - p).c_str()) : -1;
      if (!good || tid < 0 || a < 0 || a > INT32_MAX) {
        fprintf(stderr, "tbh_tool tabix: %s line %zu: not a row of a reference in %s\n", argv[3], line, argv[2]);
        w.discard();
        return 1;
      }
      if (tid < last_tid || (tid == last_tid && (int32_t)a < last_beg)) {
        fprintf(stderr, "tbh_tool tabix: %s line %zu is out of order (the rows must be sorted by reference, then start)\n", argv[3], line);
        w.discard();
        return 1;
      }
      last_tid = tid, last_beg = (int32_t)a;
      recs.push_back(tbh::BaiRec{tid, (int32_t)a, std::max<int64_t>(b, a + 1), (uint64_t)p});
      p = e;
      if (recs.size() == slice_rows) ok = flush(p);
    }
    ok = ok && flush(text.size());
    if (!ok || !w.close(err)) {
      fprintf(stderr, "tbh_tool tabix: %s\n", err.c_str());
      w.discard();
      return 1;
    }
    return 0;
  }
  if (cmd == "bai" && argc == 3) {
    std::string err;
    if (!tbh::bai_index_file(argv[2], std::string(argv[2]) + ".bai", err)) {
      fprintf(stderr, "tbh_tool bai: %s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  if (cmd == "csi" && argc == 3) {
    std::string err;
    if (!tbh::bai_index_file(argv[2], std::string(argv[2]) + ".csi", err, true)) {
      fprintf(stderr, "tbh_tool csi: %s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  // query: one REGION; rquery FILE.bam REGIONS.bed [INDEX]: the normalised table of a BED file, "regions R" first
  if ((cmd == "query" || cmd == "rquery") && (argc == 4 || argc == 5)) {
    const bool bed = cmd == "rquery";
    const std::string me = "tbh_tool " + cmd;
    std::string err;
    tbh::BamFile bf;
    tbh::RegionTable U;
    std::vector<tbh::IdxChunk> chunks;
    std::vector<tbh::RegionSpan> spans;
    bool ok = bf.open(argv[2], err, 1);
    if (ok && bed) {
      ok = tbh::regions_from_bed_file(bf.hdr, argv[3], U, err);
    } else if (ok) {
      int32_t tid = 0;
      int64_t beg = 0, end = 0;
      ok = tbh::parse_region(bf.hdr, argv[3], &tid, &beg, &end, err);
      U.add(tid, beg, end);
    }
    if (!ok || (U.beg[0] < U.end[0] && !tbh::index_query_regions_file(argv[2], argc == 5 ? argv[4] : "", U, chunks, err)) ||
        !tbh::read_spans(argv[2], chunks, spans, nullptr, err)) {
      fprintf(stderr, "%s: %s\n", me.c_str(), err.c_str());
      return 1;
    }
    if (bed) printf("regions %zu\n", U.n());
    for (size_t r = 0; r < U.n(); ++r) printf("region %d %lld %lld\n", U.tid[r], (long long)U.beg[r], (long long)U.end[r]);
    uint64_t n_rec = 0, n_hit = 0;
    std::vector<uint64_t> hits;
    for (size_t c = 0; c < chunks.size(); ++c) {
      printf("%llx %llx\n", (unsigned long long)chunks[c].beg, (unsigned long long)chunks[c].end);
      std::vector<tbh::BaiRec> recs;
      if (!tbh::span_records(spans[c], chunks[c].beg >> 16, recs, err)) {
        fprintf(stderr, "%s: %s\n", me.c_str(), err.c_str());
        return 1;
      }
      n_rec += recs.size();
      for (const tbh::BaiRec& r : recs)
        if (overlaps_any(U, r)) hits.push_back(r.vbeg);
    }
    n_hit = hits.size();
    printf("records %llu\noverlapping %llu\n", (unsigned long long)n_rec, (unsigned long long)n_hit);
    for (uint64_t v : hits) printf("hit %llx\n", (unsigned long long)v);
    return 0;
  }
  // the host plumbing of `tiebrush -r`: REGION against the first input's header, every input's index found, checked and
  // queried (region_input_chunks), the chunks of all inputs read on THREADS threads (read_spans_many), the records counted by the host codec
  // mrquery REGIONS.bed THREADS IN1.bam ...: the same for the table of a BED file (`tiebrush -R`), "regions R" first
  if ((cmd == "mquery" || cmd == "mrquery") && argc >= 5) {
    const bool bed = cmd == "mrquery";
    const std::string me = "tbh_tool " + cmd;
    std::string err;
    const int threads = atoi(argv[3]);
    std::vector<std::string> paths(argv + 4, argv + argc);
    tbh::RegionTable U;
    std::vector<std::vector<tbh::IdxChunk>> chunks(paths.size());
    std::vector<std::vector<tbh::RegionSpan>> spans;
    uint64_t bytes = 0;
    for (size_t f = 0; f < paths.size(); ++f) {
      tbh::BamFile bf;
      std::string ix;
      bool ok = bf.open(paths[f], err, 1);
      if (ok && f == 0 && bed) {
        ok = tbh::regions_from_bed_file(bf.hdr, argv[2], U, err);
      } else if (ok && f == 0) {
        int32_t tid = 0;
        int64_t beg = 0, end = 0;
        ok = tbh::parse_region(bf.hdr, argv[2], &tid, &beg, &end, err);
        U.add(tid, beg, end);
      }
      if (!ok || !tbh::regions_input_chunks(paths[f], bf.hdr.n_targets, U, chunks[f], ix, err)) {
        fprintf(stderr, "%s: %s\n", me.c_str(), err.c_str());
        return 1;
      }
    }
    if (!tbh::read_spans_many(paths, chunks, threads, spans, &bytes, err)) {
      fprintf(stderr, "%s: %s\n", me.c_str(), err.c_str());
      return 1;
    }
    if (bed) printf("regions %zu\n", U.n());
    for (size_t r = 0; r < U.n(); ++r) printf("region %d %lld %lld\n", U.tid[r], (long long)U.beg[r], (long long)U.end[r]);
    printf("bytes %llu\n", (unsigned long long)bytes);
    for (size_t f = 0; f < paths.size(); ++f) {
      uint64_t n_rec = 0, n_hit = 0;
      for (size_t c = 0; c < chunks[f].size(); ++c) {
        std::vector<tbh::BaiRec> recs;
        if (!tbh::span_records(spans[f][c], chunks[f][c].beg >> 16, recs, err)) {
          fprintf(stderr, "%s: %s: %s\n", me.c_str(), paths[f].c_str(), err.c_str());
          return 1;
        }
        n_rec += recs.size();
        for (const tbh::BaiRec& r : recs) n_hit += overlaps_any(U, r);
      }
      printf("file %zu chunks %zu records %llu overlapping %llu\n", f, chunks[f].size(), (unsigned long long)n_rec, (unsigned long long)n_hit);
    }
    return 0;
  }
  // the host-only form of `tiecov --features FEATURES.bed --summary OUT.tsv`: our own plain tracks read back (a first line
  // that begins with "track" is the header; "-" in the place of a track: that part of the summary stays zero), the host summariser, the
  // TSV writer.  The tracks' values are what "%.3f" printed.
  if (cmd == "summary" && argc == 7) {
    std::string err;
    tbh::BamFile bf;
    tbh::FeatureTable F;
    if (!bf.open(argv[2], err, 1) || !tbh::features_from_bed_file(bf.hdr, argv[5], F, err)) {
      fprintf(stderr, "tbh_tool summary: %s\n", err.c_str());
      return 1;
    }
    std::vector<int32_t> tid[2], start[2], end[2];
    std::vector<double> val[2];
    std::vector<uint8_t> jstrand;
    bool have[2] = {false, false};
    for (int k = 0; k < 2; ++k) {
      const std::string path = argv[3 + k];
      if (path == "-") continue;
      have[k] = true;
      FILE* f = fopen(path.c_str(), "r");
      if (!f) {
        fprintf(stderr, "tbh_tool summary: cannot read %s\n", path.c_str());
        return 1;
      }
      char line[4096], name[2048], jname[64], strand = '.';
      for (size_t lineno = 1; fgets(line, sizeof(line), f); ++lineno) {
        if (lineno == 1 && strncmp(line, "track", 5) == 0) continue;
        long long s = 0, e = 0;
        double v = 0;
        const bool ok = k == 0 ? sscanf(line, "%2047s %lld %lld %lf", name, &s, &e, &v) == 4
                               : sscanf(line, "%2047s %lld %lld %63s %lf %c", name, &s, &e, jname, &v, &strand) == 6;
        const int t = ok ? bf.hdr.name2tid(name) : -1;
        if (t < 0) {
          fprintf(stderr, "tbh_tool summary: %s line %zu: not a row of the track\n", path.c_str(), lineno);
          fclose(f);
          return 1;
        }
        tid[k].push_back(t), start[k].push_back((int32_t)s), end[k].push_back((int32_t)e), val[k].push_back(v);
        if (k == 1) jstrand.push_back((uint8_t)strand);
      }
      fclose(f);
    }
    tbh::FeatSummary S;
    tbh::summarise_features(F, have[0], (uint32_t)tid[0].size(), tid[0].data(), start[0].data(), end[0].data(), val[0].data(), have[1], (uint32_t)tid[1].size(),
                            tid[1].data(), start[1].data(), end[1].data(), jstrand.data(), val[1].data(), S);
    if (!tbh::write_summary_tsv(argv[6], bf.hdr.target_name, F, S, err)) {
      fprintf(stderr, "tbh_tool summary: %s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  // the host-only form of `tiecov --thresholds THRESHOLDS --depth-summary OUT.tsv` and, with a BED file, of `--features FEATURES.bed
  // --feature-depth OUT.tsv`: our own plain coverage track read back, the host loops, the table writers
  if (cmd == "depth" && (argc == 6 || argc == 7)) {
    std::string err;
    tbh::BamFile bf;
    if (!bf.open(argv[2], err, 1)) {
      fprintf(stderr, "tbh_tool depth: %s\n", err.c_str());
      return 1;
    }
    const bool per_feature = argc == 7;
    std::vector<double> thr;
    std::vector<std::string> thr_text;
    if (strcmp(argv[4], "-") != 0 || per_feature) {
      if (!tbh::parse_thresholds(argv[4], thr, thr_text, err)) {
        fprintf(stderr, "tbh_tool depth: --thresholds: %s\n", err.c_str());
        return 1;
      }
    }
    tbh::FeatureTable F;
    if (per_feature && !tbh::features_from_bed_file(bf.hdr, argv[6], F, err)) {
      fprintf(stderr, "tbh_tool depth: %s\n", err.c_str());
      return 1;
    }
    std::vector<int32_t> tid, start, end;
    std::vector<double> val;
    {
      FILE* f = fopen(argv[3], "r");
      if (!f) {
        fprintf(stderr, "tbh_tool depth: cannot read %s\n", argv[3]);
        return 1;
      }
      char line[4096], name[2048];
      for (size_t lineno = 1; fgets(line, sizeof(line), f); ++lineno) {
        if (lineno == 1 && strncmp(line, "track", 5) == 0) continue;
        long long s = 0, e = 0;
        double v = 0;
        const int t = sscanf(line, "%2047s %lld %lld %lf", name, &s, &e, &v) == 4 ? bf.hdr.name2tid(name) : -1;
        if (t < 0) {
          fprintf(stderr, "tbh_tool depth: %s line %zu: not a row of the track\n", argv[3], lineno);
          fclose(f);
          return 1;
        }
        tid.push_back(t), start.push_back((int32_t)s), end.push_back((int32_t)e), val.push_back(v);
      }
      fclose(f);
    }
    const uint32_t ni = (uint32_t)tid.size(), nt = (uint32_t)thr.size();
    const std::vector<std::string>& names = bf.hdr.target_name;
    bool ok;
    if (per_feature) {
      std::vector<uint64_t> covered(F.n()), ge(F.n() * nt);
      tbh::threshold_features(F.n(), F.tid.data(), F.beg.data(), F.end.data(), ni, tid.data(), start.data(), end.data(), val.data(), thr.data(), nt, covered.data(), ge.data());
      ok = tbh::write_feature_depth_tsv(argv[5], names, F, thr_text, covered.data(), ge.data(), err);
    } else {
      const std::vector<uint32_t>& lens = bf.hdr.target_len;
      tbh::FeatureTable R;  // [0, LN) of every reference with a base
      for (size_t r = 0; r < lens.size(); ++r)
        if (lens[r]) R.tid.push_back((int32_t)r), R.beg.push_back(0), R.end.push_back((int64_t)lens[r]), R.strand.push_back((uint8_t)'.');
      tbh::DepthTable D;
      D.resize(lens.size(), nt);
      if (R.n()) {
        tbh::FeatSummary S;
        tbh::summarise_features(R, true, ni, tid.data(), start.data(), end.data(), val.data(), false, 0, nullptr, nullptr, nullptr, nullptr, nullptr, S);
        std::vector<uint64_t> ge(R.n() * nt + 1);
        if (nt) tbh::threshold_features(R.n(), R.tid.data(), R.beg.data(), R.end.data(), ni, tid.data(), start.data(), end.data(), val.data(), thr.data(), nt, nullptr, ge.data());
        for (size_t i = 0; i < R.n(); ++i) {
          const size_t r = (size_t)R.tid[i];
          D.covered[r] = S.covered[i], D.sum[r] = S.sum[i], D.max[r] = S.max[i];
          for (uint32_t k = 0; k < nt; ++k) D.ge[r * nt + k] = ge[i * nt + k];
        }
      }
      ok = tbh::write_depth_tsv(argv[5], names, lens, thr_text, D, err);
    }
    if (!ok) {
      fprintf(stderr, "tbh_tool depth: %s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  // the host-only form of `tiecov --gtf ANNOT.gtf --transcripts OUT.tsv`: transcripts IN.bam COV.bedgraph JUNC.bed
  // ANNOT.gtf OUT.tsv — our own plain tracks read back as `summary` reads them, the host summariser, the TSV writer
  if (cmd == "transcripts" && argc == 7) {
    std::string err;
    tbh::BamFile bf;
    tbh::TranscriptTable X;
    if (!bf.open(argv[2], err, 1) || !tbh::transcripts_from_gtf_file(bf.hdr, argv[5], X, err)) {
      fprintf(stderr, "tbh_tool transcripts: %s\n", err.c_str());
      return 1;
    }
    std::vector<int32_t> tid[2], start[2], end[2];
    std::vector<double> val[2];
    std::vector<uint8_t> jstrand;
    bool have[2] = {false, false};
    for (int k = 0; k < 2; ++k) {
      const std::string path = argv[3 + k];
      if (path == "-") continue;
      have[k] = true;
      FILE* f = fopen(path.c_str(), "r");
      if (!f) {
        fprintf(stderr, "tbh_tool transcripts: cannot read %s\n", path.c_str());
        return 1;
      }
      char line[4096], name[2048], jname[64], strand = '.';
      for (size_t lineno = 1; fgets(line, sizeof(line), f); ++lineno) {
        if (lineno == 1 && strncmp(line, "track", 5) == 0) continue;
        long long s = 0, e = 0;
        double v = 0;
        const bool ok = k == 0 ? sscanf(line, "%2047s %lld %lld %lf", name, &s, &e, &v) == 4
                               : sscanf(line, "%2047s %lld %lld %63s %lf %c", name, &s, &e, jname, &v, &strand) == 6;
        const int t = ok ? bf.hdr.name2tid(name) : -1;
        if (t < 0) {
          fprintf(stderr, "tbh_tool transcripts: %s line %zu: not a row of the track\n", path.c_str(), lineno);
          fclose(f);
          return 1;
        }
        tid[k].push_back(t), start[k].push_back((int32_t)s), end[k].push_back((int32_t)e), val[k].push_back(v);
        if (k == 1) jstrand.push_back((uint8_t)strand);
      }
      fclose(f);
    }
    tbh::TxSummary S;
    tbh::summarise_transcripts(X, have[0], (uint32_t)tid[0].size(), tid[0].data(), start[0].data(), end[0].data(), val[0].data(), have[1], (uint32_t)tid[1].size(),
                               tid[1].data(), start[1].data(), end[1].data(), jstrand.data(), val[1].data(), S);
    if (!tbh::write_transcripts_tsv(argv[6], bf.hdr.target_name, X, S, err)) {
      fprintf(stderr, "tbh_tool transcripts: %s\n", err.c_str());
      return 1;
    }
    return 0;
  }
  if (cmd == "batches" && argc == 4) {  // batches FILE.bam BYTES
    tbh::StreamReader rd;
    std::string err;
    if (!rd.open(argv[2], strtoull(argv[3], nullptr, 10), err)) {
      fprintf(stderr, "tbh_tool batches: %s\n", err.c_str());
      return 1;
    }
    printf("header n_targets=%d\n", rd.header().n_targets);
    tbh::StreamBatch b;
    uint64_t rec = 0, k = 0;
    while (rd.next(b, err)) {
      uint64_t n = 0, tail = 0;
      if (!tbh::stream_host_tail(b, &n, &tail, err)) {
        fprintf(stderr, "tbh_tool batches: %s: %s\n", argv[2], err.c_str());
        return 1;
      }
      printf("batch %llu members=%llu..%llu first_uoff=%u records=%llu..%llu tail=%llu last=%d\n", (unsigned long long)k++, (unsigned long long)b.first_member,
             (unsigned long long)(b.first_member + b.csize.size()), b.first_uoff, (unsigned long long)rec, (unsigned long long)(rec + n), (unsigned long long)tail,
             (int)b.last);
      rec += n;
      if (!rd.advance(b, tail, err)) {
        fprintf(stderr, "tbh_tool batches: %s\n", err.c_str());
        return 1;
      }
    }
    if (!err.empty()) {
      fprintf(stderr, "tbh_tool batches: %s\n", err.c_str());
      return 1;
    }
    printf("end records=%llu members=%llu bytes_read=%llu reinflated=%llu\n", (unsigned long long)rec, (unsigned long long)rd.members(),
           (unsigned long long)rd.bytes_read(), (unsigned long long)rd.reinflated());
    return 0;
  }
  fprintf(stderr, "usage: tbh_tool cat|mergeorder|soa|fastsoa|mkbam|tiles|tags|bedgraph2bw|bai|csi|tabix|query|rquery|mquery|mrquery|summary|depth|transcripts|batches ...\n");
  return 2;
}
