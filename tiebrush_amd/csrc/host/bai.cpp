// bai.cpp — see bai.h
#include "bai.h"

#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "bgzf.h"

namespace tbh {

namespace {
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
void put32(std::vector<uint8_t>& o, uint32_t v) {
  for (int q = 0; q < 4; ++q) o.push_back((uint8_t)(v >> (8 * q)));
}
void put64(std::vector<uint8_t>& o, uint64_t v) {
  for (int q = 0; q < 8; ++q) o.push_back((uint8_t)(v >> (8 * q)));
}
// one BGZF member at z[at, zn): its size, where its deflate stream lies, its ISIZE; false when it is not one
bool member_at(const uint8_t* z, size_t zn, size_t at, size_t* size, size_t* cdata, uint32_t* isize) {
  if (at + 18 > zn || z[at] != 31 || z[at + 1] != 139 || z[at + 2] != 8 || !(z[at + 3] & 4)) return false;
  const size_t xlen = (size_t)z[at + 10] | (size_t)z[at + 11] << 8;
  if (at + 12 + xlen > zn) return false;
  size_t bsize = 0;
  for (size_t x = at + 12; x + 4 <= at + 12 + xlen;) {
    const size_t sl = (size_t)z[x + 2] | (size_t)z[x + 3] << 8;
    if (z[x] == 'B' && z[x + 1] == 'C' && sl == 2 && x + 6 <= at + 12 + xlen) bsize = ((size_t)z[x + 4] | (size_t)z[x + 5] << 8) + 1;
    x += 4 + sl;
  }
  if (bsize < 12 + xlen + 8 || at + bsize > zn) return false;
  *size = bsize;
  *cdata = at + 12 + xlen;
  *isize = le32(z + at + bsize - 4);
  return true;
}
}  // namespace

// UCSC binning (SAM specification 5.3; htslib hts_reg2bin(beg, end, 14, depth): 5 for a BAI)
uint32_t bai_reg2bin(int64_t beg, int64_t end, int depth) {
  --end;
  int s = 14;
  int64_t t = ((1ll << (3 * depth)) - 1) / 7;
  for (int l = depth; l > 0; --l) {
    if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    s += 3, t -= 1ll << (3 * (l - 1));
  }
  return 0;
}

int csi_depth(uint64_t max_len) {
  int d = 0;
  while (d < kCsiMaxDepth && max_len + 256 > (1ull << (14 + 3 * d))) ++d;
  return d;
}

bool bai_rec_span(const uint8_t* r, size_t len, int32_t* tid, int32_t* beg, int64_t* end) {
  if (len < 32) return false;
  const uint32_t l_qname = r[8], n_cig = (uint32_t)r[12] | (uint32_t)r[13] << 8;
  if (32ull + l_qname + 4ull * n_cig > len) return false;
  *tid = (int32_t)le32(r);
  *beg = (int32_t)le32(r + 4);
  uint64_t rl = 0;
  for (uint32_t i = 0; i < n_cig; ++i) {
    const uint32_t c = le32(r + 32 + l_qname + 4 * (size_t)i);
    if ((0x18Du >> (c & 15u)) & 1u) rl += c >> 4;  // M D N = X consume the reference
  }
  *end = (int64_t)((uint64_t)(uint32_t)*beg + (rl ? rl : 1));  // (at most 2^32 + 65535 * 2^28)
  return true;
}

bool bai_member_voffsets(const uint8_t* z, size_t zn, std::vector<BaiRec>& recs, std::string& err) {
  size_t at = 0, ri = 0;
  uint64_t pay = 0;  // payload bytes before the member at `at`
  while (at < zn && ri < recs.size()) {
    size_t size, cdata;
    uint32_t isize;
    if (!member_at(z, zn, at, &size, &cdata, &isize)) {
      err = "bai: not a run of whole BGZF members";
      return false;
    }
    for (; ri < recs.size() && recs[ri].vbeg < pay + isize; ++ri) {
      if (recs[ri].vbeg < pay) {
        err = "bai: record offsets do not ascend";
        return false;
      }
      recs[ri].vbeg = (uint64_t)at << 16 | (recs[ri].vbeg - pay);
    }
    pay += isize, at += size;
  }
  if (ri < recs.size()) {
    err = "bai: a record lies behind the members' payload";
    return false;
  }
  return true;
}

bool bai_build_part(const BaiRec* recs, size_t n, uint64_t vend_last, const std::vector<uint32_t>& ref_len, BaiPart& out, std::string& err, int depth) {
  out.chunks.clear(), out.lin.clear(), out.refs.clear();
  out.lin_first = 0;
  if (n == 0) return true;
  const size_t n_ref = ref_len.size();
  std::vector<uint64_t> base(n_ref + 1, 0);
  for (size_t t = 0; t < n_ref; ++t) base[t + 1] = base[t] + (((uint64_t)ref_len[t] + 16383) >> 14);
  const uint64_t max_end = 1ull << (14 + 3 * depth);
  for (size_t i = 0; i < n; ++i) {
    const BaiRec& r = recs[i];
    if (r.tid < 0 || (size_t)r.tid >= n_ref || r.beg < 0 || r.end <= r.beg || (uint64_t)r.end > max_end ||
        (((uint64_t)r.end - 1) >> 14) >= base[(size_t)r.tid + 1] - base[(size_t)r.tid]) {
      err = "bai: record " + std::to_string(i) + " lies outside what " + (depth == kBaiDepth ? std::string("a BAI") : "an index of depth " + std::to_string(depth)) +
            " addresses (refID not in the header, negative pos, or an end beyond 2^" + std::to_string(14 + 3 * depth) + " or its reference)";
      return false;
    }
    if (i && r.tid < recs[i - 1].tid) {
      err = "bai: the records' refIDs decrease at record " + std::to_string(i);
      return false;
    }
  }
  auto vend = [&](size_t i) { return i + 1 < n ? recs[i + 1].vbeg : vend_last; };
  // runs of equal (tid, bin)
  for (size_t i = 0; i < n;) {
    const uint32_t bin = bai_reg2bin(recs[i].beg, recs[i].end, depth);
    size_t j = i + 1;
    while (j < n && recs[j].tid == recs[i].tid && bai_reg2bin(recs[j].beg, recs[j].end, depth) == bin) ++j;
    out.chunks.push_back(BaiChunk{recs[i].tid, bin, recs[i].vbeg, vend(j - 1)});
    i = j;
  }
  std::stable_sort(out.chunks.begin(), out.chunks.end(), [](const BaiChunk& a, const BaiChunk& b) {
    if (a.tid != b.tid) return a.tid < b.tid;
    if (a.bin != b.bin) return a.bin < b.bin;
    return a.beg < b.beg;
  });
  size_t l = 0;
  for (size_t m = 1; m < out.chunks.size(); ++m) {  // htslib's compress_binning: neighbours of one bin that meet in one member
    BaiChunk& a = out.chunks[l];
    const BaiChunk& b = out.chunks[m];
    if (a.tid == b.tid && a.bin == b.bin && (a.end >> 16) >= (b.beg >> 16)) a.end = b.end;
    else out.chunks[++l] = b;
  }
  out.chunks.resize(l + 1);
  // linear table and per-reference ranges
  const int32_t t0 = recs[0].tid, t1 = recs[n - 1].tid;
  int64_t max_end_last = 0;
  for (size_t i = n; i-- > 0 && recs[i].tid == t1;) max_end_last = std::max(max_end_last, recs[i].end);
  out.lin_first = base[(size_t)t0];
  out.lin.assign((size_t)(base[(size_t)t1] + (((uint64_t)max_end_last - 1) >> 14) + 1 - out.lin_first), ~0ull);
  for (size_t i = 0; i < n;) {
    const int32_t t = recs[i].tid;
    uint64_t w_next = 0;  // the first window of t no record has reached yet
    size_t j = i;
    for (; j < n && recs[j].tid == t; ++j) {
      const uint64_t w_end = (((uint64_t)recs[j].end - 1) >> 14) + 1;
      for (; w_next < w_end; ++w_next) out.lin[(size_t)(base[(size_t)t] + w_next - out.lin_first)] = recs[j].vbeg;
    }
    out.refs.push_back(BaiRef{t, 0, (uint64_t)(j - i), recs[i].vbeg, vend(j - 1)});
    i = j;
  }
  return true;
}

bool BaiIndex::init(const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::string& err) {
  for (size_t t = 0; t < lens.size(); ++t)
    if ((uint64_t)lens[t] > kBaiMaxRef) {
      err = "reference " + (t < names.size() ? names[t] : std::to_string(t)) + " is longer than 2^29 (" + std::to_string(lens[t]) + "): a BAI index cannot address it";
      return false;
    }
  csi_ = false, depth_ = kBaiDepth;
  set_refs(lens);
  return true;
}

bool BaiIndex::init_csi(const std::vector<std::string>&, const std::vector<uint32_t>& lens, std::string&) {
  uint64_t longest = 0;
  for (uint32_t l : lens) longest = std::max<uint64_t>(longest, l);
  csi_ = true, depth_ = csi_depth(longest);  // (BAM lengths are below 2^31: depth 6 covers them)
  set_refs(lens);
  return true;
}

void BaiIndex::set_refs(const std::vector<uint32_t>& lens) {
  len_ = lens;
  base_.assign(lens.size() + 1, 0);
  for (size_t t = 0; t < lens.size(); ++t) base_[t + 1] = base_[t] + (((uint64_t)lens[t] + 16383) >> 14);
  ref_.assign(lens.size(), Ref());
  active_ = true;
}

void BaiIndex::add(uint64_t file_base, const BaiChunk* chunks, size_t n_chunks, uint64_t lin_first, const uint64_t* lin, size_t n_lin, const BaiRef* refs,
                   size_t n_refs) {
  const uint64_t sh = file_base << 16;
  for (size_t i = 0; i < n_chunks; ++i) {
    const BaiChunk& c = chunks[i];
    if (c.tid < 0 || (size_t)c.tid >= ref_.size()) continue;
    auto& v = ref_[(size_t)c.tid].bins[c.bin];
    const uint64_t b = c.beg + sh, e = c.end + sh;
    // (a run that straddles two parts ends where the next part begins: the rule that merges neighbours inside a part joins it again)
    if (!v.empty() && (v.back().second >> 16) >= (b >> 16)) v.back().second = e;
    else v.emplace_back(b, e);
  }
  size_t t = 0;
  for (size_t i = 0; i < n_lin; ++i) {
    if (lin[i] == ~0ull) continue;
    const uint64_t f = lin_first + i;
    while (t + 1 < ref_.size() && base_[t + 1] <= f) ++t;
    if (t >= ref_.size() || f < base_[t] || f >= base_[t + 1]) continue;
    std::vector<uint64_t>& L = ref_[t].lin;
    const size_t w = (size_t)(f - base_[t]);
    if (L.size() <= w) L.resize(w + 1, ~0ull);
    L[w] = std::min(L[w], lin[i] + sh);
  }
  for (size_t i = 0; i < n_refs; ++i) {
    if (refs[i].tid < 0 || (size_t)refs[i].tid >= ref_.size()) continue;
    Ref& r = ref_[(size_t)refs[i].tid];
    r.n += refs[i].n_records;
    r.first = std::min(r.first, refs[i].first + sh);
    r.last = std::max(r.last, refs[i].last + sh);
  }
}

// CSIv1 before compression: a bin's loff is the linear table's entry of the bin's first 16 kb window (a record of the bin ends behind the
// bin's start, so the entry exists); the table itself is not written
void BaiIndex::put_ref_csi(std::vector<uint8_t>& o, const Ref& r) const {
  std::vector<uint32_t> first((size_t)depth_ + 2, 0);  // first[l]: the first bin of level l; first[depth + 1] + 1: the meta bin
  for (int l = 0; l <= depth_; ++l) first[(size_t)l + 1] = first[(size_t)l] + (1u << (3 * l));
  put32(o, (uint32_t)r.bins.size() + 1);
  for (const auto& b : r.bins) {
    int l = depth_;
    while (b.first < first[(size_t)l]) --l;
    const uint64_t w = (uint64_t)(b.first - first[(size_t)l]) << (3 * (depth_ - l));
    put32(o, b.first);
    put64(o, w < r.lin.size() && r.lin[w] != ~0ull ? r.lin[w] : 0);
    put32(o, (uint32_t)b.second.size());
    for (const auto& c : b.second) put64(o, c.first), put64(o, c.second);
  }
  put32(o, first[(size_t)depth_ + 1] + 1), put64(o, 0), put32(o, 2);  // the meta bin: what the BAI's pseudo-bin holds
  put64(o, r.first), put64(o, r.last), put64(o, r.n), put64(o, 0);
}

void BaiIndex::serialize_csi(std::vector<uint8_t>& o) const {
  o.insert(o.end(), {'C', 'S', 'I', 1});
  put32(o, 14), put32(o, (uint32_t)depth_), put32(o, 0);
  put32(o, (uint32_t)ref_.size());
  for (const Ref& r : ref_) {
    if (r.n == 0) put32(o, 0);
    else put_ref_csi(o, r);
  }
  put64(o, 0);  // n_no_coor
}

void BaiIndex::put_ref_bai(std::vector<uint8_t>& o, const Ref& r) const {
  put32(o, (uint32_t)r.bins.size() + 1);
  for (const auto& b : r.bins) {  // (a map: ascending bin numbers)
    put32(o, b.first);
    put32(o, (uint32_t)b.second.size());
    for (const auto& c : b.second) put64(o, c.first), put64(o, c.second);
  }
  put32(o, 37450), put32(o, 2);  // the pseudo-bin: the reference's range in the file, mapped / unmapped counts
  put64(o, r.first), put64(o, r.last), put64(o, r.n), put64(o, 0);
  put32(o, (uint32_t)r.lin.size());
  for (uint64_t v : r.lin) put64(o, v);
}

void BaiIndex::serialize(std::vector<uint8_t>& o) const {
  o.clear();
  if (csi_) return serialize_csi(o);
  o.insert(o.end(), {'B', 'A', 'I', 1});
  put32(o, (uint32_t)ref_.size());
  for (const Ref& r : ref_) {
    if (r.n == 0) put32(o, 0), put32(o, 0);
    else put_ref_bai(o, r);
  }
  put64(o, 0);  // n_no_coor: the output holds no unplaced reads
}

void BaiIndex::serialize_tabix(std::vector<uint8_t>& o, const std::vector<std::string>& names, int32_t skip) const {
  o.clear();
  std::vector<uint8_t> hb;  // the header block (htslib: the index's `meta`)
  uint32_t n_live = 0, l_nm = 0;
  for (size_t t = 0; t < ref_.size(); ++t)
    if (ref_[t].n) ++n_live, l_nm += (uint32_t)(t < names.size() ? names[t].size() : 0) + 1;
  put32(hb, 0x10000), put32(hb, 1), put32(hb, 2), put32(hb, 3), put32(hb, '#'), put32(hb, (uint32_t)skip), put32(hb, l_nm);
  for (size_t t = 0; t < ref_.size(); ++t)
    if (ref_[t].n) {
      if (t < names.size()) hb.insert(hb.end(), names[t].begin(), names[t].end());
      hb.push_back(0);
    }
  if (csi_) {
    o.insert(o.end(), {'C', 'S', 'I', 1});
    put32(o, 14), put32(o, (uint32_t)depth_), put32(o, (uint32_t)hb.size());
    o.insert(o.end(), hb.begin(), hb.end());
    put32(o, n_live);
  } else {
    o.insert(o.end(), {'T', 'B', 'I', 1});
    put32(o, n_live);
    o.insert(o.end(), hb.begin(), hb.end());
  }
  for (const Ref& r : ref_) {
    if (r.n == 0) continue;
    if (csi_) put_ref_csi(o, r);
    else put_ref_bai(o, r);
  }
  put64(o, 0);  // n_no_coor
}

namespace {
bool write_bgzf_renamed(const std::vector<uint8_t>& o, const std::string& path, std::string& err) {
  const std::string tmp = path + ".tmp";
  BgzfWriter w;
  const bool ok = w.open(tmp, 6, 1) && w.write(o.data(), o.size());
  if (!(w.close() && ok) || rename(tmp.c_str(), path.c_str()) != 0) {
    (void)unlink(tmp.c_str());
    err = "cannot write " + path;
    return false;
  }
  return true;
}
}  // namespace

bool BaiIndex::write_tabix(const std::string& path, const std::vector<std::string>& names, int32_t skip, std::string& err) const {
  std::vector<uint8_t> o;
  serialize_tabix(o, names, skip);
  return write_bgzf_renamed(o, path, err);
}

bool BaiIndex::write(const std::string& path, std::string& err) const {
  std::vector<uint8_t> o;
  serialize(o);
  const std::string tmp = path + ".tmp";
  if (csi_) return write_bgzf_renamed(o, path, err);  // BGZF members and the EOF member, by the host codec
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) {
    err = "cannot create " + tmp;
    return false;
  }
  const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
  if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) {
    (void)unlink(tmp.c_str());
    err = "cannot write " + path;
    return false;
  }
  return true;
}

bool bai_index_file(const std::string& bam_path, const std::string& bai_path, std::string& err, bool csi) {
  std::vector<uint8_t> z;
  {
    FILE* f = fopen(bam_path.c_str(), "rb");
    if (!f) {
      err = "cannot open " + bam_path;
      return false;
    }
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) z.insert(z.end(), buf, buf + got);
    fclose(f);
  }
  // members: file offset and payload range of each
  struct Mem {
    uint64_t at, pay0, pay1;
  };
  std::vector<Mem> mem;
  std::vector<uint8_t> pay;
  for (size_t at = 0; at < z.size();) {
    size_t size, cdata;
    uint32_t isize;
    if (!member_at(z.data(), z.size(), at, &size, &cdata, &isize)) {
      err = bam_path + ": not a BGZF file";
      return false;
    }
    const size_t p0 = pay.size();
    pay.resize(p0 + isize);
    if (!bgzf_inflate_member(z.data() + cdata, at + size - 8 - cdata, pay.data() + p0, isize, le32(z.data() + at + size - 8))) {
      err = bam_path + ": a BGZF member does not inflate";
      return false;
    }
    mem.push_back(Mem{at, p0, p0 + isize});
    at += size;
  }
  // header
  auto need = [&](size_t p, size_t k) { return p + k <= pay.size(); };
  if (!need(0, 12) || memcmp(pay.data(), "BAM\1", 4) != 0) {
    err = bam_path + ": not a BAM file";
    return false;
  }
  size_t p = 8 + (size_t)le32(pay.data() + 4);
  if (!need(p, 4)) {
    err = bam_path + ": truncated header";
    return false;
  }
  const uint32_t n_ref = le32(pay.data() + p);
  p += 4;
  std::vector<std::string> names;
  std::vector<uint32_t> lens;
  for (uint32_t t = 0; t < n_ref; ++t) {
    if (!need(p, 4)) {
      err = bam_path + ": truncated header";
      return false;
    }
    const uint32_t ln = le32(pay.data() + p);
    if (!need(p + 4, (size_t)ln + 4)) {
      err = bam_path + ": truncated header";
      return false;
    }
    names.emplace_back((const char*)pay.data() + p + 4, ln ? ln - 1 : 0);
    lens.push_back(le32(pay.data() + p + 4 + ln));
    p += 8 + (size_t)ln;
  }
  BaiIndex ix;
  if (!(csi ? ix.init_csi(names, lens, err) : ix.init(names, lens, err))) return false;
  // records; a payload offset's virtual offset: the member that holds the byte (the end of the payload: the EOF member, else the file's end)
  size_t mi = 0;
  auto voff = [&](uint64_t q) {
    while (mi < mem.size() && q >= mem[mi].pay1) ++mi;
    if (mi < mem.size()) return mem[mi].at << 16 | (q - mem[mi].pay0);
    return (!mem.empty() && mem.back().pay0 == mem.back().pay1 ? mem.back().at : (uint64_t)z.size()) << 16;
  };
  std::vector<BaiRec> recs;
  while (p < pay.size()) {
    if (!need(p, 4) || !need(p + 4, le32(pay.data() + p))) {
      err = bam_path + ": truncated record";
      return false;
    }
    const uint32_t bs = le32(pay.data() + p);
    BaiRec r;
    if (!bai_rec_span(pay.data() + p + 4, bs, &r.tid, &r.beg, &r.end)) {
      err = bam_path + ": malformed record";
      return false;
    }
    if (r.tid < 0) {
      err = bam_path + ": an unplaced read (the index of tiebrush's output holds none)";
      return false;
    }
    r.vbeg = voff(p);
    recs.push_back(r);
    p += 4 + (size_t)bs;
  }
  BaiPart part;
  if (!bai_build_part(recs.data(), recs.size(), voff(pay.size()), lens, part, err, ix.depth())) return false;
  ix.add(0, part);
  return ix.write(bai_path, err);
}

}  // namespace tbh
