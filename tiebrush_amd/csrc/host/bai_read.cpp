// bai_read.cpp — BAI / CSI reader, region query, region parser, chunk reads (bai_read.h)
#include "bai_read.h"

#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <unordered_map>

#include "bgzf.h"

namespace tbh {
namespace {
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

bool slurp(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t buf[1 << 16];
  size_t got;
  out.clear();
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  const bool ok = !ferror(f);
  fclose(f);
  return ok;
}
bool exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
// the size of the BGZF member whose first bytes are h[0, n) (n >= 12 + its XLEN); 0 when it is not one
size_t member_size(const uint8_t* h, size_t n) {
  if (n < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return 0;
  const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
  if (12 + xlen > n) return 0;
  for (size_t x = 12; x + 4 <= 12 + xlen;) {
    const size_t sl = (size_t)h[x + 2] | (size_t)h[x + 3] << 8;
    if (h[x] == 'B' && h[x + 1] == 'C' && sl == 2 && x + 6 <= 12 + xlen) {
      const size_t bsize = ((size_t)h[x + 4] | (size_t)h[x + 5] << 8) + 1;
      return bsize < 12 + xlen + 8 ? 0 : bsize;
    }
    x += 4 + sl;
  }
  return 0;
}
bool pread_all(int fd, uint64_t at, uint8_t* dst, size_t n) {
  while (n) {
    const ssize_t got = pread(fd, dst, n, (off_t)at);
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) return false;
    dst += got, at += (uint64_t)got, n -= (size_t)got;
  }
  return true;
}
// where the bytes of chunk c end in its file (*stop): c.end's member, or behind it when the chunk ends inside it (the member's size is in
// its own header, which is read).  false, with err, for a chunk that lies outside the file of fsize bytes, begins before prev_end (the
// stop of the chunk before it) or does not end in a member.  `index` is how the message names the index.
bool chunk_extent(int fd, uint64_t fsize, const IdxChunk& c, uint64_t prev_end, uint64_t* stop, const std::string& index, const std::string& bam_path,
                  std::string& err) {
  const uint64_t c0 = c.beg >> 16, c1 = c.end >> 16;
  const uint32_t u1 = (uint32_t)(c.end & 0xffff);
  char where[96];
  snprintf(where, sizeof(where), "%llx-%llx", (unsigned long long)c.beg, (unsigned long long)c.end);
  if (c.beg >= c.end || c0 + 18 > fsize || c1 > fsize || (u1 && c1 + 18 > fsize) || c0 < prev_end)
    return err = index + " names a chunk outside " + bam_path + " (" + where + ", file size " + std::to_string(fsize) + ")", false;
  *stop = c1;
  if (u1) {  // the last member is part of the chunk
    uint8_t h[18 + 256];
    const size_t hn = (size_t)std::min<uint64_t>(sizeof(h), fsize - c1);
    const size_t ms = pread_all(fd, c1, h, hn) ? member_size(h, hn) : 0;
    if (!ms || c1 + ms > fsize) return err = index + " names a chunk that does not end in a BGZF member of " + bam_path + " (" + where + ")", false;
    *stop = c1 + ms;
  }
  return true;
}
}  // namespace

bool RegionIndex::load(const std::string& path, std::string& err) {
  std::vector<uint8_t> b;
  if (!slurp(path, b)) {
    err = "cannot read the index " + path;
    return false;
  }
  if (!parse(b, err)) {
    err = path + ": " + err;
    return false;
  }
  return true;
}

bool RegionIndex::parse(const std::vector<uint8_t>& file_bytes, std::string& err) {
  refs_.clear();
  std::vector<uint8_t> inflated;
  const std::vector<uint8_t>* src = &file_bytes;
  if (file_bytes.size() >= 4 && memcmp(file_bytes.data(), "BAI\1", 4) == 0) {
    csi_ = false, min_shift_ = 14, depth_ = 5;
  } else if (file_bytes.size() >= 18 && file_bytes[0] == 31 && file_bytes[1] == 139) {
    size_t used = 0;
    std::string e;
    if (!bgzf_inflate_chunk(file_bytes.data(), file_bytes.size(), true, inflated, &used, e, 1, "index") || used != file_bytes.size()) {
      err = "truncated or damaged CSI index (" + (e.empty() ? std::string("a cut member") : e) + ")";
      return false;
    }
    if (inflated.size() < 4 || memcmp(inflated.data(), "CSI\1", 4) != 0) {
      err = "not a BAI or CSI index (magic)";
      return false;
    }
    csi_ = true;
    src = &inflated;
  } else {
    err = "not a BAI or CSI index (magic)";
    return false;
  }
  const uint8_t* b = src->data();
  const size_t n = src->size();
  size_t p = 4;
  auto need = [&](size_t k) { return k <= n && p <= n - k; };
  const char* cut = "truncated index";
  int32_t n_ref;
  if (csi_) {
    if (!need(16)) return err = cut, false;
    min_shift_ = (int32_t)le32(b + p), depth_ = (int32_t)le32(b + p + 4);
    const int32_t l_aux = (int32_t)le32(b + p + 8);
    p += 12;
    if (min_shift_ < 1 || min_shift_ > 30 || depth_ < 0 || depth_ > 10 || min_shift_ + 3 * depth_ > 62 || l_aux < 0) return err = "CSI header out of range", false;
    if (!need((size_t)l_aux + 4)) return err = cut, false;
    p += (size_t)l_aux;
  } else if (!need(4)) {
    return err = cut, false;
  }
  n_ref = (int32_t)le32(b + p);
  p += 4;
  if (n_ref < 0) return err = "negative n_ref", false;
  const uint32_t skip_bin = csi_ ? (uint32_t)(((1ull << (3 * (depth_ + 1))) - 1) / 7 + 1) : 37450u;
  for (int32_t t = 0; t < n_ref; ++t) {
    if (!need(4)) return err = cut, false;
    const int32_t n_bin = (int32_t)le32(b + p);
    p += 4;
    if (n_bin < 0) return err = "negative n_bin", false;
    Ref R;
    for (int32_t k = 0; k < n_bin; ++k) {
      if (!need(csi_ ? 16 : 8)) return err = cut, false;
      Bin B;
      B.bin = le32(b + p);
      B.loff = csi_ ? le64(b + p + 4) : 0;
      const int32_t nc = (int32_t)le32(b + p + (csi_ ? 12 : 4));
      p += csi_ ? 16 : 8;
      if (nc < 0 || !need((size_t)nc * 16)) return err = cut, false;
      if (B.bin != skip_bin) {
        B.chunks.resize((size_t)nc);
        for (int32_t c = 0; c < nc; ++c) B.chunks[(size_t)c] = IdxChunk{le64(b + p + 16 * (size_t)c), le64(b + p + 16 * (size_t)c + 8)};
        R.bins.push_back(std::move(B));
      }
      p += (size_t)nc * 16;
    }
    if (!csi_) {
      if (!need(4)) return err = cut, false;
      const int32_t n_intv = (int32_t)le32(b + p);
      p += 4;
      if (n_intv < 0 || !need((size_t)n_intv * 8)) return err = cut, false;
      R.lin.resize((size_t)n_intv);
      for (int32_t w = 0; w < n_intv; ++w) R.lin[(size_t)w] = le64(b + p + 8 * (size_t)w);
      p += (size_t)n_intv * 8;
    }
    std::sort(R.bins.begin(), R.bins.end(), [](const Bin& a, const Bin& c) { return a.bin < c.bin; });
    refs_.push_back(std::move(R));
  }
  // (n_no_coor is optional in both formats)
  if (p != n && p + 8 != n) return err = "trailing bytes behind the index", false;
  return true;
}

const RegionIndex::Bin* RegionIndex::find(const Ref& r, uint32_t bin) const {
  auto it = std::lower_bound(r.bins.begin(), r.bins.end(), bin, [](const Bin& a, uint32_t b) { return a.bin < b; });
  return it != r.bins.end() && it->bin == bin ? &*it : nullptr;
}

void RegionIndex::query(int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& out) const {
  std::vector<IdxChunk> all;
  collect(tid, beg, end, all);
  merge(all, out);
}

void RegionIndex::query_regions(const RegionTable& U, std::vector<IdxChunk>& out) const {
  std::vector<IdxChunk> all;
  for (size_t r = 0; r < U.n(); ++r) collect(U.tid[r], U.beg[r], U.end[r], all);
  merge(all, out);
}

void RegionIndex::merge(std::vector<IdxChunk>& all, std::vector<IdxChunk>& out) {
  out.clear();
  std::sort(all.begin(), all.end(), [](const IdxChunk& a, const IdxChunk& c) { return a.beg < c.beg || (a.beg == c.beg && a.end < c.end); });
  for (const IdxChunk& c : all) {
    if (!out.empty() && (out.back().end >> 16) >= (c.beg >> 16)) {
      if (c.end > out.back().end) out.back().end = c.end;
    } else {
      out.push_back(c);
    }
  }
}

void RegionIndex::collect(int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& all) const {
  if (tid < 0 || (size_t)tid >= refs_.size() || beg < 0) return;
  const int64_t reach = 1ll << (min_shift_ + 3 * depth_);  // no record the index holds ends behind it
  if (end > reach) end = reach;
  if (beg >= end) return;
  const Ref& R = refs_[(size_t)tid];
  uint64_t min_off = 0;
  if (!csi_) {
    const uint64_t w = (uint64_t)beg >> 14;
    if (!R.lin.empty()) min_off = w < R.lin.size() ? R.lin[w] : R.lin.back();
  } else {
    uint64_t b = ((1ull << (3 * depth_)) - 1) / 7 + ((uint64_t)beg >> min_shift_);
    for (;;) {
      if (const Bin* B = find(R, (uint32_t)b)) {
        min_off = B->loff;
        break;
      }
      if (b == 0) break;
      b = (b - 1) >> 3;
    }
  }
  auto take = [&](uint64_t bin) {
    if (const Bin* B = find(R, (uint32_t)bin))
      for (const IdxChunk& c : B->chunks)
        if (c.end > min_off && c.beg < c.end) all.push_back(c);
  };
  take(0);
  for (int l = 1; l <= depth_; ++l) {
    const int s = min_shift_ + 3 * (depth_ - l);
    const uint64_t first = ((1ull << (3 * l)) - 1) / 7;
    // (the bins present are few: walk them, not the range, when the range is the longer of the two)
    const uint64_t lo = first + ((uint64_t)beg >> s), hi = first + ((uint64_t)(end - 1) >> s);
    if (hi - lo + 1 <= R.bins.size()) {
      for (uint64_t bin = lo; bin <= hi; ++bin) take(bin);
    } else {
      for (const Bin& B : R.bins)
        if (B.bin >= lo && B.bin <= hi) take(B.bin);
    }
  }
}

bool find_index(const std::string& bam_path, const std::string& explicit_path, std::string& found, std::string& err) {
  if (!explicit_path.empty()) {
    if (exists(explicit_path)) return found = explicit_path, true;
    err = "no index found: " + explicit_path + " does not exist";
    return false;
  }
  std::vector<std::string> tries = {bam_path + ".csi", bam_path + ".bai"};
  const size_t dot = bam_path.rfind('.'), slash = bam_path.rfind('/');
  if (dot != std::string::npos && (slash == std::string::npos || dot > slash + 1)) tries.push_back(bam_path.substr(0, dot) + ".bai");
  for (const std::string& t : tries)
    if (exists(t)) return found = t, true;
  err = "no index found for " + bam_path + " (tried";
  for (size_t i = 0; i < tries.size(); ++i) err += (i ? ", " : " ") + tries[i];
  err += "): write one with `tiebrush --index` / `--csi`, or name it with --index-file";
  return false;
}

static bool parse_coord(const std::string& s, int64_t* v) {  // digits and commas, at least one digit, no more than 2^40
  int64_t x = 0;
  bool any = false;
  for (char c : s) {
    if (c == ',') continue;
    if (c < '0' || c > '9') return false;
    x = x * 10 + (c - '0');
    any = true;
    if (x > (1ll << 40)) return false;
  }
  *v = x;
  return any;
}

bool parse_region(const BamHeader& hdr, const std::string& region, int32_t* tid, int64_t* beg, int64_t* end, std::string& err) {
  if (region.empty()) return err = "malformed region '' (expected NAME, NAME:BEG or NAME:BEG-END)", false;
  int t = hdr.name2tid(region);
  if (t >= 0) {
    *tid = t, *beg = 0, *end = hdr.target_len[(size_t)t];
    return true;
  }
  const size_t colon = region.rfind(':');
  if (colon == std::string::npos) return err = "unknown reference name '" + region + "'", false;
  const std::string name = region.substr(0, colon), range = region.substr(colon + 1);
  t = hdr.name2tid(name);
  if (t < 0) return err = "unknown reference name '" + name + "' (region '" + region + "')", false;
  const int64_t len = hdr.target_len[(size_t)t];
  const std::string bad = "malformed region '" + region + "' (expected NAME, NAME:BEG or NAME:BEG-END, 1-based, BEG >= 1)";
  int64_t b1 = 0, e1 = len;
  const size_t dash = range.find('-');
  if (!parse_coord(range.substr(0, dash), &b1) || b1 < 1) return err = bad, false;
  if (dash != std::string::npos) {
    if (!parse_coord(range.substr(dash + 1), &e1)) return err = bad, false;
    if (b1 > e1) return err = "malformed region '" + region + "': BEG > END", false;
  }
  *tid = t;
  *end = std::min(e1, len);
  *beg = std::min(b1 - 1, *end);  // (a BEG behind the reference: the empty region at its end)
  return true;
}

bool RegionTable::normalised() const {
  if (tid.empty() || beg.size() != tid.size() || end.size() != tid.size()) return false;
  for (size_t r = 0; r < tid.size(); ++r) {
    if (tid[r] < 0 || beg[r] < 0 || end[r] <= beg[r]) return false;
    if (r && (tid[r] < tid[r - 1] || (tid[r] == tid[r - 1] && beg[r] <= end[r - 1]))) return false;
  }
  return true;
}

static bool bed_coord(const std::string& s, int64_t* v) {  // digits only, no more than 2^40
  if (s.empty()) return false;
  int64_t x = 0;
  for (char c : s) {
    if (c < '0' || c > '9') return false;
    x = x * 10 + (c - '0');
    if (x > (1ll << 40)) return false;
  }
  *v = x;
  return true;
}

bool regions_from_bed(const BamHeader& hdr, const std::string& text, const std::string& what, RegionTable& U, std::string& err) {
  struct Iv {
    int32_t tid;
    int64_t beg, end;
  };
  std::vector<Iv> iv;
  size_t lineno = 0;
  bool any = false;
  for (size_t p = 0; p < text.size();) {
    size_t nl = text.find('\n', p);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(p, nl - p);
    p = nl + 1;
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const std::string at = what + " line " + std::to_string(lineno) + ": ";
    std::vector<std::string> f;
    for (size_t q = 0; q < line.size() && f.size() < 3;) {
      while (q < line.size() && (line[q] == '\t' || line[q] == ' ')) ++q;
      size_t e = q;
      while (e < line.size() && line[e] != '\t' && line[e] != ' ') ++e;
      if (e > q) f.push_back(line.substr(q, e - q));
      q = e;
    }
    if (f.empty() || f[0][0] == '#' || f[0] == "track" || f[0] == "browser") continue;
    if (f.size() < 3) return err = at + "fewer than three fields (expected chrom start end)", false;
    int64_t b = 0, e = 0;
    if (!bed_coord(f[1], &b)) return err = at + "the start '" + f[1] + "' is not a non-negative integer", false;
    if (!bed_coord(f[2], &e)) return err = at + "the end '" + f[2] + "' is not a non-negative integer", false;
    if (b > e) return err = at + "start > end", false;
    const int t = hdr.name2tid(f[0]);
    if (t < 0) return err = at + "unknown reference name '" + f[0] + "'", false;
    any = true;
    e = std::min<int64_t>(e, hdr.target_len[(size_t)t]);
    if (b < e) iv.push_back(Iv{(int32_t)t, b, e});
  }
  U = RegionTable();
  std::sort(iv.begin(), iv.end(), [](const Iv& a, const Iv& c) { return a.tid < c.tid || (a.tid == c.tid && (a.beg < c.beg || (a.beg == c.beg && a.end < c.end))); });
  for (const Iv& x : iv) {
    if (U.n() && U.tid.back() == x.tid && x.beg <= U.end.back())  // overlap or abut: one interval
      U.end.back() = std::max(U.end.back(), x.end);
    else
      U.add(x.tid, x.beg, x.end);
  }
  if (U.n() == 0) return err = what + ": no region" + (any ? " left (every interval is empty on its reference)" : " in it"), false;
  return true;
}

bool regions_from_bed_file(const BamHeader& hdr, const std::string& bed_path, RegionTable& U, std::string& err) {
  std::vector<uint8_t> b;
  if (!slurp(bed_path, b)) return err = "cannot read the regions file " + bed_path, false;
  return regions_from_bed(hdr, std::string(b.begin(), b.end()), bed_path, U, err);
}

bool features_from_bed(const BamHeader& hdr, const std::string& text, const std::string& what, FeatureTable& F, std::string& err) {
  F = FeatureTable();
  size_t lineno = 0;
  for (size_t p = 0; p < text.size();) {
    size_t nl = text.find('\n', p);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(p, nl - p);
    p = nl + 1;
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const std::string at = what + " line " + std::to_string(lineno) + ": ";
    std::vector<std::string> f;
    for (size_t q = 0; q < line.size() && f.size() < 6;) {
      while (q < line.size() && (line[q] == '\t' || line[q] == ' ')) ++q;
      size_t e = q;
      while (e < line.size() && line[e] != '\t' && line[e] != ' ') ++e;
      if (e > q) f.push_back(line.substr(q, e - q));
      q = e;
    }
    if (f.empty() || f[0][0] == '#' || f[0] == "track" || f[0] == "browser") continue;
    if (f.size() < 3) return err = at + "fewer than three fields (expected chrom start end [name [score [strand]]])", false;
    int64_t b = 0, e = 0;
    if (!bed_coord(f[1], &b)) return err = at + "the start '" + f[1] + "' is not a non-negative integer", false;
    if (!bed_coord(f[2], &e)) return err = at + "the end '" + f[2] + "' is not a non-negative integer", false;
    if (b > e) return err = at + "start > end", false;
    const int t = hdr.name2tid(f[0]);
    if (t < 0) return err = at + "unknown reference name '" + f[0] + "'", false;
    uint8_t strand = '.';
    if (f.size() >= 6) {
      if (f[5] != "+" && f[5] != "-" && f[5] != ".") return err = at + "the strand '" + f[5] + "' is not one of + - .", false;
      strand = (uint8_t)f[5][0];
    }
    e = std::min<int64_t>(e, hdr.target_len[(size_t)t]);
    if (b >= e) return err = at + "the feature is empty on its reference", false;
    F.tid.push_back((int32_t)t), F.beg.push_back(b), F.end.push_back(e), F.strand.push_back(strand);
    F.name.push_back(f.size() >= 4 ? f[3] : std::string("."));
    F.line.push_back(lineno);
  }
  if (F.n() == 0) return err = what + ": no feature in it", false;
  return true;
}

bool features_from_bed_file(const BamHeader& hdr, const std::string& bed_path, FeatureTable& F, std::string& err) {
  std::vector<uint8_t> b;
  if (!slurp(bed_path, b)) return err = "cannot read the features file " + bed_path, false;
  return features_from_bed(hdr, std::string(b.begin(), b.end()), bed_path, F, err);
}

bool features_inside(const FeatureTable& F, const RegionTable& U, const std::string& what, std::string& err) {
  for (size_t i = 0; i < F.n(); ++i) {
    // the last interval that begins at or before the feature's begin on its reference
    size_t lo = 0, hi = U.n();
    while (lo < hi) {
      const size_t m = lo + (hi - lo) / 2;
      if (U.tid[m] < F.tid[i] || (U.tid[m] == F.tid[i] && U.beg[m] <= F.beg[i]))
        lo = m + 1;
      else
        hi = m;
    }
    if (lo == 0 || U.tid[lo - 1] != F.tid[i] || U.end[lo - 1] < F.end[i])
      return err = what + " line " + std::to_string(F.line[i]) + ": the feature is not wholly inside one interval of the region", false;
  }
  return true;
}

// the value of `key` among the `key value;` pairs of a GTF line's ninth column: quoted (a ';' inside the quotes belongs to it) or bare
static bool gtf_attr(const std::string& a, const char* key, std::string* value) {
  const size_t klen = strlen(key);
  for (size_t p = 0; p < a.size();) {
    while (p < a.size() && (a[p] == ' ' || a[p] == '\t' || a[p] == ';')) ++p;
    size_t k = p;
    while (k < a.size() && a[k] != ' ' && a[k] != '\t' && a[k] != ';' && a[k] != '"') ++k;
    const bool hit = k - p == klen && a.compare(p, klen, key) == 0;
    p = k;
    while (p < a.size() && (a[p] == ' ' || a[p] == '\t')) ++p;
    std::string v;
    if (p < a.size() && a[p] == '"') {
      const size_t q = a.find('"', p + 1);
      v = a.substr(p + 1, (q == std::string::npos ? a.size() : q) - p - 1);
      p = q == std::string::npos ? a.size() : q + 1;
      while (p < a.size() && a[p] != ';') ++p;  // (whatever stands between the closing quote and the ';')
    } else {
      size_t q = p;
      while (q < a.size() && a[q] != ';') ++q;
      v = a.substr(p, q - p);
      while (!v.empty() && (v.back() == ' ' || v.back() == '\t')) v.pop_back();
      p = q;
    }
    if (hit) return *value = v, true;
  }
  return false;
}

bool transcripts_from_gtf(const BamHeader& hdr, const std::string& text, const std::string& what, TranscriptTable& X, std::string& err) {
  struct Exon {
    int64_t beg, end;
    uint64_t line;
  };
  struct Tx {
    int32_t tid;
    uint8_t strand;
    uint64_t line;
    std::string id, gene;
    std::vector<Exon> ex;
  };
  std::vector<Tx> txs;
  std::unordered_map<std::string, size_t> by_id;
  size_t lineno = 0;
  for (size_t p = 0; p < text.size();) {
    size_t nl = text.find('\n', p);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(p, nl - p);
    p = nl + 1;
    ++lineno;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    const size_t first = line.find_first_not_of(" \t");
    if (first == std::string::npos || line[first] == '#') continue;
    const std::string at = what + " line " + std::to_string(lineno) + ": ";
    std::vector<std::string> f;  // eight columns and the rest
    for (size_t q = 0; f.size() < 9;) {
      const size_t e = f.size() == 8 ? std::string::npos : line.find('\t', q);
      f.push_back(line.substr(q, e == std::string::npos ? std::string::npos : e - q));
      if (e == std::string::npos) break;
      q = e + 1;
    }
    if (f.size() < 3 || f[2] != "exon") continue;
    if (f.size() < 9) return err = at + "fewer than nine columns on an exon line", false;
    int64_t b1 = 0, e1 = 0;
    if (!bed_coord(f[3], &b1)) return err = at + "the start '" + f[3] + "' is not a non-negative integer", false;
    if (!bed_coord(f[4], &e1)) return err = at + "the end '" + f[4] + "' is not a non-negative integer", false;
    if (b1 < 1) return err = at + "start < 1 (GTF coordinates are 1-based)", false;
    if (e1 < b1) return err = at + "end < start", false;
    const int t = hdr.name2tid(f[0]);
    if (t < 0) return err = at + "unknown reference name '" + f[0] + "'", false;
    if (e1 > (int64_t)hdr.target_len[(size_t)t]) return err = at + "the exon ends beyond its reference (" + f[0] + " has " + std::to_string(hdr.target_len[(size_t)t]) + " bases)", false;
    if (f[6] != "+" && f[6] != "-" && f[6] != ".") return err = at + "the strand '" + f[6] + "' is not one of + - .", false;
    std::string id, gene = ".";
    if (!gtf_attr(f[8], "transcript_id", &id) || id.empty()) return err = at + "an exon line without transcript_id", false;
    (void)gtf_attr(f[8], "gene_id", &gene);
    if (gene.empty()) gene = ".";
    auto it = by_id.find(id);
    if (it == by_id.end()) {
      it = by_id.emplace(id, txs.size()).first;
      txs.push_back(Tx{(int32_t)t, (uint8_t)f[6][0], lineno, id, gene, {}});
    }
    Tx& x = txs[it->second];
    if (x.tid != t) return err = at + "transcript " + id + " is on two references (" + hdr.target_name[(size_t)x.tid] + " on line " + std::to_string(x.line) + ")", false;
    if (x.strand != (uint8_t)f[6][0]) return err = at + "transcript " + id + " is on two strands (" + std::string(1, (char)x.strand) + " on line " + std::to_string(x.line) + ")", false;
    x.ex.push_back(Exon{b1 - 1, e1, lineno});
  }
  if (txs.empty()) return err = what + ": no exon line in it", false;
  X = TranscriptTable();
  for (Tx& x : txs) {
    std::stable_sort(x.ex.begin(), x.ex.end(), [](const Exon& a, const Exon& c) { return a.beg < c.beg; });
    for (size_t e = 1; e < x.ex.size(); ++e)
      if (x.ex[e].beg <= x.ex[e - 1].end)
        return err = what + " line " + std::to_string(std::max(x.ex[e].line, x.ex[e - 1].line)) + ": two exons of transcript " + x.id + " overlap or abut (the other is on line " +
                     std::to_string(std::min(x.ex[e].line, x.ex[e - 1].line)) + "; an intron has at least one base)",
               false;
    X.tid.push_back(x.tid), X.strand.push_back(x.strand), X.line.push_back(x.line), X.id.push_back(x.id), X.gene.push_back(x.gene);
    for (const Exon& e : x.ex) X.ex_beg.push_back(e.beg), X.ex_end.push_back(e.end);
    X.tx_off.push_back((uint32_t)X.ex_beg.size());
  }
  return true;
}

bool transcripts_from_gtf_file(const BamHeader& hdr, const std::string& gtf_path, TranscriptTable& X, std::string& err) {
  std::vector<uint8_t> b;
  if (!slurp(gtf_path, b)) return err = "cannot read the annotation file " + gtf_path, false;
  return transcripts_from_gtf(hdr, std::string(b.begin(), b.end()), gtf_path, X, err);
}

FeatureTable transcript_spans(const TranscriptTable& X) {
  FeatureTable F;
  for (size_t t = 0; t < X.n_tx(); ++t) {
    F.tid.push_back(X.tid[t]), F.beg.push_back(X.ex_beg[X.tx_off[t]]), F.end.push_back(X.ex_end[X.tx_off[t + 1] - 1]);
    F.strand.push_back(X.strand[t]), F.name.push_back(X.id[t]), F.line.push_back(X.line[t]);
  }
  return F;
}

bool read_spans(const std::string& bam_path, const std::vector<IdxChunk>& chunks, std::vector<RegionSpan>& spans, uint64_t* bytes_read, std::string& err) {
  spans.clear();
  if (bytes_read) *bytes_read = 0;
  const int fd = open(bam_path.c_str(), O_RDONLY);
  if (fd < 0) return err = "cannot open " + bam_path, false;
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return err = "cannot stat " + bam_path, false;
  }
  const uint64_t fsize = (uint64_t)st.st_size;
  auto rd = [&](uint64_t at, uint8_t* dst, size_t n) { return pread_all(fd, at, dst, n); };
  bool ok = true;
  uint64_t prev_end = 0;
  for (const IdxChunk& c : chunks) {
    const uint64_t c0 = c.beg >> 16;
    uint64_t stop = 0;
    if (!chunk_extent(fd, fsize, c, prev_end, &stop, "the index", bam_path, err)) {
      ok = false;
      break;
    }
    RegionSpan s;
    s.first_uoff = (uint32_t)(c.beg & 0xffff), s.last_uoff = (uint32_t)(c.end & 0xffff);
    s.z.resize((size_t)(stop - c0));
    if (!rd(c0, s.z.data(), s.z.size())) {
      err = "read failed on " + bam_path;
      ok = false;
      break;
    }
    if (bytes_read) *bytes_read += s.z.size();
    prev_end = stop;
    spans.push_back(std::move(s));
  }
  close(fd);
  return ok;
}

bool inflate_span(const RegionSpan& s, std::vector<uint8_t>& records, std::string& err) {
  records.clear();
  std::vector<uint8_t> pay;
  size_t used = 0, last_isize = 0;
  if (!s.z.empty() && (!bgzf_inflate_chunk(s.z.data(), s.z.size(), true, pay, &used, err, 1, "chunk") || used != s.z.size())) {
    if (err.empty()) err = "a chunk is not a run of whole BGZF members";
    return false;
  }
  if (s.z.size() >= 4) last_isize = le32(s.z.data() + s.z.size() - 4);
  size_t stop = pay.size();
  if (s.last_uoff) {
    if (s.last_uoff > last_isize || last_isize > pay.size()) return err = "a chunk ends behind its last member's payload", false;
    stop = pay.size() - last_isize + s.last_uoff;
  }
  if (s.first_uoff > stop) return err = "a chunk begins behind its end", false;
  records.assign(pay.begin() + s.first_uoff, pay.begin() + (ptrdiff_t)stop);
  return true;
}

bool span_records(const RegionSpan& s, uint64_t file_off, std::vector<BaiRec>& recs, std::string& err) {
  recs.clear();
  std::vector<uint8_t> r;
  if (!inflate_span(s, r, err)) return false;
  for (size_t p = 0; p < r.size();) {
    if (r.size() - p < 4) return err = "a chunk does not end on a record", false;
    const uint32_t bs = le32(r.data() + p);
    BaiRec b;
    if (bs < 32 || bs > r.size() - p - 4 || !bai_rec_span(r.data() + p + 4, bs, &b.tid, &b.beg, &b.end)) return err = "a chunk does not end on a record", false;
    b.vbeg = s.first_uoff + p;
    recs.push_back(b);
    p += 4 + (size_t)bs;
  }
  if (!bai_member_voffsets(s.z.data(), s.z.size(), recs, err)) return false;
  for (BaiRec& b : recs) b.vbeg += file_off << 16;
  return true;
}

// the intervals of U against a header of n_ref references: what index_query_file's one region has always been held to
static bool table_in_range(const RegionTable& U, int32_t n_ref) {
  for (size_t r = 0; r < U.n(); ++r)
    if (U.tid[r] < 0 || U.tid[r] >= n_ref || U.beg[r] < 0 || U.end[r] < U.beg[r]) return false;
  return true;
}
static RegionTable table_of_one(int32_t tid, int64_t beg, int64_t end) {
  RegionTable U;
  U.add(tid, beg, end);
  return U;
}

bool index_query_file(const std::string& bam_path, const std::string& index_path, int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& out,
                      std::string& err) {
  return index_query_regions_file(bam_path, index_path, table_of_one(tid, beg, end), out, err);
}

bool index_query_regions_file(const std::string& bam_path, const std::string& index_path, const RegionTable& U, std::vector<IdxChunk>& out, std::string& err) {
  BamFile bf;
  if (!bf.open(bam_path, err, 1)) return false;
  std::string found;
  if (!find_index(bam_path, index_path, found, err)) return false;
  RegionIndex ix;
  if (!ix.load(found, err)) return false;
  if (ix.n_ref() != (size_t)bf.hdr.n_targets) {
    err = found + ": the index has " + std::to_string(ix.n_ref()) + " references, the header of " + bam_path + " has " + std::to_string(bf.hdr.n_targets);
    return false;
  }
  if (!table_in_range(U, bf.hdr.n_targets)) return err = "index query: tid / beg / end out of range", false;
  if (U.n() > 1 && !U.normalised()) return err = "index query: the region table is not sorted, disjoint, non-empty and non-adjacent", false;
  ix.query_regions(U, out);
  return true;
}

bool region_input_chunks(const std::string& bam_path, int32_t file_n_ref, int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& chunks,
                         std::string& index_path, std::string& err) {
  return regions_input_chunks(bam_path, file_n_ref, table_of_one(tid, beg, end), chunks, index_path, err);
}

bool regions_input_chunks(const std::string& bam_path, int32_t file_n_ref, const RegionTable& U, std::vector<IdxChunk>& chunks, std::string& index_path,
                          std::string& err) {
  chunks.clear();
  if (!find_index(bam_path, "", index_path, err)) {  // (the paths tried; the advice is find_index's caller's)
    const size_t cut = err.find("): ");
    if (cut != std::string::npos) err = err.substr(0, cut) + "): write one with `tiebrush --index` / `--csi` or `samtools index`";
    return false;
  }
  RegionIndex ix;
  if (!ix.load(index_path, err)) {
    if (err.find(index_path) == std::string::npos) err = index_path + ": " + err;
    return false;
  }
  if (ix.n_ref() != (size_t)file_n_ref) {
    err = index_path + ": the index has " + std::to_string(ix.n_ref()) + " references, the header of " + bam_path + " has " + std::to_string(file_n_ref);
    return false;
  }
  if (!table_in_range(U, file_n_ref)) return err = bam_path + ": index query: tid / beg / end out of range", false;
  ix.query_regions(U, chunks);  // (an empty interval names no chunk)
  if (chunks.empty()) return true;
  const int fd = open(bam_path.c_str(), O_RDONLY);  // (read_spans' own conditions, the header of each chunk's last member included)
  if (fd < 0) return err = "cannot open " + bam_path, false;
  struct stat st;
  bool ok = fstat(fd, &st) == 0;
  if (!ok) err = "cannot stat " + bam_path;
  uint64_t prev = 0;
  for (size_t i = 0; ok && i < chunks.size(); ++i) ok = chunk_extent(fd, (uint64_t)st.st_size, chunks[i], prev, &prev, "the index " + index_path, bam_path, err);
  close(fd);
  return ok;
}

bool read_spans_many(const std::vector<std::string>& paths, const std::vector<std::vector<IdxChunk>>& chunks, int threads,
                     std::vector<std::vector<RegionSpan>>& spans, uint64_t* bytes_read, std::string& err) {
  const size_t k = paths.size();
  spans.assign(k, {});
  std::vector<uint64_t> bytes(k, 0);
  std::vector<std::string> errs(k);
  std::vector<uint8_t> ok(k, 1);
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (;;) {
      const size_t f = next.fetch_add(1);
      if (f >= k) break;
      if (chunks[f].empty()) continue;
      ok[f] = read_spans(paths[f], chunks[f], spans[f], &bytes[f], errs[f]) ? 1 : 0;
    }
  };
  const size_t nt = std::min<size_t>(k, (size_t)std::max(1, threads));
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  if (bytes_read) *bytes_read = 0;
  for (size_t f = 0; f < k; ++f) {
    if (!ok[f]) return err = errs[f], false;
    if (bytes_read) *bytes_read += bytes[f];
  }
  return true;
}

}  // namespace tbh
