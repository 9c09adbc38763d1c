// bigwig.cpp — see bigwig.h.  All integers little-endian (the writer's magic says so).
#include "bigwig.h"

#include <math.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>

namespace tbh {

namespace {
constexpr uint32_t BW_MAGIC = 0x888FFC26u, BPT_MAGIC = 0x78CA8C91u, CIR_MAGIC = 0x2468ACE0u;
constexpr uint32_t ITEMS_PER_SLOT = 1024, BLOCK = 256;
constexpr int MAX_ZOOM = 10;

struct Buf {
  std::vector<uint8_t> d;
  void u8(uint32_t v) { d.push_back((uint8_t)v); }
  void u16(uint32_t v) {
    d.push_back((uint8_t)v);
    d.push_back((uint8_t)(v >> 8));
  }
  void u32(uint32_t v) {
    for (int i = 0; i < 4; ++i) d.push_back((uint8_t)(v >> (8 * i)));
  }
  void u64(uint64_t v) {
    for (int i = 0; i < 8; ++i) d.push_back((uint8_t)(v >> (8 * i)));
  }
  void f32(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    u32(b);
  }
  void f64(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    u64(b);
  }
};
bool put(FILE* f, const std::vector<uint8_t>& d) { return d.empty() || fwrite(d.data(), 1, d.size(), f) == d.size(); }
}  // namespace

bool BigWigWriter::open(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::string& err) {
  path_ = path;
  names_ = names;
  lens_ = lens;
  f_ = fopen(path.c_str(), "wb");
  if (!f_) {
    err = "cannot create " + path;
    return false;
  }
  return true;
}

void BigWigWriter::add(uint32_t chrom, uint32_t start, uint32_t end, float value) { items_.push_back(Item{chrom, start, end, value}); }

// one compressed section; remembers its place for the index
bool BigWigWriter::write_sections(const std::vector<uint8_t>& payload, uint32_t chrom, uint32_t start, uint32_t end, std::vector<Block>& blocks) {
  uLongf clen = compressBound((uLong)payload.size());
  std::vector<uint8_t> z(clen);
  if (compress2(z.data(), &clen, payload.data(), (uLong)payload.size(), Z_DEFAULT_COMPRESSION) != Z_OK) return false;
  const uint64_t off = (uint64_t)ftello(f_);
  if (fwrite(z.data(), 1, clen, f_) != clen) return false;
  blocks.push_back(Block{chrom, start, end, off, (uint64_t)clen});
  if (payload.size() > max_uncompressed_) max_uncompressed_ = (uint32_t)payload.size();
  return true;
}

// R-tree over the sections, bottom-up: leaves of up to BLOCK sections, parents of up to BLOCK children; written root first
bool BigWigWriter::write_index(const std::vector<Block>& blocks, uint64_t* index_off) {
  struct Node {
    uint32_t c0, s0, c1, e1;  // bounding range: (start chrom, start base) .. (end chrom, end base)
    size_t first, count;      // children (index into the level below, or into blocks for leaves)
    uint64_t off = 0;
  };
  auto bound = [](Node& n, uint32_t c0, uint32_t s0, uint32_t c1, uint32_t e1, bool first) {
    if (first) {
      n.c0 = c0;
      n.s0 = s0;
      n.c1 = c1;
      n.e1 = e1;
      return;
    }
    if (c0 < n.c0 || (c0 == n.c0 && s0 < n.s0)) {
      n.c0 = c0;
      n.s0 = s0;
    }
    if (c1 > n.c1 || (c1 == n.c1 && e1 > n.e1)) {
      n.c1 = c1;
      n.e1 = e1;
    }
  };
  std::vector<std::vector<Node>> levels;  // levels[0] = leaves
  {
    std::vector<Node> leaves;
    for (size_t i = 0; i < blocks.size(); i += BLOCK) {
      Node n{};
      n.first = i;
      n.count = std::min<size_t>(BLOCK, blocks.size() - i);
      for (size_t j = 0; j < n.count; ++j) bound(n, blocks[i + j].chrom, blocks[i + j].start, blocks[i + j].chrom, blocks[i + j].end, j == 0);
      leaves.push_back(n);
    }
    if (leaves.empty()) {
      Node n{};
      leaves.push_back(n);
    }
    levels.push_back(leaves);
  }
  while (levels.back().size() > 1) {
    const std::vector<Node>& below = levels.back();
    std::vector<Node> up;
    for (size_t i = 0; i < below.size(); i += BLOCK) {
      Node n{};
      n.first = i;
      n.count = std::min<size_t>(BLOCK, below.size() - i);
      for (size_t j = 0; j < n.count; ++j) bound(n, below[i + j].c0, below[i + j].s0, below[i + j].c1, below[i + j].e1, j == 0);
      up.push_back(n);
    }
    levels.push_back(up);
  }
  *index_off = (uint64_t)ftello(f_);
  const Node& root = levels.back()[0];
  // node offsets: root first, then each level below in order
  uint64_t off = *index_off + 48;
  for (size_t L = levels.size(); L-- > 0;) {
    for (Node& n : levels[L]) {
      n.off = off;
      off += 4 + (uint64_t)n.count * (L == 0 ? 32 : 24);
    }
  }
  Buf h;
  h.u32(CIR_MAGIC);
  h.u32(BLOCK);
  h.u64(blocks.size());
  h.u32(root.c0);
  h.u32(root.s0);
  h.u32(root.c1);
  h.u32(root.e1);
  h.u64(*index_off);  // endFileOffset: where the indexed data ends (the index follows it)
  h.u32(ITEMS_PER_SLOT);
  h.u32(0);
  if (!put(f_, h.d)) return false;
  for (size_t L = levels.size(); L-- > 0;) {
    for (const Node& n : levels[L]) {
      Buf b;
      b.u8(L == 0 ? 1 : 0);
      b.u8(0);
      b.u16((uint32_t)n.count);
      for (size_t j = 0; j < n.count; ++j) {
        if (L == 0) {
          const Block& k = blocks[n.first + j];
          b.u32(k.chrom);
          b.u32(k.start);
          b.u32(k.chrom);
          b.u32(k.end);
          b.u64(k.off);
          b.u64(k.size);
        } else {
          const Node& c = levels[L - 1][n.first + j];
          b.u32(c.c0);
          b.u32(c.s0);
          b.u32(c.c1);
          b.u32(c.e1);
          b.u64(c.off);
        }
      }
      if (!put(f_, b.d)) return false;
    }
  }
  return true;
}


bool BigWigWriter::fail(std::string& err, const char* what) {
  err = std::string(what) + " (" + path_ + ")";
  if (f_) fclose(f_);
  f_ = nullptr;
  return false;
}

bool BigWigWriter::restart(std::string& err) {
  if (f_) fclose(f_);
  f_ = fopen(path_.c_str(), "wb");
  max_uncompressed_ = 0;
  if (!f_) {
    err = "cannot create " + path_;
    return false;
  }
  return true;
}

// the 40-byte total summary: one pass over the rows, double sums in row order
BigWigWriter::Summary BigWigWriter::summarise() const {
  Summary s;
  for (size_t i = 0; i < items_.size(); ++i) {
    const Item& it = items_[i];
    const double w = (double)(it.end - it.start), v = (double)it.val;
    s.covered += it.end - it.start;
    if (i == 0 || v < s.vmin) s.vmin = v;
    if (i == 0 || v > s.vmax) s.vmax = v;
    s.vsum += v * w;
    s.vsq += v * v * w;
  }
  return s;
}

// ---- the layout: everything of the file but the sections' bytes.  begin(nz), then per level begin_level / the sections / end_level,
// then finish.  Both section producers write through it, so the two kinds of file differ in their compressed bytes alone.
class BigWigWriter::Layout {
 public:
  explicit Layout(BigWigWriter& w) : w_(w), f_(w.f_) {}
  // fixed part (rewritten by finish with the offsets) and the chromosome tree
  bool begin(uint32_t nz) {
    nz_ = nz;
    zdata_.assign(nz, 0);
    zindex_.assign(nz, 0);
    summary_off_ = 64 + 24ull * nz;
    tree_off_ = summary_off_ + 40;
    {
      std::vector<uint8_t> zero((size_t)tree_off_, 0);
      if (!put(f_, zero)) return false;
    }
    const std::vector<std::string>& names_ = w_.names_;
    const std::vector<uint32_t>& lens_ = w_.lens_;
    uint32_t key = 1;
    for (auto& n : names_) key = std::max<uint32_t>(key, (uint32_t)n.size());
    // leaves of up to BLOCK chromosomes (sorted by name, as a B+ tree needs), parents of up to BLOCK children; every node is
    // padded to BLOCK items so that the offsets are known before anything is written
    std::vector<uint32_t> order(names_.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names_[a] < names_[b]; });
    std::vector<size_t> level_nodes;  // nodes per level, leaves first
    size_t cnt = std::max<size_t>(1, (order.size() + BLOCK - 1) / BLOCK);
    level_nodes.push_back(cnt);
    while (cnt > 1) {
      cnt = (cnt + BLOCK - 1) / BLOCK;
      level_nodes.push_back(cnt);
    }
    const uint64_t node_bytes = 4 + (uint64_t)BLOCK * (key + 8);
    std::vector<uint64_t> level_off(level_nodes.size());
    uint64_t off = tree_off_ + 32;
    for (size_t L = level_nodes.size(); L-- > 0;) {
      level_off[L] = off;
      off += level_nodes[L] * node_bytes;
    }
    Buf b;
    b.u32(BPT_MAGIC);
    b.u32(BLOCK);
    b.u32(key);
    b.u32(8);
    b.u64(order.size());
    b.u64(0);
    auto put_key = [&](const std::string& s) {
      for (uint32_t i = 0; i < key; ++i) b.u8(i < s.size() ? (uint8_t)s[i] : 0);
    };
    // first key under node j of level L
    auto first_key = [&](size_t L, size_t j) -> const std::string& {
      size_t span = 1;
      for (size_t l = 0; l < L; ++l) span *= BLOCK;
      return names_[order[std::min(order.size() - 1, j * span * BLOCK)]];
    };
    for (size_t L = level_nodes.size(); L-- > 0;) {
      for (size_t j = 0; j < level_nodes[L]; ++j) {
        const size_t below = L == 0 ? order.size() : level_nodes[L - 1];
        const size_t first = j * BLOCK, n = below > first ? std::min<size_t>(BLOCK, below - first) : 0;
        b.u8(L == 0 ? 1 : 0);
        b.u8(0);
        b.u16((uint32_t)n);
        for (size_t i = 0; i < BLOCK; ++i) {
          if (i < n && L == 0) {
            const uint32_t id = order[first + i];
            put_key(names_[id]);
            b.u32(id);
            b.u32(lens_[id]);
          } else if (i < n) {
            put_key(first_key(L - 1, first + i));
            b.u64(level_off[L - 1] + (first + i) * node_bytes);
          } else {
            for (uint32_t z = 0; z < key + 8; ++z) b.u8(0);
          }
        }
      }
    }
    return put(f_, b.d);
  }
  // level 0: the data's section count (patched by finish); a zoom level: its record count.  The sections follow.
  bool begin_level(uint32_t L, uint64_t n_items) {
    blocks.clear();
    Buf c;
    if (L == 0) {
      data_off_ = (uint64_t)ftello(f_);
      c.u64(0);
    } else {
      zdata_[L - 1] = (uint64_t)ftello(f_);
      c.u32((uint32_t)n_items);
    }
    return put(f_, c.d);
  }
  // the R-tree over the level's sections
  bool end_level(uint32_t L) {
    if (L == 0) {
      n_data_sections_ = blocks.size();
      return w_.write_index(blocks, &index_off_);
    }
    return w_.write_index(blocks, &zindex_[L - 1]);
  }
  // trailer; header, zoom headers, summary, section count
  bool finish(const std::vector<uint32_t>& reductions, const Summary& sm) {
    {
      Buf m;
      m.u32(BW_MAGIC);  // the file ends with the magic again
      if (!put(f_, m.d)) return false;
    }
    Buf h;
    h.u32(BW_MAGIC);
    h.u16(4);
    h.u16(nz_);
    h.u64(tree_off_);
    h.u64(data_off_);
    h.u64(index_off_);
    h.u16(0);
    h.u16(0);
    h.u64(0);
    h.u64(summary_off_);
    h.u32(w_.max_uncompressed_);
    h.u64(0);
    for (uint32_t z = 0; z < nz_; ++z) {
      h.u32(reductions[z]);
      h.u32(0);
      h.u64(zdata_[z]);
      h.u64(zindex_[z]);
    }
    h.u64(sm.covered);
    h.f64(sm.vmin);
    h.f64(sm.vmax);
    h.f64(sm.vsum);
    h.f64(sm.vsq);
    if (fseeko(f_, 0, SEEK_SET) != 0 || !put(f_, h.d)) return false;
    Buf c;
    c.u64(n_data_sections_);
    return fseeko(f_, (off_t)data_off_, SEEK_SET) == 0 && put(f_, c.d);
  }
  std::vector<Block> blocks;  // of the level being written

 private:
  BigWigWriter& w_;
  FILE* f_;
  uint32_t nz_ = 0;
  uint64_t summary_off_ = 0, tree_off_ = 0, data_off_ = 0, index_off_ = 0, n_data_sections_ = 0;
  std::vector<uint64_t> zdata_, zindex_;
};

// the writer's own section producer: zoom plan and records on this core, one compress2 call per section
bool BigWigWriter::close(std::string& err) {
  if (!f_) return fail(err, "bigWig file is not open");
  const Summary sm = summarise();
  // ---- zoom plan: reductions of 4x from a first level a few times the mean interval, while a level still has many records
  struct ZRec {
    uint32_t chrom, start, end, valid;
    float mn, mx, sum, sq;
  };
  std::vector<uint32_t> reductions;
  std::vector<std::vector<ZRec>> zoom;
  if (!items_.empty()) {
    uint64_t red = std::max<uint64_t>(32, 4 * (sm.covered / items_.size() + 1));
    for (int z = 0; z < MAX_ZOOM && red < (1ull << 31); ++z, red *= 4) {
      std::vector<ZRec> recs;
      for (const Item& it : items_) {  // bins aligned to multiples of the reduction; an interval feeds every bin it overlaps
        for (uint64_t b = it.start / red; b * red < it.end; ++b) {
          const uint32_t bs = (uint32_t)(b * red), be = (uint32_t)std::min<uint64_t>((b + 1) * red, UINT32_MAX);
          const uint32_t lo = std::max(bs, it.start), hi = std::min(be, it.end);
          if (recs.empty() || recs.back().chrom != it.chrom || recs.back().start != bs) {
            const uint32_t clen = it.chrom < lens_.size() ? lens_[it.chrom] : be;
            recs.push_back(ZRec{it.chrom, bs, std::min(be, std::max(clen, hi)), 0, it.val, it.val, 0.f, 0.f});
          }
          ZRec& r = recs.back();
          const float w = (float)(hi - lo);
          r.valid += hi - lo;
          r.mn = std::min(r.mn, it.val);
          r.mx = std::max(r.mx, it.val);
          r.sum += it.val * w;
          r.sq += it.val * it.val * w;
        }
      }
      if (z > 0 && recs.size() * 2 > zoom.back().size()) break;  // no longer shrinking
      reductions.push_back((uint32_t)red);
      zoom.push_back(std::move(recs));
      if (zoom.back().size() < 1000) break;
    }
  }
  const uint32_t nz = (uint32_t)zoom.size();
  Layout lay(*this);
  if (!lay.begin(nz)) return fail(err, "write failed");
  // ---- data sections
  if (!lay.begin_level(0, items_.size())) return fail(err, "write failed");
  {
    size_t i = 0;
    while (i < items_.size()) {
      size_t j = i;
      while (j < items_.size() && j - i < ITEMS_PER_SLOT && items_[j].chrom == items_[i].chrom) ++j;
      Buf s;
      s.u32(items_[i].chrom);
      s.u32(items_[i].start);
      s.u32(items_[j - 1].end);
      s.u32(0);  // itemStep
      s.u32(0);  // itemSpan
      s.u8(1);   // bedGraph
      s.u8(0);
      s.u16((uint32_t)(j - i));
      for (size_t q = i; q < j; ++q) {
        s.u32(items_[q].start);
        s.u32(items_[q].end);
        s.f32(items_[q].val);
      }
      if (!write_sections(s.d, items_[i].chrom, items_[i].start, items_[j - 1].end, lay.blocks)) return fail(err, "write failed");
      i = j;
    }
  }
  if (!lay.end_level(0)) return fail(err, "write failed");
  // ---- zoom levels
  for (uint32_t z = 0; z < nz; ++z) {
    if (!lay.begin_level(1 + z, zoom[z].size())) return fail(err, "write failed");
    size_t i = 0;
    while (i < zoom[z].size()) {
      size_t j = i;
      while (j < zoom[z].size() && j - i < ITEMS_PER_SLOT && zoom[z][j].chrom == zoom[z][i].chrom) ++j;
      Buf s;
      for (size_t q = i; q < j; ++q) {
        const ZRec& r = zoom[z][q];
        s.u32(r.chrom);
        s.u32(r.start);
        s.u32(r.end);
        s.u32(r.valid);
        s.f32(r.mn);
        s.f32(r.mx);
        s.f32(r.sum);
        s.f32(r.sq);
      }
      if (!write_sections(s.d, zoom[z][i].chrom, zoom[z][i].start, zoom[z][j - 1].end, lay.blocks)) return fail(err, "write failed");
      i = j;
    }
    if (!lay.end_level(1 + z)) return fail(err, "write failed");
  }
  if (!lay.finish(reductions, sm)) return fail(err, "write failed");
  if (fclose(f_) != 0) {
    f_ = nullptr;
    return fail(err, "write failed");
  }
  f_ = nullptr;
  return true;
}

// sections from a feed: the same layout calls, driven by the producer's
bool BigWigWriter::close_with(const std::function<bool(BigWigFeed&)>& produce, std::string& err) {
  if (!f_) return fail(err, "bigWig file is not open");
  const Summary sm = summarise();
  struct Feed : BigWigFeed {
    BigWigWriter& w;
    Layout lay;
    std::vector<uint32_t> reductions;
    std::vector<uint64_t> n_items;
    bool planned = false, io_ok = true;
    int open_level = -1;
    explicit Feed(BigWigWriter& w_) : w(w_), lay(w_) {}
    bool io(bool ok) {
      if (!ok) io_ok = false;
      return ok;
    }
    bool plan(const uint32_t* red, const uint64_t* items, uint32_t nz) override {
      if (planned) return false;
      planned = true;
      reductions.assign(red, red + nz);
      n_items.assign(items, items + 1 + nz);
      return io(lay.begin(nz));
    }
    bool level(uint32_t L, const BigWigSection* s, size_t n, uint32_t max_payload) override {
      if (!planned || (int)L != open_level + 1 || L >= n_items.size()) return false;
      if (open_level >= 0 && !io(lay.end_level((uint32_t)open_level))) return false;
      if (!io(lay.begin_level(L, n_items[L]))) return false;
      open_level = (int)L;
      const uint64_t base = (uint64_t)ftello(w.f_);
      for (size_t i = 0; i < n; ++i) lay.blocks.push_back(Block{s[i].chrom, s[i].start, s[i].end, base + s[i].off, s[i].size});
      if (max_payload > w.max_uncompressed_) w.max_uncompressed_ = max_payload;
      return true;
    }
    bool bytes(const void* p, size_t n) override { return open_level >= 0 && io(n == 0 || fwrite(p, 1, n, w.f_) == n); }
  } feed(*this);
  if (!produce(feed)) {
    err = feed.io_ok ? "the section producer gave up" : "write failed";
    err += " (" + path_ + ")";
    return false;  // (the file stays open: restart() and close() can still write it)
  }
  if (!feed.planned || feed.open_level + 1 != (int)feed.n_items.size()) return fail(err, "the section producer left levels out");
  if (!feed.lay.end_level((uint32_t)feed.open_level) || !feed.lay.finish(feed.reductions, sm)) return fail(err, "write failed");
  if (fclose(f_) != 0) {
    f_ = nullptr;
    return fail(err, "write failed");
  }
  f_ = nullptr;
  return true;
}

}  // namespace tbh
