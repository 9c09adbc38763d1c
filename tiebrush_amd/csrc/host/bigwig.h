// bigwig.h — bigWig writer for tiecov -W (the reference hands its intervals to libBigWig: tiecov.cpp:243-275, :365-402).
// Written from the bigWig / bbi file format (Kent et al. 2010, supplement): header, zoom headers, total summary, chromosome
// B+ tree, bedGraph-type data sections (zlib-compressed, up to 1024 items, one chromosome each), R-tree index, and zoom levels
// (32-byte summary records with their own R-trees).  Values are float32, as in the reference's bwAddIntervals call.
// libBigWig is not in this image, so byte identity with the reference's files is not claimed: the intervals a reader gets
// back are the bedGraph lines of `tiecov -c` (tests/test_gpu_cli.py reads the file back with an independent parser).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

namespace tbh {

// One compressed section of a level: its R-tree key, and where its zlib stream lies — in the file for the writer's own sections,
// from the level's first byte for a feed's.
struct BigWigSection {
  uint32_t chrom, start, end;
  uint64_t off, size;
};

// What a section producer other than the writer's own compress2 loop hands over (close_with), in this order: plan() once; then for
// every level 0 .. nz, data first, level() followed by that level's bytes() in order.
class BigWigFeed {
 public:
  virtual ~BigWigFeed() {}
  // the zoom plan: reductions[nz]; n_items[1 + nz] = the data rows, then the records of every zoom level
  virtual bool plan(const uint32_t* reductions, const uint64_t* n_items, uint32_t nz) = 0;
  // the sections of level L (offsets from the level's first byte) and the largest uncompressed section among them
  virtual bool level(uint32_t L, const BigWigSection* sections, size_t n, uint32_t max_payload) = 0;
  virtual bool bytes(const void* p, size_t n) = 0;
};

class BigWigWriter {
 public:
  // chromosome names and lengths in id order (the BAM header's @SQ order)
  bool open(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::string& err);
  // intervals in (chromosome id, start) order, half-open, 0-based, non-overlapping
  void add(uint32_t chrom, uint32_t start, uint32_t end, float value);
  // The file: the layout (fixed part, chromosome tree, section count, an R-tree per level, trailer, header, the summary from a loop over
  // the rows) is one piece of code; the sections come from the writer's own producer (zoom plan, zoom records and compress2 on this
  // core) ...
  bool close(std::string& err);
  // ... or from `produce`, which drives a BigWigFeed (the device's sections: tracks.cpp).  When produce returns false nothing of the
  // file is valid; restart() empties it, the rows are kept, and close() can still write it.
  bool close_with(const std::function<bool(BigWigFeed&)>& produce, std::string& err);
  bool restart(std::string& err);
  size_t n_items() const { return items_.size(); }

 private:
  struct Item {
    uint32_t chrom, start, end;
    float val;
  };
  typedef BigWigSection Block;
  struct Summary {
    uint64_t covered = 0;
    double vmin = 0, vmax = 0, vsum = 0, vsq = 0;
  };
  class Layout;
  friend class Layout;
  Summary summarise() const;
  bool fail(std::string& err, const char* what);
  bool write_index(const std::vector<Block>& blocks, uint64_t* index_off);
  bool write_sections(const std::vector<uint8_t>& payload, uint32_t chrom, uint32_t start, uint32_t end, std::vector<Block>& blocks);
  FILE* f_ = nullptr;
  std::string path_;
  std::vector<std::string> names_;
  std::vector<uint32_t> lens_;
  std::vector<Item> items_;
  uint32_t max_uncompressed_ = 0;
};

}  // namespace tbh
