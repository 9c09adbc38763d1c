// bai.h — the BAM index (BAI, SAM specification 5.2; or CSI for references beyond 2^29) of the output, built while it is written
// (`tiebrush --index` / `--csi`).
// What `samtools index` (htslib hts_idx_push / hts_idx_finish) makes of a second pass over the file.  Three pieces:
//   the host builder   the index part of a run of records from (tid, beg, end, vbeg) — what tbk_bam_encode_indexed returns for a run
//                      the device encoded, for the runs the host writer deflates (and for `tbh_tool bai`)
//   the combiner       parts in file order, each shifted by its run's file offset -> bins, linear index, counts
//   the file writer
// The contract per record: beg = pos, end = pos + the CIGAR's reference length (M D N = X; pos + 1 when 0), bin = reg2bin(beg, end),
// vbeg = member offset << 16 | offset in the member's payload, vend = the next record's vbeg.
// CSI (min_shift 14): the same with reg2bin(beg, end, depth), depth from the longest reference; a bin carries loff = the linear table's
// entry of its first window in place of the table, and the meta bin (8^(depth+1) - 1) / 7 + 1 stands where the BAI's pseudo-bin does.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

namespace tbh {

struct BaiRec {
  int32_t tid, beg;
  int64_t end;    // (pos = 2^31 - 1 with 1M ends on 2^31)
  uint64_t vbeg;  // bai_member_voffsets: the record's payload offset in the run on the way in
};
struct BaiChunk {  // (the layout of tbk_ix_chunk)
  int32_t tid;
  uint32_t bin;
  uint64_t beg, end;
};
struct BaiRef {  // (the layout of tbk_ix_ref)
  int32_t tid;
  uint32_t reserved;
  uint64_t n_records, first, last;
};
struct BaiPart {
  std::vector<BaiChunk> chunks;  // runs of equal (tid, bin), sorted by (tid, bin, beg), neighbours merged when earlier.end >> 16 >= later.beg >> 16
  uint64_t lin_first = 0;        // flat window of lin[0]: (windows of the references before tid) + window
  std::vector<uint64_t> lin;     // smallest vbeg of the records with end > window << 14; UINT64_MAX: none
  std::vector<BaiRef> refs;
};

constexpr uint64_t kBaiMaxRef = 1ull << 29;  // the longest reference a BAI addresses

constexpr int kBaiDepth = 5;                 // the BAI's binning: reg2bin(beg, end, 14, 5)
constexpr int kCsiMaxDepth = 6;              // 2^(14 + 3 * 6) covers every BAM length (< 2^31)

uint32_t bai_reg2bin(int64_t beg, int64_t end, int depth = kBaiDepth);
// the smallest depth whose bins cover max_len + 256 (the rule of htslib's index builder, as far as it is known here; any covering depth
// is a valid CSI: readers take it from the file)
int csi_depth(uint64_t max_len);
// tid / beg / end of a raw record (WITHOUT its block_size field); false when it is cut short
bool bai_rec_span(const uint8_t* rec, size_t len, int32_t* tid, int32_t* beg, int64_t* end);
// payload offsets -> virtual offsets for records (ascending offsets) inside the run of whole BGZF members z[0, zn): a record belongs to
// the member that holds its first byte
bool bai_member_voffsets(const uint8_t* z, size_t zn, std::vector<BaiRec>& recs, std::string& err);
// the host builder; vend_last = where the record behind the run starts.  false: a record the index cannot hold (err says which).
// depth: the binning's (a record may end at 2^(14 + 3 * depth) and no further)
bool bai_build_part(const BaiRec* recs, size_t n, uint64_t vend_last, const std::vector<uint32_t>& ref_len, BaiPart& out, std::string& err, int depth = kBaiDepth);

class BaiIndex {
 public:
  // false (err names the contig) when a reference is longer than 2^29
  bool init(const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::string& err);
  // CSI mode: any header (the depth follows the longest reference)
  bool init_csi(const std::vector<std::string>& names, const std::vector<uint32_t>& lens, std::string& err);
  bool active() const { return active_; }
  bool csi() const { return csi_; }
  int depth() const { return depth_; }                                // of the binning the parts must come with
  uint32_t ix_format() const { return csi_ ? (uint32_t)depth_ + 1 : 0u; }  // tbk_ix_opts.reserved
  const std::vector<uint32_t>& ref_len() const { return len_; }
  // parts in FILE order; file_base = the file offset of the part's first member
  void add(uint64_t file_base, const BaiChunk* chunks, size_t n_chunks, uint64_t lin_first, const uint64_t* lin, size_t n_lin, const BaiRef* refs, size_t n_refs);
  void add(uint64_t file_base, const BaiPart& p) { add(file_base, p.chunks.data(), p.chunks.size(), p.lin_first, p.lin.data(), p.lin.size(), p.refs.data(), p.refs.size()); }
  void serialize(std::vector<uint8_t>& out) const;  // BAI, or the CSI's bytes before BGZF compression
  // written beside its final name and renamed when complete: no half-written index is left behind (a CSI: BGZF members and the EOF member)
  bool write(const std::string& path, std::string& err) const;
  // The index of a BGZF text track (tabix): the same bins, chunks, windows and pseudo / meta bins behind tabix's header
  // block {format 0x10000 (UCSC: 0-based, half-open), col_seq 1, col_beg 2, col_end 3, meta '#', skip, l_nm, names}.  The references
  // are renumbered to those that have rows, in file order (what `tabix -l` lists).  "TBI\1" n_ref header bodies n_no_coor, or in CSI
  // mode the CSI with the header block as its aux field (l_aux = 28 + l_nm).  The bytes before BGZF compression.
  void serialize_tabix(std::vector<uint8_t>& out, const std::vector<std::string>& names, int32_t skip) const;
  // BGZF members and the EOF member by the host codec, written beside the final name and renamed when complete
  bool write_tabix(const std::string& path, const std::vector<std::string>& names, int32_t skip, std::string& err) const;

 private:
  struct Ref {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> lin;
    uint64_t n = 0, first = ~0ull, last = 0;
  };
  void set_refs(const std::vector<uint32_t>& lens);
  void serialize_csi(std::vector<uint8_t>& out) const;
  void put_ref_bai(std::vector<uint8_t>& out, const Ref& r) const;  // a reference's body with records: bins, pseudo-bin, windows
  void put_ref_csi(std::vector<uint8_t>& out, const Ref& r) const;  // the same for a CSI: a loff per bin, the meta bin
  bool active_ = false, csi_ = false;
  int depth_ = kBaiDepth;
  std::vector<uint32_t> len_;
  std::vector<uint64_t> base_;  // [n_ref + 1] flat window of every reference's window 0
  std::vector<Ref> ref_;
};

// `tbh_tool bai` / `tbh_tool csi`, tbh_bai_index_file / tbh_csi_index_file: the index of an existing BAM by the host builder alone
bool bai_index_file(const std::string& bam_path, const std::string& bai_path, std::string& err, bool csi = false);

}  // namespace tbh
