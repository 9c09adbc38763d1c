// bai_read.h — the reader of the indexes bai.h writes (BAI, SAM specification 5.2; CSI v1), the region query behind `tiecov -r`, and
// the region parser.  The reference reads no index at all (it has no region option; tiecov.cpp walks the whole file
// through GSamReader::next), so nothing here replaces a reference interface: the rules are the SAM specification's and samtools' own
// region syntax.
//   query      bins of reg2bins(beg, end) minus the pseudo / meta bin -> chunks that end behind min_off -> sorted by beg -> neighbours
//              that overlap, touch, or end and begin in the same BGZF member merged.  After the merge no file byte is in two chunks: a
//              parent-bin record between two runs of a leaf bin lies INSIDE the leaf bin's merged chunk (§4d "same block" rule) and
//              would otherwise be read twice.
//   min_off    BAI: lin[beg >> 14], the last entry when the window lies beyond the table (0 for an empty table);
//              CSI: the loff of the leaf bin that holds beg, or of its nearest present ancestor (0: none)
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "bai.h"
#include "bam.h"

namespace tbh {

struct IdxChunk {
  uint64_t beg, end;  // virtual offsets: member offset << 16 | offset in the member's payload
};

// A region table U: R intervals [beg, end) on tid, 0-based half-open.  Normalised: sorted by (tid, beg), disjoint,
// non-empty and non-adjacent (intervals that overlap or abut are one).
struct RegionTable {
  std::vector<int32_t> tid;
  std::vector<int64_t> beg, end;
  size_t n() const { return tid.size(); }
  void add(int32_t t, int64_t b, int64_t e) { tid.push_back(t), beg.push_back(b), end.push_back(e); }
  bool normalised() const;
};

class RegionIndex {
 public:
  // the format comes from the magic: "BAI\1", or a BGZF file whose payload starts with "CSI\1"
  bool load(const std::string& path, std::string& err);
  bool parse(const std::vector<uint8_t>& file_bytes, std::string& err);
  bool csi() const { return csi_; }
  int min_shift() const { return min_shift_; }
  int depth() const { return depth_; }
  size_t n_ref() const { return refs_.size(); }
  // the chunks a reader of [beg, end) on tid has to read: sorted, disjoint, merged (see above); beg < end, both >= 0
  void query(int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& out) const;
  // the same for every interval of a region table: the union of the intervals' chunk lists, sorted and merged by the
  // same rule over the whole set, so that no file byte is in two chunks; for a table of one it is query's result
  void query_regions(const RegionTable& U, std::vector<IdxChunk>& out) const;

 private:
  struct Bin {
    uint32_t bin;
    uint64_t loff;
    std::vector<IdxChunk> chunks;
  };
  struct Ref {
    std::vector<Bin> bins;  // ascending bin number (sorted after parsing), pseudo / meta bin dropped
    std::vector<uint64_t> lin;
  };
  const Bin* find(const Ref& r, uint32_t bin) const;
  void collect(int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& all) const;  // the chunks of one interval, neither sorted nor merged
  static void merge(std::vector<IdxChunk>& all, std::vector<IdxChunk>& out);
  bool csi_ = false;
  int min_shift_ = 14, depth_ = 5;
  std::vector<Ref> refs_;
};

// IN.bam.csi, IN.bam.bai, then IN.bai (IN.bam with its last extension replaced): the first that exists; `explicit_path` (not empty)
// is taken as it is.  false: err names the paths tried.
bool find_index(const std::string& bam_path, const std::string& explicit_path, std::string& found, std::string& err);

// NAME | NAME:BEG | NAME:BEG-END, 1-based inclusive, commas allowed in the numbers; the whole string is tried as a name first (a name
// may hold ':').  Out: tid and the 0-based half-open [beg, end), END cut to the reference's length.
bool parse_region(const BamHeader& hdr, const std::string& region, int32_t* tid, int64_t* beg, int64_t* end, std::string& err);

// BED text (`chrom start end` separated by tabs or spaces, 0-based half-open; further columns ignored; blank lines and lines beginning
// with '#', "track" or "browser" skipped; a trailing '\r' tolerated) -> the normalised table: an end beyond the reference cut to its
// length, empty intervals dropped, the rest sorted by (tid, beg) and merged where they overlap or abut.  false, with the line number in
// err: fewer than three fields, a start or end that is not a non-negative integer, start > end, a chrom the header does not list;
// (without a line number) a text that yields no region at all.  `what` names the text in the messages (the file's path).
bool regions_from_bed(const BamHeader& hdr, const std::string& text, const std::string& what, RegionTable& U, std::string& err);
bool regions_from_bed_file(const BamHeader& hdr, const std::string& bed_path, RegionTable& U, std::string& err);

// The features of `--features BED --summary OUT`: one per BED line, in the file's order — nothing is merged, sorted or
// dropped, so features may overlap, nest and repeat.  line[i] is the feature's line in the text (1-based).
struct FeatureTable {
  std::vector<int32_t> tid;
  std::vector<int64_t> beg, end;
  std::vector<uint8_t> strand;  // '+', '-', '.'
  std::vector<std::string> name;
  std::vector<uint64_t> line;
  size_t n() const { return tid.size(); }
};
// BED text as regions_from_bed reads it (separators, skipped lines, '\r'), columns 1-3 required, 4 the name (default "."), 5 ignored, 6 the
// strand (default '.').  An end beyond the reference is cut to its length.  false, with the line number in err: what regions_from_bed
// refuses, a strand other than + - ., a feature that is empty after the cut; (without a line number) a text without a feature.
bool features_from_bed(const BamHeader& hdr, const std::string& text, const std::string& what, FeatureTable& F, std::string& err);
bool features_from_bed_file(const BamHeader& hdr, const std::string& bed_path, FeatureTable& F, std::string& err);
// true when every feature lies wholly inside one interval of the normalised table U; false: err names the first one's line that does not
bool features_inside(const FeatureTable& F, const RegionTable& U, const std::string& what, std::string& err);

// The annotation of `--gtf FILE --transcripts OUT`: transcripts as runs of exons, the introns implied between them.
// Transcripts are numbered by the first appearance of their transcript_id among the file's exon lines; a transcript's exons are sorted
// by start whatever their order in the file.  tx_off is CSR into ex_beg / ex_end (0-based half-open); line[t] is the line of the
// transcript's first exon line in the text (1-based).
struct TranscriptTable {
  std::vector<uint32_t> tx_off{0};
  std::vector<int32_t> tid;
  std::vector<uint8_t> strand;  // '+', '-', '.'
  std::vector<uint64_t> line;
  std::vector<std::string> id, gene;  // transcript_id, gene_id (default ".")
  std::vector<int64_t> ex_beg, ex_end;
  size_t n_tx() const { return tid.size(); }
  size_t n_exon() const { return ex_beg.size(); }
};
// GTF text: nine tab-separated columns; a line whose first non-blank character is '#' and a blank line are skipped, a trailing '\r' is
// dropped.  Only lines whose column 3 is exactly `exon` are read (the others without a look at their other columns): columns 4 and 5 are
// 1-based inclusive, column 7 the strand, column 9 `key value;` pairs with the value quoted (a ';' inside the quotes belongs to it) or
// bare; transcript_id is required, gene_id optional.  false, with the line number in err: fewer than nine columns, a coordinate that is
// not a number, start < 1, end < start, an end beyond the reference (an exon is not cut), an unknown chrom, a strand other than + - .,
// no transcript_id, a transcript on two chroms or two strands, two exons of a transcript that overlap or abut; (without a line number)
// a text without an exon line.  GFF3 is not read.
bool transcripts_from_gtf(const BamHeader& hdr, const std::string& text, const std::string& what, TranscriptTable& X, std::string& err);
bool transcripts_from_gtf_file(const BamHeader& hdr, const std::string& gtf_path, TranscriptTable& X, std::string& err);
// the transcripts' spans [first exon's begin, last exon's end) as features (name: the transcript's id, line: its first exon line's)
FeatureTable transcript_spans(const TranscriptTable& X);

// One merged chunk's bytes: the whole BGZF members from the chunk's first member on; the records are the inflated bytes from first_uoff
// in the first member up to last_uoff in the last one (0: the last member read is whole, the chunk ends where it ends).
struct RegionSpan {
  std::vector<uint8_t> z;
  uint32_t first_uoff = 0, last_uoff = 0;
};
// pread of the chunks' byte ranges (the last member's size comes from its BSIZE field); a chunk that points outside the file is refused
bool read_spans(const std::string& bam_path, const std::vector<IdxChunk>& chunks, std::vector<RegionSpan>& spans, uint64_t* bytes_read, std::string& err);
// inflate a span on the host and cut it to its record bytes (block_size fields included); false on a malformed span
bool inflate_span(const RegionSpan& s, std::vector<uint8_t>& records, std::string& err);

// the records of a span by the host codec: tid / beg / end by the index's own rule (bai.h) and the virtual offset of each, the span's
// first member lying at file_off
bool span_records(const RegionSpan& s, uint64_t file_off, std::vector<BaiRec>& recs, std::string& err);

// header + index + query in one step (tbh_index_query, `tbh_tool query`, tiecov -r): opens the header of bam_path, finds and loads the
// index, refuses an index whose n_ref is not the header's
bool index_query_file(const std::string& bam_path, const std::string& index_path, int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& out,
                      std::string& err);

// the same for a normalised region table (tbh_index_query_regions, `tbh_tool rquery`, tiecov -R)
bool index_query_regions_file(const std::string& bam_path, const std::string& index_path, const RegionTable& U, std::vector<IdxChunk>& out, std::string& err);

// One input of `tiebrush -r`: its index found (find_index's order), loaded and checked against the file — the index's
// n_ref is file_n_ref, the file's header's — and queried; every chunk checked against the file by read_spans' own conditions, the header
// of the member it ends in read (so that a caller can refuse before it has created anything: what read_spans refuses, this refuses).
// err names the file concerned.
bool region_input_chunks(const std::string& bam_path, int32_t file_n_ref, int32_t tid, int64_t beg, int64_t end, std::vector<IdxChunk>& chunks,
                         std::string& index_path, std::string& err);
// the same for a normalised region table (`tiebrush -R`)
bool regions_input_chunks(const std::string& bam_path, int32_t file_n_ref, const RegionTable& U, std::vector<IdxChunk>& chunks, std::string& index_path,
                          std::string& err);
// The spans of several inputs, read on `threads` threads (file after file on each): spans[f] = read_spans(paths[f], chunks[f]).  false:
// err is the first failing file's.  *bytes_read = the sum over all inputs.
bool read_spans_many(const std::vector<std::string>& paths, const std::vector<std::vector<IdxChunk>>& chunks, int threads,
                     std::vector<std::vector<RegionSpan>>& spans, uint64_t* bytes_read, std::string& err);

}  // namespace tbh
