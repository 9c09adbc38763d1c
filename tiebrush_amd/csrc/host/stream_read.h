// stream_read.h — a BAM file read sequentially in batches of whole BGZF members: the host side of a streamed decode.
// A batch is handed to tbk_bam_decode_open (or, in `tbh_tool batches`, to the host codec), which says where the whole records end
// (tail_off); advance() turns that into the member that holds the tail and the offset in it, and the next batch STARTS WITH THAT MEMBER
// AGAIN — at most a member or two is inflated twice, nothing inflated is kept here.  A batch that yields no whole record (a record longer
// than the batch) keeps all its members and adds new ones, so the walk always reaches the end of the file.  Host memory holds up to three batches
// of compressed bytes: a helper thread reads the file's next stretch while the caller works on the current batch.
#pragma once
#include <stdint.h>

#include <future>
#include <string>
#include <vector>

#include "bam.h"

namespace tbh {

struct StreamBatch {
  std::vector<uint8_t> z;        // the members' compressed bytes, back to back
  std::vector<uint32_t> csize;   // per member: compressed size (BSIZE + 1)
  std::vector<uint32_t> isize;   // per member: payload size (ISIZE)
  uint64_t first_member = 0;     // index in the file of the batch's first member
  uint32_t first_uoff = 0;       // where the record stream starts in the first member's payload
  bool last = false;             // the file ends behind this batch
  uint64_t payload() const;      // sum of isize
};

class StreamReader {
 public:
  ~StreamReader();
  // Reads and parses the header (whatever members it spans).  tile_bytes: about how many NEW compressed bytes a batch takes (a value
  // below a member's size: one member a batch).  Errors name the file.
  bool open(const std::string& path, uint64_t tile_bytes, std::string& err);
  const BamHeader& header() const { return hdr_; }
  // The next batch.  false with an empty err: the file has been read to its end (after the batch flagged `last` was advanced over).
  bool next(StreamBatch& b, std::string& err);
  // tail_off: what the decode of `b` reported — the offset, from the first member's payload start, of the first byte that no whole
  // record consumed.  false: a tail outside the batch, or records that end behind the end of the file (a truncated file).
  bool advance(const StreamBatch& b, uint64_t tail_off, std::string& err);
  uint64_t bytes_read() const { return bytes_read_; }    // compressed bytes read from the file
  uint64_t reinflated() const { return reinflated_; }    // payload bytes of members that went into more than one batch
  uint64_t members() const { return next_member_; }      // members read so far

 private:
  struct Stretch {  // whole members read from the file in one go
    std::vector<uint8_t> z;
    std::vector<uint32_t> csize, isize;
    bool eof = false;
    std::string err;
  };
  Stretch read_stretch(uint64_t pos) const;
  void start_ahead();
  std::string path_;
  int fd_ = -1;
  uint64_t tile_bytes_ = 0, file_pos_ = 0, next_member_ = 0, bytes_read_ = 0, reinflated_ = 0;
  BamHeader hdr_;
  StreamBatch keep_;          // the members the next batch starts with (from the tail's member on), first_uoff set
  bool eof_ = false, done_ = false;
  std::future<Stretch> ahead_;
};

// One member's payload by the host codec: m.z + offset -> out (isize bytes).  false: a corrupt member
bool stream_inflate_member(const uint8_t* member, uint32_t csize, uint32_t isize, uint8_t* out);
// The whole records of a batch by the host codec: their count and the tail (as tbk_bam_decode_open reports them).  false: a corrupt
// member or a block_size below 32.
bool stream_host_tail(const StreamBatch& b, uint64_t* n_records, uint64_t* tail_off, std::string& err);

}  // namespace tbh
