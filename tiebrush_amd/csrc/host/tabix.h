// tabix.h — a text track as FILE.gz (BGZF) with its tabix index FILE.gz.tbi / .csi, written in one pass (`tiecov --tabix`,
// `tiebrush --tabix`, `tbh_tool tabix`).  What `bgzip FILE && tabix -p bed -S 1 FILE.gz` make of the plain track.
// The index is the BAM index of bai.h with the lines as records: beg = start, end = max(end, start + 1), bin = reg2bin(beg, end), a
// line's vbeg = member offset << 16 | offset in the member's payload of its first byte, its vend = the next line's vbeg (the last
// line's: the EOF member's offset << 16).  Two producers feed one writer:
//   the device   tbk_track_bgzf hands over runs of whole members with their index parts (add_run)
//   the host     the formatted lines of a slice, deflated into members of 0xff00 payload bytes by bgzf.h, indexed by bai_build_part
//                (add_text) — `tbh_tool tabix`, TBK_TRACK_HOST_FMT=1, and the command lines' fallback when the device call refuses
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../../../include/tbk.h"
#include "bai.h"

namespace tbh {

class TabixWriter {
 public:
  ~TabixWriter();
  // `path` is the .gz.  Older files of the names this run writes (path, path.tbi, path.csi) are removed first.  The index is a TBI, or
  // a tabix CSI when a reference is longer than 2^29 (its depth by csi_depth).  `head`: the track's header line ("" for none); it is
  // the caller's to hand over with the first run or slice, here it decides the index's `skip` (1 for a "track" line).
  bool open(const std::string& path, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::string& head, std::string& err);
  bool is_open() const { return f_ != nullptr; }
  const std::string& path() const { return path_; }
  const std::string& head() const { return head_; }
  const BaiIndex& index() const { return ix_; }
  uint64_t bytes() const { return off_; }  // of the .gz so far
  uint64_t runs() const { return runs_; }
  uint64_t text_bytes() const { return text_; }  // of the slices add_text took
  // a run of whole members and its index part (offsets relative to the run's first byte), in file order
  bool add_run(const uint8_t* z, size_t n, const BaiChunk* chunks, size_t n_chunks, uint64_t lin_first, const uint64_t* lin, size_t n_lin, const BaiRef* refs,
               size_t n_refs);
  // the host path: a slice of whole lines (the header line first, in the first slice) and per row (tid, beg, end, offset of its line in
  // `text`).  false: a row the index cannot hold or rows out of order (err names the row, counted from 0 over the whole track)
  bool add_text(const char* text, size_t n, std::vector<BaiRec>& recs, std::string& err);
  // the EOF member, then the index under a temporary name, renamed when complete
  bool close(std::string& err);
  void discard();  // a track that failed: the file is closed and removed, no index is written

 private:
  FILE* f_ = nullptr;
  std::string path_, head_;
  std::vector<std::string> names_;
  BaiIndex ix_;
  uint64_t off_ = 0, runs_ = 0, rows_ = 0, text_ = 0;
  int32_t last_tid_ = -1, last_beg_ = 0;
};

// The host path of a whole track: fmt(i, buf, cap) is snprintf-like (tracks.h).  Slices of `slice_rows` rows (0: 2^19; the first
// carries the writer's header line), formatted and deflated on `threads` workers.
bool tabix_host_track(TabixWriter& w, uint32_t n, const int32_t* tid, const int32_t* start, const int32_t* end,
                      const std::function<int(uint32_t, char*, size_t)>& fmt, uint32_t slice_rows, int threads, std::string& err, bool with_head = true);

struct TrackApi;  // tracks.h: the device entry points as a command line has them
// The reference names onto the context, for tbk_format_track and tbk_track_bgzf.  Errors are fatal (GError).
void set_track_names(const TrackApi& api, const std::vector<std::string>& names);
// One track from HOST rows into an open writer, and the writer closed.  TBK_TRACK_HOST_FMT: the host path.  Else the runs are
// api.track_bgzf's, after set_track_names unless *names_set says the run has called it (it does afterwards); a refusal of that call
// before its first run hands the track to the host path (a line on stderr says so).
// Errors are fatal (GError).  TBK_TIMING: a "tabix phase ms" line on stderr.
void write_tabix_track(TabixWriter& w, const tbk_track_rows& rows, const std::vector<std::string>& names, const TrackApi& api, bool* names_set);
// The same without the close, for a track that arrives in several pieces (TrackStream, tracks.h): the rows of one piece as further runs
// (device) or slices (host) behind what the writer has.  with_head: the writer's header line goes in front of these rows — the first
// piece.  true: the device wrote them (*device_text_bytes: their text).  A device refusal before the call's first run hands the piece to
// the host path.  The caller closes the writer.
bool feed_tabix_track(TabixWriter& w, const tbk_track_rows& rows, const std::vector<std::string>& names, const TrackApi& api, bool* names_set, bool with_head,
                      uint64_t* device_text_bytes);

}  // namespace tbh
