// stream_read.cpp — see stream_read.h
#include "stream_read.h"

#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "bgzf.h"

namespace tbh {

namespace {
uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The member at z[off, n): 0 = not all of it is there, -1 = not a BGZF member, else its size (BSIZE + 1)
int64_t member_size(const uint8_t* z, size_t off, size_t n) {
  if (off + 18 > n) return 0;
  const uint8_t* c = z + off;
  if (c[0] != 0x1f || c[1] != 0x8b || c[2] != 8 || !(c[3] & 4)) return -1;
  const uint32_t xlen = c[10] | (c[11] << 8);
  if (off + 12 + xlen > n) return 0;
  int64_t bsize = -1;
  for (size_t p = 12; p + 4 <= 12 + (size_t)xlen;) {
    const uint32_t slen = c[p + 2] | (c[p + 3] << 8);
    if (p + 4 + slen > 12 + (size_t)xlen) break;
    if (c[p] == 'B' && c[p + 1] == 'C' && slen == 2) bsize = c[p + 4] | (c[p + 5] << 8);
    p += 4 + slen;
  }
  if (bsize < 0 || (uint64_t)bsize + 1 < 12ull + xlen + 8) return -1;
  if (off + (size_t)bsize + 1 > n) return 0;
  return bsize + 1;
}
}  // namespace

uint64_t StreamBatch::payload() const {
  uint64_t s = 0;
  for (uint32_t v : isize) s += v;
  return s;
}

StreamReader::~StreamReader() {
  if (ahead_.valid()) ahead_.wait();
  if (fd_ >= 0) close(fd_);
}

StreamReader::Stretch StreamReader::read_stretch(uint64_t pos) const {
  Stretch s;
  const size_t want = (size_t)std::min<uint64_t>(std::max<uint64_t>(tile_bytes_, 1), (uint64_t)1 << 32);
  std::vector<uint8_t> buf(want + 65536 + 64);  // (a member is at most 64 KiB: the last one that begins below `want` is whole)
  size_t got = 0;
  while (got < buf.size()) {
    const ssize_t r = pread(fd_, buf.data() + got, buf.size() - got, (off_t)(pos + got));
    if (r < 0) return s.err = path_ + ": read error", s;
    if (r == 0) break;
    got += (size_t)r;
  }
  const bool hit_end = got < buf.size();
  size_t off = 0;
  while (off < got && off < want) {
    const int64_t m = member_size(buf.data(), off, got);
    if (m < 0) return s.err = path_ + ": not a BGZF file (bad member header)", s;
    if (m == 0) {
      if (hit_end) return s.err = path_ + ": truncated file (the last BGZF member is incomplete)", s;
      break;  // (cannot happen below `want`: the buffer reaches 64 KiB beyond it)
    }
    const uint32_t isz = rd32(buf.data() + off + (size_t)m - 4);
    if (isz > 65536) return s.err = path_ + ": not a BGZF file (a member of more than 64 KiB)", s;
    s.csize.push_back((uint32_t)m);
    s.isize.push_back(isz);
    off += (size_t)m;
  }
  s.eof = hit_end && off == got;
  buf.resize(off);
  s.z.swap(buf);
  return s;
}

void StreamReader::start_ahead() {
  if (eof_) return;
  const uint64_t pos = file_pos_;
  ahead_ = std::async(std::launch::async, [this, pos]() { return read_stretch(pos); });
}

bool stream_inflate_member(const uint8_t* m, uint32_t csize, uint32_t isize, uint8_t* out) {
  const uint32_t xlen = m[10] | (m[11] << 8);
  if (csize < 12 + xlen + 8) return false;
  return bgzf_inflate_member(m + 12 + xlen, csize - 12 - xlen - 8, out, isize, rd32(m + csize - 8));
}

bool StreamReader::open(const std::string& path, uint64_t tile_bytes, std::string& err) {
  path_ = path, tile_bytes_ = tile_bytes;
  fd_ = ::open(path.c_str(), O_RDONLY);
  if (fd_ < 0) return err = "cannot open " + path, false;
  // the header: members are taken, stretch after stretch, until it parses; what lies behind it in them opens the first batch
  std::vector<uint8_t> inf;
  size_t rec_begin = 0, parsed_members = 0;
  bool have = false;
  std::string herr = "not a BAM stream";
  while (!have) {
    if (eof_) return err = path + ": " + herr, false;
    Stretch s = read_stretch(file_pos_);
    if (!s.err.empty()) return err = s.err, false;
    file_pos_ += s.z.size(), bytes_read_ += s.z.size(), next_member_ += s.csize.size(), eof_ = s.eof;
    keep_.z.insert(keep_.z.end(), s.z.begin(), s.z.end());
    keep_.csize.insert(keep_.csize.end(), s.csize.begin(), s.csize.end());
    keep_.isize.insert(keep_.isize.end(), s.isize.begin(), s.isize.end());
    size_t zoff = 0;
    for (size_t j = 0; j < parsed_members; ++j) zoff += keep_.csize[j];
    for (; parsed_members < keep_.csize.size() && !have; ++parsed_members) {
      const size_t j = parsed_members, at = inf.size();
      inf.resize(at + keep_.isize[j]);
      if (!stream_inflate_member(keep_.z.data() + zoff, keep_.csize[j], keep_.isize[j], inf.data() + at)) return err = path + ": corrupt BGZF member", false;
      zoff += keep_.csize[j];
      if (inf.size() >= 12 && memcmp(inf.data(), "BAM\1", 4) != 0) return err = path + ": not a BAM stream", false;
      have = inf.size() >= 12 && hdr_.parse(inf, &rec_begin, herr);
    }
  }
  // the member that holds the first record (the first one whose payload reaches beyond rec_begin), and the offset in it
  size_t j = 0, zoff = 0;
  uint64_t cum = 0;
  while (j < keep_.isize.size() && cum + keep_.isize[j] <= rec_begin) cum += keep_.isize[j], zoff += keep_.csize[j], ++j;
  keep_.z.erase(keep_.z.begin(), keep_.z.begin() + (std::ptrdiff_t)zoff);
  keep_.csize.erase(keep_.csize.begin(), keep_.csize.begin() + (std::ptrdiff_t)j);
  keep_.isize.erase(keep_.isize.begin(), keep_.isize.begin() + (std::ptrdiff_t)j);
  keep_.first_member = j;
  keep_.first_uoff = keep_.isize.empty() ? 0u : (uint32_t)(rec_begin - cum);
  start_ahead();
  return true;
}

bool StreamReader::next(StreamBatch& b, std::string& err) {
  err.clear();
  if (done_) return false;
  Stretch s;
  if (ahead_.valid())
    s = ahead_.get();
  else
    s.eof = true;  // (the file's end was seen: nothing more to read)
  if (!s.err.empty()) return err = s.err, false;
  if (keep_.csize.empty() && s.csize.empty()) return done_ = true, false;
  b = std::move(keep_);
  keep_ = StreamBatch();
  if (b.csize.empty()) b.first_member = next_member_, b.first_uoff = 0;
  b.z.insert(b.z.end(), s.z.begin(), s.z.end());
  b.csize.insert(b.csize.end(), s.csize.begin(), s.csize.end());
  b.isize.insert(b.isize.end(), s.isize.begin(), s.isize.end());
  file_pos_ += s.z.size(), bytes_read_ += s.z.size(), next_member_ += s.csize.size();
  eof_ = s.eof;
  b.last = eof_;
  start_ahead();
  return true;
}

bool StreamReader::advance(const StreamBatch& b, uint64_t tail_off, std::string& err) {
  const uint64_t total = b.payload();
  if (tail_off > total || tail_off < b.first_uoff) return err = path_ + ": the decode's tail lies outside its batch", false;
  if (b.last) {
    if (tail_off != total) return err = path_ + ": truncated file (the last record runs past the end)", false;
    done_ = true;
    return true;
  }
  size_t j = 0, zoff = 0;
  uint64_t cum = 0;
  while (j < b.isize.size() && cum + b.isize[j] <= tail_off) cum += b.isize[j], zoff += b.csize[j], ++j;
  keep_ = StreamBatch();
  keep_.first_member = b.first_member + j;
  if (j < b.isize.size()) {  // the tail's member and what follows it go into the next batch again
    keep_.z.assign(b.z.begin() + (std::ptrdiff_t)zoff, b.z.end());
    keep_.csize.assign(b.csize.begin() + (std::ptrdiff_t)j, b.csize.end());
    keep_.isize.assign(b.isize.begin() + (std::ptrdiff_t)j, b.isize.end());
    keep_.first_uoff = (uint32_t)(tail_off - cum);
    reinflated_ += keep_.payload();
  }
  return true;
}

bool stream_host_tail(const StreamBatch& b, uint64_t* n_records, uint64_t* tail_off, std::string& err) {
  std::vector<uint8_t> inf((size_t)b.payload());
  size_t zoff = 0, at = 0;
  for (size_t j = 0; j < b.csize.size(); ++j) {
    if (!stream_inflate_member(b.z.data() + zoff, b.csize[j], b.isize[j], inf.data() + at)) return err = "corrupt BGZF member", false;
    zoff += b.csize[j], at += b.isize[j];
  }
  uint64_t p = b.first_uoff, n = 0;
  while (p + 4 <= inf.size()) {
    const uint32_t bs = rd32(inf.data() + p);
    if (bs < 32) return err = "corrupt BAM record chain (block_size below 32)", false;
    if (p + 4 + (uint64_t)bs > inf.size()) break;
    ++n;
    p += 4 + (uint64_t)bs;
  }
  *n_records = n, *tail_off = p;
  return true;
}

}  // namespace tbh
