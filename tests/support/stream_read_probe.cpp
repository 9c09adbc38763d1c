// stream_read_probe — tbh::StreamReader (tiebrush_amd/csrc/host/stream_read.h) driven on its own for tests/test_stream_read_cpu.py, which
// builds it with the host sources, once as it is and once under the address and undefined-behaviour sanitizers:
//   stream_read_probe FILE.bam BYTES   one line per batch (member range, first_uoff, the whole records and the tail by the host codec),
//                                      as `tbh_tool batches` prints them; status 1 and the reader's message for a file it refuses
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../tiebrush_amd/csrc/host/stream_read.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  tbh::StreamReader rd;
  std::string err;
  if (!rd.open(argv[1], strtoull(argv[2], nullptr, 10), err)) {
    fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  printf("header n_targets=%d\n", rd.header().n_targets);
  tbh::StreamBatch b;
  unsigned long long rec = 0, k = 0;
  while (rd.next(b, err)) {
    uint64_t n = 0, tail = 0;
    if (!tbh::stream_host_tail(b, &n, &tail, err) || !rd.advance(b, tail, err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
    printf("batch %llu members=%llu..%llu first_uoff=%u records=%llu..%llu tail=%llu last=%d\n", k++, (unsigned long long)b.first_member,
           (unsigned long long)(b.first_member + b.csize.size()), b.first_uoff, rec, rec + (unsigned long long)n, (unsigned long long)tail, (int)b.last);
    rec += n;
  }
  if (!err.empty()) {
    fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  printf("end records=%llu members=%llu bytes_read=%llu reinflated=%llu\n", rec, (unsigned long long)rd.members(), (unsigned long long)rd.bytes_read(),
         (unsigned long long)rd.reinflated());
  return 0;
}
