// tiebrush — drop-in command line of the reference's collapse tool (/root/reference/src/tiebrush.cpp:557-676),
// with the per-record main loop (:570-592) replaced by one call into the MI355X hot path:
//   decode every input into a SoA tile (host: BGZF inflate + record / aux scan on every core, fastload.cpp; inputs larger than
//   memory stream through TInputFiles::next_tile)  ->  tbk_collapse_tile (HIP)  ->  tag + deflate + write (host).
// With -r REGION (no counterpart in the reference) only the chunks that every input's index names for the region are read,
// and they are inflated, decoded and filtered on the device (run_region below).
// libtbk.so (and with it the HIP runtime) is bound with dlopen on a helper thread while the inputs are read (tbk_dl.h).
// There is no CPU implementation of the collapse in this binary: without a usable GPU it exits with an error.
#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <memory>
#include <signal.h>
#include <spawn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <chrono>
#include <time.h>
#include <thread>
#include <vector>

#include "../../../include/tbk.h"
#include "GSam.h"
#include "args.h"
#include "bgzf.h"
#include "devwriter.h"
#include "fastload.h"
#include "tagwrite.h"
#include "bai.h"
#include "bai_read.h"
#include "sam.h"
#include "tbk_dl.h"
#include "tmerge.h"
#include "tracks.h"

extern char** environ;

#define VERSION "0.0.7"

static const char* USAGE =
    "TieBrush v" VERSION " (MI355X build)\n"
    "Collapses identical alignments from several coordinate-sorted BAM files into one BAM.\n"
    "Every output alignment carries: YC (how many alignments it stands for), YX (in how many\n"
    "samples it was seen) and YD (upstream extent of its coverage island, omitted when 0).\n"
    "\n"
    " usage: tiebrush [options] -o OUT.bam IN1.bam [IN2.bam ...]   (or one text file listing the inputs)\n"
    "\n"
    "  -h,--help            print this text and exit\n"
    "  --version            print the version and exit\n"
    "  -o FILE              output BAM (required)\n"
    "  -L,--full            group by CIGAR and MD\n"
    "  -P,--clip            group by CIGAR after removing soft clips\n"
    "  -E,--exon            group by exon coordinates\n"
    "                       (default: group by CIGAR; the three are mutually exclusive)\n"
    "  -S,--keep-supp       keep supplementary alignments\n"
    "  --keep-secondary     keep secondary alignments\n"
    "  -M,--keep-unmap      keep unmapped reads (not available in the GPU build)\n"
    "  -N INT               drop alignments with NH above INT\n"
    "  -Q INT               drop alignments with mapping quality below INT\n"
    "  -F INT               flag bits that must agree (not available in the GPU build)\n"
    "  -A,--collapse-same   do not count the same read of the same sample twice\n"
    "  --store-frac         YC adds 1/NH per alignment (needs --keep-secondary)\n"
    "  -V,--verbose         echo the command line\n"
    "  -r,--region REGION   collapse only the alignments that overlap REGION: NAME, NAME:BEG or NAME:BEG-END (1-based, inclusive,\n"
    "                       commas allowed; one region per run), read through every input's index (IN.bam.csi, IN.bam.bai or IN.bai;\n"
    "                       `tiebrush --index` / `--csi` and `samtools index` write one).  The output is what the same command line\n"
    "                       without -r makes of inputs cut to their records that overlap the region; not with --ranks\n"
    "  -R,--regions-file FILE   the same for several regions in one run: FILE is BED (chrom start end, 0-based half-open; further\n"
    "                       columns ignored); a record that overlaps two of them is kept once; not with -r or --ranks\n"
    "  --ranks N            shard the input files over N GPUs of this node (one process each), one output BAM\n"
    "  --writer WHICH       device (default): the output records are tagged and BGZF-compressed on the GPU; host: by the CPU cores\n"
    "  --cov PREFIX         also write tiecov's coverage track of the output (as tiecov -c; - or stdout: standard output)\n"
    "  --junc PREFIX        also write tiecov's junction track of the output (as tiecov -j)\n"
    "  --samp PREFIX        also write tiecov's sample-count track of the output (as tiecov -s; needs @CO SAMPLE: header lines)\n"
    "  --strand-cov PREFIX  also write the output's coverage per splice strand (as tiecov --strand-cov): PREFIX.plus.bedgraph,\n"
    "                       PREFIX.minus.bedgraph, PREFIX.none.bedgraph; with --bigwig .bigwig, with --tabix .bedgraph.gz and an index each\n"
    "  --bigwig             write the coverage track as PREFIX.bigwig (as tiecov -W; needs --cov)\n"
    "  --bigwig-writer host|device   with --bigwig: the file's sections and zoom levels by this core with zlib (host, the default)\n"
    "                       or by the GPU (device: the same payloads, compressed by the device's deflater)\n"
    "  --tabix              write every text track BGZF-compressed with its tabix index (PREFIX.bedgraph.gz / PREFIX.bed.gz and\n"
    "                       FILE.gz.tbi, or FILE.gz.csi for references longer than 2^29), as tiecov --tabix; with --bigwig the\n"
    "                       coverage stays the bigWig; needs one of --cov / --junc / --samp, not --cov - and not --ranks\n"
    "                       (the tracks are what tiecov writes when it reads OUT.bam; not with --ranks)\n"
    "  --features BED --summary OUT.tsv   also write tiecov's per-feature summary of the output (as tiecov --features --summary: one\n"
    "                       line per line of BED with size, covered bases, sum, mean0, mean and max of the coverage and the junction\n"
    "                       support of the feature taken as an intron); goes with any of the tracks or alone; with -r / -R every\n"
    "                       feature must lie inside one interval of the region; not with --ranks\n"
    "  --thresholds T1,T2,... --depth-summary OUT.tsv   also write tiecov's table of bases at depth of the output (as tiecov\n"
    "                       --depth-summary: per reference and in total length, covered bases, sum, mean0, mean, max and, per\n"
    "                       threshold, the bases covered at depth >= T; 1 to 16 ascending thresholds, none: no ge_ columns); not\n"
    "                       with -r / -R or --ranks\n"
    "  --feature-depth OUT.tsv   with --features BED and --thresholds: per line of BED its size, covered bases and the bases at depth\n"
    "                       >= T (as tiecov --feature-depth); with -r / -R as --summary; not with --ranks\n"
    "  --gtf FILE --transcripts OUT.tsv   also write tiecov's per-transcript support of the output (as tiecov --gtf --transcripts: per\n"
    "                       transcript of the GTF's exon lines its exons' coverage and how many of its introns are junctions of the\n"
    "                       output); goes with any of the tracks or alone; with -r / -R every transcript's span must lie inside one\n"
    "                       interval of the region; not with --ranks\n"
    "  --index             also write the output's BAM index OUT.bam.bai (what samtools index makes of OUT.bam; not with --ranks,\n"
    "                       not when the output goes to standard output)\n"
    "  --csi                also write the output's CSI index OUT.bam.csi (what samtools index -c makes of OUT.bam: for references\n"
    "                       longer than 2^29, which a BAI cannot address; not with --index, --ranks or standard output)\n";

// a buffer that is allocated, not initialised (untouched pages cost nothing), on huge pages when it is large, and not freed at
// the end: these buffers live as long as the process, which ends with _exit — returning gigabytes page by page first only
// delays that.  The contents do not survive a resize (every caller fills the buffer afresh), so a buffer that grows gives its
// old block back first and grows by half at least: the streaming path resizes per tile, and tiles come in any order of size.
template <class T>
struct RawBuf {
  T* p = nullptr;
  size_t cap = 0, len = 0;
  bool borrowed = false;
  // another buffer's pages for a while (a dead array of the input tile: resident already, nothing to fault in)
  void borrow(T* q, size_t n) {
    if (!borrowed) tbh::big_free(p);
    p = q, cap = len = n, borrowed = true;
  }
  void resize(size_t n) {
    if (borrowed) p = nullptr, cap = 0, borrowed = false;
    if (n > cap) {
      const size_t want = cap ? std::max(n, cap + cap / 2) : n;
      tbh::big_free(p);
      p = (T*)tbh::big_alloc(want * sizeof(T));
      if (!p) GError("Error: out of memory\n");
      cap = want;
    }
    len = n;
  }
  T* data() { return p; }
  size_t size() const { return len; }
  T& operator[](size_t i) { return p[i]; }
};

// an input file as the page cache holds it: the device decode uploads it through its own pinned ring (tbk_bam_decode), so a private copy
// made with read() would only be one more pass over gigabytes
struct FileMap {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool map(const std::string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0) {
      close(fd);
      return false;
    }
    n = (size_t)st.st_size;
    if (n) {
      void* q = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
      if (q == MAP_FAILED) {
        close(fd);
        n = 0;
        return false;
      }
      (void)madvise(q, n, MADV_SEQUENTIAL);
      p = (const uint8_t*)q;
    }
    close(fd);
    return true;
  }
  void unmap() {
    if (p) munmap(const_cast<uint8_t*>(p), n);
    p = nullptr, n = 0;
  }
};

using Clock = std::chrono::steady_clock::time_point;
static Clock tnow() { return std::chrono::steady_clock::now(); }
static double tms(Clock a, Clock b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
using RecFn = std::function<tbh::RecView(uint32_t)>;
using PrefetchFn = std::function<void(uint32_t, int)>;

static bool env_set(const char* name) { return getenv(name) != nullptr; }
static long long env_num(const char* name, long long unset) { return getenv(name) ? atoll(getenv(name)) : unset; }

// Every TBK_* variable this file reads, read once at start-up (devwriter.h reads its own tuning and test hooks).
struct Env {
  bool timing = env_set("TBK_TIMING");  // phase lines on stderr
  // (TBK_TIMING=2: the calls' kernels too, through the library's HIP events — two events per launch are themselves milliseconds of a
  // run this short, so the phase lines of TBK_TIMING=1, which the bench's end-to-end legs run under, come without them)
  bool ktiming = env_num("TBK_TIMING", 0) > 1;
  int device = (int)env_num("TBK_DEVICE", 0);
  bool threads_set = env_set("TBK_THREADS");  // the host's worker threads: the CPU budget (1..128) or TBK_THREADS
  int threads = threads_set ? std::max(1, (int)env_num("TBK_THREADS", 1)) : std::min(128, std::max(1, tbh::cpu_budget()));
  bool host_fast_off = env_num("TBK_HOST_FAST", 1) == 0;
  bool hybrid_off = env_num("TBK_HYBRID", 1) == 0, hybrid_on = env_num("TBK_HYBRID", 0) != 0;
  bool hybrid_share_set = env_set("TBK_HYBRID_SHARE");  // the device's share of the hybrid decode, per cent
  double hybrid_share = hybrid_share_set ? atof(getenv("TBK_HYBRID_SHARE")) : 0;
  bool device_decode_set = env_set("TBK_DEVICE_DECODE"), device_decode_on = env_num("TBK_DEVICE_DECODE", 0) != 0;
  uint64_t device_decode_max = (uint64_t)env_num("TBK_DEVICE_DECODE_MAX", (long long)6 << 30);
  bool tile_records_set = env_set("TBK_TILE_RECORDS");  // records per streamed tile
  size_t tile_records = (size_t)env_num("TBK_TILE_RECORDS", (long long)64 << 20);
  bool no_warmup = env_set("TBK_NO_WARMUP");
  bool dw_one_encoder = env_set("TBK_DW_ONE_ENCODER");    // no second context for the device writer
  bool no_keep_results = env_set("TBK_NO_KEEP_RESULTS");  // the tags' values come back with the collapse
  bool test_whole_enomem = env_set("TBK_TEST_WHOLE_ENOMEM");  // test hook: a whole-input collapse reports TBK_ENOMEM
  bool test_fetch_enomem = env_set("TBK_TEST_FETCH_ENOMEM");  // test hook: the representative-record fetch reports TBK_ENOMEM
  bool track_host_fmt = env_set("TBK_TRACK_HOST_FMT");        // the track text by the host formatter instead of tbk_format_track
  int exit_timing = (int)env_num("TBK_EXIT_TIMING", -1);      // diagnosis of the process exit (-1: unset)
  std::string python = getenv("TBK_PYTHON") ? getenv("TBK_PYTHON") : "python3";  // the interpreter that runs --ranks
};

// `tiebrush --ranks N ...`: the multi-GPU form (tiebrush_amd/ranks.py: one process per GPU over torch.distributed / RCCL, the input
// files sharded by rank, one output BAM).  The launcher, which starts the ranks, runs as a child of this process.
static volatile pid_t g_ranks_child = 0;
static void forward_to_ranks_child(int sig) {
  if (g_ranks_child > 0) kill(g_ranks_child, sig);
}
static void spawn_ranks_launcher_if_asked(int argc, char* argv[], const Env& env) {
  bool want = false;
  for (int i = 1; i < argc; ++i) want = want || strcmp(argv[i], "--ranks") == 0 || strncmp(argv[i], "--ranks=", 8) == 0;
  if (!want) return;
  char exe[PATH_MAX];
  const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
  if (n <= 0) GError("Error: --ranks: cannot locate the installation\n");
  exe[n] = 0;
  std::string root(exe);  // <root>/tiebrush_amd/_build/tiebrush
  for (int up = 0; up < 3; ++up) {
    const size_t sl = root.rfind('/');
    if (sl == std::string::npos) GError("Error: --ranks: cannot locate the installation\n");
    root.resize(sl);
  }
  std::string pp = root;
  if (const char* old = getenv("PYTHONPATH")) pp += std::string(":") + old;
  setenv("PYTHONPATH", pp.c_str(), 1);
  std::vector<char*> av;
  const char* py = env.python.c_str();
  av.push_back(const_cast<char*>(py));
  av.push_back(const_cast<char*>("-m"));
  av.push_back(const_cast<char*>("tiebrush_amd.ranks"));
  for (int i = 1; i < argc; ++i) av.push_back(argv[i]);
  av.push_back(nullptr);
  // a CHILD, never an exec of this process: under a profiler or any launcher that preloads a GPU-initialising library this process may
  // already hold the GPU, and replacing such a process is what takes a node down.  The launcher runs as a fresh process; this one
  // waits, forwards the signals a caller's timeout would send and leaves with the child's status.
  pid_t child = 0;
  const int rc = posix_spawnp(&child, py, nullptr, nullptr, av.data(), environ);
  if (rc != 0) GError("Error: --ranks: cannot start %s (%s)\n", py, strerror(rc));
  g_ranks_child = child;
  signal(SIGTERM, forward_to_ranks_child);
  signal(SIGINT, forward_to_ranks_child);
  signal(SIGHUP, forward_to_ranks_child);
  int status = 0;
  while (waitpid(child, &status, 0) < 0)
    if (errno != EINTR) GError("Error: --ranks: waiting for the launcher failed (%s)\n", strerror(errno));
  fflush(stdout);
  fflush(stderr);
  _exit(WIFEXITED(status) ? WEXITSTATUS(status) : 128 + (WIFSIGNALED(status) ? WTERMSIG(status) : 0));
}

// ---- tracks (--cov / --junc / --samp): what tiecov would read back from the output BAM.  Every group that goes into the file adds its
// record to a tbh::CovRecs as tiecov decodes it (tracks.h: tid, pos, flag, CIGAR, splice strand) with the YC / YX values the writer
// put into that record: written_values.  Those are (float)yc and yx for a record that carried none of the three tags, and otherwise
// whatever the tag update left: an integer YC of an old TieBrush input is not replaced by bam_aux_update_float (bam.cpp: update_float),
// and tiecov reads that stale value.  The one source of the written bytes is the writer's own tagging (tagwrite.cpp), so such records
// are tagged again here and their tags read back.  Once the routes are done the whole file's records go through tbh::run_tracks, as in
// tiecov, so the JUNC numbering and the bundles run over the whole file whatever tiles the collapse used.
static void written_values(const tbh::RecView& v, double gyc, int64_t gyx, int32_t gyd, double* wyc, int64_t* wyx) {
  bool fresh = gyx >= 0 && gyx <= (int64_t)UINT32_MAX;  // (tagwrite.cpp: the tags are appended as they are)
  for (const uint8_t* a = v.aux_begin(); fresh && a + 3 <= v.aux_end();) {
    const size_t sz = tbh::aux_field_size(a, v.aux_end());
    if (!sz) break;
    if (a[0] == 'Y' && (a[1] == 'C' || a[1] == 'X' || a[1] == 'D')) fresh = false;
    a += sz;
  }
  if (fresh) {
    *wyc = (double)(float)gyc, *wyx = gyx;
    return;
  }
  thread_local std::vector<uint8_t> o;
  thread_local tbh::BamRec rr;
  o.clear();
  tbh::append_tagged(v, gyc, gyx, gyd, o, rr);
  tbh::RecView w;
  w.p = o.data() + 4;
  w.len = (uint32_t)(o.size() - 4);
  *wyc = 1.0, *wyx = 1;  // (tiecov.cpp:482-485 defaults)
  if (const uint8_t* t = tbh::aux_get(w.aux_begin(), w.aux_end(), "YC")) *wyc = tbh::aux2f(t);
  if (const uint8_t* t = tbh::aux_get(w.aux_begin(), w.aux_end(), "YX")) *wyx = tbh::aux2i(t);
}

// The inputs as the routes see them.
struct Inputs {
  std::vector<std::string> paths;
  std::vector<uint64_t> size;    // compressed bytes (0 when stat fails)
  std::vector<uint8_t> merged;   // TieBrush-merged: their tags are updated in place
  uint64_t total = 0;
  bool all_bgzf = true, any_merged = false, all_sized = true;  // (SAM text inputs are decoded by the streaming reader)
  explicit Inputs(const TInputFiles& in) {
    for (const TSamReader* r : in.freaders) {
      struct stat st;
      const bool sized = stat(r->fname.c_str(), &st) == 0;
      paths.push_back(r->fname);
      size.push_back(sized ? (uint64_t)st.st_size : 0);
      merged.push_back(r->tbMerged ? 1 : 0);
      total += size.back();
      all_bgzf = all_bgzf && tbh::bgzf_probe(r->fname);
      any_merged = any_merged || r->tbMerged;
      all_sized = all_sized && sized;
    }
  }
};

// Which routes may take the inputs.  They are tried in this order; one that gives up hands the inputs over to the next eligible one
// (the whole-input host loader excepted: it does not run after a hybrid decode that gave up), and the streaming route takes the rest.
//   route          inputs                                          options          environment
//   hybrid         >= 2, all BGZF, none TieBrush-merged,           not -L, not -A   TBK_HOST_FAST != 0, TBK_HYBRID != 0, TBK_TILE_RECORDS
//                  >= 768 MB in all unless TBK_HYBRID != 0                          unset, TBK_DEVICE_DECODE unset (any value, 0 too, turns it off)
//   whole host     >= 1, all BGZF, within host_budget() (the       not -L, not -A   TBK_HOST_FAST != 0, TBK_DEVICE_DECODE unset or 0,
//                  loader finds out; else it gives up)                              TBK_TILE_RECORDS unset
//   device decode  all BGZF, 0 < total <= TBK_DEVICE_DECODE_MAX    any              TBK_DEVICE_DECODE != 0 (opt in: with libdeflate on every
//                  (6 GiB)                                                          core the host is faster end to end)
//   streaming      everything else
struct Routes {
  bool hybrid, whole_host, device_decode;
};
static Routes eligible_routes(const Env& e, const tbk_collapse_opts& opt, const Inputs& in) {
  const bool host = !e.host_fast_off && !e.tile_records_set && opt.strategy != TBK_STRAT_FULL && !opt.collapse_same;
  Routes r;
  r.hybrid = host && in.paths.size() >= 2 && in.all_bgzf && !in.any_merged && in.all_sized && !e.hybrid_off && !e.device_decode_set &&
             (e.hybrid_on || in.total >= ((uint64_t)768 << 20));
  r.whole_host = host && !e.device_decode_on && in.all_bgzf && !in.paths.empty();
  r.device_decode = e.device_decode_on && in.all_bgzf && in.total > 0 && in.total <= e.device_decode_max;
  return r;
}

// The device's bring-up.  Binding libtbk.so (the HIP runtime comes with it) and bringing the device up take ~0.3 s: both happen on a
// helper thread while the inputs are opened, inflated and parsed.  The thread brings the device up and then warms the context.  A caller
// that can use the context the moment it exists — the hybrid route's device decode — says so (take_now) and gets it unwarmed: it runs
// the warm-up itself (warm_own) when its decode is done and the cores are still busy with their share.
class Device {
 public:
  TbkApi api;
  tbk_ctx* ctx = nullptr;
  DeviceWriter* dw = nullptr;  // (pinned staging: lives until the process ends)
  const Clock t_start;         // the run's start
  double ms_ready = 0;         // the context existed this long after it

  Device(const Env& env, const tbk_collapse_opts& opt, bool dev_writer, bool tracks, Clock start) : t_start(start), env_(env), opt_(opt), tracks_(tracks) {
    thread_ = std::thread([this, dev_writer] { bring_up(dev_writer); });
  }
  // the context, warmed (this joins the helper thread)
  void wait() {
    if (joined_) return;
    thread_.join();
    joined_ = true;
    check();
  }
  // the context as soon as it exists, unwarmed; the helper thread is NOT joined here
  void take_now() {
    urgent_.store(true);
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return created_ && !warming_; });
    lk.unlock();
    check();
  }
  // the context's own part of the warm-up (the helper thread leaves it to the caller of take_now)
  void warm_own() {
    if (warm_ || !api_ok_ || rc_ != 0 || env_.no_warmup) return;
    warm_ = true;
    (void)api.warmup(ctx);
  }

 private:
  const Env& env_;
  const tbk_collapse_opts opt_;
  const bool tracks_;
  std::thread thread_;
  bool joined_ = false, api_ok_ = false, warm_ = false;
  int rc_ = 0;
  std::mutex m_;
  std::condition_variable cv_;
  bool created_ = false, warming_ = false;  // (under m_)
  std::atomic<bool> urgent_{false};

  void check() {
    if (!api_ok_) GError("Error: cannot load libtbk.so (%s); this build has no CPU collapse path\n", api.error.c_str());
    if (rc_ != 0) GError("Error: cannot use GPU %d (%s); this build has no CPU collapse path\n", env_.device, api.strerror_(rc_));
    if (tracks_ && !api.has_tracks()) GError("Error: --cov / --junc / --samp: libtbk.so lacks the track entry points (tbk_format_track)\n");
  }
  void bring_up(bool dev_writer) {
    api_ok_ = api.load();
    if (api_ok_) rc_ = api.create(env_.device, &ctx);
    if (api_ok_ && rc_ == 0 && dev_writer) dw = new DeviceWriter(api, tbh::cpu_budget());
    ms_ready = tms(t_start, tnow());
    bool warm_here;
    {
      std::lock_guard<std::mutex> lk(m_);
      created_ = true;
      warm_here = !urgent_.load();
      warming_ = warm_here;
    }
    cv_.notify_all();
    // (page-locking the writer's staging buffers: ~ 12 ms, beside the decode — and behind the hand-over: a decode that waits for the
    // context does not wait for this)
    if (dw) (void)dw->reserve();
    // ... and a second context for the writer's second encode thread (its queue: ~ 10 ms to create)
    if (dw && !env_.dw_one_encoder) {
      tbk_ctx* c2 = nullptr;
      if (api.create(env_.device, &c2) == 0) dw->set_second(c2);
    }
    const bool can_warm = api_ok_ && rc_ == 0 && !env_.no_warmup;
    if (warm_here) {
      if (can_warm) warm_process(ctx), warm_own();
      {
        std::lock_guard<std::mutex> lk(m_);
        warming_ = false;
      }
      cv_.notify_all();
    } else if (can_warm) {
      // the context is in use already (the hybrid route's device decode): the process-wide part on a context of this thread's own,
      // beside that decode; the decode thread does the context's part when its call has returned
      tbk_ctx* wc = nullptr;
      if (api.create(env_.device, &wc) == 0) {
        warm_process(wc);
        api.destroy(wc);
      }
    }
  }
  // What a first call pays beyond its kernels, paid ahead: (a) for the PROCESS — the library's code objects mapped onto the device by a
  // first launch, the copy engines' first use — with one tiny collapse and tbk_warmup on whatever context `c` is; (b) for the context
  // that will run the real call — its second queue, its list machines' first dispatch, its staging buffer: tbk_warmup(ctx), warm_own.
  void warm_process(tbk_ctx* c) {
    // (65 inputs of one record each: more than 64 inputs take the window path, whose kernels — the larger part of the library's
    // device code — would otherwise be mapped by the first real collapse)
    constexpr uint32_t WK = 65;
    uint32_t fo[WK + 1], co[WK + 1], cg[WK];
    uint8_t tb0[WK], mq[WK], st[WK];
    int32_t ti[WK], po[WK], nh[WK];
    uint16_t fl[WK];
    for (uint32_t i = 0; i < WK; ++i) fo[i] = co[i] = i, cg[i] = 50u << 4, tb0[i] = 0, mq[i] = 60, st[i] = '.', ti[i] = 0, po[i] = 10, nh[i] = 1, fl[i] = 0;
    fo[WK] = co[WK] = WK;
    tbk_soa_in w;
    memset(&w, 0, sizeof(w));
    w.mem = TBK_MEM_HOST;
    w.n_files = WK, w.n_records = WK, w.n_cigar_ops = WK;
    w.file_off = fo, w.tbmerged = tb0, w.tid = ti, w.pos = po, w.flag = fl, w.mapq = mq, w.strand = st, w.nh = nh, w.cig_off = co, w.cig = cg;
    uint32_t wrep[WK];
    double wyc[WK];
    int64_t wyx[WK];
    int32_t wyd[WK];
    tbk_groups_out wo;
    memset(&wo, 0, sizeof(wo));
    wo.mem = TBK_MEM_HOST;
    wo.cap_groups = WK;
    wo.rep = wrep, wo.yc = wyc, wo.yx = wyx, wo.yd = wyd;
    tbk_collapse_opts wopt = opt_;
    (void)api.collapse_tile(c, &wopt, &w, &wo);
    if (c != ctx) (void)api.warmup(c);  // (the engines; ctx gets its own call: warm_own)
  }
};

// The output side: the BAM file, the whole-input routes' result arrays, and what went into the file.
class Output {
 public:
  // the whole-input routes' results (size_results: a value-initialising resize of 32 M entries x 24 B costs more than the collapse)
  RawBuf<uint32_t> rep;
  RawBuf<double> yc;
  RawBuf<int64_t> yx;
  RawBuf<int32_t> yd;
  uint64_t groups = 0;                  // groups in the file
  double ms_dev_write = 0;              // the device writer's time, its bytes of tagged records and of BGZF members
  uint64_t dev_payload = 0, dev_z = 0;

  Output(const char* fname, sam_hdr_t* hdr, Device& dev, const Env& env, tbh::CovRecs* tracks, tbh::BaiIndex* bai = nullptr)
      : file_(new GSamWriter(fname, hdr, GSamFile_BAM)), dev_(dev), env_(env), tracks_(tracks), bai_(bai), bai_path_(std::string(fname) + (bai && bai->csi() ? ".csi" : ".bai")) {}
  // (the end of the file: the EOF member; the index goes out once that is on disk)
  void close() {
    file_.reset();
    if (!bai_) return;
    auto a = tnow();
    std::string err;
    if (!bai_->write(bai_path_, err)) GError("Error: writing the index failed: %s\n", err.c_str());
    if (env_.timing) fprintf(stderr, "index: %s written in %.1f ms\n", bai_path_.c_str(), tms(a, tnow()));
  }
  // whether the whole-input routes leave the tags' values on the device for the device writer (tbk_collapse_opts.keep_results)
  bool keep_results() const { return dev_.dw && file_->level() != 0 && !env_.no_keep_results; }

  // Groups [0, ng) of one collapse: rep / yc / yx / yd are host arrays in output order (yc == nullptr: the values stayed on the device,
  // keep_results).  The device writer takes them when there is one (devwriter.h; c: its context): tags, framing and BGZF deflate as
  // kernels, the host only gathers the records it decoded itself (rec(g) for rep[g] >= n_dev) and appends the finished members.  From
  // the group it refuses on, the host writer goes on — after before_host(), which readies what rec() reads for it.  When that fails,
  // write returns false; the groups before the refused one are in the file (groups says how many).  With tracks, the groups of a write
  // that returns true go to them (after before_host() when the device writer took every group: the tracks read the records).
  bool write(tbk_ctx* c, uint32_t ng, const uint32_t* rp, const double* ycp, const int64_t* yxp, const int32_t* ydp, uint32_t n_dev, const RecFn& rec,
             const PrefetchFn& prefetch = nullptr, const std::function<bool()>& before_host = nullptr) {
    uint32_t done = 0;
    const bool kept = ycp == nullptr;
    if (c && dev_.dw && file_->level() != 0) {
      auto a = tnow();
      uint64_t pb = 0, zb = 0;
      std::string why;
      const bool ok = dev_.dw->write(c, *file_, ng, rp, ycp, yxp, ydp, n_dev, rec, &pb, &zb, why, &done, prefetch, bai_);
      ms_dev_write += tms(a, tnow()), dev_payload += pb, dev_z += zb;
      groups += ok ? ng : done;
      if (ok) {
        if (tracks_ && before_host && !before_host()) GError("Error: fetching the representative records for the tracks failed after %llu groups were written\n", (unsigned long long)groups);
        return add_tracks(c, ng, ycp, yxp, ydp, kept, rec);
      }
      if (env_.timing) fprintf(stderr, "device writer stopped after %u of %u groups (%s): host writer\n", done, ng, why.c_str());
    }
    if (before_host && !before_host()) return false;
    if (ng <= done) return true;
    if (!ycp) {  // (the host writer fetches the values of the groups it writes)
      yc.resize(ng), yx.resize(ng), yd.resize(ng);
      const int frc = dev_.api.kept_results(c, done, ng - done, nullptr, yc.data() + done, yx.data() + done, yd.data() + done);
      if (frc != 0) GError("Error: fetching the collapse's results failed: %s (%s)\n", dev_.api.strerror_(frc), dev_.api.last_error(c));
      ycp = yc.data(), yxp = yx.data(), ydp = yd.data();
    }
    // flushPData's tagging on every core (tagwrite.h); one slice when a single thread writes
    auto from_done = [&](uint32_t g) { return rec(done + g); };
    // (--index: a slice's records come with its members; the slice's index part is the host builder's, bai.h)
    std::vector<std::vector<tbh::BaiRec>> slice_recs;
    size_t slice = 0;
    auto emit = [&](const uint8_t* z, size_t n) {
      if (bai_) {
        const std::vector<tbh::BaiRec>& sr = slice_recs[slice++];
        tbh::BaiPart part;
        std::string err;
        if (!tbh::bai_build_part(sr.data(), sr.size(), (uint64_t)n << 16, bai_->ref_len(), part, err, bai_->depth())) GError("Error: indexing the output failed: %s\n", err.c_str());
        bai_->add(file_->tell(), part);
      }
      return file_->write_members(z, n), true;
    };
    if (!tbh::tag_deflate_ordered(ng - done, from_done, ycp + done, yxp + done, ydp + done, file_->level(), env_.threads, emit, env_.threads > 1 ? 16384 : 0,
                                  bai_ ? &slice_recs : nullptr))
      GError("Error: deflate failed\n");
    groups += ng - done;
    return add_tracks(c, ng, ycp, yxp, ydp, kept && done > 0, rec);
  }

  // A route that cannot finish hands the inputs over to the next one, which writes from group 0: only while the file holds no groups.
  void fall_through(const char* what, const std::string& why) {
    if (groups) GError("Error: %s (%s) after %llu groups were written\n", what, why.c_str(), (unsigned long long)groups);
    if (env_.timing) fprintf(stderr, "%s (%s): streaming host path\n", what, why.c_str());
    rep.resize(0);  // (drops pages borrowed from the route's input tile)
  }

 private:
  std::unique_ptr<GSamWriter> file_;
  Device& dev_;
  const Env& env_;
  tbh::CovRecs* tracks_;
  tbh::BaiIndex* bai_;  // --index / --csi: the parts of everything that goes into the file, in file order
  std::string bai_path_;

  // fetch: the values of groups [0, ng) are on the device only (keep_results)
  bool add_tracks(tbk_ctx* c, uint32_t ng, const double* ycp, const int64_t* yxp, const int32_t* ydp, bool fetch, const RecFn& rec) {
    if (!tracks_) return true;
    auto a = tnow();
    if (fetch) {
      yc.resize(ng), yx.resize(ng), yd.resize(ng);
      const int frc = dev_.api.kept_results(c, 0, ng, nullptr, yc.data(), yx.data(), yd.data());
      if (frc != 0) GError("Error: fetching the collapse's results failed: %s (%s)\n", dev_.api.strerror_(frc), dev_.api.last_error(c));
      ycp = yc.data(), yxp = yx.data(), ydp = yd.data();
    }
    auto values = [&](uint32_t g, const tbh::RecView& v, double* wyc, int64_t* wyx) { written_values(v, ycp[g], yxp[g], ydp[g], wyc, wyx); };
    if (!tracks_->append(ng, rec, values, ng < 16384 ? 1 : env_.threads)) GError("Error: the output is too large for one coverage tile (--cov / --junc / --samp)\n");
    if (env_.timing) fprintf(stderr, "tracks: %u records added in %.1f ms\n", ng, tms(a, tnow()));
    return true;
  }
};

// the device entry points for tbh::run_tracks (tiebrush cuts the records of a region run, not the rows: no clip entries)
static tbh::TrackApi track_api(const Device& dev) {
  const TbkApi& d = dev.api;
  tbh::TrackApi a;
  a.ctx = dev.ctx;
  a.coverage_tile = d.coverage_tile, a.sample_tile = d.sample_tile;
  a.track_names = d.track_names, a.format_track = d.format_track, a.track_bgzf = d.track_bgzf, a.bigwig_build = d.bigwig_build, a.cov_summary = d.cov_summary, a.cov_thresholds = d.cov_thresholds, a.tx_summary = d.tx_summary, a.cov_split_strand = d.cov_split_strand;
  a.strerror_ = d.strerror_, a.last_error = d.last_error;
  return a;
}

// What the summary lines count.
struct Totals {
  double ms_load = 0, ms_gpu = 0, ms_tag = 0, ms_inflate = 0;
  uint64_t in = 0, out = 0;
  size_t n_tiles = 0;
};

enum class Route { done, fall_through };

// a whole-input route's end: one tile
static Route account_whole(Totals& t, const tbk_groups_out& res, double ms_inflate, double ms_gpu, double ms_tag) {
  t.ms_inflate += ms_inflate, t.ms_gpu += ms_gpu, t.ms_tag += ms_tag;
  t.in += res.n_passed, t.out += res.n_groups;
  t.n_tiles = 1;
  return Route::done;
}

static std::string why_rc(Device& dev, int rc) { return std::string(dev.api.strerror_(rc)) + ": " + dev.api.last_error(dev.ctx); }

// TBK_TIMING=2: the kernels of the call just made (HIP events) — what of its wall time the GPU was busy with
static void print_kernel_times(Device& dev, const char* call, double ms_call) {
  tbk_kernel_time kt[64];
  const int nk = dev.api.kernel_times(dev.ctx, kt, 64);
  std::string line = std::string(call) + " kernels ms:";
  double sum = 0;
  for (int i = 0; i < nk; ++i) {
    char b[96];
    snprintf(b, sizeof(b), " %s %.1f (%u)", kt[i].name, kt[i].ms, kt[i].launches);
    line += b;
    sum += kt[i].ms;
  }
  fprintf(stderr, "%s | sum %.1f of the call's %.1f\n", line.c_str(), sum, ms_call);
  (void)dev.api.set_profiling(dev.ctx, 0);
}

// The results of a collapse of n records: host arrays (none when `arrays` is false: the results stay on the device) sized by the upper
// bound, one group per record, but never initialised — the pages a call does not write are never touched.
static void size_results(tbk_groups_out* res, size_t n, RawBuf<uint32_t>& rep, RawBuf<double>& yc, RawBuf<int64_t>& yx, RawBuf<int32_t>& yd,
                         bool arrays = true) {
  if (n == 0) n = 1;
  memset(res, 0, sizeof(*res));
  res->mem = TBK_MEM_HOST;
  res->cap_groups = (uint32_t)n;
  if (!arrays) return;
  rep.resize(n), yc.resize(n), yx.resize(n), yd.resize(n);
  res->rep = rep.data(), res->yc = yc.data(), res->yx = yx.data(), res->yd = yd.data();
}

// One collapse of a whole-input tile into out's arrays.  keep: the tags' values stay on the device for the device writer
// (keep_results), and only `rep` comes back, once the number of groups is known — into pages that are resident already when a dead
// array of the host's input tile (`dead`, 4 bytes a record) is long enough: a fresh block of tens of megabytes is faulted in at
// 1-2 GB/s this late in the run.  An unsorted input is fatal; any other code is the caller's.
static int collapse_whole(Device& dev, Output& out, const Env& env, tbk_collapse_opts opt, bool keep, tbk_soa_in* in, tbk_groups_out* res,
                          int32_t* dead = nullptr, size_t dead_n = 0) {
  size_results(res, in->n_records, out.rep, out.yc, out.yx, out.yd, !keep);
  opt.keep_results = keep ? 1 : 0;
  auto a = tnow();
  if (env.ktiming) (void)dev.api.set_profiling(dev.ctx, 1);
  int rc = dev.api.collapse_tile(dev.ctx, &opt, in, res);
  if (rc == 0 && env.test_whole_enomem) rc = TBK_ENOMEM;  // test hook: exercise the fall-through
  if (rc == 0 && keep) {
    const uint32_t ng = res->n_groups;
    if (dead && ng <= dead_n) out.rep.borrow((uint32_t*)dead, dead_n);
    else out.rep.resize(ng ? ng : 1);
    auto f0 = tnow();
    const int frc = dev.api.kept_results(dev.ctx, 0, ng, out.rep.data(), nullptr, nullptr, nullptr);
    if (frc != 0) GError("Error: fetching the collapse's results failed: %s (%s)\n", dev.api.strerror_(frc), dev.api.last_error(dev.ctx));
    if (env.timing) fprintf(stderr, "representatives of %u groups fetched in %.1f ms (%s)\n", ng, tms(f0, tnow()), out.rep.borrowed ? "into the input tile's pages" : "into a new block");
  }
  if (env.ktiming) print_kernel_times(dev, "collapse call", tms(a, tnow()));
  if (rc == TBK_EUNSORTED) GError("Error: an input file is not coordinate-sorted!\n");
  return rc;
}

// The raw records of n representatives of the tile tbk_bam_decode left on the device (ids: its record indices): record i at
// blob[roff[i] + 4, roff[i + 1]) (the block_size field first).  `guess`: bytes a record, for the first try; a blob too small
// (TBK_E2BIG) is grown to what it takes and asked once more.
static int fetch_device_records(Device& dev, const Env& env, const uint32_t* ids, uint32_t n, size_t guess, RawBuf<uint8_t>& blob, RawBuf<uint64_t>& roff) {
  roff.resize((size_t)n + 1);
  blob.resize((size_t)n * guess + 4096);
  int rc = dev.api.bam_records(dev.ctx, ids, n, TBK_MEM_HOST, blob.data(), blob.size(), roff.data());
  if (rc == TBK_E2BIG) {
    blob.resize(roff[n]);
    rc = dev.api.bam_records(dev.ctx, ids, n, TBK_MEM_HOST, blob.data(), blob.size(), roff.data());
  }
  if (rc == 0 && env.test_fetch_enomem) rc = TBK_ENOMEM;  // test hook: a fetch that fails behind groups already written
  return rc;
}

// half of what the host may still use (MemAvailable, the cgroup's limit): what the whole-input loaders may fill with inflated inputs
static size_t host_budget() {
  size_t budget = (size_t)8 << 30;
  if (FILE* mf = fopen("/proc/meminfo", "r")) {
    char line[256];
    while (fgets(line, sizeof(line), mf))
      if (strncmp(line, "MemAvailable:", 13) == 0) budget = (size_t)atoll(line + 13) * 1024 / 2;
    fclose(mf);
  }
  if (FILE* cf = fopen("/sys/fs/cgroup/memory.max", "r")) {
    char q[64];
    if (fscanf(cf, "%63s", q) == 1 && strcmp(q, "max") != 0) budget = std::min<size_t>(budget, (size_t)atoll(q) / 2);
    fclose(cf);
  }
  return budget;
}

// ---- hybrid decode: records with SEQ / QUAL are ~ 240 inflated bytes each and the run is BGZF on the host's cores (SURVEY.md
// §8 f1).  The GPU inflates and decodes the first files of the list (tbk_bam_decode) WHILE the cores inflate and decode the rest
// (fastload.cpp); tbk_tile_join makes one device tile of the two, the collapse runs on it, and a representative's raw record
// comes from wherever its file was decoded.  TBK_HYBRID=0 / 1 switches it off / on (default: inputs of 768 MB and more),
// TBK_HYBRID_SHARE = the device's share of the compressed bytes in per cent.
static Route run_hybrid(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, const Inputs& inp, Totals& tot) {
  const size_t k = inp.paths.size();
  // The device's share of the compressed bytes: both sides should end together.  The device starts late — the HIP runtime takes
  // ~ 0.1 s to come up (t_ctx = 0.15: the helper thread's warm-up beside the decode and the context's own behind it cost the
  // device's side another 0.05), the cores work alone meanwhile — and is then several times faster: with x of T bytes on the device,
  // t_ctx + x / R_dev = (T - x) / R_host.  Rates measured on an MI355X box with a 16-core quota (round 5's end-to-end legs, tools/e2e_leg.py): the
  // device side 4.7 GB/s of compressed BAM (upload, inflate, record index, SoA), a core 0.18 GB/s (inflate with the record index
  // riding along, SoA).  1.8 GB of input: 54 % (17 of 32 files; measured round 6, five runs a share: 16 files 407 ms for the
  // decode, 17 files 351-361, 18 files 374-382, 19 files 377-384); 7.1 GB: 63 %.  TBK_HYBRID_SHARE (per cent) overrides.
  const int host_threads = env.threads_set ? env.threads : std::max(2, env.threads - 3);
  double share;
  if (env.hybrid_share_set) {
    share = env.hybrid_share / 100.0;
  } else {
    const double T = (double)inp.total / 1e9, r_dev = 4.7, r_host = 0.18 * host_threads, t_ctx = 0.15;
    const double x = (T / r_host - t_ctx) / (1.0 / r_dev + 1.0 / r_host);
    share = std::min(0.9, std::max(0.2, x / T));
  }
  const std::vector<uint64_t>& fsz = inp.size;
  size_t kd = 0;
  uint64_t acc = 0;
  while (kd + 1 < k && (double)(acc + fsz[kd]) <= share * (double)inp.total + (double)fsz[kd] / 2) acc += fsz[kd++];
  if (kd == 0) kd = 1;
  const size_t budget = host_budget();
  auto t0 = tnow();
  if (env.timing) fprintf(stderr, "hybrid decode starts at %.1f ms\n", tms(dev.t_start, t0));
  // the device's share, on a thread of its own: read the files, wait for the context, decode
  tbk_soa_in in_d;
  memset(&in_d, 0, sizeof(in_d));
  std::vector<uint32_t> fo_d(kd + 1, 0);
  std::vector<uint8_t> tb_d(kd, 0);
  int rc_d = -1;
  bool read_ok = true;
  double ms_dread = 0, ms_ddec = 0, ms_dcall = 0;
  std::thread dth([&]() {
    auto d0 = tnow();
    std::vector<FileMap> comp(kd);
    for (size_t f = 0; f < kd; ++f)
      if (!comp[f].map(inp.paths[f]) || comp[f].n != fsz[f]) read_ok = false;
    auto d1 = tnow();
    ms_dread = tms(d0, d1);
    if (!read_ok) return;
    dev.take_now();
    auto d2 = tnow();
    std::vector<const uint8_t*> ptr(kd);
    for (size_t f = 0; f < kd; ++f) ptr[f] = comp[f].p;
    if (env.ktiming) (void)dev.api.set_profiling(dev.ctx, 1);
    rc_d = dev.api.bam_decode(dev.ctx, (uint32_t)kd, ptr.data(), fsz.data(), tb_d.data(), 0, 0, &in_d, fo_d.data());
    ms_dcall = tms(d2, tnow());
    if (env.ktiming) print_kernel_times(dev, "device decode", ms_dcall);
    for (auto& c : comp) c.unmap();
    if (rc_d == 0 && acc > 0) {  // the arena for the joined tile, sized while the cores are still decoding their share
      // (tbk_reserve_tile sizes for the window path AND a deferred YD stage that borrows its range of the arena: 165 bytes a record.
      // This call defers nothing — 84 bytes a record and the CIGAR words —: six tenths of the tile's size asks for what it takes.
      // An allocation of gigabytes is now and then 20-25 ms per GB of the driver's time)
      const double up = (double)inp.total / (double)acc * 1.05 * 0.6;
      (void)dev.api.reserve_tile(dev.ctx, (uint64_t)((double)in_d.n_records * up), (uint64_t)((double)in_d.n_cigar_ops * up));
    }
    ms_ddec = tms(d1, tnow());
    dev.warm_own();  // (the helper thread left the context's own part to this one: take_now)
  });
  // the cores' share
  tbh::FastTile& ft = *new tbh::FastTile();  // (gigabytes, needed until the last record is written: left to the process exit)
  std::vector<std::string> ph(inp.paths.begin() + (long)kd, inp.paths.end());
  std::vector<uint8_t> tbh_(k - kd, 0);
  bool fits = false;
  std::string err;
  // (the device's side needs cores too while it runs — the HIP start-up, then the threads that feed the upload ring —, and a
  // container's CPU quota stalls EVERY thread of the process once the sum goes over it: the loader leaves them room)
  const bool okh = tbh::fast_load(ph, tbh_, host_threads, budget, ft, &fits, err);
  dth.join();
  auto t1 = tnow();
  dev.wait();  // (the helper thread ended long ago; this only joins it)
  if (!okh) GError("Error: reading the input failed (%s)\n", err.c_str());
  if (!read_ok) GError("Error: reading the input failed\n");
  if (rc_d != 0 && rc_d != TBK_ENOMEM && rc_d != TBK_E2BIG) GError("Error: decoding the input on the GPU failed: %s (%s)\n", dev.api.strerror_(rc_d), dev.api.last_error(dev.ctx));
  int rc = 0;
  tbk_soa_in in;
  std::vector<uint32_t> fo(k + 1, 0);
  std::vector<uint8_t> tbm(k, 0);
  tbk_groups_out res;
  memset(&res, 0, sizeof(res));
  const uint32_t n_d = in_d.n_records;
  auto t_join = t1, t_col = t1, t_rec = t1;
  bool wrote = false, via_host = false, released = false;
  auto release = [&]() {
    auto r0 = tnow();
    dev.api.bam_release(dev.ctx);
    released = true;
    if (env.timing) fprintf(stderr, "bam_release %.1f ms\n", tms(r0, tnow()));
  };
  if (fits && rc_d == 0) {
    tbk_soa_in in_h = ft.view();
    rc = dev.api.tile_join(dev.ctx, &in_d, &in_h, &in, fo.data(), tbm.data());
    t_join = tnow();
    const bool keep = out.keep_results();
    if (rc == 0) rc = collapse_whole(dev, out, env, opt, keep, &in, &res, ft.tid, ft.n);  // (the host part's SoA went to the device with tbk_tile_join)
    t_rec = t_col = tnow();  // (t_rec: the end of the fetch below, when there is one)
    // a representative the device decoded: its raw record comes back from there (dev_slot: its place among those fetched)
    std::vector<uint32_t> dev_slot;
    RawBuf<uint64_t> roff;
    RawBuf<uint8_t> blob;
    auto rec = [&](uint32_t g) {
      tbh::RecView v;
      if (out.rep[g] < n_d) {
        const uint32_t s = dev_slot[g];
        v.p = blob.data() + roff[s] + 4;
        v.len = (uint32_t)(roff[s + 1] - roff[s] - 4);
      } else {
        v.p = ft.record(out.rep[g] - n_d, &v.len);
      }
      return v;
    };
    auto fetch = [&]() {
      via_host = true;
      std::vector<uint32_t> dev_rep;
      dev_slot.assign(res.n_groups, 0);
      for (uint32_t g = 0; g < res.n_groups; ++g)
        if (out.rep[g] < n_d) {
          dev_slot[g] = (uint32_t)dev_rep.size();
          dev_rep.push_back(out.rep[g]);
        }
      rc = fetch_device_records(dev, env, dev_rep.data(), (uint32_t)dev_rep.size(), 260, blob, roff);
      t_rec = tnow();
      if (rc == 0) release();
      return rc == 0;
    };
    if (rc == 0)
      wrote = out.write(dev.ctx, res.n_groups, out.rep.data(), keep ? nullptr : out.yc.data(), out.yx.data(), out.yd.data(), n_d, rec,
                        [&](uint32_t g, int stage) { stage == 0 ? ft.prefetch_index(out.rep[g] - n_d) : ft.prefetch_record(out.rep[g] - n_d); }, fetch);
  }
  if (!wrote) {
    if (rc != 0 && rc != TBK_ENOMEM && rc != TBK_E2BIG && rc != TBK_EUNSUPPORTED) GError("Error: GPU collapse failed: %s (%s)\n", dev.api.strerror_(rc), dev.api.last_error(dev.ctx));
    if (!released) release();
    out.fall_through("hybrid decode given up", rc_d != 0 ? dev.api.strerror_(rc_d) : (fits ? dev.api.strerror_(rc) : "the host's share does not fit"));
    tbh::big_release_all(env.threads);
    return Route::fall_through;
  }
  auto t3 = tnow();
  if (env.timing && !via_host)  // (the device writer took every group)
    fprintf(stderr,
            "hybrid path ms: device %zu of %zu files (context ready at %.1f | map %.1f | decode incl. context %.1f, the call %.1f) beside host (read %.1f | inflate %.1f | index %.1f | SoA %.1f) = %.1f | "
            "join %.1f | collapse %.1f | gather + tag + deflate (GPU) + write %.1f (%.1f MB of records -> %.1f MB)\n",
            kd, k, dev.ms_ready, ms_dread, ms_ddec, ms_dcall, ft.ms_read, ft.ms_inflate, ft.ms_index, ft.ms_soa, tms(t0, t1), tms(t1, t_join), tms(t_join, t_col), tms(t_col, t3),
            out.dev_payload / 1e6, out.dev_z / 1e6);
  else if (env.timing)
    fprintf(stderr,
            "hybrid path ms: device %zu of %zu files (read %.1f | decode incl. context %.1f) beside host (read %.1f | inflate %.1f | index %.1f | SoA %.1f) = %.1f | "
            "join %.1f | collapse %.1f | fetch representatives %.1f | tag+deflate+write %.1f\n",
            kd, k, ms_dread, ms_ddec, ft.ms_read, ft.ms_inflate, ft.ms_index, ft.ms_soa, tms(t0, t1), tms(t1, t_join), tms(t_join, t_col), tms(t_col, t_rec), tms(t_rec, t3));
  account_whole(tot, res, tms(t0, t1), tms(t1, t_rec), tms(t_rec, t3));
  if (!released) release();
  return Route::done;
}

// ---- whole-input host route: inputs that fit in memory are read, inflated and decoded into the tile in two parallel passes
// (fastload.cpp) while the helper thread brings the device up; one collapse, one tagged output pass
static Route run_whole_host(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, const Inputs& inp, Totals& tot) {
  tbh::FastTile& ft = *new tbh::FastTile();  // (gigabytes, needed until the last record is written: left to the process exit)
  bool fits = false;
  std::string err;
  auto t0 = tnow();
  if (!tbh::fast_load(inp.paths, inp.merged, env.threads, host_budget(), ft, &fits, err)) GError("Error: reading the input failed (%s)\n", err.c_str());
  if (!fits) return Route::fall_through;
  auto t1 = tnow();
  tbk_soa_in in = ft.view();
  dev.wait();
  auto t_ctxw = tnow();
  tbk_groups_out res;
  const bool keep = out.keep_results();
  const int rc = collapse_whole(dev, out, env, opt, keep, &in, &res, ft.tid, ft.n);  // (the SoA went to the device with the call)
  auto t2 = tnow();
  if (rc == TBK_ENOMEM || rc == TBK_E2BIG) {  // one tile of everything is more than the GPU takes: the streaming route bounds it
    out.fall_through("whole-input tile not used", why_rc(dev, rc));
    tbh::big_release_all(env.threads);
    return Route::fall_through;
  }
  if (rc != 0) GError("Error: GPU collapse failed: %s (%s)\n", dev.api.strerror_(rc), dev.api.last_error(dev.ctx));
  out.write(
      dev.ctx, res.n_groups, out.rep.data(), keep ? nullptr : out.yc.data(), out.yx.data(), out.yd.data(), 0,
      [&](uint32_t g) {
        tbh::RecView v;
        v.p = ft.record(out.rep[g], &v.len);
        return v;
      },
      [&](uint32_t g, int stage) { stage == 0 ? ft.prefetch_index(out.rep[g]) : ft.prefetch_record(out.rep[g]); });
  auto t3 = tnow();
  if (env.timing)
    fprintf(stderr, "host path ms: read %.1f | inflate %.1f | index %.1f | SoA %.1f | wait for the device %.1f | collapse (PCIe incl.) %.1f | tag+deflate+write %.1f\n",
            ft.ms_read, ft.ms_inflate, ft.ms_index, ft.ms_soa, tms(t1, t_ctxw), tms(t_ctxw, t2), tms(t2, t3));
  return account_whole(tot, res, tms(t0, t1), tms(t1, t2), tms(t2, t3));
}

// The end of a route whose tile lies decoded on the device (run_device_decode, run_region): one collapse, the output records by the
// device writer — or the representatives' raw records fetched (tbk_bam_records) for the host writer —, the write, the tile's release.
// Returns 0, or TBK_ENOMEM / TBK_E2BIG (the tile is more than the GPU takes: nothing is released, the caller decides); anything else is
// fatal here.
struct DeviceTail {
  tbk_groups_out res;
  Clock t_col, t_rec, t_rel;         // the collapse done; the records fetched (or written by the device writer); the tile released
  std::function<void()> on_release;  // (the route's phase line)
};
static int device_tile_tail(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, tbk_soa_in* in, DeviceTail& T) {
  int rc = collapse_whole(dev, out, env, opt, false, in, &T.res);
  T.t_col = T.t_rec = T.t_rel = tnow();
  RawBuf<uint64_t> roff;
  RawBuf<uint8_t> blob;
  bool released = false;
  auto release = [&]() {
    T.t_rec = tnow();
    dev.api.bam_release(dev.ctx);
    released = true;
    T.t_rel = tnow();
    if (T.on_release) T.on_release();
  };
  auto fetch = [&]() {
    rc = fetch_device_records(dev, env, out.rep.data(), T.res.n_groups, 96, blob, roff);
    if (rc == 0) release();
    return rc == 0;
  };
  auto rec = [&](uint32_t g) {  // (the device writer asks for none: every record is on the device)
    tbh::RecView v;
    v.p = blob.data() + roff[g] + 4;
    v.len = (uint32_t)(roff[g + 1] - roff[g] - 4);
    return v;
  };
  if (rc == 0)  // (false only when the fetch fails: rc says why)
    (void)out.write(dev.ctx, T.res.n_groups, out.rep.data(), out.yc.data(), out.yx.data(), out.yd.data(), (uint32_t)in->n_records, rec, nullptr, fetch);
  if (rc == TBK_ENOMEM || rc == TBK_E2BIG) return rc;
  if (rc != 0) GError("Error: GPU collapse / fetching the representative records failed: %s (%s)\n", dev.api.strerror_(rc), dev.api.last_error(dev.ctx));
  if (!released) release();
  return 0;
}

// ---- device decode: when the inputs fit, their BGZF members go to the GPU as they are — inflate, record index, aux
// scan and SoA happen there (tbk_bam_decode), the collapse reads the tile where it lies, and only the representatives' raw records come
// back (tbk_bam_records) to be tagged.  Anything it cannot take falls through to the streaming route.
static Route run_device_decode(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, const Inputs& inp, Totals& tot) {
  const size_t k = inp.paths.size();
  auto t0 = tnow();
  std::vector<FileMap> comp(k);
  std::vector<const uint8_t*> ptr(k);
  for (size_t f = 0; f < k; ++f) {
    if (!comp[f].map(inp.paths[f]) || comp[f].n != inp.size[f]) GError("Error: reading the input failed\n");
    ptr[f] = comp[f].p;
  }
  std::vector<uint32_t> fo(k + 1, 0);
  auto t_read = tnow();
  dev.wait();
  auto t_ctxw = tnow();
  tbk_soa_in in;
  int rc = dev.api.bam_decode(dev.ctx, (uint32_t)k, ptr.data(), inp.size.data(), inp.merged.data(), opt.strategy == TBK_STRAT_FULL, opt.collapse_same != 0, &in,
                              fo.data());
  auto t1 = tnow();
  for (auto& c : comp) c.unmap();
  if (rc != 0) {
    out.fall_through("device decode not used", why_rc(dev, rc));
    dev.api.bam_release(dev.ctx);  // (whatever the failed decode left on the device goes back before the streaming route sizes its tiles)
    return Route::fall_through;
  }
  DeviceTail T;
  T.on_release = [&]() {
    if (env.timing)
      fprintf(stderr, "device path ms: read files %.1f | wait for the HIP context %.1f | decode %.1f | collapse %.1f | fetch representatives %.1f | release %.1f\n",
              tms(t0, t_read), tms(t_read, t_ctxw), tms(t_ctxw, t1), tms(t1, T.t_col), tms(T.t_col, T.t_rec), tms(T.t_rec, T.t_rel));
  };
  rc = device_tile_tail(dev, out, opt, env, &in, T);
  if (rc == TBK_ENOMEM || rc == TBK_E2BIG) {  // decoded, but the whole input as one tile is more than the GPU takes:
    out.fall_through("device decode given up", why_rc(dev, rc));  // give the device copies back and let the streaming route bound the tile
    dev.api.bam_release(dev.ctx);
    return Route::fall_through;
  }
  auto t3 = tnow();
  account_whole(tot, T.res, tms(t0, t1), tms(t1, T.t_rel), tms(T.t_rel, t3));
  if (env.timing) fprintf(stderr, "device decode: %zu records from %llu compressed bytes\n", (size_t)in.n_records, (unsigned long long)inp.total);
  return Route::done;
}

// ---- -r REGION (the reference has no region option): only the chunks that every input's index names for the region are
// read; they are inflated and decoded on the device with the records grouped by input file (tbk_bam_decode_file_spans), the records that
// overlap the region are compacted into a collapse tile there (tbk_tile_region), and from then on the run is the device decode route's.
// One tile, no fall-through: the output is what the same command line without -r makes of inputs cut to the region.
// -R FILE is the same run over the region table of a BED file: every input's chunks merged over the whole table
// (regions_input_chunks), the records that overlap any interval kept once (tbk_tile_regions).
struct RegionPlan {
  tbh::RegionTable U;                              // -r: the region itself (it may be empty); -R: the normalised table
  bool one = true;                                 // -r: the one-region entries
  const char* opt = "-r";                          // how the messages name the option
  std::vector<std::string> paths;
  std::vector<std::vector<tbh::IdxChunk>> chunks;  // per input, as its index names them
  size_t n_chunks = 0;
  double ms_index = 0;
};
static bool list_argument(const std::string& p) { return !tbh::bgzf_probe(p) && !tbh::sam_probe(p); }
// what -r refuses of the inputs before they are opened: standard input, and (unless the one argument is a list of paths) anything
// that is not a BGZF file
static void refuse_region_inputs(TInputFiles& in, bool before_open, const char* o) {
  const bool list = before_open && in.freaders.size() == 1 && in.freaders[0]->fname != "-" && list_argument(in.freaders[0]->fname);
  for (const TSamReader* r : in.freaders) {
    if (r->fname == "-") GError("Error: %s: the input - (standard input) has no index; %s takes BGZF-compressed BAM files\n", o, o);
    if (!list && !tbh::bgzf_probe(r->fname)) GError("Error: %s: %s is not a BGZF-compressed BAM file (SAM text has no index)\n", o, r->fname.c_str());
  }
}
// every refusal that needs no device, in the order of DESIGN.md §4f; nothing has been created when one of them ends the run
static RegionPlan plan_region(TInputFiles& in, const char* region, const char* regions_file) {
  RegionPlan P;
  auto t0 = tnow();
  std::string err;
  sam_hdr_t* mh = in.header();
  if (regions_file) {
    P.one = false, P.opt = "-R";
    if (!tbh::regions_from_bed_file(*mh, regions_file, P.U, err)) GError("Error: -R: %s\n", err.c_str());
  } else {
    int32_t tid = 0;
    int64_t beg = 0, end = 0;
    if (!tbh::parse_region(*mh, region, &tid, &beg, &end, err)) GError("Error: -r: %s\n", err.c_str());
    P.U.add(tid, beg, end);
  }
  const int32_t max_tid = P.U.tid.back();  // (the table is sorted)
  const std::string& rname = mh->target_name[(size_t)max_tid];
  const size_t k = in.freaders.size();
  if (k > 65535) GError("Error: %s: %zu inputs; the device decode takes 65535\n", P.opt, k);
  P.chunks.resize(k);
  for (size_t f = 0; f < k; ++f) {
    const std::string& path = in.freaders[f]->fname;
    P.paths.push_back(path);
    sam_hdr_t* h = in.freaders[f]->samreader->header();
    // (the header merge has refused, with the file's name, a list that has another name at a position or a name at another position:
    // an input's list is the head of the merged one, and can only be too short for the region's reference)
    if (max_tid >= h->n_targets)
      GError("Error: %s: %s does not list the region's reference %s as reference %d, as the merged header does\n", P.opt, path.c_str(), rname.c_str(), (int)max_tid);
    std::string index_path;
    if (!tbh::regions_input_chunks(path, h->n_targets, P.U, P.chunks[f], index_path, err)) GError("Error: %s: %s\n", P.opt, err.c_str());
    P.n_chunks += P.chunks[f].size();
  }
  if (P.n_chunks > 65535 && P.one)
    GError("Error: -r: the indexes of the %zu inputs name %zu chunks for the region in all; the device decode takes 65535 (first input: %s)\n", k, P.n_chunks,
           P.paths[0].c_str());
  if (P.n_chunks > 65535)
    GError("Error: -R: the indexes of the %zu inputs name %zu chunks for the %zu regions in all; the device decode takes 65535 (first input: %s)\n", k,
           P.n_chunks, P.U.n(), P.paths[0].c_str());
  P.ms_index = tms(t0, tnow());
  return P;
}

static Route run_region(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, const Inputs& inp, const RegionPlan& plan, int32_t n_ref,
                        Totals& tot) {
  const size_t k = plan.paths.size();
  auto t0 = tnow();
  // the chunk reads, on every thread, beside the context's bring-up
  std::vector<std::vector<tbh::RegionSpan>> spans;
  uint64_t bytes_read = 0;
  std::string err;
  const bool read_ok = tbh::read_spans_many(plan.paths, plan.chunks, env.threads, spans, &bytes_read, err);
  auto t_read = tnow();
  dev.wait();
  auto t_ctx = tnow();
  if (!read_ok) GError("Error: %s: %s\n", plan.opt, err.c_str());
  std::vector<uint32_t> span_first(k + 1, 0), first_uoff, last_uoff, fo(k + 1, 0);
  std::vector<const uint8_t*> comp;
  std::vector<uint64_t> comp_bytes;
  for (size_t f = 0; f < k; ++f) {
    for (const tbh::RegionSpan& s : spans[f]) comp.push_back(s.z.data()), comp_bytes.push_back(s.z.size()), first_uoff.push_back(s.first_uoff), last_uoff.push_back(s.last_uoff);
    span_first[f + 1] = (uint32_t)comp.size();
  }
  const int want_md = opt.strategy == TBK_STRAT_FULL, want_names = opt.collapse_same != 0;
  auto too_large = [&](int rc) { GError("Error: %s: region too large for one tile (%s)\n", plan.opt, why_rc(dev, rc).c_str()); };
  tbk_soa_in tile;
  int rc = dev.api.bam_decode_file_spans(dev.ctx, (uint32_t)k, span_first.data(), comp.data(), comp_bytes.data(), first_uoff.data(), last_uoff.data(), n_ref,
                                         inp.merged.data(), want_md, want_names, &tile, fo.data());
  if (rc == TBK_ENOMEM || rc == TBK_E2BIG) too_large(rc);
  if (rc == TBK_EINVAL) {  // a malformed span: the inputs' spans one by one name the file
    const std::string why = why_rc(dev, rc);
    for (size_t f = 0; f < k; ++f) {
      const uint32_t a = span_first[f], b = span_first[f + 1];
      if (a == b) continue;
      const uint32_t one[2] = {0, b - a};
      uint32_t fo1[2] = {0, 0};
      tbk_soa_in t1;
      if (dev.api.bam_decode_file_spans(dev.ctx, 1, one, comp.data() + a, comp_bytes.data() + a, first_uoff.data() + a, last_uoff.data() + a, n_ref,
                                        inp.merged.data() + f, want_md, want_names, &t1, fo1) == TBK_EINVAL)
        GError("Error: %s: could not decode the chunks of %s its index names (%s): is the index the file's own?\n", plan.opt, plan.paths[f].c_str(), why.c_str());
    }
    GError("Error: %s: could not decode the chunks the indexes name (%s; first input: %s): is the index the file's own?\n", plan.opt, why.c_str(), plan.paths[0].c_str());
  }
  if (rc != 0) GError("Error: %s: decoding the chunks on the GPU failed: %s (first input: %s)\n", plan.opt, why_rc(dev, rc).c_str(), plan.paths[0].c_str());
  auto t_dec = tnow();
  const uint32_t n_decoded = tile.n_records;
  tbk_soa_in in;
  uint32_t n_kept = 0;
  if (plan.one) {
    rc = dev.api.tile_region(dev.ctx, &tile, plan.U.tid[0], plan.U.beg[0], plan.U.end[0], &in, fo.data(), &n_kept);
  } else {
    tbk_regions regs;
    regs.n = (uint32_t)plan.U.n(), regs.tid = plan.U.tid.data(), regs.beg = plan.U.beg.data(), regs.end = plan.U.end.data();
    rc = dev.api.tile_regions(dev.ctx, &tile, &regs, &in, fo.data(), &n_kept);
  }
  if (rc == TBK_ENOMEM || rc == TBK_E2BIG) too_large(rc);
  if (rc != 0) GError("Error: %s: GPU region filter failed: %s\n", plan.opt, why_rc(dev, rc).c_str());
  auto t_fil = tnow();
  spans.clear();
  DeviceTail T;
  memset(&T.res, 0, sizeof(T.res));
  T.t_col = T.t_rec = T.t_rel = t_fil;
  if (n_kept) {  // (a region without a record: header + EOF member)
    rc = device_tile_tail(dev, out, opt, env, &in, T);
    if (rc != 0) too_large(rc);
  } else {
    dev.api.bam_release(dev.ctx);
  }
  auto t3 = tnow();
  if (env.timing)
    fprintf(stderr,
            "region path ms: index queries %.1f (%zu regions) | chunk reads %.1f (%llu bytes in %zu chunks of %zu inputs, %llu bytes in all) | context up at %.1f | decode %.1f | "
            "filter %.1f (%u of %u records) | collapse %.1f | write %.1f\n",
            plan.ms_index, plan.U.n(), tms(t0, t_read), (unsigned long long)bytes_read, plan.n_chunks, k, (unsigned long long)inp.total, tms(dev.t_start, t_ctx), tms(t_ctx, t_dec),
            tms(t_dec, t_fil), n_kept, n_decoded, tms(t_fil, T.t_col), tms(T.t_col, t3));
  return account_whole(tot, T.res, tms(t0, t_dec), tms(t_dec, T.t_col), tms(T.t_col, t3));
}

// ---- streaming route: the inputs go through in tiles (TInputFiles::next_tile), and the OUTPUT side of tile i runs beside the input
// side of tile i + 1.  The inputs stream through in tiles of about TBK_TILE_RECORDS records, cut where no read of any input reaches
// across: exact — nothing the collapse computes crosses such a point — and host memory holds one tile's window of every input instead of
// the inflated files (the reference holds one record per input, tmerge.cpp:331-344).  A tile's representatives are copied out of the
// input windows right behind its collapse (the windows move on with the next tile); tags, deflate and the write of the tile then belong
// to a writer thread with a context of its own (the device writer, or every core under --writer host), while this thread inflates,
// decodes and collapses the next tile.  Two slots: a tile's arrays are free again once its members are in the file.
static void run_streaming(Device& dev, Output& out, const tbk_collapse_opts& opt, const Env& env, TInputFiles& inRecords, Totals& tot) {
  struct StreamSlot {
    RawBuf<uint32_t> rep;
    RawBuf<double> yc;
    RawBuf<int64_t> yx;
    RawBuf<int32_t> yd;
    RawBuf<uint8_t> blob;   // the representatives' raw records, group after group (no block_size)
    RawBuf<uint64_t> boff;  // [ng + 1]
    uint32_t ng = 0;
    bool busy = false;
  };
  StreamSlot slots[2];
  std::mutex sm;
  std::condition_variable scv;
  std::vector<int> queue_;   // slots handed to the writer, in tile order
  bool producer_done = false;
  double ms_writer_busy = 0, ms_wait_slot = 0, ms_gather = 0;
  tbk_ctx* wctx = nullptr;   // the writer's context (the collapse of the next tile keeps `ctx` busy)
  std::thread writer_thread;
  auto writer_main = [&]() {
    for (;;) {
      int si = -1;
      {
        std::unique_lock<std::mutex> lk(sm);
        scv.wait(lk, [&] { return !queue_.empty() || producer_done; });
        if (queue_.empty()) return;
        si = queue_.front();
        queue_.erase(queue_.begin());
      }
      StreamSlot& S = slots[si];
      auto a = tnow();
      const RecFn from_blob = [&S](uint32_t g) {
        tbh::RecView v;
        v.p = S.blob.data() + S.boff[g];
        v.len = (uint32_t)(S.boff[g + 1] - S.boff[g]);
        return v;
      };
      out.write(wctx, S.ng, S.rep.data(), S.yc.data(), S.yx.data(), S.yd.data(), 0, from_blob);
      ms_writer_busy += tms(a, tnow());
      {
        std::lock_guard<std::mutex> lk(sm);
        S.busy = false;
      }
      scv.notify_all();
    }
  };
  TbkTile tile;
  TInputFiles::TilePlan plan;
  const int nthreads = env.threads;
  int next_slot = 0;
  for (;;) {
    auto ti = tnow();
    const bool more = inRecords.next_tile(plan, env.tile_records, nthreads);
    tot.ms_inflate += tms(ti, tnow());
    if (!more) break;
    ++tot.n_tiles;
    auto t0 = tnow();
    inRecords.load_tile(tile, opt.strategy == TBK_STRAT_FULL, opt.collapse_same != 0, nthreads, &plan);
    auto t1 = tnow();
    tbk_soa_in in = tile.view();
    size_t n = tile.n();
    StreamSlot& S = slots[next_slot];
    {
      auto w0 = tnow();
      std::unique_lock<std::mutex> lk(sm);
      scv.wait(lk, [&] { return !S.busy; });
      ms_wait_slot += tms(w0, tnow());
    }
    tbk_groups_out res;
    size_results(&res, n, S.rep, S.yc, S.yx, S.yd);
    dev.wait();
    if (!writer_thread.joinable()) {
      if (dev.dw && dev.api.create(env.device, &wctx) != 0) wctx = nullptr;  // (no second context: the host writer takes the output)
      writer_thread = std::thread(writer_main);
    }
    tbk_collapse_opts copt = opt;
    const int rc = dev.api.collapse_tile(dev.ctx, &copt, &in, &res);
    auto t2 = tnow();
    if (rc == TBK_EUNSORTED) GError("Error: an input file is not coordinate-sorted!\n");
    if (rc != 0) GError("Error: GPU collapse failed: %s (%s)\n", dev.api.strerror_(rc), dev.api.last_error(dev.ctx));
    // the representatives leave the windows: sizes per slice of groups, a prefix, the copies — every core
    {
      const uint32_t ng = res.n_groups;
      S.ng = ng;
      S.boff.resize((size_t)ng + 1);
      const int T = ng < 8192 ? 1 : nthreads;
      std::vector<uint64_t> part((size_t)T + 1, 0);
      auto slice = [&](int t, uint32_t* a, uint32_t* b) {
        *a = (uint32_t)((uint64_t)ng * (uint32_t)t / (uint32_t)T);
        *b = (uint32_t)((uint64_t)ng * ((uint32_t)t + 1) / (uint32_t)T);
      };
      auto par = [&](const std::function<void(int)>& f) {
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(f, t);
        f(0);
        for (auto& x : th) x.join();
      };
      par([&](int t) {
        uint32_t a, b;
        slice(t, &a, &b);
        uint64_t by = 0;
        for (uint32_t g = a; g < b; ++g) by += inRecords.record(S.rep[g]).len;
        part[(size_t)t + 1] = by;
      });
      for (int t = 0; t < T; ++t) part[(size_t)t + 1] += part[(size_t)t];
      S.blob.resize((size_t)part[(size_t)T] + 16);
      par([&](int t) {
        uint32_t a, b;
        slice(t, &a, &b);
        uint64_t o = part[(size_t)t];
        for (uint32_t g = a; g < b; ++g) {
          const tbh::RecView v = inRecords.record(S.rep[g]);
          S.boff[g] = o;
          memcpy(S.blob.data() + o, v.p, v.len);
          o += v.len;
        }
      });
      S.boff[ng] = part[(size_t)T];
    }
    auto t3 = tnow();
    ms_gather += tms(t2, t3);
    tot.in += res.n_passed;
    tot.out += res.n_groups;
    inRecords.release_tile(plan);
    {
      std::lock_guard<std::mutex> lk(sm);
      S.busy = true;
      queue_.push_back(next_slot);
    }
    scv.notify_all();
    next_slot ^= 1;
    tot.ms_load += tms(t0, t1);
    tot.ms_gpu += tms(t1, t2);
  }
  if (writer_thread.joinable()) {
    {
      std::lock_guard<std::mutex> lk(sm);
      producer_done = true;
    }
    scv.notify_all();
    auto w0 = tnow();
    writer_thread.join();
    tot.ms_tag += tms(w0, tnow());
    if (wctx) dev.api.destroy(wctx);
    if (env.timing)
      fprintf(stderr, "streamed: %zu tiles; this thread inflate+index %.1f | SoA %.1f | collapse %.1f | gather representatives %.1f | waited for a free slot %.1f | "
                      "waited for the writer at the end %.1f; writer thread busy %.1f\n",
              tot.n_tiles, tot.ms_inflate, tot.ms_load, tot.ms_gpu, ms_gather, ms_wait_slot, tms(w0, tnow()), ms_writer_busy);
  }
}

// the track options and --index with --ranks: refused before the launcher starts (the multi-rank tracks and index are not built)
static void refuse_tracks_with_ranks(int argc, char* argv[]) {
  static const char* const value_longs[] = {"writer", "cov", "junc", "samp", "ranks", "regions-file", "bigwig-writer", "features", "summary", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", "strand-cov", nullptr};
  const int regions = count_value_option(argc, argv, "region", 'r', value_longs, "oNQFR");
  static const char* const value_longs_R[] = {"writer", "cov", "junc", "samp", "ranks", "region", "bigwig-writer", "features", "summary", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", "strand-cov", nullptr};
  const int region_files = count_value_option(argc, argv, "regions-file", 'R', value_longs_R, "oNQFr");
  static const char* const value_longs_S[] = {"writer", "cov", "junc", "samp", "ranks", "region", "regions-file", "bigwig-writer", "features", "summary", "thresholds", "depth-summary", "feature-depth", "gtf", "transcripts", nullptr};
  const int strand_covs = count_value_option(argc, argv, "strand-cov", 0, value_longs_S, "oNQFrR");
  const char* strand_prefix = nullptr;  // (the value as given, for the refusals that come before the launcher and before Args)
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "--strand-cov") == 0 && i + 1 < argc) strand_prefix = argv[i + 1];
    else if (strncmp(argv[i], "--strand-cov=", 13) == 0) strand_prefix = argv[i] + 13;
  }
  bool ranks = false, tracks = false, index = false, csi = false, tabix = false, summary = false, depth = false, transcripts = false;
  for (int i = 1; i < argc; ++i) {
    ranks = ranks || strcmp(argv[i], "--ranks") == 0 || strncmp(argv[i], "--ranks=", 8) == 0;
    tabix = tabix || strcmp(argv[i], "--tabix") == 0;
    index = index || strcmp(argv[i], "--index") == 0;
    csi = csi || strcmp(argv[i], "--csi") == 0;
    for (const char* o : {"--features", "--summary"}) {
      const size_t k = strlen(o);
      summary = summary || (strncmp(argv[i], o, k) == 0 && (argv[i][k] == 0 || argv[i][k] == '='));
    }
    for (const char* o : {"--thresholds", "--depth-summary", "--feature-depth"}) {
      const size_t k = strlen(o);
      depth = depth || (strncmp(argv[i], o, k) == 0 && (argv[i][k] == 0 || argv[i][k] == '='));
    }
    for (const char* o : {"--gtf", "--transcripts"}) {
      const size_t k = strlen(o);
      transcripts = transcripts || (strncmp(argv[i], o, k) == 0 && (argv[i][k] == 0 || argv[i][k] == '='));
    }
    for (const char* o : {"--cov", "--junc", "--samp", "--bigwig"}) {
      const size_t k = strlen(o);
      tracks = tracks || (strncmp(argv[i], o, k) == 0 && (argv[i][k] == 0 || argv[i][k] == '='));
    }
  }
  if (strand_covs) tbh::check_strand_cov(strand_prefix ? strand_prefix : "", strand_covs, ranks ? 2 : 1);
  if (ranks && tabix) GError("Error: --tabix is not available with --ranks (run tiecov --tabix on the output)\n");
  if (ranks && tracks) GError("Error: --cov / --junc / --samp / --bigwig are not available with --ranks (run tiecov on the output)\n");
  if (ranks && depth) GError("Error: --thresholds / --depth-summary / --feature-depth are not available with --ranks (run tiecov --depth-summary on the output)\n");
  if (ranks && summary) GError("Error: --features / --summary are not available with --ranks (run tiecov --features --summary on the output)\n");
  if (ranks && transcripts) GError("Error: --gtf / --transcripts are not available with --ranks (run tiecov --gtf --transcripts on the output)\n");
  if (ranks && index) GError("Error: --index is not available with --ranks (index the output afterwards)\n");
  if (ranks && csi) GError("Error: --csi is not available with --ranks (index the output afterwards)\n");
  if (regions > 1) GError("Error: -r / --region given more than once (one region per run)\n");
  if (ranks && regions) GError("Error: -r / --region is not available with --ranks\n");
  if (region_files > 1) GError("Error: -R / --regions-file given more than once (one file of regions per run)\n");
  if (region_files && regions) GError("Error: -R / --regions-file and -r / --region do not go together\n");
  if (ranks && region_files) GError("Error: -R / --regions-file is not available with --ranks\n");
}

int main(int argc, char* argv[]) {
  const Env env;
  refuse_tracks_with_ranks(argc, argv);
  spawn_ranks_launcher_if_asked(argc, argv, env);
  TInputFiles inRecords;
  inRecords.setup(VERSION, argc, argv);
  Args args(argc, argv, "help;debug;verbose;version;full;clip;exon;keep-supp;keep-secondary;keep-unmap;collapse-same;store-frac;writer=;cov=;junc=;samp=;bigwig;bigwig-writer=;tabix;index;csi;region=;regions-file=;features=;summary=;thresholds=;depth-summary=;feature-depth=;gtf=;transcripts=;strand-cov=;SMLPEDVho:N:Q:F:r:R:A");
  if (!args.error().empty()) {
    GMessage("%s\n%s\n", USAGE, args.error().c_str());
    return 1;
  }
  if (args.getOpt('h') || args.getOpt("help")) {
    fprintf(stdout, "%s", USAGE);
    return 0;
  }
  if (args.getOpt("version")) {
    fprintf(stdout, "%s\n", VERSION);
    return 0;
  }
  if (args.startNonOpt() == 0) {
    GMessage("%s", USAGE);
    GMessage("\nError: no input provided!\n");
    return 1;
  }
  const char* outfname = args.getOpt('o');
  if (!outfname || !*outfname) {
    GMessage("%s", USAGE);
    GMessage("\nError: output filename must be provided (-o)!\n");
    return 1;
  }
  tbk_collapse_opts opt;  // (tbk_collapse_opts_default: the library is not bound yet)
  memset(&opt, 0, sizeof(opt));
  opt.strategy = TBK_STRAT_CIGAR;
  opt.max_nh = INT32_MAX;
  opt.min_qual = -1;
  if (const char* s = args.getOpt('N')) opt.max_nh = atoi(s);
  if (const char* s = args.getOpt('Q')) opt.min_qual = atoi(s);
  if (const char* s = args.getOpt('F')) opt.flags_mask = (uint32_t)atoi(s);
  opt.keep_supplementary = (args.getOpt("keep-supp") || args.getOpt('S')) ? 1 : 0;
  opt.keep_secondary = args.getOpt("keep-secondary") ? 1 : 0;
  opt.keep_unmapped = (args.getOpt("keep-unmap") || args.getOpt('M')) ? 1 : 0;
  opt.collapse_same = (args.getOpt("collapse-same") || args.getOpt('A')) ? 1 : 0;
  opt.store_frac = args.getOpt("store-frac") ? 1 : 0;
  if (opt.store_frac && !opt.keep_secondary) GError("Error: --store-frac requires --keep-secondary to be enabled.\n");
  bool stratF = args.getOpt("full") || args.getOpt('L');
  bool stratP = args.getOpt("clip") || args.getOpt('P');
  bool stratE = args.getOpt("exon") || args.getOpt('E');
  if (stratF | stratP | stratE) {
    if (!(stratF ^ stratP ^ stratE)) GError("Error: only one merging strategy can be requested.\n");
    opt.strategy = stratF ? TBK_STRAT_FULL : (stratP ? TBK_STRAT_CLIP : TBK_STRAT_EXON);
  }
  if (args.getOpt("verbose") || args.getOpt('V')) {
    fprintf(stderr, "Running TieBrush " VERSION ". Command line:\n");
    args.printCmdLine(stderr);
  }
  bool dev_writer = true;
  if (const char* w = args.getOpt("writer")) {
    if (strcmp(w, "host") == 0) dev_writer = false;
    else if (strcmp(w, "device") != 0) GError("Error: --writer takes host or device\n");
  }
  if (opt.flags_mask != 0) GError("Error: -F is not supported by the GPU build (its reference semantics are unpinned)\n");
  if (opt.keep_unmapped) GError("Error: -M/--keep-unmap is not supported by the GPU build\n");
  const std::string cov_prefix = args.getOpt("cov") ? args.getOpt("cov") : "", junc_prefix = args.getOpt("junc") ? args.getOpt("junc") : "",
                    samp_prefix = args.getOpt("samp") ? args.getOpt("samp") : "";
  const bool bigwig = args.getOpt("bigwig") != nullptr;
  const std::string strand_prefix = args.getOpt("strand-cov") ? args.getOpt("strand-cov") : "";
  if (bigwig && cov_prefix.empty() && strand_prefix.empty()) GError("Error: --bigwig needs --cov\n");
  if (args.getOpt("bigwig-writer") && !bigwig) GError("Error: --bigwig-writer needs --bigwig\n");
  const bool bw_device = args.getOpt("bigwig-writer") && tbh::parse_bigwig_writer(args.getOpt("bigwig-writer"));
  const bool want_index = args.getOpt("index") != nullptr;
  if (want_index && strcmp(outfname, "-") == 0)
    GError("Error: --index needs an output file (-o FILE): an index addresses file offsets, standard output has none\n");
  const bool want_csi = args.getOpt("csi") != nullptr;
  if (want_csi && want_index) GError("Error: --csi and --index do not go together (their bins differ: one run builds one index)\n");
  if (want_csi && strcmp(outfname, "-") == 0)
    GError("Error: --csi needs an output file (-o FILE, not -o -): an index addresses file offsets, standard output has none\n");
  const bool tracks = !cov_prefix.empty() || !junc_prefix.empty() || !samp_prefix.empty() || !strand_prefix.empty();
  const bool tabix = args.getOpt("tabix") != nullptr;
  if (tabix && !tracks) GError("Error: --tabix needs at least one of --cov / --junc / --samp (it applies to their tracks)\n");
  if (tabix && !bigwig && (cov_prefix == "-" || cov_prefix == "stdout"))
    GError("Error: --tabix needs a coverage file (--cov PREFIX, not --cov %s): an index addresses file offsets, standard output has none\n", cov_prefix.c_str());
  // (--features serves --summary and --feature-depth: with neither, today's sentence)
  if (args.getOpt("summary") ? !args.getOpt("features") : (args.getOpt("features") && !args.getOpt("feature-depth")))
    GError("Error: --features BED and --summary OUT.tsv go together (%s is missing)\n", args.getOpt("summary") ? "--features" : "--summary");
  if (args.getOpt("transcripts") ? !args.getOpt("gtf") : args.getOpt("gtf") != nullptr)
    GError("Error: --gtf FILE and --transcripts OUT.tsv go together (%s is missing)\n", args.getOpt("transcripts") ? "--gtf" : "--transcripts");
  const bool depth = args.getOpt("thresholds") || args.getOpt("depth-summary") || args.getOpt("feature-depth");
  const bool summary = args.getOpt("summary") != nullptr || depth || args.getOpt("transcripts") != nullptr;  // (what needs the output's rows and its header up front)
  const char* region = args.getOpt('r') ? args.getOpt('r') : args.getOpt("region");
  const char* regions_file = args.getOpt('R') ? args.getOpt('R') : args.getOpt("regions-file");
  const bool regional = region || regions_file;
  const char* ropt = regions_file ? "-R" : "-r";
  while (const char* ifn = args.nextNonOpt()) {
    if (regional && strcmp(ifn, "-") == 0) GError("Error: %s: the input - (standard input) has no index; %s takes BGZF-compressed BAM files\n", ropt, ropt);
    inRecords.addFile(tbh_realpath(ifn).c_str());
  }

  // -r REGION: the inputs are opened, the region resolved against the merged header and every input's index queried BEFORE the device
  // is brought up or any output file exists (plan_region's refusals)
  std::unique_ptr<RegionPlan> rplan;
  const Clock t_begin = tnow();
  if (regional) {
    refuse_region_inputs(inRecords, true, ropt);
    inRecords.name_ref_file = true;
    inRecords.start();
    refuse_region_inputs(inRecords, false, ropt);
    rplan.reset(new RegionPlan(plan_region(inRecords, region, regions_file)));
  }
  // --features / --summary: the BED file is read (and refused) against the output's header before any output file exists — and before
  // the device's helper thread does: a refusal leaves through exit(), which must not run beside a thread that is bringing the runtime up
  // (so a summary run opens its inputs ahead of the device, as a region run does)
  tbh::SummaryJob sjob;
  tbh::DepthJob djob;
  tbh::TxJob xjob;
  if (summary) {
    if (!regional) inRecords.start();
    sjob.setup(args.getOpt("summary") ? args.getOpt("features") : nullptr, args.getOpt("summary"), *inRecords.header(), rplan ? &rplan->U : nullptr);
    djob.setup(args.getOpt("thresholds"), args.getOpt("depth-summary"), args.getOpt("feature-depth"), args.getOpt("features"), *inRecords.header(), rplan ? &rplan->U : nullptr);
    xjob.setup(args.getOpt("gtf"), args.getOpt("transcripts"), *inRecords.header(), rplan ? &rplan->U : nullptr);
  }
  Device dev(env, opt, dev_writer, tracks || summary, regional || summary ? t_begin : tnow());
  if (!regional && !summary) inRecords.start();
  auto t_ctx = tnow();
  Totals tot;
  // the tracks: the output header's sample lines (load_sample_info, commons.h:47-71) are checked before any work, the files opened
  std::unique_ptr<tbh::CovRecs> trecs;
  tbh::TrackFiles tfiles;
  int num_samples = 0;
  if (tracks) {
    sam_hdr_t* h = inRecords.header();
    if (!samp_prefix.empty()) {
      num_samples = (int)h->co_samples().size();
      if (num_samples == 0) GError("Error: no sample lines found in header");
    }
    tbh::TrackOptions topt;
    topt.cov = cov_prefix, topt.junc = junc_prefix, topt.samp = samp_prefix, topt.bigwig = bigwig, topt.bw_device = bw_device, topt.tabix = tabix;
    topt.strand_cov = strand_prefix;
    tfiles.open(topt, h->target_name, h->target_len);
  }
  if (tracks || summary) trecs.reset(new tbh::CovRecs());
  // the index: a reference a BAI cannot address is refused before the output is created; an older index of the same name goes now
  tbh::BaiIndex bai;
  if (want_index) {
    std::string err;
    if (!bai.init(inRecords.header()->target_name, inRecords.header()->target_len, err)) GError("Error: --index: %s\n", err.c_str());
    (void)unlink((std::string(outfname) + ".bai").c_str());
  }
  if (want_csi) {  // (any header: the depth follows its longest reference)
    std::string err;
    if (!bai.init_csi(inRecords.header()->target_name, inRecords.header()->target_len, err)) GError("Error: --csi: %s\n", err.c_str());
    (void)unlink((std::string(outfname) + ".csi").c_str());
  }
  Output out(outfname, inRecords.header(), dev, env, trecs.get(), want_index || want_csi ? &bai : nullptr);
  const Inputs inp(inRecords);
  const Routes can = eligible_routes(env, opt, inp);
  Route r = Route::fall_through;
  if (rplan) r = run_region(dev, out, opt, env, inp, *rplan, inRecords.header()->n_targets, tot);
  else if (can.hybrid) r = run_hybrid(dev, out, opt, env, inp, tot);
  else if (can.whole_host) r = run_whole_host(dev, out, opt, env, inp, tot);
  if (r == Route::fall_through && can.device_decode) r = run_device_decode(dev, out, opt, env, inp, tot);
  if (r == Route::fall_through) run_streaming(dev, out, opt, env, inRecords, tot);
  if (env.timing) fprintf(stderr, "tiles: %zu (at %.1f ms)\n", tot.n_tiles, tms(dev.t_start, tnow()));
  out.close();
  if (trecs) {
    dev.wait();
    // the tracks of the whole output, as tiecov computes them from its decode of the file; the text by tbk_format_track (the host
    // formatter when the device formatter refuses a value, or with TBK_TRACK_HOST_FMT)
    const auto t0 = tnow();
    tbh::TrackTimes tt;
    tbh::TrackRun run;
    run.num_samples = num_samples, run.bw_device = bw_device, run.summary = &sjob, run.depth = &djob, run.transcripts = &xjob, run.device_text = !env.track_host_fmt, run.times = &tt;
    tbh::run_tracks(track_api(dev), trecs->as_cov_in(), inRecords.header()->target_name, tfiles, run);
    if (env.timing)
      fprintf(stderr, "tracks ms: %zu records | coverage call %.1f | sample call %.1f | text + write %.1f (%d of the tracks by the host formatter) | total %.1f\n",
              trecs->tid.size(), tt.ms_cov, tt.ms_samp, tt.ms_text, tt.host_tracks, tms(t0, tnow()));
  }
  auto t_closed = tnow();
  if (env.timing) fprintf(stderr, "writer closed at %.1f ms\n", tms(dev.t_start, t_closed));
  dev.wait();
  // (no tbk_destroy / stop: the process ends below, the OS reclaims device and host memory faster than piecewise frees)
  if (env.timing && out.dev_z)
    fprintf(stderr, "device writer: %.1f MB of tagged records -> %.1f MB of BGZF members in %.1f ms\n", out.dev_payload / 1e6, out.dev_z / 1e6, out.ms_dev_write);
  if (env.timing)
    fprintf(stderr, "timing ms: open+context %.1f | inflate+index %.1f | SoA %.1f | collapse (PCIe incl.) %.1f | tag+queue %.1f | total to writer close %.1f\n",
            tms(dev.t_start, t_ctx), tot.ms_inflate, tot.ms_load, tot.ms_gpu, tot.ms_tag, tms(dev.t_start, t_closed));
  double p = 100.00 - (double)(tot.out * 100.00) / (double)tot.in;
  if (rplan && !tot.in) p = 0.0;  // (-r: a region without a record; without -r the line is what it always was)
  GMessage("%ld input records written as %ld (%.2f%% reduction)\n", (long)tot.in, (long)tot.out, p);
  fflush(stdout);
  fflush(stderr);
  // the gigabytes of the whole-input routes go back in parallel: a process that just exits returns them in one thread while its
  // caller waits (measured: 0.17 s for 2.7 GB)
  {
    auto a = tnow();
    tbh::big_release_all(env.threads);
    if (env.timing) fprintf(stderr, "released the large buffers in %.1f ms\n", tms(a, tnow()));
  }
  if (env.exit_timing >= 0) {  // (diagnosis: what is left of the process exit)
    auto a = tnow();
    if (env.exit_timing > 1) dev.api.destroy(dev.ctx);
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    fprintf(stderr, "exit timing: tbk_destroy %.1f ms; _exit at %.3f\n", tms(a, tnow()), (double)ts.tv_sec + ts.tv_nsec * 1e-9);
    if (env.exit_timing > 2) return 0;  // (a plain return: what a profiler's exit handlers need to write their traces)
  }
  _exit(0);  // the output is closed and flushed: skip the runtime's teardown of a process that is done (tens of ms of hipFree / unload)
}
