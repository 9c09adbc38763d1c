// collapse_plan.hpp — which route a tile takes through the collapse stage (collapse.hip: tbk_collapse_device) and where it goes when
// that route hands it on.  Pure host arithmetic on a few facts about the tile: no HIP, no project header, so that it compiles with a
// plain C++ compiler and is tested without a GPU (tests/test_collapse_plan_cpu.py against tests/route_model.py).  The same plan sizes
// tbk_collapse_tile's arena hint (tbk_api.hip).
#pragma once
#include <stdint.h>

// the route's numbers are tbk_last_route's (include/tbk.h: TBK_ROUTE_*), the error bits the device's (tbk_internal.h: TBK_DERR_*), the
// strategy tbk.h's TBK_STRAT_FULL: collapse.hip asserts that they agree
enum : int { COLP_ROUTE_RAW_WINDOW = 1, COLP_ROUTE_COMPACTED_WINDOW = 2, COLP_ROUTE_SORT = 3 };
enum : uint32_t { COLP_ERR_COLLISION = 1u << 1, COLP_ERR_FRACTIONAL = 1u << 5, COLP_ERR_BIGBUCKET = 1u << 8, COLP_ERR_RAWORDER = 1u << 9 };
enum : int { COLP_STRAT_FULL = 1 };

// The run-merge sort (msort.hip): ceil(log2(files)) merge rounds + one local pass against ~12 radix passes.  Measured on MI355X:
// 2 files x 1 M 0.17 ms vs 0.47 ms; 16 files x 0.5 M: whole step 3.90 vs 4.13 ms; 64 files x 0.25 M (6 rounds): 8.58 vs 8.67 ms —
// level there, so more files than that take the radix sort.
constexpr uint32_t COLP_RUNS_MAX_FILES = 64;
constexpr uint32_t COLP_RUNS_MIN_RECORDS = 32768;  // below this the tile is launch-bound either way; keep the one code path
// The window path (wgroup.hip) takes tiles of at most this many files (the runs' offsets of a block lie in LDS)
constexpr uint32_t COLP_WINDOW_MAX_FILES = 1024;
// Small tiles of a few files are launch-bound either way and the lean run-sort path needs no read-back: it keeps them.  The window
// path takes a tile from this many records on, or — with more files than the run-merge sort takes — from that many
constexpr uint32_t COLP_WINDOW_MIN_RECORDS = 8u << 20;
constexpr uint32_t COLP_WINDOW_MIN_RECORDS_MANY_FILES = 65536;
// Group partials of other ranks (the PART form): at most this many source ranks; smaller tiles keep the sort path
constexpr uint32_t COLP_PART_MAX_FILES = 64;
constexpr uint32_t COLP_PART_MIN_RECORDS = 65536;
// the raw window kernels address a record's fields by 32-bit byte offsets: fewer records and CIGAR words than this
constexpr uint32_t COLP_RAW_MAX_ITEMS = 1u << 30;

inline bool collapse_window_supported(uint32_t k) { return k >= 1 && k <= COLP_WINDOW_MAX_FILES; }

// Everything the decision reads, and nothing else.
struct CollapsePlanIn {
  uint32_t n_records = 0, n_cigar_ops = 0, n_files = 0;
  // tbk_soa_in::tbmerged, scanned once by the caller: no file is TieBrush-merged (or there is no array), every file is, some file is
  bool tbm_none = true, tbm_all = false, tbm_any = false;
  bool has_prio = false;     // explicit merge priorities (prio_hi and prio_lo)
  bool has_carried = false;  // carried tags (yc_in, yx_in and yd_in)
  int strategy = 0, store_frac = 0, collapse_same = 0;
  int path = 0, raw = -1, sort = 0;  // the debug keys path= / raw= / sort= (TbkDebug)
};

struct CollapsePlan {
  int route = COLP_ROUTE_SORT;  // the first route of the tile (COLP_ROUTE_*)
  bool part = false;            // raw window route: the records are group partials of other ranks (wgroup.hip: the PART form)
  bool use_runs = false;        // sort route: the run-merge sort orders the records (else the radix sort) ...
  uint32_t runs_min = COLP_RUNS_MIN_RECORDS;  // ... when at least this many pass the filter
  bool lean = false;            // sort route: nothing is read back before the one synchronisation at its end
};

inline CollapsePlan collapse_plan(const CollapsePlanIn& in) {
  CollapsePlan p;
  const uint32_t n = in.n_records, k = in.n_files;
  p.use_runs = k <= COLP_RUNS_MAX_FILES;
  if (in.sort) {  // test hook: sort=radix / runs force one path whatever the shape
    p.use_runs = in.sort != 1 && (p.use_runs || in.sort == 2);
    if (in.sort == 2) p.runs_min = 0;
  }
  // The window path goes from the runs to the groups without sorting the records; it covers plain BAM inputs with integral YC (the
  // ordered / carried-tag cases keep the sort path, which has the per-record order they need).
  const bool plain = !in.store_frac && !in.collapse_same;
  const bool win_ok = collapse_window_supported(k) && plain && in.tbm_none;
  bool use_win = win_ok && (n >= COLP_WINDOW_MIN_RECORDS || (k > COLP_RUNS_MAX_FILES && n >= COLP_WINDOW_MIN_RECORDS_MANY_FILES));
  if (in.path == 1) use_win = false;  // test hook: path=sort keeps the sort path,
  if (in.path == 2) use_win = win_ok;  // path=window takes the window path whatever the size
  // Group partials of other ranks (multi-GPU owner side): every "file" is the run of one source rank, all flagged
  // TieBrush-merged, with explicit priorities — the window path in its PART form (wgroup.hip) is the reduce-by-key.  Small tiles
  // and anything that form cannot hold (TBK_DERR_FRACTIONAL) keep the sort path, which treats them as TieBrush-merged inputs.
  p.part = in.tbm_all && in.has_prio && in.has_carried && k <= COLP_PART_MAX_FILES && plain && in.strategy != COLP_STRAT_FULL &&
           in.path != 1 && (n >= COLP_PART_MIN_RECORDS || in.path == 2);
  if (p.part) use_win = true;
  // Raw window path: plain tiles without an explicit merge priority go from the input records straight to the groups — the key
  // pass, the effective-end scan and the compaction are folded into the window kernels (raw=0: test hook, keeps them apart)
  bool use_raw = use_win && (in.raw != 0 || p.part);  // (the PART form exists in raw mode only)
  if (n >= COLP_RAW_MAX_ITEMS || in.n_cigar_ops >= COLP_RAW_MAX_ITEMS) {
    use_raw = false;
    if (p.part) p.part = false, use_win = false;
  }
  p.route = use_raw ? COLP_ROUTE_RAW_WINDOW : use_win ? COLP_ROUTE_COMPACTED_WINDOW : COLP_ROUTE_SORT;
  // Every kernel reads the record / group counts from the device scalars, so the host only needs them where it must size something
  // by them.  "Lean" tiles — plain BAM inputs on the run-sort path, integral YC — need that nowhere: grids and arrays take the upper
  // bound n, nothing is read back until the single synchronisation at the end, and the rare events that want a different path (a
  // bucket too long for the local sort, a key-hash collision) simply restart the tile.
  p.lean = p.use_runs && !in.store_frac && !in.tbm_any && n >= p.runs_min;
  return p;
}

// tbk_collapse_tile's arena hints: the raw window form works on the input where it lies and needs half of what the other routes
// keep per record.  Only where nothing but the tile's shape chose that form: a device-resident tile without explicit priorities,
// no path= / raw= key.
inline bool collapse_arena_lean(const CollapsePlanIn& in, const CollapsePlan& p, bool input_on_device) {
  return input_on_device && !in.has_prio && in.path == 0 && in.raw < 0 && p.route == COLP_ROUTE_RAW_WINDOW;
}

// What the driver does when a route comes back with the device's error bits.
enum : int { COLP_DONE = 0, COLP_RESEED, COLP_RESTART, COLP_ERROR };
struct CollapseNext {
  int action = COLP_DONE;
  CollapsePlan plan;             // COLP_RESTART: the plan to go on with (any other answer: the plan that ran)
  bool raw_handed_back = false;  // for tbk_last_route: the raw form refused the input; a pile-up sent the tile to the sort path
  bool big_bucket = false;
};

// The hand-over table (DESIGN.md §3 has it as a table).  Every restart leads to a route further down — raw window, compacted window,
// lean sort, sort — so a tile restarts three times at the most.
inline CollapseNext collapse_plan_after(const CollapsePlan& ran, uint32_t err_bits) {
  CollapseNext r;
  r.plan = ran;
  const bool big = (err_bits & COLP_ERR_BIGBUCKET) != 0;
  int to = 0;
  switch (ran.route) {
    case COLP_ROUTE_RAW_WINDOW:
      // a pile-up beyond the group table, or (PART) a carried value the form cannot hold: the sort path
      if (err_bits & (COLP_ERR_BIGBUCKET | COLP_ERR_FRACTIONAL)) to = COLP_ROUTE_SORT;
      // not the raw form's kind of input: the general front end decides what is an error (group partials have the sort path only)
      else if (err_bits & COLP_ERR_RAWORDER) to = ran.part ? COLP_ROUTE_SORT : COLP_ROUTE_COMPACTED_WINDOW;
      r.raw_handed_back = to && (err_bits & COLP_ERR_RAWORDER);
      r.big_bucket = to && big;
      break;
    case COLP_ROUTE_COMPACTED_WINDOW:
      // a pile-up with more distinct alignments than the LDS table holds: the sort path
      if (big) to = COLP_ROUTE_SORT, r.big_bucket = true;
      break;
    default:
      // lean run sort, a bucket longer than the local sort's window: the same keys on the radix path, counts read back
      // (the run sort that is not lean redoes the order itself, on the merged runs: it never reports the bit)
      if (big && ran.lean) to = COLP_ROUTE_SORT, r.plan.use_runs = false, r.plan.lean = false;
      break;
  }
  if (to) {
    r.action = COLP_RESTART;
    r.plan.route = to;
    r.plan.part = false;
  } else if (err_bits & COLP_ERR_COLLISION) {  // a key-hash collision, on any route: the next seed
    r.action = COLP_RESEED;
  } else if (err_bits) {  // anything else is the input's fault
    r.action = COLP_ERROR;
  }
  return r;
}
