// record_pass.h -- the host frame of the record passes: ngsld_prune (prune.hip), ngsld_decay (decay.hip), ngsld_blocks
// (blocks.hip), ngsld_site_ld (site_ld.hip), ngsld_clusters (cluster.hip), ngsld_grid (grid.hip), ngsld_linked_pairs (linked.hip)
// and ngsld_scan (scan.hip) read the records of rows chunk
// by chunk and run a kernel of their own over each chunk's items (ld_records.h).  What they share on the host is here, once: the
// site filter's arrays (SiteFilter), the chunk loop (RecordPass), the refusals of a value or a sum out of range, the sum / max /
// linked accumulators of site LD and the grid, a label's CHR:pos.  The kernels share nothing of it: their filters differ -- but for
// ngsld_decay and ngsld_decay_map (decay_map.hip), whose filter is one and which run one kernel (ld_decay_bins.h).
// (ngsld_scan uses the site filter, the chunk loop, the two refusals and the guard of the sums; ngsld_cross_ld (cross.hip) all of
// it, as the grid does.)
// The chunk loop takes a list of passes: the pairs of a chunk run once and every pass of the list reads them (ngsld_analyze,
// analyze.hip); the six passes it can list are AnalysisPass objects, and their single calls are a list of one.
// Host code; the definitions are in record_pass.hip.
#pragma once

#include <memory>

#include "engine.h"
#include "ld_records.h"

namespace ngsld {
namespace eng {

// ---- the site filter: dist from prefix sums, the maf filter on the printed maf ----
// The host arrays of dist_prefix (engine.h), maf_ok[s] = the maf of site s is a number that prints as >= min_maf, and their
// copies on the device for a kernel's argument struct.
struct SiteFilter {
  std::vector<double> cum;
  std::vector<uint32_t> infc;
  std::vector<uint8_t> maf_ok;  // empty unless a min_maf was given
  bool exact_gaps = false;      // integer gaps >= 0: cum[s2] - cum[s1] is the dist the TSV prints
  DevBuf<double> d_cum;
  DevBuf<uint32_t> d_infc;
  DevBuf<uint8_t> d_maf_ok;

  // the host arrays; min_maf null: no maf filter (ngsld_prune)
  void prepare(const ngsld_ctx *c, const double *min_maf);
  // a finite limit on dist needs exact_gaps: "<pass> max_kb_dist needs integer position gaps" otherwise
  int check_limit(ngsld_ctx *c, const char *pass, double limit) const;
  // the device copies (blocking: the arrays are pageable)
  int upload(ngsld_ctx *c);
};

// ---- the chunk loop ----
// records of one chunk of rows (32 B each)
constexpr uint64_t kRecordChunkPairs = 1ull << 24;
// the chunk of a pass: kRecordChunkPairs, or a test knob's smaller value (knob: test_knob("NAME") or null)
inline uint64_t record_chunk(const char *knob) {
  return knob ? std::max<uint64_t>(1, std::min<uint64_t>(kRecordChunkPairs, std::strtoull(knob, nullptr, 10))) : kRecordChunkPairs;
}

// the items of one launch of a pass's kernel: a launch's grid stays below 2^32 threads at one wavefront per item (2^24 items), or
// NGSLD_TEST_RECORD_SLICE_ITEMS if that is fewer (tests: a chunk's items in many launches)
inline uint64_t record_slice_items() {
  uint64_t max_items = (1ull << 22) * 4;
  if (const char *e = test_knob("RECORD_SLICE_ITEMS")) max_items = std::min<uint64_t>(max_items, std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)));
  return max_items;
}

// two events that bracket device work on the context's stream; add_elapsed: *ms += their span once the second has passed
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(const EventPair &) = delete;
  EventPair &operator=(const EventPair &) = delete;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  hipError_t create() {
    hipError_t e = hipEventCreate(&a);
    return e == hipSuccess ? hipEventCreate(&b) : e;
  }
  hipError_t add_elapsed(double *ms) const {
    float t = 0.f;
    const hipError_t e = hipEventElapsedTime(&t, a, b);
    if (e == hipSuccess) *ms += t;
    return e;
  }
};

// a chunk: the consecutive rows [r0, r1), their pairs, the global index of its record 0 (a kernel's out_base)
struct RecordChunk {
  uint64_t r0, r1, pairs, out_base;
};

// The rows of one or several passes, chunk by chunk, through the pair kernels -- once -- into one record buffer, and every
// pass's kernel over each chunk's items.
struct RecordPass {
  // launch(chunk, items, n_items): the pass's kernel over one slice of the chunk's items (device pointer)
  using Launch = std::function<void(const RecordChunk &, const ngsld_item *items, uint64_t n_items)>;
  // before(chunk): the chunk's records are final, nothing of the pass is launched yet (outside the events);
  // after(chunk): once the chunk's launches are done (the next chunk's pairs overwrite the records)
  using Step = std::function<int(const RecordChunk &)>;
  // A pass as the chunk loop sees it: its three hooks, where its kernel time goes, and the events that bracket its launches.
  // A client without a launch has nothing to read (a pass with no bin to fill): the loop passes it by.
  struct Client {
    Step before;
    Launch launch;
    Step after;
    double *kernel_ms = nullptr;  // where the span of its events adds (a field of its stats)
    double kernel_total_ms = 0;   // the same span, for the list's total
    EventPair ev;
  };
  // what the clients share: the wall time of the pair phase, the chunks, the pairs handed to ngsld_run_device
  struct Shared {
    double pairs_ms = 0;
    uint64_t chunks = 0, pairs_run = 0;
  };

  // The record buffer.  The rows: every row, or the rows s with rows[s] != 0 (it must outlive run).  Chunks of
  // consecutive rows of up to chunk_pairs records; a row is never cut, so the buffer holds the chunk (at most the rows' pairs)
  // or the longest row where that is longer -- or, with fit_longest_row false, just chunk_pairs records: a longer row is refused
  // in run ("a row of N pairs does not fit the record buffer").  with_ext: a second buffer of as many 40 B records, which the pair
  // kernels fill as the plan's extend_out has them (ngsld_linked_pairs prints them).
  int open(ngsld_ctx *c, uint64_t chunk_pairs, const uint8_t *rows = nullptr, bool fit_longest_row = true, bool with_ext = false);
  // Every chunk: ngsld_run_device + ngsld_finish_device on the context's stream, once, so every record is final (replayed pairs
  // carry their replayed values); then the clients in list order, each: its before; its launch for each slice of the chunk's
  // items, every slice below 2^32 threads at one wavefront per item (2^24 items, or NGSLD_TEST_RECORD_SLICE_ITEMS if that is
  // fewer), all of them between its two events; the wait for the second, whose span adds to its kernel_ms; then its after.
  // Nothing runs when no client has a launch.  *shared (when not null) adds the pair phase's wall time, chunks and pairs.
  int run(Client *const *clients, size_t n_clients, Shared *shared);
  // a list of one, from its parts (ngsld_blocks, ngsld_linked_pairs)
  int run(double *pairs_ms, double *kernel_ms, uint64_t *chunks, const Step &before, const Launch &launch, const Step &after = nullptr);
  ngsld_rec_std *records() const { return d_rec.p; }
  ngsld_rec_ext *ext_records() const { return d_ext.p; }  // null unless opened with_ext
  void close() {
    d_rec.release();
    d_ext.release();
  }

 private:
  ngsld_ctx *c = nullptr;
  uint64_t chunk_pairs = 0;
  const uint8_t *rows = nullptr;
  DevBuf<ngsld_rec_std> d_rec;
  DevBuf<ngsld_rec_ext> d_ext;
};

// ---- a pass in four parts ----
// ngsld_prune, ngsld_decay, ngsld_site_ld, ngsld_clusters, ngsld_grid and ngsld_scan are each one object of this shape, so that
// the single calls and ngsld_analyze (analyze.hip) drive the same code: run_passes below over a list of one, or of several.
struct AnalysisPass {
  RecordPass::Client client;
  virtual ~AnalysisPass() = default;
  // the parameters (host only, no device is touched): the single call's codes and messages
  virtual int validate(ngsld_ctx *c) = 0;
  // the context's store of this kind, emptied: its getters answer as before any call
  virtual void clear(ngsld_ctx *c) = 0;
  // the site arrays, the device buffers and their uploads, the track_* decisions, the hooks of `client`; chunk_pairs is the
  // chunk the records will come in
  virtual int prepare(ngsld_ctx *c, uint64_t chunk_pairs) = 0;
  // false: the record buffer holds chunk_pairs records and a longer row is refused (pruning)
  virtual bool fit_longest_row() const { return true; }
  // the record buffer, open now, that the hooks read
  virtual void bind(ngsld_rec_std *records) = 0;
  // the copy back, the guards of the sums, the store in the context, the stats (the record buffer is closed by now)
  virtual int finish(ngsld_ctx *c, const RecordPass::Shared &shared) = 0;
};
// prepare each, one RecordPass over all their clients, finish each; the first failure ends it
int run_passes(ngsld_ctx *c, AnalysisPass *const *passes, size_t n, uint64_t chunk_pairs, RecordPass::Shared *shared);
// a single call: validate, then a list of one
int run_single(ngsld_ctx *c, AnalysisPass &pass, uint64_t chunk_pairs);
std::unique_ptr<AnalysisPass> make_prune_pass(const ngsld_prune_params *p, const char *const *labels, uint8_t *site_state, ngsld_prune_stats *stats);
std::unique_ptr<AnalysisPass> make_decay_pass(const ngsld_decay_params *p, ngsld_decay_stats *stats);
std::unique_ptr<AnalysisPass> make_site_ld_pass(const ngsld_site_ld_params *p, ngsld_site_ld_stats *stats);
std::unique_ptr<AnalysisPass> make_clusters_pass(const ngsld_clusters_params *p, ngsld_clusters_stats *stats);
std::unique_ptr<AnalysisPass> make_grid_pass(const ngsld_grid_params *p, const char *const *labels, ngsld_grid_stats *stats);
std::unique_ptr<AnalysisPass> make_scan_pass(const ngsld_scan_params *p, ngsld_scan_stats *stats);

// ---- what the entries share ----
// the refusals every pass makes once its own parameters have passed, the device, the zeroed stats
template <class S>
int begin_pass(ngsld_ctx *c, S &stats) {
  if (c->n_sites >= 0xffffffffull) return fail(c, NGSLD_ERR_UNSUPPORTED, "n_sites must be below 2^32 - 1");
  HIP_TRY(c, hipSetDevice(c->device));
  std::memset(&stats, 0, sizeof(stats));
  stats.struct_size = sizeof(stats);
  return NGSLD_OK;
}

// a kernel's meta[0] != 0: (s1 << 32 | s2) + 1 of a pair whose printed value does not fit the micro-units (ld_prune.h)
int fail_value_range(ngsld_ctx *c, const char *pass, unsigned long long meta0);

// Sums of integer micro-units are exact while max |q| * (the rows of a sum) < 2^63: certain below 2^25 rows (|q| < 2^38), where
// the kernels do not track max |q| at all.  True when a sum of `rows` values of up to max_q may have wrapped.
// NGSLD_TEST_SUM_WRAP_LIMIT = L (tests; 1 <= L <= 2^63): the limit is L instead of 2^63, and track_sums holds whatever the
// job's size, so that a small job runs the tracking of a large one and the kernels' max |q| can be pinned to the unit.
inline bool sum_may_wrap(unsigned long long max_q, uint64_t rows) {
  unsigned __int128 limit = (unsigned __int128)1 << 63;
  if (const char *e = test_knob("SUM_WRAP_LIMIT")) limit = std::max<uint64_t>(1, std::min<uint64_t>(1ull << 63, std::strtoull(e, nullptr, 10)));
  return max_q > 0 && (unsigned __int128)max_q * rows >= limit;
}
// whether a pass tracks max |q|: `large` is its own condition (a sum of 2^25 rows or more, a row longer than a chunk)
inline bool track_sums(bool large) { return large || test_knob("SUM_WRAP_LIMIT") != nullptr; }

// One entry of the accumulators of ngsld_site_ld and ngsld_grid, acc[1 + 3 * fields][n] (rows; then per field the int64 sum in
// two's complement, the biased maximum, the linked rows): field v of entry k, which has rows > 0.  The mean is the double nearest
// to sum / (10^6 * rows): one rounding (ld_mean.h).
struct FieldSummary {
  int64_t sum, max;
  uint64_t linked;
  double mean;
};
inline FieldSummary field_summary(const unsigned long long *acc, size_t n, int v, size_t k) {
  const unsigned long long *a = acc + (size_t)(1 + 3 * v) * n + k;
  const uint64_t rows = acc[k];
  const int64_t sum = (int64_t)a[0];
  const double m = mean_nearest(sum < 0 ? (uint64_t)0 - (uint64_t)sum : (uint64_t)sum, rows);
  return {sum, (int64_t)(a[n] - kMaxBias), a[2 * n], sum < 0 ? -m : m};
}

// A site's label as ngsld_blocks and ngsld_grid read it: the key is the label up to its first TAB (a pos file with extra columns
// puts them behind one), CHR:num with the colon at `colon` (npos: no colon, the whole key is CHR).  Nothing more is built per
// label than the key: a pass over 100,000 labels that are mostly on another chromosome pays for no more.
struct LabelPos {
  std::string key;
  size_t colon;
  bool on(const std::string &chr) const { return key.compare(0, colon, chr) == 0; }
  std::string chr() const { return key.substr(0, colon); }
  // num as a position: 1 to 19 plain decimal digits, or false
  bool position(uint64_t *pos) const;
};
LabelPos label_pos(const char *label);

}  // namespace eng
}  // namespace ngsld
