// scan.hip -- the LD scan on the device (ngsld_scan, include/ngsld.h): a window centred on every site, the rows inside it split
// at the site into left-left, right-right and across -- Kelly's ZnS and Kim and Nielsen's omega per site -- from the pair records
// where they are computed; no TSV, a few numbers per site leave the device.  SCAN.md has the rule, the refusals and why the sums
// are exact.
//
//   windows  the host walks the dist prefix sums with two pointers: the window of site c is the index range [a_c, b_c]
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   scan     one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the
//            filters of site LD, each chosen field as |its printed value| in integer micro-units (ld_prune.h).  A counted row
//            (i, j) is in the windows of a contiguous range of centre sites per class -- LL [j, b_i], RR [a_j, i - 1], LR
//            [max(a_j, i), min(b_i, j - 1)] -- so it is three range-adds into difference arrays: +v where the range begins, -v
//            one past its end.  Inside an item i is shared and j consecutive: four of the lanes' six end points fall in a few
//            runs of one index, two (j, and min(b_i + 1, j) where j <= b_i) are mostly a word a lane.  A segmented scan merges
//            each run and its last lane adds once (decay.hip's scheme, which does not rely on the order of the keys), with
//            global 64-bit atomics that wrap: up to 2 x 64 coalesced adds per word of an item, plus a few
//   sums     after the last chunk an inclusive prefix sum over each difference array (hipcub), exact modulo 2^64 and hence exact
//            where the true window sum is in range, which the guard of SITES.md ensures; one copy back
//   host     zns is the double nearest to sum / (10^6 * rows) (mean_nearest), omega the double nearest to the exact ratio
//            (ratio_nearest, ld_mean.h)
#include <hipcub/hipcub.hpp>

#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

enum { kLL = 0, kRR = 1, kLR = 2 };

struct ScanArgs {
  const ngsld_item *items;    // the items of this launch
  uint64_t n_items;
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  const uint32_t *win_a;      // the window of site c is [win_a[c], win_b[c]]
  const uint32_t *win_b;
  double limit;               // dist <= limit (+inf: no limit)
  uint32_t n_sites;
  int ns;                     // chosen fields
  int field[4];               // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int track_max;              // a window may hold 2^25 rows or more: max |q| goes to meta[1]
  unsigned long long *acc;    // [3 classes][1 + ns][n_sites + 1] difference arrays: rows, then the sums of each field
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] counted rows
};

// One end of the lanes' ranges in one class: every lane that is `on` adds (1, q[]) -- or their negatives -- at word `key` of
// the class's difference arrays.  Runs of one key are numbered from lane 0, a segmented inclusive scan leaves a run's totals in
// its last lane, and that lane adds once.  A lane that is not on carries zeros under whatever key it has: it may split a run,
// never change a sum.  Every lane of the wavefront takes part in every shuffle.
__device__ __forceinline__ void add_at(const ScanArgs &A, int cls, uint32_t key, bool on, bool minus, const long long (&q)[4], int lane) {
  if (__ballot(on) == 0) return;  // (the whole wavefront)
  const uint32_t prev = __shfl_up(key, 1);
  const uint64_t heads = __ballot(lane == 0 || prev != key);
  const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));
  const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  uint32_t cnt = on ? 1u : 0u;
  long long v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = on ? q[k] : 0;
  // (not unrolled: six copies of this function with six steps each would keep every step's lane masks in scalar registers
  // across the whole item loop, more than there are)
#pragma unroll 1
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t ro = __shfl_up(run, o);
    const bool add = lane >= o && ro == run;
    const uint32_t co = __shfl_up(cnt, o);
    if (add) cnt += co;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= A.ns) break;
      const long long vo = __shfl_up(v[k], o);
      if (add) v[k] += vo;
    }
  }
  if (last && cnt > 0 && key <= A.n_sites) {  // (a key beyond the arrays cannot be on: the windows end inside them)
    const size_t n1 = (size_t)A.n_sites + 1;
    unsigned long long *p = A.acc + (size_t)cls * (size_t)(1 + A.ns) * n1 + key;
    atomicAdd(p, minus ? 0ull - (unsigned long long)cnt : (unsigned long long)cnt);
    for (int k = 0; k < A.ns; ++k) atomicAdd(p + (size_t)(1 + k) * n1, minus ? 0ull - (unsigned long long)v[k] : (unsigned long long)v[k]);
  }
}

__global__ __launch_bounds__(256) void scan_kernel(ScanArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  unsigned long long qmax = 0, counted = 0;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; i < A.n_items; i += waves) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    const bool live = c < it.count;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    // (site LD's filter: dist as the difference of the prefix sums, which is the printed value since the gaps are integers)
    if (live && ((it.mask >> c) & 1ull) && A.infc[s1] == A.infc[s2]  // (across a chromosome dist is not finite: never counted)
        && A.cum[s2] - A.cum[s1] <= A.limit && A.maf_ok[s1] && A.maf_ok[s2]) {
      const ngsld_rec_std r = A.rec[record_of(it, c, A.out_base)];
      take = true;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        const double x = field_of(r, A.field[v]);
        if (!(x - x == 0.0)) take = false;  // NaN or +-inf in any chosen field: the row drops out of every one
      }
      if (take) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (v >= A.ns) break;
          int64_t m = 0;
          if (!ngsld::printed_micro(field_of(r, A.field[v]), &m)) {
            atomicCAS(A.meta, 0ull, (((unsigned long long)s1 << 32) | s2) + 1ull);
            take = false;
          }
          q[v] = m < 0 ? -m : m;
        }
      }
    }
    const uint64_t taken = __ballot(take);
    if (taken == 0) continue;
    if (!take) q[0] = q[1] = q[2] = q[3] = 0;
    counted += (unsigned long long)__popcll(taken);
    if (A.track_max) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        qmax = (unsigned long long)q[v] > qmax ? (unsigned long long)q[v] : qmax;
      }
    }
    // the window ends: b_i is the item's, a_j the lane's (a lane past the row reads nothing and is never on)
    const uint32_t bi1 = A.win_b[s1] + 1u;
    const uint32_t j = live ? s2 : 0xffffffffu;
    const uint32_t aj = live ? A.win_a[s2] : 0xffffffffu;
    bool on = take && j < bi1;  // LL: the centres [j, b_i]
    add_at(A, kLL, j, on, false, q, lane);
    add_at(A, kLL, bi1, on, true, q, lane);
    on = take && aj < s1;  // RR: [a_j, i - 1]
    add_at(A, kRR, aj, on, false, q, lane);
    add_at(A, kRR, s1, on, true, q, lane);
    const uint32_t lo = aj > s1 ? aj : s1, end = bi1 < j ? bi1 : j;  // LR: [max(a_j, i), min(b_i, j - 1)]
    on = take && lo < end;
    add_at(A, kLR, lo, on, false, q, lane);
    add_at(A, kLR, end, on, true, q, lane);
  }
  if (lane == 0 && counted) atomicAdd(A.meta + 2, counted);
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
}

// ngsld_scan in four parts (record_pass.h AnalysisPass)
struct ScanPass final : AnalysisPass {
  const ngsld_scan_params *p;
  ngsld_scan_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_scan_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  uint32_t words = 0;
  std::vector<uint32_t> win_a, win_b;
  uint64_t rows_max = 0;
  bool track = false;
  size_t n1 = 0, W = 0;
  std::vector<unsigned long long> h_acc;
  DevBuf<unsigned long long> d_acc, d_sum, d_meta;
  DevBuf<uint32_t> d_a, d_b;
  ScanArgs A{};
  ngsld_rec_std *rec = nullptr;
  uint64_t plant_at = ~0ull;
  double plant_dp = 0.0;

  ScanPass(const ngsld_scan_params *params, ngsld_scan_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_scan_params", stats, "ngsld_scan_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "scan fields must be a non-empty mask of 1, 2, 4, 8");
    if (p->half_window >= (1ull << 31)) return fail(c, NGSLD_ERR_INVALID, "scan half_window must be below 2^31");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "scan max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "scan min_maf is NaN");
    // a window holds the site pairs up to 2 H apart: a plan that stops short of them would leave a window's mean without rows
    // the TSV never had, silently
    if (c->params.max_kb_dist > 0 && c->params.max_kb_dist * 1000 < 2 * p->half_window)
      return fail(c, NGSLD_ERR_INVALID, "scan half_window " + std::to_string(p->half_window) + " needs the pairs up to " +
                                            std::to_string(2 * p->half_window) + " bp apart: the plan's max_kb_dist holds them up to " +
                                            std::to_string(c->params.max_kb_dist * 1000) + " bp");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.scan.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    if (n >= 0x7fffffffull) return fail(c, NGSLD_ERR_UNSUPPORTED, "scan needs n_sites below 2^31 - 1");
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    words = 1u + (uint32_t)ns;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf, the windows ----
    const double limit = p->max_kb_dist * 1000.0;
    F.prepare(c, &p->min_maf);
    if (!F.exact_gaps) return fail(c, NGSLD_ERR_UNSUPPORTED, "scan needs integer position gaps");
    win_a.resize(n);
    win_b.resize(n);
    uint64_t largest = 0;
    {
      const double H = (double)p->half_window;
      uint64_t lo = 0, hi = 0;  // both only move forward: cum does not decrease inside a chromosome
      for (uint64_t s = 0; s < n; ++s) {
        while (F.infc[lo] != F.infc[s] || F.cum[s] - F.cum[lo] > H) ++lo;
        if (hi < s) hi = s;
        while (hi + 1 < n && F.infc[hi + 1] == F.infc[s] && F.cum[hi + 1] - F.cum[s] <= H) ++hi;
        win_a[s] = (uint32_t)lo;
        win_b[s] = (uint32_t)hi;
        largest = std::max<uint64_t>(largest, hi - lo + 1);
      }
    }
    S.largest_window = largest;
    // every partial sum of a window is exact while max |q| * (the rows it can hold) < 2^63: certain below 2^25 rows (|q| < 2^38)
    rows_max = largest * (largest - (largest > 0 ? 1 : 0)) / 2;
    track = track_sums(rows_max >= (1ull << 25));

    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    n1 = (size_t)n + 1;
    W = (size_t)3 * words * n1;
    h_acc.assign(W, 0);
    if (n_pairs > 0) {
      if (const int rc = F.upload(c)) return rc;
      HIP_TRY(c, d_a.resize(n));
      HIP_TRY(c, d_b.resize(n));
      HIP_TRY(c, hipMemcpy(d_a.p, win_a.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(d_b.p, win_b.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
      HIP_TRY(c, d_acc.resize(W));
      HIP_TRY(c, d_sum.resize(W));
      HIP_TRY(c, d_meta.resize(3));
      HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, W * sizeof(unsigned long long), st));
      HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(unsigned long long), st));
      A.cum = F.d_cum.p;
      A.infc = F.d_infc.p;
      A.maf_ok = F.d_maf_ok.p;
      A.win_a = d_a.p;
      A.win_b = d_b.p;
      A.limit = limit;
      A.n_sites = (uint32_t)n;
      A.ns = ns;
      for (int v = 0; v < 4; ++v) A.field[v] = field[v];
      A.track_max = track ? 1 : 0;
      A.acc = d_acc.p;
      A.meta = d_meta.p;
      const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 8;
      // NGSLD_TEST_SCAN_PLANT_DP = "R:X" (tests): record R of the plan gets D' = X once its chunk's records are final.  Valid
      // haplotype frequencies give no finite D' near 2^38 micro-units, so this is the only way to the refusal of such a value
      // (and to a sum that holds the largest value allowed)
      if (const char *e = test_knob("SCAN_PLANT_DP")) {
        char *colon = nullptr;
        const uint64_t at = std::strtoull(e, &colon, 10);
        if (colon != e && *colon == ':') {
          plant_at = at;
          plant_dp = std::strtod(colon + 1, nullptr);
        }
      }
      const RecordPass::Step plant = [this, c, st](const RecordChunk &ch) -> int {
        if (plant_at < ch.out_base || plant_at - ch.out_base >= ch.pairs) return NGSLD_OK;
        HIP_TRY(c, hipMemcpyAsync(&rec[plant_at - ch.out_base].Dp, &plant_dp, sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return NGSLD_OK;
      };
      client.kernel_ms = &S.scan_ms;
      if (plant_at != ~0ull) client.before = plant;
      client.launch = [this, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
        A.out_base = ch.out_base;
        A.items = items;
        A.n_items = n_items;
        const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
        hipLaunchKernelGGL(scan_kernel, dim3(blocks), dim3(256), 0, st, A);
      };
      client.after = [this, c, st](const RecordChunk &) -> int {
        unsigned long long bad = 0;
        HIP_TRY(c, hipMemcpyAsync(&bad, d_meta.p, sizeof(bad), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return bad != 0 ? fail_value_range(c, "scan", bad) : NGSLD_OK;
      };
    }
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override {
    A.rec = records;
    rec = records;
  }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      // ---- the differences become the windows' totals: one inclusive sum per array, wrapping ----
      EventPair ev;
      HIP_TRY(c, ev.create());
      size_t temp_bytes = 0;
      HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, temp_bytes, d_acc.p, d_sum.p, (int)n1, st));
      DevBuf<char> d_temp;
      HIP_TRY(c, d_temp.resize(std::max<size_t>(temp_bytes, 1)));
      HIP_TRY(c, hipEventRecord(ev.a, st));
      for (size_t k = 0; k < (size_t)3 * words; ++k)
        HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(d_temp.p, temp_bytes, d_acc.p + k * n1, d_sum.p + k * n1, (int)n1, st));
      HIP_TRY(c, hipEventRecord(ev.b, st));
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_sum.p, W * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, ev.add_elapsed(&S.scan_ms));
      S.pairs_counted = meta[2];
      if (track && sum_may_wrap(meta[1], rows_max))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a window of up to " + std::to_string(rows_max) + " pairs with values too large to sum exactly");
    }

    // ---- per site: exact integer sums, one rounding each for zns and omega ----
    ScanResult &R = c->res.scan;
    R.first = std::move(win_a);
    R.last = std::move(win_b);
    R.n.resize(3 * n);
    R.sum.resize((size_t)ns * 3 * n);
    R.zns.resize((size_t)ns * n);
    R.omega.resize((size_t)ns * n);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t s = 0; s < n; ++s) {
      uint64_t cnt[3];
      for (int k = 0; k < 3; ++k) cnt[k] = R.n[(size_t)k * n + s] = h_acc[(size_t)k * words * n1 + s];
      const uint64_t rows = cnt[kLL] + cnt[kRR] + cnt[kLR], inside = cnt[kLL] + cnt[kRR];
      for (int v = 0; v < ns; ++v) {
        uint64_t sum[3];
        for (int k = 0; k < 3; ++k) {
          sum[k] = h_acc[((size_t)k * words + 1 + v) * n1 + s];
          R.sum[((size_t)v * 3 + k) * n + s] = (int64_t)sum[k];
        }
        const size_t at = (size_t)v * n + s;
        R.zns[at] = rows > 0 ? mean_nearest(sum[kLL] + sum[kRR] + sum[kLR], rows) : nan;
        R.omega[at] = (inside > 0 && cnt[kLR] > 0 && sum[kLR] > 0)
                          ? ratio_nearest((unsigned __int128)(sum[kLL] + sum[kRR]) * cnt[kLR], (unsigned __int128)inside * sum[kLR])
                          : nan;
      }
    }
    R.fields = p->fields;
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_scan_pass(const ngsld_scan_params *p, ngsld_scan_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new ScanPass(p, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_scan(ngsld_ctx *c, const ngsld_scan_params *p, ngsld_scan_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  ScanPass pass(p, stats);
  return run_single(c, pass, record_chunk(test_knob("SCAN_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_scan_get(ngsld_ctx *c, int field, uint32_t *win_first, uint32_t *win_last, uint64_t *n_ll, uint64_t *n_rr, uint64_t *n_lr,
                   int64_t *sum_ll, int64_t *sum_rr, int64_t *sum_lr, double *zns, double *omega) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const ScanResult &R = c->res.scan;
  if (!R.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_scan result (it goes with the next ngsld_plan or ngsld_set_*)");
  const int rank = field_rank(R.fields, field);
  if (rank < 0) return fail(c, NGSLD_ERR_INVALID, "not a field of the last ngsld_scan (TSV column 4..7)");
  const size_t v = (size_t)rank, m = R.first.size();
  if (m == 0) return NGSLD_OK;
  if (win_first) std::memcpy(win_first, R.first.data(), m * sizeof(uint32_t));
  if (win_last) std::memcpy(win_last, R.last.data(), m * sizeof(uint32_t));
  uint64_t *const cnt[3] = {n_ll, n_rr, n_lr};
  int64_t *const sum[3] = {sum_ll, sum_rr, sum_lr};
  for (int k = 0; k < 3; ++k) {
    if (cnt[k]) std::memcpy(cnt[k], R.n.data() + (size_t)k * m, m * sizeof(uint64_t));
    if (sum[k]) std::memcpy(sum[k], R.sum.data() + (v * 3 + k) * m, m * sizeof(int64_t));
  }
  if (zns) std::memcpy(zns, R.zns.data() + v * m, m * sizeof(double));
  if (omega) std::memcpy(omega, R.omega.data() + v * m, m * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
