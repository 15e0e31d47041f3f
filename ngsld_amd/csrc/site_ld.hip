// site_ld.hip -- per-site LD summaries on the device (ngsld_site_ld, include/ngsld.h): the pair table collapsed per site -- rows,
// sum (the LD score), mean, maximum and linked partners of every site -- from the pair records where they are computed; no
// TSV, a few numbers per site leave the device.  SITES.md has the rule, the deviations and why the sums are exact.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   sites    one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the filters,
//            each chosen field as its printed value in integer micro-units (ld_prune.h), added to BOTH sites of the pair.
//            The row end: the 64 lanes of an item share s1 -- rows, sums, maximum and linked rows are reduced across the
//            wavefront and added once per item.  The column end: the lanes of an item are 64 consecutive sites, and in a
//            windowed run the rows of a neighbourhood all hit the same few hundred columns.  A workgroup therefore takes a
//            tile of kTileRows consecutive rows, keeps the accumulators of the sites those rows can reach -- the plan bounds
//            the span -- in LDS and flushes the non-zero ones once, with global 64-bit atomics; where the span does not fit
//            (all pairs, no window) every add is a global atomic.  Integer adds and maxima commute: every launch shape and
//            order gives the same bits.
//   host     the accumulators come back once, after the last chunk; a site's mean is the double nearest to
//            sum / (10^6 * rows) (mean_nearest, ld_mean.h)
#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// LDS of a tile's accumulators.  configs[2] (windows of ~1,000 sites), one field: (1,000 + 16) sites x 4 words x 8 B = 32 KB,
// four workgroups (16 wavefronts) a compute unit; SITES.md has the measurements
constexpr uint32_t kLdsBudget = 64u << 10;
constexpr uint32_t kTileRows = 16;

struct SiteArgs {
  const ngsld_item *items;    // the context's items, all of them
  const uint64_t *item_off;   // ... and how many lie before each row
  uint64_t i0, i1;            // the items of this launch
  uint64_t r0, r1;            // the chunk's rows
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  double limit;               // dist <= limit (+inf: no limit)
  double linked_min;
  uint32_t n_sites;
  uint32_t cols;              // LDS path: the sites [tile's first row, + cols) have their accumulators in LDS
  int ns;                     // chosen fields
  int field[4];               // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  int track_max;              // a site may be in 2^25 rows or more: max |q| goes to meta[1]
  unsigned long long *acc;    // [1 + 3 * ns][n_sites]: rows; then per field the int64 sum (two's complement), the biased maximum, the linked rows
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|
};

// word w of a site's accumulators: in the tile's LDS window where the site lies in it, else in global memory
template <bool kLds>
__device__ __forceinline__ void accumulate(const SiteArgs &A, unsigned long long *lds, uint32_t base, uint32_t w, uint32_t site,
                                           unsigned long long v) {
  unsigned long long *p = (kLds && site - base < A.cols) ? lds + (size_t)w * A.cols + (site - base) : A.acc + (size_t)w * A.n_sites + site;
  if (is_max_word(w))
    atomicMax(p, v);
  else
    atomicAdd(p, v);
}

template <bool kLds>
__global__ __launch_bounds__(256) void site_kernel(SiteArgs A) {
  extern __shared__ unsigned long long lds[];
  const int lane = (int)__lane_id();
  const uint32_t words = 1u + 3u * (uint32_t)A.ns;
  uint64_t first, end, step;
  uint32_t base = 0;
  if (kLds) {  // a workgroup per tile of rows: its items are consecutive
    const uint64_t ra = A.r0 + (uint64_t)blockIdx.x * kTileRows, rb = ra + kTileRows < A.r1 ? ra + kTileRows : A.r1;
    const uint64_t ib = A.item_off[ra] > A.i0 ? A.item_off[ra] : A.i0;
    end = A.item_off[rb] < A.i1 ? A.item_off[rb] : A.i1;
    if (ib >= end) return;  // (the whole workgroup: nothing of this tile in this launch)
    base = (uint32_t)ra;
    for (uint32_t j = threadIdx.x; j < words * A.cols; j += 256) lds[j] = 0;
    __syncthreads();
    first = ib + (threadIdx.x >> 6);
    step = 4;
  } else {
    first = A.i0 + (((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6);
    end = A.i1;
    step = (uint64_t)gridDim.x * 4;
  }
  unsigned long long qmax = 0;
  for (uint64_t i = first; i < end; i += step) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    // (dist as the difference of the prefix sums, without decay's rounding to what "%.0f" prints: a finite limit is refused
    // unless the gaps are integers, where the difference is the printed value, and without a limit only finiteness matters)
    if (c < it.count && ((it.mask >> c) & 1ull) && A.infc[s1] == A.infc[s2]  // (across a chromosome dist is not finite: never counted)
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
          q[v] = (A.abs_value && m < 0) ? -m : m;
        }
      }
    }
    const uint64_t taken = __ballot(take);
    if (taken == 0) continue;
    if (!take) q[0] = q[1] = q[2] = q[3] = 0;
    // the column end: this lane's site
    if (take) accumulate<kLds>(A, lds, base, 0, s2, 1ull);
    const unsigned long long rows = (unsigned long long)__popcll(taken);
    if (lane == 0) accumulate<kLds>(A, lds, base, 0, s1, rows);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v >= A.ns) break;
      const uint32_t w = 1u + 3u * (uint32_t)v;
      const bool linked = take && (double)q[v] / 1e6 >= A.linked_min;  // the printed value read back (ld_prune.h), as doubles
      const unsigned long long biased = take ? (unsigned long long)(q[v] + (long long)kMaxBias) : 0ull;
      if (take) {
        accumulate<kLds>(A, lds, base, w, s2, (unsigned long long)q[v]);
        accumulate<kLds>(A, lds, base, w + 1, s2, biased);
        if (linked) accumulate<kLds>(A, lds, base, w + 2, s2, 1ull);
      }
      // the row end: one add per item
      const long long sum = wave_sum(q[v]);
      const unsigned long long top = wave_max(biased);
      const unsigned long long n_linked = (unsigned long long)__popcll(__ballot(linked));
      if (lane == 0) {
        accumulate<kLds>(A, lds, base, w, s1, (unsigned long long)sum);
        accumulate<kLds>(A, lds, base, w + 1, s1, top);
        if (n_linked) accumulate<kLds>(A, lds, base, w + 2, s1, n_linked);
      }
      if (A.track_max) {
        const unsigned long long a = (unsigned long long)(q[v] < 0 ? -q[v] : q[v]);
        qmax = a > qmax ? a : qmax;
      }
    }
  }
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
  if (kLds) {
    __syncthreads();
    for (uint32_t w = 0; w < words; ++w)
      for (uint32_t col = threadIdx.x; col < A.cols; col += 256) {
        const unsigned long long v = lds[(size_t)w * A.cols + col];
        const uint64_t site = (uint64_t)base + col;
        if (v == 0 || site >= A.n_sites) continue;
        if (is_max_word(w))
          atomicMax(A.acc + (size_t)w * A.n_sites + site, v);
        else
          atomicAdd(A.acc + (size_t)w * A.n_sites + site, v);
      }
  }
}

// ngsld_site_ld in four parts (record_pass.h AnalysisPass)
struct SiteLdPass final : AnalysisPass {
  const ngsld_site_ld_params *p;
  ngsld_site_ld_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_site_ld_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  uint32_t words = 0;
  uint64_t cols = 0, degree_max = 0;
  bool use_lds = false;
  size_t W = 0;
  std::vector<unsigned long long> h_acc;
  DevBuf<unsigned long long> d_acc, d_meta;
  SiteArgs A{};

  SiteLdPass(const ngsld_site_ld_params *params, ngsld_site_ld_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_site_ld_params", stats, "ngsld_site_ld_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "site_ld fields must be a non-empty mask of 1, 2, 4, 8");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "site_ld max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "site_ld min_maf is NaN");
    if (std::isnan(p->linked_min)) return fail(c, NGSLD_ERR_INVALID, "site_ld linked_min is NaN");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.site_ld.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    words = 1u + 3u * (uint32_t)ns;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
    const double limit = p->max_kb_dist * 1000.0;
    F.prepare(c, &p->min_maf);
    if (const int rc = F.check_limit(c, "site_ld", limit)) return rc;

    // ---- from the plan: how far a row reaches (the LDS window of a tile), how many rows a site can be in (the sums' bound) ----
    uint64_t span = 0;
    {
      std::vector<int64_t> cover(n + 1, 0);  // +1 where a row's candidates begin, -1 where they end
      for (uint64_t s = 0; s < n; ++s) {
        if (c->h_row_off[s + 1] == c->h_row_off[s] || c->h_row_end[s] <= s + 1) continue;
        span = std::max<uint64_t>(span, c->h_row_end[s] - s - 1);
        ++cover[s + 1];
        --cover[c->h_row_end[s]];
      }
      int64_t columns = 0;
      for (uint64_t s = 0; s < n; ++s) {
        columns += cover[s];
        degree_max = std::max<uint64_t>(degree_max, (c->h_row_off[s + 1] - c->h_row_off[s]) + (uint64_t)columns);
      }
    }
    cols = std::min<uint64_t>(span + kTileRows, n);
    uint64_t lds_budget = kLdsBudget;
    if (const char *e = test_knob("SITE_LDS_BYTES")) lds_budget = std::min<uint64_t>(std::strtoull(e, nullptr, 10), kLdsBudget);
    use_lds = span > 0 && (uint64_t)words * cols * 8 <= lds_budget;
    S.lds = use_lds ? 1 : 0;

    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    W = (size_t)words * n;
    h_acc.assign(W, 0);
    if (n_pairs == 0) return NGSLD_OK;
    if (const int rc = F.upload(c)) return rc;
    HIP_TRY(c, d_acc.resize(W));
    HIP_TRY(c, d_meta.resize(2));
    HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, W * sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 2 * sizeof(unsigned long long), st));
    A.items = c->d_items.p;
    A.item_off = c->d_item_off.p;
    A.cum = F.d_cum.p;
    A.infc = F.d_infc.p;
    A.maf_ok = F.d_maf_ok.p;
    A.limit = limit;
    A.linked_min = p->linked_min;
    A.n_sites = (uint32_t)n;
    A.cols = (uint32_t)cols;
    A.ns = ns;
    for (int v = 0; v < 4; ++v) A.field[v] = field[v];
    A.abs_value = p->abs_value != 0 ? 1 : 0;
    // every partial sum of a site is exact while max |q| * (the rows it can be in) < 2^63: certain below 2^25 rows (|q| < 2^38)
    A.track_max = track_sums(degree_max >= (1ull << 25)) ? 1 : 0;
    A.acc = d_acc.p;
    A.meta = d_meta.p;
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
    client.kernel_ms = &S.site_ms;
    client.launch = [this, c, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      A.out_base = ch.out_base;
      A.r0 = ch.r0;
      A.r1 = ch.r1;
      A.i0 = (uint64_t)(items - c->d_items.p);
      A.i1 = A.i0 + n_items;
      if (use_lds) {
        const unsigned tiles = blocks_for(ch.r1 - ch.r0, kTileRows);
        hipLaunchKernelGGL(site_kernel<true>, dim3(tiles), dim3(256), (size_t)words * cols * 8, st, A);
      } else {
        const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
        hipLaunchKernelGGL(site_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
      }
    };
    client.after = [this, c, st](const RecordChunk &) -> int {
      unsigned long long bad = 0;
      HIP_TRY(c, hipMemcpyAsync(&bad, d_meta.p, sizeof(bad), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      return bad != 0 ? fail_value_range(c, "site_ld", bad) : NGSLD_OK;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      unsigned long long meta[2] = {0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc.p, W * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (A.track_max && sum_may_wrap(meta[1], degree_max))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a site in up to " + std::to_string(degree_max) + " pairs with values too large to sum exactly");
    }

    // ---- the summaries: exact integer sums, one rounding for the mean ----
    c->res.site_ld.n.assign(h_acc.begin(), h_acc.begin() + n);
    c->res.site_ld.sum.resize((size_t)ns * n);
    c->res.site_ld.max.resize((size_t)ns * n);
    c->res.site_ld.linked.resize((size_t)ns * n);
    c->res.site_ld.mean.resize((size_t)ns * n);
    uint64_t ends = 0;
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t rows = c->res.site_ld.n[s];
      ends += rows;
      if (rows > 0) ++S.sites_with_pairs;
      for (int v = 0; v < ns; ++v) {
        const size_t k = (size_t)v * n + s;
        // (no rows: nothing was added to the site's words)
        const FieldSummary f = rows > 0 ? field_summary(h_acc.data(), n, v, s)
                                        : FieldSummary{0, std::numeric_limits<int64_t>::min(), 0, std::numeric_limits<double>::quiet_NaN()};
        c->res.site_ld.sum[k] = f.sum;
        c->res.site_ld.max[k] = f.max;
        c->res.site_ld.linked[k] = f.linked;
        c->res.site_ld.mean[k] = f.mean;
      }
    }
    S.pairs_counted = ends / 2;
    c->res.site_ld.fields = p->fields;
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_site_ld_pass(const ngsld_site_ld_params *p, ngsld_site_ld_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new SiteLdPass(p, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_site_ld(ngsld_ctx *c, const ngsld_site_ld_params *p, ngsld_site_ld_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  SiteLdPass pass(p, stats);
  return run_single(c, pass, record_chunk(test_knob("SITE_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_site_ld_get(ngsld_ctx *c, int field, uint64_t *n, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked, double *mean) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const SiteLdResult &R = c->res.site_ld;
  if (!R.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_site_ld result (it goes with the next ngsld_plan or ngsld_set_*)");
  const int v = field_rank(R.fields, field);
  if (v < 0) return fail(c, NGSLD_ERR_INVALID, "not a field of the last ngsld_site_ld (TSV column 4..7)");
  const size_t m = R.n.size(), k = (size_t)v * m;
  if (m == 0) return NGSLD_OK;
  if (n) std::memcpy(n, R.n.data(), m * sizeof(uint64_t));
  if (sum_micro) std::memcpy(sum_micro, R.sum.data() + k, m * sizeof(int64_t));
  if (max_micro) std::memcpy(max_micro, R.max.data() + k, m * sizeof(int64_t));
  if (linked) std::memcpy(linked, R.linked.data() + k, m * sizeof(uint64_t));
  if (mean) std::memcpy(mean, R.mean.data() + k, m * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
