// decay.hip -- LD decay on the device (ngsld_decay, include/ngsld.h): the bins scripts/fit_LDdecay.R averages, from the pair
// records where they are computed -- no TSV; a few hundred bin means leave the device.  DECAY.md has the rule, the deviations
// and why the sums are exact.  The bin kernel and its host side (DecayBins, ld_decay_bins.h) are here, once, for this call and for
// ngsld_decay_map (decay_map.hip), which keeps the bins per group: the pooled decay is the map with a single group.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   bins     one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the filters,
//            dist as the TSV prints it (dist_prefix), the right-closed bin, each chosen field as its printed value in integer
//            micro-units (ld_prune.h).  The key is (group, bin); dist rises with the candidate, so a wavefront's lanes fall in a
//            few runs of one key: a segmented scan merges each run and its last lane adds once per word.  A workgroup takes a
//            contiguous span of the launch's items -- rows in order, so almost always one group -- and keeps the bins of the span's
//            first group (its home) in LDS, flushed once; a run of any other group adds to global memory.  Integer adds commute:
//            the home, the launch shape and the order give the same bits.  Where a group's bins do not fit the LDS budget every
//            run adds to global memory.
//   host     a chunk's int64 sums fold into 128-bit totals (with |q| < 2^38, a chunk of kRecordChunkPairs sums below 2^62); a
//            bin's mean is the double nearest to sum / (10^6 * rows) (append_bin_means, ld_mean.h)
#include "engine.h"
#include "ld_decay_bins.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// per-workgroup LDS for the home group's bins (configs[2]: 400 bins x (1 + 4 fields) x 8 B = 16 KB)
constexpr uint32_t kLdsBudget = 32u << 10, kLdsMax = 64u << 10;
// bins sized from the plan beyond this are refused (raise the bin size or set max_kb_dist): 2^22 bins of 250 bp span 10^9 bp
constexpr uint64_t kMaxSlots = 1ull << 22;

// the group slot of the pair (s1, s2) of one chromosome
__device__ __forceinline__ uint32_t group_of(const DecayBinArgs &A, const uint4 a, const uint4 b) {
  return a.y + b.z + ((unsigned long long)a.w + b.w >= A.two_w ? 1u : 0u);
}

template <bool kLds>
__global__ __launch_bounds__(256) void bin_kernel(DecayBinArgs A) {
  extern __shared__ unsigned long long lds[];
  const uint32_t W = (uint32_t)(1 + A.ns) * A.n_bins;
  const uint64_t slots = (uint64_t)A.n_groups * A.n_bins;
  const int lane = (int)__lane_id();
  uint64_t first, end, step;
  uint32_t home = 0xffffffffu;
  if (kLds) {  // a workgroup per contiguous span of items
    const uint64_t span = (A.n_items + gridDim.x - 1) / gridDim.x;
    const uint64_t ib = (uint64_t)blockIdx.x * span;
    end = ib + span < A.n_items ? ib + span : A.n_items;
    if (ib >= end) return;  // (the whole workgroup)
    const ngsld_item it0 = A.items[ib];
    if (it0.s1 < A.n_sites && it0.s2_begin < A.n_sites) home = group_of(A, A.site[it0.s1], A.site[it0.s2_begin]);
    for (uint32_t j = threadIdx.x; j < W; j += 256) lds[j] = 0;
    __syncthreads();
    first = ib + (threadIdx.x >> 6);
    step = 4;
  } else {
    first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    end = A.n_items;
    step = (uint64_t)gridDim.x * 4;
  }
  unsigned long long qmax = 0;
  for (uint64_t i = first; i < end; i += step) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    unsigned long long key = ~0ull;  // past the row (or its chromosome): one run at the tail
    uint32_t group = 0xffffffffu;
    long long bin = -1;
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    if (c < it.count) {
      const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
      const uint4 a = A.site[s1], b = A.site[s2 < A.n_sites ? s2 : s1];
      if (s2 < A.n_sites && (a.x >> 1) == (b.x >> 1)) {  // (across a chromosome dist is not finite: never counted)
        const double d = printed_dist(A.cum[s2] - A.cum[s1]);
        bin = bin_of(d, A.bin);
        group = group_of(A, a, b);
        key = ((unsigned long long)group << 32) | (unsigned long long)(uint32_t)bin;
        if (((it.mask >> c) & 1ull) && bin >= 0 && d < A.limit && (a.x & b.x & 1u)) {
          const ngsld_rec_std r = A.rec[record_of(it, c, A.out_base)];
          take = true;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (v >= A.ns) break;
            const double x = field_of(r, (int)((A.field4 >> (4 * v)) & 3u));
            if (!(x - x == 0.0)) take = false;  // NaN or +-inf in any chosen field: the row drops out of every one
          }
          if (take) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              if (v >= A.ns) break;
              int64_t m = 0;
              if (!ngsld::printed_micro(field_of(r, (int)((A.field4 >> (4 * v)) & 3u)), &m)) {
                atomicCAS(A.meta, 0ull, (((unsigned long long)s1 << 32) | s2) + 1ull);
                take = false;
              }
              q[v] = m;
            }
          }
          if (!take) q[0] = q[1] = q[2] = q[3] = 0;
        }
      }
    }
    if (__ballot(take) == 0) continue;
    if (A.track_max) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        const unsigned long long a = (unsigned long long)(q[v] < 0 ? -q[v] : q[v]);
        qmax = a > qmax ? a : qmax;
      }
    }
    // runs of one key, numbered from lane 0 (keys rise with the lane; the numbering does not rely on it)
    const unsigned long long prev = __shfl_up(key, 1);
    const uint64_t heads = __ballot(lane == 0 || prev != key);
    const uint32_t run = (uint32_t)__popcll(heads & ((2ull << lane) - 1ull));
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    uint32_t cnt = take ? 1u : 0u;
    for (int o = 1; o < 64; o <<= 1) {  // segmented inclusive scan: the run's last lane holds its totals
      const uint32_t ro = __shfl_up(run, o);  // (every lane takes part in every shuffle)
      const bool add = lane >= o && ro == run;
      const uint32_t co = __shfl_up(cnt, o);
      if (add) cnt += co;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        const long long qo = __shfl_up(q[v], o);
        if (add) q[v] += qo;
      }
    }
    if (last && cnt > 0) {
      if (bin >= 0 && bin < (long long)A.n_bins && group < A.n_groups) {
        const bool at_home = kLds && group == home;
        unsigned long long *p = at_home ? lds + bin : A.acc + (uint64_t)group * A.n_bins + bin;
        const uint64_t stride = at_home ? A.n_bins : slots;
        atomicAdd(p, (unsigned long long)cnt);
        for (int v = 0; v < A.ns; ++v) atomicAdd(p + (uint64_t)(1 + v) * stride, (unsigned long long)q[v]);
      } else {
        atomicOr(A.meta + 2, 1ull);  // (the plan says this cannot happen: reported, never written)
      }
    }
  }
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
  if (kLds) {
    __syncthreads();
    if (home < A.n_groups)  // (a word of LDS is non-zero only through a run of the home group, which passed the check above)
      for (int v = 0; v <= A.ns; ++v)
        for (uint32_t j = threadIdx.x; j < A.n_bins; j += 256) {
          const unsigned long long x = lds[(uint32_t)v * A.n_bins + j];
          if (x != 0) atomicAdd(A.acc + (uint64_t)v * slots + (uint64_t)home * A.n_bins + j, x);
        }
  }
}

}  // namespace

int DecayBins::check_params(ngsld_ctx *c, const char *pass, uint32_t fields, double bin_size, double max_kb_dist, double min_maf) {
  const std::string who = pass;
  if (fields == 0 || fields > 15) return fail(c, NGSLD_ERR_INVALID, who + " fields must be a non-empty mask of 1, 2, 4, 8");
  if (!(bin_size > 1.0) || !std::isfinite(bin_size)) return fail(c, NGSLD_ERR_INVALID, who + " bin_size must be a finite number > 1");
  if (std::isnan(max_kb_dist) || max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, who + " max_kb_dist must be >= 0");
  if (std::isnan(min_maf)) return fail(c, NGSLD_ERR_INVALID, who + " min_maf is NaN");
  return NGSLD_OK;
}

int DecayBins::plan(ngsld_ctx *c, const char *pass, const char *lds_knob, uint32_t fields, double bin_size, double max_kb_dist,
                    double min_maf) {
  int field[4] = {0, 0, 0, 0};
  A.ns = ns = field_list(fields, field);
  for (int v = 0; v < ns; ++v) A.field4 |= (uint32_t)field[v] << (4 * v);
  A.limit = max_kb_dist * 1000.0;
  A.bin = bin_size;
  // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
  F.prepare(c, &min_maf);
  if (const int rc = F.check_limit(c, pass, A.limit)) return rc;
  n_bins = planned_bins(F.infc, F.cum, F.exact_gaps, c->h_row_off, c->h_row_end, A.limit, A.bin);
  uint64_t lds_budget = kLdsBudget;
  if (const char *e = test_knob(lds_knob)) lds_budget = std::min<uint64_t>(std::strtoull(e, nullptr, 10), kLdsMax);
  use_lds = n_bins > 0 && n_bins <= lds_budget / (8 * (uint64_t)(1 + ns));
  return NGSLD_OK;
}

int DecayBins::upload(ngsld_ctx *c, const std::vector<uint4> &site, uint64_t n_groups, uint32_t two_w, RecordPass::Client &client) {
  const uint64_t n = c->n_sites;
  hipStream_t st = c->stream;
  words = (uint64_t)(1 + ns) * n_groups * n_bins;
  HIP_TRY(c, F.d_cum.resize(n));
  HIP_TRY(c, d_site.resize(n));
  HIP_TRY(c, d_acc.resize(words));
  HIP_TRY(c, d_meta.resize(3));
  HIP_TRY(c, hipMemcpy(F.d_cum.p, F.cum.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_site.p, site.data(), n * sizeof(uint4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(unsigned long long), st));
  A.cum = F.d_cum.p;
  A.site = d_site.p;
  A.two_w = two_w;
  A.n_sites = (uint32_t)n;
  A.n_bins = (uint32_t)n_bins;
  A.n_groups = (uint32_t)n_groups;
  A.acc = d_acc.p;
  A.meta = d_meta.p;
  const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
  client.launch = [this, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
    A.out_base = ch.out_base;
    A.items = items;
    A.n_items = n_items;
    const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
    if (use_lds)
      hipLaunchKernelGGL(bin_kernel<true>, dim3(blocks), dim3(256), (size_t)(1 + ns) * n_bins * 8, st, A);
    else
      hipLaunchKernelGGL(bin_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
  };
  return NGSLD_OK;
}

int DecayBins::read_meta(ngsld_ctx *c, const char *pass, const char *beyond, unsigned long long meta[3]) {
  HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (meta[0] != 0) return fail_value_range(c, pass, meta[0]);
  if (meta[2] != 0) return fail(c, NGSLD_ERR_INVALID, beyond);
  return NGSLD_OK;
}

namespace {

// ngsld_decay in four parts (record_pass.h AnalysisPass)
struct DecayPass final : AnalysisPass {
  const ngsld_decay_params *p;
  ngsld_decay_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_decay_stats S;
  DecayBins bins;
  int ns = 0;
  uint64_t n_slots = 0, chunk = 0;
  std::vector<unsigned __int128> sum;
  std::vector<uint64_t> count, h_acc;

  DecayPass(const ngsld_decay_params *params, ngsld_decay_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_decay_params", stats, "ngsld_decay_stats")) return rc;
    return DecayBins::check_params(c, "decay", p->fields, p->bin_size, p->max_kb_dist, p->min_maf);
  }

  void clear(ngsld_ctx *c) override { c->res.decay.clear(); }

  int prepare(ngsld_ctx *c, uint64_t chunk_pairs) override {
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    chunk = chunk_pairs;
    if (const int rc = bins.plan(c, "decay", "DECAY_LDS_BYTES", p->fields, p->bin_size, p->max_kb_dist, p->min_maf)) return rc;
    if (bins.n_bins > kMaxSlots) return fail(c, NGSLD_ERR_UNSUPPORTED, "more than 2^22 decay bins (raise bin_size or set max_kb_dist)");
    ns = bins.ns;
    S.bin_slots = n_slots = bins.n_bins;
    S.lds = bins.use_lds ? 1 : 0;
    S.pairs = c->h_row_off[c->n_sites];
    sum.assign(ns * n_slots, 0);
    count.assign(n_slots, 0);
    if (n_slots == 0 || S.pairs == 0) return NGSLD_OK;
    // one group: with y, z and w 0 and U out of reach the slot of every pair is 0, and the accumulators are [1 + ns][n_slots]
    std::vector<uint4> site(c->n_sites);
    for (uint64_t s = 0; s < site.size(); ++s) site[s] = make_uint4(bins.site_x(s), 0, 0, 0);
    if (const int rc = bins.upload(c, site, 1, 0xffffffffu, client)) return rc;
    h_acc.resize(bins.words);
    client.kernel_ms = &S.bin_ms;
    client.before = [this, c, st](const RecordChunk &ch) -> int {
      bins.A.track_max = track_sums(ch.pairs > chunk) ? 1 : 0;
      HIP_TRY(c, hipMemsetAsync(bins.d_acc.p, 0, bins.words * sizeof(unsigned long long), st));
      return NGSLD_OK;
    };
    client.after = [this, c, st](const RecordChunk &ch) -> int {
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), bins.d_acc.p, bins.words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      if (const int rc = bins.read_meta(c, "decay", "decay: a row fell beyond the planned bins (internal error)", meta)) return rc;
      // a row longer than a chunk is one chunk: every partial sum of it is exact when max |q| * pairs < 2^63
      if (bins.A.track_max && sum_may_wrap(meta[1], ch.pairs))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a row of " + std::to_string(ch.pairs) + " pairs with values too large to sum exactly");
      for (uint64_t k = 0; k < n_slots; ++k) {
        count[k] += h_acc[k];
        for (int v = 0; v < ns; ++v) sum[v * n_slots + k] += (unsigned __int128)(__int128)(int64_t)h_acc[(1 + v) * n_slots + k];
      }
      return NGSLD_OK;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { bins.A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
    }
    // ---- the means: exact integer sums, one rounding ----
    DecayResult &D = c->res.decay;
    const double B = p->bin_size;
    S.pairs_counted = append_bin_means(
        n_slots, count.data(), ns, [&](int v, uint64_t k) { return (__int128)sum[v * n_slots + k]; },
        [&](uint64_t k) { return break_value(k, B); }, D.dist, D.count, D.mean);
    D.fields = p->fields;
    S.bins = D.count.size();
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_decay_pass(const ngsld_decay_params *p, ngsld_decay_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new DecayPass(p, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_decay(ngsld_ctx *c, const ngsld_decay_params *p, ngsld_decay_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  DecayPass pass(p, stats);
  return run_single(c, pass, record_chunk(test_knob("DECAY_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_decay_bins(ngsld_ctx *c, uint64_t cap, double *dist, uint64_t *count, double *mean, uint64_t *n_bins) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  copy_out_bins(c->res.decay, cap, dist, count, mean, n_bins);
  return NGSLD_OK;
}

}  // extern "C"
