// decay.hip -- LD decay on the device (ngsld_decay, include/ngsld.h): the bins scripts/fit_LDdecay.R averages, from the pair
// records where they are computed -- no TSV; a few hundred bin means leave the device.  DECAY.md has the rule, the deviations
// and why the sums are exact.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   bins     one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the filters,
//            dist as the TSV prints it (dist_prefix), the right-closed bin, each chosen field as its printed value in integer
//            micro-units (ld_prune.h).  dist rises with the candidate, so a wavefront's lanes fall in a few runs of one bin: a
//            segmented scan merges each run and its last lane adds once, into a per-workgroup LDS histogram flushed once per
//            workgroup (when it fits) or into global memory
//   host     a chunk's int64 sums fold into 128-bit totals (with |q| < 2^38, a chunk of kRecordChunkPairs sums below 2^62); a
//            bin's mean is the double nearest to sum / (10^6 * rows)
#include "engine.h"
#include "ld_decay_bins.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// per-workgroup LDS for the histogram (configs[2]: 400 bins x (1 + 4 fields) x 8 B = 16 KB)
constexpr uint32_t kLdsBudget = 32u << 10;
// bins sized from the plan beyond this are refused (raise the bin size or set max_kb_dist): 2^22 bins of 250 bp span 10^9 bp
constexpr uint64_t kMaxSlots = 1ull << 22;

struct BinArgs {
  const ngsld_item *items;
  uint64_t n_items;
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  double limit;               // dist < limit (+inf: no limit)
  double bin;                 // bin size B
  uint32_t n_slots;           // bins 0 .. n_slots-1
  int ns;                     // chosen fields
  int field[4];               // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int track_max;              // a chunk of more pairs than the pass's chunk (one row): max |q| goes to meta[1]
  unsigned long long *acc;    // [(1 + ns) * n_slots]: rows per bin, then the int64 sums of each field (two's complement)
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] a bin beyond n_slots
};

template <bool kLds>
__global__ __launch_bounds__(256) void bin_kernel(BinArgs A) {
  extern __shared__ unsigned long long lds[];
  const uint32_t W = (uint32_t)(1 + A.ns) * A.n_slots;
  unsigned long long *acc = kLds ? lds : A.acc;
  if (kLds) {
    for (uint32_t j = threadIdx.x; j < W; j += 256) lds[j] = 0;
    __syncthreads();
  }
  const int lane = (int)__lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  unsigned long long qmax = 0;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; i < A.n_items; i += waves) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    long long key = 0x7fffffffffffffffll;  // past the row (or its chromosome): one run at the tail
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    if (c < it.count) {
      const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
      if (A.infc[s1] == A.infc[s2]) {  // (across a chromosome dist is not finite: never counted)
        const double d = printed_dist(A.cum[s2] - A.cum[s1]);
        key = bin_of(d, A.bin);
        if (((it.mask >> c) & 1ull) && key >= 0 && d < A.limit && A.maf_ok[s1] && A.maf_ok[s2]) {
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
    const long long prev = __shfl_up(key, 1);
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
      if (key >= 0 && key < (long long)A.n_slots) {
        atomicAdd(acc + key, (unsigned long long)cnt);
        for (int v = 0; v < A.ns; ++v) atomicAdd(acc + (uint64_t)(1 + v) * A.n_slots + key, (unsigned long long)q[v]);
      } else {
        atomicOr(A.meta + 2, 1ull);
      }
    }
  }
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
  if (kLds) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < W; j += 256)
      if (lds[j] != 0) atomicAdd(A.acc + j, lds[j]);
  }
}

// ngsld_decay in four parts (record_pass.h AnalysisPass)
struct DecayPass final : AnalysisPass {
  const ngsld_decay_params *p;
  ngsld_decay_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_decay_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  uint64_t n_slots = 0, W = 0, chunk = 0;
  bool use_lds = false;
  std::vector<unsigned __int128> sum;
  std::vector<uint64_t> count;
  DevBuf<unsigned long long> d_acc, d_meta;
  std::vector<unsigned long long> h_acc;
  BinArgs A{};

  DecayPass(const ngsld_decay_params *params, ngsld_decay_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_decay_params", stats, "ngsld_decay_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "decay fields must be a non-empty mask of 1, 2, 4, 8");
    if (!(p->bin_size > 1.0) || !std::isfinite(p->bin_size)) return fail(c, NGSLD_ERR_INVALID, "decay bin_size must be a finite number > 1");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "decay max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "decay min_maf is NaN");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.decay.clear(); }

  int prepare(ngsld_ctx *c, uint64_t chunk_pairs) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    const double B = p->bin_size;
    chunk = chunk_pairs;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
    const double limit = p->max_kb_dist * 1000.0;
    F.prepare(c, &p->min_maf);
    if (const int rc = F.check_limit(c, "decay", limit)) return rc;
    const std::vector<double> &cum = F.cum;
    const std::vector<uint32_t> &infc = F.infc;

    // ---- bins sized from the plan: the largest finite planned dist, capped by the limit ----
    {
      std::vector<uint64_t> chr_last(n ? (size_t)infc[n - 1] + 1 : 0, 0);
      std::vector<double> chr_lo(chr_last.size(), INFINITY), chr_hi(chr_last.size(), -INFINITY);
      for (uint64_t s = 0; s < n; ++s) {
        chr_last[infc[s]] = s;
        chr_lo[infc[s]] = std::min(chr_lo[infc[s]], cum[s]);
        chr_hi[infc[s]] = std::max(chr_hi[infc[s]], cum[s]);
      }
      double dmax = 0.0;
      for (uint64_t s1 = 0; s1 < n; ++s1) {
        if (c->h_row_off[s1 + 1] == c->h_row_off[s1]) continue;
        const uint64_t s2 = std::min<uint64_t>(c->h_row_end[s1] - 1, chr_last[infc[s1]]);
        if (s2 <= s1) continue;
        // gaps >= 0 (every position file): dist rises along the row; any other gaps: the chromosome's span bounds it
        const double d = F.exact_gaps ? cum[s2] - cum[s1] : chr_hi[infc[s1]] - chr_lo[infc[s1]];
        dmax = std::max(dmax, printed_dist(d));
      }
      if (dmax >= limit) dmax = limit;  // (dist < limit: the limit's own bin is the last one that can fill)
      const long long kmax = bin_of(dmax, B);
      if (kmax >= 0) {
        if ((uint64_t)kmax >= kMaxSlots)
          return fail(c, NGSLD_ERR_UNSUPPORTED, "more than 2^22 decay bins (raise bin_size or set max_kb_dist)");
        n_slots = (uint64_t)kmax + 1;
      }
    }
    S.bin_slots = n_slots;
    W = (uint64_t)(1 + ns) * n_slots;
    uint64_t lds_budget = kLdsBudget;
    if (const char *e = test_knob("DECAY_LDS_BYTES")) lds_budget = std::min<uint64_t>(std::strtoull(e, nullptr, 10), 64u << 10);
    use_lds = W > 0 && W * 8 <= lds_budget;
    S.lds = use_lds ? 1 : 0;

    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    sum.assign(ns * n_slots, 0);
    count.assign(n_slots, 0);
    if (n_slots == 0 || n_pairs == 0) return NGSLD_OK;
    if (const int rc = F.upload(c)) return rc;
    HIP_TRY(c, d_acc.resize(W));
    HIP_TRY(c, d_meta.resize(3));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(unsigned long long), st));
    A.cum = F.d_cum.p;
    A.infc = F.d_infc.p;
    A.maf_ok = F.d_maf_ok.p;
    A.limit = limit;
    A.bin = B;
    A.n_slots = (uint32_t)n_slots;
    A.ns = ns;
    for (int v = 0; v < 4; ++v) A.field[v] = field[v];
    A.acc = d_acc.p;
    A.meta = d_meta.p;
    h_acc.resize(W);
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
    client.kernel_ms = &S.bin_ms;
    client.before = [this, c, st](const RecordChunk &ch) -> int {
      A.track_max = track_sums(ch.pairs > chunk) ? 1 : 0;
      HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, W * sizeof(unsigned long long), st));
      return NGSLD_OK;
    };
    client.launch = [this, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      A.out_base = ch.out_base;
      A.items = items;
      A.n_items = n_items;
      const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
      if (use_lds)
        hipLaunchKernelGGL(bin_kernel<true>, dim3(blocks), dim3(256), (size_t)W * 8, st, A);
      else
        hipLaunchKernelGGL(bin_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
    };
    client.after = [this, c, st](const RecordChunk &ch) -> int {
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc.p, W * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (meta[0] != 0) return fail_value_range(c, "decay", meta[0]);
      if (meta[2] != 0) return fail(c, NGSLD_ERR_INVALID, "decay: a row fell beyond the planned bins (internal error)");
      // a row longer than a chunk is one chunk: every partial sum of it is exact when max |q| * pairs < 2^63
      if (A.track_max && sum_may_wrap(meta[1], ch.pairs))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a row of " + std::to_string(ch.pairs) + " pairs with values too large to sum exactly");
      for (uint64_t k = 0; k < n_slots; ++k) {
        count[k] += h_acc[k];
        for (int v = 0; v < ns; ++v) sum[v * n_slots + k] += (unsigned __int128)(__int128)(int64_t)h_acc[(1 + v) * n_slots + k];
      }
      return NGSLD_OK;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
    }
    // ---- the means: exact integer sums, one rounding ----
    const double B = p->bin_size;
    for (uint64_t k = 0; k < n_slots; ++k) {
      if (count[k] == 0) continue;
      c->res.decay.dist.push_back(break_value(k, B));
      c->res.decay.count.push_back(count[k]);
      S.pairs_counted += count[k];
      for (int v = 0; v < ns; ++v) {
        const __int128 s = (__int128)sum[v * n_slots + k];
        const unsigned __int128 a = (unsigned __int128)(s < 0 ? -s : s), b = (unsigned __int128)count[k] * 1000000u;
        const double m = div_nearest(a, b);
        c->res.decay.mean.push_back(s < 0 ? -m : m);
      }
    }
    c->res.decay.fields = p->fields;
    S.bins = c->res.decay.count.size();
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
  const DecayResult &D = c->res.decay;
  const uint64_t nb = D.count.size();
  if (n_bins) *n_bins = nb;
  const uint64_t m = std::min<uint64_t>(cap, nb);
  const int nf = __builtin_popcount(D.fields);
  if (m > 0 && dist) std::memcpy(dist, D.dist.data(), m * sizeof(double));
  if (m > 0 && count) std::memcpy(count, D.count.data(), m * sizeof(uint64_t));
  if (m > 0 && mean) std::memcpy(mean, D.mean.data(), m * nf * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
