// decay_map.hip -- the LD decay map on the device (ngsld_decay_map, include/ngsld.h): ngsld_decay's bins kept per group -- a
// chromosome, or the window of W bp that holds a pair's midpoint -- instead of pooled, from the pair records where they are
// computed; no TSV.  DECAY_MAP.md has the rule, the refusals and the measurements; DECAY.md why the sums are exact.
//
//   groups   host: a chromosome is a run of sites between the non-finite gaps of pos_dist (infc).  Per chromosome one slot, or
//            with a window the slots of the windows from its first site's to its last site's.  With U = 2 W a site carries
//            qa = pos / U (less its chromosome's first) and rem = pos % U, so that (p1 + p2) / U = qa1 + qa2 + (rem1 + rem2 >= U):
//            the kernel divides nothing.  gq[s] folds the chromosome's first slot into qa[s]: the slot of a pair is
//            gq[s1] + qa[s2] + carry.  Per chromosome qa and rem are 0 and U is out of reach: the slot is gq[s1].
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//   bins     decay's kernel (decay.hip) with the composite key (slot, bin): one wavefront per work item, one lane per candidate,
//            a segmented scan merges each run of one key and its last lane adds once per word.  A workgroup takes a contiguous
//            span of the launch's items -- rows in order, so almost always one group -- and keeps the bins of the span's first
//            group (its home) in LDS, flushed once; a run of any other group adds to global memory.  Integer adds commute: the
//            home, the launch shape and the order give the same bits.  Where a group's bins do not fit the LDS budget every run
//            adds to global memory.
//   host     the accumulators stay on the device across the chunks and come back once; a bin's mean is the double nearest to
//            sum / (10^6 * rows) (div_nearest_small, ld_mean.h)
#include "engine.h"
#include "ld_decay_bins.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// per-workgroup LDS for the home group's bins, as decay's histogram (configs[2]: 400 bins x (1 + 4 fields) x 8 B = 16 KB)
constexpr uint32_t kLdsBudget = 32u << 10, kLdsMax = 64u << 10;
// the accumulators of a call: (1 + fields) x group slots x bin slots x 8 B
constexpr uint64_t kMaxAccBytes = 1ull << 30;

struct MapArgs {
  const ngsld_item *items;
  uint64_t n_items;
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint4 *site;          // per site, one 16 B load: x = infc << 1 | (printed maf >= min_maf), y = gq (its chromosome's first slot
                              // + qa, less one where the first window begins in the upper half of a U), z = qa (pos / U less its
                              // chromosome's first), w = rem (pos % U)
  double limit;               // dist < limit (+inf: no limit)
  double bin;                 // bin size B
  uint32_t n_sites;
  uint32_t n_bins;            // bins 0 .. n_bins-1 of every group
  uint32_t n_groups;          // group slots
  uint32_t two_w;             // U = 2 W (per chromosome: 2^32 - 1, and every rem is 0)
  int ns;                     // chosen fields
  uint32_t field4;            // ... four bits each: 0 r2_ExpG, 1 D, 2 D', 3 r2
  int track_max;              // the planned pairs reach 2^25: max |q| goes to meta[1]
  unsigned long long *acc;    // [1 + ns][n_groups * n_bins]: rows per (group, bin), then the int64 sums of each field (two's complement)
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] a key beyond the slots
};

// the group slot of the pair (s1, s2) of one chromosome
__device__ __forceinline__ uint32_t group_of(const MapArgs &A, const uint4 a, const uint4 b) {
  return a.y + b.z + ((unsigned long long)a.w + b.w >= A.two_w ? 1u : 0u);
}

template <bool kLds>
__global__ __launch_bounds__(256) void map_kernel(MapArgs A) {
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

// ngsld_decay_map in four parts (record_pass.h AnalysisPass); it is no kind of ngsld_analyze
struct DecayMapPass final : AnalysisPass {
  const ngsld_decay_map_params *p;
  const char *const *labels;
  ngsld_decay_map_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_decay_map_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  struct Chr {
    std::string name;
    uint64_t first_site, last_site, first_win, slot0;  // first_win: the window of its first site; slot0: that window's slot
  };
  std::vector<Chr> chrs;
  uint64_t n_bins = 0, n_groups = 0, slots = 0, W = 0, n_pairs = 0;
  bool use_lds = false;
  DevBuf<uint4> d_site;
  DevBuf<unsigned long long> d_acc, d_meta;
  std::vector<unsigned long long> h_acc;
  MapArgs A{};

  DecayMapPass(const ngsld_decay_map_params *params, const char *const *site_labels, ngsld_decay_map_stats *out)
      : p(params), labels(site_labels), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_decay_map_params", stats, "ngsld_decay_map_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "decay map fields must be a non-empty mask of 1, 2, 4, 8");
    if (!(p->bin_size > 1.0) || !std::isfinite(p->bin_size)) return fail(c, NGSLD_ERR_INVALID, "decay map bin_size must be a finite number > 1");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "decay map max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "decay map min_maf is NaN");
    if (p->window >= (1ull << 31)) return fail(c, NGSLD_ERR_INVALID, "decay map window must be 0 (per chromosome) or an integer in [1, 2^31)");
    if (p->window > 0 && labels == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD decay map: a window needs positions: the labels are NULL");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.decay_map.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    const double B = p->bin_size;
    const uint64_t Wbp = p->window, U = 2 * Wbp;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
    const double limit = p->max_kb_dist * 1000.0;
    F.prepare(c, &p->min_maf);
    if (const int rc = F.check_limit(c, "decay map", limit)) return rc;
    const std::vector<double> &cum = F.cum;
    const std::vector<uint32_t> &infc = F.infc;

    // ---- groups: a chromosome is a run of sites between the +inf gaps of pos_dist; with a window, each label's CHR:pos ----
    std::vector<uint32_t> gq(n, 0), qa(n, 0), rem(n, 0);
    {
      std::vector<uint64_t> pos(Wbp > 0 ? n : 0);
      std::string prev_key;
      for (uint64_t s = 0; s < n; ++s) {
        const bool new_run = s == 0 || infc[s] != infc[s - 1];
        LabelPos L{std::string(), std::string::npos};
        if (labels != nullptr && (Wbp > 0 || new_run)) {
          if (labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD decay map: a label is NULL");
          L = label_pos(labels[s]);
        }
        if (Wbp > 0) {
          if (L.key == "(null)") return fail(c, NGSLD_ERR_INVALID, "LD decay map: a window needs positions: a label is \"(null)\"");
          if (!L.position(&pos[s]) || pos[s] >= (1ull << 62))
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD decay map: the position of label \"" + L.key + "\" is not plain decimal digits below 2^62");
          if (!new_run && pos[s] < pos[s - 1])
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD decay map: the position of site \"" + L.key + "\" is below that of the site before it, \"" +
                                                      prev_key + "\"");
          prev_key = L.key;
        }
        if (new_run) chrs.push_back({labels != nullptr ? L.chr() : std::to_string(chrs.size() + 1), s, s, 0, 0});
        chrs.back().last_site = s;
      }
      unsigned __int128 total = 0;  // (a chromosome of 2^62 bp in windows of 1 bp: counted before anything is narrowed)
      for (Chr &ch : chrs) {
        ch.slot0 = (uint64_t)std::min<unsigned __int128>(total, ~0ull);
        ch.first_win = Wbp > 0 ? pos[ch.first_site] / Wbp : 0;
        total += Wbp > 0 ? pos[ch.last_site] / Wbp - ch.first_win + 1 : 1;
      }
      n_groups = (uint64_t)std::min<unsigned __int128>(total, ~0ull);
      S.group_slots = n_groups;

      // ---- bins sized from the plan, as ngsld_decay sizes them: the largest finite planned dist, capped by the limit ----
      std::vector<double> chr_lo(chrs.size(), INFINITY), chr_hi(chrs.size(), -INFINITY);
      for (size_t k = 0; k < chrs.size(); ++k)
        for (uint64_t s = chrs[k].first_site; s <= chrs[k].last_site; ++s) {
          chr_lo[k] = std::min(chr_lo[k], cum[s]);
          chr_hi[k] = std::max(chr_hi[k], cum[s]);
        }
      double dmax = 0.0;
      for (size_t k = 0; k < chrs.size(); ++k)
        for (uint64_t s1 = chrs[k].first_site; s1 <= chrs[k].last_site; ++s1) {
          if (c->h_row_off[s1 + 1] == c->h_row_off[s1]) continue;
          const uint64_t s2 = std::min<uint64_t>(c->h_row_end[s1] - 1, chrs[k].last_site);
          if (s2 <= s1) continue;
          // gaps >= 0 (every position file): dist rises along the row; any other gaps: the chromosome's span bounds it
          const double d = F.exact_gaps ? cum[s2] - cum[s1] : chr_hi[k] - chr_lo[k];
          dmax = std::max(dmax, printed_dist(d));
        }
      if (dmax >= limit) dmax = limit;  // (dist < limit: the limit's own bin is the last one that can fill)
      const long long kmax = bin_of(dmax, B);
      n_bins = kmax >= 0 ? (uint64_t)kmax + 1 : 0;
      S.bin_slots = n_bins;
      const unsigned __int128 words = total * n_bins * (unsigned)(1 + ns);
      if (n_bins > (1ull << 32) || words * 8 > kMaxAccBytes)
        return fail(c, NGSLD_ERR_UNSUPPORTED, "LD decay map: " + std::to_string(n_groups) + (total > n_groups ? "+" : "") + " group slots x " +
                                                  std::to_string(n_bins) + " bins x " + std::to_string(1 + ns) +
                                                  " words of 8 B pass 1 GiB of accumulators: a larger window or bin_size is needed");

      // ---- per site: what the kernel adds up to a pair's slot ----
      for (const Chr &ch : chrs) {
        if (Wbp == 0) {
          for (uint64_t s = ch.first_site; s <= ch.last_site; ++s) gq[s] = (uint32_t)ch.slot0;
          continue;
        }
        // first_win = 2 * (pos_first / U) + (pos_first % U >= W): the slot of window w is slot0 + w - first_win
        const uint64_t q0 = pos[ch.first_site] / U, up = pos[ch.first_site] % U >= Wbp ? 1 : 0;
        for (uint64_t s = ch.first_site; s <= ch.last_site; ++s) {
          qa[s] = (uint32_t)(pos[s] / U - q0);  // (at most half the chromosome's slots: the cap holds them below 2^27)
          rem[s] = (uint32_t)(pos[s] % U);
          gq[s] = (uint32_t)(ch.slot0 - up) + qa[s];  // (modulo 2^32: with qa[s2] and the carry it is never below slot0)
        }
      }
    }
    slots = n_groups * n_bins;
    W = (uint64_t)(1 + ns) * slots;
    uint64_t lds_budget = kLdsBudget;
    if (const char *e = test_knob("DMAP_LDS_BYTES")) lds_budget = std::min<uint64_t>(std::strtoull(e, nullptr, 10), kLdsMax);
    use_lds = n_bins > 0 && (uint64_t)(1 + ns) * n_bins * 8 <= lds_budget;
    S.lds = use_lds ? 1 : 0;

    n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    if (W == 0 || n_pairs == 0) return NGSLD_OK;
    h_acc.assign(W, 0);
    std::vector<uint4> site(n);
    for (uint64_t s = 0; s < n; ++s) site[s] = make_uint4((infc[s] << 1) | (F.maf_ok[s] ? 1u : 0u), gq[s], qa[s], rem[s]);
    HIP_TRY(c, F.d_cum.resize(n));
    HIP_TRY(c, d_site.resize(n));
    HIP_TRY(c, d_acc.resize(W));
    HIP_TRY(c, d_meta.resize(3));
    HIP_TRY(c, hipMemcpy(F.d_cum.p, cum.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d_site.p, site.data(), n * sizeof(uint4), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, W * sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(unsigned long long), st));
    A.cum = F.d_cum.p;
    A.site = d_site.p;
    A.two_w = Wbp > 0 ? (uint32_t)U : 0xffffffffu;
    A.limit = limit;
    A.bin = B;
    A.n_sites = (uint32_t)n;
    A.n_bins = (uint32_t)n_bins;
    A.n_groups = (uint32_t)n_groups;
    A.ns = ns;
    for (int v = 0; v < ns; ++v) A.field4 |= (uint32_t)field[v] << (4 * v);
    // the sums stay on the device over every chunk: exact while max |q| * (the planned pairs) < 2^63, certain below 2^25 pairs
    A.track_max = track_sums(n_pairs >= (1ull << 25)) ? 1 : 0;
    A.acc = d_acc.p;
    A.meta = d_meta.p;
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
    const size_t lds_bytes = use_lds ? (size_t)(1 + ns) * n_bins * 8 : 0;
    client.kernel_ms = &S.kernel_ms;
    client.launch = [this, st, max_blocks, lds_bytes](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      A.out_base = ch.out_base;
      A.items = items;
      A.n_items = n_items;
      const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
      if (use_lds)
        hipLaunchKernelGGL(map_kernel<true>, dim3(blocks), dim3(256), lds_bytes, st, A);
      else
        hipLaunchKernelGGL(map_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
    };
    client.after = [this, c, st](const RecordChunk &) -> int {
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (meta[0] != 0) return fail_value_range(c, "decay map", meta[0]);
      if (meta[2] != 0) return fail(c, NGSLD_ERR_INVALID, "LD decay map: a row fell beyond the planned groups or bins (internal error)");
      return NGSLD_OK;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    hipStream_t st = c->stream;
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), d_acc.p, W * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (A.track_max && sum_may_wrap(meta[1], n_pairs))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a decay map of " + std::to_string(n_pairs) + " pairs with values too large to sum exactly");
    }

    // ---- the groups with rows, by chromosome and window (the order of the slots): exact integer sums, one rounding ----
    DecayMapResult &M = c->res.decay_map;
    const double B = p->bin_size;
    for (const Chr &ch : chrs) M.chr_name.push_back(ch.name);
    std::vector<double> lower(h_acc.empty() ? 0 : n_bins);  // (every group has the same breaks: formatted once, not once per group)
    for (uint64_t k = 0; k < lower.size(); ++k) lower[k] = break_value(k, B);
    for (size_t ci = 0; ci < chrs.size() && !h_acc.empty(); ++ci) {
      const uint64_t g1 = ci + 1 < chrs.size() ? chrs[ci + 1].slot0 : n_groups;
      for (uint64_t g = chrs[ci].slot0; g < g1; ++g) {
        const size_t before = M.count.size();
        for (uint64_t k = 0; k < n_bins; ++k) {
          const uint64_t rows = h_acc[g * n_bins + k];
          if (rows == 0) continue;
          M.dist.push_back(lower[k]);
          M.count.push_back(rows);
          S.pairs_counted += rows;
          for (int v = 0; v < ns; ++v) {
            const int64_t s = (int64_t)h_acc[(uint64_t)(1 + v) * slots + g * n_bins + k];
            const unsigned __int128 a = s < 0 ? (uint64_t)0 - (uint64_t)s : (uint64_t)s, b = (unsigned __int128)rows * 1000000u;
            const double m = div_nearest_small(a, b);  // (100 groups x 400 bins x 4 statistics: 160,000 of them)
            M.mean.push_back(s < 0 ? -m : m);
          }
        }
        if (M.count.size() == before) continue;
        M.chr.push_back((uint32_t)ci);
        M.win_start.push_back((chrs[ci].first_win + (g - chrs[ci].slot0)) * p->window);
        M.bin_off.push_back(before);
      }
    }
    M.bin_off.push_back(M.count.size());
    M.fields = p->fields;
    S.groups = M.chr.size();
    S.bins = M.count.size();
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

const char *const kNoResult = "no ngsld_decay_map result (it goes with the next ngsld_plan or ngsld_set_*)";

}  // namespace

extern "C" {

int ngsld_decay_map(ngsld_ctx *c, const ngsld_decay_map_params *p, const char *const *labels, ngsld_decay_map_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  DecayMapPass pass(p, labels, stats);
  pass.clear(c);  // (a refusal of the parameters leaves the store empty too)
  const int rc = run_single(c, pass, record_chunk(test_knob("DMAP_CHUNK_PAIRS")));
  if (rc != NGSLD_OK) pass.clear(c);
  return rc;
} NGSLD_CATCH(c)

int ngsld_decay_map_chromosomes(ngsld_ctx *c, uint64_t cap, const char **name, uint64_t *n_chr) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const DecayMapResult &M = c->res.decay_map;
  if (!M.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  if (n_chr) *n_chr = M.chr_name.size();
  if (name)
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, M.chr_name.size()); ++k) name[k] = M.chr_name[k].c_str();
  return NGSLD_OK;
}

int ngsld_decay_map_groups(ngsld_ctx *c, uint64_t cap, uint32_t *chr, uint64_t *win_start, uint64_t *first_bin, uint64_t *n_bins,
                           uint64_t *n_groups) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const DecayMapResult &M = c->res.decay_map;
  if (!M.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  const uint64_t m = M.chr.size(), k = std::min<uint64_t>(cap, m);
  if (n_groups) *n_groups = m;
  if (k == 0) return NGSLD_OK;
  if (chr) std::memcpy(chr, M.chr.data(), k * sizeof(uint32_t));
  if (win_start) std::memcpy(win_start, M.win_start.data(), k * sizeof(uint64_t));
  if (first_bin) std::memcpy(first_bin, M.bin_off.data(), k * sizeof(uint64_t));
  if (n_bins)
    for (uint64_t g = 0; g < k; ++g) n_bins[g] = M.bin_off[g + 1] - M.bin_off[g];
  return NGSLD_OK;
}

int ngsld_decay_map_bins(ngsld_ctx *c, uint64_t cap, double *dist, uint64_t *count, double *mean, uint64_t *n_bins) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const DecayMapResult &M = c->res.decay_map;
  if (!M.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  const uint64_t nb = M.count.size(), m = std::min<uint64_t>(cap, nb);
  if (n_bins) *n_bins = nb;
  const int nf = __builtin_popcount(M.fields);
  if (m > 0 && dist) std::memcpy(dist, M.dist.data(), m * sizeof(double));
  if (m > 0 && count) std::memcpy(count, M.count.data(), m * sizeof(uint64_t));
  if (m > 0 && mean) std::memcpy(mean, M.mean.data(), m * nf * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
