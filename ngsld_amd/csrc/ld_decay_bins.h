// ld_decay_bins.h -- the bins of LD decay (DECAY.md rules 4 and 5), shared by ngsld_decay (decay.hip) and ngsld_decay_map
// (decay_map.hip): dist as the TSV prints it, the right-closed bin of a dist, a bin's lower break as R labels it, the bins a plan
// can fill; then the one bin kernel behind both calls (bin_kernel, decay.hip) as its two hosts see it: its arguments, and DecayBins,
// the host side they have in common, which launches it.
#pragma once

#include <cstdio>
#include <cstdlib>

#include "record_pass.h"

// dist as the TSV prints it ("%.0f", read back): the exact binary value rounded half-to-even (exact for integer gaps)
__host__ __device__ inline double printed_dist(double x) { return __builtin_rint(x); }

// the right-closed bin (k*B, (k+1)*B] of d, with the breaks computed as R's seq(0, ., B) does (k * B); -1 for d <= 0
__host__ __device__ inline long long bin_of(double d, double B) {
  if (!(d > 0.0)) return -1;
  long long k = (long long)__builtin_ceil(d / B) - 1;
  if (k < 0) k = 0;
  while (k > 0 && !(d > (double)k * B)) --k;
  while (d > (double)(k + 1) * B) ++k;
  return k;
}

// R's as.character of a break (15 significant digits) read back
inline double break_value(uint64_t k, double B) {
  char buf[64];
  std::snprintf(buf, sizeof(buf), "%.15g", (double)k * B);
  return std::strtod(buf, nullptr);
}

// The bins sized from the plan: bins 0 .. the bin of the largest finite planned dist, capped by the limit (0: no planned pair has a
// bin).  infc and cum are dist_prefix's (engine.h), exact_gaps its answer: a chromosome is a run of one infc; row s1 is planned up
// to row_end[s1] where row_off[s1 + 1] > row_off[s1].
inline uint64_t planned_bins(const std::vector<uint32_t> &infc, const std::vector<double> &cum, bool exact_gaps,
                             const std::vector<uint64_t> &row_off, const std::vector<uint32_t> &row_end, double limit, double B) {
  const uint64_t n = infc.size();
  double dmax = 0.0;
  for (uint64_t first = 0, end; first < n; first = end) {  // the chromosome of sites first .. end - 1
    double lo = INFINITY, hi = -INFINITY;
    for (end = first; end < n && infc[end] == infc[first]; ++end) {
      lo = std::min(lo, cum[end]);
      hi = std::max(hi, cum[end]);
    }
    for (uint64_t s1 = first; s1 < end; ++s1) {
      if (row_off[s1 + 1] == row_off[s1]) continue;
      const uint64_t s2 = std::min<uint64_t>(row_end[s1], end) - 1;
      if (s2 <= s1) continue;
      // gaps >= 0 (every position file): dist rises along the row; any other gaps: the chromosome's span bounds it
      dmax = std::max(dmax, printed_dist(exact_gaps ? cum[s2] - cum[s1] : hi - lo));
    }
  }
  if (dmax >= limit) dmax = limit;  // (dist < limit: the limit's own bin is the last one that can fill)
  return (uint64_t)(bin_of(dmax, B) + 1);
}

// ---- the bin kernel (decay.hip) ----
struct DecayBinArgs {
  const ngsld_item *items;
  uint64_t n_items;
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint4 *site;          // per site, one 16 B load: x = infc << 1 | (printed maf >= min_maf); the group of a pair (decay_map.hip):
                              // y = gq (its chromosome's first slot + qa, less one where the first window begins in the upper half of
                              // a U), z = qa (pos / U less its chromosome's first), w = rem (pos % U)
  double limit;               // dist < limit (+inf: no limit)
  double bin;                 // bin size B
  uint32_t n_sites;
  uint32_t n_bins;            // bins 0 .. n_bins-1 of every group
  uint32_t n_groups;          // group slots
  uint32_t two_w;             // U = 2 W (no window: 2^32 - 1, and every rem is 0)
  int ns;                     // chosen fields
  uint32_t field4;            // ... four bits each: 0 r2_ExpG, 1 D, 2 D', 3 r2
  int track_max;              // max |q| goes to meta[1]
  unsigned long long *acc;    // [1 + ns][n_groups * n_bins]: rows per (group, bin), then the int64 sums of each field (two's complement)
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] a key beyond the slots
};

// The host side both calls have in common: the parameter checks, the site filter, the planned bins, the LDS decision, the device
// buffers, the kernel's arguments and launch, its two reports.  What differs stays with the caller: the groups (the site entries'
// y, z, w), its cap on the bins, when the accumulators are zeroed and read, track_max.
struct DecayBins {
  SiteFilter F;
  int ns = 0;
  uint64_t n_bins = 0, words = 0;  // words: (1 + ns) * n_groups * n_bins of A.acc
  bool use_lds = false;
  DevBuf<uint4> d_site;
  DevBuf<unsigned long long> d_acc, d_meta;
  DecayBinArgs A{};

  // the four parameters both calls take: "<pass> fields must ..." and so on
  static int check_params(ngsld_ctx *c, const char *pass, uint32_t fields, double bin_size, double max_kb_dist, double min_maf);
  // the filter's arrays, the refusal of a limit over inexact gaps, n_bins, use_lds (lds_knob: the call's test knob of the budget)
  int plan(ngsld_ctx *c, const char *pass, const char *lds_knob, uint32_t fields, double bin_size, double max_kb_dist, double min_maf);
  // the x of site s's entry: its chromosome and whether its printed maf passes (after plan)
  uint32_t site_x(uint64_t s) const { return (F.infc[s] << 1) | (F.maf_ok[s] ? 1u : 0u); }
  // the uploads of cum and the site entries, the buffers (the accumulators are the caller's to zero), A, client's launch
  int upload(ngsld_ctx *c, const std::vector<uint4> &site, uint64_t n_groups, uint32_t two_w, RecordPass::Client &client);
  // meta comes back once the stream is done; a value out of range (meta[0]) and a key beyond the slots (meta[2]: `beyond`) are refused
  int read_meta(ngsld_ctx *c, const char *pass, const char *beyond, unsigned long long meta[3]);
};

// ngsld_decay_bins and ngsld_decay_map_bins: up to cap bins of a result (results.h) copied out, *n_bins = how many it holds
template <class R>
void copy_out_bins(const R &res, uint64_t cap, double *dist, uint64_t *count, double *mean, uint64_t *n_bins) {
  const uint64_t nb = res.count.size(), m = std::min<uint64_t>(cap, nb);
  if (n_bins) *n_bins = nb;
  const int nf = __builtin_popcount(res.fields);
  if (m > 0 && dist) std::memcpy(dist, res.dist.data(), m * sizeof(double));
  if (m > 0 && count) std::memcpy(count, res.count.data(), m * sizeof(uint64_t));
  if (m > 0 && mean) std::memcpy(mean, res.mean.data(), m * nf * sizeof(double));
}
