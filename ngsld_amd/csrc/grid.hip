// grid.hip -- the LD grid on the device (ngsld_grid, include/ngsld.h): a chromosome cut into windows of B bp and, for every pair
// of windows, the rows, sum, mean, maximum and linked rows of the site pairs between them -- the long form of the LD heat map
// along a whole chromosome -- from the pair records where they are computed; no TSV, a few numbers per cell leave the device.
// GRID.md has the rule, the refusals and why the sums are exact.
//
//   bins     host: each label's CHR:pos (up to the first TAB), bin(s) = pos / B; gbin[s] numbers the bins consecutively over the
//            chromosomes; the band K is the furthest a row's bins reach (from the plan's row_end); cell (s1, s2) is word
//            gbin[s1] * K + (gbin[s2] - gbin[s1]) of each of the 1 + 3 * fields accumulators
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   cells    one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the filters,
//            each chosen field as its printed value in integer micro-units (ld_prune.h).  The lanes of an item share s1 and
//            their gbin[s2] never decreases: they fall into a few runs of one cell.  One ballot numbers the runs, a segmented
//            scan merges each (counts, sums, maxima: six steps), and the run's last lane adds once per word -- never an atomic
//            per pair.  A workgroup takes a tile of kTileRows consecutive rows and keeps the cells of the tile's row bins x K
//            in LDS, flushed once with global 64-bit atomics; where that window is larger than pays (GRID.md), the same kernel without it:
//            a capped grid looping over the items, every run's add a global atomic.  Integer adds and maxima commute: every
//            launch shape and order gives the same bits.
//   host     the accumulators come back once, after the last chunk; a cell's mean is the double nearest to
//            sum / (10^6 * rows) (mean_nearest, ld_mean.h)
#include <unordered_set>

#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// LDS of a tile's cells.  The most a workgroup gets without asking the runtime for more is 64 KiB, but a tile zeroes and flushes
// its whole window, and the runs of a wavefront are merged before they add: measured (GRID.md), the tiles beat global atomics at
// windows of 0.7 and 2.3 KB (1.13x, 1.03x) and lose at 9.7 KB and beyond (0.96x ... 0.24x).  Windows up to kLdsDefault take the
// tiles; NGSLD_TEST_GRID_LDS_BYTES moves the limit anywhere up to kLdsMax.
constexpr uint32_t kLdsMax = 64u << 10, kLdsDefault = 4u << 10;
// rows of a tile
constexpr uint32_t kTileRows = 16;
// the accumulators of a call: (1 + 3 * fields) x cells x 8 B
constexpr uint64_t kMaxAccBytes = 2ull << 30;

struct GridArgs {
  const ngsld_item *items;    // the context's items, all of them
  const uint64_t *item_off;   // ... and how many lie before each row
  uint64_t i0, i1;            // the items of this launch
  uint64_t r0, r1;            // the chunk's rows
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  const uint32_t *gbin;       // a site's bin, numbered consecutively over the chromosomes
  double limit;               // dist <= limit (+inf: no limit)
  double linked_min;
  uint32_t n_sites;
  uint32_t band;              // K: a row's cells are words gbin[s1] * K + [0, K)
  uint32_t tile_rows;         // LDS path: consecutive rows a workgroup takes
  uint32_t tile_bins;         // ... which lie in bins [gbin of the first, + tile_bins)
  uint64_t cells;             // bins * K
  int ns;                     // chosen fields
  int field[4];               // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  int track_max;              // a cell may hold 2^25 rows or more: max |q| goes to meta[1]
  unsigned long long *acc;    // [1 + 3 * ns][cells]: rows; then per field the int64 sum (two's complement), the biased maximum, the linked rows
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] a cell beyond the band
};

// word w of cell (row bin, offset k): in the tile's LDS window where the row bin lies in it, else in global memory
template <bool kLds>
__device__ __forceinline__ void accumulate(const GridArgs &A, unsigned long long *lds, uint32_t base, uint32_t w, uint32_t row_bin,
                                           uint32_t k, unsigned long long v) {
  const uint32_t window = A.tile_bins * A.band;
  unsigned long long *p = (kLds && row_bin - base < A.tile_bins) ? lds + (size_t)w * window + (size_t)(row_bin - base) * A.band + k
                                                                 : A.acc + (size_t)w * A.cells + (size_t)row_bin * A.band + k;
  if (is_max_word(w))
    atomicMax(p, v);
  else
    atomicAdd(p, v);
}

template <bool kLds>
__global__ __launch_bounds__(256) void grid_kernel(GridArgs A) {
  extern __shared__ unsigned long long lds[];
  const int lane = (int)__lane_id();
  const uint32_t words = 1u + 3u * (uint32_t)A.ns;
  const uint32_t window = A.tile_bins * A.band;
  uint64_t first, end, step;
  uint32_t base = 0;
  if (kLds) {  // a workgroup per tile of rows: its items are consecutive
    const uint64_t ra = A.r0 + (uint64_t)blockIdx.x * A.tile_rows, rb = ra + A.tile_rows < A.r1 ? ra + A.tile_rows : A.r1;
    const uint64_t ib = A.item_off[ra] > A.i0 ? A.item_off[ra] : A.i0;
    end = A.item_off[rb] < A.i1 ? A.item_off[rb] : A.i1;
    if (ib >= end) return;  // (the whole workgroup: nothing of this tile in this launch)
    base = A.gbin[ra];
    for (uint32_t j = threadIdx.x; j < words * window; j += 256) lds[j] = 0;
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
    uint32_t key = 0xffffffffu;  // past the row: one run at the tail
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    if (c < it.count && s2 < A.n_sites) {
      key = A.gbin[s2];
      // (dist as the difference of the prefix sums: a finite limit is refused unless the gaps are integers, where the difference
      // is the printed value, and without a limit only finiteness matters)
      if (((it.mask >> c) & 1ull) && A.infc[s1] == A.infc[s2]  // (across a chromosome dist is not finite: never counted)
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
    }
    if (__ballot(take) == 0) continue;
    if (!take) q[0] = q[1] = q[2] = q[3] = 0;
    // rows in byte 0, the linked rows of field v in byte 1 + v: a run is at most 64 lanes, one shuffle carries all five counts
    unsigned long long counts = take ? 1ull : 0ull;
    unsigned long long top[4] = {0, 0, 0, 0};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v >= A.ns) break;
      if (take) {
        if ((double)q[v] / 1e6 >= A.linked_min) counts |= 1ull << (8 * (1 + v));  // the printed value read back (ld_prune.h), as doubles
        top[v] = (unsigned long long)(q[v] + (long long)kMaxBias);
        if (A.track_max) {
          const unsigned long long a = (unsigned long long)(q[v] < 0 ? -q[v] : q[v]);
          qmax = a > qmax ? a : qmax;
        }
      }
    }
    // runs of one cell (gbin[s2] rises with the lane; the numbering does not rely on it): heads marks each run's first lane
    const uint32_t prev = __shfl_up(key, 1);
    const uint64_t heads = __ballot(lane == 0 || prev != key);
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    for (int o = 1; o < 64; o <<= 1) {  // segmented inclusive scan: the run's last lane holds its totals
      // lane - o is of this lane's run iff no run begins in (lane - o, lane]  (every lane takes part in every shuffle)
      const bool add = lane >= o && ((heads >> (lane - o + 1)) & ((1ull << o) - 1ull)) == 0;
      const unsigned long long co = __shfl_up(counts, o);
      if (add) counts += co;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        const long long qo = __shfl_up(q[v], o);
        const unsigned long long to = __shfl_up(top[v], o);
        if (add) {
          q[v] += qo;
          top[v] = to > top[v] ? to : top[v];
        }
      }
    }
    const unsigned long long rows = counts & 0xffull;
    if (last && rows > 0) {
      const uint32_t row_bin = A.gbin[s1], k = key - row_bin;
      if (key >= row_bin && k < A.band && (uint64_t)row_bin * A.band + k < A.cells) {
        accumulate<kLds>(A, lds, base, 0, row_bin, k, rows);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (v >= A.ns) break;
          const uint32_t w = 1u + 3u * (uint32_t)v;
          const unsigned long long n_linked = (counts >> (8 * (1 + v))) & 0xffull;
          accumulate<kLds>(A, lds, base, w, row_bin, k, (unsigned long long)q[v]);
          accumulate<kLds>(A, lds, base, w + 1, row_bin, k, top[v]);
          if (n_linked) accumulate<kLds>(A, lds, base, w + 2, row_bin, k, n_linked);
        }
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
    for (uint32_t w = 0; w < words; ++w)
      for (uint32_t j = threadIdx.x; j < window; j += 256) {
        const unsigned long long v = lds[(size_t)w * window + j];
        const uint64_t cell = (uint64_t)base * A.band + j;
        if (v == 0 || cell >= A.cells) continue;
        if (is_max_word(w))
          atomicMax(A.acc + (size_t)w * A.cells + cell, v);
        else
          atomicAdd(A.acc + (size_t)w * A.cells + cell, v);
      }
  }
}

// ngsld_grid in four parts (record_pass.h AnalysisPass)
struct GridPass final : AnalysisPass {
  const ngsld_grid_params *p;
  const char *const *labels;
  ngsld_grid_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_grid_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  uint32_t words = 0;
  struct Chr {
    std::string name;
    uint64_t first_site, last_site, first_bin, gbin0;  // gbin0: the consecutive number of its first bin
  };
  std::vector<Chr> chrs;
  uint64_t n_bins = 0, band = 0, cells = 0, cell_rows = 0, tile_bins = 1;
  bool use_lds = false;
  size_t W = 0, lds_bytes = 0;
  std::vector<unsigned long long> h_acc;
  DevBuf<uint32_t> d_gbin;
  DevBuf<unsigned long long> d_acc, d_meta;
  GridArgs A{};

  GridPass(const ngsld_grid_params *params, const char *const *site_labels, ngsld_grid_stats *out)
      : p(params), labels(site_labels), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_grid_params", stats, "ngsld_grid_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "grid fields must be a non-empty mask of 1, 2, 4, 8");
    if (p->bin_size < 1 || p->bin_size >= (1ull << 31)) return fail(c, NGSLD_ERR_INVALID, "grid bin_size must be an integer in [1, 2^31)");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "grid max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "grid min_maf is NaN");
    if (std::isnan(p->linked_min)) return fail(c, NGSLD_ERR_INVALID, "grid linked_min is NaN");
    if (labels == nullptr) return fail(c, NGSLD_ERR_INVALID, "the LD grid needs positions: the labels are NULL");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.grid.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    words = 1u + 3u * (uint32_t)ns;
    const uint64_t B = p->bin_size;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
    const double limit = p->max_kb_dist * 1000.0;
    F.prepare(c, &p->min_maf);
    if (const int rc = F.check_limit(c, "grid", limit)) return rc;

    // ---- bins: each label's CHR:pos; a chromosome is a run of sites between the +inf gaps of pos_dist ----
    std::vector<uint32_t> gbin(n), chr_of(n);
    {
      std::unordered_set<std::string> seen;
      std::string prev_key;
      uint64_t prev_pos = 0;
      for (uint64_t s = 0; s < n; ++s) {
        if (labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "a label is NULL");
        const LabelPos L = label_pos(labels[s]);
        const std::string &key = L.key, name = L.chr();
        if (key == "(null)") return fail(c, NGSLD_ERR_INVALID, "the LD grid needs positions: a label is \"(null)\"");
        uint64_t pos = 0;
        if (!L.position(&pos)) return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: the position of label \"" + key + "\" is not plain decimal digits");
        const bool new_run = s == 0 || F.infc[s] != F.infc[s - 1];
        if (new_run) {
          if (s > 0 && name == chrs.back().name)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: site \"" + key + "\" is on the chromosome of the site before it, \"" + prev_key +
                                                      "\", but their distance is not finite");
          if (!seen.insert(name).second)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: chromosome \"" + name + "\" begins a second time at site \"" + key + "\"");
          if (!chrs.empty()) n_bins = chrs.back().gbin0 + (prev_pos / B - chrs.back().first_bin) + 1;
          chrs.push_back({name, s, s, pos / B, n_bins});
        } else {
          if (name != chrs.back().name)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: site \"" + key + "\" is on another chromosome than the site before it, \"" +
                                                      prev_key + "\", but their distance is finite");
          if (pos < prev_pos)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: the position of site \"" + key + "\" is below that of the site before it, \"" +
                                                      prev_key + "\"");
        }
        Chr &ch = chrs.back();
        ch.last_site = s;
        const uint64_t g = ch.gbin0 + (pos / B - ch.first_bin);
        if (g >= 0xffffffffull) return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: more than 2^32 - 1 bins up to site \"" + key + "\": a larger bin_size is needed");
        gbin[s] = (uint32_t)g;
        chr_of[s] = (uint32_t)(chrs.size() - 1);
        prev_key = key;
        prev_pos = pos;
      }
      if (!chrs.empty()) n_bins = chrs.back().gbin0 + (prev_pos / B - chrs.back().first_bin) + 1;
    }

    // ---- from the plan: the band (how many bins a row's candidates reach), the row bins of a tile, the rows a cell can hold ----
    for (uint64_t s = 0; s < n; ++s) {
      if (c->h_row_off[s + 1] == c->h_row_off[s] || c->h_row_end[s] <= s + 1) continue;
      const uint64_t far = std::min<uint64_t>(c->h_row_end[s] - 1, chrs[chr_of[s]].last_site);  // (never across a chromosome)
      band = std::max<uint64_t>(band, (uint64_t)gbin[far] - gbin[s] + 1);
    }
    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    S.bins = n_bins;
    S.band = band;
    cells = n_bins * band;  // (both below 2^32)
    if ((unsigned __int128)cells * words * 8 > kMaxAccBytes)
      return fail(c, NGSLD_ERR_UNSUPPORTED, "LD grid: " + std::to_string(n_bins) + " bins x a band of " + std::to_string(band) + " = " +
                                                std::to_string(cells) + " cells, whose accumulators pass 2 GiB: a larger bin_size is needed");
    // the most rows a cell can hold: the two largest bin populations p1 >= p2 give p1 * p2 between two bins and p1 * (p1 - 1) / 2
    // inside one; or every pair, if that is fewer
    {
      uint64_t top1 = 0, top2 = 0, run = 0;
      for (uint64_t s = 0; s < n; ++s) {
        run = (s > 0 && gbin[s] == gbin[s - 1]) ? run + 1 : 1;
        if (s + 1 == n || gbin[s + 1] != gbin[s]) {
          if (run > top1) {
            top2 = top1;
            top1 = run;
          } else if (run > top2) {
            top2 = run;
          }
        }
      }
      const unsigned __int128 most = std::max((unsigned __int128)top1 * top2, (unsigned __int128)top1 * (top1 - (top1 > 0)) / 2);
      cell_rows = most < n_pairs ? (uint64_t)most : n_pairs;
    }
    uint64_t lds_budget = kLdsDefault;
    if (const char *e = test_knob("GRID_LDS_BYTES")) lds_budget = std::min<uint64_t>(std::strtoull(e, nullptr, 10), kLdsMax);
    // The window of a tile: the row bins that 99 of 100 tiles span (a tile may begin at any row: a chunk does).  Not the largest
    // span: gbin counts the empty bins too, and one gap of megabases -- a centromere -- would size every tile for it.  The rows of a
    // tile that lie beyond the window add to global memory (accumulate).
    if (band > 0) {
      std::vector<uint32_t> spans(n);
      for (uint64_t s = 0; s < n; ++s) spans[s] = gbin[std::min<uint64_t>(s + kTileRows, n) - 1] - gbin[s] + 1;
      const auto q99 = spans.begin() + (n - 1) * 99 / 100;
      std::nth_element(spans.begin(), q99, spans.end());
      tile_bins = *q99;
    }
    use_lds = band > 0 && (unsigned __int128)words * tile_bins * band * 8 <= lds_budget;
    S.lds = use_lds ? 1 : 0;

    W = (size_t)words * cells;
    h_acc.assign(W, 0);
    if (n_pairs > 0 && cells > 0) {
      if (const int rc = F.upload(c)) return rc;
      HIP_TRY(c, d_gbin.resize(n));
      HIP_TRY(c, d_acc.resize(W));
      HIP_TRY(c, d_meta.resize(3));
      HIP_TRY(c, hipMemcpy(d_gbin.p, gbin.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, W * sizeof(unsigned long long), st));
      HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(unsigned long long), st));
      A.items = c->d_items.p;
      A.item_off = c->d_item_off.p;
      A.cum = F.d_cum.p;
      A.infc = F.d_infc.p;
      A.maf_ok = F.d_maf_ok.p;
      A.gbin = d_gbin.p;
      A.limit = limit;
      A.linked_min = p->linked_min;
      A.n_sites = (uint32_t)n;
      A.band = (uint32_t)band;
      A.tile_rows = kTileRows;
      A.tile_bins = (uint32_t)tile_bins;
      A.cells = cells;
      A.ns = ns;
      for (int v = 0; v < 4; ++v) A.field[v] = field[v];
      A.abs_value = p->abs_value != 0 ? 1 : 0;
      // every partial sum of a cell is exact while max |q| * (the rows it can hold) < 2^63: certain below 2^25 rows (|q| < 2^38)
      A.track_max = track_sums(cell_rows >= (1ull << 25)) ? 1 : 0;
      A.acc = d_acc.p;
      A.meta = d_meta.p;
      const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
      lds_bytes = use_lds ? (size_t)words * tile_bins * band * 8 : 0;
      client.kernel_ms = &S.grid_ms;
      client.launch = [this, c, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
        A.out_base = ch.out_base;
        A.r0 = ch.r0;
        A.r1 = ch.r1;
        A.i0 = (uint64_t)(items - c->d_items.p);
        A.i1 = A.i0 + n_items;
        if (use_lds) {
          const unsigned tiles = blocks_for(ch.r1 - ch.r0, A.tile_rows);
          hipLaunchKernelGGL(grid_kernel<true>, dim3(tiles), dim3(256), lds_bytes, st, A);
        } else {
          const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
          hipLaunchKernelGGL(grid_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
        }
      };
      client.after = [this, c, st](const RecordChunk &) -> int {
        unsigned long long meta[3] = {0, 0, 0};
        HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (meta[0] != 0) return fail_value_range(c, "grid", meta[0]);
        if (meta[2] != 0) return fail(c, NGSLD_ERR_INVALID, "LD grid: a pair beyond the band of its row (internal error)");
        return NGSLD_OK;
      };
    }
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
      if (A.track_max && sum_may_wrap(meta[1], cell_rows))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a grid cell of up to " + std::to_string(cell_rows) + " pairs with values too large to sum exactly");
    }

    // ---- the cells with rows, by chromosome, b1, b2 (the order of the words): exact integer sums, one rounding for the mean ----
    GridResult &G = c->res.grid;
    for (const Chr &ch : chrs) G.chr_name.push_back(ch.name);
    uint64_t n_cells = 0;
    for (uint64_t w = 0; w < cells; ++w) n_cells += h_acc[w] != 0;
    G.chr.reserve(n_cells);
    G.b1.reserve(n_cells);
    G.b2.reserve(n_cells);
    G.n.reserve(n_cells);
    size_t ci = 0;
    for (uint64_t g = 0; g < n_bins && band > 0; ++g) {
      while (ci + 1 < chrs.size() && chrs[ci + 1].gbin0 <= g) ++ci;
      const uint64_t b1 = chrs[ci].first_bin + (g - chrs[ci].gbin0);
      for (uint64_t k = 0; k < band; ++k) {
        const uint64_t rows = h_acc[g * band + k];
        if (rows == 0) continue;
        G.chr.push_back((uint32_t)ci);
        G.b1.push_back(b1);
        G.b2.push_back(b1 + k);
        G.n.push_back(rows);
        S.pairs_counted += rows;
      }
    }
    G.sum.resize((size_t)ns * n_cells);
    G.max.resize((size_t)ns * n_cells);
    G.linked.resize((size_t)ns * n_cells);
    G.mean.resize((size_t)ns * n_cells);
    for (int v = 0; v < ns; ++v) {
      size_t k = (size_t)v * n_cells;
      for (uint64_t w = 0; w < cells; ++w) {
        if (h_acc[w] == 0) continue;
        const FieldSummary f = field_summary(h_acc.data(), cells, v, w);
        G.sum[k] = f.sum;
        G.max[k] = f.max;
        G.linked[k] = f.linked;
        G.mean[k] = f.mean;
        ++k;
      }
    }
    G.fields = p->fields;
    S.cells = n_cells;
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_grid_pass(const ngsld_grid_params *p, const char *const *labels, ngsld_grid_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new GridPass(p, labels, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_grid(ngsld_ctx *c, const ngsld_grid_params *p, const char *const *labels, ngsld_grid_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  GridPass pass(p, labels, stats);
  return run_single(c, pass, record_chunk(test_knob("GRID_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_grid_cells(ngsld_ctx *c, uint64_t cap, uint32_t *chr, uint64_t *bin1, uint64_t *bin2, uint64_t *n, uint64_t *n_cells) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const GridResult &G = c->res.grid;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_grid result (it goes with the next ngsld_plan or ngsld_set_*)");
  const uint64_t m = G.n.size(), k = std::min<uint64_t>(cap, m);
  if (n_cells) *n_cells = m;
  if (k == 0) return NGSLD_OK;
  if (chr) std::memcpy(chr, G.chr.data(), k * sizeof(uint32_t));
  if (bin1) std::memcpy(bin1, G.b1.data(), k * sizeof(uint64_t));
  if (bin2) std::memcpy(bin2, G.b2.data(), k * sizeof(uint64_t));
  if (n) std::memcpy(n, G.n.data(), k * sizeof(uint64_t));
  return NGSLD_OK;
}

int ngsld_grid_chromosomes(ngsld_ctx *c, uint64_t cap, const char **name, uint64_t *n_chr) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const GridResult &G = c->res.grid;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_grid result (it goes with the next ngsld_plan or ngsld_set_*)");
  if (n_chr) *n_chr = G.chr_name.size();
  if (name)
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, G.chr_name.size()); ++k) name[k] = G.chr_name[k].c_str();
  return NGSLD_OK;
}

int ngsld_grid_get(ngsld_ctx *c, int field, uint64_t cap, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked, double *mean) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const GridResult &G = c->res.grid;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_grid result (it goes with the next ngsld_plan or ngsld_set_*)");
  const int v = field_rank(G.fields, field);
  if (v < 0) return fail(c, NGSLD_ERR_INVALID, "not a field of the last ngsld_grid (TSV column 4..7)");
  const size_t m = G.n.size(), at = (size_t)v * m, k = (size_t)std::min<uint64_t>(cap, m);
  if (k == 0) return NGSLD_OK;
  if (sum_micro) std::memcpy(sum_micro, G.sum.data() + at, k * sizeof(int64_t));
  if (max_micro) std::memcpy(max_micro, G.max.data() + at, k * sizeof(int64_t));
  if (linked) std::memcpy(linked, G.linked.data() + at, k * sizeof(uint64_t));
  if (mean) std::memcpy(mean, G.mean.data() + at, k * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
