// cross.hip -- LD across chromosomes on the device (ngsld_cross_ld, include/ngsld.h): the whole-genome form of the LD grid.  For
// every pair of chromosomes, or of windows of B bp anywhere in the genome, the rows, sum, mean, maximum and linked rows of the
// site pairs between them -- the rows across two chromosomes (dist not finite) included -- from the pair records where they are
// computed; no TSV, a few numbers per cell leave the device.  CROSS.md has the rule, the refusals and the measurements; GRID.md
// why the sums are exact.
//
//   bins     host: a chromosome is a run of sites between the +inf gaps of pos_dist; with B > 0 each label's CHR:pos gives
//            bin(s) = pos / B; gbin[s] numbers the bins consecutively over the chromosomes (B == 0: the chromosome's ordinal).
//            Cell (s1, s2) is word tri(gbin[s1]) + (gbin[s2] - gbin[s1]) of each of the 1 + 3 * fields accumulators, with
//            tri(g) = g * bins - g * (g - 1) / 2: the upper triangle with its diagonal, row by row
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//   cells    one wavefront per work item, one lane per candidate (ld_records.h); the filters, the printed values and the run
//            numbering by one ballot plus a segmented scan are grid.hip's.  In an all-pairs plan a row is thousands of candidates
//            long: item after item falls into the same cell, and with a few hundred cells every wavefront of the device would add
//            to the same few words.  So a wavefront takes a contiguous span of M items of the launch and carries the totals of
//            its current cell in registers from item to item: an item's first run merges into the carry when its cell is the
//            carried one, inner runs add to memory at once, the item's last run becomes the new carry, and the carry is flushed
//            when the cell changes and at the span's end.  Integer adds and maxima commute: every span length, chunking and
//            slicing gives the same bits.
//   host     the accumulators stay on the device across the chunks and come back once; a cell's mean is the double nearest to
//            sum / (10^6 * rows) (field_summary, record_pass.h)
#include <unordered_set>

#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// items a wavefront carries its cell over: measured (CROSS.md), NGSLD_TEST_CROSS_SPAN_ITEMS moves it anywhere in [1, kSpanMax]
constexpr uint32_t kSpanDefault = 16, kSpanMax = 1u << 20;
// the accumulators of a call: (1 + 3 * fields) x bins * (bins + 1) / 2 x 8 B
constexpr uint64_t kMaxAccBytes = 2ull << 30;
constexpr unsigned long long kNoCell = ~0ull;

struct CrossArgs {
  const ngsld_item *items;    // the context's items, all of them
  uint64_t i0, i1;            // the items of this launch
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  const uint32_t *gbin;       // a site's bin, numbered consecutively over the chromosomes
  double min_dist;            // inside a chromosome: dist >= min_dist (-inf: no limit)
  double linked_min;
  uint32_t n_sites;
  uint32_t span;              // M: consecutive items a wavefront takes
  uint64_t bins;
  uint64_t cells;             // T = bins * (bins + 1) / 2
  int ns;                     // chosen fields
  int field[4];               // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  int within;                 // rows inside one chromosome count
  int track_max;              // a cell may hold 2^25 rows or more: max |q| goes to meta[1]
  unsigned long long *acc;    // [1 + 3 * ns][cells]: rows; then per field the int64 sum (two's complement), the biased maximum, the linked rows
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|, [2] a cell beyond the triangle
};

// the totals of one cell in full words: a carried cell holds far more than the 64 rows of a run
struct Totals {
  unsigned long long rows;
  long long sum[4];
  unsigned long long top[4], linked[4];
};

// one set of atomics: 1 + 3 * fields words of cell `cell` (the linked rows only where there are some)
__device__ __forceinline__ void add_cell(const CrossArgs &A, unsigned long long cell, const Totals &t) {
  atomicAdd(A.acc + cell, t.rows);
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if (v >= A.ns) break;
    unsigned long long *p = A.acc + (size_t)(1 + 3 * v) * A.cells + cell;
    atomicAdd(p, (unsigned long long)t.sum[v]);
    atomicMax(p + A.cells, t.top[v]);
    if (t.linked[v]) atomicAdd(p + 2 * A.cells, t.linked[v]);
  }
}

__global__ __launch_bounds__(256) void cross_kernel(CrossArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  // a contiguous span of the launch's items, never beyond them
  const uint64_t first = A.i0 + wave * A.span;
  if (first >= A.i1) return;  // (the whole wavefront)
  const uint64_t end = A.i1 - first < A.span ? A.i1 : first + A.span;
  unsigned long long qmax = 0;
  // the carried cell and its totals, the same in every lane
  unsigned long long c_cell = kNoCell;
  Totals C = {};
  for (uint64_t i = first; i < end; ++i) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    uint32_t key = 0xffffffffu;  // past the row: one run at the tail
    bool take = false;
    long long q[4] = {0, 0, 0, 0};
    if (c < it.count && s2 < A.n_sites) {
      key = A.gbin[s2];
      if (((it.mask >> c) & 1ull) && A.maf_ok[s1] && A.maf_ok[s2]) {
        // across two chromosomes dist is not finite and the row counts; inside one it is the difference of the prefix sums (a
        // limit is refused unless the gaps are integers, where the difference is the printed value)
        const bool same = A.infc[s1] == A.infc[s2];
        if (!same || (A.within && A.cum[s2] - A.cum[s1] >= A.min_dist)) {
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
    }
    if (__ballot(take) == 0) continue;  // (the carry stays)
    if (!take) q[0] = q[1] = q[2] = q[3] = 0;
    // inside an item a run is at most 64 lanes: rows in byte 0, the linked rows of field v in byte 1 + v, as in grid.hip.  They
    // are unpacked into full words before they meet the carry.
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
    // this lane's run in full words, and its cell in the triangle
    Totals R;
    R.rows = counts & 0xffull;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      R.sum[v] = q[v];
      R.top[v] = top[v];
      R.linked[v] = (counts >> (8 * (1 + v))) & 0xffull;
    }
    const uint64_t g1 = A.gbin[s1];
    bool mine = last && R.rows > 0;
    unsigned long long cell = kNoCell;
    if (mine) {
      if (key >= g1 && key < A.bins) {
        cell = g1 * A.bins - g1 * (g1 - (g1 > 0)) / 2 + (key - g1);
      } else {
        atomicOr(A.meta + 2, 1ull);  // (the bins say this cannot happen: reported, never written)
        mine = false;
      }
    }
    const uint64_t runs = __ballot(mine);
    if (runs == 0) continue;
    const int lf = __ffsll((long long)runs) - 1, ll = 63 - __clzll((long long)runs);
    // the item's last run, in every lane
    const unsigned long long n_cell = __shfl(cell, ll);
    Totals N = {};
    N.rows = __shfl(R.rows, ll);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v >= A.ns) break;
      N.sum[v] = __shfl(R.sum[v], ll);
      N.top[v] = __shfl(R.top[v], ll);
      N.linked[v] = __shfl(R.linked[v], ll);
    }
    const unsigned long long f_cell = __shfl(cell, lf);
    if (n_cell == c_cell) {  // (every branch on the carry is the wavefront's: its cell is the same in every lane)
      C.rows += N.rows;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if (v >= A.ns) break;
        C.sum[v] += N.sum[v];
        C.top[v] = N.top[v] > C.top[v] ? N.top[v] : C.top[v];
        C.linked[v] += N.linked[v];
      }
    } else {
      if (lf != ll && f_cell == c_cell) {  // the first run takes the carry with it
        if (lane == lf) {
          R.rows += C.rows;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (v >= A.ns) break;
            R.sum[v] += C.sum[v];
            R.top[v] = C.top[v] > R.top[v] ? C.top[v] : R.top[v];
            R.linked[v] += C.linked[v];
          }
        }
      } else if (c_cell != kNoCell && lane == 0) {
        add_cell(A, c_cell, C);
      }
      c_cell = n_cell;
      C = N;
    }
    if (mine && lane != ll) add_cell(A, cell, R);  // the runs before the last
  }
  if (c_cell != kNoCell && lane == 0) add_cell(A, c_cell, C);
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
}

// ngsld_cross_ld in four parts (record_pass.h AnalysisPass); it is no kind of ngsld_analyze
struct CrossPass final : AnalysisPass {
  const ngsld_cross_ld_params *p;
  const char *const *labels;
  ngsld_cross_ld_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_cross_ld_stats S;
  SiteFilter F;
  int field[4] = {0, 0, 0, 0};
  int ns = 0;
  uint32_t words = 0;
  struct Chr {
    std::string name;
    uint64_t first_bin, gbin0;  // the bin of its first site; the consecutive number of that bin
  };
  std::vector<Chr> chrs;
  uint64_t n_bins = 0, cells = 0, cell_rows = 0;
  size_t W = 0;
  std::vector<unsigned long long> h_acc;
  DevBuf<uint32_t> d_gbin;
  DevBuf<unsigned long long> d_acc, d_meta;
  CrossArgs A{};
  uint64_t plant_at = ~0ull;
  double plant_dp = 0.0;

  CrossPass(const ngsld_cross_ld_params *params, const char *const *site_labels, ngsld_cross_ld_stats *out)
      : p(params), labels(site_labels), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_cross_ld_params", stats, "ngsld_cross_ld_stats")) return rc;
    if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: fields must be a non-empty mask of 1, 2, 4, 8");
    if (p->bin_size >= (1ull << 31)) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: bin_size must be 0 (per chromosome) or an integer in [1, 2^31)");
    if (std::isnan(p->min_kb_dist) || p->min_kb_dist < 0 || std::isinf(p->min_kb_dist))
      return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: min_kb_dist must be a number >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: min_maf is NaN");
    if (std::isnan(p->linked_min)) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: linked_min is NaN");
    if (p->bin_size > 0 && labels == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: a bin_size needs positions: the labels are NULL");
    bool any_gap = false;
    for (uint64_t s = 0; s < c->n_sites && !any_gap; ++s) any_gap = std::isfinite(c->h_pos_dist[s]);
    if (!any_gap) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: the context has no position gaps (ngsld_set_pos_dist): every site would be a chromosome");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.cross.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;
    ns = field_list(p->fields, field);
    words = 1u + 3u * (uint32_t)ns;
    const uint64_t B = p->bin_size;

    // ---- sites: the dist prefix sums, the maf filter on the printed maf ----
    F.prepare(c, &p->min_maf);
    if (const int rc = F.check_limit(c, "LD across chromosomes: min_kb_dist as", p->min_kb_dist > 0 ? p->min_kb_dist * 1000.0 : (double)INFINITY))
      return rc;

    // ---- bins: a chromosome is a run of sites between the +inf gaps of pos_dist; its name and, with B > 0, the positions
    // come from the labels' CHR:pos ----
    std::vector<uint32_t> gbin(n);
    {
      std::unordered_set<std::string> seen;
      std::string prev_key, prev_name;
      uint64_t prev_pos = 0;
      for (uint64_t s = 0; s < n; ++s) {
        const bool new_run = s == 0 || F.infc[s] != F.infc[s - 1];
        std::string key, name;
        uint64_t pos = 0;
        if (labels != nullptr) {
          if (labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: a label is NULL");
          const LabelPos L = label_pos(labels[s]);
          key = L.key;
          name = L.chr();
          if (B > 0) {
            if (key == "(null)") return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: a bin_size needs positions: a label is \"(null)\"");
            if (!L.position(&pos))
              return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: the position of label \"" + key + "\" is not plain decimal digits");
          }
        } else if (new_run) {
          name = std::to_string(chrs.size() + 1);
        } else {
          name = prev_name;
        }
        if (new_run) {
          if (s > 0 && name == prev_name)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: site \"" + key + "\" is on the chromosome of the site before it, \"" +
                                                      prev_key + "\", but their distance is not finite");
          if (!seen.insert(name).second)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: chromosome \"" + name + "\" begins a second time at site \"" + key + "\"");
          if (!chrs.empty()) n_bins = chrs.back().gbin0 + (B > 0 ? prev_pos / B - chrs.back().first_bin : 0) + 1;
          chrs.push_back({name, B > 0 ? pos / B : 0, n_bins});
        } else {
          if (name != prev_name)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: site \"" + key + "\" is on another chromosome than the site before it, \"" +
                                                      prev_key + "\", but their distance is finite");
          if (pos < prev_pos)
            return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: the position of site \"" + key + "\" is below that of the site before it, \"" +
                                                      prev_key + "\"");
        }
        const Chr &ch = chrs.back();
        const uint64_t g = ch.gbin0 + (B > 0 ? pos / B - ch.first_bin : 0);
        if (g >= 0xffffffffull)
          return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: more than 2^32 - 1 bins up to site \"" + key + "\": a larger bin_size is needed");
        gbin[s] = (uint32_t)g;
        prev_key = key;
        prev_name = name;
        prev_pos = pos;
      }
      if (!chrs.empty()) n_bins = chrs.back().gbin0 + (B > 0 ? prev_pos / B - chrs.back().first_bin : 0) + 1;
    }
    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    S.bins = n_bins;
    const unsigned __int128 tri = (unsigned __int128)n_bins * (n_bins + 1) / 2;
    if (tri * words * 8 > kMaxAccBytes)
      return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: " + std::to_string(n_bins) + " bins make " +
                                                std::to_string((uint64_t)std::min<unsigned __int128>(tri, ~0ull)) +
                                                " cells, whose accumulators pass 2 GiB: a larger bin_size is needed");
    cells = (uint64_t)tri;
    // the most rows a cell can hold (GRID.md): the two largest bin populations p1 >= p2 give p1 * p2 between two bins and
    // p1 * (p1 - 1) / 2 inside one; or every pair, if that is fewer
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
    uint64_t span = kSpanDefault;
    if (const char *e = test_knob("CROSS_SPAN_ITEMS")) span = std::max<uint64_t>(1, std::min<uint64_t>(std::strtoull(e, nullptr, 10), kSpanMax));
    S.span_items = span;
    S.lds = 0;

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
      A.cum = F.d_cum.p;
      A.infc = F.d_infc.p;
      A.maf_ok = F.d_maf_ok.p;
      A.gbin = d_gbin.p;
      A.min_dist = p->min_kb_dist > 0 ? p->min_kb_dist * 1000.0 : -(double)INFINITY;
      A.linked_min = p->linked_min;
      A.n_sites = (uint32_t)n;
      A.span = (uint32_t)span;
      A.bins = n_bins;
      A.cells = cells;
      A.ns = ns;
      for (int v = 0; v < 4; ++v) A.field[v] = field[v];
      A.abs_value = p->abs_value != 0 ? 1 : 0;
      A.within = p->within != 0 ? 1 : 0;
      // every partial sum of a cell is exact while max |q| * (the rows it can hold) < 2^63: certain below 2^25 rows (|q| < 2^38)
      A.track_max = track_sums(cell_rows >= (1ull << 25)) ? 1 : 0;
      A.acc = d_acc.p;
      A.meta = d_meta.p;
      // NGSLD_TEST_CROSS_PLANT_DP = "R:X" (tests): record R of the plan gets D' = X once its chunk's records are final, as
      // NGSLD_TEST_SCAN_PLANT_DP does (scan.hip): no input gives a finite D' near 2^38 micro-units
      if (const char *e = test_knob("CROSS_PLANT_DP")) {
        char *colon = nullptr;
        const uint64_t at = std::strtoull(e, &colon, 10);
        if (colon != e && *colon == ':') {
          plant_at = at;
          plant_dp = std::strtod(colon + 1, nullptr);
        }
      }
      if (plant_at != ~0ull)
        client.before = [this, c, st](const RecordChunk &ch) -> int {
          if (plant_at < ch.out_base || plant_at - ch.out_base >= ch.pairs) return NGSLD_OK;
          HIP_TRY(c, hipMemcpyAsync(const_cast<double *>(&A.rec[plant_at - ch.out_base].Dp), &plant_dp, sizeof(double), hipMemcpyHostToDevice, st));
          HIP_TRY(c, hipStreamSynchronize(st));
          return NGSLD_OK;
        };
      client.kernel_ms = &S.cross_ms;
      client.launch = [this, c, st](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
        A.out_base = ch.out_base;
        A.i0 = (uint64_t)(items - c->d_items.p);
        A.i1 = A.i0 + n_items;  // (a span never crosses the launch's items)
        const uint64_t waves = (n_items + A.span - 1) / A.span;
        hipLaunchKernelGGL(cross_kernel, dim3(blocks_for(waves * 64)), dim3(256), 0, st, A);
      };
      client.after = [this, c, st](const RecordChunk &) -> int {
        unsigned long long meta[3] = {0, 0, 0};
        HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (meta[0] != 0) return fail_value_range(c, "LD across chromosomes", meta[0]);
        if (meta[2] != 0) return fail(c, NGSLD_ERR_INVALID, "LD across chromosomes: a pair beyond the triangle of its bins (internal error)");
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
        return fail(c, NGSLD_ERR_UNSUPPORTED, "LD across chromosomes: a cell of up to " + std::to_string(cell_rows) +
                                                  " pairs with values too large to sum exactly");
    }

    // ---- the cells with rows, by (gbin1, gbin2) -- the order of the words: exact integer sums, one rounding for the mean ----
    CrossResult &G = c->res.cross;
    for (const Chr &ch : chrs) G.chr_name.push_back(ch.name);
    uint64_t n_cells = 0;
    for (uint64_t w = 0; w < cells; ++w) n_cells += h_acc[w] != 0;
    G.chr1.reserve(n_cells);
    G.chr2.reserve(n_cells);
    G.b1.reserve(n_cells);
    G.b2.reserve(n_cells);
    G.n.reserve(n_cells);
    size_t c1 = 0;
    uint64_t w = 0;
    for (uint64_t g1 = 0; g1 < n_bins; ++g1) {
      while (c1 + 1 < chrs.size() && chrs[c1 + 1].gbin0 <= g1) ++c1;
      size_t c2 = c1;
      for (uint64_t g2 = g1; g2 < n_bins; ++g2, ++w) {
        const uint64_t rows = h_acc[w];
        if (rows == 0) continue;
        while (c2 + 1 < chrs.size() && chrs[c2 + 1].gbin0 <= g2) ++c2;
        G.chr1.push_back((uint32_t)c1);
        G.chr2.push_back((uint32_t)c2);
        G.b1.push_back(chrs[c1].first_bin + (g1 - chrs[c1].gbin0));
        G.b2.push_back(chrs[c2].first_bin + (g2 - chrs[c2].gbin0));
        G.n.push_back(rows);
        S.pairs_counted += rows;
        if (c1 != c2) S.pairs_cross += rows;
      }
    }
    G.sum.resize((size_t)ns * n_cells);
    G.max.resize((size_t)ns * n_cells);
    G.linked.resize((size_t)ns * n_cells);
    G.mean.resize((size_t)ns * n_cells);
    for (int v = 0; v < ns; ++v) {
      size_t k = (size_t)v * n_cells;
      for (uint64_t x = 0; x < cells; ++x) {
        if (h_acc[x] == 0) continue;
        const FieldSummary f = field_summary(h_acc.data(), cells, v, x);
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

const char *const kNoResult = "no ngsld_cross_ld result (it goes with the next ngsld_plan or ngsld_set_*)";

}  // namespace

extern "C" {

int ngsld_cross_ld(ngsld_ctx *c, const ngsld_cross_ld_params *p, const char *const *labels, ngsld_cross_ld_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  CrossPass pass(p, labels, stats);
  pass.clear(c);  // (a refusal of the parameters leaves the store empty too)
  const int rc = run_single(c, pass, record_chunk(test_knob("CROSS_CHUNK_PAIRS")));
  if (rc != NGSLD_OK) pass.clear(c);
  return rc;
} NGSLD_CATCH(c)

int ngsld_cross_ld_cells(ngsld_ctx *c, uint64_t cap, uint32_t *chr1, uint64_t *bin1, uint32_t *chr2, uint64_t *bin2, uint64_t *n,
                         uint64_t *n_cells) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const CrossResult &G = c->res.cross;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  const uint64_t m = G.n.size(), k = std::min<uint64_t>(cap, m);
  if (n_cells) *n_cells = m;
  if (k == 0) return NGSLD_OK;
  if (chr1) std::memcpy(chr1, G.chr1.data(), k * sizeof(uint32_t));
  if (bin1) std::memcpy(bin1, G.b1.data(), k * sizeof(uint64_t));
  if (chr2) std::memcpy(chr2, G.chr2.data(), k * sizeof(uint32_t));
  if (bin2) std::memcpy(bin2, G.b2.data(), k * sizeof(uint64_t));
  if (n) std::memcpy(n, G.n.data(), k * sizeof(uint64_t));
  return NGSLD_OK;
}

int ngsld_cross_ld_chromosomes(ngsld_ctx *c, uint64_t cap, const char **name, uint64_t *n_chr) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const CrossResult &G = c->res.cross;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  if (n_chr) *n_chr = G.chr_name.size();
  if (name)
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, G.chr_name.size()); ++k) name[k] = G.chr_name[k].c_str();
  return NGSLD_OK;
}

int ngsld_cross_ld_get(ngsld_ctx *c, int field, uint64_t cap, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked, double *mean) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const CrossResult &G = c->res.cross;
  if (!G.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  const int v = field_rank(G.fields, field);
  if (v < 0) return fail(c, NGSLD_ERR_INVALID, "not a field of the last ngsld_cross_ld (TSV column 4..7)");
  const size_t m = G.n.size(), at = (size_t)v * m, k = (size_t)std::min<uint64_t>(cap, m);
  if (k == 0) return NGSLD_OK;
  if (sum_micro) std::memcpy(sum_micro, G.sum.data() + at, k * sizeof(int64_t));
  if (max_micro) std::memcpy(max_micro, G.max.data() + at, k * sizeof(int64_t));
  if (linked) std::memcpy(linked, G.linked.data() + at, k * sizeof(uint64_t));
  if (mean) std::memcpy(mean, G.mean.data() + at, k * sizeof(double));
  return NGSLD_OK;
}

}  // extern "C"
