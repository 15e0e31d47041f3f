// partners.hip -- LD partners on the device (ngsld_partners, include/ngsld.h): for every site (or every site of a query) the k
// sites that tag it best -- its partner rows ranked by (printed value descending, partner index ascending) -- and its count of
// partner rows; no TSV, k numbers per site leave the device.  PARTNERS.md has the rule, the deviations and why the insertion is
// exact.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   partners one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the
//            filters of the linked pairs (LINKED.md), the chosen field as its printed value q in integer micro-units
//            (ld_prune.h), and the key (q + 2^31) << 32 | (2^32 - 1 - partner): never 0 for |q| < 2^31, distinct within a site,
//            and its unsigned order is the rule's order.  slots[site][k], zeroed once, keep a site's k largest keys in
//            descending order through a chain of atomicMax (insert below): no lock, no sort pass, and every launch shape and
//            order gives the same bits.  The column end: a taking lane inserts (q, s1) into its own s2.  The row end: the 64
//            lanes share s1 -- the wavefront hands over its keys largest first, one lane inserting, and stops at the first
//            that s1's last slot already beats (at most k of them).
//   host     the slots and the counts come back once, after the last chunk, and are unpacked
#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

constexpr uint32_t kMaxK = 64;
constexpr long long kQLimit = 1ll << 31;  // |q| below it

struct PartnersArgs {
  const ngsld_item *items;    // the items of this launch
  uint64_t n_items;
  uint64_t out_base;          // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  const uint8_t *query;       // null: every site collects partners
  double limit;               // has_limit: dist <= limit
  double min_weight;
  int has_limit;              // a finite max_kb_dist was given; 0: no condition on dist at all
  int field;                  // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  uint32_t k;
  unsigned long long *slots;  // [n_sites][k] keys, descending; 0: empty
  unsigned long long *rows;   // [n_sites] partner rows of a collecting site
  unsigned long long *meta;   // [0] (s1 << 32 | s2) + 1 of a value of 2^31 micro-units or more, [1] partner rows
};

__device__ __forceinline__ unsigned long long peek(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// key into the k slots of one site.  Slot j ends as the maximum of every key that reached it and hands the others on to slot
// j + 1, so it ends as the (j + 1)-th largest; the last slot only grows, so a key at or below any reading of it is in no final
// slot and is dropped where it stands.
__device__ __forceinline__ void insert(unsigned long long *slot, uint32_t k, unsigned long long key) {
  const unsigned long long *last = slot + (k - 1);
  if (key <= peek(last)) return;
  unsigned long long carry = key;
  for (uint32_t j = 0; j < k; ++j) {
    const unsigned long long old = atomicMax(slot + j, carry);
    carry = old < carry ? old : carry;
    if (carry == 0 || carry <= peek(last)) break;
  }
}

__global__ __launch_bounds__(256) void partners_kernel(PartnersArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, step = (uint64_t)gridDim.x * 4;
  unsigned long long counted = 0;  // (lane 0)
  for (uint64_t i = first; i < A.n_items; i += step) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    bool take = false;
    long long q = 0;
    if (c < it.count && ((it.mask >> c) & 1ull) && A.maf_ok[s1] && A.maf_ok[s2] &&
        (!A.has_limit || (A.infc[s1] == A.infc[s2] && A.cum[s2] - A.cum[s1] <= A.limit))) {
      const double x = ngsld::field_of(A.rec[ngsld::record_of(it, c, A.out_base)], A.field);
      if (x - x == 0.0) {  // (not NaN or +-inf)
        int64_t m = 0;
        if (!ngsld::printed_micro(x, &m) || m >= kQLimit || m <= -kQLimit) {
          atomicCAS(A.meta, 0ull, (((unsigned long long)s1 << 32) | s2) + 1ull);
        } else {
          q = (A.abs_value && m < 0) ? -m : m;
          take = (double)q / 1e6 >= A.min_weight;  // the printed value read back (ld_prune.h), as doubles
        }
      }
    }
    const unsigned long long taken = __ballot(take);
    if (taken == 0) continue;
    const unsigned long long hi = (unsigned long long)(q + kQLimit) << 32;
    // the column end: this lane's site
    if (take && (A.query == nullptr || A.query[s2])) {
      insert(A.slots + (size_t)s2 * A.k, A.k, hi | (0xffffffffull - s1));
      atomicAdd(A.rows + s2, 1ull);
    }
    const unsigned long long n_taken = (unsigned long long)__popcll(taken);
    if (lane == 0) counted += n_taken;
    // the row end: the wavefront's keys, largest first
    if (A.query != nullptr && !A.query[s1]) continue;  // (the whole wavefront)
    if (lane == 0) atomicAdd(A.rows + s1, n_taken);
    unsigned long long key = take ? hi | (0xffffffffull - s2) : 0ull;
    unsigned long long *slot = A.slots + (size_t)s1 * A.k;
    const uint32_t rounds = n_taken < A.k ? (uint32_t)n_taken : A.k;
    for (uint32_t r = 0; r < rounds; ++r) {
      const unsigned long long m = ngsld::wave_max(key);
      unsigned long long floor_key = 0;
      if (lane == 0) floor_key = peek(slot + (A.k - 1));
      floor_key = __shfl(floor_key, 0);
      if (m <= floor_key) break;  // (the later maxima are smaller still)
      if (lane == 0) insert(slot, A.k, m);
      if (key == m) key = 0;
    }
  }
  if (lane == 0 && counted) atomicAdd(A.meta + 1, counted);
}

}  // namespace

extern "C" {

int ngsld_partners(ngsld_ctx *c, const ngsld_partners_params *p, const uint8_t *query, ngsld_partners_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const auto t_all = std::chrono::steady_clock::now();
  c->res.partners.clear();
  if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
  if (const int rc = check_struct_sizes(c, p, "ngsld_partners_params", stats, "ngsld_partners_stats")) return rc;
  if (p->k < 1 || p->k > kMaxK) return fail(c, NGSLD_ERR_INVALID, "partners k must be in 1..64");
  if (p->field < 4 || p->field > 7) return fail(c, NGSLD_ERR_INVALID, "partners field must be a TSV column 4..7");
  if (std::isnan(p->min_weight)) return fail(c, NGSLD_ERR_INVALID, "partners min_weight is NaN");
  if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "partners max_kb_dist must be >= 0");
  if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "partners min_maf is NaN");
  ngsld_partners_stats S;
  if (const int rc = begin_pass(c, S)) return rc;
  hipStream_t st = c->stream;
  const uint64_t n = c->n_sites;
  const uint32_t k = p->k;

  // ---- sites: the dist prefix sums (the limit comes from them), the maf filter on the printed maf ----
  SiteFilter F;
  F.prepare(c, &p->min_maf);
  const bool has_limit = std::isfinite(p->max_kb_dist);
  if (const int rc = F.check_limit(c, "partners", p->max_kb_dist)) return rc;
  const uint64_t chunk = record_chunk(test_knob("PARTNERS_CHUNK_PAIRS"));
  const uint64_t n_pairs = c->h_row_off[n];
  S.pairs = n_pairs;

  std::vector<unsigned long long> h_slots((size_t)n * k, 0), h_rows(n, 0);
  if (n_pairs > 0) {
    if (const int rc = F.upload(c)) return rc;
    DevBuf<unsigned long long> d_slots, d_rows, d_meta;
    DevBuf<uint8_t> d_query;
    HIP_TRY(c, d_slots.resize(h_slots.size()));
    HIP_TRY(c, d_rows.resize(n));
    HIP_TRY(c, d_meta.resize(2));
    HIP_TRY(c, hipMemsetAsync(d_slots.p, 0, h_slots.size() * sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemsetAsync(d_rows.p, 0, n * sizeof(unsigned long long), st));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 2 * sizeof(unsigned long long), st));
    if (query != nullptr) {
      HIP_TRY(c, d_query.resize(n));
      HIP_TRY(c, hipMemcpy(d_query.p, query, n, hipMemcpyHostToDevice));
    }
    RecordPass R;
    if (const int rc = R.open(c, chunk)) return rc;

    PartnersArgs A{};
    A.rec = R.records();
    A.cum = F.d_cum.p;
    A.infc = F.d_infc.p;
    A.maf_ok = F.d_maf_ok.p;
    A.query = query != nullptr ? d_query.p : nullptr;
    A.limit = p->max_kb_dist * 1000.0;
    A.min_weight = p->min_weight;
    A.has_limit = has_limit ? 1 : 0;
    A.field = p->field - 4;
    A.abs_value = p->abs_value != 0 ? 1 : 0;
    A.k = k;
    A.slots = d_slots.p;
    A.rows = d_rows.p;
    A.meta = d_meta.p;
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 8;

    // NGSLD_TEST_PARTNERS_PLANT_DP = "R:X" (tests): record R of the plan gets D' = X once its chunk's records are final.  Valid
    // haplotype frequencies give no finite D' near 2^31 micro-units, so this is the only way to the refusal of such a value
    uint64_t plant_at = ~0ull;
    double plant_dp = 0.0;
    if (const char *e = test_knob("PARTNERS_PLANT_DP")) {
      char *colon = nullptr;
      const uint64_t at = std::strtoull(e, &colon, 10);
      if (colon != e && *colon == ':') {
        plant_at = at;
        plant_dp = std::strtod(colon + 1, nullptr);
      }
    }

    const int rc = R.run(&S.pairs_ms, &S.kernel_ms, &S.chunks, [&](const RecordChunk &ch) -> int {
      if (plant_at < ch.out_base || plant_at - ch.out_base >= ch.pairs) return NGSLD_OK;
      HIP_TRY(c, hipMemcpyAsync(&R.records()[plant_at - ch.out_base].Dp, &plant_dp, sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      return NGSLD_OK;
    }, [&](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      A.out_base = ch.out_base;
      A.items = items;
      A.n_items = n_items;
      const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
      hipLaunchKernelGGL(partners_kernel, dim3(blocks), dim3(256), 0, st, A);
    }, [&](const RecordChunk &) -> int {
      unsigned long long bad = 0;
      HIP_TRY(c, hipMemcpyAsync(&bad, d_meta.p, sizeof(bad), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (bad == 0) return NGSLD_OK;
      const unsigned long long pair = bad - 1;
      return fail(c, NGSLD_ERR_UNSUPPORTED, "a partners value of the pair of sites " + std::to_string(pair >> 32) + " - " +
                                                std::to_string(pair & 0xffffffffull) + " reaches 2^31 micro-units (|x| >= 2147.483648)");
    });
    if (rc != NGSLD_OK) return rc;
    unsigned long long meta[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(h_slots.data(), d_slots.p, h_slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_rows.data(), d_rows.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    S.rows_counted = meta[1];
  }

  // ---- the lists: a key back into its partner and its value ----
  std::vector<uint32_t> partner((size_t)n * k, 0xffffffffu);
  std::vector<int64_t> value((size_t)n * k, 0);
  for (uint64_t s = 0; s < n; ++s) {
    if (h_rows[s] > 0) ++S.sites_with_partners;
    for (uint32_t j = 0; j < k; ++j) {
      const unsigned long long key = h_slots[(size_t)s * k + j];
      if (key == 0) break;  // (the slots fill from the front)
      partner[(size_t)s * k + j] = (uint32_t)(0xffffffffull - (key & 0xffffffffull));
      value[(size_t)s * k + j] = (int64_t)(key >> 32) - (int64_t)kQLimit;
      ++S.entries;
    }
  }
  c->res.partners.rows.assign(h_rows.begin(), h_rows.end());
  c->res.partners.partner.swap(partner);
  c->res.partners.value.swap(value);
  c->res.partners.k = k;
  c->res.partners.field = (uint32_t)p->field;
  S.total_ms = ms_since(t_all);
  copy_stats(stats, S);
  return NGSLD_OK;
} NGSLD_CATCH(c)

int ngsld_partners_info(ngsld_ctx *c, uint32_t *k, uint64_t *n_sites, uint32_t *field) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.partners.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_partners result (it goes with the next ngsld_plan or ngsld_set_*)");
  if (k) *k = c->res.partners.k;
  if (n_sites) *n_sites = c->res.partners.rows.size();
  if (field) *field = c->res.partners.field;
  return NGSLD_OK;
}

int ngsld_partners_get(ngsld_ctx *c, uint64_t *rows, uint32_t *partner, int64_t *value_micro) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.partners.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_partners result (it goes with the next ngsld_plan or ngsld_set_*)");
  const size_t n = c->res.partners.rows.size(), m = n * c->res.partners.k;
  if (n == 0) return NGSLD_OK;
  if (rows) std::memcpy(rows, c->res.partners.rows.data(), n * sizeof(uint64_t));
  if (partner) std::memcpy(partner, c->res.partners.partner.data(), m * sizeof(uint32_t));
  if (value_micro) std::memcpy(value_micro, c->res.partners.value.data(), m * sizeof(int64_t));
  return NGSLD_OK;
}

}  // extern "C"
