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
//   bins     the bin kernel of decay.hip through its host side (DecayBins, ld_decay_bins.h), which ngsld_decay drives with one group
//   host     the accumulators stay on the device across the chunks and come back once; a bin's mean is the double nearest to
//            sum / (10^6 * rows) (append_bin_means, ld_mean.h)
#include "engine.h"
#include "ld_decay_bins.h"
#include "record_pass.h"

namespace {

// the accumulators of a call: (1 + fields) x group slots x bin slots x 8 B
constexpr uint64_t kMaxAccBytes = 1ull << 30;
const char *const kBeyond = "LD decay map: a row fell beyond the planned groups or bins (internal error)";

// ngsld_decay_map in four parts (record_pass.h AnalysisPass); it is no kind of ngsld_analyze
struct DecayMapPass final : AnalysisPass {
  const ngsld_decay_map_params *p;
  const char *const *labels;
  ngsld_decay_map_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_decay_map_stats S;
  DecayBins bins;
  struct Chr {
    std::string name;
    uint64_t first_site, last_site, first_win, slot0;  // first_win: the window of its first site; slot0: that window's slot
  };
  std::vector<Chr> chrs;
  uint64_t n_bins = 0, n_groups = 0, n_pairs = 0;
  std::vector<uint64_t> h_acc;

  DecayMapPass(const ngsld_decay_map_params *params, const char *const *site_labels, ngsld_decay_map_stats *out)
      : p(params), labels(site_labels), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_decay_map_params", stats, "ngsld_decay_map_stats")) return rc;
    if (const int rc = DecayBins::check_params(c, "decay map", p->fields, p->bin_size, p->max_kb_dist, p->min_maf)) return rc;
    if (p->window >= (1ull << 31)) return fail(c, NGSLD_ERR_INVALID, "decay map window must be 0 (per chromosome) or an integer in [1, 2^31)");
    if (p->window > 0 && labels == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD decay map: a window needs positions: the labels are NULL");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.decay_map.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    const uint64_t Wbp = p->window, U = 2 * Wbp;
    if (const int rc = bins.plan(c, "decay map", "DMAP_LDS_BYTES", p->fields, p->bin_size, p->max_kb_dist, p->min_maf)) return rc;
    const std::vector<uint32_t> &infc = bins.F.infc;
    const int ns = bins.ns;

    // ---- groups: a chromosome is a run of sites between the +inf gaps of pos_dist; with a window, each label's CHR:pos ----
    std::vector<uint4> site(n);
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
      S.bin_slots = n_bins = bins.n_bins;
      const unsigned __int128 words = total * n_bins * (unsigned)(1 + ns);
      if (n_bins > (1ull << 32) || words * 8 > kMaxAccBytes)
        return fail(c, NGSLD_ERR_UNSUPPORTED, "LD decay map: " + std::to_string(n_groups) + (total > n_groups ? "+" : "") + " group slots x " +
                                                  std::to_string(n_bins) + " bins x " + std::to_string(1 + ns) +
                                                  " words of 8 B pass 1 GiB of accumulators: a larger window or bin_size is needed");

      // ---- per site: its filter word, and what the kernel adds up to a pair's slot: gq, qa, rem ----
      for (const Chr &ch : chrs) {
        if (Wbp == 0) {
          for (uint64_t s = ch.first_site; s <= ch.last_site; ++s) site[s] = make_uint4(bins.site_x(s), (uint32_t)ch.slot0, 0, 0);
          continue;
        }
        // first_win = 2 * (pos_first / U) + (pos_first % U >= W): the slot of window w is slot0 + w - first_win
        const uint64_t q0 = pos[ch.first_site] / U, up = pos[ch.first_site] % U >= Wbp ? 1 : 0;
        for (uint64_t s = ch.first_site; s <= ch.last_site; ++s) {
          const uint32_t qa = (uint32_t)(pos[s] / U - q0);  // (at most half the chromosome's slots: the cap holds them below 2^27)
          // gq modulo 2^32: with qa[s2] and the carry it is never below slot0
          site[s] = make_uint4(bins.site_x(s), (uint32_t)(ch.slot0 - up) + qa, qa, (uint32_t)(pos[s] % U));
        }
      }
    }
    S.lds = bins.use_lds ? 1 : 0;
    n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    if (n_groups * n_bins == 0 || n_pairs == 0) return NGSLD_OK;
    if (const int rc = bins.upload(c, site, n_groups, Wbp > 0 ? (uint32_t)U : 0xffffffffu, client)) return rc;
    h_acc.assign(bins.words, 0);
    HIP_TRY(c, hipMemsetAsync(bins.d_acc.p, 0, bins.words * sizeof(unsigned long long), c->stream));
    // the sums stay on the device over every chunk: exact while max |q| * (the planned pairs) < 2^63, certain below 2^25 pairs
    bins.A.track_max = track_sums(n_pairs >= (1ull << 25)) ? 1 : 0;
    client.kernel_ms = &S.kernel_ms;
    client.after = [this, c](const RecordChunk &) -> int {
      unsigned long long meta[3] = {0, 0, 0};
      return bins.read_meta(c, "decay map", kBeyond, meta);
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { bins.A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      unsigned long long meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h_acc.data(), bins.d_acc.p, bins.words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      if (const int rc = bins.read_meta(c, "decay map", kBeyond, meta)) return rc;
      if (bins.A.track_max && sum_may_wrap(meta[1], n_pairs))
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a decay map of " + std::to_string(n_pairs) + " pairs with values too large to sum exactly");
    }

    // ---- the groups with rows, by chromosome and window (the order of the slots): exact integer sums, one rounding ----
    DecayMapResult &M = c->res.decay_map;
    const uint64_t slots = n_groups * n_bins;
    for (const Chr &ch : chrs) M.chr_name.push_back(ch.name);
    std::vector<double> lower(h_acc.empty() ? 0 : n_bins);  // (every group has the same breaks: formatted once, not once per group)
    for (uint64_t k = 0; k < lower.size(); ++k) lower[k] = break_value(k, p->bin_size);
    for (size_t ci = 0; ci < chrs.size() && !h_acc.empty(); ++ci) {
      const uint64_t g1 = ci + 1 < chrs.size() ? chrs[ci + 1].slot0 : n_groups;
      for (uint64_t g = chrs[ci].slot0; g < g1; ++g) {
        const size_t before = M.count.size();
        S.pairs_counted += append_bin_means(
            n_bins, h_acc.data() + g * n_bins, bins.ns,
            [&](int v, uint64_t k) { return (__int128)(int64_t)h_acc[(uint64_t)(1 + v) * slots + g * n_bins + k]; },
            [&](uint64_t k) { return lower[k]; }, M.dist, M.count, M.mean);
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
  if (!c->res.decay_map.valid()) return fail(c, NGSLD_ERR_INVALID, kNoResult);
  copy_out_bins(c->res.decay_map, cap, dist, count, mean, n_bins);
  return NGSLD_OK;
}

}  // extern "C"
