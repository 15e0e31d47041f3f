// analyze.hip -- several record passes over one run of the pair kernels (ngsld_analyze, include/ngsld.h).  ANALYZE.md has the
// rule.  Each listed analysis is the object its single call runs (record_pass.h AnalysisPass: prune.hip, decay.hip, site_ld.hip,
// cluster.hip, grid.hip, scan.hip); what is here is the list: its checks, the stores it empties, one run_passes over all of it.
// Host code only.
#include "engine.h"
#include "record_pass.h"

namespace {

std::unique_ptr<AnalysisPass> make_pass(const ngsld_analysis &a) {
  switch (a.kind) {
    case NGSLD_AN_PRUNE:
      return make_prune_pass((const ngsld_prune_params *)a.params, a.labels, a.site_state, (ngsld_prune_stats *)a.stats);
    case NGSLD_AN_DECAY:
      return make_decay_pass((const ngsld_decay_params *)a.params, (ngsld_decay_stats *)a.stats);
    case NGSLD_AN_SITE_LD:
      return make_site_ld_pass((const ngsld_site_ld_params *)a.params, (ngsld_site_ld_stats *)a.stats);
    case NGSLD_AN_CLUSTERS:
      return make_clusters_pass((const ngsld_clusters_params *)a.params, (ngsld_clusters_stats *)a.stats);
    case NGSLD_AN_GRID:
      return make_grid_pass((const ngsld_grid_params *)a.params, a.labels, (ngsld_grid_stats *)a.stats);
    case NGSLD_AN_SCAN:
      return make_scan_pass((const ngsld_scan_params *)a.params, (ngsld_scan_stats *)a.stats);
  }
  return nullptr;
}

}  // namespace

extern "C" {

int ngsld_analyze(ngsld_ctx *c, ngsld_analysis *list, uint32_t n, ngsld_analyze_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const auto t_all = std::chrono::steady_clock::now();
  if (stats != nullptr && stats->struct_size < sizeof(uint32_t)) return fail(c, NGSLD_ERR_INVALID, "ngsld_analyze_stats: struct_size not set");
  ngsld_analyze_stats S;
  std::memset(&S, 0, sizeof(S));
  S.struct_size = sizeof(S);
  S.n_analyses = n;
  copy_stats(stats, S);  // (a refusal leaves pairs_run 0: the pair kernels did not start)
  if (list == nullptr || n == 0) return fail(c, NGSLD_ERR_INVALID, "ngsld_analyze: the list of analyses is empty");

  // ---- the list: every entry a known kind, once ----
  // (a list that is refused empties the stores of the kinds it names all the same: the first fault is kept until they are)
  std::vector<std::unique_ptr<AnalysisPass>> passes;
  std::string fault;
  uint32_t seen = 0;
  for (uint32_t k = 0; k < n; ++k) {
    std::unique_ptr<AnalysisPass> pass;
    std::string what;
    if (list[k].struct_size != sizeof(ngsld_analysis))
      what = "ngsld_analysis: struct_size must be sizeof(ngsld_analysis)";
    else if (!(pass = make_pass(list[k])))
      what = "ngsld_analyze: analysis " + std::to_string(k) + " has the unknown kind " + std::to_string(list[k].kind);
    else if ((seen >> list[k].kind) & 1u)
      what = "ngsld_analyze: kind " + std::to_string(list[k].kind) + " is listed twice (a context keeps one result per kind)";
    if (fault.empty()) fault = what;
    if (!pass) continue;
    seen |= 1u << list[k].kind;
    passes.push_back(std::move(pass));
  }
  // ---- every listed store empty from here on, whatever happens; on success the finishes fill them ----
  struct Stores {
    ngsld_ctx *c;
    std::vector<std::unique_ptr<AnalysisPass>> &passes;
    bool keep = false;
    void clear() {
      for (auto &pass : passes) pass->clear(c);
    }
    ~Stores() {
      if (!keep) clear();
    }
  } stores{c, passes};
  stores.clear();
  if (!fault.empty()) return fail(c, NGSLD_ERR_INVALID, fault);
  // ---- every entry's parameters, before any device work: the single call's message ----
  for (auto &pass : passes)
    if (const int rc = pass->validate(c)) return rc;

  std::vector<AnalysisPass *> ptrs;
  for (auto &pass : passes) ptrs.push_back(pass.get());
  RecordPass::Shared sh;
  const int rc = run_passes(c, ptrs.data(), ptrs.size(), record_chunk(test_knob("ANALYZE_CHUNK_PAIRS")), &sh);
  S.pairs = c->h_row_off[c->n_sites];
  S.pairs_run = sh.pairs_run;
  S.chunks = sh.chunks;
  S.pairs_ms = sh.pairs_ms;
  for (auto &pass : passes) S.kernels_ms += pass->client.kernel_total_ms;
  S.total_ms = ms_since(t_all);
  copy_stats(stats, S);
  if (rc != NGSLD_OK) return rc;
  stores.keep = true;
  return NGSLD_OK;
} NGSLD_CATCH(c)

}  // extern "C"
