// record_pass.hip -- the host frame of the record passes (record_pass.h): the site filter's arrays, the chunk loop over
// ngsld_run_device + ngsld_finish_device, the refusal of a value out of range, a label's CHR:pos.  Host code only.
#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace ngsld {
namespace eng {

void SiteFilter::prepare(const ngsld_ctx *c, const double *min_maf) {
  exact_gaps = dist_prefix(c, cum, infc);
  if (min_maf == nullptr) return;
  maf_ok.resize(c->n_sites);
  for (uint64_t s = 0; s < c->n_sites; ++s) {
    const double m = c->h_maf[s];
    maf_ok[s] = (m - m == 0.0 && ngsld::prune_printed(m) >= *min_maf) ? 1 : 0;  // (a NaN maf never passes, as in R)
  }
}

int SiteFilter::check_limit(ngsld_ctx *c, const char *pass, double limit) const {
  if (!exact_gaps && std::isfinite(limit)) return fail(c, NGSLD_ERR_UNSUPPORTED, std::string(pass) + " max_kb_dist needs integer position gaps");
  return NGSLD_OK;
}

int SiteFilter::upload(ngsld_ctx *c) {
  const uint64_t n = c->n_sites;
  HIP_TRY(c, d_cum.resize(n));
  HIP_TRY(c, d_infc.resize(n));
  HIP_TRY(c, hipMemcpy(d_cum.p, cum.data(), n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d_infc.p, infc.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (maf_ok.empty()) return NGSLD_OK;
  HIP_TRY(c, d_maf_ok.resize(n));
  HIP_TRY(c, hipMemcpy(d_maf_ok.p, maf_ok.data(), n, hipMemcpyHostToDevice));
  return NGSLD_OK;
}

int RecordPass::open(ngsld_ctx *ctx, uint64_t chunk, const uint8_t *only_rows, bool fit_longest_row, bool with_ext) {
  c = ctx;
  chunk_pairs = chunk;
  rows = only_rows;
  uint64_t cap = chunk;
  if (fit_longest_row) {
    uint64_t pairs = 0, longest = 0;
    for (uint64_t s = 0; s < c->n_sites; ++s)
      if (rows == nullptr || rows[s]) {
        pairs += c->h_row_off[s + 1] - c->h_row_off[s];
        longest = std::max<uint64_t>(longest, c->h_row_off[s + 1] - c->h_row_off[s]);
      }
    cap = std::max<uint64_t>(std::min<uint64_t>(pairs, chunk), longest);
  }
  HIP_TRY(c, d_rec.resize(cap));
  if (with_ext) HIP_TRY(c, d_ext.resize(cap));
  return NGSLD_OK;
}

int RecordPass::run(double *pairs_ms, double *kernel_ms, uint64_t *chunks, const Step &before, const Launch &launch, const Step &after) {
  Client one;
  one.before = before;
  one.launch = launch;
  one.after = after;
  one.kernel_ms = kernel_ms;
  Client *const list[1] = {&one};
  Shared sh;
  const int rc = run(list, 1, &sh);
  if (pairs_ms) *pairs_ms += sh.pairs_ms;
  if (chunks) *chunks += sh.chunks;
  return rc;
}

int RecordPass::run(Client *const *clients, size_t n_clients, Shared *shared) {
  const uint64_t n = c->n_sites;
  bool any = false;
  for (size_t k = 0; k < n_clients; ++k) {
    if (!clients[k]->launch) continue;
    any = true;
    if (clients[k]->ev.a == nullptr) HIP_TRY(c, clients[k]->ev.create());
  }
  if (!any) return NGSLD_OK;
  Shared sh;
  struct Report {  // (a failure reports the pairs that ran before it too)
    Shared *out, *sh;
    ~Report() {
      if (out == nullptr) return;
      out->pairs_ms += sh->pairs_ms;
      out->chunks += sh->chunks;
      out->pairs_run += sh->pairs_run;
    }
  } report{shared, &sh};
  // The records are read as printed (ld_prune.h): the launches flag, and the replay settles, the pairs whose sixth decimal
  // or sign rounding noise could change, as for text output -- a D one ulp off an odd / 128 tie would quantise to the other
  // neighbour than the reference's "%f"
  struct FlagText {
    ngsld_ctx *c;
    ~FlagText() { c->dev_run_flag_text = false; }
  } flag_text{c};
  c->dev_run_flag_text = true;
  uint64_t end = 0;  // where the rows that are run, from r0 on, end (a chunk ends at a row that is not run)
  for (uint64_t r0 = 0; r0 < n;) {
    if (rows != nullptr && !rows[r0]) {
      ++r0;
      continue;
    }
    if (end <= r0)
      for (end = r0 + 1; end < n && (rows == nullptr || rows[end]);) ++end;
    const uint64_t r1 = rows_within(c->h_row_off, r0, end, chunk_pairs);
    const RecordChunk ch{r0, r1, c->h_row_off[r1] - c->h_row_off[r0], c->h_row_off[r0]};
    if (ch.pairs > d_rec.n) return fail(c, NGSLD_ERR_UNSUPPORTED, "a row of " + std::to_string(ch.pairs) + " pairs does not fit the record buffer");
    if (ch.pairs > 0) {
      const auto t0 = std::chrono::steady_clock::now();
      sh.pairs_run += ch.pairs;
      int rc = ngsld_run_device(c, r0, r1, d_rec.p, d_ext.p, nullptr);  // (the ctx's stream: records final, replay done)
      if (rc == NGSLD_OK) rc = ngsld_finish_device(c);
      if (rc != NGSLD_OK) return rc;
      sh.pairs_ms += ms_since(t0);
      ++sh.chunks;
      const uint64_t i0 = c->h_item_off[r0], i1 = c->h_item_off[r1];
      const uint64_t max_items = record_slice_items();
      for (size_t k = 0; k < n_clients; ++k) {
        Client &cl = *clients[k];
        if (!cl.launch) continue;
        if (cl.before) {
          rc = cl.before(ch);
          if (rc != NGSLD_OK) return rc;
        }
        HIP_TRY(c, hipEventRecord(cl.ev.a, c->stream));
        for (uint64_t off = i0; off < i1; off += max_items) {
          cl.launch(ch, c->d_items.p + off, std::min<uint64_t>(max_items, i1 - off));
          HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(cl.ev.b, c->stream));
        HIP_TRY(c, hipEventSynchronize(cl.ev.b));
        double span = 0;
        HIP_TRY(c, cl.ev.add_elapsed(&span));
        cl.kernel_total_ms += span;
        if (cl.kernel_ms) *cl.kernel_ms += span;
        if (cl.after) {
          rc = cl.after(ch);
          if (rc != NGSLD_OK) return rc;
        }
      }
    }
    r0 = r1;
  }
  return NGSLD_OK;
}

int run_passes(ngsld_ctx *c, AnalysisPass *const *passes, size_t n, uint64_t chunk_pairs, RecordPass::Shared *shared) {
  RecordPass::Shared sh;
  bool any = false, fit = true;
  std::vector<RecordPass::Client *> clients;
  for (size_t k = 0; k < n; ++k) {
    if (const int rc = passes[k]->prepare(c, chunk_pairs)) return rc;
    any = any || passes[k]->client.launch;
    fit = fit && passes[k]->fit_longest_row();
    clients.push_back(&passes[k]->client);
  }
  if (any) {
    RecordPass R;
    const uint64_t n_pairs = c->h_row_off[c->n_sites];
    if (const int rc = R.open(c, fit ? chunk_pairs : std::max<uint64_t>(1, std::min<uint64_t>(n_pairs, chunk_pairs)), nullptr, fit)) return rc;
    for (size_t k = 0; k < n; ++k) passes[k]->bind(R.records());
    const int rc = R.run(clients.data(), n, &sh);
    if (shared) *shared = sh;
    if (rc != NGSLD_OK) return rc;
  }  // (the records go before the finishes: pruning builds its graph in their room)
  for (size_t k = 0; k < n; ++k)
    if (const int rc = passes[k]->finish(c, sh)) return rc;
  return NGSLD_OK;
}

int run_single(ngsld_ctx *c, AnalysisPass &pass, uint64_t chunk_pairs) {
  if (const int rc = pass.validate(c)) return rc;
  AnalysisPass *const list[1] = {&pass};
  return run_passes(c, list, 1, chunk_pairs, nullptr);
}

int fail_value_range(ngsld_ctx *c, const char *pass, unsigned long long meta0) {
  const unsigned long long k = meta0 - 1;
  return fail(c, NGSLD_ERR_UNSUPPORTED, std::string("a ") + pass + " value of the pair of sites " + std::to_string(k >> 32) + " - " +
                                            std::to_string(k & 0xffffffffull) + " reaches 2^38 micro-units (|x| >= 274877.906944)");
}

LabelPos label_pos(const char *label) {
  const char *t = std::strchr(label, '\t');
  LabelPos L{t ? std::string(label, t) : std::string(label), 0};
  L.colon = L.key.find(':');
  return L;
}

bool LabelPos::position(uint64_t *pos) const {
  const char *num = colon == std::string::npos ? "" : key.c_str() + colon + 1;
  const size_t len = std::strlen(num);
  bool digits = len > 0 && len <= 19;
  for (const char *q = num; *q; ++q) digits = digits && *q >= '0' && *q <= '9';
  if (digits) *pos = std::strtoull(num, nullptr, 10);
  return digits;
}
}  // namespace eng
}  // namespace ngsld
