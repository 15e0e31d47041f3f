// prune.hip -- LD pruning on the device (ngsld_prune, include/ngsld.h): the set of sites prune_graph.pl keeps, from the pair
// records where they are computed -- no TSV, and the graph leaves the device only as a small remainder.  PRUNE.md has the rule,
// the deviations and why the parallel rounds end in the sequential rule's sets.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into
//            records (replayed pairs carry their replayed values)
//   edges    one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: node
//            marks, the printed-value filter (ld_prune.h), the surviving (s1, s2, label) compacted with one ballot and one
//            atomic per wavefront
//   graph    both directions of every edge radix-sorted by their first end (hipCUB): CSR offsets, neighbours, int64 weights
//   rounds   mark (strict local maximum of (weight desc, rank asc) among the live neighbours) + remove (atomic int64 subtract
//            on the neighbours), a wavefront per node; plain launches
//   host     once a round removes few nodes (a chain takes a round per node), the live remainder goes to the host's exact
//            sequential rule (prune_host.cpp).  keep_heavy and negative labels take that rule for the whole graph.
#include <hipcub/hipcub.hpp>

#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"
#include "../../include/ngsld_host.h"

namespace {

// a round that removes fewer nodes than this hands the rest to the host
constexpr unsigned long long kHostFinishBelow = 64;

struct EdgeArgs {
  const ngsld_item *items;
  uint64_t n_items;
  uint64_t out_base;  // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  int field;          // 0 r2_ExpG, 1 D, 2 D', 3 r2
  const double *cum;
  const uint32_t *infc;
  double max_dist;    // bp; +inf = no limit
  double min_weight, scale;
  char type;
  const uint8_t *in_subset;  // null = every site
  uint8_t *node;
  uint32_t *ea, *eb;
  int64_t *el;
  uint64_t cap;
  unsigned long long *meta;  // [0] edges, [1] max |label|, [2] a label < 0, [3] (s1 << 32 | s2) + 1 of a label beyond 2^62
};

__global__ __launch_bounds__(256) void edge_kernel(EdgeArgs A) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = t >> 6;
  const uint32_t c = (uint32_t)(t & 63u);
  bool edge = false;
  uint32_t s1 = 0, s2 = 0;
  int64_t lab = 0;
  if (i < A.n_items) {
    const ngsld_item it = A.items[i];
    if (c < it.count && ((it.mask >> c) & 1ull)) {
      s1 = it.s1;
      s2 = it.s2_begin + c;
      const uint64_t k = record_of(it, c, A.out_base);
      const bool in1 = A.in_subset == nullptr || A.in_subset[s1], in2 = A.in_subset == nullptr || A.in_subset[s2];
      if (in1) A.node[s1] = 1;
      if (in2) A.node[s2] = 1;
      // dist as the TSV prints it (ld_text.hip format_row); not finite across a chromosome change: never an edge
      if (in1 && in2 && A.infc[s1] == A.infc[s2] && !(A.cum[s2] - A.cum[s1] > A.max_dist)) {
        const ngsld_rec_std r = A.rec[k];
        const int q = prune_label(field_of(r, A.field), A.min_weight, A.type, A.scale, &lab);
        if (q == kPruneEdge)
          edge = true;
        else if (q == kPruneTooLarge)
          atomicCAS(A.meta + 3, 0ull, (((unsigned long long)s1 << 32) | s2) + 1ull);
      }
    }
  }
  const uint64_t bal = __ballot(edge);
  if (bal == 0) return;
  const int lane = (int)__lane_id(), leader = __ffsll((long long)bal) - 1;
  const unsigned long long mag = wave_max(edge ? (unsigned long long)(lab < 0 ? -lab : lab) : 0ull);
  const bool any_neg = __ballot(edge && lab < 0) != 0;
  unsigned long long base = 0;
  if (lane == leader) {
    base = atomicAdd(A.meta, (unsigned long long)__popcll(bal));
    atomicMax(A.meta + 1, mag);
    if (any_neg) atomicOr(A.meta + 2, 1ull);
  }
  base = __shfl(base, leader);
  const uint64_t pos = base + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (edge && pos < A.cap) {
    A.ea[pos] = s1;
    A.eb[pos] = s2;
    A.el[pos] = lab;
  }
}

// both directions of every edge: key = the first end, value = the edge
__global__ void dir_fill_kernel(const uint32_t *ea, const uint32_t *eb, uint64_t E, uint32_t *key, uint32_t *val) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= E) return;
  key[t] = ea[t];
  val[t] = (uint32_t)t;
  key[E + t] = eb[t];
  val[E + t] = (uint32_t)t;
}

// off[v] = first sorted entry with key >= v, v = 0 .. n
__global__ void offsets_kernel(const uint32_t *key, uint64_t n2, uint32_t n, uint64_t *off) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n) return;
  uint64_t lo = 0, hi = n2;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (key[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  off[v] = lo;
}

__global__ void adjacency_kernel(const uint32_t *key, const uint32_t *val, const uint32_t *ea, const uint32_t *eb,
                                 const int64_t *el, uint64_t n2, uint32_t *nbr, int64_t *lab) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n2) return;
  const uint32_t e = val[j];
  nbr[j] = ea[e] == key[j] ? eb[e] : ea[e];
  lab[j] = el[e];
}

// a wavefront per node: windows give a node thousands of neighbours
__global__ __launch_bounds__(256) void weight_kernel(const uint64_t *off, const int64_t *lab, uint32_t n, int64_t *w) {
  const uint64_t v = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (v >= n) return;
  const int lane = (int)__lane_id();
  long long s = 0;
  for (uint64_t j = off[v] + lane; j < off[v + 1]; j += 64) s += lab[j];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) w[v] = s;
}

// v goes in this round iff it is live, its weight is > 0, and its key (weight desc, rank asc) beats every live neighbour's
__global__ __launch_bounds__(256) void mark_kernel(const uint64_t *off, const uint32_t *nbr, const int64_t *w, const uint32_t *rank,
                                                   const uint8_t *alive, uint32_t n, uint8_t *mark, unsigned long long *counts) {
  const uint64_t v = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (v >= n || !alive[v]) return;
  const int64_t wv = w[v];
  if (wv <= 0) return;
  const uint32_t rv = rank[v];
  const int lane = (int)__lane_id();
  bool lose = false;
  for (uint64_t j = off[v] + lane; j < off[v + 1] && !lose; j += 64) {
    const uint32_t u = nbr[j];
    if (!alive[u]) continue;
    const int64_t wu = w[u];
    lose = wu > wv || (wu == wv && rank[u] < rv);
  }
  lose = __any(lose);
  if (lane == 0) {
    atomicAdd(counts, 1ull);
    if (!lose) {
      mark[v] = 1;
      atomicAdd(counts + 1, 1ull);
    }
  }
}

// the marked nodes go: no two of them are neighbours, so every weight changed here belongs to a node that stays
__global__ __launch_bounds__(256) void remove_kernel(const uint64_t *off, const uint32_t *nbr, const int64_t *lab, int64_t *w, uint32_t n,
                                                     uint8_t *alive, uint8_t *mark) {
  const uint64_t v = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (v >= n || !mark[v]) return;
  const int lane = (int)__lane_id();
  for (uint64_t j = off[v] + lane; j < off[v + 1]; j += 64)
    atomicAdd(reinterpret_cast<unsigned long long *>(w + nbr[j]), (unsigned long long)(-lab[j]));
  if (lane == 0) {
    alive[v] = 0;
    mark[v] = 0;
  }
}

// the edges whose two ends are still live
__global__ __launch_bounds__(256) void residual_kernel(const uint32_t *ea, const uint32_t *eb, const int64_t *el, uint64_t E,
                                                       const uint8_t *alive, uint32_t *ra, uint32_t *rb, int64_t *rl,
                                                       unsigned long long *count) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool keep = t < E && alive[ea[t]] && alive[eb[t]];
  const uint64_t bal = __ballot(keep);
  if (bal == 0) return;
  const int lane = (int)__lane_id(), leader = __ffsll((long long)bal) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(bal));
  base = __shfl(base, leader);
  if (keep) {
    const uint64_t pos = base + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
    ra[pos] = ea[t];
    rb[pos] = eb[t];
    rl[pos] = el[t];
  }
}

// grow an edge list to `cap` entries, keeping the first `keep`
template <typename T>
hipError_t grow(DevBuf<T> &b, size_t cap, size_t keep, hipStream_t st) {
  if (b.n >= cap) return hipSuccess;
  T *p = nullptr;
  hipError_t e = hipMalloc((void **)&p, cap * sizeof(T));
  if (e != hipSuccess) return e;
  if (keep) e = hipMemcpyAsync(p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return e;
  }
  b.release();
  b.p = p;
  b.n = cap;
  return hipSuccess;
}

bool lower_less(const std::string &x, const std::string &y) {  // Perl's lc(...) cmp lc(...): ASCII letters only, then bytes
  const size_t n = std::min(x.size(), y.size());
  for (size_t i = 0; i < n; ++i) {
    unsigned char a = (unsigned char)x[i], b = (unsigned char)y[i];
    if (a >= 'A' && a <= 'Z') a = (unsigned char)(a + 32);
    if (b >= 'A' && b <= 'Z') b = (unsigned char)(b + 32);
    if (a != b) return a < b;
  }
  return x.size() < y.size();
}

// ngsld_selftest_printed: the quantiser of this file's edge_kernel and decay.hip's bin_kernel (ld_prune.h), value by value
__global__ void printed_kernel(const double *x, uint64_t n, double min_weight, char type, double scale, int64_t *micro,
                               int32_t *micro_ok, int64_t *label, int32_t *label_rc) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double v = x[t];
  int64_t q = 0, lab = 0;
  const bool ok = ngsld::printed_micro(v, &q);  // (false for NaN / inf too; the bin kernel drops those before it quantises)
  micro[t] = q;
  micro_ok[t] = ok ? 1 : 0;
  label_rc[t] = ngsld::prune_label(v, min_weight, type, scale, &lab);
  label[t] = lab;
}

// ngsld_prune in four parts (record_pass.h AnalysisPass)
struct PrunePass final : AnalysisPass {
  const ngsld_prune_params *p;
  const char *const *labels;
  uint8_t *site_state;
  ngsld_prune_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_prune_stats S;
  char type = 0;
  std::vector<std::string> lab;
  std::vector<uint32_t> order, rank;
  std::vector<uint8_t> in_subset;
  SiteFilter F;
  DevBuf<uint32_t> d_rank, d_ea, d_eb;
  DevBuf<uint8_t> d_subset, d_node, d_mark;
  DevBuf<unsigned long long> d_meta;
  DevBuf<int64_t> d_el;
  uint64_t n_pairs = 0;
  EdgeArgs A{};
  unsigned long long meta[4] = {0, 0, 0, 0};

  PrunePass(const ngsld_prune_params *params, const char *const *site_labels, uint8_t *state, ngsld_prune_stats *out)
      : p(params), labels(site_labels), site_state(state), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_prune_params", stats, "ngsld_prune_stats")) return rc;
    if (site_state == nullptr) return fail(c, NGSLD_ERR_INVALID, "site_state is NULL");
    if (p->field < 4 || p->field > 7) return fail(c, NGSLD_ERR_INVALID, "prune field must be 4, 5, 6 or 7");
    type = (char)p->weight_type;
    if (type != 'a' && type != 'e' && type != 'n') return fail(c, NGSLD_ERR_INVALID, "prune weight type must be 'a', 'e' or 'n'");
    if (p->precision < 0 || p->precision > 15) return fail(c, NGSLD_ERR_INVALID, "prune precision must be in [0, 15]");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "prune max_kb_dist must be >= 0");
    if (std::isnan(p->min_weight)) return fail(c, NGSLD_ERR_INVALID, "prune min_weight is NaN");
    if (p->n_subset > 0 && p->subset == nullptr) return fail(c, NGSLD_ERR_INVALID, "prune subset is NULL");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *) override {}  // (the result is the caller's site_state: nothing is kept in the context)

  bool fit_longest_row() const override { return false; }  // (a row longer than the chunk is refused)

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    hipStream_t st = c->stream;

    // ---- sites: labels, ranks (lc(label), label, index), the subset, the dist prefix sums ----
    lab.resize(n);
    for (uint64_t s = 0; s < n; ++s) {
      if (labels != nullptr && labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "a label is NULL");
      lab[s] = labels ? labels[s] : "(null)";
    }
    order.resize(n);
    for (uint64_t s = 0; s < n; ++s) order[s] = (uint32_t)s;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      if (lower_less(lab[x], lab[y])) return true;
      if (lower_less(lab[y], lab[x])) return false;
      return lab[x] != lab[y] ? lab[x] < lab[y] : x < y;
    });
    rank.resize(n);
    for (uint64_t r = 0; r < n; ++r) rank[order[r]] = (uint32_t)r;
    if (p->subset != nullptr) {
      std::unordered_map<std::string, int> want;
      for (uint64_t i = 0; i < p->n_subset; ++i)
        if (p->subset[i] != nullptr) want.emplace(p->subset[i], 1);
      in_subset.assign(n, 0);
      for (uint64_t s = 0; s < n; ++s) in_subset[s] = want.count(lab[s]) ? 1 : 0;
    }
    const double max_dist = p->max_kb_dist * 1000.0;
    F.prepare(c, nullptr);
    if (const int rc = F.check_limit(c, "prune", max_dist)) return rc;
    if (const int rc = F.upload(c)) return rc;
    HIP_TRY(c, d_rank.resize(n));
    HIP_TRY(c, d_node.resize(n));
    HIP_TRY(c, d_mark.resize(n));
    HIP_TRY(c, d_meta.resize(4));
    HIP_TRY(c, hipMemcpy(d_rank.p, rank.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!in_subset.empty()) {
      HIP_TRY(c, d_subset.resize(n));
      HIP_TRY(c, hipMemcpy(d_subset.p, in_subset.data(), n, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipMemsetAsync(d_node.p, 0, n, st));
    HIP_TRY(c, hipMemsetAsync(d_mark.p, 0, n, st));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 4 * sizeof(unsigned long long), st));

    // ---- pairs and edges, chunk of rows by chunk ----
    n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    A.field = p->field - 4;
    A.cum = F.d_cum.p;
    A.infc = F.d_infc.p;
    A.max_dist = max_dist;
    A.min_weight = p->min_weight;
    A.scale = prune_scale(p->precision);
    A.type = type;
    A.in_subset = in_subset.empty() ? nullptr : d_subset.p;
    A.node = d_node.p;
    A.meta = d_meta.p;
    client.kernel_ms = &S.edges_ms;
    client.before = [this, c, st](const RecordChunk &ch) -> int {
      // room for every pair of this chunk to be an edge
      const uint64_t need = meta[0] + ch.pairs;
      if (d_el.n < need) {
        const size_t cap = (size_t)std::max<uint64_t>(need, std::min<uint64_t>(n_pairs, 2 * (uint64_t)d_el.n));
        HIP_TRY(c, grow(d_ea, cap, meta[0], st));
        HIP_TRY(c, grow(d_eb, cap, meta[0], st));
        HIP_TRY(c, grow(d_el, cap, meta[0], st));
      }
      A.ea = d_ea.p;
      A.eb = d_eb.p;
      A.el = d_el.p;
      A.cap = d_el.n;
      A.out_base = ch.out_base;
      return NGSLD_OK;
    };
    client.launch = [this, st](const RecordChunk &, const ngsld_item *items, uint64_t n_items) {
      A.items = items;
      A.n_items = n_items;
      hipLaunchKernelGGL(edge_kernel, dim3(blocks_for(n_items * 64)), dim3(256), 0, st, A);
    };
    client.after = [this, c, st](const RecordChunk &) -> int {
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (meta[3] != 0) {
        const unsigned long long k = meta[3] - 1;
        return fail(c, NGSLD_ERR_UNSUPPORTED, "the edge label of the pair " + lab[k >> 32] + " - " + lab[k & 0xffffffffull] +
                                                  " reaches 2^62 (lower the precision)");
      }
      return NGSLD_OK;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    S.pairs_ms = shared.pairs_ms;
    const uint64_t E = meta[0];
    S.edges = E;

    // ---- nodes; two node sites with one label are refused (the script would merge them) ----
    std::vector<uint8_t> node(n);
    HIP_TRY(c, hipMemcpy(node.data(), d_node.p, n, hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < n;) {
      uint64_t r1 = r + 1;
      while (r1 < n && lab[order[r1]] == lab[order[r]]) ++r1;
      uint64_t nodes_here = 0;
      for (uint64_t q = r; q < r1; ++q) nodes_here += node[order[q]];
      if (nodes_here > 1) return fail(c, NGSLD_ERR_INVALID, "two sites share the label " + lab[order[r]]);
      r = r1;
    }
    for (uint64_t s = 0; s < n; ++s) S.nodes += node[s];
    if (E >= (1ull << 30)) return fail(c, NGSLD_ERR_UNSUPPORTED, "more than 2^30 - 1 edges");  // (both directions: an int count for hipCUB)

    // ---- graph: CSR of both directions, int64 weights ----
    auto t_graph = std::chrono::steady_clock::now();
    const uint64_t n2 = 2 * E;
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_nbr;
    DevBuf<int64_t> d_lab, d_w;
    HIP_TRY(c, d_off.resize(n + 1));
    HIP_TRY(c, d_w.resize(n));
    std::vector<uint64_t> off(n + 1, 0);
    if (E > 0) {
      DevBuf<uint32_t> k_in, k_out, v_in, v_out;
      HIP_TRY(c, k_in.resize(n2));
      HIP_TRY(c, k_out.resize(n2));
      HIP_TRY(c, v_in.resize(n2));
      HIP_TRY(c, v_out.resize(n2));
      hipLaunchKernelGGL(dir_fill_kernel, dim3(blocks_for(E)), dim3(256), 0, st, d_ea.p, d_eb.p, E, k_in.p, v_in.p);
      HIP_TRY(c, hipGetLastError());
      int bits = 1;
      while (bits < 32 && (n >> bits) != 0) ++bits;
      size_t tmp_bytes = 0;
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p, (int)n2, 0, bits, st));
      DevBuf<char> tmp;
      HIP_TRY(c, tmp.resize(tmp_bytes ? tmp_bytes : 1));
      HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p, (int)n2, 0, bits, st));
      hipLaunchKernelGGL(offsets_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, st, k_out.p, n2, (uint32_t)n, d_off.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, d_nbr.resize(n2));
      HIP_TRY(c, d_lab.resize(n2));
      hipLaunchKernelGGL(adjacency_kernel, dim3(blocks_for(n2)), dim3(256), 0, st, k_out.p, v_out.p, d_ea.p, d_eb.p, d_el.p, n2,
                         d_nbr.p, d_lab.p);
      HIP_TRY(c, hipGetLastError());
      hipLaunchKernelGGL(weight_kernel, dim3(blocks_for(n * 64)), dim3(256), 0, st, d_off.p, d_lab.p, (uint32_t)n, d_w.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(off.data(), d_off.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
    }
    {  // every partial sum of a node's weight exact: max |label| times its degree below 2^63
      uint64_t max_deg = 0;
      for (uint64_t v = 0; v < n; ++v) max_deg = std::max<uint64_t>(max_deg, off[v + 1] - off[v]);
      if (max_deg > 0 && meta[1] > (unsigned long long)INT64_MAX / max_deg)
        return fail(c, NGSLD_ERR_UNSUPPORTED, "edge labels too large to sum exactly (lower the precision)");
    }
    S.graph_ms = ms_since(t_graph);

    // ---- rounds (labels >= 0 and the heaviest removed: PRUNE.md) ----
    auto t_rounds = std::chrono::steady_clock::now();
    DevBuf<uint8_t> &d_alive = d_node;  // live = a node not removed yet
    DevBuf<unsigned long long> d_cnt;
    HIP_TRY(c, d_cnt.resize(2));
    long long host_after = -1;  // tests: hand the rest to the host after this many rounds
    if (const char *e = test_knob("PRUNE_HOST_AFTER")) host_after = std::atoll(e);
    const bool device_rounds = E > 0 && !p->keep_heavy && meta[2] == 0;
    while (device_rounds && (host_after < 0 || (long long)S.rounds < host_after)) {
      unsigned long long cnt[2] = {0, 0};
      HIP_TRY(c, hipMemsetAsync(d_cnt.p, 0, sizeof(cnt), st));
      hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(n * 64)), dim3(256), 0, st, d_off.p, d_nbr.p, d_w.p, d_rank.p, d_alive.p,
                         (uint32_t)n, d_mark.p, d_cnt.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (cnt[0] == 0) break;  // no live node of weight > 0: done
      hipLaunchKernelGGL(remove_kernel, dim3(blocks_for(n * 64)), dim3(256), 0, st, d_off.p, d_nbr.p, d_lab.p, d_w.p, (uint32_t)n,
                         d_alive.p, d_mark.p);
      HIP_TRY(c, hipGetLastError());
      ++S.rounds;
      if (cnt[1] < kHostFinishBelow) break;
    }
    std::vector<uint8_t> alive(n);
    HIP_TRY(c, hipMemcpyAsync(alive.data(), d_alive.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    S.rounds_ms = ms_since(t_rounds);

    // ---- host finish: the live remainder through the exact sequential rule ----
    auto t_host = std::chrono::steady_clock::now();
    std::vector<uint8_t> state(n, 0);
    for (uint64_t s = 0; s < n; ++s) state[s] = node[s] ? (alive[s] ? 1 : 2) : 0;
    if (E > 0) {
      DevBuf<uint32_t> ra, rb;
      DevBuf<int64_t> rl;
      HIP_TRY(c, ra.resize(E));
      HIP_TRY(c, rb.resize(E));
      HIP_TRY(c, rl.resize(E));
      HIP_TRY(c, hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st));
      hipLaunchKernelGGL(residual_kernel, dim3(blocks_for(E)), dim3(256), 0, st, d_ea.p, d_eb.p, d_el.p, E, d_alive.p, ra.p, rb.p,
                         rl.p, d_cnt.p);
      HIP_TRY(c, hipGetLastError());
      unsigned long long R = 0;
      HIP_TRY(c, hipMemcpyAsync(&R, d_cnt.p, sizeof(R), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (R > 0) {
        std::vector<uint32_t> ha(R), hb(R);
        std::vector<int64_t> hl(R);
        HIP_TRY(c, hipMemcpy(ha.data(), ra.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(hb.data(), rb.p, R * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(hl.data(), rl.p, R * sizeof(int64_t), hipMemcpyDeviceToHost));
        // the remainder's nodes, numbered in site order
        std::vector<uint32_t> local(n, 0xffffffffu), site;
        for (uint64_t e = 0; e < R; ++e)
          for (uint32_t s : {ha[e], hb[e]})
            if (local[s] == 0xffffffffu) {
              local[s] = 0;
              site.push_back(s);
            }
        std::sort(site.begin(), site.end());
        std::vector<uint64_t> lrank(site.size());
        for (size_t i = 0; i < site.size(); ++i) {
          local[site[i]] = (uint32_t)i;
          lrank[i] = rank[site[i]];
        }
        for (uint64_t e = 0; e < R; ++e) {
          ha[e] = local[ha[e]];
          hb[e] = local[hb[e]];
        }
        std::vector<uint8_t> excl(site.size());
        uint64_t steps = 0;
        const int rc = ngsld_host_prune_graph(site.size(), lrank.data(), R, ha.data(), hb.data(), hl.data(), p->keep_heavy ? 1 : 0,
                                              excl.data(), &steps);
        if (rc == NGSLD_ERR_UNSUPPORTED) return fail(c, rc, "edge labels too large to sum exactly (lower the precision)");
        if (rc != NGSLD_OK) return fail(c, rc, "host pruning failed");
        for (size_t i = 0; i < site.size(); ++i)
          if (excl[i]) state[site[i]] = 2;
        S.host_steps = steps;
        S.host_nodes = site.size();
        S.host_edges = R;
      }
    }
    S.host_ms = ms_since(t_host);
    for (uint64_t s = 0; s < n; ++s) {
      site_state[s] = state[s];
      S.kept += state[s] == 1;
      S.excluded += state[s] == 2;
    }
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_prune_pass(const ngsld_prune_params *p, const char *const *labels, uint8_t *site_state,
                                              ngsld_prune_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new PrunePass(p, labels, site_state, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_prune(ngsld_ctx *c, const ngsld_prune_params *p, const char *const *labels, uint8_t *site_state,
                ngsld_prune_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  PrunePass pass(p, labels, site_state, stats);
  return run_single(c, pass, record_chunk(test_knob("PRUNE_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_selftest_printed(ngsld_ctx *c, uint64_t n, const double *x, int32_t precision, int32_t weight_type, double min_weight,
                           int64_t *micro, int32_t *micro_ok, int64_t *label, int32_t *label_rc) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (n == 0 || n > (1ull << 26) || x == nullptr || micro == nullptr || micro_ok == nullptr || label == nullptr ||
      label_rc == nullptr)
    return fail(c, NGSLD_ERR_INVALID, "ngsld_selftest_printed: 1 <= n <= 2^26 values and every pointer set");
  if (precision < 0 || precision > 15) return fail(c, NGSLD_ERR_INVALID, "prune precision must be in [0, 15]");
  if (weight_type != 'a' && weight_type != 'e' && weight_type != 'n')
    return fail(c, NGSLD_ERR_INVALID, "prune weight type must be 'a', 'e' or 'n'");
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  DevBuf<double> d_x;
  DevBuf<int64_t> d_micro, d_label;
  DevBuf<int32_t> d_ok, d_rc;
  HIP_TRY(c, d_x.resize(n));
  HIP_TRY(c, d_micro.resize(n));
  HIP_TRY(c, d_label.resize(n));
  HIP_TRY(c, d_ok.resize(n));
  HIP_TRY(c, d_rc.resize(n));
  HIP_TRY(c, hipMemcpy(d_x.p, x, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(printed_kernel, dim3(blocks_for(n)), dim3(256), 0, c->stream, d_x.p, n, min_weight, (char)weight_type,
                     ngsld::prune_scale(precision), d_micro.p, d_ok.p, d_label.p, d_rc.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(micro, d_micro.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(micro_ok, d_ok.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(label, d_label.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(label_rc, d_rc.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return NGSLD_OK;
} NGSLD_CATCH(c)

}  // extern "C"
