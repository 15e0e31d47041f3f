// tree.hip -- the LD tree on the device (ngsld_ld_tree, include/ngsld.h): the single-linkage tree of the sites, that is the maximum
// spanning forest of the graph ngsld_clusters unites, from the pair records where they are computed; no TSV, and never the
// graph's whole edge list: the forest, one chunk's candidates and a few words per site.  TREE.md has the rule, why the forest is a
// function of the edge set alone, and why the order of the atomics cannot change a selection.
//
//   pairs       RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//               (replayed pairs carry their replayed values)
//   candidates  one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items:
//               both sites are marked as nodes, the edge filter of cluster.hip on the printed value in integer micro-units
//               (ld_prune.h), and the chunk's edges (q, s1, s2) are appended behind the forest with one ballot and one atomic per
//               wavefront, as prune.hip's extraction does
//   reduce      forest + candidates -> the new forest, in Boruvka rounds of five launches over that list and the sites:
//                 best q     every edge between two components: atomicMax of q on both components' words
//                 best key   ... of that q: atomicMin of s1 << 32 | s2 on both components' words
//                 hook       an edge that is a component's (q, key) is a forest edge: it is written out, and the component
//                            that chose it hooks under the other one -- where both chose it, the larger under the smaller
//                 flatten    every site's label follows the hooks to its new root
//               until a round finds no edge between two components.  An edge's place in the list decides nothing.
//   host        the forest (at most n_sites - 1 edges) and the node marks come back once; the edges in rule order, one union-find
//               pass for left, right, size, first and last.  ngsld_ld_tree_cut is a host pass over the stored merges.
#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

// an edge of the forest or a candidate: 16 B
struct TreeEdge {
  long long q;  // the printed value in micro-units, |q| < 2^38
  uint32_t s1, s2;
};

// q as a word an unsigned atomicMax orders: q + 2^38 > 0, so 0 is "no edge yet"
constexpr long long kBias = 1ll << 38;

struct CandArgs {
  const ngsld_item *items;  // the items of this launch
  uint64_t n_items;
  uint64_t out_base;        // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const double *cum;
  const uint32_t *infc;
  const uint8_t *maf_ok;    // printed maf >= min_maf, per site
  double limit;             // dist <= limit (+inf: no limit)
  double min_weight;
  int field;                // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  uint8_t *node;            // [n_sites] one end of an emitted pair
  TreeEdge *edge;           // the list: the forest, then this chunk's candidates
  uint64_t cap;             // its entries
  unsigned long long *meta; // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] entries of the list,
                            // [2] edges written by the reduce, [3] ... that came from the old forest
};

__global__ __launch_bounds__(256) void candidates_kernel(CandArgs A) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = t >> 6;
  const uint32_t c = (uint32_t)(t & 63u);
  bool edge = false;
  uint32_t s1 = 0, s2 = 0;
  long long q = 0;
  if (i < A.n_items) {
    const ngsld_item it = A.items[i];
    if (c < it.count && ((it.mask >> c) & 1ull)) {
      s1 = it.s1;
      s2 = it.s2_begin + c;
      A.node[s1] = 1;
      A.node[s2] = 1;
      // (dist as the difference of the prefix sums: the call is refused unless the gaps are integers, where it is the printed value)
      if (A.infc[s1] == A.infc[s2] && A.cum[s2] - A.cum[s1] <= A.limit && A.maf_ok[s1] && A.maf_ok[s2]) {
        const double x = field_of(A.rec[record_of(it, c, A.out_base)], A.field);
        if (x - x == 0.0) {  // (not NaN or +-inf)
          int64_t m = 0;
          if (!ngsld::printed_micro(x, &m)) {
            atomicCAS(A.meta, 0ull, (((unsigned long long)s1 << 32) | s2) + 1ull);
          } else {
            q = (A.abs_value && m < 0) ? -m : m;
            edge = (double)q / 1e6 >= A.min_weight;  // the printed value read back (ld_prune.h), as doubles
          }
        }
      }
    }
  }
  const uint64_t bal = __ballot(edge);
  if (bal == 0) return;
  const int lane = (int)__lane_id(), leader = __ffsll((long long)bal) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(A.meta + 1, (unsigned long long)__popcll(bal));
  base = __shfl(base, leader);
  const uint64_t pos = base + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (edge && pos < A.cap) A.edge[pos] = TreeEdge{q, s1, s2};
}

struct ReduceArgs {
  const TreeEdge *edge;      // forest + candidates
  uint64_t n_edges;
  uint64_t n_old;            // the first n_old are the forest so far
  uint32_t n_sites;
  uint32_t *comp;            // [n_sites] every site's component: a site, its root
  uint32_t *hook;            // [n_sites] a root's new parent (itself: none)
  unsigned long long *best_q;    // [n_sites] by root: max of q + 2^38 over its outgoing edges, 0: none
  unsigned long long *best_key;  // [n_sites] by root: min of s1 << 32 | s2 over its outgoing edges of that q
  TreeEdge *out;             // the new forest
  uint64_t out_cap;
  unsigned long long *meta;  // as CandArgs
};

__device__ __forceinline__ uint32_t load_u32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long load_u64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void identity_kernel(uint32_t *comp, uint32_t *hook, uint32_t n) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  comp[v] = (uint32_t)v;
  hook[v] = (uint32_t)v;
}

// the largest q of every component's outgoing edges.  A word only grows, and an atomicMax that cannot raise it is left out: what
// the word holds after the launch is the maximum over the edges, whichever order they came in
__global__ __launch_bounds__(256) void best_q_kernel(ReduceArgs A) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n_edges) return;
  const TreeEdge ed = A.edge[e];
  const uint32_t a = A.comp[ed.s1], b = A.comp[ed.s2];
  if (a == b) return;
  const unsigned long long w = (unsigned long long)(ed.q + kBias);
  if (load_u64(A.best_q + a) < w) atomicMax(A.best_q + a, w);
  if (load_u64(A.best_q + b) < w) atomicMax(A.best_q + b, w);
}

// among a component's outgoing edges of its largest q, the smallest (s1, s2): the words of the first launch are final here
__global__ __launch_bounds__(256) void best_key_kernel(ReduceArgs A) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= A.n_edges) return;
  const TreeEdge ed = A.edge[e];
  const uint32_t a = A.comp[ed.s1], b = A.comp[ed.s2];
  if (a == b) return;
  const unsigned long long w = (unsigned long long)(ed.q + kBias), key = ((unsigned long long)ed.s1 << 32) | ed.s2;
  if (A.best_q[a] == w && load_u64(A.best_key + a) > key) atomicMin(A.best_key + a, key);
  if (A.best_q[b] == w && load_u64(A.best_key + b) > key) atomicMin(A.best_key + b, key);
}

// An edge that is the choice (q, key) of one of its components is an edge of the forest: it is written out once, by its own
// thread, and the component that chose it hooks under the other.  Where both chose it -- the only cycle a strict total order
// allows -- the larger root hooks under the smaller.  Every root has one choice, so every hook word has one writer.
__global__ __launch_bounds__(256) void hook_kernel(ReduceArgs A) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  TreeEdge ed{0, 0, 0};
  if (e < A.n_edges) {
    ed = A.edge[e];
    const uint32_t a = A.comp[ed.s1], b = A.comp[ed.s2];
    if (a != b) {
      const unsigned long long w = (unsigned long long)(ed.q + kBias), key = ((unsigned long long)ed.s1 << 32) | ed.s2;
      const bool by_a = A.best_q[a] == w && A.best_key[a] == key, by_b = A.best_q[b] == w && A.best_key[b] == key;
      keep = by_a || by_b;
      if (by_a && by_b) {
        if (a > b) A.hook[a] = b;
        else A.hook[b] = a;
      } else if (by_a) {
        A.hook[a] = b;
      } else if (by_b) {
        A.hook[b] = a;
      }
    }
  }
  const uint64_t bal = __ballot(keep);
  if (bal == 0) return;
  const int lane = (int)__lane_id(), leader = __ffsll((long long)bal) - 1;
  const int old = __popcll(__ballot(keep && e < A.n_old));
  unsigned long long base = 0;
  if (lane == leader) {
    base = atomicAdd(A.meta + 2, (unsigned long long)__popcll(bal));
    if (old) atomicAdd(A.meta + 3, (unsigned long long)old);
  }
  base = __shfl(base, leader);
  const uint64_t pos = base + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (keep && pos < A.out_cap) A.out[pos] = ed;
}

// comp[v] = the root the hooks lead to from v's old root.  A root that hooked is no root from here on, and every value its hook
// word ever holds is one of its ancestors: the walk's end is written back to it, so that the next site of the component walks less
__global__ __launch_bounds__(256) void flatten_kernel(ReduceArgs A) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= A.n_sites) return;
  const uint32_t c0 = A.comp[v];
  uint32_t r = c0, p = load_u32(A.hook + r);
  if (p == r) return;
  while (p != r) {
    r = p;
    p = load_u32(A.hook + r);
  }
  A.comp[v] = r;
  __hip_atomic_store(A.hook + c0, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rule 2: q descending, then s1, then s2 ascending
bool rule_before(const TreeEdge &x, const TreeEdge &y) {
  if (x.q != y.q) return x.q > y.q;
  if (x.s1 != y.s1) return x.s1 < y.s1;
  return x.s2 < y.s2;
}

// ngsld_ld_tree in four parts (record_pass.h AnalysisPass)
struct TreePass final : AnalysisPass {
  const ngsld_ld_tree_params *p;
  ngsld_ld_tree_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_ld_tree_stats S;
  SiteFilter F;
  DevBuf<uint8_t> d_node;
  DevBuf<TreeEdge> d_edge, d_out;
  DevBuf<uint32_t> d_comp, d_hook;
  DevBuf<unsigned long long> d_bq, d_bk, d_meta;
  CandArgs A{};
  uint64_t n_forest = 0;  // the forest's edges, at the head of d_edge

  TreePass(const ngsld_ld_tree_params *params, ngsld_ld_tree_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_ld_tree_params", stats, "ngsld_ld_tree_stats")) return rc;
    if (p->field < 4 || p->field > 7) return fail(c, NGSLD_ERR_INVALID, "tree field must be a TSV column 4..7");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "tree max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "tree min_maf is NaN");
    if (std::isnan(p->min_weight)) return fail(c, NGSLD_ERR_INVALID, "tree min_weight is NaN");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.tree.clear(); }

  // the list with room for `need` entries, its first `keep` kept
  int grow_list(ngsld_ctx *c, uint64_t need, uint64_t keep) {
    if (d_edge.n >= need) return NGSLD_OK;
    DevBuf<TreeEdge> bigger;
    HIP_TRY(c, bigger.resize(need));
    if (keep) HIP_TRY(c, hipMemcpyAsync(bigger.p, d_edge.p, keep * sizeof(TreeEdge), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    d_edge.release();
    d_edge.p = bigger.p;
    d_edge.n = bigger.n;
    bigger.p = nullptr;
    bigger.n = 0;
    return NGSLD_OK;
  }

  // forest + candidates, the first n_list entries of d_edge, to the new forest at its head
  int reduce(ngsld_ctx *c, uint64_t n_list) {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    ReduceArgs R{};
    R.edge = d_edge.p;
    R.n_edges = n_list;
    R.n_old = n_forest;
    R.n_sites = (uint32_t)n;
    R.comp = d_comp.p;
    R.hook = d_hook.p;
    R.best_q = d_bq.p;
    R.best_key = d_bk.p;
    R.out = d_out.p;
    R.out_cap = d_out.n;
    R.meta = d_meta.p;
    const dim3 by_edge(blocks_for(n_list)), by_site(blocks_for(n)), block(256);
    HIP_TRY(c, hipMemsetAsync(d_meta.p + 2, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(identity_kernel, by_site, block, 0, st, d_comp.p, d_hook.p, (uint32_t)n);
    HIP_TRY(c, hipGetLastError());
    unsigned long long kept[2] = {0, 0};
    uint64_t rounds = 0;
    while (true) {
      const unsigned long long had = kept[0];
      HIP_TRY(c, hipMemsetAsync(d_bq.p, 0, n * sizeof(unsigned long long), st));
      HIP_TRY(c, hipMemsetAsync(d_bk.p, 0xff, n * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(best_q_kernel, by_edge, block, 0, st, R);
      hipLaunchKernelGGL(best_key_kernel, by_edge, block, 0, st, R);
      hipLaunchKernelGGL(hook_kernel, by_edge, block, 0, st, R);
      hipLaunchKernelGGL(flatten_kernel, by_site, block, 0, st, R);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(kept, d_meta.p + 2, sizeof(kept), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      ++rounds;
      if (kept[0] == had) break;  // no edge between two components is left
      // (every round at least halves the components that still have an edge out: cannot happen)
      if (rounds > 40) return fail(c, NGSLD_ERR_DEVICE, "tree: the reduce does not end");
    }
    if (kept[0] >= n || kept[0] > d_out.n || kept[1] > n_forest) return fail(c, NGSLD_ERR_DEVICE, "tree: more forest edges than sites");  // (cannot happen)
    S.rounds += rounds;
    S.max_rounds = std::max<uint64_t>(S.max_rounds, rounds);
    S.displaced += n_forest - kept[1];
    n_forest = kept[0];
    if (n_forest) HIP_TRY(c, hipMemcpyAsync(d_edge.p, d_out.p, n_forest * sizeof(TreeEdge), hipMemcpyDeviceToDevice, st));
    return NGSLD_OK;
  }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;

    // ---- sites: the dist prefix sums (the limit and the merges' dist come from them), the maf filter on the printed maf ----
    F.prepare(c, &p->min_maf);
    if (!F.exact_gaps) return fail(c, NGSLD_ERR_UNSUPPORTED, "tree needs integer position gaps");
    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;
    if (n_pairs == 0) return NGSLD_OK;

    if (const int rc = F.upload(c)) return rc;
    HIP_TRY(c, d_node.resize(n));
    HIP_TRY(c, d_out.resize(n));
    HIP_TRY(c, d_comp.resize(n));
    HIP_TRY(c, d_hook.resize(n));
    HIP_TRY(c, d_bq.resize(n));
    HIP_TRY(c, d_bk.resize(n));
    HIP_TRY(c, d_meta.resize(4));
    HIP_TRY(c, hipMemsetAsync(d_node.p, 0, n, st));
    HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 4 * sizeof(unsigned long long), st));
    A.cum = F.d_cum.p;
    A.infc = F.d_infc.p;
    A.maf_ok = F.d_maf_ok.p;
    A.limit = p->max_kb_dist * 1000.0;
    A.min_weight = p->min_weight;
    A.field = p->field - 4;
    A.abs_value = p->abs_value != 0 ? 1 : 0;
    A.node = d_node.p;
    A.meta = d_meta.p;

    // NGSLD_TEST_TREE_PLANT = "R:X" (tests): record R of the plan gets the chosen field = X once its chunk's records are final, as
    // NGSLD_TEST_SCAN_PLANT_DP does (scan.hip): no input gives a finite value near 2^38 micro-units
    uint64_t plant_at = ~0ull;
    double plant_x = 0.0;
    if (const char *e = test_knob("TREE_PLANT")) {
      char *colon = nullptr;
      const uint64_t at = std::strtoull(e, &colon, 10);
      if (colon != e && *colon == ':') {
        plant_at = at;
        plant_x = std::strtod(colon + 1, nullptr);
      }
    }

    client.kernel_ms = &S.edges_ms;
    client.before = [this, c, st, plant_at, plant_x](const RecordChunk &ch) -> int {
      // room for every pair of this chunk to be an edge, behind the forest
      RC_TRY(grow_list(c, n_forest + ch.pairs, n_forest));
      const unsigned long long head = n_forest;
      HIP_TRY(c, hipMemcpyAsync(d_meta.p + 1, &head, sizeof(head), hipMemcpyHostToDevice, st));
      if (plant_at >= ch.out_base && plant_at - ch.out_base < ch.pairs) {
        ngsld_rec_std *r = const_cast<ngsld_rec_std *>(A.rec) + (plant_at - ch.out_base);
        double *x = A.field == 0 ? &r->r2_ExpG : A.field == 1 ? &r->D : A.field == 2 ? &r->Dp : &r->r2;
        HIP_TRY(c, hipMemcpyAsync(x, &plant_x, sizeof(double), hipMemcpyHostToDevice, st));
      }
      HIP_TRY(c, hipStreamSynchronize(st));  // (head and plant_x leave the stack here)
      A.edge = d_edge.p;
      A.cap = d_edge.n;
      A.out_base = ch.out_base;
      return NGSLD_OK;
    };
    client.launch = [this, st](const RecordChunk &, const ngsld_item *items, uint64_t n_items) {
      A.items = items;
      A.n_items = n_items;
      hipLaunchKernelGGL(candidates_kernel, dim3(blocks_for(n_items * 64)), dim3(256), 0, st, A);
    };
    client.after = [this, c, st](const RecordChunk &) -> int {
      unsigned long long meta[2] = {0, 0};
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (meta[0] != 0) return fail_value_range(c, "tree", meta[0]);
      if (meta[1] < n_forest || meta[1] > d_edge.n) return fail(c, NGSLD_ERR_DEVICE, "tree: more candidates than pairs");  // (cannot happen)
      S.edges += meta[1] - n_forest;
      if (meta[1] == n_forest) return NGSLD_OK;  // no candidate: the forest stays
      const auto t_red = std::chrono::steady_clock::now();
      const int rc = reduce(c, meta[1]);
      S.reduce_ms += ms_since(t_red);
      return rc;
    };
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    const auto t_fin = std::chrono::steady_clock::now();
    std::vector<TreeEdge> forest(n_forest);
    TreeResult &T = c->res.tree;
    T.node.assign(n, 0);
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      if (n_forest) HIP_TRY(c, hipMemcpyAsync(forest.data(), d_edge.p, n_forest * sizeof(TreeEdge), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(T.node.data(), d_node.p, n, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
    }

    // ---- the merges: the forest in rule order, one union-find pass (a root is the smallest site of its cluster) ----
    std::sort(forest.begin(), forest.end(), rule_before);
    std::vector<uint32_t> parent(n), size(n, 1), last(n);
    std::vector<int64_t> name(n);  // a root's cluster: -(site + 1), or the merge that made it
    for (uint64_t s = 0; s < n; ++s) {
      parent[s] = last[s] = (uint32_t)s;
      name[s] = -(int64_t)(s + 1);
      S.nodes += T.node[s];
    }
    const auto find = [&parent](uint32_t v) {
      while (parent[v] != v) {
        parent[v] = parent[parent[v]];
        v = parent[v];
      }
      return v;
    };
    const size_t M = forest.size();
    T.s1.resize(M); T.s2.resize(M); T.q.resize(M); T.dist.resize(M); T.left.resize(M); T.right.resize(M);
    T.size.resize(M); T.first.resize(M); T.last.resize(M);
    for (size_t k = 0; k < M; ++k) {
      const TreeEdge &e = forest[k];
      const uint32_t a = find(e.s1), b = find(e.s2);
      if (e.s1 >= n || e.s2 >= n || a == b) {
        T.clear();
        return fail(c, NGSLD_ERR_DEVICE, "tree: the forest has a cycle");  // (cannot happen)
      }
      const uint32_t lo = std::min(a, b), hi = std::max(a, b);
      T.s1[k] = e.s1;
      T.s2[k] = e.s2;
      T.q[k] = e.q;
      T.dist[k] = (uint64_t)(F.cum[e.s2] - F.cum[e.s1]);
      T.left[k] = name[a];
      T.right[k] = name[b];
      parent[hi] = lo;
      size[lo] += size[hi];
      last[lo] = std::max(last[lo], last[hi]);
      name[lo] = (int64_t)(k + 1);
      T.size[k] = size[lo];
      T.first[k] = lo;
      T.last[k] = last[lo];
    }
    T.min_weight = p->min_weight;
    T.filled = true;
    S.merges = M;
    S.clusters = S.nodes - M;
    S.finish_ms = ms_since(t_fin);
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

extern "C" {

int ngsld_ld_tree(ngsld_ctx *c, const ngsld_ld_tree_params *p, ngsld_ld_tree_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  TreePass pass(p, stats);
  return run_single(c, pass, record_chunk(test_knob("TREE_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_ld_tree_merges(ngsld_ctx *c, uint64_t cap, uint32_t *s1, uint32_t *s2, int64_t *q_micro, uint64_t *dist, int64_t *left,
                         int64_t *right, uint32_t *size, uint32_t *first, uint32_t *last, uint64_t *n) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const TreeResult &T = c->res.tree;
  if (!T.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_ld_tree result (it goes with the next ngsld_plan or ngsld_set_*)");
  const uint64_t rows = std::min<uint64_t>(cap, T.q.size());
  for (uint64_t k = 0; k < rows; ++k) {
    if (s1) s1[k] = T.s1[k];
    if (s2) s2[k] = T.s2[k];
    if (q_micro) q_micro[k] = T.q[k];
    if (dist) dist[k] = T.dist[k];
    if (left) left[k] = T.left[k];
    if (right) right[k] = T.right[k];
    if (size) size[k] = T.size[k];
    if (first) first[k] = T.first[k];
    if (last) last[k] = T.last[k];
  }
  if (n) *n = T.q.size();
  return NGSLD_OK;
}

int ngsld_ld_tree_cut(ngsld_ctx *c, double t, uint32_t *cluster, uint64_t *n_clusters) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const TreeResult &T = c->res.tree;
  if (!T.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_ld_tree result (it goes with the next ngsld_plan or ngsld_set_*)");
  if (std::isnan(t) || t < T.min_weight)
    return fail(c, NGSLD_ERR_INVALID, "a cut of the tree must be at or above the min_weight it was built with (" + std::to_string(T.min_weight) + ")");
  const size_t n = T.node.size();
  std::vector<uint32_t> parent(n);
  for (size_t s = 0; s < n; ++s) parent[s] = (uint32_t)s;
  const auto find = [&parent](uint32_t v) {
    while (parent[v] != v) {
      parent[v] = parent[parent[v]];
      v = parent[v];
    }
    return v;
  };
  // the merges at or above t are a prefix: q only falls along the list
  for (size_t k = 0; k < T.q.size() && (double)T.q[k] / 1e6 >= t; ++k) {
    const uint32_t a = find(T.s1[k]), b = find(T.s2[k]);
    parent[std::max(a, b)] = std::min(a, b);
  }
  // a root is the smallest site of its cluster, so the roots come in id order
  std::vector<uint32_t> id(n, 0);
  uint32_t clusters = 0;
  for (size_t s = 0; s < n; ++s) {
    if (!T.node[s]) continue;
    const uint32_t r = find((uint32_t)s);
    id[s] = r == s ? ++clusters : id[r];
  }
  if (cluster && n) std::memcpy(cluster, id.data(), n * sizeof(uint32_t));
  if (n_clusters) *n_clusters = clusters;
  return NGSLD_OK;
} NGSLD_CATCH(c)

}  // extern "C"
