// cluster.hip -- LD clusters on the device (ngsld_clusters, include/ngsld.h): the connected components of the graph that
// ngsld_prune prunes, from the pair records where they are computed; no TSV and no edge list, one word per site.  CLUSTERS.md
// has the rule, the deviations and why the result does not depend on the order of the atomics.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records
//            (replayed pairs carry their replayed values)
//   union    one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: both sites
//            are marked as nodes, the edge filter on the printed value in integer micro-units (ld_prune.h), and every edge unites
//            its two sites in parent[n_sites] -- a lock-free union-find that lives on the device across the chunks.  A root is
//            only ever hooked under a smaller site, with a compare-and-swap on the root's own word: parent[v] <= v and only
//            decreases, a hook that loses starts again from the word's new value, finds halve their paths with atomicMin.
//            The 64 lanes of an item share s1: its root is found once, the lanes' roots are reduced to their minimum across
//            the wavefront, and only the lanes whose root is not that minimum hook -- each on its own root's word.  The edges
//            of an item and the sum of their values are a ballot and a shuffle reduction, one 64-bit add each to s1's words.
//   flatten  one launch after the last chunk: parent[v] = the root of v = the smallest site of v's component
//   host     parent, the node marks and the per-site edge counts and sums come back once; ids in increasing order of the
//            roots, sizes, last sites, edges and sums folded by root, one rounding for the mean and the density (ld_mean.h)
#include "engine.h"
#include "ld_prune.h"
#include "record_pass.h"

namespace {

struct ClusterArgs {
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
  int track_max;            // a cluster may hold 2^25 edges or more: max |q| goes to meta[1]
  uint32_t n_sites;
  uint32_t *parent;         // [n_sites] the union-find forest: parent[v] <= v
  uint8_t *node;            // [n_sites] one end of an emitted pair
  unsigned long long *acc;  // [2][n_sites], by s1: edges, then the int64 sum of their q (two's complement)
  unsigned long long *meta; // [0] (s1 << 32 | s2) + 1 of a value beyond 2^38 micro-units, [1] max |q|
};

__device__ __forceinline__ uint32_t parent_of(const uint32_t *parent, uint32_t v) {
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v, halving the path on the way: every value a word ever held is an ancestor of its site, so a word read late or
// early still leads to the root, and atomicMin keeps every word decreasing whichever halving lands last
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t v) {
  uint32_t p = parent_of(parent, v);
  while (p != v) {
    const uint32_t g = parent_of(parent, p);
    if (g != p) atomicMin(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}

// unites the trees of a and b, both roots when read: the larger is hooked under the smaller by a compare-and-swap on its own
// word, which succeeds only while it still is a root; a hook that loses goes on from what the word holds now
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
  while (a != b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = find_root(parent, old);
    b = find_root(parent, lo);
  }
}

// the min of v over the 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return ~(uint32_t)wave_max((unsigned long long)(uint32_t)~v); }

__global__ __launch_bounds__(256) void init_kernel(uint32_t *parent, uint32_t n) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) parent[v] = (uint32_t)v;
}

__global__ __launch_bounds__(256) void union_kernel(ClusterArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, step = (uint64_t)gridDim.x * 4;
  unsigned long long qmax = 0;
  for (uint64_t i = first; i < A.n_items; i += step) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    const bool pair = c < it.count && ((it.mask >> c) & 1ull);
    if (__ballot(pair) == 0) continue;
    if (pair) A.node[s2] = 1;
    if (lane == 0) A.node[s1] = 1;
    bool edge = false;
    long long q = 0;
    // (dist as the difference of the prefix sums: the call is refused unless the gaps are integers, where it is the printed value)
    if (pair && A.infc[s1] == A.infc[s2] && A.cum[s2] - A.cum[s1] <= A.limit && A.maf_ok[s1] && A.maf_ok[s2]) {
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
    const uint64_t edges = __ballot(edge);
    if (edges == 0) continue;
    if (!edge) q = 0;
    // the row end: this item's edges and their sum, once
    const long long sum = wave_sum(q);
    if (lane == 0) {
      atomicAdd(A.acc + s1, (unsigned long long)__popcll(edges));
      atomicAdd(A.acc + A.n_sites + s1, (unsigned long long)sum);
    }
    if (A.track_max) {
      const unsigned long long a = (unsigned long long)(q < 0 ? -q : q);
      qmax = a > qmax ? a : qmax;
    }
    // the union: s1's root once, the smallest root of the item, and a hook for every root that is not it
    const int leader = __ffsll((long long)edges) - 1;
    uint32_t r1 = lane == leader ? find_root(A.parent, s1) : 0u;
    r1 = __shfl(r1, leader);
    const uint32_t r2 = edge ? find_root(A.parent, s2) : r1;
    const uint32_t low = wave_min(r2 < r1 ? r2 : r1);
    if (edge && r2 != low) unite(A.parent, r2, low);  // (lanes without an edge carry r1: the leader hooks it, once)
    if (lane == leader && r1 != low) unite(A.parent, r1, low);
  }
  if (A.track_max) {
    qmax = wave_max(qmax);
    if (lane == 0 && qmax) atomicMax(A.meta + 1, qmax);
  }
}

// parent[v] = v's root.  In place: a word another thread has flattened already is still an ancestor
__global__ __launch_bounds__(256) void flatten_kernel(uint32_t *parent, uint32_t n) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  uint32_t r = (uint32_t)v, p = parent_of(parent, r);
  while (p != r) {
    r = p;
    p = parent_of(parent, r);
  }
  if (r != (uint32_t)v) atomicMin(parent + v, r);
}

// ngsld_clusters in four parts (record_pass.h AnalysisPass)
struct ClustersPass final : AnalysisPass {
  const ngsld_clusters_params *p;
  ngsld_clusters_stats *stats;
  const std::chrono::steady_clock::time_point t_all = std::chrono::steady_clock::now();
  ngsld_clusters_stats S;
  SiteFilter F;
  std::vector<uint32_t> parent;
  std::vector<uint8_t> node;
  std::vector<unsigned long long> acc;
  bool track_max = false;
  DevBuf<uint32_t> d_parent;
  DevBuf<uint8_t> d_node;
  DevBuf<unsigned long long> d_acc, d_meta;
  ClusterArgs A{};

  ClustersPass(const ngsld_clusters_params *params, ngsld_clusters_stats *out) : p(params), stats(out) {}

  int validate(ngsld_ctx *c) override {
    if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
    if (const int rc = check_struct_sizes(c, p, "ngsld_clusters_params", stats, "ngsld_clusters_stats")) return rc;
    if (p->field < 4 || p->field > 7) return fail(c, NGSLD_ERR_INVALID, "clusters field must be a TSV column 4..7");
    if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "clusters max_kb_dist must be >= 0");
    if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "clusters min_maf is NaN");
    if (std::isnan(p->min_weight)) return fail(c, NGSLD_ERR_INVALID, "clusters min_weight is NaN");
    return NGSLD_OK;
  }

  void clear(ngsld_ctx *c) override { c->res.clusters.clear(); }

  int prepare(ngsld_ctx *c, uint64_t) override {
    const uint64_t n = c->n_sites;
    if (const int rc = begin_pass(c, S)) return rc;
    clear(c);
    hipStream_t st = c->stream;

    // ---- sites: the dist prefix sums (the limit and the spans come from them), the maf filter on the printed maf ----
    F.prepare(c, &p->min_maf);
    if (!F.exact_gaps) return fail(c, NGSLD_ERR_UNSUPPORTED, "clusters need integer position gaps");
    const uint64_t n_pairs = c->h_row_off[n];
    S.pairs = n_pairs;

    parent.resize(n);
    node.assign(n, 0);
    acc.assign(2 * n, 0);
    for (uint64_t s = 0; s < n; ++s) parent[s] = (uint32_t)s;
    // every partial sum of a cluster is exact while max |q| * its edges < 2^63: certain below 2^25 edges (|q| < 2^38)
    track_max = track_sums(n_pairs >= (1ull << 25));
    if (n_pairs > 0) {
      if (const int rc = F.upload(c)) return rc;
      HIP_TRY(c, d_parent.resize(n));
      HIP_TRY(c, d_node.resize(n));
      HIP_TRY(c, d_acc.resize(2 * n));
      HIP_TRY(c, d_meta.resize(2));
      HIP_TRY(c, hipMemsetAsync(d_node.p, 0, n, st));
      HIP_TRY(c, hipMemsetAsync(d_acc.p, 0, 2 * n * sizeof(unsigned long long), st));
      HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 2 * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(init_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_parent.p, (uint32_t)n);
      HIP_TRY(c, hipGetLastError());
      A.cum = F.d_cum.p;
      A.infc = F.d_infc.p;
      A.maf_ok = F.d_maf_ok.p;
      A.limit = p->max_kb_dist * 1000.0;
      A.min_weight = p->min_weight;
      A.field = p->field - 4;
      A.abs_value = p->abs_value != 0 ? 1 : 0;
      A.track_max = track_max ? 1 : 0;
      A.n_sites = (uint32_t)n;
      A.parent = d_parent.p;
      A.node = d_node.p;
      A.acc = d_acc.p;
      A.meta = d_meta.p;
      const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 8;
      client.kernel_ms = &S.union_ms;
      client.launch = [this, st, max_blocks](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
        A.out_base = ch.out_base;
        A.items = items;
        A.n_items = n_items;
        const unsigned blocks = std::min<unsigned>(blocks_for(n_items * 64), max_blocks);
        hipLaunchKernelGGL(union_kernel, dim3(blocks), dim3(256), 0, st, A);
        ++S.union_launches;
      };
      client.after = [this, c, st](const RecordChunk &) -> int {
        unsigned long long bad = 0;
        HIP_TRY(c, hipMemcpyAsync(&bad, d_meta.p, sizeof(bad), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return bad != 0 ? fail_value_range(c, "clusters", bad) : NGSLD_OK;
      };
    }
    return NGSLD_OK;
  }

  void bind(ngsld_rec_std *records) override { A.rec = records; }

  int finish(ngsld_ctx *c, const RecordPass::Shared &shared) override {
    const uint64_t n = c->n_sites;
    hipStream_t st = c->stream;
    unsigned long long meta[2] = {0, 0};
    if (client.launch) {
      S.pairs_ms = shared.pairs_ms;
      S.chunks = shared.chunks;
      const auto t_fin = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_parent.p, (uint32_t)n);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(parent.data(), d_parent.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(node.data(), d_node.p, n, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(acc.data(), d_acc.p, 2 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      S.finish_ms = ms_since(t_fin);
    }

    // ---- the clusters: a root is the smallest site of its component, so the roots come in id order ----
    const auto t_host = std::chrono::steady_clock::now();
    ClustersResult &K = c->res.clusters;
    K.id.assign(n, 0);
    for (uint64_t s = 0; s < n; ++s) {
      if (!node[s]) continue;
      ++S.nodes;
      const uint32_t root = parent[s];
      if (root == s) {
        K.size.push_back(0);
        K.first.push_back((uint32_t)s);
        K.last.push_back((uint32_t)s);
        K.edges.push_back(0);
        K.sum.push_back(0);
        K.id[s] = (uint32_t)K.size.size();
      } else {
        if (root > s || K.id[root] == 0) return fail(c, NGSLD_ERR_DEVICE, "clusters: the forest is not flat");  // (cannot happen)
        K.id[s] = K.id[root];
      }
      const size_t k = K.id[s] - 1;
      ++K.size[k];
      K.last[k] = (uint32_t)s;
      K.edges[k] += acc[s];
      K.sum[k] = (int64_t)((uint64_t)K.sum[k] + acc[n + s]);  // (two's complement, as on the device: checked below before it is read)
    }
    const size_t nk = K.size.size();
    K.span.resize(nk);
    K.mean.resize(nk);
    K.density.resize(nk);
    {  // the cluster of the most edges bounds every other's sums: the refusal names it
      const uint64_t most = nk ? *std::max_element(K.edges.begin(), K.edges.end()) : 0;
      if (track_max && track_sums(most >= (1ull << 25)) && sum_may_wrap(meta[1], most)) {
        K.clear();
        return fail(c, NGSLD_ERR_UNSUPPORTED, "a cluster of " + std::to_string(most) + " edges with values too large to sum exactly");
      }
    }
    for (size_t k = 0; k < nk; ++k) {
      const uint64_t size = K.size[k], edges = K.edges[k];
      S.edges += edges;
      if (size >= 2) ++S.clusters_multi;
      S.largest = std::max<uint64_t>(S.largest, size);
      K.span[k] = (uint64_t)(F.cum[K.last[k]] - F.cum[K.first[k]]);
      const int64_t sum = K.sum[k];
      if (edges == 0) {
        K.mean[k] = std::numeric_limits<double>::quiet_NaN();
      } else {
        const double m = div_nearest((unsigned __int128)(sum < 0 ? -(__int128)sum : (__int128)sum), (unsigned __int128)edges * 1000000u);
        K.mean[k] = sum < 0 ? -m : m;
      }
      K.density[k] = size < 2 ? std::numeric_limits<double>::quiet_NaN()
                              : div_nearest((unsigned __int128)edges, (unsigned __int128)size * (size - 1) / 2);
    }
    S.clusters = nk;
    K.filled = true;
    S.finish_ms += ms_since(t_host);
    S.total_ms = ms_since(t_all);
    copy_stats(stats, S);
    return NGSLD_OK;
  }
};

}  // namespace

namespace ngsld {
namespace eng {
std::unique_ptr<AnalysisPass> make_clusters_pass(const ngsld_clusters_params *p, ngsld_clusters_stats *stats) {
  return std::unique_ptr<AnalysisPass>(new ClustersPass(p, stats));
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

int ngsld_clusters(ngsld_ctx *c, const ngsld_clusters_params *p, ngsld_clusters_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  ClustersPass pass(p, stats);
  return run_single(c, pass, record_chunk(test_knob("CLUSTER_CHUNK_PAIRS")));
} NGSLD_CATCH(c)

int ngsld_clusters_sites(ngsld_ctx *c, uint32_t *cluster) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.clusters.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_clusters result (it goes with the next ngsld_plan or ngsld_set_*)");
  if (cluster && !c->res.clusters.id.empty()) std::memcpy(cluster, c->res.clusters.id.data(), c->res.clusters.id.size() * sizeof(uint32_t));
  return NGSLD_OK;
}

int ngsld_clusters_table(ngsld_ctx *c, uint64_t min_size, uint64_t cap, uint32_t *id, uint32_t *size, uint32_t *first, uint32_t *last,
                         uint64_t *span, uint64_t *edges, int64_t *sum_micro, double *mean, double *density, uint64_t *n) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const ClustersResult &K = c->res.clusters;
  if (!K.valid()) return fail(c, NGSLD_ERR_INVALID, "no ngsld_clusters result (it goes with the next ngsld_plan or ngsld_set_*)");
  uint64_t rows = 0;
  for (size_t k = 0; k < K.size.size(); ++k) {
    if (K.size[k] < min_size) continue;
    if (rows < cap) {
      if (id) id[rows] = (uint32_t)(k + 1);
      if (size) size[rows] = K.size[k];
      if (first) first[rows] = K.first[k];
      if (last) last[rows] = K.last[k];
      if (span) span[rows] = K.span[k];
      if (edges) edges[rows] = K.edges[k];
      if (sum_micro) sum_micro[rows] = K.sum[k];
      if (mean) mean[rows] = K.mean[k];
      if (density) density[rows] = K.density[k];
    }
    ++rows;
  }
  if (n) *n = rows;
  return NGSLD_OK;
}

}  // extern "C"
