// prune_host.cpp -- the exact sequential LD pruner on the host (include/ngsld_host.h: ngsld_host_prune_graph,
// ngsld_host_prune_label).  ngsld_prune (prune.hip) finishes every graph here: the remainder the device rounds leave, or the
// whole graph where the rounds do not apply (keep_heavy, negative labels).  PRUNE.md has the rule and why the device's rounds
// end in the same sets.
#include <cstdint>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "../../include/ngsld_host.h"
#include "ld_prune.h"

extern "C" {

int ngsld_host_prune_label(double x, int prec, char type, int64_t *label) {
  if (label == nullptr || prec < 0 || prec > 15 || (type != 'a' && type != 'e' && type != 'n')) return NGSLD_ERR_INVALID;
  // (no weight floor here: -inf lets every finite value through, whatever its sign)
  const int r = ngsld::prune_label(x, -__builtin_inf(), type, ngsld::prune_scale(prec), label);
  if (r == ngsld::kPruneSkip) return NGSLD_ERR_INVALID;
  if (r == ngsld::kPruneTooLarge) return NGSLD_ERR_UNSUPPORTED;
  return NGSLD_OK;
}

int ngsld_host_prune_graph(uint64_t n_nodes, const uint64_t *rank, uint64_t n_edges, const uint32_t *a, const uint32_t *b,
                           const int64_t *label, int keep_heavy, uint8_t *excluded, uint64_t *n_steps) try {
  if (excluded == nullptr || (n_edges > 0 && (a == nullptr || b == nullptr || label == nullptr))) return NGSLD_ERR_INVALID;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (a[e] >= n_nodes || b[e] >= n_nodes || a[e] == b[e]) return NGSLD_ERR_INVALID;
  // adjacency, both directions
  std::vector<uint64_t> off(n_nodes + 1, 0);
  for (uint64_t e = 0; e < n_edges; ++e) {
    ++off[a[e] + 1];
    ++off[b[e] + 1];
  }
  for (uint64_t v = 0; v < n_nodes; ++v) off[v + 1] += off[v];
  std::vector<uint32_t> nbr(2 * n_edges);
  std::vector<int64_t> lab(2 * n_edges);
  {
    std::vector<uint64_t> fill(off.begin(), off.end() - 1);
    for (uint64_t e = 0; e < n_edges; ++e) {
      nbr[fill[a[e]]] = b[e];
      lab[fill[a[e]]++] = label[e];
      nbr[fill[b[e]]] = a[e];
      lab[fill[b[e]]++] = label[e];
    }
  }
  // weights; every partial sum stays exact when the sum of |labels| of each node does
  std::vector<int64_t> w(n_nodes, 0);
  for (uint64_t v = 0; v < n_nodes; ++v) {
    int64_t abs_sum = 0;
    for (uint64_t j = off[v]; j < off[v + 1]; ++j) {
      const int64_t l = lab[j];
      if (l == INT64_MIN || __builtin_add_overflow(abs_sum, l < 0 ? -l : l, &abs_sum)) return NGSLD_ERR_UNSUPPORTED;
      w[v] += l;
    }
  }
  auto rk = [&](uint64_t v) { return rank ? rank[v] : v; };
  // heaviest first, then the lower rank; (weight desc, rank asc) is a strict order as long as the ranks are distinct
  typedef std::tuple<int64_t, uint64_t, uint32_t> Key;  // (-weight, rank, node)
  std::set<Key> heap;
  std::vector<uint8_t> alive(n_nodes, 1);
  for (uint64_t v = 0; v < n_nodes; ++v) {
    excluded[v] = 0;
    if (off[v + 1] > off[v]) heap.insert(Key(-w[v], rk(v), (uint32_t)v));
  }
  auto remove = [&](uint32_t v) {
    alive[v] = 0;
    excluded[v] = 1;
    heap.erase(Key(-w[v], rk(v), v));
    for (uint64_t j = off[v]; j < off[v + 1]; ++j) {
      const uint32_t u = nbr[j];
      if (!alive[u]) continue;
      heap.erase(Key(-w[u], rk(u), u));
      w[u] -= lab[j];
      heap.insert(Key(-w[u], rk(u), u));
    }
  };
  uint64_t steps = 0;
  while (!heap.empty()) {
    const uint32_t top = std::get<2>(*heap.begin());
    if (w[top] <= 0) break;
    if (keep_heavy) {
      for (uint64_t j = off[top]; j < off[top + 1]; ++j)
        if (alive[nbr[j]]) remove(nbr[j]);
    } else {
      remove(top);
    }
    ++steps;
  }
  if (n_steps) *n_steps = steps;
  return NGSLD_OK;
} catch (...) {
  return NGSLD_ERR_NOMEM;
}

}  // extern "C"
