// results.h -- what the on-device analyses leave in the context until a getter copies it out: one struct per analysis with the test
// its getters make (valid) and a clear of its own; Results holds the ten and the one rule of what a new plan makes stale.
#pragma once  // (host code; engine.h includes it behind DevBuf)

// rank of TSV column `field` (4..7) among the chosen fields (1 r2_ExpG, 2 D, 4 D', 8 r2), -1 when it was not chosen
inline int field_rank(uint32_t fields, int field) {
  if (field < 4 || field > 7 || !((fields >> (field - 4)) & 1u)) return -1;
  return __builtin_popcount(fields & ((1u << (field - 4)) - 1u));
}

// ngsld_decay (decay.hip): per bin with rows its lower break and rows, then [bin][field] a mean per chosen field in TSV column order
struct DecayResult {
  uint32_t fields = 0;
  std::vector<double> dist, mean;
  std::vector<uint64_t> count;
  bool valid() const { return fields != 0; }  void clear() { *this = DecayResult(); }
};

// ngsld_site_ld (site_ld.hip): rows per site, then per chosen field [rank][site] sum and maximum in micro-units, linked rows, mean
struct SiteLdResult {
  uint32_t fields = 0;
  std::vector<uint64_t> n, linked;
  std::vector<int64_t> sum, max;
  std::vector<double> mean;
  bool valid() const { return fields != 0; }  void clear() { *this = SiteLdResult(); }
};

// ngsld_clusters (cluster.hip): every site's cluster id (0: not a node), then per cluster in id order its table row
struct ClustersResult {
  bool filled = false;  // (a result may hold no cluster at all)
  std::vector<uint32_t> id, size, first, last;
  std::vector<uint64_t> span, edges;
  std::vector<int64_t> sum;
  std::vector<double> mean, density;
  bool valid() const { return filled; }  void clear() { *this = ClustersResult(); }
};

// ngsld_grid (grid.hip): the chromosomes in file order, then per cell with rows -- by chromosome, b1, b2 -- its chromosome, bins
// and rows, and per chosen field [rank][cell] the sum and the maximum in micro-units, the linked rows and the mean
struct GridResult {
  uint32_t fields = 0;
  std::vector<std::string> chr_name;
  std::vector<uint32_t> chr;
  std::vector<uint64_t> b1, b2, n, linked;
  std::vector<int64_t> sum, max;
  std::vector<double> mean;
  bool valid() const { return fields != 0; }  void clear() { *this = GridResult(); }
};

// ngsld_scan (scan.hip): per site its window and the rows of the three classes, and per chosen field [rank][class LL, RR, LR][site]
// the sums in micro-units, then [rank][site] zns and omega
struct ScanResult {
  uint32_t fields = 0;
  std::vector<uint32_t> first, last;
  std::vector<uint64_t> n;  // [class][site]
  std::vector<int64_t> sum;
  std::vector<double> zns, omega;
  bool valid() const { return fields != 0; }  void clear() { *this = ScanResult(); }
};

// ngsld_partners (partners.hip): per site its partner rows, then [site][rank] the partner (0xFFFFFFFF: none) and its value in micro-units
struct PartnersResult {
  uint32_t k = 0, field = 0;
  std::vector<uint64_t> rows;
  std::vector<uint32_t> partner;
  std::vector<int64_t> value;
  bool valid() const { return k != 0; }  void clear() { *this = PartnersResult(); }
};

// ngsld_blocks (blocks.hip): per chosen field a members x members matrix of the records' doubles, a presence byte per cell, the matrix sites
struct BlocksResult {
  uint32_t fields = 0;
  uint64_t members = 0;
  DevBuf<double> d_val;            // [field rank][members][members], written only where present
  DevBuf<uint8_t> d_present;       // [members][members]
  DevBuf<uint32_t> d_col;          // [sites] member index of each matrix site, in matrix order
  std::vector<uint64_t> site;      // [sites] site index of each matrix site
  std::vector<std::string> label;  // [sites] its label up to the first TAB
  DevBuf<char> d_label;            // ... back to back, for the text rows
  DevBuf<uint64_t> d_label_off;    // [sites + 1]
  bool valid() const { return fields != 0; }
  void clear() {  // (the device memory goes back)
    fields = 0; members = 0;
    site.clear(); label.clear();
    d_val.release(); d_present.release(); d_col.release(); d_label.release(); d_label_off.release();
  }
};

// ngsld_decay_map (decay_map.hip): the chromosomes in file order, then per group with a non-empty bin -- by chromosome, window --
// its chromosome, win_start and the offset of its first bin (bin_off has one entry more: the end), then every group's non-empty
// bins back to back as DecayResult holds them
struct DecayMapResult {
  uint32_t fields = 0;
  std::vector<std::string> chr_name;
  std::vector<uint32_t> chr;
  std::vector<uint64_t> win_start, bin_off, count;
  std::vector<double> dist, mean;
  bool valid() const { return fields != 0; }  void clear() { *this = DecayMapResult(); }
};

// ngsld_cross_ld (cross.hip): the chromosomes in file order, then per cell with rows -- by the consecutive bin of the first site,
// then of the second -- the chromosome and bin of both sites and its rows, and per chosen field [rank][cell] what GridResult holds
struct CrossResult {
  uint32_t fields = 0;
  std::vector<std::string> chr_name;
  std::vector<uint32_t> chr1, chr2;
  std::vector<uint64_t> b1, b2, n, linked;
  std::vector<int64_t> sum, max;
  std::vector<double> mean;
  bool valid() const { return fields != 0; }  void clear() { *this = CrossResult(); }
};

// ngsld_ld_tree (tree.hip): the merges in rule order, the floor they were built at and the node marks a cut needs
struct TreeResult {
  bool filled = false;  // (a result may hold no merge at all)
  double min_weight = 0;
  std::vector<uint8_t> node;
  std::vector<uint32_t> s1, s2, size, first, last;
  std::vector<int64_t> q, left, right;
  std::vector<uint64_t> dist;
  bool valid() const { return filled; }  void clear() { *this = TreeResult(); }
};

// The lifetime rule, stated here alone.  An analysis clears its own store when it begins and touches no other.  ngsld_plan and every
// ngsld_set_* call invalidate_for_new_plan: eight stores hold values per site, region, cell or group of the plan that made them, which a new
// matrix, setting or plan makes stale.  The decay bins are indexed by distance, not by site: they stay until the next ngsld_decay.
struct Results {
  DecayResult decay;  // (by distance: a new plan leaves it)
  BlocksResult blocks; SiteLdResult site_ld; ClustersResult clusters; GridResult grid; ScanResult scan; PartnersResult partners;
  DecayMapResult decay_map; CrossResult cross; TreeResult tree;
  void invalidate_for_new_plan() { blocks.clear(); site_ld.clear(); clusters.clear(); grid.clear(); scan.clear(); partners.clear(); decay_map.clear(); cross.clear(); tree.clear(); }
};
