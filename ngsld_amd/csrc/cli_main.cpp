// cli_main.cpp -- the `ngsLD` command line of the MI355X-native engine: same flags, defaults, validation
// messages, stderr chatter and TSV as the reference binary (parse_args.cpp:6-184, ngsLD.cpp:27-223), with
// the thread-pool section (ngsLD.cpp:153-198) replaced by the C-ABI in include/ngsld.h.
//
// Differences a user can see (all listed in DESIGN.md):
//   * rows are written in (site1, site2) order (the reference's order is arbitrary for --n_threads > 1);
//   * --n_threads sets the number of host threads that format the TSV; --device N (new) picks the GPU, --max_gpu_mem GB (new)
//     caps the device memory: a windowed run on binary input that does not fit is streamed slab by slab;
//   * --devices 0-7 (or 0,2,5; new) runs the job on several GPUs of the node from this one process (ngsld_run_multi):
//     the rows are cut into one part per device, the output is the single-device output;
//   * --prune_out FILE (new) and the other --prune_* flags: the sites scripts/prune_graph.pl would keep, pruned on the device
//     (ngsld_prune, PRUNE.md); without --out no TSV is written.  Exact flag names only: they are taken out of argv before
//     getopt runs, so the reference's flags keep every abbreviation and message they have;
//   * --decay_out FILE / --decay_fit FILE (new) and the other --decay_* flags: the distance bins and the decay fit of
//     scripts/fit_LDdecay.R, binned on the device (ngsld_decay, DECAY.md); taken out of argv the same way, no TSV without --out;
//   * --blocks_out PREFIX (new) and the other --blocks_* flags: the r2 / D' matrices of one region that scripts/LD_blocks.sh
//     hands to LDheatmap, built on the device (ngsld_blocks, BLOCKS.md) and written as PREFIX.<stat>.tsv; taken out of argv
//     the same way, no TSV without --out;
//   * --site_out FILE (new) and the other --site_* flags: the pair table collapsed per site -- rows, LD score, mean, maximum
//     and linked partners of every site -- summed on the device (ngsld_site_ld, SITES.md); taken out of argv the same way, no
//     TSV without --out;
//   * --cluster_out FILE / --cluster_table FILE (new) and the other --cluster_* flags: the LD clusters -- the connected
//     components of the graph --prune_out prunes -- united on the device without an edge list (ngsld_clusters, CLUSTERS.md);
//     taken out of argv the same way, no TSV without --out;
//   * --grid_out FILE --grid_bin_size B (new) and the other --grid_* flags: the LD heat map along each chromosome -- rows, sum,
//     mean, maximum and linked rows of the site pairs between every two windows of B bp -- binned on the device (ngsld_grid,
//     GRID.md); taken out of argv the same way, no TSV without --out;
//   * --linked_out FILE / --linked_outH FILE (new) and the other --linked_* flags: the rows of the table at or above an LD floor,
//     each as the table prints it and in the table's order, compacted on the device (ngsld_linked_pairs, LINKED.md); taken out
//     of argv the same way, no TSV without --out; a name ending in .gz is written gzip-compressed;
//   * --scan_out FILE --scan_half_window H (new) and the other --scan_* flags: a window of H bp to either side of every site --
//     the rows inside its two flanks and across the site, Kelly's ZnS and Kim and Nielsen's omega -- summed on the device
//     (ngsld_scan, SCAN.md); taken out of argv the same way, no TSV without --out;
//   * --partners_out FILE --partners_k K (new) and the other --partners_* flags: for every site, or the sites --partners_sites
//     names, the K sites that tag it best -- its rows at or above an LD floor ranked by value -- kept on the device
//     (ngsld_partners, PARTNERS.md); taken out of argv the same way, no TSV without --out;
//   * --dmap_out FILE / --dmap_fit FILE (new) and the other --dmap_* flags: --decay_out's bins and --decay_fit's fit per
//     chromosome, or with --dmap_window W per window of W bp, binned on the device (ngsld_decay_map, DECAY_MAP.md); taken out of
//     argv the same way, no TSV without --out;
//   * --cross_out FILE (new) and the other --cross_* flags: the whole-genome form of --grid_out -- the rows between every two
//     chromosomes, or with --cross_bin_size B every two windows of B bp anywhere in the genome, those across two chromosomes
//     included -- binned on the device (ngsld_cross_ld, CROSS.md); taken out of argv the same way, no TSV without --out;
//   * --tree_out FILE (new) and the other --tree_* flags: the single-linkage tree of the sites -- the maximum spanning forest of
//     the graph --cluster_out unites, every merge in order of falling LD -- kept on the device while the rows stream past, and
//     with --tree_cut T1,T2,... --tree_cut_out FILE the clusters at those floors from that one run (ngsld_ld_tree, TREE.md);
//     taken out of argv the same way, no TSV without --out;
#include <getopt.h>
#include <zlib.h>
#include <sys/stat.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <string>
#include <algorithm>
#include <chrono>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/ngsld.h"
#include "../../include/ngsld_host.h"
#include "knobs.h"
#include "host_buf.h"

namespace {

const char *kVersion = "1.2.1-mi355x";

struct Params {  // ngsLD.hpp:11-44
  char *in_geno = nullptr;
  bool in_bin = false, in_probs = false, in_logscale = false;
  uint64_t n_ind = 0, n_sites = 0;
  char *in_pos = nullptr;
  bool in_pos_header = false;
  uint64_t max_kb_dist = 100, max_snp_dist = 0;
  double min_maf = 0;
  bool ignore_miss_data = false, call_geno = false;
  double N_thresh = 0, call_thresh = 0, rnd_sample = 1;
  uint64_t seed = 0;
  bool extend_out = false;
  char *out = nullptr;
  FILE *out_fh = stdout;
  unsigned n_threads = 1, verbose = 1;
  int device = 0;
  double max_gpu_mem = 0;  // GB of device memory the run may use; 0 = what is free on the device
  std::vector<int> devices;  // --devices: more than one entry = one part of the rows per device
  bool keep_parts = false;   // --keep_parts: with --devices and --out, leave parts 1.. in <out>.part<k> instead of appending them
};

// "0-3", "0,2,5", "1" -> device indices; empty on a malformed list
std::vector<int> parse_devices(const char *txt) {
  std::vector<int> out;
  const char *p = txt;
  while (*p) {
    char *end = nullptr;
    const long a = strtol(p, &end, 10);
    if (end == p || a < 0) return {};
    long b = a;
    p = end;
    if (*p == '-') {
      b = strtol(p + 1, &end, 10);
      if (end == p + 1 || b < a) return {};
      p = end;
    }
    for (long d = a; d <= b; ++d) out.push_back((int)d);
    if (*p == ',') ++p;
    else if (*p) return {};
  }
  return out;
}

[[noreturn]] void error(const char *func, const char *msg) {  // gen_func.cpp:12-18
  fflush(stdout);
  fprintf(stderr, "\n=====\nERROR: [%s] %s\n=====\n\n", func, msg);
  perror("\t");
  fflush(stderr);
  exit(-1);
}

// The function the reference names in front of an error of its positions reader: the file is opened by read_file
// (gen_func.cpp:244-246), its fields are counted by read_split (read_data.cpp:134-147), everything else is read_dist's own.
const char *pos_error_function(const char *msg, const char *path) {
  // (a file that opens but holds no usable line is "cannot open file!" too -- from read_split, read_data.cpp:134-136)
  if (std::strcmp(msg, "cannot open file!") == 0) return path != nullptr && access(path, R_OK) == 0 ? "read_split" : "read_file";
  if (std::strcmp(msg, "invalid number of fields in file!") == 0) return "read_split";
  return "read_dist";
}

// ---- --prune_* (new): LD pruning on the device ----
struct PruneArgs {
  bool given = false;  // any --prune_* flag
  const char *out = nullptr, *excl = nullptr, *subset_file = nullptr;
  const char *field = nullptr, *type = nullptr, *precision = nullptr, *max_kb_dist = nullptr, *min_weight = nullptr;
  bool keep_heavy = false;
  ngsld_prune_params p{};
  std::vector<std::string> subset;
  // from the call to the writer: the stats, the labels and the subset the call read, the site states it filled
  ngsld_prune_stats st{};
  std::vector<const char *> lab, sub;
  std::vector<uint8_t> state;
} prune;

// ---- --decay_* (new): LD decay bins and fit on the device ----
struct DecayArgs {
  bool given = false;  // any --decay_* flag
  const char *out = nullptr, *fit = nullptr, *ld = nullptr, *bin_size = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr;
  const char *n_ind = nullptr, *recomb_rate = nullptr;
  ngsld_decay_params p{};
  double n_ind_v = 0, recomb_rate_v = 1;
  ngsld_decay_stats st{};  // from the call to the writer
} decay;

// ---- --blocks_* (new): LD block matrices of one region on the device ----
struct BlocksArgs {
  bool given = false;  // any --blocks_* flag
  const char *out = nullptr, *chr = nullptr, *start = nullptr, *end = nullptr, *ld = nullptr;
  ngsld_blocks_params p{};
} blocks;

// ---- --site_* (new): per-site LD summaries on the device ----
struct SiteArgs {
  bool given = false;  // any --site_* flag
  const char *out = nullptr, *ld = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr, *linked_min = nullptr;
  bool is_signed = false;
  ngsld_site_ld_params p{};
  ngsld_site_ld_stats st{};  // from the call to the writer
} site;

// ---- --cluster_* (new): LD clusters on the device ----
struct ClusterArgs {
  bool given = false;  // any --cluster_* flag
  const char *out = nullptr, *table = nullptr, *field = nullptr, *min_weight = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr;
  const char *min_size = nullptr;
  bool is_signed = false;
  uint64_t min_size_v = 2;
  ngsld_clusters_params p{};
  ngsld_clusters_stats st{};  // from the call to the writer
} cluster;

// ---- --grid_* (new): the LD grid on the device ----
struct GridArgs {
  bool given = false;  // any --grid_* flag
  const char *out = nullptr, *bin_size = nullptr, *ld = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr, *linked_min = nullptr;
  bool is_signed = false;
  ngsld_grid_params p{};
  ngsld_grid_stats st{};  // from the call to the writer
  std::vector<const char *> lab;
} grid;

// ---- --linked_* (new): the linked pairs on the device ----
struct LinkedArgs {
  bool given = false;  // any --linked_* flag
  const char *out = nullptr, *outH = nullptr, *field = nullptr, *min_weight = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr;
  bool is_signed = false;
  ngsld_linked_params p{};
} linked;

// ---- --partners_* (new): every site's top-K LD partners on the device ----
struct PartnersArgs {
  bool given = false;  // any --partners_* flag
  const char *out = nullptr, *k = nullptr, *field = nullptr, *min_weight = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr,
             *sites_file = nullptr;
  bool is_signed = false;
  std::vector<std::string> sites;  // the labels of --partners_sites
  ngsld_partners_params p{};
} partners;

// ---- --scan_* (new): the LD scan on the device ----
struct ScanArgs {
  bool given = false;  // any --scan_* flag
  const char *out = nullptr, *half_window = nullptr, *ld = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr;
  ngsld_scan_params p{};
  ngsld_scan_stats st{};  // from the call to the writer
} scan;

// ---- --dmap_* (new): the LD decay map on the device ----
struct DmapArgs {
  bool given = false;  // any --dmap_* flag
  const char *out = nullptr, *fit = nullptr, *window = nullptr, *ld = nullptr, *bin_size = nullptr, *max_kb_dist = nullptr,
             *min_maf = nullptr, *n_ind = nullptr, *recomb_rate = nullptr, *fit_min_bins = nullptr;
  ngsld_decay_map_params p{};
  double n_ind_v = 0, recomb_rate_v = 1;
  uint64_t fit_min_bins_v = 3;
} dmap;

// ---- --cross_* (new): LD across chromosomes on the device ----
struct CrossArgs {
  bool given = false;  // any --cross_* flag
  const char *out = nullptr, *bin_size = nullptr, *ld = nullptr, *min_maf = nullptr, *linked_min = nullptr, *min_kb_dist = nullptr;
  bool is_signed = false, only = false;
  ngsld_cross_ld_params p{};
} cross;

// ---- --tree_* (new): the single-linkage LD tree on the device ----
struct TreeArgs {
  bool given = false;  // any --tree_* flag
  const char *out = nullptr, *field = nullptr, *min_weight = nullptr, *max_kb_dist = nullptr, *min_maf = nullptr, *cut = nullptr,
             *cut_out = nullptr;
  bool is_signed = false;
  std::vector<std::string> cut_text;  // the floors of --tree_cut as they were typed
  std::vector<double> cut_v;
  ngsld_ld_tree_params p{};
} tree;

bool parse_double(const char *txt, double *out) {
  char *end = nullptr;
  if (txt == nullptr || *txt == 0) return false;
  *out = strtod(txt, &end);
  return *end == 0 && !std::isnan(*out);
}

// The values several families take: flag is the option as the user writes it ("--site_min_maf"), func the checker the ERROR
// block names; a flag that was not given (txt null) leaves *out alone.
[[noreturn]] void bad_value(const char *func, const char *flag, const char *must) {
  const std::string msg = std::string(flag) + must;
  error(func, msg.c_str());
}
// a number (nan is none)
void number_arg(const char *func, const char *flag, const char *txt, double *out) {
  if (txt && !parse_double(txt, out)) bad_value(func, flag, " must be a number!");
}
// a number >= 0 or inf: *_max_kb_dist
void dist_arg(const char *func, const char *flag, const char *txt, double *out) {
  if (txt && (!parse_double(txt, out) || *out < 0)) bad_value(func, flag, " must be a number >= 0 (or inf)!");
}
// a finite number >= 0: *_min_maf, --decay_n_ind
void finite_arg(const char *func, const char *flag, const char *txt, double *out) {
  if (txt && (!parse_double(txt, out) || *out < 0 || std::isinf(*out))) bad_value(func, flag, " must be a number >= 0!");
}
// a TSV column 4..7: --prune_field, --cluster_field
void column_arg(const char *func, const char *flag, const char *txt, int32_t *out) {
  if (txt == nullptr) return;
  char *end = nullptr;
  const long f = strtol(txt, &end, 10);
  if (*txt == 0 || *end != 0 || f < 4 || f > 7) bad_value(func, flag, " must be 4 (r2_ExpG), 5 (D), 6 (D') or 7 (r2)!");
  *out = (int32_t)f;
}
// out_flag ("--site_out") runs on one device
void one_device(const char *func, const Params &pars, const char *out_flag) {
  if (pars.devices.size() > 1) bad_value(func, out_flag, " runs on one device: it cannot be combined with --devices!");
}

// one label per line, plain or gzip-compressed (the script's IO::Zlib reads both); false: the file cannot be opened
bool read_label_file(const char *path, std::vector<std::string> *labels) {
  gzFile f = gzopen(path, "rb");
  if (f == nullptr) return false;
  std::string line;
  char buf[4096];
  while (gzgets(f, buf, sizeof(buf)) != nullptr) {
    line += buf;
    if (!line.empty() && line.back() == '\n') {
      line.pop_back();
      labels->push_back(line);
      line.clear();
    }
  }
  if (!line.empty()) labels->push_back(line);
  gzclose(f);
  return true;
}

void check_prune_args(const Params &pars) {
  PruneArgs *pa = &prune;
  if (pa->out == nullptr || *pa->out == 0) error(__FUNCTION__, "the --prune_* options need --prune_out FILE!");
  ngsld_prune_params &p = pa->p;
  p.struct_size = sizeof(p);
  p.field = 7;
  p.max_kb_dist = INFINITY;
  p.min_weight = 0;
  p.weight_type = 'a';
  p.precision = 4;
  p.keep_heavy = pa->keep_heavy ? 1 : 0;
  column_arg(__FUNCTION__, "--prune_field", pa->field, &p.field);
  if (pa->type) {
    if (std::strlen(pa->type) != 1 || std::strchr("aen", pa->type[0]) == nullptr)
      error(__FUNCTION__, "--prune_weight_type must be a, e or n!");
    p.weight_type = pa->type[0];
  }
  if (pa->precision) {
    char *end = nullptr;
    const long v = strtol(pa->precision, &end, 10);
    if (*pa->precision == 0 || *end != 0 || v < 0 || v > 15) error(__FUNCTION__, "--prune_precision must be an integer in [0,15]!");
    p.precision = (int32_t)v;
  }
  dist_arg(__FUNCTION__, "--prune_max_kb_dist", pa->max_kb_dist, &p.max_kb_dist);
  number_arg(__FUNCTION__, "--prune_min_weight", pa->min_weight, &p.min_weight);
  if (pa->excl != nullptr && *pa->excl == 0) error(__FUNCTION__, "--prune_excl needs a file name!");
  one_device(__FUNCTION__, pars, "--prune_out");
  if (pa->subset_file && !read_label_file(pa->subset_file, &pa->subset)) error(__FUNCTION__, "cannot open --prune_subset file!");
}

// the statistics of --decay_ld, in TSV column order (bit k = column 4 + k)
const char *const kDecayFields[4] = {"r2_ExpG", "D", "Dp", "r2"};

// the statistics of a comma-separated list (--decay_ld, --blocks_ld, --site_ld, --grid_ld) as a mask, bit k = column 4 + k; 0 when a name is unknown
uint32_t parse_ld_list(const char *txt) {
  uint32_t fields = 0;
  const std::string s = txt;
  size_t b = 0;
  while (true) {
    const size_t e = std::min(s.find(',', b), s.size());
    const std::string name = s.substr(b, e - b);
    int f = -1;
    for (int k = 0; k < 4; ++k)
      if (name == kDecayFields[k]) f = k;
    if (f < 0) return 0;
    fields |= 1u << f;
    if (e == s.size()) return fields;
    b = e + 1;
  }
}

// ... into *fields, where the flag was given
void ld_arg(const char *func, const char *flag, const char *txt, uint32_t *fields) {
  if (txt && (*fields = parse_ld_list(txt)) == 0) bad_value(func, flag, " must be a comma-separated list of r2_ExpG, D, Dp and r2!");
}

// the statistics of a mask, as indices into kDecayFields
std::vector<int> fields_of(uint32_t mask) {
  std::vector<int> fields;
  for (int k = 0; k < 4; ++k)
    if ((mask >> k) & 1u) fields.push_back(k);
  return fields;
}

void check_decay_args(const Params &pars) {
  DecayArgs *da = &decay;
  if (da->out == nullptr && da->fit == nullptr) error(__FUNCTION__, "the --decay_* options need --decay_out FILE or --decay_fit FILE!");
  if (da->out != nullptr && *da->out == 0) error(__FUNCTION__, "--decay_out needs a file name!");
  if (da->fit != nullptr && *da->fit == 0) error(__FUNCTION__, "--decay_fit needs a file name!");
  ngsld_decay_params &p = da->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.bin_size = 250;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  ld_arg(__FUNCTION__, "--decay_ld", da->ld, &p.fields);
  if (da->bin_size && (!parse_double(da->bin_size, &p.bin_size) || !(p.bin_size > 1) || std::isinf(p.bin_size)))
    error(__FUNCTION__, "--decay_bin_size must be a number > 1!");
  dist_arg(__FUNCTION__, "--decay_max_kb_dist", da->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--decay_min_maf", da->min_maf, &p.min_maf);
  finite_arg(__FUNCTION__, "--decay_n_ind", da->n_ind, &da->n_ind_v);
  if (da->recomb_rate && (!parse_double(da->recomb_rate, &da->recomb_rate_v) || !(da->recomb_rate_v > 0) || std::isinf(da->recomb_rate_v)))
    error(__FUNCTION__, "--decay_recomb_rate must be a number > 0!");
  if (da->n_ind_v > 0 && (p.fields & (1u | 8u)) == 0) error(__FUNCTION__, "--decay_n_ind is only used for the r2 and r2_ExpG fits!");
  if (da->n_ind_v > 0 && da->fit != nullptr && (p.fields & 4u))
    error(__FUNCTION__, "--decay_n_ind cannot be combined with a Dp fit!");
  one_device(__FUNCTION__, pars, "--decay_out");
}

// a --blocks_start / --blocks_end value: plain decimal digits
bool parse_position(const char *txt, uint64_t *out) {
  if (txt == nullptr || *txt == 0 || std::strlen(txt) > 19) return false;
  for (const char *q = txt; *q; ++q)
    if (*q < '0' || *q > '9') return false;
  *out = std::strtoull(txt, nullptr, 10);
  return true;
}

void check_blocks_args(const Params &pars) {
  BlocksArgs *ba = &blocks;
  if (ba->out == nullptr) error(__FUNCTION__, "the --blocks_* options need --blocks_out PREFIX!");
  if (*ba->out == 0) error(__FUNCTION__, "--blocks_out needs a file name prefix!");
  ngsld_blocks_params &p = ba->p;
  p.struct_size = sizeof(p);
  p.fields = 4u | 8u;  // Dp, r2: the script's pair
  if (ba->chr == nullptr || *ba->chr == 0) error(__FUNCTION__, "--blocks_out needs the region's chromosome: --blocks_chr CHR!");
  p.chr = ba->chr;
  if (ba->start == nullptr) error(__FUNCTION__, "--blocks_out needs the region's start: --blocks_start INT!");
  if (ba->end == nullptr) error(__FUNCTION__, "--blocks_out needs the region's end: --blocks_end INT!");
  if (!parse_position(ba->start, &p.start)) error(__FUNCTION__, "--blocks_start must be a non-negative integer!");
  if (!parse_position(ba->end, &p.end)) error(__FUNCTION__, "--blocks_end must be a non-negative integer!");
  if (p.start >= p.end) error(__FUNCTION__, "start position must be smaller than end position.");
  ld_arg(__FUNCTION__, "--blocks_ld", ba->ld, &p.fields);
  if (pars.in_pos == nullptr) error(__FUNCTION__, "--blocks_out needs positions: it cannot run without --pos!");
  one_device(__FUNCTION__, pars, "--blocks_out");
}

void check_site_args(const Params &pars) {
  SiteArgs *sa = &site;
  if (sa->out == nullptr) error(__FUNCTION__, "the --site_* options need --site_out FILE!");
  if (*sa->out == 0) error(__FUNCTION__, "--site_out needs a file name!");
  ngsld_site_ld_params &p = sa->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.linked_min = 0.5;
  p.abs_value = sa->is_signed ? 0 : 1;
  ld_arg(__FUNCTION__, "--site_ld", sa->ld, &p.fields);
  dist_arg(__FUNCTION__, "--site_max_kb_dist", sa->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--site_min_maf", sa->min_maf, &p.min_maf);
  number_arg(__FUNCTION__, "--site_linked_min", sa->linked_min, &p.linked_min);
  one_device(__FUNCTION__, pars, "--site_out");
}

void check_cluster_args(const Params &pars) {
  ClusterArgs *ca = &cluster;
  if (ca->out == nullptr && ca->table == nullptr)
    error(__FUNCTION__, "the --cluster_* options need --cluster_out FILE or --cluster_table FILE!");
  if (ca->out != nullptr && *ca->out == 0) error(__FUNCTION__, "--cluster_out needs a file name!");
  if (ca->table != nullptr && *ca->table == 0) error(__FUNCTION__, "--cluster_table needs a file name!");
  ngsld_clusters_params &p = ca->p;
  p.struct_size = sizeof(p);
  p.field = 7;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.min_weight = 0.5;
  p.abs_value = ca->is_signed ? 0 : 1;
  column_arg(__FUNCTION__, "--cluster_field", ca->field, &p.field);
  number_arg(__FUNCTION__, "--cluster_min_weight", ca->min_weight, &p.min_weight);
  dist_arg(__FUNCTION__, "--cluster_max_kb_dist", ca->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--cluster_min_maf", ca->min_maf, &p.min_maf);
  if (ca->min_size) {
    char *end = nullptr;
    const bool digits = *ca->min_size >= '0' && *ca->min_size <= '9';
    const unsigned long long v = digits ? strtoull(ca->min_size, &end, 10) : 0;
    if (!digits || *end != 0 || v < 1 || v > 0xffffffffull) error(__FUNCTION__, "--cluster_min_size must be an integer >= 1!");
    ca->min_size_v = v;
  }
  one_device(__FUNCTION__, pars, "--cluster_out");
}

void check_tree_args(const Params &pars) {
  TreeArgs *ta = &tree;
  if (ta->out == nullptr && ta->cut_out == nullptr) error(__FUNCTION__, "the --tree_* options need --tree_out FILE or --tree_cut_out FILE!");
  if (ta->out != nullptr && *ta->out == 0) error(__FUNCTION__, "--tree_out needs a file name!");
  if (ta->cut_out != nullptr && *ta->cut_out == 0) error(__FUNCTION__, "--tree_cut_out needs a file name!");
  if (ta->cut_out != nullptr && ta->cut == nullptr) error(__FUNCTION__, "--tree_cut_out needs the floors to cut at: --tree_cut T1,T2,...!");
  if (ta->cut != nullptr && ta->cut_out == nullptr) error(__FUNCTION__, "--tree_cut needs --tree_cut_out FILE!");
  ngsld_ld_tree_params &p = ta->p;
  p.struct_size = sizeof(p);
  p.field = 7;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.min_weight = 0.1;
  p.abs_value = ta->is_signed ? 0 : 1;
  column_arg(__FUNCTION__, "--tree_field", ta->field, &p.field);
  number_arg(__FUNCTION__, "--tree_min_weight", ta->min_weight, &p.min_weight);
  dist_arg(__FUNCTION__, "--tree_max_kb_dist", ta->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--tree_min_maf", ta->min_maf, &p.min_maf);
  if (ta->cut) {  // a comma-separated list of floors, none below the tree's own
    const std::string txt = ta->cut;
    size_t b = 0;
    while (true) {
      const size_t e = std::min(txt.find(',', b), txt.size());
      const std::string one = txt.substr(b, e - b);
      double v = 0;
      if (!parse_double(one.c_str(), &v)) error(__FUNCTION__, "--tree_cut must be a comma-separated list of numbers!");
      if (v < p.min_weight) error(__FUNCTION__, "--tree_cut cannot go below --tree_min_weight: the tree holds no edge under it!");
      ta->cut_text.push_back(one);
      ta->cut_v.push_back(v);
      if (e == txt.size()) break;
      b = e + 1;
    }
  }
  one_device(__FUNCTION__, pars, "--tree_out");
}

void check_grid_args(const Params &pars) {
  GridArgs *ga = &grid;
  if (ga->out == nullptr) error(__FUNCTION__, "the --grid_* options need --grid_out FILE!");
  if (*ga->out == 0) error(__FUNCTION__, "--grid_out needs a file name!");
  ngsld_grid_params &p = ga->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.linked_min = 0.5;
  p.abs_value = ga->is_signed ? 0 : 1;
  if (ga->bin_size == nullptr) error(__FUNCTION__, "--grid_out needs the window in bp: --grid_bin_size INT!");
  if (!parse_position(ga->bin_size, &p.bin_size) || p.bin_size < 1 || p.bin_size >= (1ull << 31))
    error(__FUNCTION__, "--grid_bin_size must be an integer in [1, 2147483647]!");
  ld_arg(__FUNCTION__, "--grid_ld", ga->ld, &p.fields);
  dist_arg(__FUNCTION__, "--grid_max_kb_dist", ga->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--grid_min_maf", ga->min_maf, &p.min_maf);
  number_arg(__FUNCTION__, "--grid_linked_min", ga->linked_min, &p.linked_min);
  if (pars.in_pos == nullptr) error(__FUNCTION__, "--grid_out needs positions: it cannot run without --pos!");
  one_device(__FUNCTION__, pars, "--grid_out");
}

// checked as the grid family is; --cross_bin_size is optional (absent: one bin per chromosome)
void check_cross_args(const Params &pars) {
  CrossArgs *ca = &cross;
  if (ca->out == nullptr) error(__FUNCTION__, "the --cross_* options need --cross_out FILE!");
  if (*ca->out == 0) error(__FUNCTION__, "--cross_out needs a file name!");
  ngsld_cross_ld_params &p = ca->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.bin_size = 0;
  p.min_maf = 0;
  p.linked_min = 0.5;
  p.min_kb_dist = 0;
  p.abs_value = ca->is_signed ? 0 : 1;
  p.within = ca->only ? 0 : 1;
  if (ca->bin_size && (!parse_position(ca->bin_size, &p.bin_size) || p.bin_size < 1 || p.bin_size >= (1ull << 31)))
    error(__FUNCTION__, "--cross_bin_size must be an integer in [1, 2147483647]!");
  ld_arg(__FUNCTION__, "--cross_ld", ca->ld, &p.fields);
  finite_arg(__FUNCTION__, "--cross_min_maf", ca->min_maf, &p.min_maf);
  number_arg(__FUNCTION__, "--cross_linked_min", ca->linked_min, &p.linked_min);
  finite_arg(__FUNCTION__, "--cross_min_kb_dist", ca->min_kb_dist, &p.min_kb_dist);
  if (pars.in_pos == nullptr) error(__FUNCTION__, "--cross_out needs positions: it cannot run without --pos!");
  one_device(__FUNCTION__, pars, "--cross_out");
}

void check_linked_args(const Params &pars) {
  LinkedArgs *la = &linked;
  if (la->out == nullptr && la->outH == nullptr) error(__FUNCTION__, "the --linked_* options need --linked_out FILE or --linked_outH FILE!");
  if (la->out != nullptr && la->outH != nullptr) error(__FUNCTION__, "--linked_out and --linked_outH cannot be combined!");
  if (la->out != nullptr && *la->out == 0) error(__FUNCTION__, "--linked_out needs a file name!");
  if (la->outH != nullptr && *la->outH == 0) error(__FUNCTION__, "--linked_outH needs a file name!");
  ngsld_linked_params &p = la->p;
  p.struct_size = sizeof(p);
  p.field = 7;
  p.min_weight = 0.5;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.abs_value = la->is_signed ? 0 : 1;
  p.want = NGSLD_LINKED_TEXT;
  column_arg(__FUNCTION__, "--linked_field", la->field, &p.field);
  number_arg(__FUNCTION__, "--linked_min_weight", la->min_weight, &p.min_weight);
  dist_arg(__FUNCTION__, "--linked_max_kb_dist", la->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--linked_min_maf", la->min_maf, &p.min_maf);
  one_device(__FUNCTION__, pars, "--linked_out");
}

void check_partners_args(const Params &pars) {
  PartnersArgs *pa = &partners;
  if (pa->out == nullptr) error(__FUNCTION__, "the --partners_* options need --partners_out FILE!");
  if (*pa->out == 0) error(__FUNCTION__, "--partners_out needs a file name!");
  ngsld_partners_params &p = pa->p;
  p.struct_size = sizeof(p);
  p.field = 7;
  p.min_weight = 0.5;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.abs_value = pa->is_signed ? 0 : 1;
  if (pa->k == nullptr) error(__FUNCTION__, "--partners_out needs the partners kept per site: --partners_k INT!");
  char *end = nullptr;
  const long k = strtol(pa->k, &end, 10);
  if (*pa->k == 0 || *end != 0 || k < 1 || k > 64) error(__FUNCTION__, "--partners_k must be an integer in [1,64]!");
  p.k = (uint32_t)k;
  column_arg(__FUNCTION__, "--partners_field", pa->field, &p.field);
  number_arg(__FUNCTION__, "--partners_min_weight", pa->min_weight, &p.min_weight);
  dist_arg(__FUNCTION__, "--partners_max_kb_dist", pa->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--partners_min_maf", pa->min_maf, &p.min_maf);
  one_device(__FUNCTION__, pars, "--partners_out");
  if (pa->sites_file && !read_label_file(pa->sites_file, &pa->sites)) error(__FUNCTION__, "cannot open --partners_sites file!");
}

void check_scan_args(const Params &pars) {
  ScanArgs *sa = &scan;
  if (sa->out == nullptr) error(__FUNCTION__, "the --scan_* options need --scan_out FILE!");
  if (*sa->out == 0) error(__FUNCTION__, "--scan_out needs a file name!");
  ngsld_scan_params &p = sa->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  if (sa->half_window == nullptr) error(__FUNCTION__, "--scan_out needs the half window in bp: --scan_half_window INT!");
  if (!parse_position(sa->half_window, &p.half_window) || p.half_window >= (1ull << 31))
    error(__FUNCTION__, "--scan_half_window must be an integer in [0, 2147483647]!");
  ld_arg(__FUNCTION__, "--scan_ld", sa->ld, &p.fields);
  dist_arg(__FUNCTION__, "--scan_max_kb_dist", sa->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--scan_min_maf", sa->min_maf, &p.min_maf);
  // (the library refuses it too: here before a device is touched)
  if (pars.max_kb_dist > 0 && pars.max_kb_dist * 1000 < 2 * p.half_window) {
    const std::string msg = "--scan_half_window " + std::to_string(p.half_window) + " needs the pairs up to " +
                            std::to_string(2 * p.half_window) + " bp apart: --max_kb_dist holds them up to " +
                            std::to_string(pars.max_kb_dist * 1000) + " bp!";
    error(__FUNCTION__, msg.c_str());
  }
  one_device(__FUNCTION__, pars, "--scan_out");
}

// checked as the decay family is; --dmap_window (absent: a group per chromosome) needs the positions of --pos
void check_dmap_args(const Params &pars) {
  DmapArgs *ma = &dmap;
  if (ma->out == nullptr && ma->fit == nullptr) error(__FUNCTION__, "the --dmap_* options need --dmap_out FILE or --dmap_fit FILE!");
  if (ma->out != nullptr && *ma->out == 0) error(__FUNCTION__, "--dmap_out needs a file name!");
  if (ma->fit != nullptr && *ma->fit == 0) error(__FUNCTION__, "--dmap_fit needs a file name!");
  ngsld_decay_map_params &p = ma->p;
  p.struct_size = sizeof(p);
  p.fields = 8;  // r2
  p.bin_size = 250;
  p.max_kb_dist = INFINITY;
  p.min_maf = 0;
  p.window = 0;
  ld_arg(__FUNCTION__, "--dmap_ld", ma->ld, &p.fields);
  if (ma->bin_size && (!parse_double(ma->bin_size, &p.bin_size) || !(p.bin_size > 1) || std::isinf(p.bin_size)))
    error(__FUNCTION__, "--dmap_bin_size must be a number > 1!");
  dist_arg(__FUNCTION__, "--dmap_max_kb_dist", ma->max_kb_dist, &p.max_kb_dist);
  finite_arg(__FUNCTION__, "--dmap_min_maf", ma->min_maf, &p.min_maf);
  finite_arg(__FUNCTION__, "--dmap_n_ind", ma->n_ind, &ma->n_ind_v);
  if (ma->recomb_rate && (!parse_double(ma->recomb_rate, &ma->recomb_rate_v) || !(ma->recomb_rate_v > 0) || std::isinf(ma->recomb_rate_v)))
    error(__FUNCTION__, "--dmap_recomb_rate must be a number > 0!");
  if (ma->n_ind_v > 0 && (p.fields & (1u | 8u)) == 0) error(__FUNCTION__, "--dmap_n_ind is only used for the r2 and r2_ExpG fits!");
  if (ma->n_ind_v > 0 && ma->fit != nullptr && (p.fields & 4u)) error(__FUNCTION__, "--dmap_n_ind cannot be combined with a Dp fit!");
  if (ma->window && (!parse_position(ma->window, &p.window) || p.window < 1 || p.window >= (1ull << 31)))
    error(__FUNCTION__, "--dmap_window must be an integer in [1, 2147483647]!");
  if (ma->fit_min_bins && (!parse_position(ma->fit_min_bins, &ma->fit_min_bins_v) || ma->fit_min_bins_v < 3))
    error(__FUNCTION__, "--dmap_fit_min_bins must be an integer >= 3 (the parameters of the fit)!");
  if (ma->window != nullptr && pars.in_pos == nullptr) error(__FUNCTION__, "--dmap_window needs positions: it cannot run without --pos!");
  one_device(__FUNCTION__, pars, "--dmap_out");
}

FILE *open_or_die(const char *path) {
  FILE *f = fopen(path, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open LD decay output file!");
  return f;
}

// Each of the six analyses that ngsld_analyze takes comes in three parts: stage_* sets up what its call reads and fills and
// describes it as an entry of ngsld_analyze's list, run_* is the single call over the same state, write_* reads the result
// through the getters and writes the files.  One output flag runs stage, run, write; several run every stage, one
// ngsld_analyze, every write (main).
ngsld_analysis analysis_entry(uint32_t kind, const void *params, void *stats, const char *const *labels = nullptr,
                              uint8_t *site_state = nullptr) {
  ngsld_analysis a{};
  a.struct_size = sizeof(a);
  a.kind = kind;
  a.params = params;
  a.stats = stats;
  a.labels = labels;
  a.site_state = site_state;
  return a;
}

ngsld_analysis stage_decay(const Params &, const ngsld_pos *) {
  decay.st = ngsld_decay_stats{};
  decay.st.struct_size = sizeof(decay.st);
  return analysis_entry(NGSLD_AN_DECAY, &decay.p, &decay.st);
}

void run_decay(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_decay(ctx, &decay.p, &decay.st) != NGSLD_OK) error("ngsld_decay", ngsld_last_error(ctx));
}

// --decay_out's bin table, and --dmap_out's behind a prefix of "chr\twin_start\t": opened with its header, then one line per
// non-empty bin: its lower break, rows, a mean per statistic (17 digits: the doubles themselves)
FILE *open_bin_table(const char *path, const char *prefix, const std::vector<int> &fields) {
  FILE *f = open_or_die(path);
  fprintf(f, "%sdist\tn", prefix);
  for (int k : fields) fprintf(f, "\t%s", kDecayFields[k]);
  fprintf(f, "\n");
  return f;
}

void write_bin_rows(FILE *f, const char *prefix, uint64_t nb, const double *dist, const uint64_t *count, const double *mean, size_t nf) {
  for (uint64_t i = 0; i < nb; ++i) {
    fprintf(f, "%s%.15g\t%lu", prefix, dist[i], (unsigned long)count[i]);
    for (size_t v = 0; v < nf; ++v) fprintf(f, "\t%.17g", mean[i * nf + v]);
    fprintf(f, "\n");
  }
}

// --decay_fit's and --dmap_fit's line of statistic `field` (column v of the nb bins' means) behind its name; empty: no fit on these bins
std::string fit_tail(uint64_t nb, const double *dist, const double *mean, size_t nf, size_t v, int field, double n_ind, double recomb_rate) {
  std::vector<double> y(nb);
  for (uint64_t i = 0; i < nb; ++i) y[i] = mean[i * nf + v];
  ngsld_decay_fit_result r{};
  if (ngsld_host_decay_fit(nb, dist, y.data(), 4 + field, n_ind, recomb_rate, &r) != NGSLD_OK) return std::string();
  char buf[512];
  std::snprintf(buf, sizeof(buf), "\t%.17g\t%.17g\t%.17g\t%.17g\t%lu\n", r.rate, r.ld_max, r.ld_min, r.sse, (unsigned long)r.n_bins);
  return buf;
}

void write_decay(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *) {
  DecayArgs &da = decay;
  const std::vector<int> fields = fields_of(da.p.fields);
  const size_t nf = fields.size();
  const uint64_t nb = da.st.bins;
  std::vector<double> dist(nb), mean(nb * nf);
  std::vector<uint64_t> count(nb);
  if (ngsld_decay_bins(ctx, nb, dist.data(), count.data(), mean.data(), nullptr) != NGSLD_OK)
    error("ngsld_decay_bins", ngsld_last_error(ctx));
  if (da.out) {
    FILE *f = open_bin_table(da.out, "", fields);
    write_bin_rows(f, "", nb, dist.data(), count.data(), mean.data(), nf);
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD decay output file!");
  }
  if (da.fit) {  // one line per fitted statistic (D has no model); a fit that fails leaves no file
    if (nb == 0) error(__FUNCTION__, "no pair falls in a decay bin: nothing to fit!");
    std::string text = "LD\tDecayRate\tLDmax\tLDmin\tSSE\tn_bins\n";
    for (size_t v = 0; v < nf; ++v) {
      if (fields[v] == 1) continue;
      const std::string name = kDecayFields[fields[v]], tail = fit_tail(nb, dist.data(), mean.data(), nf, v, fields[v], da.n_ind_v, da.recomb_rate_v);
      if (tail.empty()) error(__FUNCTION__, ("the " + name + " fit is not defined on these bins (Dp: a bin beyond 10^6 / recomb_rate bp)!").c_str());
      text += name + tail;
    }
    FILE *f = open_or_die(da.fit);
    fputs(text.c_str(), f);
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD decay fit file!");
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD decay: %lu bins from %lu of %lu pairs\n", (unsigned long)nb, (unsigned long)da.st.pairs_counted,
            (unsigned long)da.st.pairs);
}

// --dmap_out: chr, win_start, then --decay_out's own columns, one line per non-empty bin of every group; --dmap_fit: chr, win_start,
// then --decay_fit's own columns, one line per group and fitted statistic (NA where the group has fewer bins than --dmap_fit_min_bins)
void run_dmap(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  DmapArgs &ma = dmap;
  std::vector<const char *> lab;
  if (pos) {
    lab.resize(pars.n_sites);
    for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  }
  ngsld_decay_map_stats st{};
  st.struct_size = sizeof(st);
  if (ngsld_decay_map(ctx, &ma.p, pos ? lab.data() : nullptr, &st) != NGSLD_OK) error("ngsld_decay_map", ngsld_last_error(ctx));
  const std::vector<int> fields = fields_of(ma.p.fields);
  const size_t nf = fields.size();
  const uint64_t ng = st.groups, nb = st.bins;
  uint64_t n_chr = 0;
  if (ngsld_decay_map_chromosomes(ctx, 0, nullptr, &n_chr) != NGSLD_OK) error("ngsld_decay_map_chromosomes", ngsld_last_error(ctx));
  std::vector<const char *> chr_name(n_chr);
  if (ngsld_decay_map_chromosomes(ctx, n_chr, chr_name.data(), nullptr) != NGSLD_OK)
    error("ngsld_decay_map_chromosomes", ngsld_last_error(ctx));
  std::vector<uint32_t> chr(ng);
  std::vector<uint64_t> win_start(ng), first(ng), len(ng), count(nb);
  std::vector<double> dist(nb), mean(nb * nf);
  if (ngsld_decay_map_groups(ctx, ng, chr.data(), win_start.data(), first.data(), len.data(), nullptr) != NGSLD_OK)
    error("ngsld_decay_map_groups", ngsld_last_error(ctx));
  if (ngsld_decay_map_bins(ctx, nb, dist.data(), count.data(), mean.data(), nullptr) != NGSLD_OK)
    error("ngsld_decay_map_bins", ngsld_last_error(ctx));
  const auto prefix = [&](uint64_t g) { return std::string(chr_name[chr[g]]) + "\t" + std::to_string(win_start[g]) + "\t"; };
  if (ma.out) {
    FILE *f = open_bin_table(ma.out, "chr\twin_start\t", fields);
    for (uint64_t g = 0; g < ng; ++g)
      write_bin_rows(f, prefix(g).c_str(), len[g], dist.data() + first[g], count.data() + first[g], mean.data() + first[g] * nf, nf);
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD decay map output file!");
  }
  if (ma.fit) {
    FILE *f = open_or_die(ma.fit);
    fprintf(f, "chr\twin_start\tLD\tDecayRate\tLDmax\tLDmin\tSSE\tn_bins\n");
    for (uint64_t g = 0; g < ng; ++g)
      for (size_t v = 0; v < nf; ++v) {
        if (fields[v] == 1) continue;  // (D has no model)
        fprintf(f, "%s%s", prefix(g).c_str(), kDecayFields[fields[v]]);
        const std::string tail = len[g] < ma.fit_min_bins_v
                                     ? "\tNA\tNA\tNA\tNA\t" + std::to_string(len[g]) + "\n"
                                     : fit_tail(len[g], dist.data() + first[g], mean.data() + first[g] * nf, nf, v, fields[v], ma.n_ind_v, ma.recomb_rate_v);
        if (tail.empty())
          error(__FUNCTION__, (std::string("the ") + kDecayFields[fields[v]] + " fit is not defined on the bins of " + chr_name[chr[g]] + ":" +
                               std::to_string(win_start[g]) + " (Dp: a bin beyond 10^6 / recomb_rate bp)!").c_str());
        fputs(tail.c_str(), f);
      }
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD decay map fit file!");
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD decay map: %lu groups, %lu bins from %lu of %lu pairs\n", (unsigned long)ng, (unsigned long)nb,
            (unsigned long)st.pairs_counted, (unsigned long)st.pairs);
}

// a value in micro-units as exact six-decimal text
void print_micro(FILE *f, int64_t q) {
  const uint64_t a = q < 0 ? (uint64_t)0 - (uint64_t)q : (uint64_t)q;
  fprintf(f, "\t%s%lu.%06lu", q < 0 ? "-" : "", (unsigned long)(a / 1000000u), (unsigned long)(a % 1000000u));
}

// a site as --site_out, --cluster_out and --cluster_table write it: its label up to the first TAB, without --pos its 1-based index
void print_site(FILE *f, const ngsld_pos *pos, uint64_t s) {
  if (pos) {
    const char *lab = ngsld_host_label(pos, s);
    fwrite(lab, 1, strcspn(lab, "\t"), f);
  } else {
    fprintf(f, "%lu", (unsigned long)(s + 1));
  }
}

// The summaries --site_out and --grid_out write after a line's own columns: sum, mean, max and linked of every chosen statistic.
void print_summary_header(FILE *f, const std::vector<int> &fields) {
  for (int k : fields) fprintf(f, "\tsum_%s\tmean_%s\tmax_%s\tlinked_%s", kDecayFields[k], kDecayFields[k], kDecayFields[k], kDecayFields[k]);
  fprintf(f, "\n");
}
// entry i of n, which has `rows` rows (the arrays hold one statistic after the other); NA for the mean and max of no rows
void print_summaries(FILE *f, size_t nf, uint64_t n, uint64_t i, uint64_t rows, const int64_t *sum, const double *mean, const int64_t *top,
                     const uint64_t *linked) {
  for (size_t v = 0; v < nf; ++v) {
    print_micro(f, sum[v * n + i]);
    if (rows == 0) {
      fprintf(f, "\tNA\tNA");
    } else {
      fprintf(f, "\t%.17g", mean[v * n + i]);
      print_micro(f, top[v * n + i]);
    }
    fprintf(f, "\t%lu", (unsigned long)linked[v * n + i]);
  }
  fprintf(f, "\n");
}

// one line per site of the input, in file order: its label up to the first TAB (without --pos: its 1-based index), the
// counted rows, then sum, mean, max and linked of every chosen statistic; NA for the mean and max of a site without rows
ngsld_analysis stage_site(const Params &, const ngsld_pos *) {
  site.st = ngsld_site_ld_stats{};
  site.st.struct_size = sizeof(site.st);
  return analysis_entry(NGSLD_AN_SITE_LD, &site.p, &site.st);
}

void run_site(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_site_ld(ctx, &site.p, &site.st) != NGSLD_OK) error("ngsld_site_ld", ngsld_last_error(ctx));
}

void write_site(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  SiteArgs &sa = site;
  const ngsld_site_ld_stats &st = sa.st;
  const uint64_t n = pars.n_sites;
  const std::vector<int> fields = fields_of(sa.p.fields);
  const size_t nf = fields.size();
  std::vector<uint64_t> rows(n), linked(nf * n);
  std::vector<int64_t> sum(nf * n), top(nf * n);
  std::vector<double> mean(nf * n);
  for (size_t v = 0; v < nf; ++v)
    if (ngsld_site_ld_get(ctx, 4 + fields[v], rows.data(), sum.data() + v * n, top.data() + v * n, linked.data() + v * n,
                          mean.data() + v * n) != NGSLD_OK)
      error("ngsld_site_ld_get", ngsld_last_error(ctx));
  FILE *f = fopen(sa.out, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open site LD output file!");
  fprintf(f, "site\tn");
  print_summary_header(f, fields);
  for (uint64_t s = 0; s < n; ++s) {
    print_site(f, pos, s);
    fprintf(f, "\t%lu", (unsigned long)rows[s]);
    print_summaries(f, nf, n, s, rows[s], sum.data(), mean.data(), top.data(), linked.data());
  }
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write site LD output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> Site LD: %lu of %lu sites in %lu of %lu pairs\n", (unsigned long)st.sites_with_pairs, (unsigned long)n,
            (unsigned long)st.pairs_counted, (unsigned long)st.pairs);
}

// one line per site of the input, in file order: its label up to the first TAB (without --pos: its 1-based index), the sites of
// its window and of its two flanks, the rows inside the left flank, inside the right flank and across the site, then per chosen
// statistic the three sums, zns and omega; NA where a ratio is not defined
ngsld_analysis stage_scan(const Params &, const ngsld_pos *) {
  scan.st = ngsld_scan_stats{};
  scan.st.struct_size = sizeof(scan.st);
  return analysis_entry(NGSLD_AN_SCAN, &scan.p, &scan.st);
}

void run_scan(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_scan(ctx, &scan.p, &scan.st) != NGSLD_OK) error("ngsld_scan", ngsld_last_error(ctx));
}

void write_scan(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  ScanArgs &sa = scan;
  const ngsld_scan_stats &st = sa.st;
  const uint64_t n = pars.n_sites;
  const std::vector<int> fields = fields_of(sa.p.fields);
  const size_t nf = fields.size();
  std::vector<uint32_t> first(n), last(n);
  std::vector<uint64_t> rows(3 * n);
  std::vector<int64_t> sum(nf * 3 * n);
  std::vector<double> zns(nf * n), omega(nf * n);
  for (size_t v = 0; v < nf; ++v)
    if (ngsld_scan_get(ctx, 4 + fields[v], first.data(), last.data(), rows.data(), rows.data() + n, rows.data() + 2 * n,
                       sum.data() + (v * 3) * n, sum.data() + (v * 3 + 1) * n, sum.data() + (v * 3 + 2) * n, zns.data() + v * n,
                       omega.data() + v * n) != NGSLD_OK)
      error("ngsld_scan_get", ngsld_last_error(ctx));
  FILE *f = fopen(sa.out, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open LD scan output file!");
  fprintf(f, "site\twin_sites\tleft_sites\tright_sites\tn_ll\tn_rr\tn_lr");
  for (int k : fields)
    fprintf(f, "\tsum_ll_%s\tsum_rr_%s\tsum_lr_%s\tzns_%s\tomega_%s", kDecayFields[k], kDecayFields[k], kDecayFields[k], kDecayFields[k],
            kDecayFields[k]);
  fprintf(f, "\n");
  uint64_t with_rows = 0;
  for (uint64_t s = 0; s < n; ++s) {
    print_site(f, pos, s);
    fprintf(f, "\t%lu\t%lu\t%lu\t%lu\t%lu\t%lu", (unsigned long)(last[s] - first[s] + 1), (unsigned long)(s - first[s] + 1),
            (unsigned long)(last[s] - s), (unsigned long)rows[s], (unsigned long)rows[n + s], (unsigned long)rows[2 * n + s]);
    if (rows[s] + rows[n + s] + rows[2 * n + s] > 0) ++with_rows;
    for (size_t v = 0; v < nf; ++v) {
      for (size_t k = 0; k < 3; ++k) print_micro(f, sum[(v * 3 + k) * n + s]);
      for (const double x : {zns[v * n + s], omega[v * n + s]}) {
        if (std::isnan(x))
          fprintf(f, "\tNA");
        else
          fprintf(f, "\t%.17g", x);
      }
    }
    fprintf(f, "\n");
  }
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD scan output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD scan: %lu of %lu windows with rows (the largest of %lu sites), %lu of %lu pairs counted\n",
            (unsigned long)with_rows, (unsigned long)n, (unsigned long)st.largest_window, (unsigned long)st.pairs_counted,
            (unsigned long)st.pairs);
}

// one line per cell with rows, by chromosome (file order), bin1, bin2: the chromosome, the lower breaks b * B of the two
// windows, the counted rows, then sum, mean, max and linked of every chosen statistic -- the long form geom_tile and image read
ngsld_analysis stage_grid(const Params &pars, const ngsld_pos *pos) {
  grid.lab.resize(pars.n_sites);
  for (uint64_t s = 0; s < pars.n_sites; s++) grid.lab[s] = ngsld_host_label(pos, s);
  grid.st = ngsld_grid_stats{};
  grid.st.struct_size = sizeof(grid.st);
  return analysis_entry(NGSLD_AN_GRID, &grid.p, &grid.st, grid.lab.data());
}

void run_grid(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_grid(ctx, &grid.p, grid.lab.data(), &grid.st) != NGSLD_OK) error("ngsld_grid", ngsld_last_error(ctx));
}

void write_grid(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *) {
  GridArgs &ga = grid;
  const ngsld_grid_stats &st = ga.st;
  const uint64_t n = st.cells, B = ga.p.bin_size;
  const std::vector<int> fields = fields_of(ga.p.fields);
  const size_t nf = fields.size();
  uint64_t n_chr = 0;
  if (ngsld_grid_chromosomes(ctx, 0, nullptr, &n_chr) != NGSLD_OK) error("ngsld_grid_chromosomes", ngsld_last_error(ctx));
  std::vector<const char *> chr_name(n_chr);
  if (ngsld_grid_chromosomes(ctx, n_chr, chr_name.data(), nullptr) != NGSLD_OK) error("ngsld_grid_chromosomes", ngsld_last_error(ctx));
  std::vector<uint32_t> chr(n);
  std::vector<uint64_t> b1(n), b2(n), rows(n), linked(nf * n);
  std::vector<int64_t> sum(nf * n), top(nf * n);
  std::vector<double> mean(nf * n);
  if (ngsld_grid_cells(ctx, n, chr.data(), b1.data(), b2.data(), rows.data(), nullptr) != NGSLD_OK)
    error("ngsld_grid_cells", ngsld_last_error(ctx));
  for (size_t v = 0; v < nf; ++v)
    if (ngsld_grid_get(ctx, 4 + fields[v], n, sum.data() + v * n, top.data() + v * n, linked.data() + v * n, mean.data() + v * n) !=
        NGSLD_OK)
      error("ngsld_grid_get", ngsld_last_error(ctx));
  FILE *f = fopen(ga.out, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open LD grid output file!");
  fprintf(f, "chr\tbin1\tbin2\tn");
  print_summary_header(f, fields);
  for (uint64_t i = 0; i < n; ++i) {
    fprintf(f, "%s\t%lu\t%lu\t%lu", chr_name[chr[i]], (unsigned long)(b1[i] * B), (unsigned long)(b2[i] * B), (unsigned long)rows[i]);
    print_summaries(f, nf, n, i, rows[i], sum.data(), mean.data(), top.data(), linked.data());  // (a cell has rows)
  }
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD grid output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD grid: %lu cells (%lu bins, a band of %lu) from %lu of %lu pairs\n", (unsigned long)n, (unsigned long)st.bins,
            (unsigned long)st.band, (unsigned long)st.pairs_counted, (unsigned long)st.pairs);
}

// --cross_out: one line per cell with rows, by the bin of the pair's first site, then of its second (the bins numbered over the
// chromosomes in file order): both chromosomes, the lower breaks b * B of the two windows (0 without --cross_bin_size), the
// counted rows, then sum, mean, max and linked of every chosen statistic
void run_cross(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  CrossArgs &ca = cross;
  std::vector<const char *> lab(pars.n_sites);
  for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  ngsld_cross_ld_stats st{};
  st.struct_size = sizeof(st);
  if (ngsld_cross_ld(ctx, &ca.p, lab.data(), &st) != NGSLD_OK) error("ngsld_cross_ld", ngsld_last_error(ctx));
  const uint64_t n = st.cells, B = ca.p.bin_size;
  const std::vector<int> fields = fields_of(ca.p.fields);
  const size_t nf = fields.size();
  uint64_t n_chr = 0;
  if (ngsld_cross_ld_chromosomes(ctx, 0, nullptr, &n_chr) != NGSLD_OK) error("ngsld_cross_ld_chromosomes", ngsld_last_error(ctx));
  std::vector<const char *> chr_name(n_chr);
  if (ngsld_cross_ld_chromosomes(ctx, n_chr, chr_name.data(), nullptr) != NGSLD_OK)
    error("ngsld_cross_ld_chromosomes", ngsld_last_error(ctx));
  std::vector<uint32_t> chr1(n), chr2(n);
  std::vector<uint64_t> b1(n), b2(n), rows(n), linked(nf * n);
  std::vector<int64_t> sum(nf * n), top(nf * n);
  std::vector<double> mean(nf * n);
  if (ngsld_cross_ld_cells(ctx, n, chr1.data(), b1.data(), chr2.data(), b2.data(), rows.data(), nullptr) != NGSLD_OK)
    error("ngsld_cross_ld_cells", ngsld_last_error(ctx));
  for (size_t v = 0; v < nf; ++v)
    if (ngsld_cross_ld_get(ctx, 4 + fields[v], n, sum.data() + v * n, top.data() + v * n, linked.data() + v * n, mean.data() + v * n) !=
        NGSLD_OK)
      error("ngsld_cross_ld_get", ngsld_last_error(ctx));
  FILE *f = fopen(ca.out, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open LD across chromosomes output file!");
  fprintf(f, "chr1\tbin1\tchr2\tbin2\tn");
  print_summary_header(f, fields);
  for (uint64_t i = 0; i < n; ++i) {
    fprintf(f, "%s\t%lu\t%s\t%lu\t%lu", chr_name[chr1[i]], (unsigned long)(b1[i] * B), chr_name[chr2[i]], (unsigned long)(b2[i] * B),
            (unsigned long)rows[i]);
    print_summaries(f, nf, n, i, rows[i], sum.data(), mean.data(), top.data(), linked.data());  // (a cell has rows)
  }
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD across chromosomes output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD across chromosomes: %lu cells (%lu bins) from %lu of %lu pairs, %lu across chromosomes\n", (unsigned long)n,
            (unsigned long)st.bins, (unsigned long)st.pairs_counted, (unsigned long)st.pairs, (unsigned long)st.pairs_cross);
}

// --cluster_out: one line per site of the input, in file order, its cluster or NA; --cluster_table: one line per cluster of
// at least --cluster_min_size sites, in id order
ngsld_analysis stage_clusters(const Params &, const ngsld_pos *) {
  cluster.st = ngsld_clusters_stats{};
  cluster.st.struct_size = sizeof(cluster.st);
  return analysis_entry(NGSLD_AN_CLUSTERS, &cluster.p, &cluster.st);
}

void run_clusters(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_clusters(ctx, &cluster.p, &cluster.st) != NGSLD_OK) error("ngsld_clusters", ngsld_last_error(ctx));
}

void write_clusters(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  ClusterArgs &ca = cluster;
  const ngsld_clusters_stats &st = ca.st;
  const uint64_t n = pars.n_sites;
  if (ca.out) {
    std::vector<uint32_t> id(n);
    if (ngsld_clusters_sites(ctx, id.data()) != NGSLD_OK) error("ngsld_clusters_sites", ngsld_last_error(ctx));
    FILE *f = fopen(ca.out, "w");
    if (f == nullptr) error(__FUNCTION__, "cannot open LD clusters output file!");
    fprintf(f, "site\tcluster\n");
    for (uint64_t s = 0; s < n; ++s) {
      print_site(f, pos, s);
      if (id[s] == 0)
        fprintf(f, "\tNA\n");
      else
        fprintf(f, "\t%u\n", id[s]);
    }
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD clusters output file!");
  }
  if (ca.table) {
    uint64_t rows = 0;
    if (ngsld_clusters_table(ctx, ca.min_size_v, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             &rows) != NGSLD_OK)
      error("ngsld_clusters_table", ngsld_last_error(ctx));
    std::vector<uint32_t> id(rows), size(rows), first(rows), last(rows);
    std::vector<uint64_t> span(rows), edges(rows);
    std::vector<int64_t> sum(rows);
    std::vector<double> mean(rows), density(rows);
    if (ngsld_clusters_table(ctx, ca.min_size_v, rows, id.data(), size.data(), first.data(), last.data(), span.data(), edges.data(),
                             sum.data(), mean.data(), density.data(), nullptr) != NGSLD_OK)
      error("ngsld_clusters_table", ngsld_last_error(ctx));
    FILE *f = fopen(ca.table, "w");
    if (f == nullptr) error(__FUNCTION__, "cannot open LD clusters table file!");
    fprintf(f, "cluster\tsize\tfirst\tlast\tspan\tedges\tsum\tmean\tdensity\n");
    for (uint64_t k = 0; k < rows; ++k) {
      fprintf(f, "%u\t%u\t", id[k], size[k]);
      print_site(f, pos, first[k]);
      fprintf(f, "\t");
      print_site(f, pos, last[k]);
      fprintf(f, "\t%lu\t%lu", (unsigned long)span[k], (unsigned long)edges[k]);
      print_micro(f, sum[k]);
      if (std::isnan(mean[k]))
        fprintf(f, "\tNA");
      else
        fprintf(f, "\t%.17g", mean[k]);
      if (std::isnan(density[k]))
        fprintf(f, "\tNA\n");
      else
        fprintf(f, "\t%.17g\n", density[k]);
    }
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD clusters table file!");
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD clusters: %lu of %lu sites in %lu clusters (%lu of two sites or more, the largest of %lu), %lu edges of %lu pairs\n",
            (unsigned long)st.nodes, (unsigned long)n, (unsigned long)st.clusters, (unsigned long)st.clusters_multi,
            (unsigned long)st.largest, (unsigned long)st.edges, (unsigned long)st.pairs);
}

int write_linked_batch(void *user, const ngsld_linked_batch *b) {
  return fwrite(b->text, 1, b->text_len, static_cast<FILE *>(user)) == b->text_len ? 0 : 1;
}

// the rows of the table that pass the filter, as the table prints them; --linked_outH: under the table's header; a name ending
// in .gz is written gzip-compressed, as --out is
void run_linked(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  LinkedArgs &la = linked;
  const char *path = la.out ? la.out : la.outH;
  std::vector<const char *> lab;
  if (pos) {
    lab.resize(pars.n_sites);
    for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  }
  const size_t len = std::strlen(path);
  ngsld_gz *gz = nullptr;
  FILE *f = nullptr;
  if (len > 3 && std::strcmp(path + len - 3, ".gz") == 0) {
    int wfd = -1;
    if (ngsld_host_gz_open(path, (int)pars.n_threads, &gz, &wfd) != NGSLD_OK) error(__FUNCTION__, "cannot open linked pairs output file!");
    f = fdopen(wfd, "w");
  } else {
    f = fopen(path, "w");
  }
  if (f == nullptr) error(__FUNCTION__, "cannot open linked pairs output file!");
  if (la.outH) {
    char hdr[512];
    const size_t hn = ngsld_host_format_header(hdr, sizeof(hdr), pars.extend_out);
    if (fwrite(hdr, 1, hn, f) != hn) error(__FUNCTION__, "cannot write linked pairs output file!");
  }
  ngsld_linked_stats st{};
  st.struct_size = sizeof(st);
  const int rc = ngsld_linked_pairs(ctx, &la.p, pos ? lab.data() : nullptr, write_linked_batch, f, &st);
  if (rc > 0) error(__FUNCTION__, "cannot write linked pairs output file!");  // (the sink's own return value: the library's are negative)
  if (rc != NGSLD_OK) error("ngsld_linked_pairs", ngsld_last_error(ctx));
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write linked pairs output file!");
  if (gz != nullptr && ngsld_host_gz_close(gz) != NGSLD_OK) error(__FUNCTION__, "cannot write linked pairs output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> Linked pairs: %lu of %lu pairs (%lu bytes, %lu rows formatted on the host)\n", (unsigned long)st.rows,
            (unsigned long)st.pairs, (unsigned long)st.text_bytes, (unsigned long)st.host_rows);
}

// every query site's partners, one line each: site, rank from 1, partner, the value as the table prints it
void run_partners(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  PartnersArgs &pa = partners;
  const uint64_t n = pars.n_sites;
  std::vector<uint8_t> query;
  if (pa.sites_file) {  // the labels up to their first TAB, as print_site names a site; without --pos the 1-based index
    std::unordered_map<std::string, uint64_t> index;
    for (uint64_t s = 0; s < n; ++s) {
      if (pos) {
        const char *lab = ngsld_host_label(pos, s);
        index.emplace(std::string(lab, strcspn(lab, "\t")), s);
      } else {
        index.emplace(std::to_string(s + 1), s);
      }
    }
    query.assign(n, 0);
    for (const std::string &x : pa.sites) {
      const auto it = index.find(x.substr(0, x.find('\t')));
      if (it == index.end()) {
        const std::string msg = "--partners_sites names a site that is not in the data: " + x;
        error(__FUNCTION__, msg.c_str());
      }
      query[it->second] = 1;
    }
  }
  ngsld_partners_stats st{};
  st.struct_size = sizeof(st);
  if (ngsld_partners(ctx, &pa.p, pa.sites_file ? query.data() : nullptr, &st) != NGSLD_OK) error("ngsld_partners", ngsld_last_error(ctx));
  const uint32_t k = pa.p.k;
  std::vector<uint64_t> rows(n);
  std::vector<uint32_t> partner(n * k);
  std::vector<int64_t> value(n * k);
  if (ngsld_partners_get(ctx, rows.data(), partner.data(), value.data()) != NGSLD_OK) error("ngsld_partners_get", ngsld_last_error(ctx));
  FILE *f = fopen(pa.out, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open LD partners output file!");
  fprintf(f, "site\trank\tpartner\t%s\n", kDecayFields[pa.p.field - 4]);
  for (uint64_t s = 0; s < n; ++s)
    for (uint32_t j = 0; j < k && partner[s * k + j] != 0xffffffffu; ++j) {
      print_site(f, pos, s);
      fprintf(f, "\t%u\t", j + 1);
      print_site(f, pos, partner[s * k + j]);
      print_micro(f, value[s * k + j]);
      fprintf(f, "\n");
    }
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD partners output file!");
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD partners: %lu partners of %lu sites (up to %u each) from %lu partner rows of %lu pairs\n",
            (unsigned long)st.entries, (unsigned long)st.sites_with_partners, k, (unsigned long)st.rows_counted, (unsigned long)st.pairs);
}

// --tree_out: one line per merge, in rule order (the merge and size columns load as R's hclust$merge and the sizes); --tree_cut_out:
// one line per site of the input, in file order, its cluster at every floor of --tree_cut or NA
void run_tree(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  TreeArgs &ta = tree;
  const uint64_t n = pars.n_sites;
  ngsld_ld_tree_stats st{};
  st.struct_size = sizeof(st);
  if (ngsld_ld_tree(ctx, &ta.p, &st) != NGSLD_OK) error("ngsld_ld_tree", ngsld_last_error(ctx));
  if (ta.out) {
    const uint64_t rows = st.merges;
    std::vector<uint32_t> s1(rows), s2(rows), size(rows), first(rows), last(rows);
    std::vector<int64_t> q(rows), left(rows), right(rows);
    std::vector<uint64_t> dist(rows);
    if (ngsld_ld_tree_merges(ctx, rows, s1.data(), s2.data(), q.data(), dist.data(), left.data(), right.data(), size.data(), first.data(),
                             last.data(), nullptr) != NGSLD_OK)
      error("ngsld_ld_tree_merges", ngsld_last_error(ctx));
    FILE *f = fopen(ta.out, "w");
    if (f == nullptr) error(__FUNCTION__, "cannot open LD tree output file!");
    fprintf(f, "merge\tsite1\tsite2\tweight\tdist\tleft\tright\tsize\tfirst\tlast\n");
    for (uint64_t k = 0; k < rows; ++k) {
      fprintf(f, "%lu\t", (unsigned long)(k + 1));
      print_site(f, pos, s1[k]);
      fprintf(f, "\t");
      print_site(f, pos, s2[k]);
      print_micro(f, q[k]);
      fprintf(f, "\t%lu\t%ld\t%ld\t%u\t", (unsigned long)dist[k], (long)left[k], (long)right[k], size[k]);
      print_site(f, pos, first[k]);
      fprintf(f, "\t");
      print_site(f, pos, last[k]);
      fprintf(f, "\n");
    }
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD tree output file!");
  }
  if (ta.cut_out) {
    const size_t cuts = ta.cut_v.size();
    std::vector<uint32_t> id(cuts * n);
    for (size_t k = 0; k < cuts; ++k)
      if (ngsld_ld_tree_cut(ctx, ta.cut_v[k], id.data() + k * n, nullptr) != NGSLD_OK) error("ngsld_ld_tree_cut", ngsld_last_error(ctx));
    FILE *f = fopen(ta.cut_out, "w");
    if (f == nullptr) error(__FUNCTION__, "cannot open LD tree cuts output file!");
    fprintf(f, "site");
    for (const std::string &t : ta.cut_text) fprintf(f, "\t%s", t.c_str());
    fprintf(f, "\n");
    for (uint64_t s = 0; s < n; ++s) {
      print_site(f, pos, s);
      for (size_t k = 0; k < cuts; ++k) {
        if (id[k * n + s] == 0)
          fprintf(f, "\tNA");
        else
          fprintf(f, "\t%u", id[k * n + s]);
      }
      fprintf(f, "\n");
    }
    if (fclose(f) != 0) error(__FUNCTION__, "cannot write LD tree cuts output file!");
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD tree: %lu merges of %lu nodes (%lu clusters at the floor), %lu edges of %lu pairs, %lu rounds in %lu chunks\n",
            (unsigned long)st.merges, (unsigned long)st.nodes, (unsigned long)st.clusters, (unsigned long)st.edges, (unsigned long)st.pairs,
            (unsigned long)st.rounds, (unsigned long)st.chunks);
}

int write_blocks_text(void *user, const char *text, uint64_t len) {
  return fwrite(text, 1, len, static_cast<FILE *>(user)) == len ? 0 : 1;
}

void run_blocks(ngsld_ctx *ctx, const Params &pars, const ngsld_pos *pos) {
  BlocksArgs &ba = blocks;
  std::vector<const char *> lab(pars.n_sites);
  for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  ngsld_blocks_stats st{};
  st.struct_size = sizeof(st);
  if (ngsld_blocks(ctx, &ba.p, lab.data(), &st) != NGSLD_OK) error("ngsld_blocks", ngsld_last_error(ctx));
  if (st.sites == 0) error(__FUNCTION__, "no SNPs found in region.");
  for (int k = 0; k < 4; ++k) {
    if (!((ba.p.fields >> k) & 1u)) continue;
    const std::string path = std::string(ba.out) + "." + kDecayFields[k] + ".tsv";
    FILE *f = fopen(path.c_str(), "w");
    if (f == nullptr) error(__FUNCTION__, "cannot open LD blocks output file!");
    const int rc = ngsld_blocks_text(ctx, 4 + k, write_blocks_text, f, &st);
    if (rc == NGSLD_ERR_SINK || fclose(f) != 0) error(__FUNCTION__, "cannot write LD blocks output file!");
    if (rc != NGSLD_OK) error("ngsld_blocks_text", ngsld_last_error(ctx));
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> LD blocks: %lu sites, %lu pairs in region\n", (unsigned long)st.sites, (unsigned long)st.pairs_in_region);
}

// labels one per line, in site order; a name ending in .gz is written gzip-compressed
void write_labels(const char *path, const std::vector<const char *> &labels) {
  const size_t n = std::strlen(path);
  if (n > 3 && std::strcmp(path + n - 3, ".gz") == 0) {
    gzFile f = gzopen(path, "wb6");
    if (f == nullptr) error(__FUNCTION__, "cannot open pruning output file!");
    for (const char *l : labels)
      if (gzputs(f, l) < 0 || gzputc(f, '\n') < 0) error(__FUNCTION__, "cannot write pruning output file!");
    if (gzclose(f) != Z_OK) error(__FUNCTION__, "cannot write pruning output file!");
    return;
  }
  FILE *f = fopen(path, "w");
  if (f == nullptr) error(__FUNCTION__, "cannot open pruning output file!");
  for (const char *l : labels) fprintf(f, "%s\n", l);
  if (fclose(f) != 0) error(__FUNCTION__, "cannot write pruning output file!");
}

ngsld_analysis stage_prune(const Params &pars, const ngsld_pos *pos) {
  PruneArgs &pa = prune;
  std::vector<const char *> &lab = pa.lab, &sub = pa.sub;
  lab.assign(pars.n_sites, "(null)");
  if (pos)
    for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  sub.clear();
  for (const std::string &x : pa.subset) sub.push_back(x.c_str());
  if (pa.subset_file) {
    pa.p.subset = sub.data();
    pa.p.n_subset = sub.size();
  }
  static const char *const kEmpty[1] = {""};
  if (pa.subset_file && sub.empty()) pa.p.subset = kEmpty;  // (an empty subset: no site is a node)
  pa.state.assign(pars.n_sites, 0);
  pa.st = ngsld_prune_stats{};
  pa.st.struct_size = sizeof(pa.st);
  return analysis_entry(NGSLD_AN_PRUNE, &pa.p, &pa.st, lab.data(), pa.state.data());
}

void run_prune(ngsld_ctx *ctx, const Params &, const ngsld_pos *) {
  if (ngsld_prune(ctx, &prune.p, prune.lab.data(), prune.state.data(), &prune.st) != NGSLD_OK) error("ngsld_prune", ngsld_last_error(ctx));
}

void write_prune(ngsld_ctx *, const Params &pars, const ngsld_pos *) {
  PruneArgs &pa = prune;
  const ngsld_prune_stats &st = pa.st;
  const std::vector<const char *> &lab = pa.lab;
  const std::vector<uint8_t> &state = pa.state;
  std::vector<const char *> kept, excl;
  for (uint64_t s = 0; s < pars.n_sites; s++) {
    if (state[s] == 1) kept.push_back(lab[s]);
    if (state[s] == 2) excl.push_back(lab[s]);
  }
  write_labels(pa.out, kept);
  if (pa.excl) write_labels(pa.excl, excl);
  if (pars.verbose >= 1)
    fprintf(stderr, "==> Pruning: %lu nodes, %lu edges: %lu kept, %lu excluded (%lu rounds on the device, %lu nodes finished on the host)\n",
            (unsigned long)st.nodes, (unsigned long)st.edges, (unsigned long)st.kept, (unsigned long)st.excluded,
            (unsigned long)st.rounds, (unsigned long)st.host_nodes);
}

// ---- the analysis families, in the order they are taken out of argv, checked and run ----
struct Family {
  const char *prefix;  // of its flags, without the dashes; prefix + "out" names the family in the refusals
  struct Valued {
    const char *name;
    const char **dst;
  };
  Valued valued[12];           // "--name value" or "--name=value"; a null name ends the list
  const char *switch_name;     // a flag without a value (may be null) ...
  bool *switch_on;             // ... and where it goes
  bool *given;                 // any flag of the family
  void (*check)(const Params &);  // once the reference's own arguments have been checked; only when given
  // stage (what the call reads and fills, as an entry of ngsld_analyze's list), run (the single call), write (the files).  A
  // family without a stage is a call of its own whatever else is asked for, and writes in run.
  ngsld_analysis (*stage)(const Params &, const ngsld_pos *);
  void (*run)(ngsld_ctx *, const Params &, const ngsld_pos *);
  void (*write)(ngsld_ctx *, const Params &, const ngsld_pos *);
  const char *timing;          // its line of the NGSLD_TIMING report
  const char *switch2_name = nullptr;  // a second flag without a value (--cross_only) ...
  bool *switch2_on = nullptr;          // ... and where it goes
};
const Family kFamilies[] = {
    {"prune_",
     {{"prune_out", &prune.out}, {"prune_excl", &prune.excl}, {"prune_subset", &prune.subset_file}, {"prune_field", &prune.field},
      {"prune_weight_type", &prune.type}, {"prune_precision", &prune.precision}, {"prune_max_kb_dist", &prune.max_kb_dist},
      {"prune_min_weight", &prune.min_weight}},
     "prune_keep_heavy", &prune.keep_heavy, &prune.given, check_prune_args, stage_prune, run_prune, write_prune, "pruning"},  // (with one more of the six analyses: one run of the pair kernels for them all)
    {"decay_",
     {{"decay_out", &decay.out}, {"decay_fit", &decay.fit}, {"decay_ld", &decay.ld}, {"decay_bin_size", &decay.bin_size},
      {"decay_max_kb_dist", &decay.max_kb_dist}, {"decay_min_maf", &decay.min_maf}, {"decay_n_ind", &decay.n_ind},
      {"decay_recomb_rate", &decay.recomb_rate}},
     nullptr, nullptr, &decay.given, check_decay_args, stage_decay, run_decay, write_decay, "LD decay"},
    {"blocks_",
     {{"blocks_out", &blocks.out}, {"blocks_chr", &blocks.chr}, {"blocks_start", &blocks.start}, {"blocks_end", &blocks.end},
      {"blocks_ld", &blocks.ld}},
     nullptr, nullptr, &blocks.given, check_blocks_args, nullptr, run_blocks, nullptr, "LD blocks"},  // (a pass of the pair kernels over the region's rows)
    {"site_",
     {{"site_out", &site.out}, {"site_ld", &site.ld}, {"site_max_kb_dist", &site.max_kb_dist}, {"site_min_maf", &site.min_maf},
      {"site_linked_min", &site.linked_min}},
     "site_signed", &site.is_signed, &site.given, check_site_args, stage_site, run_site, write_site, "site LD"},
    {"cluster_",
     {{"cluster_out", &cluster.out}, {"cluster_table", &cluster.table}, {"cluster_field", &cluster.field},
      {"cluster_min_weight", &cluster.min_weight}, {"cluster_max_kb_dist", &cluster.max_kb_dist}, {"cluster_min_maf", &cluster.min_maf},
      {"cluster_min_size", &cluster.min_size}},
     "cluster_signed", &cluster.is_signed, &cluster.given, check_cluster_args, stage_clusters, run_clusters, write_clusters, "LD clusters"},
    {"grid_",
     {{"grid_out", &grid.out}, {"grid_bin_size", &grid.bin_size}, {"grid_ld", &grid.ld}, {"grid_max_kb_dist", &grid.max_kb_dist},
      {"grid_min_maf", &grid.min_maf}, {"grid_linked_min", &grid.linked_min}},
     "grid_signed", &grid.is_signed, &grid.given, check_grid_args, stage_grid, run_grid, write_grid, "LD grid"},
    {"linked_",
     {{"linked_out", &linked.out}, {"linked_outH", &linked.outH}, {"linked_field", &linked.field},
      {"linked_min_weight", &linked.min_weight}, {"linked_max_kb_dist", &linked.max_kb_dist}, {"linked_min_maf", &linked.min_maf}},
     "linked_signed", &linked.is_signed, &linked.given, check_linked_args, nullptr, run_linked, nullptr, "linked pairs"},  // (a pass of the pair kernels of its own: the 40 B records, a sink)
    {"scan_",
     {{"scan_out", &scan.out}, {"scan_half_window", &scan.half_window}, {"scan_ld", &scan.ld}, {"scan_max_kb_dist", &scan.max_kb_dist},
      {"scan_min_maf", &scan.min_maf}},
     nullptr, nullptr, &scan.given, check_scan_args, stage_scan, run_scan, write_scan, "LD scan"},
    {"partners_",
     {{"partners_out", &partners.out}, {"partners_k", &partners.k}, {"partners_field", &partners.field},
      {"partners_min_weight", &partners.min_weight}, {"partners_max_kb_dist", &partners.max_kb_dist},
      {"partners_min_maf", &partners.min_maf}, {"partners_sites", &partners.sites_file}},
     "partners_signed", &partners.is_signed, &partners.given, check_partners_args, nullptr, run_partners, nullptr, "LD partners"},  // (a pass of the pair kernels of its own: lists that persist across its chunks)
    {"dmap_",  // (not "decay_map_": a family is matched by its prefix, and decay_ would take those flags)
     {{"dmap_out", &dmap.out}, {"dmap_fit", &dmap.fit}, {"dmap_window", &dmap.window}, {"dmap_ld", &dmap.ld},
      {"dmap_bin_size", &dmap.bin_size}, {"dmap_max_kb_dist", &dmap.max_kb_dist}, {"dmap_min_maf", &dmap.min_maf},
      {"dmap_n_ind", &dmap.n_ind}, {"dmap_recomb_rate", &dmap.recomb_rate}, {"dmap_fit_min_bins", &dmap.fit_min_bins}},
     nullptr, nullptr, &dmap.given, check_dmap_args, nullptr, run_dmap, nullptr, "LD decay map"},  // (a pass of the pair kernels of its own: it is no kind of ngsld_analyze)
    {"cross_",
     {{"cross_out", &cross.out}, {"cross_bin_size", &cross.bin_size}, {"cross_ld", &cross.ld}, {"cross_min_maf", &cross.min_maf},
      {"cross_linked_min", &cross.linked_min}, {"cross_min_kb_dist", &cross.min_kb_dist}},
     "cross_signed", &cross.is_signed, &cross.given, check_cross_args, nullptr, run_cross, nullptr, "LD across chromosomes",
     "cross_only", &cross.only},  // (a pass of the pair kernels of its own, as the decay map)
    {"tree_",
     {{"tree_out", &tree.out}, {"tree_field", &tree.field}, {"tree_min_weight", &tree.min_weight}, {"tree_max_kb_dist", &tree.max_kb_dist},
      {"tree_min_maf", &tree.min_maf}, {"tree_cut", &tree.cut}, {"tree_cut_out", &tree.cut_out}},
     "tree_signed", &tree.is_signed, &tree.given, check_tree_args, nullptr, run_tree, nullptr, "LD tree"},  // (a pass of the pair kernels of its own: a forest that persists across its chunks)
};

// Takes a family's flags (one or two dashes) out of argv.  The values are checked once the reference's own arguments have been.
void take_flags(int *argc, char **argv, const Family &fam) {
  const size_t plen = std::strlen(fam.prefix);
  int w = 1;
  for (int i = 1; i < *argc; ++i) {
    const char *a = argv[i];
    if (std::strcmp(a, "--") == 0) {  // (getopt's end of options: the rest is not ours)
      while (i < *argc) argv[w++] = argv[i++];
      break;
    }
    const char *name = a[0] == '-' ? (a[1] == '-' ? a + 2 : a + 1) : nullptr;
    if (name == nullptr || std::strncmp(name, fam.prefix, plen) != 0) {
      argv[w++] = argv[i];
      continue;
    }
    const char *eq = std::strchr(name, '=');
    const std::string key = eq ? std::string(name, eq) : std::string(name);
    *fam.given = true;
    if (fam.switch_name != nullptr && key == fam.switch_name && eq == nullptr) {
      *fam.switch_on = true;
      continue;
    }
    if (fam.switch2_name != nullptr && key == fam.switch2_name && eq == nullptr) {
      *fam.switch2_on = true;
      continue;
    }
    bool known = false;
    for (const Family::Valued *v = fam.valued; v->name != nullptr; ++v) {
      if (key != v->name) continue;
      known = true;
      if (eq != nullptr) {
        *v->dst = eq + 1;
      } else if (i + 1 < *argc) {
        *v->dst = argv[++i];
      } else {
        const std::string msg = "--" + key + " needs a value!";
        error(__FUNCTION__, msg.c_str());
      }
    }
    if (!known) {
      const std::string msg = "unknown option --" + key + "!";
      error(__FUNCTION__, msg.c_str());
    }
  }
  argv[w] = nullptr;
  *argc = w;
}

void parse_cmd_args(Params *pars, int argc, char **argv) {
  static struct option long_options[] = {{"geno", required_argument, NULL, 'g'},
                                         {"probs", no_argument, NULL, 'p'},
                                         {"log_scale", no_argument, NULL, 'l'},
                                         {"n_ind", required_argument, NULL, 'n'},
                                         {"n_sites", required_argument, NULL, 's'},
                                         {"pos", required_argument, NULL, 'a'},
                                         {"posH", required_argument, NULL, 'A'},
                                         {"max_kb_dist", required_argument, NULL, 'd'},
                                         {"max_snp_dist", required_argument, NULL, 'D'},
                                         {"min_maf", required_argument, NULL, 'f'},
                                         {"ignore_miss_data", no_argument, NULL, 'm'},
                                         {"call_geno", no_argument, NULL, 'c'},
                                         {"N_thresh", required_argument, NULL, 'N'},
                                         {"call_thresh", required_argument, NULL, 'C'},
                                         {"rnd_sample", required_argument, NULL, 'r'},
                                         {"seed", required_argument, NULL, 'S'},
                                         {"extend_out", no_argument, NULL, 'x'},
                                         {"out", required_argument, NULL, 'o'},
                                         {"outH", required_argument, NULL, 'O'},
                                         {"n_threads", required_argument, NULL, 't'},
                                         {"verbose", required_argument, NULL, 'V'},
                                         {"device", required_argument, NULL, 1001},
                                         {"max_gpu_mem", required_argument, NULL, 1002},
                                         {"devices", required_argument, NULL, 1003},
                                         {"keep_parts", no_argument, NULL, 1004},
                                         {0, 0, 0, 0}};
  pars->seed = (uint64_t)(time(NULL) + rand() % 1000);  // parse_args.cpp:23
  int c = 0;
  while ((c = getopt_long_only(argc, argv, "g:pln:s:Z:d:D:f:mcN:C:r:S:xo:t:V:", long_options, NULL)) != -1)
    switch (c) {
      case 'g': pars->in_geno = optarg; break;
      case 'p': pars->in_probs = true; break;
      case 'l': pars->in_logscale = true; pars->in_probs = true; break;
      case 'n': pars->n_ind = (uint64_t)atoi(optarg); break;
      case 's': pars->n_sites = (uint64_t)atoi(optarg); break;
      case 'a': pars->in_pos = optarg; pars->in_pos_header = false; break;
      case 'A': pars->in_pos = optarg; pars->in_pos_header = true; break;
      case 'd': pars->max_kb_dist = (uint64_t)atoi(optarg); break;
      case 'D': pars->max_snp_dist = (uint64_t)atoi(optarg); break;
      case 'f': pars->min_maf = atof(optarg); break;
      case 'm': pars->ignore_miss_data = true; break;
      case 'c': pars->call_geno = true; break;
      case 'N': pars->N_thresh = atof(optarg); pars->call_geno = true; break;
      case 'C': pars->call_thresh = atof(optarg); pars->call_geno = true; break;
      case 'r': pars->rnd_sample = atof(optarg); break;
      case 'S': pars->seed = (uint64_t)atoi(optarg); break;
      case 'x': pars->extend_out = true; break;
      case 'o': pars->out = optarg; break;
      case 't': pars->n_threads = (unsigned)atoi(optarg); break;
      case 'V': pars->verbose = (unsigned)atoi(optarg); break;
      case 1001: pars->device = atoi(optarg); break;
      case 1002: pars->max_gpu_mem = atof(optarg); break;
      case 1004: pars->keep_parts = true; break;
      case 1003:
        pars->devices = parse_devices(optarg);
        if (pars->devices.empty()) error(__FUNCTION__, "--devices takes a list like 0-7 or 0,2,5");
        pars->device = pars->devices[0];
        break;
      default: exit(-1);  // unknown flags and --outH (declared, no case: parse_args.cpp:55,130)
    }

  if (pars->verbose >= 1) {  // parse_args.cpp:135-159
    fprintf(stderr, "==> Input Arguments:\n");
    fprintf(stderr,
            "\tgeno: %s\n\tprobs: %s\n\tlog_scale: %s\n\tn_ind: %lu\n\tn_sites: %lu\n\tpos: %s (%s header)\n\t"
            "max_kb_dist (kb): %lu\n\tmax_snp_dist: %lu\n\tmin_maf: %f\n\tignore_miss_data: %s\n\tcall_geno: %s\n\t"
            "N_thresh: %f\n\tcall_thresh: %f\n\trnd_sample: %f\n\tseed: %lu\n\textend_out: %s\n\tout: %s\n\t"
            "n_threads: %d\n\tverbose: %d\n\tversion: %s (%s @ %s)\n\n",
            pars->in_geno, pars->in_probs ? "true" : "false", pars->in_logscale ? "true" : "false",
            (unsigned long)pars->n_ind, (unsigned long)pars->n_sites, pars->in_pos,
            pars->in_pos_header ? "WITH" : "WITHOUT", (unsigned long)pars->max_kb_dist,
            (unsigned long)pars->max_snp_dist, pars->min_maf, pars->ignore_miss_data ? "true" : "false",
            pars->call_geno ? "true" : "false", pars->N_thresh, pars->call_thresh, pars->rnd_sample,
            (unsigned long)pars->seed, pars->extend_out ? "true" : "false", pars->out, pars->n_threads,
            pars->verbose, kVersion, __DATE__, __TIME__);
  }
  if (pars->verbose > 4)
    fprintf(stderr,
            "==> Verbose values greater than 4 for debugging purpose only. Expect large amounts of info on screen\n");

  // parse_args.cpp:168-183
  if (pars->in_geno == NULL) error(__FUNCTION__, "genotype input file (--geno) missing!");
  if (pars->n_ind == 0) error(__FUNCTION__, "number of individuals (--n_ind) missing!");
  if (pars->n_sites == 0) error(__FUNCTION__, "number of sites (--n_sites) missing!");
  if (pars->in_pos == NULL && pars->max_kb_dist > 0)
    error(__FUNCTION__, "position file necessary in order to filter by maximum distance!");
  if (pars->min_maf < 0 || pars->min_maf > 1) error(__FUNCTION__, "minimum allele frequency must be in [0,1]!");
  if (pars->call_geno && !pars->in_probs)
    error(__FUNCTION__, "can only call genotypes from likelihoods/probabilities!");
  if (pars->rnd_sample <= 0 || pars->rnd_sample > 1)
    error(__FUNCTION__, "proportion of comparisons to sample must be in ]0,1]!");
  if (pars->n_threads < 1) error(__FUNCTION__, "number of threads cannot be less than 1!");
  // (n_threads is unsigned in the reference too, ngsLD.hpp:33: a negative value passes the test above as 4 billion and
  // its thread pool then fails to start; here it would only ask for that many formatter threads)
  if (pars->n_threads > 4096) pars->n_threads = 4096;
  // --keep_parts (new here): <out>, <out>.part1, ... in this order are the table.  Part 0 of a compressed output would be a gzip
  // member and the others plain text -- their concatenation neither a gzip stream nor a table -- so the two do not combine;
  // and without --out or with a single device there are no part files to keep: said, not silently ignored
  if (pars->keep_parts) {
    const char *dot = pars->out ? strrchr(pars->out, '.') : NULL;
    if (dot != NULL && strcmp(dot, ".gz") == 0) error(__FUNCTION__, "--keep_parts cannot be combined with a compressed output (--out *.gz)!");
    if (pars->out == NULL || pars->devices.size() < 2)
      fprintf(stderr, "WARN: --keep_parts has no effect without --out and --devices with two or more devices\n");
  }
}

ngsld_gz *g_gz = nullptr;     // --out *.gz: the compressor behind pars.out_fh
FILE *g_gz_fh = nullptr;      // ... and the stream over the compressor's pipe (owns the pipe's write descriptor)
// Ends the compressed file: the stream first (what stdio still buffers goes into the pipe, and the pipe's write end is
// closed exactly once, by its owner), then the compressor.  Registered with atexit, so that error() exits end the file
// too -- atexit handlers run BEFORE stdio flushes its streams, hence the explicit fclose here.
void finish_gz() {
  if (g_gz_fh != nullptr) {
    FILE *fh = g_gz_fh;
    g_gz_fh = nullptr;
    fclose(fh);
  }
  if (g_gz != nullptr) {
    ngsld_gz *g = g_gz;
    g_gz = nullptr;
    if (ngsld_host_gz_close(g) != NGSLD_OK) fprintf(stderr, "\nERROR: the compressed output is incomplete\n");
  }
}
// fclose(pars.out_fh) for every path out of main
void close_output(FILE *fh) {
  if (fh != nullptr && fh == g_gz_fh)
    finish_gz();
  else if (fh != nullptr)
    fclose(fh);
}

struct SinkState {
  const Params *pars;
  const ngsld_pos *pos;    // may be NULL (no --pos)
  const double *pos_dist;  // NULL => all INFINITY
  const std::vector<double> *maf;
};

// One batch, in (s1, s2) order: --n_threads threads format (the reference's threads each fprintf under a mutex,
// ngsLD.cpp:310-352), one ordered write.
double g_sink_seconds = 0.0;  // NGSLD_TIMING=1: time spent formatting + writing, reported at exit
uint64_t g_sink_batches = 0;

int write_batch(void *user, const ngsld_batch *b) {
  SinkState *st = static_cast<SinkState *>(user);
  const auto t0 = std::chrono::steady_clock::now();
  fflush(st->pars->out_fh);
  int rc = 0;
  if (b->text != nullptr) {  // rows formatted on the device (ngsld_set_text_output): only bytes to write
    const char *q = b->text;
    uint64_t left = b->text_len;
    const int fd = fileno(st->pars->out_fh);
    while (left && rc == 0) {
      const ssize_t w = ::write(fd, q, left > (1ull << 30) ? (size_t)(1ull << 30) : (size_t)left);
      if (w <= 0) rc = 1;
      else { q += w; left -= (uint64_t)w; }
    }
  } else {
    rc = ngsld_host_write_batch(b, st->pos, st->pos_dist, st->maf->data(), (int)st->pars->n_threads,
                                fileno(st->pars->out_fh)) == NGSLD_OK ? 0 : 1;
  }
  g_sink_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  ++g_sink_batches;
  return rc;
}

struct TimingReport {  // NGSLD_TIMING=1: wall time since start, per phase, and the sink's share, on stderr
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  bool on = getenv("NGSLD_TIMING") && strcmp(getenv("NGSLD_TIMING"), "1") == 0;
  void mark(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[timing] %-28s %.3f s\n", what, std::chrono::duration<double>(now - last).count());
    last = now;
  }
  bool printed = false;
  void print() {
    if (on && !printed)
      fprintf(stderr, "[timing] total %.3f s, TSV formatting + write %.3f s in %lu batches\n",
              std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), g_sink_seconds,
              (unsigned long)g_sink_batches);
    printed = true;
  }
  ~TimingReport() { print(); }
};


// (the genotype matrix in host memory: host_buf.h -- malloc semantics, huge pages)
double *alloc_matrix(size_t bytes) { return ngsld::alloc_host_matrix(bytes / sizeof(double)); }

struct ReadState {
  const Params *pars;
  char err[512];
};

int read_slab(void *user, uint64_t site_begin, uint64_t n_sites, double *dst) {
  ReadState *r = static_cast<ReadState *>(user);
  return ngsld_host_read_geno_bin_range(r->pars->in_geno, r->pars->n_ind, site_begin, n_sites, dst, r->err,
                                        sizeof(r->err)) == NGSLD_OK ? 0 : 1;
}

void fill_run_params(const Params &pars, ngsld_params *lp, ngsld_geno_opts *go) {
  lp->max_kb_dist = pars.max_kb_dist;
  lp->max_snp_dist = pars.max_snp_dist;
  lp->min_maf = pars.min_maf;
  lp->ignore_miss_data = pars.ignore_miss_data ? 1 : 0;
  lp->extend_out = pars.extend_out ? 1 : 0;
  lp->rnd_sample = pars.rnd_sample;
  lp->seed = pars.seed;
  lp->first_row = 0;
  memset(go, 0, sizeof(*go));
  go->log_scale = pars.in_logscale ? 1 : 0;
  go->ignore_miss_data = pars.ignore_miss_data ? 1 : 0;
  go->call_geno = pars.call_geno ? 1 : 0;
  go->N_thresh = pars.N_thresh;
  go->call_thresh = pars.call_thresh;
}

// The out-of-core path (no counterpart in the reference): the same TSV, the matrix read slab by slab.
// Returns false (nothing written yet) when may_fall_back and the slabs cannot hold a window.
// NGSLD_HOST_TEXT=1: every row through the host formatter (the fallback of the device-side TSV; A/B, tests)
static bool host_text_only() {
  static const bool on = getenv("NGSLD_HOST_TEXT") && strcmp(getenv("NGSLD_HOST_TEXT"), "1") == 0;
  return on;
}

bool run_streamed(Params &pars, uint64_t slab_sites, bool may_fall_back) {
  char err[512];
  ngsld_pos *pos = nullptr;
  if (pars.verbose >= 1) fprintf(stderr, "==> Getting sites coordinates\n");
  if (pars.in_pos &&
      ngsld_host_read_pos(pars.in_pos, pars.in_pos_header ? 1 : 0, pars.n_sites, &pos, err, sizeof(err)) != NGSLD_OK)
    error(pos_error_function(err, pars.in_pos), err);
  ngsld_params lp;
  ngsld_geno_opts go;
  fill_run_params(pars, &lp, &go);
  std::vector<double> maf(pars.n_sites);
  SinkState sink;
  sink.pars = &pars;
  sink.pos = pos;
  sink.pos_dist = pos ? ngsld_host_pos_dist(pos) : nullptr;
  sink.maf = &maf;
  ReadState rs;
  rs.pars = &pars;
  rs.err[0] = 0;
  uint64_t n_pairs = 0, n_slabs = 0;
  if (may_fall_back) {
    std::vector<ngsld_slab> probe(pars.n_sites);
    uint64_t n = 0;
    if (ngsld_plan_slabs(sink.pos_dist, pars.n_sites, &lp, slab_sites, probe.data(), probe.size(), &n) != NGSLD_OK) {
      ngsld_host_free_pos(pos);
      return false;
    }
  }
  if (pars.verbose >= 1)
    fprintf(stderr, "==> Streaming the genotype matrix in slabs of up to %lu sites\n", (unsigned long)slab_sites);
  const bool dev_text = !host_text_only();
  std::vector<const char *> lab;
  if (pos && dev_text) {
    lab.resize(pars.n_sites);
    for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  }
  const int rc = ngsld_run_streamed_text(pars.device, pars.n_sites, pars.n_ind, sink.pos_dist, &lp, &go, slab_sites,
                                         read_slab, &rs, maf.data(), write_batch, &sink, &n_pairs, &n_slabs, err,
                                         sizeof(err), pos && dev_text ? lab.data() : nullptr, dev_text ? 1 : 0);
  if (rc == NGSLD_ERR_NAN) error("read_geno", err);
  if (rc == NGSLD_ERR_MAF_RANGE) error("haplo_freq", err);
  if (rc != NGSLD_OK) error("ngsld_run_streamed", rs.err[0] ? rs.err : err);
  if (pars.verbose >= 2) {  // (as the resident run's line, + where: a large host share means no room for the slabs' exact stores)
    ngsld_replay_stats_t st;
    if (ngsld_streamed_replay_info(&st) == NGSLD_OK)
      fprintf(stderr, "==> %lu of %lu pairs replayed in the reference's operation order (%lu on the device, %lu on host threads)\n",
              (unsigned long)st.pairs_replayed, (unsigned long)n_pairs, (unsigned long)st.pairs_on_device, (unsigned long)st.pairs_on_host);
  }
  if (pars.verbose >= 1) fprintf(stderr, "==> Freeing memory...\n");
  close_output(pars.out_fh);
  ngsld_host_free_pos(pos);
  if (pars.verbose >= 1) fprintf(stderr, "Done!\n");
  return true;
}

// ---- several devices, one process (ngsld_run_multi): part 0 writes straight to the output, the other parts spool their
// rows to <out>.part<k> (a temporary file when the output is stdout) and are appended in order at the end ----
struct MultiSink {
  const Params *pars;
  const ngsld_pos *pos;
  const double *pos_dist;
  const double *maf;
  std::vector<FILE *> fh;  // one per part
  int n_threads;           // formatter threads per part
};

int write_part_batch(void *user, int part, const ngsld_batch *b) {
  MultiSink *m = static_cast<MultiSink *>(user);
  FILE *fh = m->fh[(size_t)part];
  fflush(fh);
  const int fd = fileno(fh);
  if (b->text != nullptr) {
    const char *q = b->text;
    uint64_t left = b->text_len;
    while (left) {
      const ssize_t w = ::write(fd, q, left > (1ull << 30) ? (size_t)(1ull << 30) : (size_t)left);
      if (w <= 0) return 1;
      q += w;
      left -= (uint64_t)w;
    }
    return 0;
  }
  return ngsld_host_write_batch(b, m->pos, m->pos_dist, m->maf, m->n_threads, fd) == NGSLD_OK ? 0 : 1;
}

void run_multi(Params &pars, const double *raw, int text_semantics, int log_scale) {
  char err[512];
  const int n = (int)pars.devices.size();
  ngsld_pos *pos = nullptr;
  if (pars.verbose >= 1) fprintf(stderr, "==> Getting sites coordinates\n");
  if (pars.in_pos &&
      ngsld_host_read_pos(pars.in_pos, pars.in_pos_header ? 1 : 0, pars.n_sites, &pos, err, sizeof(err)) != NGSLD_OK)
    error(pos_error_function(err, pars.in_pos), err);
  ngsld_params lp;
  ngsld_geno_opts go;
  fill_run_params(pars, &lp, &go);
  go.text_semantics = text_semantics;
  go.log_scale = log_scale;
  std::vector<double> maf(pars.n_sites);
  MultiSink ms;
  ms.pars = &pars;
  ms.pos = pos;
  ms.pos_dist = pos ? ngsld_host_pos_dist(pos) : nullptr;
  ms.maf = maf.data();
  ms.n_threads = (int)std::max<unsigned>(1u, pars.n_threads / (unsigned)n);
  std::vector<std::string> part_names((size_t)n);
  ms.fh.assign((size_t)n, nullptr);
  ms.fh[0] = pars.out_fh;
  for (int k = 1; k < n; ++k) {
    if (pars.out != NULL) {
      part_names[(size_t)k] = std::string(pars.out) + ".part" + std::to_string(k);
      ms.fh[(size_t)k] = fopen(part_names[(size_t)k].c_str(), "w+");
    } else {
      ms.fh[(size_t)k] = tmpfile();
    }
    if (ms.fh[(size_t)k] == nullptr) error(__FUNCTION__, "cannot open a part file next to the output");
  }
  ReadState rs;
  rs.pars = &pars;
  rs.err[0] = 0;
  const bool dev_text = !host_text_only();
  std::vector<const char *> lab;
  if (pos && dev_text) {
    lab.resize(pars.n_sites);
    for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
  }
  if (pars.verbose >= 1) fprintf(stderr, "==> Launching %d device threads...\n", n);
  std::vector<uint64_t> per((size_t)n, 0);
  const int rc = ngsld_run_multi(pars.devices.data(), n, pars.n_sites, pars.n_ind, ms.pos_dist, &lp, &go, raw,
                                 raw ? nullptr : read_slab, raw ? nullptr : &rs, maf.data(), write_part_batch, &ms,
                                 pos && dev_text ? lab.data() : nullptr, dev_text ? 1 : 0, per.data(), err, sizeof(err));
  if (rc == NGSLD_ERR_NAN) error("read_geno", err);
  if (rc == NGSLD_ERR_MAF_RANGE) error("haplo_freq", err);
  if (rc != NGSLD_OK) error("ngsld_run_multi", rs.err[0] ? rs.err : err);
  if (pars.verbose >= 2)
    for (int k = 0; k < n; ++k)
      fprintf(stderr, "\tdevice %d: %lu pairs\n", pars.devices[(size_t)k], (unsigned long)per[(size_t)k]);
  // append the spooled parts in order -- inside the kernel where the file systems allow it (copy_file_range: no trip of the
  // bytes through this process), through a buffer otherwise.  --keep_parts (with --out): the parts stay where they are,
  // <out> + <out>.part1 + ... in this order is the table (a shard per device is as good as a merged file, and at
  // 10^9 rows the merge is a second pass over seven eighths of the output)
  fflush(pars.out_fh);
  std::vector<char> buf;
  for (int k = 1; k < n; ++k) {
    FILE *fh = ms.fh[(size_t)k];
    fflush(fh);
    if (pars.keep_parts && !part_names[(size_t)k].empty()) {
      if (fclose(fh) != 0) error(__FUNCTION__, "cannot finish a part file");
      continue;
    }
    const off_t size = lseek(fileno(fh), 0, SEEK_END);
    off_t done = 0;
    while (size > 0 && done < size) {  // (the output's own position is at its end: it has only ever been appended to)
      off_t in_off = done;
      const ssize_t w = copy_file_range(fileno(fh), &in_off, fileno(pars.out_fh), nullptr, (size_t)std::min<off_t>(size - done, (off_t)1 << 30), 0);
      if (w <= 0) break;  // (a pipe, /dev/null, another file system on an old kernel: the buffered copy below takes over)
      done += w;
    }
    if (done < size) {
      if (buf.empty()) buf.resize(8u << 20);
      if (fseeko(fh, done, SEEK_SET) != 0) error(__FUNCTION__, "cannot re-read a part file");
      size_t got;
      while ((got = fread(buf.data(), 1, buf.size(), fh)) > 0)
        if (fwrite(buf.data(), 1, got, pars.out_fh) != got) error(__FUNCTION__, "cannot append a part to the output");
      fflush(pars.out_fh);
    }
    fclose(fh);
    if (!part_names[(size_t)k].empty()) unlink(part_names[(size_t)k].c_str());
  }
  if (pars.verbose >= 1) fprintf(stderr, "==> Freeing memory...\n");
  close_output(pars.out_fh);
  ngsld_host_free_pos(pos);
  if (pars.verbose >= 1) fprintf(stderr, "Done!\n");
}

}  // namespace

int main(int argc, char **argv) {
  TimingReport timing_report;
  // This program's pinned host buffers are registered anonymous memory rather than hipHostMalloc memory (engine.hip, PinBuf):
  // 4x cheaper to get and to give back -- 0.07 s of a one-second run of configs[2], 3 s of configs[4] at full size.  The
  // library leaves that off by default (in a long-lived process that forks children it cost a GPU memory fault before the
  // mapping became fork-proof); this process is short-lived, single-purpose and never forks.  NGSLD_PIN_REGISTER=0 turns it off.
  setenv("NGSLD_PIN_REGISTER", "1", /*overwrite=*/0);
  Params pars;
  for (const Family &fam : kFamilies) take_flags(&argc, argv, fam);
  parse_cmd_args(&pars, argc, argv);
  bool any_family = false;
  for (const Family &fam : kFamilies)
    if (*fam.given) {
      any_family = true;
      fam.check(pars);
    }
  // --prune_out / --decay_out / --blocks_out / --site_out / --cluster_out / --cluster_table / --grid_out / --linked_out / --scan_out / --partners_out / --dmap_out / --cross_out / --tree_out without --out: no TSV
  const bool write_tsv = !any_family || pars.out != NULL;

  // ---- check input files (ngsLD.cpp:41-57) ----
  struct stat st;
  if (stat(pars.in_geno, &st) != 0) error(__FUNCTION__, "cannot check GENO file size!");
  const char *dot = strrchr(pars.in_geno, '.');  // the reference dereferences NULL for a name without '.' (ngsLD.cpp:45)
  if (dot != NULL && strcmp(dot, ".gz") == 0) {
    if (pars.verbose >= 1) fprintf(stderr, "==> GZIP input file (not BINARY)\n");
    pars.in_bin = false;
  } else {
    if (pars.verbose >= 1) fprintf(stderr, "==> BINARY input file (always lkl)\n");
    pars.in_bin = true;
    pars.in_probs = true;
    if (!ngsld_host_geno_size_ok((uint64_t)st.st_size, pars.n_ind, pars.n_sites))
      error(__FUNCTION__, "invalid/corrupt genotype input file!");
  }
  // ---- prepare output (ngsLD.cpp:73-77): the header is always written ----
  // (new: an --out name ending in .gz is written gzip-compressed, --n_threads deflate workers; the reference has no
  // compressed output)
  const char *odot = pars.out ? strrchr(pars.out, '.') : NULL;
  if (odot != NULL && strcmp(odot, ".gz") == 0) {
    int wfd = -1;
    if (ngsld_host_gz_open(pars.out, (int)pars.n_threads, &g_gz, &wfd) != NGSLD_OK)
      error(__FUNCTION__, "cannot open output file!");
    pars.out_fh = g_gz_fh = fdopen(wfd, "w");
    atexit(finish_gz);  // every path out of main (the streamed and the multi-device runs return early) ends the file
  } else if (pars.out != NULL) {
    pars.out_fh = fopen(pars.out, "w");
  }
  if (pars.out_fh == NULL) error(__FUNCTION__, "cannot open output file!");
  if (write_tsv) {
    char hdr[512];
    const size_t hn = ngsld_host_format_header(hdr, sizeof(hdr), pars.extend_out);
    fwrite(hdr, 1, hn, pars.out_fh);
    fflush(pars.out_fh);
  }

  ngsld_host_set_threads((int)pars.n_threads);
  timing_report.mark("arguments, output header");

  // A binary matrix that will plainly run resident (below the 4 GiB from which a windowed run is pipelined in slabs, and
  // well inside any --max_gpu_mem) is read -- and the positions after it -- by a thread of its own while the device context
  // comes up: the two take 0.15-0.35 s each and used to run one after the other.  Errors wait for the join and come out
  // where and as they always did.
  struct FreeDeleter {
    void operator()(double *q) const { free(q); }
  };
  struct EarlyRead {
    std::thread th;
    bool started = false, pos_done = false;
    int geno_rc = NGSLD_OK, pos_rc = NGSLD_OK;
    char geno_err[512] = "", pos_err[512] = "";
    std::unique_ptr<double, FreeDeleter> raw;
    ngsld_pos *pos = nullptr;
  } early;
  const uint64_t geno_bytes = (uint64_t)pars.n_sites * pars.n_ind * 3 * sizeof(double);
  if (pars.in_bin && geno_bytes < (4ull << 30) && ngsld::test_knob("SLAB_SITES") == nullptr &&
      (pars.max_gpu_mem <= 0 || pars.max_gpu_mem * 1e9 > 3.0 * (double)geno_bytes)) {
    early.raw.reset(alloc_matrix((size_t)geno_bytes));
    if (early.raw) {
      early.started = true;
      early.th = std::thread([&early, &pars]() {
        early.geno_rc = ngsld_host_read_geno_bin(pars.in_geno, pars.n_ind, pars.n_sites, early.raw.get(), early.geno_err,
                                                 sizeof(early.geno_err));
        if (early.geno_rc == NGSLD_OK && pars.in_pos) {
          early.pos_rc = ngsld_host_read_pos(pars.in_pos, pars.in_pos_header ? 1 : 0, pars.n_sites, &early.pos,
                                             early.pos_err, sizeof(early.pos_err));
          early.pos_done = true;
        }
      });
    }
  }
  auto join_early = [&early]() {
    if (early.th.joinable()) early.th.join();
  };

  // ---- several devices: a windowed run on binary input lets every part read its own slab from the file ----
  if (pars.devices.size() > 1 && pars.in_bin && (pars.max_kb_dist > 0 || pars.max_snp_dist > 0)) {
    join_early();
    early.raw.reset();  // (every part reads its own slab)
    ngsld_host_free_pos(early.pos);
    if (pars.verbose >= 1) fprintf(stderr, "> Reading data from file...\n");
    run_multi(pars, nullptr, 0, pars.in_logscale ? 1 : 0);
    return 0;
  }

  // ---- device ----
  ngsld_ctx *ctx = nullptr;
  if (ngsld_create(pars.device, &ctx) != NGSLD_OK) {
    join_early();
    error("ngsld_create", ngsld_last_error(nullptr));
  }

  timing_report.mark("ngsld_create");
  char err[512];
  // ---- does the matrix fit the device?  If not, a windowed run on binary input is streamed slab by slab ----
  uint64_t budget = 0;
  {
    uint64_t free_b = 0, total_b = 0;
    if (ngsld_device_memory(pars.device, &free_b, &total_b) != NGSLD_OK)
      error("ngsld_device_memory", "cannot query the device memory");
    budget = (uint64_t)(0.9 * (double)free_b);
    if (pars.max_gpu_mem > 0 && pars.max_gpu_mem * 1e9 < (double)budget) budget = (uint64_t)(pars.max_gpu_mem * 1e9);
    // (--max_gpu_mem holds for what the library allocates by itself too: the exact store of the device-side replay)
    if (pars.max_gpu_mem > 0) (void)ngsld_set_memory_budget(pars.device, budget);
  }
  // resident = one context holding every site; the budget helpers price two, so ask with twice the budget.  `fits`: with room
  // for what the device-side replay of un-called input builds beside the planes -- the exact store and, for the lane-per-pair
  // replay kernel, its individual-major copy; this program's text batches of up to 512 individuals are the wavefront-per-pair
  // kernel's, which reads the store's own layout: the matrix twice, three times beyond.  `fits_bare`: the planes alone -- what a
  // run needs; without room for the store its flagged pairs are replayed on host threads (the same bytes, the reference's speed).
  const int copies = pars.n_ind > 512 ? 3 : 2;
  const bool fits = ngsld_sites_for_budget(pars.n_ind, 2 * budget, copies) >= pars.n_sites;
  const bool fits_bare = fits || ngsld_sites_for_budget(pars.n_ind, 2 * budget, 1) >= pars.n_sites;
  const bool streamable = pars.in_bin && (pars.max_kb_dist > 0 || pars.max_snp_dist > 0);
  uint64_t slab_sites = 0;  // > 0: run slab by slab
  if (const char *e = ngsld::test_knob("SLAB_SITES")) {  // tests: stream a small file in slabs of n sites
    if (pars.in_bin) slab_sites = strtoull(e, nullptr, 10);
  } else if (!fits) {
    // A windowed run on binary input that fits only without the store is streamed: every slab then has room for its own store.
    // Where slabs cannot be had (text input, no window, a budget below two contexts) the matrix stays resident if its planes
    // fit, without room for the store.
    if (streamable) slab_sites = ngsld_sites_for_budget(pars.n_ind, budget, copies);
    if (slab_sites < 2) slab_sites = 0;
    if (slab_sites == 0 && !fits_bare) {
      if (!pars.in_bin)
        error(__FUNCTION__, "the genotype matrix does not fit the device memory budget (only binary input is streamed)");
      slab_sites = ngsld_sites_for_budget(pars.n_ind, budget, 1);  // (slabs without room for the store before none at all)
      if (slab_sites < 2) error(__FUNCTION__, "the device memory budget is too small for this number of individuals");
    }
  } else if (!cluster.given && !grid.given && !linked.given && !partners.given && !dmap.given && !cross.given && !tree.given &&  // (the clusters, the grid, the linked pairs, the partners, the decay map, LD across chromosomes and the tree need the matrix resident: a job that fits is not cut only to overlap its read)
             pars.in_bin && (pars.max_kb_dist > 0 || pars.max_snp_dist > 0) && (uint64_t)st.st_size >= (4ull << 30) &&
             !(getenv("NGSLD_PIPELINE") && strcmp(getenv("NGSLD_PIPELINE"), "0") == 0)) {
    // a large windowed job that fits is still cut into about six slabs, only to overlap the file read and the
    // upload of one part with the pair kernels of the previous one (same output; falls back when a window is too wide).
    // From 4 GiB: a 1.2 GB file ran 0.5 s faster resident (2.2 s) than in slabs, a 5.8 GB one 0.5 s slower.
    slab_sites = std::min<uint64_t>(ngsld_sites_for_budget(pars.n_ind, budget, copies), (pars.n_sites + 5) / 6);
  }
  for (const Family &fam : kFamilies)
    if (slab_sites > 0 && *fam.given) {
      const std::string msg = std::string("--") + fam.prefix +
                              "out needs the whole matrix resident on one device: it does not fit (--max_gpu_mem) and would be cut into slabs!";
      error(__FUNCTION__, msg.c_str());
    }
  if (slab_sites > 0) {
    join_early();  // (an early read is only started for matrices far below these thresholds: normally nothing to wait for)
    early.raw.reset();
    ngsld_host_free_pos(early.pos);
    early.pos = nullptr;
    early.started = early.pos_done = false;
    ngsld_destroy(ctx);
    ctx = nullptr;
    if (run_streamed(pars, slab_sites, /*may_fall_back=*/fits_bare)) return 0;
    if (ngsld_create(pars.device, &ctx) != NGSLD_OK) error("ngsld_create", ngsld_last_error(nullptr));
  }

  // the pinned host buffers the text batches will land in: allocated by a library thread while the matrix is read, uploaded
  // and prepped (pinning ~0.7 GB costs ~0.1 s, which the first batches of the run used to wait for).  Only now that the run is
  // known to be resident: a streamed run uses contexts of its own, and destroying this one had to wait for the pinning to
  // finish only to undo it
  if (write_tsv && !host_text_only())
    (void)ngsld_reserve_text_buffers(ctx, pars.extend_out ? 190 : 95);

  // ---- read input data (ngsLD.cpp:85-114; the arithmetic runs on the device) ----
  if (pars.verbose >= 1) fprintf(stderr, "> Reading data from file...\n");
  join_early();
  // (malloc: 1.2 GB of zero-filling a std::vector before overwriting it was a third of the read time)
  std::unique_ptr<double, FreeDeleter> raw;
  if (early.started)
    raw = std::move(early.raw);
  else
    raw.reset(alloc_matrix((size_t)pars.n_sites * pars.n_ind * 3 * sizeof(double)));
  if (!raw) error(__FUNCTION__, "cannot allocate the genotype matrix");
  ngsld_geno_opts go;
  memset(&go, 0, sizeof(go));
  go.log_scale = pars.in_logscale ? 1 : 0;
  go.ignore_miss_data = pars.ignore_miss_data ? 1 : 0;
  go.call_geno = pars.call_geno ? 1 : 0;
  go.N_thresh = pars.N_thresh;
  go.call_thresh = pars.call_thresh;
  if (early.started) {
    if (early.geno_rc != NGSLD_OK) error("read_geno", early.geno_err);
  } else if (pars.in_bin) {
    if (ngsld_host_read_geno_bin(pars.in_geno, pars.n_ind, pars.n_sites, raw.get(), err, sizeof(err)) != NGSLD_OK)
      error("read_geno", err);
  } else {
    int is_log = 0;
    if (ngsld_host_read_geno_text(pars.in_geno, pars.in_probs ? 1 : 0, pars.in_logscale ? 1 : 0, pars.n_ind,
                                  pars.n_sites, raw.get(), &is_log, err, sizeof(err)) != NGSLD_OK)
      error("read_geno", err);
    go.log_scale = is_log;
    go.text_semantics = 1;
  }
  timing_report.mark("read genotype file");
  if (pars.devices.size() > 1) {  // all pairs (or text input) on several devices: the matrix is in host memory once
    ngsld_destroy(ctx);
    if (pars.call_geno && pars.verbose >= 1) fprintf(stderr, "> Calling genotypes...\n");
    if (pars.verbose >= 1) fprintf(stderr, "==> Calculating MAF for all sites...\n");
    run_multi(pars, raw.get(), go.text_semantics, go.log_scale);
    return 0;
  }
  if (pars.call_geno && pars.verbose >= 1) fprintf(stderr, "> Calling genotypes...\n");
  if (pars.verbose >= 1) fprintf(stderr, "==> Calculating MAF for all sites...\n");
  int rc = ngsld_set_geno_raw_opts(ctx, raw.get(), pars.n_sites, pars.n_ind, &go);
  if (rc == NGSLD_ERR_NAN) error("read_geno", ngsld_last_error(ctx));
  if (rc == NGSLD_ERR_INVALID && pars.call_geno) error("call_geno", ngsld_last_error(ctx));
  if (rc != NGSLD_OK) error("ngsld_set_geno_raw", ngsld_last_error(ctx));
  timing_report.mark("upload + per-site prep");
  // The matrix stays in host memory for the run (the reference holds it throughout, ngsLD.cpp:86-89): the pairs whose
  // outcome the reference's own rounding decides are replayed from it in the reference's operation order.
  struct RawSource {
    const double *raw;
    uint64_t n_sites, n_ind;
  } raw_src{raw.get(), pars.n_sites, pars.n_ind};
  auto read_raw = [](void *user, uint64_t site_begin, uint64_t n, double *dst) -> int {
    const RawSource *r = static_cast<const RawSource *>(user);
    if (site_begin + n > r->n_sites) return 1;
    memcpy(dst, r->raw + site_begin * r->n_ind * 3, n * r->n_ind * 3 * sizeof(double));
    return 0;
  };
  if (ngsld::test_knob_is("REPLAY_SOURCE", "0"))
    raw.reset();  // (tests: replay from the device's own planes)
  else if (ngsld::test_knob_is("REPLAY_SOURCE", "callback")) {  // (tests: the callback form)
    if (ngsld_set_replay_source(ctx, read_raw, &raw_src) != NGSLD_OK) error("ngsld_set_replay_source", ngsld_last_error(ctx));
  } else if (ngsld_set_replay_matrix(ctx, raw.get()) != NGSLD_OK)
    error("ngsld_set_replay_matrix", ngsld_last_error(ctx));

  if (pars.verbose >= 1) fprintf(stderr, "==> Getting sites coordinates\n");
  ngsld_pos *pos = nullptr;
  if (pars.in_pos) {
    if (early.pos_done) {
      if (early.pos_rc != NGSLD_OK) error(pos_error_function(early.pos_err, pars.in_pos), early.pos_err);
      pos = early.pos;
    } else if (ngsld_host_read_pos(pars.in_pos, pars.in_pos_header ? 1 : 0, pars.n_sites, &pos, err, sizeof(err)) != NGSLD_OK)
      error(pos_error_function(err, pars.in_pos), err);
    if (pars.verbose >= 6)
      for (uint64_t s = 0; s < (pars.n_sites < 10 ? pars.n_sites : 10); s++)
        fprintf(stderr, "%lu\t%f\n", (unsigned long)s, ngsld_host_pos_dist(pos)[s]);
  }
  if (ngsld_set_pos_dist(ctx, pos ? ngsld_host_pos_dist(pos) : nullptr) != NGSLD_OK)
    error("ngsld_set_pos_dist", ngsld_last_error(ctx));

  // ---- analyze data (replaces ngsLD.cpp:150-198) ----
  if (pars.verbose >= 1) fprintf(stderr, "==> Launching threads...\n");
  ngsld_params lp;
  lp.max_kb_dist = pars.max_kb_dist;
  lp.max_snp_dist = pars.max_snp_dist;
  lp.min_maf = pars.min_maf;
  lp.ignore_miss_data = pars.ignore_miss_data ? 1 : 0;
  lp.extend_out = pars.extend_out ? 1 : 0;
  lp.rnd_sample = pars.rnd_sample;
  lp.seed = pars.seed;
  lp.first_row = 0;
  uint64_t n_pairs = 0;
  timing_report.mark("positions");
  if (ngsld_plan(ctx, &lp, &n_pairs) != NGSLD_OK) error("ngsld_plan", ngsld_last_error(ctx));
  std::vector<double> maf(pars.n_sites);  // (after the plan: a frequency that ties --min_maf has been settled by then)
  if (ngsld_get_maf(ctx, maf.data()) != NGSLD_OK) error("ngsld_get_maf", ngsld_last_error(ctx));
  timing_report.mark("plan");
  // The rows are formatted on the device (the fprintf block of calc_pair_LD, ngsLD.cpp:310-352, at kernel rates); a
  // batch the device formatter cannot take arrives as records and goes through the --n_threads host formatter as
  // before.  NGSLD_HOST_TEXT=1 keeps everything on the host formatter (A/B, tests).
  if (write_tsv && !host_text_only()) {
    std::vector<const char *> lab;
    if (pos) {
      lab.resize(pars.n_sites);
      for (uint64_t s = 0; s < pars.n_sites; s++) lab[s] = ngsld_host_label(pos, s);
    }
    if (ngsld_set_text_output(ctx, pos ? lab.data() : nullptr, 1) != NGSLD_OK)
      error("ngsld_set_text_output", ngsld_last_error(ctx));
  }
  if (pars.verbose >= 1) fprintf(stderr, "==> Waiting for all threads to finish...\n");
  SinkState sink;
  sink.pars = &pars;
  sink.pos = pos;
  sink.pos_dist = pos ? ngsld_host_pos_dist(pos) : nullptr;
  sink.maf = &maf;
  timing_report.mark("labels to the device");
  rc = write_tsv ? ngsld_run(ctx, 0, pars.n_sites, write_batch, &sink) : NGSLD_OK;
  timing_report.mark("pair kernels + text + write");
  if (rc == NGSLD_ERR_MAF_RANGE) error("haplo_freq", ngsld_last_error(ctx));
  if (rc != NGSLD_OK) error("ngsld_run", ngsld_last_error(ctx));
  // two or more of the six analyses that read every planned pair share one run of the pair kernels (ngsld_analyze); the files
  // are written in the families' order either way
  std::vector<ngsld_analysis> bundle;
  for (const Family &fam : kFamilies)
    if (*fam.given && fam.stage != nullptr) bundle.push_back(fam.stage(pars, pos));
  if (bundle.size() >= 2) {
    ngsld_analyze_stats ast{};
    ast.struct_size = sizeof(ast);
    if (ngsld_analyze(ctx, bundle.data(), (uint32_t)bundle.size(), &ast) != NGSLD_OK) error("ngsld_analyze", ngsld_last_error(ctx));
    if (pars.verbose >= 1)
      fprintf(stderr, "==> analyses: %lu share one run of %lu pairs in %lu chunks\n", (unsigned long)bundle.size(),
              (unsigned long)ast.pairs_run, (unsigned long)ast.chunks);
    timing_report.mark("analyses (one run of the pair kernels)");
  }
  for (const Family &fam : kFamilies)
    if (*fam.given) {
      if (fam.stage == nullptr || bundle.size() < 2) fam.run(ctx, pars, pos);
      if (fam.write != nullptr) fam.write(ctx, pars, pos);
      timing_report.mark(fam.timing);
    }
  if (write_tsv && pars.verbose >= 2) {  // (level 1 is the reference's default: its stderr stays what the reference prints.  A large share
                            // here means pairs computed at the host's speed: two nearly monomorphic sites each)
    ngsld_replay_stats_t st{};
    (void)ngsld_replay_info(ctx, &st);
    fprintf(stderr, "==> %lu of %lu pairs replayed in the reference's operation order (%lu on the device, %lu on host threads)\n",
            (unsigned long)st.pairs_replayed, (unsigned long)n_pairs, (unsigned long)st.pairs_on_device, (unsigned long)st.pairs_on_host);
  }

  // ---- free memory (ngsLD.cpp:205-222) ----
  if (pars.verbose >= 1) fprintf(stderr, "==> Freeing memory...\n");
  close_output(pars.out_fh);
  ngsld_host_free_pos(pos);
  ngsld_destroy(ctx);
  timing_report.mark("free");
  if (pars.verbose >= 1) fprintf(stderr, "Done!\n");
  return 0;
}
