// blocks.hip -- LD blocks on the device (ngsld_blocks, include/ngsld.h): the square matrices scripts/LD_blocks.sh builds for
// LDheatmap over one region, from the pair records where they are computed -- no TSV; the matrices stay on the device until
// they are copied out or written as text.  BLOCKS.md has the rule, the deviations and why a cell's text is the TSV's.
//
//   members  host: each label's CHR:pos (up to the first TAB), the region's sites, their order by position (ord, -1 elsewhere)
//   pairs    RecordPass (record_pass.h) over the member rows (an in-region pair has a member as s1): replayed pairs carry their
//            replayed values, the rows of other sites are not run
//   scatter  one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the record's
//            double bits of every chosen field to M_f[ord(s1) * n + ord(s2)], a presence byte to P[...] -- pairs are unique,
//            no atomics; in file order = position order the lanes of an item write consecutive columns of one row
//   sites    members with a pair in their row or column: one pass over P (lanes over columns), compacted by hipCUB
//   text     ngsld_blocks_text: the lengths (one wavefront per matrix row, lanes over columns, a cross-lane sum), an exclusive
//            scan over the rows (text_scan), then the rows in chunks sized to a pinned buffer, each cell at its offset from a
//            wavefront prefix sum, written by ld_fmt.h's digit generator and word writer; a row with a value beyond that
//            generator's range is formatted on the host with the host TSV formatter
#include <hipcub/hipcub.hpp>

#include "../../include/ngsld_host.h"
#include "engine.h"
#include "ld_fmt.h"
#include "record_pass.h"

namespace {

// members beyond this are refused: an LDheatmap region is hundreds to a few thousand sites
constexpr uint64_t kMaxMembers = 1ull << 15;
// text of one chunk of rows (pinned); a longer row is a chunk of its own
constexpr uint64_t kTextChunkBytes = 64ull << 20;
// rows of P one workgroup of the site pass reads
constexpr uint32_t kSiteBand = 64;

struct ScatterArgs {
  const ngsld_item *items;
  uint64_t n_items;
  uint64_t out_base;                 // global index of the chunk's record 0
  const ngsld_rec_std *rec;
  const int32_t *ord;                // [n_sites] matrix index of a member, -1 elsewhere
  uint64_t n;                        // members
  int ns;                            // chosen fields
  int field[4];                      // 0 r2_ExpG, 1 D, 2 D', 3 r2
  unsigned long long *val;           // [ns][n][n] the records' bits
  uint8_t *present;                  // [n][n]
  unsigned long long *in_region;     // pairs scattered
};

__global__ __launch_bounds__(256) void scatter_kernel(ScatterArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  const uint64_t nn = A.n * A.n;
  unsigned long long hits = 0;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; i < A.n_items; i += waves) {
    const ngsld_item it = A.items[i];
    const uint32_t c = (uint32_t)lane;
    bool hit = false;
    if (c < it.count && ((it.mask >> c) & 1ull)) {
      const int32_t o1 = A.ord[it.s1], o2 = A.ord[it.s2_begin + c];
      if (o1 >= 0 && o2 >= 0) {
        // (the record's bits, a field's at its index in ngsld_rec_std: NaN signs survive)
        const unsigned long long *r = reinterpret_cast<const unsigned long long *>(A.rec + record_of(it, c, A.out_base));
        const uint64_t cell = (uint64_t)o1 * A.n + (uint64_t)o2;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (v >= A.ns) break;
          A.val[(uint64_t)v * nn + cell] = r[A.field[v]];
        }
        A.present[cell] = 1;
        hit = true;
      }
    }
    hits += (unsigned long long)__popcll(__ballot(hit));
  }
  if (lane == 0 && hits) atomicAdd(A.in_region, hits);
}

// mark[i] = 1 for a member with a pair in row i or column i of P: threads over columns, a band of rows per workgroup
__global__ __launch_bounds__(256) void sites_kernel(const uint8_t *P, uint64_t n, uint8_t *mark) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.y * kSiteBand, i1 = i0 + kSiteBand < n ? i0 + kSiteBand : n;
  bool col = false;
  for (uint64_t i = i0; i < i1; ++i) {
    const bool v = j < n && P[i * n + j] != 0;
    col |= v;
    if (__ballot(v) != 0 && __lane_id() == 0) mark[i] = 1;
  }
  if (col) mark[j] = 1;
}

struct RowTextArgs {
  const uint8_t *present;            // [n][n]
  const double *val;                 // [n][n] of the field
  uint64_t n;
  const uint32_t *col;               // [m] member index of each matrix site
  uint64_t m;
  const char *labels;                // the matrix sites' labels, back to back
  const uint64_t *label_off;         // [m + 1]
  uint64_t row0, n_rows;             // the chunk's rows
  uint64_t *lens;                    // [m] row bytes (length pass)
  const uint64_t *offs;              // [m] exclusive prefix sums of lens (write pass)
  uint64_t text_base;                // offs[row0]
  uint64_t text_cap;                 // bytes of text
  char *text;
  uint8_t *needs_host;               // [m] a value beyond the device formatter's range
  int force_host;                    // every row to the host (test knob)
  unsigned long long *overflow;      // a row would end beyond text_cap (internal error)
};

// "\t" and the cell's text (the TSV's "%f" of the record, or NA); false where the device formatter cannot take the value
template <class E>
__device__ __forceinline__ bool put_cell(E &e, const RowTextArgs &A, uint64_t a, uint64_t b) {
  e.put('\t');
  if (!A.present[a * A.n + b]) {
    e.put('N');
    e.put('A');
    return true;
  }
  return ngsld::put_fixed<6>(e, A.val[a * A.n + b]);
}

__global__ __launch_bounds__(256) void text_length_kernel(RowTextArgs A) {
  const uint64_t r = A.row0 + (((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6);
  if (r >= A.row0 + A.n_rows) return;  // (a whole wavefront)
  const int lane = (int)__lane_id();
  const uint64_t a = A.col[r];
  unsigned long long len = 0;
  bool ok = true;
  for (uint64_t j = (uint64_t)lane; j < A.m; j += 64) {
    ngsld::Counter cnt;
    ok &= put_cell(cnt, A, a, A.col[j]);
    len += cnt.n;
  }
  for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o);
  const bool any_bad = __ballot(!ok) != 0;
  if (lane == 0) {
    A.lens[r] = (A.label_off[r + 1] - A.label_off[r]) + len + 1;
    A.needs_host[r] = (any_bad || A.force_host) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void text_write_kernel(RowTextArgs A) {
  const uint64_t r = A.row0 + (((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6);
  if (r >= A.row0 + A.n_rows) return;
  if (A.needs_host[r]) return;  // (the host writes that row)
  const int lane = (int)__lane_id();
  uint64_t pos = A.offs[r] - A.text_base;
  if (pos + A.lens[r] > A.text_cap) {
    if (lane == 0) atomicOr(A.overflow, 1ull);
    return;
  }
  const uint64_t lb = A.label_off[r], ln = A.label_off[r + 1] - lb;
  if (lane == 0) {
    ngsld::WordWriter w(A.text + pos);
    for (uint64_t i = 0; i < ln; ++i) w.put(A.labels[lb + i]);
    w.finish();
  }
  pos += ln;
  const uint64_t a = A.col[r];
  for (uint64_t j0 = 0; j0 < A.m; j0 += 64) {  // (every lane takes part in every shuffle)
    const uint64_t j = j0 + (uint64_t)lane;
    ngsld::Counter cnt;
    if (j < A.m) (void)put_cell(cnt, A, a, A.col[j]);
    unsigned long long incl = cnt.n;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long x = __shfl_up(incl, o);
      if (lane >= o) incl += x;
    }
    if (j < A.m) {
      ngsld::WordWriter w(A.text + pos + (incl - cnt.n));
      (void)put_cell(w, A, a, A.col[j]);
      w.finish();
    }
    pos += __shfl(incl, 63);
  }
  if (lane == 0) A.text[pos] = '\n';
}

// the m x m matrix of one field in matrix order: the records' bits where present, NaN elsewhere
__global__ __launch_bounds__(256) void gather_kernel(const uint8_t *P, const unsigned long long *val, uint64_t n,
                                                     const uint32_t *col, uint64_t m, unsigned long long *out_val,
                                                     uint8_t *out_present) {
  const uint64_t total = m * m, stride = (uint64_t)gridDim.x * 256;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const uint64_t cell = (uint64_t)col[t / m] * n + col[t % m];
    const uint8_t p = P[cell];
    out_present[t] = p;
    out_val[t] = p ? val[cell] : 0x7ff8000000000000ull;
  }
}

}  // namespace

extern "C" {

int ngsld_blocks(ngsld_ctx *c, const ngsld_blocks_params *p, const char *const *labels, ngsld_blocks_stats *stats) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  const auto t_all = std::chrono::steady_clock::now();
  c->res.blocks.clear();  // its own store alone: the other analyses' results stay
  if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
  if (const int rc = check_struct_sizes(c, p, "ngsld_blocks_params", stats, "ngsld_blocks_stats")) return rc;
  if (p->fields == 0 || p->fields > 15) return fail(c, NGSLD_ERR_INVALID, "blocks fields must be a non-empty mask of 1, 2, 4, 8");
  if (p->chr == nullptr) return fail(c, NGSLD_ERR_INVALID, "blocks chr is NULL");
  if (!(p->start < p->end)) return fail(c, NGSLD_ERR_INVALID, "start position must be smaller than end position.");
  if (labels == nullptr) return fail(c, NGSLD_ERR_INVALID, "LD blocks need positions: the labels are NULL");
  const uint64_t n_sites = c->n_sites;
  ngsld_blocks_stats S;
  if (const int rc = begin_pass(c, S)) return rc;
  hipStream_t st = c->stream;
  int field[4] = {0, 0, 0, 0};
  const int ns = field_list(p->fields, field);

  // ---- members: CHR:p with START <= p <= END, in position order ----
  const std::string chr = p->chr;
  struct Member {
    uint64_t pos, site;
  };
  std::vector<Member> mem;
  std::vector<uint8_t> is_member(n_sites, 0);
  for (uint64_t s = 0; s < n_sites; ++s) {
    if (labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "a label is NULL");
    const LabelPos L = label_pos(labels[s]);
    if (L.key == "(null)") return fail(c, NGSLD_ERR_INVALID, "LD blocks need positions: a label is \"(null)\"");
    if (!L.on(chr)) continue;
    uint64_t pos = 0;
    if (!L.position(&pos)) return fail(c, NGSLD_ERR_UNSUPPORTED, "LD blocks: the position of label \"" + L.key + "\" is not plain decimal digits");
    if (pos < p->start || pos > p->end) continue;
    mem.push_back({pos, s});
    is_member[s] = 1;
  }
  std::sort(mem.begin(), mem.end(), [](const Member &a, const Member &b) { return a.pos < b.pos || (a.pos == b.pos && a.site < b.site); });
  for (size_t k = 1; k < mem.size(); ++k)
    if (mem[k].pos == mem[k - 1].pos)
      return fail(c, NGSLD_ERR_UNSUPPORTED, "LD blocks: sites \"" + label_pos(labels[mem[k - 1].site]).key + "\" and \"" +
                                                label_pos(labels[mem[k].site]).key + "\" of the region share a position");
  const uint64_t n = mem.size();
  S.members = n;
  const uint64_t bytes = (uint64_t)ns * n * n * 8 + n * n;
  if (n > kMaxMembers)
    return fail(c, NGSLD_ERR_UNSUPPORTED, "LD blocks: " + std::to_string(n) + " region members (at most 32768; the matrices would take " +
                                              std::to_string(bytes) + " bytes)");
  if (n > 0 && !room_for(bytes, 1ull << 30, 256ull << 20))
    return fail(c, NGSLD_ERR_UNSUPPORTED, "LD blocks: no room on the device for the matrices of " + std::to_string(n) +
                                              " region members (" + std::to_string(bytes) + " bytes)");
  for (uint64_t s = 0; s < n_sites; ++s)
    if (is_member[s]) S.pairs += c->h_row_off[s + 1] - c->h_row_off[s];

  if (n > 0 && S.pairs > 0) {
    std::vector<int32_t> ord(n_sites, -1);
    for (uint64_t k = 0; k < n; ++k) ord[mem[k].site] = (int32_t)k;
    DevBuf<int32_t> d_ord;
    DevBuf<unsigned long long> d_count;
    HIP_TRY(c, d_ord.resize(n_sites));
    HIP_TRY(c, d_count.resize(1));
    HIP_TRY(c, hipMemcpy(d_ord.p, ord.data(), n_sites * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, c->res.blocks.d_val.resize((size_t)ns * n * n));
    HIP_TRY(c, c->res.blocks.d_present.resize((size_t)n * n));
    HIP_TRY(c, hipMemsetAsync(c->res.blocks.d_present.p, 0, n * n, st));
    HIP_TRY(c, hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), st));
    // the member rows only: the rows of other sites are not run
    RecordPass R;
    if (const int rc = R.open(c, record_chunk(test_knob("BLOCKS_CHUNK_PAIRS")), is_member.data())) return rc;
    ScatterArgs A{};
    A.rec = R.records();
    A.ord = d_ord.p;
    A.n = n;
    A.ns = ns;
    for (int v = 0; v < 4; ++v) A.field[v] = field[v];
    A.val = reinterpret_cast<unsigned long long *>(c->res.blocks.d_val.p);
    A.present = c->res.blocks.d_present.p;
    A.in_region = d_count.p;
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 4;
    const int rc = R.run(&S.pairs_ms, &S.scatter_ms, &S.chunks, nullptr, [&](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      A.out_base = ch.out_base;
      A.items = items;
      A.n_items = n_items;
      hipLaunchKernelGGL(scatter_kernel, dim3(std::min<unsigned>(blocks_for(n_items * 64), max_blocks)), dim3(256), 0, st, A);
    });
    if (rc != NGSLD_OK) return rc;

    // ---- matrix sites: members with a pair in their row or column, compacted in matrix order ----
    DevBuf<uint8_t> d_mark;
    DevBuf<uint32_t> d_col, d_num;
    HIP_TRY(c, d_mark.resize(n));
    HIP_TRY(c, d_col.resize(n));
    HIP_TRY(c, d_num.resize(1));
    HIP_TRY(c, hipMemsetAsync(d_mark.p, 0, n, st));
    EventPair ev;
    HIP_TRY(c, ev.create());
    HIP_TRY(c, hipEventRecord(ev.a, st));
    hipLaunchKernelGGL(sites_kernel, dim3(blocks_for(n), (unsigned)((n + kSiteBand - 1) / kSiteBand)), dim3(256), 0, st,
                       (const uint8_t *)c->res.blocks.d_present.p, n, d_mark.p);
    HIP_TRY(c, hipGetLastError());
    hipcub::CountingInputIterator<uint32_t> idx(0);
    size_t temp_bytes = 0;
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, temp_bytes, idx, d_mark.p, d_col.p, d_num.p, (int)n, st));
    DevBuf<char> d_temp;
    HIP_TRY(c, d_temp.resize(std::max<size_t>(temp_bytes, 1)));
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(d_temp.p, temp_bytes, idx, d_mark.p, d_col.p, d_num.p, (int)n, st));
    HIP_TRY(c, hipEventRecord(ev.b, st));
    uint32_t m = 0;
    unsigned long long in_region = 0;
    HIP_TRY(c, hipMemcpyAsync(&m, d_num.p, sizeof(m), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&in_region, d_count.p, sizeof(in_region), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, ev.add_elapsed(&S.scatter_ms));
    S.pairs_in_region = in_region;
    if (m > 0) {
      std::vector<uint32_t> col(m);
      HIP_TRY(c, hipMemcpy(col.data(), d_col.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIP_TRY(c, c->res.blocks.d_col.resize(m));
      HIP_TRY(c, hipMemcpy(c->res.blocks.d_col.p, col.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
      std::vector<uint64_t> off(m + 1, 0);
      for (uint32_t k = 0; k < m; ++k) {
        const uint64_t s = mem[col[k]].site;
        c->res.blocks.site.push_back(s);
        c->res.blocks.label.push_back(label_pos(labels[s]).key);
        off[k + 1] = off[k] + c->res.blocks.label.back().size();
      }
      std::string blob;
      blob.reserve(off[m]);
      for (const std::string &l : c->res.blocks.label) blob += l;
      HIP_TRY(c, c->res.blocks.d_label.resize(std::max<size_t>(blob.size(), 1)));
      HIP_TRY(c, c->res.blocks.d_label_off.resize(m + 1));
      if (!blob.empty()) HIP_TRY(c, hipMemcpy(c->res.blocks.d_label.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(c->res.blocks.d_label_off.p, off.data(), (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
  }
  if (c->res.blocks.site.empty()) {  // (no in-region pair: nothing to keep on the device)
    c->res.blocks.d_val.release();
    c->res.blocks.d_present.release();
  }
  c->res.blocks.fields = p->fields;
  c->res.blocks.members = n;
  S.sites = c->res.blocks.site.size();
  S.cells_na = S.sites * S.sites - S.pairs_in_region;
  S.total_ms = ms_since(t_all);
  copy_stats(stats, S);
  return NGSLD_OK;
} NGSLD_CATCH(c)

int ngsld_blocks_sites(ngsld_ctx *c, uint64_t cap, uint64_t *site, uint64_t *n_sites) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.blocks.valid()) return fail(c, NGSLD_ERR_INVALID, "ngsld_blocks has not been called since the last plan or setting");
  const uint64_t m = c->res.blocks.site.size();
  if (n_sites) *n_sites = m;
  const uint64_t k = std::min<uint64_t>(cap, m);
  if (k > 0 && site) std::memcpy(site, c->res.blocks.site.data(), k * sizeof(uint64_t));
  return NGSLD_OK;
}

int ngsld_blocks_matrix(ngsld_ctx *c, int field, double *values, uint8_t *present) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.blocks.valid()) return fail(c, NGSLD_ERR_INVALID, "ngsld_blocks has not been called since the last plan or setting");
  const int v = field_rank(c->res.blocks.fields, field);
  if (v < 0) return fail(c, NGSLD_ERR_INVALID, "blocks field must be a TSV column 4..7 that ngsld_blocks was given");
  const uint64_t m = c->res.blocks.site.size(), n = c->res.blocks.members;
  if (m == 0 || (values == nullptr && present == nullptr)) return NGSLD_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  DevBuf<unsigned long long> d_val;
  DevBuf<uint8_t> d_present;
  HIP_TRY(c, d_val.resize(m * m));
  HIP_TRY(c, d_present.resize(m * m));
  const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 8;
  hipLaunchKernelGGL(gather_kernel, dim3(std::min<unsigned>(blocks_for(m * m), max_blocks)), dim3(256), 0, st,
                     (const uint8_t *)c->res.blocks.d_present.p,
                     reinterpret_cast<const unsigned long long *>(c->res.blocks.d_val.p) + (uint64_t)v * n * n, n,
                     (const uint32_t *)c->res.blocks.d_col.p, m, d_val.p, d_present.p);
  HIP_TRY(c, hipGetLastError());
  if (values) HIP_TRY(c, hipMemcpyAsync(values, d_val.p, m * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (present) HIP_TRY(c, hipMemcpyAsync(present, d_present.p, m * m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return NGSLD_OK;
} NGSLD_CATCH(c)

int ngsld_blocks_text(ngsld_ctx *c, int field, ngsld_text_fn sink, void *user, ngsld_blocks_stats *stats) try {
  if (c == nullptr || sink == nullptr) return NGSLD_ERR_INVALID;
  if (!c->res.blocks.valid()) return fail(c, NGSLD_ERR_INVALID, "ngsld_blocks has not been called since the last plan or setting");
  const int v = field_rank(c->res.blocks.fields, field);
  if (v < 0) return fail(c, NGSLD_ERR_INVALID, "blocks field must be a TSV column 4..7 that ngsld_blocks was given");
  if (stats != nullptr && stats->struct_size < sizeof(ngsld_blocks_stats))
    return fail(c, NGSLD_ERR_INVALID, "ngsld_blocks_stats: struct_size must be sizeof(ngsld_blocks_stats)");
  const auto t_all = std::chrono::steady_clock::now();
  double sink_ms = 0;
  uint64_t host_rows = 0;
  auto give = [&](const char *p, uint64_t len) -> int {
    if (len == 0) return NGSLD_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = sink(user, p, len);
    sink_ms += ms_since(t0);
    return rc == 0 ? NGSLD_OK : fail(c, NGSLD_ERR_SINK, "the blocks text sink returned non-zero");
  };
  const uint64_t m = c->res.blocks.site.size(), n = c->res.blocks.members;
  {  // the label row: an empty first cell, then the sites
    std::string head;
    for (const std::string &l : c->res.blocks.label) {
      head += '\t';
      head += l;
    }
    head += '\n';
    const int rc = give(head.data(), head.size());
    if (rc != NGSLD_OK) return rc;
  }
  if (m > 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    DevBuf<uint64_t> d_lens, d_offs, d_total;
    DevBuf<uint8_t> d_needs;
    DevBuf<unsigned long long> d_overflow;
    DevBuf<char> d_scan;
    HIP_TRY(c, d_lens.resize(m));
    HIP_TRY(c, d_offs.resize(m));
    HIP_TRY(c, d_total.resize(1));
    HIP_TRY(c, d_needs.resize(m));
    HIP_TRY(c, d_overflow.resize(1));
    HIP_TRY(c, hipMemsetAsync(d_overflow.p, 0, sizeof(unsigned long long), st));
    const size_t scan_bytes = text_scan_temp_bytes(m);
    HIP_TRY(c, d_scan.resize(std::max<size_t>(scan_bytes, 1)));
    RowTextArgs A{};
    A.present = c->res.blocks.d_present.p;
    A.val = c->res.blocks.d_val.p + (uint64_t)v * n * n;
    A.n = n;
    A.col = c->res.blocks.d_col.p;
    A.m = m;
    A.labels = c->res.blocks.d_label.p;
    A.label_off = c->res.blocks.d_label_off.p;
    A.row0 = 0;
    A.n_rows = m;
    A.lens = d_lens.p;
    A.offs = d_offs.p;
    A.needs_host = d_needs.p;
    A.force_host = test_knob_is("BLOCKS_HOST_ROWS", "1") ? 1 : 0;
    A.overflow = d_overflow.p;
    hipLaunchKernelGGL(text_length_kernel, dim3(blocks_for(m * 64)), dim3(256), 0, st, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, text_scan(d_scan.p, scan_bytes, d_lens.p, d_offs.p, m, d_total.p, st));
    std::vector<uint64_t> offs(m + 1);
    std::vector<uint8_t> needs(m);
    HIP_TRY(c, hipMemcpyAsync(offs.data(), d_offs.p, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&offs[m], d_total.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(needs.data(), d_needs.p, m, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));

    // chunks of rows: up to kTextChunkBytes of text (a longer row alone), or BLOCKS_TEXT_ROWS rows
    uint64_t max_rows = m;
    if (const char *e = test_knob("BLOCKS_TEXT_ROWS")) max_rows = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    uint64_t cap = kTextChunkBytes;
    for (uint64_t r = 0; r < m; ++r) cap = std::max<uint64_t>(cap, offs[r + 1] - offs[r]);
    cap = std::min<uint64_t>(cap, offs[m]);
    DevBuf<char> d_text;
    PinBuf<char> h_text;
    HIP_TRY(c, d_text.resize(std::max<uint64_t>(cap, 1)));
    HIP_TRY(c, h_text.resize(std::max<uint64_t>(cap, 1)));
    A.text = d_text.p;
    A.text_cap = cap;
    std::vector<uint8_t> h_present;
    std::vector<double> h_val;
    std::vector<uint32_t> h_col;
    std::string row;
    char buf[512];
    for (uint64_t r0 = 0; r0 < m;) {
      uint64_t r1 = r0 + 1;
      while (r1 < m && r1 - r0 < max_rows && offs[r1 + 1] - offs[r0] <= cap) ++r1;
      A.row0 = r0;
      A.n_rows = r1 - r0;
      A.text_base = offs[r0];
      hipLaunchKernelGGL(text_write_kernel, dim3(blocks_for(A.n_rows * 64)), dim3(256), 0, st, A);
      HIP_TRY(c, hipGetLastError());
      unsigned long long overflow = 0;
      HIP_TRY(c, hipMemcpyAsync(h_text.p, d_text.p, offs[r1] - offs[r0], hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(&overflow, d_overflow.p, sizeof(overflow), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (overflow != 0) return fail(c, NGSLD_ERR_INVALID, "blocks text: a row beyond its chunk (internal error)");
      // device rows as they are; a row the device formatter could not take, from the records' doubles with the host's "%f"
      uint64_t from = r0;
      for (uint64_t r = r0; r <= r1; ++r) {
        if (r < r1 && !needs[r]) continue;
        int rc = give(h_text.p + (offs[from] - offs[r0]), offs[r] - offs[from]);
        if (rc != NGSLD_OK) return rc;
        if (r == r1) break;
        if (h_col.empty()) {
          h_col.resize(m);
          HIP_TRY(c, hipMemcpy(h_col.data(), c->res.blocks.d_col.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
          h_present.resize(n);
          h_val.resize(n);
        }
        const uint64_t a = h_col[r];
        HIP_TRY(c, hipMemcpy(h_present.data(), c->res.blocks.d_present.p + a * n, n, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(h_val.data(), c->res.blocks.d_val.p + (uint64_t)v * n * n + a * n, n * sizeof(double), hipMemcpyDeviceToHost));
        row = c->res.blocks.label[r];
        for (uint64_t j = 0; j < m; ++j) {
          row += '\t';
          if (!h_present[h_col[j]]) {
            row += "NA";
          } else {
            const size_t k = ngsld_host_format_double(buf, sizeof(buf), h_val[h_col[j]], 6);
            row.append(buf, k);
          }
        }
        row += '\n';
        ++host_rows;
        rc = give(row.data(), row.size());
        if (rc != NGSLD_OK) return rc;
        from = r + 1;
      }
      r0 = r1;
    }
  }
  if (stats != nullptr) {
    stats->format_ms += ms_since(t_all) - sink_ms;
    stats->host_rows += host_rows;
  }
  return NGSLD_OK;
} NGSLD_CATCH(c)

}  // extern "C"
