// linked.hip -- linked pairs on the device (ngsld_linked_pairs, include/ngsld.h): the rows of the TSV that pass an LD floor, in
// the table's order, as compact records and (or) as text -- no TSV.  LINKED.md has the rule, the deviations and the design.
//
//   pairs    RecordPass (record_pass.h): ngsld_run_device + ngsld_finish_device, chunk of rows by chunk, into records -- the 40 B
//            records too where the plan has extend_out (replayed pairs carry their replayed values)
//   count    one wavefront per work item, one lane per candidate (ld_records.h), launched once per slice of a chunk's items: the
//            rule on the printed value (ld_prune.h), a passing lane measures its row with the Counter emitter (ld_text_row.h); one
//            ballot is the item's survivor mask, a wavefront sum its bytes; lane 0 stores mask, rows and bytes of the item
//   scan     two exclusive prefix sums over the chunk's items (text_scan: hipCUB); the two totals and needs_host come back in
//            one small copy and the host grows the output buffers to fit -- the write kernel has no capacity check
//   write    again per slice: a survivor's row index is the item's offset + the popcount of the mask below its lane, its byte
//            offset the item's + an exclusive wavefront scan (six shuffles) of the lanes' lengths, measured again rather than
//            kept between the kernels; it stores s1, s2 and the record(s) compactly and formats its row where it belongs
//   host     a chunk with a row beyond the device formatter's range (needs_host): its surviving rows are formatted from the
//            compacted records by the host TSV formatter, in the same order
#include "../../include/ngsld_host.h"
#include "engine.h"
#include "ld_prune.h"
#include "ld_text_row.h"
#include "record_pass.h"

namespace {

struct LinkedArgs {
  ngsld::TextArgs T;          // the items of this launch, the records, the sites' arrays and labels; lens / offs / text unused
  uint64_t item0;             // index of the launch's first item among the chunk's
  const uint8_t *maf_ok;      // printed maf >= min_maf, per site
  double limit;               // has_limit: dist <= limit
  double min_weight;
  int has_limit;              // a finite max_kb_dist was given; 0: no condition on dist at all
  int field;                  // 0 r2_ExpG, 1 D, 2 D', 3 r2
  int abs_value;
  int text;                   // count: measure the rows; write: format them
  // per item of the chunk
  unsigned long long *mask;   // the survivors among the item's candidates
  uint64_t *rows, *bytes;     // their number, the bytes of their rows
  const uint64_t *row_off, *byte_off;  // exclusive prefix sums of rows / bytes over the chunk's items
  // the chunk's linked rows, compact and in order
  uint32_t *s1, *s2;
  ngsld_rec_std *out_std;
  ngsld_rec_ext *out_ext;     // null without extend_out
  char *out_text;
};

__global__ __launch_bounds__(256) void count_kernel(LinkedArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, step = (uint64_t)gridDim.x * 4;
  for (uint64_t i = first; i < A.T.n_items; i += step) {
    const ngsld_item it = A.T.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    bool pass = false;
    long long len = 0;
    if (c < it.count && ((it.mask >> c) & 1ull) && A.maf_ok[s1] && A.maf_ok[s2] &&
        (!A.has_limit || (A.T.infc[s1] == A.T.infc[s2] && A.T.cum[s2] - A.T.cum[s1] <= A.limit))) {
      const uint64_t k = ngsld::record_of(it, c, A.T.out_base);
      const double x = ngsld::field_of(A.T.std_rec[k], A.field);
      if (x - x == 0.0) {  // (not NaN or +-inf)
        double v = ngsld::prune_printed(x);  // the printed value read back (ld_prune.h), as doubles
        if (A.abs_value && v < 0) v = -v;
        pass = v >= A.min_weight;
      }
      if (pass && A.text) {
        ngsld::Counter n;
        if (!ngsld::format_row(n, A.T, s1, s2, k)) atomicExch(A.T.needs_host, 1);
        len = (long long)n.n;
      }
    }
    const unsigned long long m = __ballot(pass);
    const long long sum = ngsld::wave_sum(len);
    if (lane == 0) {
      A.mask[A.item0 + i] = m;
      A.rows[A.item0 + i] = (uint64_t)__popcll(m);
      A.bytes[A.item0 + i] = (uint64_t)sum;
    }
  }
}

__global__ __launch_bounds__(256) void write_kernel(LinkedArgs A) {
  const int lane = (int)__lane_id();
  const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, step = (uint64_t)gridDim.x * 4;
  for (uint64_t i = first; i < A.T.n_items; i += step) {
    const unsigned long long m = A.mask[A.item0 + i];
    if (m == 0) continue;  // (the whole wavefront)
    const ngsld_item it = A.T.items[i];
    const uint32_t c = (uint32_t)lane;
    const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
    const bool pass = (m >> c) & 1ull;
    const uint64_t k = pass ? ngsld::record_of(it, c, A.T.out_base) : 0;
    if (pass) {
      const uint64_t r = A.row_off[A.item0 + i] + (uint64_t)__popcll(m & ((1ull << c) - 1ull));
      A.s1[r] = s1;
      A.s2[r] = s2;
      A.out_std[r] = A.T.std_rec[k];
      if (A.out_ext != nullptr) A.out_ext[r] = A.T.ext_rec[k];
    }
    if (!A.text) continue;
    ngsld::Counter n;
    if (pass) (void)ngsld::format_row(n, A.T, s1, s2, k);
    unsigned long long incl = n.n;  // (every lane takes part in every shuffle)
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long x = __shfl_up(incl, o);
      if (lane >= o) incl += x;
    }
    if (pass) {
      ngsld::WordWriter w(A.out_text + A.byte_off[A.item0 + i] + (incl - n.n));
      (void)ngsld::format_row(w, A.T, s1, s2, k);
      w.finish();
    }
  }
}

// room for `need` entries, doubling (the contents are not kept: a chunk's rows leave with the sink before the next chunk's come)
template <class B>
hipError_t grow(B &b, uint64_t need) {
  if (need <= b.n && b.p != nullptr) return hipSuccess;
  return b.resize((size_t)std::max<uint64_t>(need, 2 * (uint64_t)b.n));
}

}  // namespace

extern "C" {

int ngsld_linked_pairs(ngsld_ctx *c, const ngsld_linked_params *p, const char *const *labels, ngsld_linked_fn sink, void *user,
                       ngsld_linked_stats *stats) try {
  if (c == nullptr || sink == nullptr) return NGSLD_ERR_INVALID;
  const auto t_all = std::chrono::steady_clock::now();
  if (!c->planned) return fail(c, NGSLD_ERR_INVALID, "ngsld_plan has not been called");
  if (const int rc = check_struct_sizes(c, p, "ngsld_linked_params", stats, "ngsld_linked_stats")) return rc;
  if (p->field < 4 || p->field > 7) return fail(c, NGSLD_ERR_INVALID, "linked field must be a TSV column 4..7");
  if (std::isnan(p->min_weight)) return fail(c, NGSLD_ERR_INVALID, "linked min_weight is NaN");
  if (std::isnan(p->max_kb_dist) || p->max_kb_dist < 0) return fail(c, NGSLD_ERR_INVALID, "linked max_kb_dist must be >= 0");
  if (std::isnan(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "linked min_maf is NaN");
  if (p->min_maf < 0 || std::isinf(p->min_maf)) return fail(c, NGSLD_ERR_INVALID, "linked min_maf must be a number >= 0");
  if ((p->want & (NGSLD_LINKED_RECORDS | NGSLD_LINKED_TEXT)) == 0 || (p->want & ~(NGSLD_LINKED_RECORDS | NGSLD_LINKED_TEXT)) != 0)
    return fail(c, NGSLD_ERR_INVALID, "linked want must be NGSLD_LINKED_RECORDS, NGSLD_LINKED_TEXT or both");
  const uint64_t n = c->n_sites;
  const bool want_rec = (p->want & NGSLD_LINKED_RECORDS) != 0, want_text = (p->want & NGSLD_LINKED_TEXT) != 0;
  const bool ext = c->params.extend_out != 0;
  if (want_text && labels != nullptr)
    for (uint64_t s = 0; s < n; ++s)
      if (labels[s] == nullptr) return fail(c, NGSLD_ERR_INVALID, "a label is NULL");
  ngsld_linked_stats S;
  if (const int rc = begin_pass(c, S)) return rc;
  hipStream_t st = c->stream;

  // ---- sites: the dist prefix sums (the limit and the dist column come from them), the maf filter on the printed maf ----
  SiteFilter F;
  F.prepare(c, &p->min_maf);
  const bool has_limit = std::isfinite(p->max_kb_dist);
  if (const int rc = F.check_limit(c, "linked", p->max_kb_dist)) return rc;
  const uint64_t chunk = record_chunk(test_knob("LINKED_CHUNK_PAIRS"));
  const uint64_t n_pairs = c->h_row_off[n];
  S.pairs = n_pairs;
  // Without exact prefix sums the device cannot print the dist column (the host writer adds the gaps one by one): every chunk's
  // rows are then formatted on the host, as the full table's are (engine_run.hip).  NGSLD_TEST_LINKED_FORCE_HOST=1: the same, by hand.
  const bool all_host = want_text && (!F.exact_gaps || test_knob_is("LINKED_FORCE_HOST", "1"));

  if (n_pairs > 0) {
    if (const int rc = F.upload(c)) return rc;
    DevBuf<char> d_labels;
    DevBuf<uint64_t> d_label_off;
    size_t max_label = 6;  // "(null)"
    if (want_text && labels != nullptr) {
      std::vector<uint64_t> off(n + 1, 0);
      for (uint64_t s = 0; s < n; ++s) {
        const size_t len = std::strlen(labels[s]);
        off[s + 1] = off[s] + len;
        max_label = std::max(max_label, len);
      }
      std::vector<char> blob(off[n] ? off[n] : 1);
      for (uint64_t s = 0; s < n; ++s) std::memcpy(blob.data() + off[s], labels[s], off[s + 1] - off[s]);
      HIP_TRY(c, d_labels.resize(blob.size()));
      HIP_TRY(c, d_label_off.resize(n + 1));
      HIP_TRY(c, hipMemcpy(d_labels.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(d_label_off.p, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    RecordPass R;
    if (const int rc = R.open(c, chunk, nullptr, true, ext)) return rc;
    EventPair ev;
    HIP_TRY(c, ev.create());
    // per item of a chunk; [0] rows, [1] bytes, [2] needs_host (an int in its low half) in one small copy
    DevBuf<unsigned long long> d_mask;
    DevBuf<uint64_t> d_rows, d_bytes, d_row_off, d_byte_off, d_meta;
    DevBuf<char> d_scan;
    HIP_TRY(c, d_meta.resize(3));
    // the chunk's linked rows on the device and in pinned memory, grown as chunks need them
    DevBuf<uint32_t> d_s1, d_s2;
    DevBuf<ngsld_rec_std> d_std;
    DevBuf<ngsld_rec_ext> d_ext;
    DevBuf<char> d_text;
    PinBuf<uint32_t> h_s1, h_s2;
    PinBuf<ngsld_rec_std> h_std;
    PinBuf<ngsld_rec_ext> h_ext;
    PinBuf<char> h_text;
    std::string host_text;
    std::vector<char> row_buf(2 * max_label + 1024);

    LinkedArgs A{};
    A.T.std_rec = R.records();
    A.T.ext_rec = R.ext_records();
    A.T.maf = c->d_maf.p;
    A.T.cum = F.d_cum.p;
    A.T.infc = F.d_infc.p;
    A.T.labels = labels != nullptr ? d_labels.p : nullptr;
    A.T.label_off = d_label_off.p;
    A.maf_ok = F.d_maf_ok.p;
    A.limit = p->max_kb_dist * 1000.0;
    A.has_limit = has_limit ? 1 : 0;
    A.min_weight = p->min_weight;
    A.field = p->field - 4;
    A.abs_value = p->abs_value != 0 ? 1 : 0;
    const unsigned max_blocks = (unsigned)std::max(1, c->n_cus) * 8;
    auto blocks_of = [&](uint64_t n_items) { return std::min<unsigned>(blocks_for(n_items * 64), max_blocks); };

    const int rc = R.run(&S.pairs_ms, &S.count_ms, &S.chunks, [&](const RecordChunk &ch) -> int {
      // ---- before: room for the chunk's items ----
      const uint64_t n_it = c->h_item_off[ch.r1] - c->h_item_off[ch.r0];
      HIP_TRY(c, grow(d_mask, n_it));
      HIP_TRY(c, grow(d_rows, n_it));
      HIP_TRY(c, grow(d_row_off, n_it));
      HIP_TRY(c, grow(d_bytes, n_it));  // (zeros where no text is wanted of the device)
      if (want_text && !all_host) HIP_TRY(c, grow(d_byte_off, n_it));
      HIP_TRY(c, grow(d_scan, std::max<size_t>(text_scan_temp_bytes(n_it), 1)));
      HIP_TRY(c, hipMemsetAsync(d_meta.p, 0, 3 * sizeof(uint64_t), st));
      A.mask = d_mask.p;
      A.rows = d_rows.p;
      A.bytes = d_bytes.p;
      A.row_off = d_row_off.p;
      A.byte_off = d_byte_off.p;
      A.T.needs_host = reinterpret_cast<int *>(d_meta.p + 2);
      A.T.out_base = ch.out_base;
      A.text = (want_text && !all_host) ? 1 : 0;
      return NGSLD_OK;
    }, [&](const RecordChunk &ch, const ngsld_item *items, uint64_t n_items) {
      // ---- count, per slice ----
      A.T.items = items;
      A.T.n_items = n_items;
      A.item0 = (uint64_t)(items - (c->d_items.p + c->h_item_off[ch.r0]));
      hipLaunchKernelGGL(count_kernel, dim3(blocks_of(n_items)), dim3(256), 0, st, A);
    }, [&](const RecordChunk &ch) -> int {
      // ---- after: scan over the whole chunk, the totals, room for the rows, write per slice, the sink ----
      const uint64_t i0 = c->h_item_off[ch.r0], n_it = c->h_item_off[ch.r1] - i0;
      const bool dev_text_wanted = want_text && !all_host;
      HIP_TRY(c, hipEventRecord(ev.a, st));
      HIP_TRY(c, text_scan(d_scan.p, d_scan.n, d_rows.p, d_row_off.p, n_it, d_meta.p, st));
      if (dev_text_wanted) HIP_TRY(c, text_scan(d_scan.p, d_scan.n, d_bytes.p, d_byte_off.p, n_it, d_meta.p + 1, st));
      HIP_TRY(c, hipEventRecord(ev.b, st));
      uint64_t meta[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(meta, d_meta.p, sizeof(meta), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, ev.add_elapsed(&S.scan_ms));
      const uint64_t rows = meta[0];
      if (rows == 0) return NGSLD_OK;
      if (rows > ch.pairs) return fail(c, NGSLD_ERR_INVALID, "linked pairs: more rows than pairs in a chunk (internal error)");
      const bool host = want_text && (all_host || (meta[2] & 0xffffffffull) != 0);
      const bool dev_text = want_text && !host;
      const uint64_t bytes = dev_text ? meta[1] : 0;
      HIP_TRY(c, grow(d_s1, rows));
      HIP_TRY(c, grow(d_s2, rows));
      HIP_TRY(c, grow(d_std, rows));
      if (ext) HIP_TRY(c, grow(d_ext, rows));
      if (dev_text) HIP_TRY(c, grow(d_text, bytes));
      A.s1 = d_s1.p;
      A.s2 = d_s2.p;
      A.out_std = d_std.p;
      A.out_ext = ext ? d_ext.p : nullptr;
      A.out_text = d_text.p;
      A.text = dev_text ? 1 : 0;
      const uint64_t max_items = record_slice_items();
      HIP_TRY(c, hipEventRecord(ev.a, st));
      for (uint64_t off = 0; off < n_it; off += max_items) {
        A.T.items = c->d_items.p + i0 + off;
        A.T.n_items = std::min<uint64_t>(max_items, n_it - off);
        A.item0 = off;
        hipLaunchKernelGGL(write_kernel, dim3(blocks_of(A.T.n_items)), dim3(256), 0, st, A);
        HIP_TRY(c, hipGetLastError());
      }
      HIP_TRY(c, hipEventRecord(ev.b, st));
      const bool copy_rec = want_rec || host;
      if (copy_rec) {
        HIP_TRY(c, grow(h_s1, rows));
        HIP_TRY(c, grow(h_s2, rows));
        HIP_TRY(c, grow(h_std, rows));
        if (ext) HIP_TRY(c, grow(h_ext, rows));
        HIP_TRY(c, hipMemcpyAsync(h_s1.p, d_s1.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_s2.p, d_s2.p, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_std.p, d_std.p, rows * sizeof(ngsld_rec_std), hipMemcpyDeviceToHost, st));
        if (ext) HIP_TRY(c, hipMemcpyAsync(h_ext.p, d_ext.p, rows * sizeof(ngsld_rec_ext), hipMemcpyDeviceToHost, st));
      }
      if (dev_text) {
        HIP_TRY(c, grow(h_text, bytes));
        HIP_TRY(c, hipMemcpyAsync(h_text.p, d_text.p, bytes, hipMemcpyDeviceToHost, st));
      }
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, ev.add_elapsed(&S.write_ms));

      ngsld_linked_batch b{};
      b.n = rows;
      if (want_rec) {
        b.s1 = h_s1.p;
        b.s2 = h_s2.p;
        b.std = h_std.p;
        b.ext = ext ? h_ext.p : nullptr;
      }
      if (host) {
        // the host TSV formatter over the compacted records, dist as the host writer has it: the gaps added one by one from s1
        host_text.clear();
        uint64_t cur_s1 = UINT64_MAX, cur_s2 = 0;
        double dist = 0;
        for (uint64_t r = 0; r < rows; ++r) {
          const uint64_t s1 = h_s1.p[r], s2 = h_s2.p[r];
          if (s1 != cur_s1) {
            cur_s1 = s1;
            cur_s2 = s1;
            dist = 0;
          }
          while (cur_s2 < s2) dist += c->h_pos_dist[++cur_s2];
          const size_t len = ngsld_host_format_pair(row_buf.data(), row_buf.size(), labels ? labels[s1] : nullptr, labels ? labels[s2] : nullptr,
                                                    dist, &h_std.p[r], ext ? &h_ext.p[r] : nullptr, c->h_maf[s1], c->h_maf[s2]);
          if (len == 0) return fail(c, NGSLD_ERR_INVALID, "linked pairs: a row beyond the host formatter's buffer (internal error)");
          host_text.append(row_buf.data(), len);
        }
        S.host_rows += rows;
        b.text = host_text.data();
        b.text_len = host_text.size();
      } else if (dev_text) {
        b.text = h_text.p;
        b.text_len = bytes;
      }
      S.rows += rows;
      S.text_bytes += b.text_len;
      const int src = sink(user, &b);
      if (src != 0) {
        (void)fail(c, NGSLD_ERR_SINK, "the linked pairs sink returned non-zero");
        return src;
      }
      return NGSLD_OK;
    });
    if (rc != NGSLD_OK) return rc;
  }
  S.kernel_ms = S.count_ms + S.scan_ms + S.write_ms;
  S.total_ms = ms_since(t_all);
  copy_stats(stats, S);
  return NGSLD_OK;
} NGSLD_CATCH(c)

}  // extern "C"
