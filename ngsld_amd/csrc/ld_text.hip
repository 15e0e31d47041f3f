// ld_text.hip -- the TSV rows of a batch, formatted on the device (gfx950).
//
// What it replaces: calc_pair_LD's fprintf block (ngsLD.cpp:310-352) -- on the host that is
// ngsld_host_write_batch (host_io.cpp), whose bytes this file reproduces exactly: same "%f" / "%.0f" rule (the
// EXACT binary value rounded half-to-even at the decimal, as glibc prints it), "-nan" / "inf", the float chi2 of
// ngsLD.cpp:328-333, the literal "0.000000" of the loglike column.  At kernel rates the text is the bulk of an
// end-to-end run (9.9e7 extended rows = 15 GB): formatted here it costs a few tens of milliseconds and the host
// only writes bytes.
//
// A row's text itself is format_row (ld_text_row.h, shared with linked.hip).  Two passes over the batch's pairs, one thread per candidate of an item (ld_records.h): lengths, then (after an
// exclusive prefix sum, hipCUB) the rows at their final offsets -- rows come out in (s1, s2) order, byte for byte what the
// host writer produces.  A value outside the fast path of the formatter (>= 2^52, or a quotient beyond 63 bits: only absurd D' /
// chi2 of degenerate pairs get there) raises needs_host and the caller falls back to the records for that batch.
#include <hipcub/hipcub.hpp>

#include "ld_fmt.h"
#include "ld_records.h"
#include "ld_text.h"
#include "ld_text_row.h"

#ifndef NGSLD_TEXT_WORDS
#define NGSLD_TEXT_WORDS 1  // build-time A/B switch
#endif

namespace ngsld {
namespace {

template <bool WRITE>
__global__ __launch_bounds__(256) void text_kernel(TextArgs A) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i = t >> 6;
  const uint32_t c = (uint32_t)(t & 63u);
  if (i >= A.n_items) return;
  const ngsld_item it = A.items[i];
  if (c >= it.count || !((it.mask >> c) & 1ull)) return;  // ngsLD.cpp:270-282: not a computed pair
  const uint64_t k = record_of(it, c, A.out_base);
  const uint32_t s1 = it.s1, s2 = it.s2_begin + c;
  if (WRITE && A.text_cap != 0 && A.offs[k] + A.lens[k] > A.text_cap) {
    *A.overflow = 1;
    return;
  }
  if (WRITE && NGSLD_TEXT_WORDS) {
    WordWriter w(A.text + A.offs[k]);
    (void)format_row(w, A, s1, s2, k);
    w.finish();
  } else if (WRITE) {
    Writer w{A.text + A.offs[k]};
    (void)format_row(w, A, s1, s2, k);
  } else {
    Counter n;
    if (!format_row(n, A, s1, s2, k)) atomicExch(A.needs_host, 1);
    A.lens[k] = n.n;
  }
}

// Rows whose records were replaced (exact-order replay): their lengths again.  changed is set when one differs from the
// length pass -- only then do the prefix sums have to be taken again (a replayed record moves a sixth decimal, or turns a
// rounded zero's sign: the row's length changes once in a few thousand replays).
__global__ void text_relength_kernel(TextArgs A, const uint64_t *rec, const uint32_t *s1, const uint32_t *s2, uint64_t n,
                                     uint64_t *changed) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint64_t k = rec[t];
  Counter c;
  if (!format_row(c, A, s1[t], s2[t], k)) atomicExch(A.needs_host, 1);
  if (A.lens[k] != c.n) {
    A.lens[k] = c.n;
    *changed = 1;
  }
}

__global__ void text_total_kernel(const uint64_t *lens, const uint64_t *offs, uint64_t n, uint64_t *total) {
  *total = n ? offs[n - 1] + lens[n - 1] : 0;
}

hipError_t launch(const TextArgs &a, hipStream_t stream, bool write) {
  // one thread per candidate; item lists of any length go out in launches of at most 2^22 workgroups (see
  // launch_pair_kernel: gridDim.x * blockDim.x has to stay below 2^32)
  const uint64_t max_items = (1ull << 22) * 4;
  for (uint64_t off = 0; off < a.n_items; off += max_items) {
    TextArgs b = a;
    b.items = a.items + off;
    b.n_items = a.n_items - off < max_items ? a.n_items - off : max_items;
    const unsigned blocks = (unsigned)((b.n_items * 64 + 255) / 256);
    if (write)
      hipLaunchKernelGGL(text_kernel<true>, dim3(blocks), dim3(256), 0, stream, b);
    else
      hipLaunchKernelGGL(text_kernel<false>, dim3(blocks), dim3(256), 0, stream, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_text_lengths(const TextArgs &a, hipStream_t stream) { return launch(a, stream, false); }
hipError_t launch_text_relength(const TextArgs &a, const uint64_t *rec, const uint32_t *s1, const uint32_t *s2, uint64_t n,
                                uint64_t *changed, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(text_relength_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, a, rec, s1, s2, n, changed);
  return hipGetLastError();
}
hipError_t launch_text_write(const TextArgs &a, hipStream_t stream) { return launch(a, stream, true); }

size_t text_scan_temp_bytes(uint64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n);
  return bytes;
}

hipError_t text_scan(void *temp, size_t temp_bytes, const uint64_t *lens, uint64_t *offs, uint64_t n, uint64_t *total,
                     hipStream_t stream) {
  if (n > 0x7fffffffull) return hipErrorInvalidValue;
  if (n) {
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, lens, offs, (int)n, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(text_total_kernel, dim3(1), dim3(1), 0, stream, lens, offs, n, total);
  return hipGetLastError();
}

}  // namespace ngsld
