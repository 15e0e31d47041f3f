// engine_replay.hip -- exact-order replay (replay.h): the pairs the kernels flagged are re-evaluated in the reference's own
// operation order and their records overwritten -- in the host buffers of a record batch, or on the device (text batches,
// ngsld_run_device) through a small scatter kernel.
#include "engine.h"

namespace ngsld {
namespace eng {

// The read-back stream of the exact-order replay (see ngsld_ctx::replay_stream); the copy stream where it cannot be had.
hipStream_t replay_stream_of(ngsld_ctx *c) {
  std::lock_guard<std::mutex> g(c->replay_stream_mu);
  if (c->replay_stream == nullptr && hipStreamCreateWithFlags(&c->replay_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    c->replay_stream = nullptr;
    return c->copy_stream;
  }
  return c->replay_stream;
}

// Host threads this process may really run on: the affinity mask cut by the cgroup CPU quota (a lease that shows 256 CPUs
// and grants 16 is common); what the exact-order replay spreads its pairs over when nothing else was asked for.
unsigned usable_threads() {
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) {
    const int k = CPU_COUNT(&set);
    if (k > 0) n = (unsigned)k;
  }
  if (FILE *fh = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char a[64] = "";
    double period = 0;
    if (std::fscanf(fh, "%63s %lf", a, &period) == 2 && std::strcmp(a, "max") != 0 && period > 0) {
      const double q = std::atof(a) / period;
      if (q >= 1.0 && q < (double)n) n = (unsigned)(q + 0.5);
    }
    std::fclose(fh);
  }
  return n ? n : 1u;
}

__global__ void patch_records_kernel(const uint64_t *idx, uint64_t n, const ngsld_rec_std *src_std,
                                     const ngsld_rec_ext *src_ext, ngsld_rec_std *dst_std, ngsld_rec_ext *dst_ext) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  dst_std[idx[k]] = src_std[k];
  if (dst_ext != nullptr) dst_ext[idx[k]] = src_ext[k];
}

// (s1, s2) of plan records, on the device: what locate_record below does on the host copy of the items -- which a run that
// leaves its records on the device never needs otherwise (configs[3]: 7.8e7 items, 2.5 GB to copy and hold for a few
// hundred flagged pairs: 155 ms of its one 12 s step)
__device__ inline void locate_record_on_device(uint64_t r, const uint64_t *row_off, const uint64_t *item_off, const Item *items,
                                               uint32_t n_sites, uint32_t *s1, uint32_t *s2) {
  *s1 = *s2 = 0xffffffffu;
  uint32_t lo = 0, hi = n_sites;  // largest row with row_off[row] <= r
  while (lo + 1 < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (row_off[mid] <= r) lo = mid; else hi = mid;
  }
  uint64_t il = item_off[lo], ih = item_off[lo + 1];
  if (il >= ih) return;
  while (il + 1 < ih) {
    const uint64_t mid = il + (ih - il) / 2;
    if (items[mid].first_record <= r) il = mid; else ih = mid;
  }
  const Item it = items[il];
  uint64_t k = r - it.first_record, m = it.mask;
  if (k >= (uint64_t)__popcll(m)) return;
  while (k--) m &= m - 1;
  *s1 = it.s1;
  *s2 = it.s2_begin + (uint32_t)(__ffsll((unsigned long long)m) - 1);
}

__global__ void locate_records_kernel(const uint64_t *rec, uint64_t n, uint64_t base, const uint64_t *row_off,
                                      const uint64_t *item_off, const Item *items, uint32_t n_sites, uint32_t *s1, uint32_t *s2) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  locate_record_on_device(base + rec[t], row_off, item_off, items, n_sites, &s1[t], &s2[t]);
}

int ensure_host_items(ngsld_ctx *c) {  // the host copy of the plan's items, fetched on first use
  if (c->h_items.size() != c->n_items) {
    c->h_items.resize(c->n_items);
    if (c->n_items)
      HIP_TRY(c, hipMemcpy(c->h_items.data(), c->d_items.p, c->n_items * sizeof(Item), hipMemcpyDeviceToHost));
  }
  return NGSLD_OK;
}

// (s1, s2) of the plan's record `rec` (h_items must be present)
bool locate_record(const ngsld_ctx *c, uint64_t rec, uint32_t *s1, uint32_t *s2) {
  const auto &off = c->h_row_off;
  const uint64_t row = (uint64_t)(std::upper_bound(off.begin(), off.end(), rec) - off.begin()) - 1;
  if (row >= c->n_sites) return false;
  uint64_t lo = c->h_item_off[row], hi = c->h_item_off[row + 1];
  while (lo + 1 < hi) {  // last item of the row whose first record is <= rec
    const uint64_t mid = (lo + hi) / 2;
    if (c->h_items[mid].first_record <= rec) lo = mid; else hi = mid;
  }
  if (lo >= hi) return false;
  const Item &it = c->h_items[lo];
  uint64_t k = rec - it.first_record, m = it.mask;
  if (k >= (uint64_t)__builtin_popcountll(m)) return false;
  while (k--) m &= m - 1;  // drop the k lowest set bits
  *s1 = it.s1;
  *s2 = it.s2_begin + (uint32_t)__builtin_ctzll(m);
  return true;
}

// One site in the reference's arithmetic: from the caller's raw values when a source is registered, otherwise from the
// device's own planes (already normalised normal-space values; exact for ngsld_set_geno_lkl input).
int fetch_replay_site(ngsld_ctx *c, uint64_t s, std::vector<double> &tmp, ReplaySite *out) {
  const uint64_t n = c->n_ind;
  const double *v = c->replay_matrix != nullptr ? c->replay_matrix + s * 3 * n : nullptr;  // the caller's own array, read in place
  if (v == nullptr && c->replay_read != nullptr) {
    tmp.resize(3 * n);
    std::lock_guard<std::mutex> g(c->replay_mu);
    if (c->replay_read(c->replay_user, s, 1, tmp.data()) != 0) return NGSLD_ERR_SINK;
    v = tmp.data();
  }
  if (v != nullptr) {
    if (c->normalised)
      replay_site_from_lkl(v, c->h_maf[s], n, out);
    else
      replay_site_from_raw(v, n, c->gopts, out);
    return NGSLD_OK;
  }
  // (pinned staging: a pageable copy would be staged by the runtime; while a pair kernel of the next batch has the device
  // this read-back can still wait for it -- callers that care register a source)
  tmp.resize(3 * n);
  double *lkl = tmp.data();
  {
    std::lock_guard<std::mutex> g(c->replay_mu);
    if (hipSetDevice(c->device) != hipSuccess || c->h_site_stage.resize(3ull * c->np) != hipSuccess) return NGSLD_ERR_DEVICE;
    hipStream_t rs = replay_stream_of(c);
    if (hipMemcpyAsync(c->h_site_stage.p, c->d_planes.p + s * 3ull * c->np, 3ull * c->np * sizeof(double),
                       hipMemcpyDeviceToHost, rs) != hipSuccess ||
        hipStreamSynchronize(rs) != hipSuccess)
      return NGSLD_ERR_DEVICE;
    const double *planes = c->h_site_stage.p;
    for (uint64_t i = 0; i < n; ++i)
      for (int g = 0; g < 3; ++g) lkl[3 * i + g] = planes[(uint64_t)g * c->np + i];
  }
  replay_site_from_lkl(lkl, c->h_maf[s], n, out);
  return NGSLD_OK;
}

// The flagged records of a launch of n records, in increasing order.  h_head: the head of its flag buffer (counter + the
// first `cap` record indices) in host memory -- it travels with the batch, or is copied on the launch's own stream
// right behind the kernels (a copy issued later, while the next batch's pair kernel has the device, can wait for that
// kernel: measured 43 ms).  Only a launch that flagged more pairs than the list holds has its bitmap fetched from d_flags,
// on the replay stream (the kernels that set it are complete when this is called).
int flagged_records(ngsld_ctx *c, const uint32_t *h_head, const uint32_t *d_flags, uint32_t cap, uint64_t n,
                    std::vector<uint64_t> &recs, bool dev_applied) {
  recs.clear();
  const uint32_t count = h_head[0];
  if (count == 0) return NGSLD_OK;
  const size_t words = flag_bitmap_words(n);
  auto from_bitmap = [&](size_t first_word, uint32_t expect) -> int {
    HIP_TRY(c, c->h_flag_bits.resize(words ? words : 1));
    hipStream_t rs = replay_stream_of(c);
    HIP_TRY(c, hipMemcpyAsync(c->h_flag_bits.p, d_flags + first_word, words * sizeof(uint32_t), hipMemcpyDeviceToHost, rs));
    HIP_TRY(c, hipStreamSynchronize(rs));
    const uint32_t *bits = c->h_flag_bits.p;
    recs.reserve(expect);
    for (uint64_t w = 0; w < words; ++w)
      for (uint32_t m = bits[w]; m; m &= m - 1) {
        const uint64_t r = w * 32 + (uint64_t)__builtin_ctz(m);
        if (r < n) recs.push_back(r);
      }
    return NGSLD_OK;
  };
  if (h_head[7] != 0) dev_applied = true;  // (called genotypes: the launch overflowed its list and the device took all of it, ld_replay.hip)
  if (dev_applied) {
    // likelihood matrices, device-side replay behind the launch (ld_replay_lkl.hip): it settled every flagged pair but the
    // host-only ones -- head[2] says how many --, and those have a bitmap of their own
    c->replayed_on_device += h_head[2];
    c->replayed_pairs += h_head[2];
    const uint32_t host_only = h_head[1];
    if (host_only == 0) return NGSLD_OK;
    if (host_only <= kFlagHostCap) {  // (their own list names them)
      const uint64_t *list = reinterpret_cast<const uint64_t *>(h_head + kFlagListAt + 2u * cap);
      recs.assign(list, list + host_only);
      std::sort(recs.begin(), recs.end());
      while (!recs.empty() && recs.back() >= n) recs.pop_back();
      return NGSLD_OK;
    }
    return from_bitmap((size_t)flag_head_words(cap) + words, host_only);
  }
  if (count <= cap) {
    const uint64_t *list = reinterpret_cast<const uint64_t *>(h_head + kFlagListAt);
    recs.reserve(count);
    uint64_t on_device = 0;
    for (uint32_t k = 0; k < count; ++k) {
      if (list[k] & kFlagDone) {  // the device-side replay (ld_replay.hip) has rewritten this record already
        ++on_device;
        continue;
      }
      recs.push_back(list[k] & kFlagIndexMask);
    }
    c->replayed_on_device += on_device;
    c->replayed_pairs += on_device;
    std::sort(recs.begin(), recs.end());  // (the order the atomics landed in is not the record order)
    while (!recs.empty() && recs.back() >= n) recs.pop_back();
    return NGSLD_OK;
  }
  return from_bitmap(flag_head_words(cap), count);
}

// The pairs (s1[k], s2[k]), k < n, in the reference's operation order on the host's threads.
int replay_pairs_on_host(ngsld_ctx *c, const uint32_t *s1v, const uint32_t *s2v, size_t n, ngsld_rec_std *out_std, ngsld_rec_ext *out_ext) {
  if (n == 0) return NGSLD_OK;
  const bool ign = c->params.ignore_miss_data != 0;
  int T = c->replay_threads > 0 ? c->replay_threads : (int)std::min<unsigned>(32u, usable_threads());
  if ((uint64_t)T > n) T = (int)n;  // (a launch of 1e8 pairs flags a few dozen: sixteen per thread left them to two threads, 2.6 ms)
  if (T < 1) T = 1;
  std::vector<int> rcs((size_t)T, NGSLD_OK), stats((size_t)T, NGSLD_OK);
  std::vector<uint64_t> sites_done((size_t)T, 0);
  auto work = [&](int t) {
    const size_t k0 = n * (size_t)t / (size_t)T, k1 = n * (size_t)(t + 1) / (size_t)T;
    // records come in (s1, s2) order: the row's site is kept, the partners go through a bounded cache
    const size_t cache_cap = std::max<size_t>(64, (256ull << 20) / (32 * c->n_ind + 64));
    std::unordered_map<uint32_t, ReplaySite> cache;
    std::vector<double> tmp;
    ReplaySite row;
    uint32_t row_site = 0xffffffffu;
    try {
      for (size_t k = k0; k < k1; ++k) {
        const uint32_t s1 = s1v[k], s2 = s2v[k];
        if (s1 >= c->n_sites || s2 >= c->n_sites) {
          rcs[(size_t)t] = NGSLD_ERR_INVALID;
          return;
        }
        if (s1 != row_site) {
          const int rc = fetch_replay_site(c, s1, tmp, &row);
          if (rc != NGSLD_OK) { rcs[(size_t)t] = rc; return; }
          row_site = s1;
          ++sites_done[(size_t)t];
        }
        auto hit = cache.find(s2);
        if (hit == cache.end()) {
          if (cache.size() >= cache_cap) cache.clear();
          hit = cache.emplace(s2, ReplaySite()).first;
          const int rc = fetch_replay_site(c, s2, tmp, &hit->second);
          if (rc != NGSLD_OK) { rcs[(size_t)t] = rc; return; }
          ++sites_done[(size_t)t];
        }
        replay_pair(row, hit->second, c->n_ind, ign, &out_std[k], out_ext ? &out_ext[k] : nullptr, &stats[(size_t)t]);
      }
    } catch (...) {
      rcs[(size_t)t] = NGSLD_ERR_NOMEM;
    }
  };
  c->replay_pool.run(T, work);
  for (int t = 0; t < T; ++t) {
    if (rcs[(size_t)t] != NGSLD_OK)
      return fail(c, rcs[(size_t)t], rcs[(size_t)t] == NGSLD_ERR_SINK ? "the replay source callback failed"
                                                                      : "exact-order replay failed");
    if (stats[(size_t)t] == NGSLD_ERR_MAF_RANGE) {
      const int v = NGSLD_ERR_MAF_RANGE;
      HIP_TRY(c, hipMemcpy(c->d_status.p, &v, sizeof(int), hipMemcpyHostToDevice));
    }
    c->replayed_sites += sites_done[(size_t)t];
  }
  return NGSLD_OK;
}

// Records `recs` (indices into a launch whose record 0 is the plan's record `base`, increasing) are replayed; the new
// records go to h_std / h_ext (host buffers of the batch) or, when those are null, to d_std / d_ext on stream st (synchronised).
int replay_flagged(ngsld_ctx *c, const std::vector<uint64_t> &recs, uint64_t base, ngsld_rec_std *h_std,
                   ngsld_rec_ext *h_ext, ngsld_rec_std *d_std, ngsld_rec_ext *d_ext, hipStream_t st,
                   std::vector<uint32_t> *sites1, std::vector<uint32_t> *sites2) {
  Range range_("ngsld:exact-order replay (host)");
  if (recs.empty()) return NGSLD_OK;
  // which pairs these records are: from the host copy of the plan's items where the run has one anyway (the sink path), from
  // the device's otherwise
  const bool have_items = c->h_items.size() == c->n_items;
  std::vector<uint32_t> loc_s1(recs.size()), loc_s2(recs.size());
  if (!have_items) {
    hipStream_t ls = st != nullptr ? st : replay_stream_of(c);
    HIP_TRY(c, c->d_patch_idx.resize(recs.size()));
    HIP_TRY(c, c->d_patch_s1.resize(recs.size()));
    HIP_TRY(c, c->d_patch_s2.resize(recs.size()));
    HIP_TRY(c, hipMemcpyAsync(c->d_patch_idx.p, recs.data(), recs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ls));
    hipLaunchKernelGGL(locate_records_kernel, dim3((unsigned)((recs.size() + 63) / 64)), dim3(64), 0, ls, c->d_patch_idx.p,
                       (uint64_t)recs.size(), base, c->d_row_off.p, c->d_item_off.p, c->d_items.p, (uint32_t)c->n_sites,
                       c->d_patch_s1.p, c->d_patch_s2.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(loc_s1.data(), c->d_patch_s1.p, recs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ls));
    HIP_TRY(c, hipMemcpyAsync(loc_s2.data(), c->d_patch_s2.p, recs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ls));
    HIP_TRY(c, hipStreamSynchronize(ls));
  } else {
    for (size_t k = 0; k < recs.size(); ++k)
      if (!locate_record(c, base + recs[k], &loc_s1[k], &loc_s2[k])) loc_s1[k] = loc_s2[k] = 0xffffffffu;
  }
  for (size_t k = 0; k < recs.size(); ++k)
    if (loc_s1[k] == 0xffffffffu || loc_s2[k] == 0xffffffffu) return fail(c, NGSLD_ERR_INVALID, "exact-order replay failed");
  const bool ext = (h_std != nullptr ? (void *)h_ext : (void *)d_ext) != nullptr;
  std::vector<ngsld_rec_std> out_std(recs.size());
  std::vector<ngsld_rec_ext> out_ext(ext ? recs.size() : 0);
  const int rcp = replay_pairs_on_host(c, loc_s1.data(), loc_s2.data(), recs.size(), out_std.data(), ext ? out_ext.data() : nullptr);
  if (rcp != NGSLD_OK) return rcp;
  if (sites1) *sites1 = loc_s1;  // (the pairs' sites, for callers that format the replayed rows again)
  if (sites2) *sites2 = loc_s2;
  c->replayed_pairs += recs.size();
  c->host_replayed_total += recs.size();
  if (h_std != nullptr) {
    for (size_t k = 0; k < recs.size(); ++k) {
      h_std[recs[k]] = out_std[k];
      if (ext && h_ext != nullptr) h_ext[recs[k]] = out_ext[k];
    }
    return NGSLD_OK;
  }
  HIP_TRY(c, c->d_patch_idx.resize(recs.size()));
  HIP_TRY(c, c->d_patch_std.resize(recs.size()));
  if (ext) HIP_TRY(c, c->d_patch_ext.resize(recs.size()));
  HIP_TRY(c, hipMemcpyAsync(c->d_patch_idx.p, recs.data(), recs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(c->d_patch_std.p, out_std.data(), recs.size() * sizeof(ngsld_rec_std), hipMemcpyHostToDevice, st));
  if (ext)
    HIP_TRY(c, hipMemcpyAsync(c->d_patch_ext.p, out_ext.data(), recs.size() * sizeof(ngsld_rec_ext), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(patch_records_kernel, dim3((unsigned)((recs.size() + 255) / 256)), dim3(256), 0, st, c->d_patch_idx.p,
                     (uint64_t)recs.size(), c->d_patch_std.p, ext ? c->d_patch_ext.p : nullptr, d_std, ext ? d_ext : nullptr);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));  // the pageable source vectors go out of scope
  return NGSLD_OK;
}

// Text batches: which pair each record the batch leaves to the host is, and where its row lies in the batch's text -- written
// into pinned host memory right behind the batch's row lengths and prefix sums, on the pair kernel's stream.  With it the host
// settles such a batch without submitting anything to the device (engine_run.hip): the kernels that located the pairs, patched
// the records, took the rows' lengths again and wrote the text again stood -- in a hardware queue shared with the compute
// streams -- behind the pair kernels of the next two batches, and the loop ran dry behind them (GPU_MAX_HW_QUEUES=1 / 2:
// 0.67-0.69 s for configs[2]'s loop against 0.556, profiles/r05/hw_queues_ab.txt).
__global__ void flag_rows_to_host_kernel(const uint32_t *flags, uint32_t cap, int dev_applied, const uint64_t *offs, const uint64_t *lens,
                                         uint64_t n_records, uint64_t base, const uint64_t *row_off, const uint64_t *item_off, const Item *items,
                                         uint32_t n_sites, FlagRow *rows) {
  // (flags[7]: called genotypes, the launch overflowed its list and the device took all of it -- flagged_records)
  const bool host_list = dev_applied != 0 || flags[7] != 0;
  const uint32_t n = host_list ? flags[1] : flags[0];
  if (n > kFlagRowsCap || n > (host_list ? kFlagHostCap : cap)) return;
  const uint64_t *list = reinterpret_cast<const uint64_t *>(flags + kFlagListAt + (host_list ? 2u * cap : 0u));
  for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) {
    FlagRow r{};
    r.rec = list[j] & kFlagIndexMask;
    r.s1 = r.s2 = 0xffffffffu;
    if (r.rec < n_records) {
      r.off = offs[r.rec];
      r.len = (uint32_t)lens[r.rec];
      locate_record_on_device(base + r.rec, row_off, item_off, items, n_sites, &r.s1, &r.s2);
    }
    rows[j] = r;
  }
}

int send_flag_rows(ngsld_ctx *c, const uint32_t *d_flags, uint32_t cap, bool dev_applied, const uint64_t *d_offs, const uint64_t *d_lens,
                   uint64_t n_records, uint64_t base, FlagRow *h_rows, hipStream_t st) {
  FlagRow *dev_view = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer((void **)&dev_view, h_rows, 0));
  hipLaunchKernelGGL(flag_rows_to_host_kernel, dim3(1), dim3(64), 0, st, d_flags, cap, dev_applied ? 1 : 0, d_offs, d_lens, n_records, base,
                     c->d_row_off.p, c->d_item_off.p, c->d_items.p, (uint32_t)c->n_sites, dev_view);
  HIP_TRY(c, hipGetLastError());
  return NGSLD_OK;
}

// The head of a launch's flag buffer -- the counters, the listed pairs, the host-only pairs -- written into the batch's pinned
// host buffer by a one-workgroup kernel on the launch's own stream.  NOT hipMemcpyAsync: a copy of this size goes to an SDMA
// queue, where it waits for the kernels before it on its stream -- and everything queued behind it on that engine waits with
// it, whatever stream it came from: the 86 MB D2H copy of the previous batch's text (copy stream) did not start until the pair
// kernel AND the device-side replay of the next batch had finished (rocprofv3 --memory-copy-trace, profiles/r05): 8.7 ms a
// text batch instead of 7.3 on un-called input, 2.9 instead of 2.5 on the headline's.
__global__ void flag_head_to_host_kernel(const uint32_t *flags, uint32_t *h_head, uint32_t cap, int with_list) {
  const uint32_t count = flags[0], host_only = flags[1];
  if (threadIdx.x < kFlagListAt) h_head[threadIdx.x] = flags[threadIdx.x];
  // (with_list == 0: a device-side replay has been through the launch -- the host reads the counters and the host-only list)
  const uint32_t n_list = with_list ? 2u * (count < cap ? count : cap) : 0u, n_host = 2u * (host_only < kFlagHostCap ? host_only : kFlagHostCap);
  for (uint32_t w = threadIdx.x; w < n_list; w += blockDim.x) h_head[kFlagListAt + w] = flags[kFlagListAt + w];
  const uint32_t at = kFlagListAt + 2u * cap;
  for (uint32_t w = threadIdx.x; w < n_host; w += blockDim.x) h_head[at + w] = flags[at + w];
}

int send_flag_head(ngsld_ctx *c, const uint32_t *d_flags, uint32_t *h_head, uint32_t cap, hipStream_t st, bool with_list) {
  uint32_t *dev_view = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer((void **)&dev_view, h_head, 0));
  hipLaunchKernelGGL(flag_head_to_host_kernel, dim3(1), dim3(256), 0, st, d_flags, dev_view, cap, with_list ? 1 : 0);
  HIP_TRY(c, hipGetLastError());
  return NGSLD_OK;
}

// A flag buffer for n records with `cap` list entries, zeroed on `stream`.
int reset_flags(ngsld_ctx *c, DevBuf<uint32_t> &buf, uint64_t n, uint32_t cap, hipStream_t stream) {
  const size_t words = flag_words(n, cap), head = flag_head_words(cap);
  HIP_TRY(c, buf.resize(words));
  HIP_TRY(c, hipMemsetAsync(buf.p, 0, kFlagListAt * sizeof(uint32_t), stream));  // the counters (the list behind them needs no clearing)
  if (words > head)
    HIP_TRY(c, hipMemsetAsync(buf.p + head, 0, (words - head) * sizeof(uint32_t), stream));  // both bitmaps
  return NGSLD_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Likelihood matrices: the device-side replay (ld_replay_lkl.hip) on the exact store (exact_store.h)
// ---------------------------------------------------------------------------------------------------------------

bool lkl_device_eligible(const ngsld_ctx *c) {
  // (beyond 4,096 individuals the wavefront-per-pair kernel has no shape: the lanes take such cohorts -- where their copy of the
  // store cannot be had, ExactStore::start gives the matrix up to the host)
  return c->replay_on && c->replay_device && c->exact_mode != 0 && c->have_geno && c->cfg.kernel != kHard;
}

bool lkl_device_ready(const ngsld_ctx *c) { return lkl_device_eligible(c) && (c->store.started() || ExactStore::is_free(c)); }

int try_device_replay_lkl(ngsld_ctx *c, const ReplayLaunch &l, bool *applied, uint64_t need_sites) {
  *applied = false;
  RC_TRY(c->store.start(c));
  bool have = false;
  RC_TRY(c->store.wait(c, need_sites, &have));
  if (!have) return NGSLD_OK;
  RC_TRY(device_replay_lkl(c, l));
  *applied = true;
  return NGSLD_OK;
}

// The flagged pairs of a launch replayed on the device (likelihood matrices), on `st` behind the pair kernels that flagged
// them -- before the head of the flag buffer travels to the host, before text rows are formatted.  The store must be ready.
int device_replay_lkl(ngsld_ctx *c, const ReplayLaunch &l) {
  const auto [d_flags, cap, out_base, n, d_std, d_ext, st, flag_text, slot] = l;
  const ExactStore &store = c->store;
  if (!store.started() || d_flags == nullptr || n == 0) return NGSLD_OK;
  ReplayLklArgs a{};
  const size_t head = flag_head_words(cap), words = flag_bitmap_words(n);
  a.bits = d_flags + head;
  a.host_bits = d_flags + head + words;
  a.flags = d_flags;
  a.flag_cap = cap;
  a.flag_text = flag_text ? 1u : 0u;
  a.mean_e = c->d_mean.p;
  a.rsx = c->d_rsx.p;
  a.n_records = n;
  a.done = d_flags + 2;
  a.work = d_flags + 3;
  a.row_off = c->d_row_off.p;
  a.item_off = c->d_item_off.p;
  a.items = c->d_items.p;
  a.n_items = c->n_items;
  a.n_sites = (uint32_t)c->n_sites;
  a.rec_base = out_base;
  a.xplanes = store.planes(c);
  a.site_stride = 3ull * c->np;
  a.np = c->np;
  a.xmaf = store.maf(c);
  a.n_ind = (uint32_t)c->n_ind;
  a.ignore_miss = c->params.ignore_miss_data;
  a.out_std = d_std;
  a.out_ext = d_ext;
  a.status = c->d_status.p;
  a.xt_sites = c->n_sites;
  a.xdepth = store.lane_depth();
  a.xperm = store.lane_perm();
  // (a launch of a few hundred thousand records -- a text batch -- stays with the wavefront-per-pair kernel: a lane takes
  // milliseconds over ONE pair, four wavefronts to a SIMD, and such a launch has no second pair for most lanes: 6 ms a batch
  // against 4, profiles/r05/e2e_uncalled_lanes_on_text_batches.json)
  uint64_t lanes_from = 1ull << 22;
  // ... but cohorts beyond 512 individuals, where SEVERAL wavefronts share a pair and all of them wait for the four lanes'
  // chain (2,000 individuals: 6e6 replayed pairs/s), go to the lanes whatever the launch's size, with a cap on a lane's EM
  // steps so that the launch does not last as long as its slowest pair (what is over the cap is the wavefront kernel's)
  const uint32_t team_waves = replay_lkl_waves((uint32_t)c->n_ind);  // (0: beyond 4,096 individuals -- the lanes or nothing)
  const bool big_cohort = team_waves >= 2 || team_waves == 0;
  if (big_cohort) lanes_from = 0;
  if (team_waves == 0 && !store.has_lane_copy()) return fail(c, NGSLD_ERR_INVALID, "device-side replay without a kernel for this cohort");
  if (store.has_lane_copy() && (n >= lanes_from || team_waves == 0)) {
    // one lane per pair wherever the individual-major copy is there: the launch's bitmap becomes a list of located pairs (the
    // bits listed are cleared), the lanes work through it; what stays in the bitmap -- ill-conditioned Pearson moments, pairs
    // beyond the list -- is the wavefront-per-pair kernel's, as everything is without the copy
    ngsld_ctx::LaneScratch &ls = slot < 0 ? c->lane_scratch_dev : c->lane_scratch[slot];
    const uint64_t list_cap = std::min<uint64_t>(n, 1ull << 26);
    // (the lanes' scratch -- 40 bytes per record of the launch + the sort's own -- is something the run can do without: where the
    // device has no room for it the launch stays with the wavefront-per-pair kernel, or the host where that has no shape)
    if (ls.reserve(list_cap, c->n_sites)) {
      a.after_lanes = 1;
      HIP_TRY(c, launch_replay_expand(a, ls.list.p, list_cap, st));
      HIP_TRY(c, launch_replay_sort(a, ls.list.p, list_cap, ls.keys_a.p, ls.keys_b.p, ls.vals_a.p, ls.vals_b.p, ls.temp.p, ls.temp_bytes, st));
      int lane_waves = n >= (1ull << 22) ? 4 : 1;
      if (n < (1ull << 22) && team_waves != 0) {  // (no wavefront kernel to hand a long pair back to: no cap)
        a.lane_iter_cap = 12;
        if (const char *v = test_knob("LANE_ITER_CAP")) a.lane_iter_cap = (uint32_t)std::strtoul(v, nullptr, 10);  // (tests: hand-backs on every pair)
      }
      HIP_TRY(c, launch_replay_lanes(a, ls.list.p, ls.vals_b.p, store.lane_copy(), c->n_cus, lane_waves, st));
    }
  }
  HIP_TRY(c, team_waves == 0 ? launch_replay_leftover(a, st) : launch_replay_lkl(a, c->n_cus, st));
  return NGSLD_OK;
}

// Called-genotype matrices: the flagged pairs of a launch replayed on the device (ld_replay.hip), right behind the pair
// kernels on their stream -- before the head of the flag buffer travels to the host, before text rows are formatted.
int device_replay(ngsld_ctx *c, const ReplayLaunch &l) {
  const auto [d_flags, cap, out_base, n, d_std, d_ext, st, flag_text, slot] = l;
  if (!c->replay_on || !c->replay_device || c->cfg.kernel != kHard || d_flags == nullptr || n == 0) return NGSLD_OK;
  // A launch that flags more pairs than its list holds (every pair of a monomorphic called site): the bitmap is turned into a
  // list of located pairs and a second kernel works through that -- both leave at once unless the list did overflow
  ngsld_ctx::LaneScratch &ls = slot < 0 ? c->lane_scratch_dev : c->lane_scratch[slot];
  uint64_t list_cap = std::min<uint64_t>(n, 1ull << 26);
  if (const char *v = test_knob("REPLAY_LIST_CAP")) list_cap = std::min<uint64_t>(list_cap, std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)));  // tests: a list that overflows
  HIP_TRY(c, ls.list.resize(list_cap));
  ReplayHardArgs a{};
  a.list = ls.list.p;
  a.host_bits = d_flags + flag_head_words(cap) + flag_bitmap_words(n);
  a.flags = d_flags;
  a.flag_cap = cap;
  a.row_off = c->d_row_off.p;
  a.item_off = c->d_item_off.p;
  a.items = c->d_items.p;
  a.n_sites = (uint32_t)c->n_sites;
  a.rec_base = out_base;
  a.masks = c->d_hard_masks.p;
  a.words = c->mask_words;
  a.n_ind = (uint32_t)c->n_ind;
  a.ignore_miss = c->params.ignore_miss_data;
  // "no data" individuals: only call_geno's triple is the same arithmetic on every individual (gen_func.cpp:903-905); a
  // matrix that came called from elsewhere may hold any three equal values -- its pairs at sites with missing data stay
  // with the host, which has the caller's raw values
  // (text genotype files without --call_geno: the reader's own triple for a missing call, log(1/3) three times and then
  // post_prob -- another two constants; the prep pass has looked at every individual without data, engine.hip)
  a.miss_ok = (c->gopts.call_geno && !c->normalised) || c->missing_canonical ? 1 : 0;
  if (c->missing_canonical)
    replay_missing_constants_text(&a.u_lkl, &a.u_pp);
  else
    replay_missing_constants(&a.u_lkl, &a.u_pp);
  a.out_std = d_std;
  a.out_ext = d_ext;
  a.status = c->d_status.p;
  HIP_TRY(c, launch_replay_hard(a, n, st));
  {
    ReplayLklArgs x{};  // (what launch_replay_expand reads)
    x.bits = d_flags + flag_head_words(cap);
    x.host_bits = a.host_bits;
    x.n_records = n;
    x.flags = d_flags;
    x.flag_cap = cap;
    x.row_off = a.row_off;
    x.item_off = a.item_off;
    x.items = a.items;
    x.n_items = c->n_items;
    x.n_sites = a.n_sites;
    x.rec_base = out_base;
    x.rsx = c->d_rsx.p;
    x.n_ind = a.n_ind;
    x.only_if_overflow = 1;
    HIP_TRY(c, launch_replay_expand(x, ls.list.p, list_cap, st));
    HIP_TRY(c, launch_replay_hard_list(a, c->n_cus, st));
    // what the expansion could not list (a launch that flags more pairs than the list's 2^26 entries: only ngsld_run_device makes
    // launches that large) is still in the bitmap, and flags[7] tells the host that everything but the host-only pairs is done:
    // those pairs join the host-only bitmap and list (a no-op unless the launch overflowed)
    HIP_TRY(c, launch_replay_leftover(x, st));
  }
  return NGSLD_OK;
}

// Everything ngsld_run_device + the device-side replay allocate for a launch of n records, taken now -- all of it grow-only, so
// that a sequence of launches of up to n records (run_grouped: a small first group, then full ones) allocates once, before its
// first kernel, instead of freeing and allocating gigabytes between two groups (125 ms each, measured, with the device idle).
int reserve_device_run(ngsld_ctx *c, uint64_t n) {
  if (!c->replay_on || n == 0) return NGSLD_OK;
  const uint32_t cap = flag_cap_for(n);
  HIP_TRY(c, c->d_flags_dev.resize(flag_words(n, cap)));
  HIP_TRY(c, c->h_flags_dev.resize(flag_head_words(cap)));
  // (no room: the launches will find out themselves, and do without the lanes)
  if (lkl_device_eligible(c)) (void)c->lane_scratch_dev.reserve(std::min<uint64_t>(n, 1ull << 26), c->n_sites);
  return NGSLD_OK;
}

int finish_device_run(ngsld_ctx *c) {
  if (!c->dev_run.pending) return NGSLD_OK;
  c->dev_run.pending = false;
  const bool trace = std::getenv("NGSLD_TRACE") != nullptr;  // dev: where ngsld_finish_device's time goes, on stderr
  const auto t0 = std::chrono::steady_clock::now();
  auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  HIP_TRY(c, hipStreamSynchronize(c->dev_run.st));  // (the head of the flag buffer came over behind the kernels, ngsld_run_device)
  const double t_sync = ms();
  if (!c->replay_on || c->d_flags_dev.p == nullptr || c->h_flags_dev.p == nullptr) return NGSLD_OK;
  c->flagged_pairs = c->h_flags_dev.p[0];
  if (c->h_flags_dev.p[0] == 0) return NGSLD_OK;
  const uint64_t base = c->h_row_off[c->dev_run.s1_begin], n = c->h_row_off[c->dev_run.s1_end] - base;
  bool applied = c->dev_run.dev_applied;
  if (!applied && c->store.wanted(c, c->h_flags_dev.p[0] - c->h_flags_dev.p[1])) {
    // a likelihood matrix that flags more pairs than the host should replay: the exact store is built (once per matrix) and
    // the pairs are replayed on the device, behind the kernels on their stream
    const ReplayLaunch l{c->d_flags_dev.p, c->flag_cap_dev, base, n, c->dev_run.d_std, c->dev_run.d_ext, c->dev_run.st, c->dev_run_flag_text, -1};
    RC_TRY(try_device_replay_lkl(c, l, &applied, c->n_sites));
    if (applied) {
      RC_TRY(send_flag_head(c, c->d_flags_dev.p, c->h_flags_dev.p, c->flag_cap_dev, c->dev_run.st, false));
      HIP_TRY(c, hipStreamSynchronize(c->dev_run.st));
    }
  }
  const double t_dev = ms();
  std::vector<uint64_t> recs;
  RC_TRY(flagged_records(c, c->h_flags_dev.p, c->d_flags_dev.p, c->flag_cap_dev, n, recs, applied));
  const double t_list = ms();
  const int rcr = replay_flagged(c, recs, base, nullptr, nullptr, c->dev_run.d_std, c->dev_run.d_ext, c->dev_run.st);
  if (trace)
    std::fprintf(stderr, "[trace] finish_device: waited for the kernels %.2f ms, exact store + device replay %.2f ms, flag list %.2f ms "
                         "(%u flagged, %u on the device, %zu for the host), host replay + patch %.2f ms\n", t_sync, t_dev - t_sync,
                 t_list - t_dev, c->h_flags_dev.p[0], applied ? c->h_flags_dev.p[2] : 0u, recs.size(), ms() - t_list);
  return rcr;
}
}  // namespace eng
}  // namespace ngsld

extern "C" {

static int set_replay_source(ngsld_ctx *c, const double *matrix, ngsld_read_sites_fn read, void *user) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (!c->have_geno) return fail(c, NGSLD_ERR_INVALID, "set the genotype data before its replay source");
  c->store.stop();  // (the exact store is built from the source)
  c->replay_matrix = matrix;
  c->replay_read = read;
  c->replay_user = user;
  c->planned = false;  // a --min_maf tie is settled at plan time
  c->res.invalidate_for_new_plan();
  return NGSLD_OK;
}
int ngsld_set_replay_source(ngsld_ctx *c, ngsld_read_sites_fn read, void *user) { return set_replay_source(c, nullptr, read, user); }
int ngsld_set_replay_matrix(ngsld_ctx *c, const double *values) { return set_replay_source(c, values, nullptr, nullptr); }

int ngsld_set_replay(ngsld_ctx *c, int enable) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  c->replay_on = enable != 0;
  c->planned = false;
  c->res.invalidate_for_new_plan();
  return NGSLD_OK;
}

int ngsld_set_exact_store(ngsld_ctx *c, int mode) {
  if (c == nullptr || mode < 0 || mode > 2) return NGSLD_ERR_INVALID;
  c->exact_mode = mode;
  c->res.invalidate_for_new_plan();
  return NGSLD_OK;
}

int ngsld_replay_info(ngsld_ctx *c, ngsld_replay_stats_t *out) {
  if (c == nullptr || out == nullptr) return NGSLD_ERR_INVALID;
  out->pairs_flagged = c->flagged_pairs;
  out->pairs_replayed = c->replayed_pairs;
  out->pairs_on_device = c->replayed_on_device;
  out->pairs_on_host = c->replayed_pairs - c->replayed_on_device;
  out->sites_reevaluated = c->replayed_sites;
  out->exact_store = c->store.kind();
  out->text_rows_patched = (int32_t)std::min<uint64_t>(c->text_rows_patched, 0x7fffffffull);
  out->exact_store_build_s = c->store.build_seconds();
  out->sites_degenerate = c->h_skip_count;
  return NGSLD_OK;
}

int ngsld_replay_stats(ngsld_ctx *c, uint64_t *pairs, uint64_t *sites) {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  if (pairs) *pairs = c->replayed_pairs;
  if (sites) *sites = c->replayed_sites;
  return NGSLD_OK;
}

int ngsld_finish_device(ngsld_ctx *c) try {
  if (c == nullptr) return NGSLD_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  (void)hipGetLastError();  // (a failure some earlier call already reported must not surface as a launch's "last error")
  RC_TRY(finish_device_run(c));
  return check_status(c);
} NGSLD_CATCH(c)

}  // extern "C"
