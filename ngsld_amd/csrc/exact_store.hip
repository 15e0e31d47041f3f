// exact_store.hip -- ExactStore (exact_store.h): the exact store of the device-side replay of likelihood matrices -- when it is
// wanted, its alias and built forms, the thread that builds it beside a run, and its one release list.
#include "engine.h"

namespace ngsld {
namespace eng {

const double *ExactStore::planes(const ngsld_ctx *c) const { return alias_ ? c->d_planes.p : xplanes_.p; }
const double *ExactStore::maf(const ngsld_ctx *c) const { return alias_ ? c->d_maf.p : xmaf_.p; }

bool ExactStore::is_free(const ngsld_ctx *c) { return c->normalised || (c->replay_matrix == nullptr && c->replay_read == nullptr); }

// Host replay costs ~0.15 us per individual and pair on one thread, the store ~0.25 us per individual and SITE (17 libm calls
// per triple: read_geno's log + post_prob, est_maf's post_prob + exp, main's exp), once: it pays as soon as the host would
// otherwise replay more pairs than half the matrix has sites.
bool ExactStore::wanted(const ngsld_ctx *c, uint64_t pending) const {
  if (!lkl_device_eligible(c) || failed_) return false;
  if (started() || is_free(c)) return pending > 0;
  if (c->exact_mode >= 2) return pending > 0;
  return c->host_replayed_total + pending > std::max<uint64_t>(4096, c->n_sites / 2);
}

// The individual-major copy for the lane-per-pair kernel, where the device has room for the matrix once more: its memory
bool ExactStore::alloc_lane_copy(ngsld_ctx *c) {
  xT_ready_ = false;
  const size_t elems = (size_t)c->n_sites * c->n_ind * 3;
  // (4 GB of the device left for what comes later -- text buffers, the lanes' list and sort scratch; under a cap: half a GB of it)
  if (!room_for(elems * sizeof(double), 4ull << 30, 512ull << 20)) return false;
  // The order of the sites in the copy: the RARE ones first (folded frequency below 1/32, or no frequency), the others behind,
  // each class in site order.  The pairs the lanes replay are pairs with a (nearly) monomorphic site, a wavefront's 64 lanes hold
  // a few neighbouring rare sites x 8 partners they share (replay_keys_kernel), and per individual the rare sites' triples are
  // 24 bytes each out of a cache line of their own while they stand among 32 consecutive sites: the launch fetched 1.3 TB
  // through an L2 that hit 18 % of the time (profiles/r06/replay_lane).  Standing together they share their lines: same-box
  // 612.5 / 613.3 -> 601.2 / 602.5 ms a pass at 20 % monomorphic sites (profiles/r06/lane/perm_ab.txt).
  std::vector<uint32_t> perm(c->n_sites);
  {
    uint32_t n_rare = 0;
    auto rare = [&](uint64_t s) {
      const double m = c->h_maf[s], r = m <= 0.5 ? m : 1 - m;
      return !(r >= 0.03125);
    };
    for (uint64_t s = 0; s < c->n_sites; ++s) n_rare += rare(s) ? 1u : 0u;
    uint32_t at_rare = 0, at_rest = n_rare;
    for (uint64_t s = 0; s < c->n_sites; ++s) perm[s] = rare(s) ? at_rare++ : at_rest++;
  }
  if (xT_.resize(elems) != hipSuccess || xdepth_.resize(c->n_sites) != hipSuccess ||
      hipMemset(xdepth_.p, 0, c->n_sites * sizeof(uint32_t)) != hipSuccess ||
      xperm_.resize(c->n_sites) != hipSuccess ||
      hipMemcpy(xperm_.p, perm.data(), c->n_sites * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    xT_.release();
    xperm_.release();
    return false;
  }
  return true;
}

// ... and all of it at once from planes that are a store already (the alias forms), on stream st, synchronised
hipError_t ExactStore::fill_lane_copy(ngsld_ctx *c, hipStream_t st) {
  if (!alloc_lane_copy(c)) return hipSuccess;
  hipError_t e = launch_transpose_store(planes(c), 3ull * c->np, c->np, (uint32_t)c->n_ind, c->n_sites, xT_.p, xdepth_.p, xperm_.p, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  xT_ready_ = true;
  return hipSuccess;
}

// a chunk of the store from pinned host memory into place (site_elems is even: np is a multiple of 8)
__global__ __launch_bounds__(256) void store_chunk_kernel(const double *__restrict__ src, double *__restrict__ dst, uint64_t n,
                                                          const double *__restrict__ src_maf, double *__restrict__ dst_maf, uint64_t n_maf) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, T = (uint64_t)gridDim.x * blockDim.x;
  const double2 *s2 = reinterpret_cast<const double2 *>(src);
  double2 *d2 = reinterpret_cast<double2 *>(dst);
  for (uint64_t i = t; i < n / 2; i += T) d2[i] = s2[i];
  if (t == 0 && (n & 1)) dst[n - 1] = src[n - 1];
  for (uint64_t i = t; i < n_maf; i += T) dst_maf[i] = src_maf[i];
}

// The builder (ExactStore::thread_): the registered source through the host's libm, chunk by chunk in site order -- two pinned
// staging buffers, a chunk's upload (and its transposition into the lane kernel's copy) beside the next chunk's arithmetic --,
// the frontier published as the uploads land.  Touches nothing of the context a run touches but the store's own buffers and
// atomics.  Every stage answers with an NGSLD_* code and leaves its text in `msg`; run() is the one way out.
struct ExactStore::Builder {
  ngsld_ctx *const c;
  ExactStore &s;
  Range range_{"ngsld:exact store (host libm -> device)"};
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  const uint64_t n = c->n_sites, ni = c->n_ind, np = c->np, site_elems = 3 * np;
  uint64_t chunk = std::max<uint64_t>(1, (32ull << 20) / (site_elems * sizeof(double))), slow_us = 0;
  const int T = c->replay_threads > 0 ? c->replay_threads : (int)std::min<unsigned>(32u, usable_threads());
  hipEvent_t up[2] = {nullptr, nullptr};  // a staging buffer's upload has landed
  std::vector<double> raw_chunk;          // (callback source: the chunk's raw values, fetched with one call)
  std::string msg;

  int hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return NGSLD_OK;
    (void)hipGetLastError();
    return bad(NGSLD_ERR_DEVICE, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  }
  int bad(int rc, const char *text) { return msg = text, rc; }

  int setup() {
    // tests: small chunks, a builder the run has to wait for
    if (const char *e = test_knob("EXACT_CHUNK_SITES")) chunk = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    if (const char *e = test_knob("EXACT_SLOW_US")) slow_us = std::strtoull(e, nullptr, 10);
    if (chunk > n) chunk = n;
    RC_TRY(hip(hipSetDevice(c->device), "exact store"));
    if (s.stream_ == nullptr) {
      // a HIGH-PRIORITY stream: the runtime gives it a hardware queue of that priority instead of a share in one of the run's
      // four -- where a chunk's upload stood behind an 80 ms replay kernel of the run, which itself waited for the builder's
      // frontier: one chunk per batch, 120,000 x 2,000 built in 5.1 s instead of 0.4
      int least = 0, greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
        (void)hipGetLastError();
        least = greatest = 0;
      }
      RC_TRY(hip(hipStreamCreateWithPriority(&s.stream_, hipStreamNonBlocking, greatest), "exact store stream"));
    }
    for (int k = 0; k < 2; ++k) {
      RC_TRY(hip(s.stage_[k].resize((size_t)chunk * (site_elems + 1)), "exact store staging"));  // (+ 1: the site's est_maf behind the planes)
      RC_TRY(hip(hipEventCreateWithFlags(&up[k], hipEventDisableTiming), "exact store event"));
    }
    return NGSLD_OK;
  }

  // the raw values of sites [s0, s0 + m): the caller's array in place, or its callback under replay_mu
  int fetch_chunk(uint64_t s0, uint64_t m, const double **raw) {
    if (c->replay_matrix != nullptr) {
      *raw = c->replay_matrix + s0 * 3 * ni;
      return NGSLD_OK;
    }
    raw_chunk.resize((size_t)m * 3 * ni);
    std::lock_guard<std::mutex> g(c->replay_mu);
    if (c->replay_read(c->replay_user, s0, m, raw_chunk.data()) != 0) return bad(NGSLD_ERR_SINK, "the replay source callback failed");
    *raw = raw_chunk.data();
    return NGSLD_OK;
  }

  // ... through the host's libm into staging buffer b, on the builder's own threads
  // (buffer b was last read by the upload of chunk k - 2, whose event was waited for when chunk k - 1 was issued)
  int compute_chunk(const double *raw, uint64_t m, int b) {
    double *stage = s.stage_[b].p, *stage_maf = stage + (size_t)chunk * site_elems;
    const int Tm = (int)std::min<uint64_t>((uint64_t)T, m);
    std::atomic<bool> good{true};
    s.pool_.run(Tm, [&](int t) {
      try {
        for (uint64_t k = m * (uint64_t)t / (uint64_t)Tm; k < m * (uint64_t)(t + 1) / (uint64_t)Tm; ++k)
          replay_site_planes(raw + k * 3 * ni, ni, c->gopts, np, stage + k * site_elems, &stage_maf[k]);
      } catch (...) {
        good = false;
      }
    });
    return good ? NGSLD_OK : bad(NGSLD_ERR_NOMEM, "out of host memory");
  }

  // ... into place on the builder's stream, the lane kernel's copy of these sites behind their planes, the buffer's event
  int upload_chunk(uint64_t s0, uint64_t m, int b) {
    // (a KERNEL reads the pinned chunk over the host link, not hipMemcpyAsync: an SDMA copy can queue behind the run's text
    // copies on that engine, each of which waits for its batch's kernels -- send_flag_head)
    double *stage_dev = nullptr;
    RC_TRY(hip(hipHostGetDevicePointer((void **)&stage_dev, s.stage_[b].p, 0), "exact store upload"));
    hipLaunchKernelGGL(store_chunk_kernel, dim3(512), dim3(256), 0, s.stream_, stage_dev, s.xplanes_.p + s0 * site_elems, (uint64_t)m * site_elems,
                       stage_dev + (size_t)chunk * site_elems, s.xmaf_.p + s0, (uint64_t)m);
    RC_TRY(hip(hipGetLastError(), "exact store upload"));
    if (s.xT_ready_.load())
      RC_TRY(hip(launch_transpose_store(s.xplanes_.p, site_elems, (uint32_t)np, (uint32_t)ni, n, s.xT_.p, s.xdepth_.p, s.xperm_.p, s.stream_, s0, s0 + m),
                 "exact store, individual-major copy"));
    return hip(hipEventRecord(up[b], s.stream_), "exact store upload");
  }

  // the chunk before the one just issued has landed (its upload ran beside that one's arithmetic): sites [0, end) are there
  int publish(int b, uint64_t end) {
    RC_TRY(hip(hipEventSynchronize(up[b]), "exact store upload"));
    s.frontier_.store(end);
    s.cv_.notify_all();
    return NGSLD_OK;
  }

  int chunks() try {
    RC_TRY(setup());
    uint64_t k = 0, prev_end = 0;
    for (uint64_t s0 = 0; s0 < n && !s.cancel_.load(); s0 += chunk, ++k) {
      const int b = (int)(k & 1);
      const uint64_t m = std::min(chunk, n - s0);
      const double *raw = nullptr;
      RC_TRY(fetch_chunk(s0, m, &raw));
      if (slow_us) std::this_thread::sleep_for(std::chrono::microseconds(slow_us));
      RC_TRY(compute_chunk(raw, m, b));
      RC_TRY(upload_chunk(s0, m, b));
      if (k >= 1) RC_TRY(publish(b ^ 1, prev_end));
      prev_end = s0 + m;
    }
    return NGSLD_OK;
  } catch (...) {
    return bad(NGSLD_ERR_NOMEM, "out of host memory");
  }

  // Whatever became of the chunks: the stream is quiet, the staging is given back, the result stands under mu_, waiters wake.
  void finish(int rc) {
    if (s.stream_ != nullptr) {
      const hipError_t e = hipStreamSynchronize(s.stream_);
      if (rc == NGSLD_OK) rc = hip(e, "exact store upload");
    }
    if (rc == NGSLD_OK && !s.cancel_.load()) {
      s.frontier_.store(n);
      s.cv_.notify_all();
    }
    for (auto &b : s.stage_) b.release();  // (64 MB of pinned host memory, used once per matrix)
    for (hipEvent_t e : up)
      if (e) (void)hipEventDestroy(e);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    {
      std::lock_guard<std::mutex> g(s.mu_);
      s.rc_ = rc;
      s.msg_ = msg;
      s.build_s_ = secs;
      s.state_.store(rc == NGSLD_OK && !s.cancel_.load() ? 2 : -1);
    }
    s.cv_.notify_all();
    if (std::getenv("NGSLD_TRACE") != nullptr)
      std::fprintf(stderr, "[trace] exact store: %llu sites x %llu individuals through the host's libm in %.3f s (a thread of its own beside the run)\n",
                   (unsigned long long)n, (unsigned long long)ni, secs);
  }

  void run() { finish(chunks()); }
};

int ExactStore::start(ngsld_ctx *c) {
  if (state_.load() != 0 || failed_) return NGSLD_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (is_free(c)) {  // the planes ARE the store
    alias_ = true;
    frontier_.store(c->n_sites);
    const hipError_t e = fill_lane_copy(c, replay_stream_of(c));
    if (e != hipSuccess) return hip_fail(c, e, "exact store, individual-major copy");
    // (beyond 4,096 individuals the wavefront-per-pair kernel has no shape: without room for the copy the lanes read there is no
    // kernel for this cohort)
    failed_ = !xT_ready_.load() && replay_lkl_waves((uint32_t)c->n_ind) == 0;
    if (!failed_) state_.store(2);
    return NGSLD_OK;
  }
  // (a device without room for the matrix once more: no store for this matrix -- its flagged pairs stay with the host's threads)
  const bool pretend = test_knob("EXACT_STORE_NO_ROOM") != nullptr;
  const bool no_room = !room_for((uint64_t)c->n_sites * (3ull * c->np + 1) * sizeof(double), 0, 256ull << 20);  // (ngsld_set_memory_budget)
  failed_ = pretend || no_room || xplanes_.resize((size_t)c->n_sites * 3 * c->np) != hipSuccess || xmaf_.resize(c->n_sites) != hipSuccess;
  if (failed_) (void)hipGetLastError();
  if (!failed_) {
    if (thread_.joinable()) thread_.join();  // (a builder that ended by itself)
    alias_ = false;
    xT_ready_ = alloc_lane_copy(c);  // (filled chunk by chunk behind the planes: usable as far as the frontier, like them)
    failed_ = !xT_ready_.load() && replay_lkl_waves((uint32_t)c->n_ind) == 0;  // (see the alias form above)
  }
  if (failed_) {
    xplanes_.release();
    xmaf_.release();
    return NGSLD_OK;
  }
  cancel_.store(false);
  frontier_.store(0);
  state_.store(1);
  try {
    thread_ = std::thread([this, c] { Builder{c, *this}.run(); });
  } catch (...) {
    state_.store(0);
    failed_ = true;  // (no thread to be had: host replay)
  }
  return NGSLD_OK;
}

int ExactStore::wait(ngsld_ctx *c, uint64_t need_sites, bool *have) {
  *have = false;
  if (failed_ || state_.load() == 0) return NGSLD_OK;
  const bool all = need_sites >= c->n_sites;
  {
    std::unique_lock<std::mutex> lk(mu_);
    // (the builder publishes the frontier without the lock: a short timed wait instead of a missed wake-up)
    while (state_.load() == 1 && (all || frontier_.load() < need_sites)) cv_.wait_for(lk, std::chrono::milliseconds(1));
    if (state_.load() == -1) {
      const int rc = rc_;
      const std::string msg = msg_;
      lk.unlock();
      stop();          // (joins the builder, which has ended, and releases what it filled)
      failed_ = true;  // (not again for this matrix)
      return rc != NGSLD_OK ? fail(c, rc, msg.c_str()) : NGSLD_OK;
    }
  }
  if (state_.load() == 2 && thread_.joinable()) thread_.join();
  *have = true;
  return NGSLD_OK;
}

void ExactStore::wait_idle() {
  std::unique_lock<std::mutex> lk(mu_);
  while (state_.load() == 1) cv_.wait_for(lk, std::chrono::milliseconds(1));
}

void ExactStore::stop() {
  if (thread_.joinable()) {
    cancel_.store(true);
    thread_.join();
  }
  cancel_.store(false);
  state_.store(0);
  frontier_.store(0);
  rc_ = NGSLD_OK;
  msg_.clear();
  release_buffers();  // (a new source or matrix: nothing of the old store is of use, start allocates what it needs)
}

void ExactStore::destroy() {
  stop();
  if (stream_) (void)hipStreamDestroy(stream_);
  stream_ = nullptr;
  for (auto &b : stage_) b.release();
}

}  // namespace eng
}  // namespace ngsld
