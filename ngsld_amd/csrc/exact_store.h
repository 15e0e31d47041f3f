// exact_store.h -- the exact store of the device-side replay of LIKELIHOOD matrices (ld_replay_lkl.hip) and its one owner:
// included by engine.h between the buffer types and the context, which holds one ExactStore; the code is exact_store.hip.
// The store: normal-space likelihoods and est_maf as the reference holds them when calc_pair_LD runs -- the HOST's libm, the
// sequential est_maf -- laid out like the planes.  Input that came through ngsld_set_geno_lkl is such a store already (the
// planes are the caller's values), and so are the planes when no replay source is registered (the replay then runs on the
// device's own values, as the host's did): an ALIAS, complete at once.  With a source it is BUILT from the caller's raw values,
// the first time a run flags more pairs than the host should replay (wanted), and kept until the matrix or its source changes.
// A store that has to be built is built by a thread of its own, in site order, while the run that asked for it goes on: a
// launch's device-side replay needs the sites up to the end of its last row's window only (the frontier), and the build
// (~0.25 us per individual and site) stays ahead of the pipeline (pair kernel + replay of the rows of those sites).  A run
// that started the build waits for its end before it returns (wait_idle): the registered source is read during runs only.
#pragma once

struct ngsld_ctx;

namespace ngsld {
namespace eng {

class ExactStore {
 public:
  // ---- what a replay launch reads (valid as far as wait() said) ----
  const double *planes(const ngsld_ctx *c) const;  // the context's own planes / frequencies where the store is an alias
  const double *maf(const ngsld_ctx *c) const;
  bool has_lane_copy() const { return xT_ready_.load(); }  // the store once more, individual-major: what the lane-per-pair kernel reads
  const double *lane_copy() const { return xT_.p; }
  const uint32_t *lane_perm() const { return xperm_.p; }    // ... where each site stands in it (rare sites first: ReplayLklArgs::xperm)
  const uint32_t *lane_depth() const { return xdepth_.p; }  // ... and how small its sites' likelihoods get (ReplayLklArgs::xdepth)

  // ---- where it stands ----
  static bool is_free(const ngsld_ctx *c);  // the planes ARE the store: ngsld_set_geno_lkl input, or no source to build another from
  bool started() const { return state_.load() >= 1; }   // there or on its way (a replay may be asked for launches whose sites it covers)
  bool building() const { return state_.load() == 1; }
  bool failed() const { return failed_; }                // no store for this matrix: its flagged pairs stay with the host's threads
  bool wanted(const ngsld_ctx *c, uint64_t pending) const;  // should a run with `pending` flagged pairs for the host have the store instead?
  int kind() const { return state_.load() == 2 ? (alias_ ? 1 : 2) : 0; }  // ngsld_replay_stats_t::exact_store: complete, as an alias (1) or built (2)
  double build_seconds() const { return build_s_; }      // host seconds the store of this matrix took to build (0: an alias, or not built)

  // ---- its life (the run thread's calls) ----
  // starts the build where there is something to build (idempotent); the alias forms are complete at once.  A device without
  // room, or a cohort no kernel could read the store for, is no error: failed() from then on
  int start(ngsld_ctx *c);
  // waits until sites [0, need_sites) are on the device (need_sites >= n_sites: until the store is complete); *have = false when
  // there is no store to be had (host replay); an error of the build comes back as the return value, once, and is failed() after
  int wait(ngsld_ctx *c, uint64_t need_sites, bool *have);
  void wait_idle();  // until no builder is at work, whatever became of it (the end of every run: StoreGuard, engine_run.hip)
  // The SOURCE changes: the builder is cancelled and joined, nothing of the old store is of use.  failed() SURVIVES this: a matrix
  // whose store failed -- no room on the device, a failing source callback -- keeps its flagged pairs on the host's threads even
  // after a new source is registered; only a new matrix (reset) tries again.  Safe at any time: the builder looks at `cancel_`
  // between chunks (only a builder that outlived its run would see it set, which wait_idle prevents).
  void stop();
  void reset() {   // the MATRIX changes: stop() + a clean slate -- not failed, no alias, no build time
    stop();
    alias_ = failed_ = false;
    build_s_ = 0.0;
  }
  void destroy();  // the context goes: stop() + the builder's stream and staging

 private:
  struct Builder;                       // exact_store.hip: the builder thread's stages
  void release_buffers() { xplanes_.release(); xmaf_.release(); xT_.release(); xperm_.release(); xdepth_.release(); xT_ready_ = false; }
  bool alloc_lane_copy(ngsld_ctx *c);   // room for xT_ + the sites' order in it; false: the lanes go without
  hipError_t fill_lane_copy(ngsld_ctx *c, hipStream_t st);  // ... and all of it at once from planes that are a store already

  // WHO TOUCHES WHAT.  The device buffers: the run thread's while no builder exists; the builder fills them, launches read them
  // as far as the frontier.
  DevBuf<double> xplanes_, xmaf_, xT_;
  DevBuf<uint32_t> xperm_, xdepth_;
  // the builder thread alone
  PinBuf<double> stage_[2];
  hipStream_t stream_ = nullptr;        // its uploads (made by the first builder, kept for the context's life)
  ReplayPool pool_;                     // its threads (the context's replay_pool is the run's: host-only pairs beside the build)
  // shared: atomics, or under mu_
  std::thread thread_;                  // (the handle is the run thread's: started, joined)
  std::atomic<int> state_{0};           // 0 no store, 1 being built, 2 complete (every site + the lane kernel's copy where it fits), -1 the build failed
  std::atomic<uint64_t> frontier_{0};   // sites [0, frontier_) of xplanes_ / xmaf_ (and xT_) are on the device
  std::atomic<bool> cancel_{false};
  std::atomic<bool> xT_ready_{false};   // xT_ is allocated (a built store: filled as far as the frontier, like the planes)
  std::mutex mu_;                       // cv_, rc_, msg_, build_s_, and state_'s step from 1 to 2 / -1
  std::condition_variable cv_;
  int rc_ = 0;
  std::string msg_;
  double build_s_ = 0.0;
  // the run thread alone
  bool alias_ = false, failed_ = false;
};

}  // namespace eng
}  // namespace ngsld
