/*
 * ngsld.h -- C-ABI of the MI355X-native pairwise-LD engine (drop-in for the pair-LD path of
 * fgvieira/ngsLD v1.2.1).  Plain C: opaque handle, pointers and sizes, int return codes, no C++ or
 * torch types, no exceptions across the boundary.
 *
 * What this boundary replaces in the reference (paths relative to the reference tree):
 *   ngsLD.cpp:153-198   threadpool_create -> per-s1 threadpool_add(calc_pair_LD) -> threadpool_wait
 *                       -> threadpool_destroy            => ngsld_create / ngsld_plan / ngsld_run / ngsld_destroy
 *   ngsLD.cpp:229-359   calc_pair_LD (window walk, filters, haplo_freq, pearson_r, D/D'/r2)
 *                                                         => the HIP pair kernel behind ngsld_run
 *   ngsLD.cpp:103-114   est_maf + exp() + expected genotypes => ngsld_set_geno_raw (device prep kernel)
 *   ngsLD.hpp:11-44     `params`: geno_lkl, maf, pos_dist, max_kb_dist, max_snp_dist, min_maf,
 *                       ignore_miss_data, extend_out      => ngsld_set_geno_*, ngsld_set_pos_dist, ngsld_params
 * The text side (labels, dist column, %f formatting, chi2 in float) stays with the caller; helpers
 * that mirror it live in ngsld_host.h.
 *
 * Errors: the reference is fatal-on-error (error(), gen_func.cpp:12-18).  This library never exits:
 * every entry point returns NGSLD_OK or a negative code and ngsld_last_error() gives the text; the
 * ngsLD command-line wrapper turns them back into the reference's stderr format and exit(-1).
 *
 * Threading: one thread per ngsld_ctx at a time.  ngsld_run blocks; the sink is called on the calling
 * thread, batches arrive in increasing (s1, s2) order.
 */
#ifndef NGSLD_H
#define NGSLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ngsld_ctx ngsld_ctx;

enum {
  NGSLD_OK = 0,
  NGSLD_ERR_INVALID = -1,    /* bad argument or call order (cf. threadpool_invalid, threadpool.h:39) */
  NGSLD_ERR_DEVICE = -2,     /* HIP runtime failure, or no usable gfx950 device */
  NGSLD_ERR_NOMEM = -3,      /* host or device allocation failed */
  NGSLD_ERR_NAN = -4,        /* "NaN found! Is the file format correct?" (read_data.cpp:42-45) */
  NGSLD_ERR_MAF_RANGE = -5,  /* "invalid allele frequencies" (gen_func.cpp:1030-1031) */
  NGSLD_ERR_SINK = -6,       /* the sink callback returned non-zero */
  NGSLD_ERR_UNSUPPORTED = -7 /* problem shape outside the supported range (n_sites or n_ind >= 2^32 - 64) */
};

/* The fields of `params` (ngsLD.hpp:11-44) that calc_pair_LD reads. */
typedef struct {
  uint64_t max_kb_dist;      /* 0 = no distance limit (ngsLD.cpp:252) */
  uint64_t max_snp_dist;     /* 0 = no limit (ngsLD.cpp:258) */
  double min_maf;            /* ngsLD.cpp:264-275: s1 below -> row empty, s2 below -> pair skipped */
  int32_t ignore_miss_data;  /* gen_func.cpp:1089 */
  int32_t extend_out;        /* also produce ngsld_rec_ext */
  double rnd_sample;         /* ngsLD.cpp:277: keep a pair iff its Tausworthe draw <= rnd_sample; 0 or 1 = keep all */
  uint64_t seed;             /* --seed of the master gsl_rng_taus stream (ngsLD.cpp:69-70); used iff rnd_sample < 1 */
  uint64_t first_row;        /* global index of this context's site 0 when it holds a slab of a larger matrix (multi-GPU
                                row sharding): that many draws of the master stream are skipped so that every row gets
                                the seed it has in the single-process run (ngsLD.cpp:165-166).  0 otherwise. */
} ngsld_params;

/* Standard columns computed per pair (ngsLD.cpp:290-306): 32 bytes. */
typedef struct {
  double r2_ExpG; /* pearson_r(expected_geno[s1], expected_geno[s2])^2 */
  double D;
  double Dp;
  double r2;
} ngsld_rec_std;

/* What the extended columns (ngsLD.cpp:336-349) need beyond per-site data: 40 bytes. */
typedef struct {
  double hap[4];       /* hap_freq[0..3] after the EM */
  uint32_t n_ind_data; /* sample_size: individuals used by the EM (bit-exact) */
  uint32_t n_iter;     /* return value of haplo_freq */
} ngsld_rec_ext;

/* One unit of the pair space: the pairs (s1, s2_begin + c) for the bits c set in `mask` (c < count <= 64), i.e.
 * the candidates of row s1 that survived the maf[s2] skip (ngsLD.cpp:270) and the random sub-sampling
 * (ngsLD.cpp:277).  Their records are consecutive, starting at `first_record`, in increasing c. */
typedef struct {
  uint32_t s1, s2_begin, count, reserved;
  uint64_t mask;
  uint64_t first_record;
} ngsld_item;

/* One batch of results: all pairs of rows [s1_begin, s1_end), in (s1, s2) order.  `items` lists them row by row
 * (increasing s1, then increasing s2_begin), first_record relative to this batch.  Pointers are valid only
 * during the callback. */
typedef struct {
  uint64_t s1_begin, s1_end;
  uint64_t n_pairs;
  uint64_t n_items;
  const ngsld_item *items;   /* [n_items] */
  const ngsld_rec_std *std;  /* [n_pairs] */
  const ngsld_rec_ext *ext;  /* [n_pairs] or NULL when extend_out == 0 */
  /* Only after ngsld_set_text_output(..., 1): the batch's TSV rows, formatted on the device -- byte for byte what
   * ngsld_host_write_batch writes for this batch (ngsLD.cpp:314-351).  When text != NULL, items / std / ext are NULL
   * (the records were not copied to the host).  A batch the device formatter cannot take (a value beyond its
   * fast path) arrives as records, text == NULL, as without text output. */
  const char *text;
  uint64_t text_len;
} ngsld_batch;

typedef int (*ngsld_sink_fn)(void *user, const ngsld_batch *batch);

/* Fill dst with the raw values ([site][ind][3] doubles, as ngsld_set_geno_raw_opts takes them) of sites
 * [site_begin, site_begin + n_sites).  Called on a library thread, never concurrently.  Non-zero = failure. */
typedef int (*ngsld_read_sites_fn)(void *user, uint64_t site_begin, uint64_t n_sites, double *dst);

const char *ngsld_version(void);

/* Bind to HIP device `device` (must be gfx950).  Fails with NGSLD_ERR_DEVICE when there is no GPU:
 * there is no CPU fallback behind this API. */
int ngsld_create(int device, ngsld_ctx **ctx);
void ngsld_destroy(ngsld_ctx *ctx);
/* Text of the last failure on ctx (ctx may be NULL: last ngsld_create failure of this thread). */
const char *ngsld_last_error(const ngsld_ctx *ctx);

/* Genotype likelihoods exactly as the reference's binary input holds them: n_sites*n_ind*3 doubles,
 * [site][ind][geno] (read_data.cpp:28-47), natural scale or logs (log_scale).  The device does what
 * read_geno + main do to them: log, -inf -> -1e15, log-normalise, NaN check, est_maf, exp, expected
 * genotypes.  `on_device` != 0: gl_raw is a device pointer on this ctx's device (not modified).
 * `ignore_miss_data` here also picks the device layout of the matrix (for some cohort sizes the kernels measured best
 * differ with the flag, and their plane padding with them): give the value ngsld_params.ignore_miss_data will have.
 * A plan with the other value is computed all the same -- same records, possibly on the slower of two kernels. */
int ngsld_set_geno_raw(ngsld_ctx *ctx, const double *gl_raw, uint64_t n_sites, uint64_t n_ind, int log_scale,
                       int ignore_miss_data, int on_device);
/* The same with every input-side switch of the reference's main():
 *   text_semantics  the values came from a text (.gz) genotype file: plain log() with no -inf -> -1e15
 *                   replacement and no NaN check, as the text branch of read_geno (read_data.cpp:83-99)
 *   call_geno       harden the likelihoods first (ngsLD.cpp:92-98 -> call_geno, gen_func.cpp:886-914):
 *                   best genotype below N_thresh -> missing, at or above call_thresh -> called
 *   per_individual_only  never switch to the genotype-combination kernel (ngsld_pair_kernel): a caller that computes
 *                   parts of one matrix in several contexts sets it unless ALL parts qualify, so that every part
 *                   runs the same arithmetic */
typedef struct {
  int32_t log_scale;
  int32_t ignore_miss_data;
  int32_t on_device;
  int32_t text_semantics;
  int32_t call_geno;
  int32_t per_individual_only;
  double N_thresh;
  double call_thresh;
} ngsld_geno_opts;
int ngsld_set_geno_raw_opts(ngsld_ctx *ctx, const double *gl_raw, uint64_t n_sites, uint64_t n_ind,
                            const ngsld_geno_opts *opts);
/* The reference's own data contract at calc_pair_LD: normalised normal-space geno_lkl
 * [site][ind][3] and maf[site] already computed by the caller (ngsLD.hpp:36-37). */
int ngsld_set_geno_lkl(ngsld_ctx *ctx, const double *geno_lkl, const double *maf, uint64_t n_sites, uint64_t n_ind,
                       int on_device);
/* Copy the per-site allele frequencies (est_maf) to host memory, n_sites doubles. */
int ngsld_get_maf(ngsld_ctx *ctx, double *maf_out);
/* pos_dist[s] = bp gap to the previous site, INFINITY at a chromosome change (read_data.cpp:165-218).
 * NULL = all INFINITY (the reference's no --pos case, ngsLD.cpp:134).  Host pointer, n_sites doubles. */
int ngsld_set_pos_dist(ngsld_ctx *ctx, const double *pos_dist);

/* Fix the filters and enumerate the pair space (the s2 walk of ngsLD.cpp:240-282 for every s1).
 * Returns the total number of pairs that reach haplo_freq. */
int ngsld_plan(ngsld_ctx *ctx, const ngsld_params *params, uint64_t *n_pairs);
/* Host views of the plan, valid until the next ngsld_plan/ngsld_set_*: row_off [n_sites+1] (pairs
 * before each row), row_end [n_sites].  Used to shard rows across GPUs by pair count. */
int ngsld_plan_rows(ngsld_ctx *ctx, const uint64_t **row_off, const uint32_t **row_end);

/* Compute every pair of rows [s1_begin, s1_end) and hand the records to `sink`, batch by batch.  The records of a batch are
 * in pinned host memory the pair kernels wrote directly (no device copy, no D2H behind the last kernel): the host-resident
 * rate is the kernels' rate to within 1 %. */
int ngsld_run(ngsld_ctx *ctx, uint64_t s1_begin, uint64_t s1_end, ngsld_sink_fn sink, void *user);

/* Device-side TSV for ngsld_run (replaces the fprintf block of calc_pair_LD, ngsLD.cpp:310-352, at kernel rates):
 * labels = n_sites C strings as they appear in the first two columns (ngsLD.cpp:127-132), or NULL for the
 * reference's no --pos output "(null)".  enable != 0: ngsld_run hands over text (ngsld_batch.text) instead of records.
 * Call after ngsld_set_geno_* (the labels belong to that matrix); the dist column comes from ngsld_set_pos_dist and
 * needs its finite gaps to be integers (as read_dist produces them), otherwise batches arrive as records. */
int ngsld_set_text_output(ngsld_ctx *ctx, const char *const *labels, int enable);

/* Optional: start allocating the pinned host buffers of the text batches (three, each for one batch of rows of about
 * bytes_per_row) on a library thread, so that pinning them overlaps whatever the caller does next (reading,
 * ngsld_set_geno_*, ngsld_plan) instead of the first batches of ngsld_run.  A batch that needs more gets a larger buffer
 * then.  Callable any time after ngsld_create. */
int ngsld_reserve_text_buffers(ngsld_ctx *ctx, uint64_t bytes_per_row);

/* ---- Exact-order replay ------------------------------------------------------------------------------------
 * The kernels evaluate every pair with reordered arithmetic (tree sums, fused multiply-adds), which agrees with the
 * reference to ~1e-15 wherever the outcome is well conditioned.  A few outcomes are decided by the reference's own
 * rounding noise: D' and r2 of a pair with a site (nearly) monomorphic in the estimated haplotypes (0/0-type
 * quotients, ngsLD.cpp:296-306: -nan, 0.000000 or inf), nIter when eps lands within 1e-12 of EPSILON
 * (gen_func.cpp:1054), the maf < min_maf tests when a frequency ties --min_maf (ngsLD.cpp:264-275), r2_ExpG of a
 * pair of sites whose expected genotypes are both nearly constant (1 / (std1 std2) > 2^13; ngsLD.cpp:365-367).  The kernels flag those pairs and
 * the engine re-evaluates them on the host in the reference's operation order (sequential sums over individuals,
 * the sequential renormalisation, no fused multiply-add: ngsld_host_replay_pair in ngsld_host.h) and overwrites
 * their records -- before a batch reaches the sink, before it is formatted on the device, before ngsld_run_device
 * returns.  On by default.
 *
 * The replay needs the two sites' values again.  ngsld_set_replay_source registers where to get them: `read` fills
 * dst with the RAW values of sites [site_begin, site_begin + n) of this context ([site][ind][3], exactly what
 * ngsld_set_geno_raw_opts / ngsld_set_geno_lkl was given) and may be called from several library threads, one call
 * at a time.  With a source the replayed records are the reference's own bits (same libm).  Without one the
 * library reads its prepped planes back from the device: same operation order, inputs that differ from the
 * reference's by the device's exp/log rounding (exact for ngsld_set_geno_lkl), and --min_maf ties are left to the
 * device's est_maf.  Call after ngsld_set_geno_* (the source belongs to that matrix), before ngsld_plan. */
int ngsld_set_replay_source(ngsld_ctx *ctx, ngsld_read_sites_fn read, void *user);
/* The common case of a source -- the caller still HOLDS the matrix it gave ngsld_set_geno_raw_opts / ngsld_set_geno_lkl, as
 * the reference's main does throughout (ngsLD.cpp:86-89): `values` = that same host array, [site][ind][3], which must stay
 * valid and unchanged until the context is destroyed or given other data.  Read in place by the replay threads: no callback,
 * no copy, no lock (the callback form serialises its calls).  NULL removes it.  Replaces any registered callback. */
int ngsld_set_replay_matrix(ngsld_ctx *ctx, const double *values);
/* enable == 0: no replay, every record is the kernels' own value. */
int ngsld_set_replay(ngsld_ctx *ctx, int enable);
/* Pairs replayed by the last ngsld_run / ngsld_run_device (+ ngsld_finish_device) and sites re-evaluated by the last
 * ngsld_plan and run.  Either pointer may be NULL. */
int ngsld_replay_stats(ngsld_ctx *ctx, uint64_t *pairs, uint64_t *sites);

/* Where the flagged pairs are replayed.  Called-genotype matrices: on the device (their values are the same bits there).
 * LIKELIHOOD matrices: a few dozen pairs per 10^8 on SNP-called input, which host threads replay -- but on matrices that are
 * NOT SNP-called (the reference's README.md:73: "comparisons will show up as nan or inf") every pair with a (nearly)
 * monomorphic site is flagged, a third of all pairs at 20 % monomorphic sites.  Those are replayed on the DEVICE too, a
 * wavefront per pair, in the reference's operation order (ld_replay_lkl.hip) -- on an "exact store": the matrix once more in
 * device memory, normal-space likelihoods and est_maf as the reference holds them when calc_pair_LD runs, i.e. through the
 * HOST's libm.  Data given through ngsld_set_geno_lkl is that already (nothing is built, the replay is on the device from the
 * first pair on); without a replay source the device's own prepped values serve (the replay then runs on the device's
 * exp / log rounding, as the host's did); with a source the store is built from the caller's raw values -- 17 libm calls per
 * triple, ~0.25 us per individual and site on one thread, once per matrix -- the first time a run has flagged more pairs than
 * the host should replay (more than half as many as the matrix has sites).  The build runs on threads of its own BESIDE the
 * ngsld_run that asked for it, in site order: a batch's replay waits only until the builder has passed the batch's last
 * window; the run returns when the build has ended (the source is read during runs only).  ngsld_finish_device builds it
 * before it replays.
 * mode: 0 never (host replay only), 1 as described (default), 2 build at the first flagged pair.
 * (0.4.0) Such a matrix is recognised when it is set: ngsld_set_geno_* marks the DEGENERATE sites -- the one-locus EM of the site,
 * from its est_maf frequency, ends below 3e-6: every pair of such a site (nearly) is one the replay settles.  Where the device can
 * replay (mode != 0) the pair kernels leave the EM of those pairs out -- the replay, exact for any pair, is their one evaluation --
 * and ngsld_run with text output computes in groups of up to 2^25 pairs (one launch of pair kernels + one replay per group) instead
 * of batch by batch; the sink sees the same batches.  ngsld_replay_stats_t.sites_degenerate; NGSLD_REPLAY_SKIP=0 turns the marks off. */
int ngsld_set_exact_store(ngsld_ctx *ctx, int mode);
typedef struct {
  uint64_t pairs_flagged;      /* pairs the kernels of the last run flagged */
  uint64_t pairs_replayed;     /* ... of them replayed (all, unless the replay is off) */
  uint64_t pairs_on_device;    /* ... on the device */
  uint64_t pairs_on_host;      /* ... on host threads */
  uint64_t sites_reevaluated;  /* sites the host re-evaluated for the last plan + run */
  int32_t exact_store;         /* 0 none, 1 the planes themselves serve as the store, 2 built from the replay source */
  int32_t text_rows_patched;   /* text runs: rows of pairs replayed on the host whose value columns were overwritten in the host's copy of the text */
  double exact_store_build_s;  /* host seconds the build took (once per matrix) */
  uint64_t sites_degenerate;   /* (0.4.0) sites of the matrix marked degenerate -- their one-locus EM ends below 3e-6: the pair kernels leave
                                  the EM of such a site's pairs to the exact-order replay, which was going to start them over (0 on SNP-called
                                  input, or where the device cannot replay: nothing is skipped then) */
} ngsld_replay_stats_t;
int ngsld_replay_info(ngsld_ctx *ctx, ngsld_replay_stats_t *out);

/* Same computation with the records left in caller-owned DEVICE memory (no host transfer):
 * d_std holds ngsld_rec_std[n], d_ext ngsld_rec_ext[n] (may be NULL), n = row_off[s1_end] -
 * row_off[s1_begin], record k = global pair index - row_off[s1_begin].  `hip_stream` is a hipStream_t
 * (NULL = the ctx's own stream); the call returns after enqueueing when a stream is given. */
int ngsld_run_device(ngsld_ctx *ctx, uint64_t s1_begin, uint64_t s1_end, void *d_std, void *d_ext, void *hip_stream);
/* After ngsld_run_device on a caller's stream: waits for that stream, replays the flagged pairs and patches the device
 * records (exact-order replay, above).  A context has ONE pending device run: the next ngsld_run_device, ngsld_run,
 * ngsld_plan or ngsld_set_geno_* finishes it first (as this call would), so a flagged record is never left with the
 * kernels' own value.  A no-op after a run on the ctx's own stream (hip_stream == NULL does all of it before returning).
 * BUFFER LIFETIME: the replay of a pending run reads the matrix it was started with -- through the registered replay source
 * or matrix (ngsld_set_replay_source / ngsld_set_replay_matrix) -- at the moment the run is finished, whoever finishes it.
 * Keep that host array (or what the callback reads) valid and UNCHANGED until ngsld_finish_device, or the call that
 * finishes the run implicitly, has returned: refilling the buffer with the next matrix before ngsld_set_geno_* would have
 * the old run's flagged records recomputed from the new values, silently. */
int ngsld_finish_device(ngsld_ctx *ctx);

/* Timing of the pair kernel launches issued by the last ngsld_run / ngsld_run_device, measured with
 * HIP events on the stream they ran on (synchronises that stream).  Any pointer may be NULL. */
int ngsld_last_kernel_time(ngsld_ctx *ctx, double *total_ms, uint64_t *n_launches, uint64_t *n_pairs);

/* Which pair kernel family the genotype data set last will run on: "group" (8 / 16 / 32 lanes per pair), "run" (one
 * wavefront per pair, up to 640 individuals), "ab" (one wavefront per pair, a/b form of the EM step: 641..960 individuals), "multi" / "multi-ab" (several wavefronts per pair, P form / a/b form, up to 7,680 individuals), "stream" (beyond: one vector in registers, the other re-read in every EM iteration), or "hard" -- every
 * likelihood triple is a called genotype or "no data" (text genotypes, --call_geno: ngsLD.cpp:92-98,
 * read_data.cpp:83-99), the pairs run on their 16 genotype-combination counts.  "" before any data is set. */
const char *ngsld_pair_kernel(const ngsld_ctx *ctx);
/* The same decision without a device or a context: which kernel family and shape a likelihood matrix of n_ind individuals set
 * with this ignore_miss_data runs on, as text -- "<family> <wavefronts per pair>x<individuals per lane> lanes=<lanes per pair>
 * np=<padded individuals per genotype plane>", e.g. "run 1x8 lanes=64 np=512" for 500.  (Called-genotype matrices take "hard"
 * whatever the cohort, up to 4,096 individuals.)  Returns NGSLD_ERR_UNSUPPORTED for a cohort size outside the supported range,
 * NGSLD_ERR_INVALID when buf is too short.  tests/golden/dispatch_table.txt is this function over 1..12,000. */
int ngsld_describe_dispatch(uint64_t n_ind, int ignore_miss_data, char *buf, size_t buf_len);

/* Tuning knobs (optional): pairs per work item, max pairs per batch of ngsld_run. 0 keeps the default -- record batches of
 * 2^24 pairs (the pair kernels write them straight into two pinned host buffers of that many records; halved, down to 2^16,
 * on a host that cannot pin them), text batches of 2^19 rows.  A value given here is taken as it is for record batches and as
 * an upper bound for text batches. */
int ngsld_set_tuning(ngsld_ctx *ctx, uint32_t pairs_per_item, uint64_t batch_pairs);

/* On-device self test of the wavefront primitives the pair kernel relies on (cross-lane fold
 * reduction, refined reciprocal).  Returns NGSLD_OK or NGSLD_ERR_DEVICE with a message. */
int ngsld_selftest(ngsld_ctx *ctx);

/* On-device self test of the text formatter: n rows, row i the pair (2i, 2i+1) of a batch of 2n sites with the records
 * std[i] (and ext[i]; ext NULL: standard rows), the printed dist dist[i] (+INFINITY: a chromosome change) and the site
 * frequencies maf1[i], maf2[i]; labels print as "(null)".  The rows go through the production passes (lengths, prefix sums,
 * write) into text (text_cap bytes: NGSLD_ERR_INVALID when they do not fit), row_len[n] receives each row's length and
 * *needs_host 1 when a value lies beyond the device formatter, as a run would hand that batch over as records.  Host
 * pointers. */
int ngsld_selftest_format(ngsld_ctx *ctx, uint64_t n, const ngsld_rec_std *std, const ngsld_rec_ext *ext, const double *dist,
                          const double *maf1, const double *maf2, char *text, uint64_t text_cap, uint64_t *row_len,
                          int32_t *needs_host);
/* On-device self test of the printed-value quantiser (PRUNE.md, DECAY.md), for n doubles x[]: micro[i] / micro_ok[i] what LD
 * decay's bin kernel sums for x[i] (its "%f" in integer micro-units; ok 0 from 2^38 on), label[i] / label_rc[i] the edge label
 * LD pruning gives it with the weight type ('a', 'e', 'n'), precision (0..15) and min_weight (rc 0 an edge, 1 skipped, 2 a label
 * of 2^62 or more).  Host pointers. */
int ngsld_selftest_printed(ngsld_ctx *ctx, uint64_t n, const double *x, int32_t precision, int32_t weight_type,
                           double min_weight, int64_t *micro, int32_t *micro_ok, int64_t *label, int32_t *label_rc);

/* ---- Streaming: matrices larger than the device budget (windowed runs only) ------------------------------
 * The reference keeps the whole matrix in host memory (twice during the transpose, ngsLD.cpp:87-89).  Here a
 * windowed run (max_kb_dist and/or max_snp_dist > 0) can be cut into slabs of rows: slab k holds the sites
 * [row_begin, site_end) = its rows plus the halo their windows reach into, and computes the rows
 * [row_begin, row_end).  Two contexts on the same device alternate, so the file read + upload + prep of slab
 * k+1 overlap the pair kernels of slab k; neither the host nor the device ever holds more than two slabs. */
typedef struct {
  uint64_t row_begin, row_end; /* rows (s1) this slab computes */
  uint64_t site_end;           /* one past the last site any of those rows pairs with */
} ngsld_slab;

/* Upper end of the s2 walk of every row from the distance / SNP-count limits alone (ngsLD.cpp:240-262):
 * row s1 pairs with sites (s1, row_end[s1]).  Host only, no device needed; pos_dist NULL = all INFINITY. */
int ngsld_window_ends(const double *pos_dist, uint64_t n_sites, const ngsld_params *params, uint32_t *row_end);

/* Cut rows [0, n_sites) into slabs of at most max_slab_sites sites (rows + halo).  slabs has room for `cap`
 * entries (n_sites always suffices).  NGSLD_ERR_NOMEM when a single row's window does not fit. Host only. */
int ngsld_plan_slabs(const double *pos_dist, uint64_t n_sites, const ngsld_params *params, uint64_t max_slab_sites,
                     ngsld_slab *slabs, uint64_t cap, uint64_t *n_slabs);

/* How many sites of n_ind individuals fit a slab when `budget_bytes` of device memory may be used in total
 * (both contexts, their record buffers included, the matrix priced THREE times per context: the planes, and the exact store of
 * the device-side replay with its individual-major copy, which input that is not SNP-called makes the library build); 0 when
 * the budget is too small for any. */
uint64_t ngsld_slab_sites_for_budget(uint64_t n_ind, uint64_t budget_bytes);
/* (0.4.0) The same with the matrix priced `matrix_copies` times per context: 1 = the planes only -- what a run NEEDS (SNP-called
 * input never builds the store; un-called input without room for it has its flagged pairs replayed on host threads, slower and
 * the same bytes), 3 = ngsld_slab_sites_for_budget.  A caller that cannot stream (text input, no window) asks with 1 before it
 * gives up. */
uint64_t ngsld_sites_for_budget(uint64_t n_ind, uint64_t budget_bytes, int matrix_copies);

/* (0.4.0) ngsld_replay_info of the last ngsld_run_streamed / ngsld_run_streamed_text of this process, added up over its slabs
 * (exact_store: the largest of the slabs' values; sites_degenerate counts a halo site once per slab that holds it). */
int ngsld_streamed_replay_info(ngsld_replay_stats_t *out);

/* (0.4.0) A cap, in bytes, on the device memory this PROCESS takes on `device` from now on (0: none) -- what the drop-in binary's
 * --max_gpu_mem sets.  Slab sizes are the caller's to plan (ngsld_slab_sites_for_budget); the cap is looked at where the library
 * allocates what it can do without: the exact store of the device-side replay (without room: flagged pairs on host threads) and
 * its individual-major copy (without room: the wavefront-per-pair replay kernel, which reads the store's own layout). */
int ngsld_set_memory_budget(int device, uint64_t bytes);

/* Free and total memory of HIP device `device`, in bytes. */
int ngsld_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);


/* The whole job, slab by slab: create two contexts on `device`, and for every slab read -> ngsld_set_geno_raw_opts
 * -> ngsld_set_pos_dist -> ngsld_plan (first_row = row_begin) -> ngsld_run.  The sink sees the batches of all
 * slabs in global (s1, s2) order with GLOBAL site indices in ngsld_batch and ngsld_item.  maf_out (n_sites
 * doubles, may be NULL) receives est_maf of every site; entries are final before the first batch that refers to
 * them is handed to the sink.  pos_dist: n_sites doubles or NULL.  err (may be NULL) receives the message. */
int ngsld_run_streamed(int device, uint64_t n_sites, uint64_t n_ind, const double *pos_dist,
                       const ngsld_params *params, const ngsld_geno_opts *opts, uint64_t max_slab_sites,
                       ngsld_read_sites_fn read, void *read_user, double *maf_out, ngsld_sink_fn sink,
                       void *sink_user, uint64_t *n_pairs, uint64_t *n_slabs, char *err, size_t errlen);

/* The same with device-side TSV (ngsld_set_text_output on every slab): labels = n_sites C strings or NULL ("(null)"),
 * text_output != 0 makes the sink receive text batches (ngsld_batch.text), in global (s1, s2) order. */
int ngsld_run_streamed_text(int device, uint64_t n_sites, uint64_t n_ind, const double *pos_dist,
                            const ngsld_params *params, const ngsld_geno_opts *opts, uint64_t max_slab_sites,
                            ngsld_read_sites_fn read, void *read_user, double *maf_out, ngsld_sink_fn sink,
                            void *sink_user, uint64_t *n_pairs, uint64_t *n_slabs, char *err, size_t errlen,
                            const char *const *labels, int text_output);

/* ---- Several GPUs of one node, one process (replaces the thread-pool section of the reference's main(),
 * ngsLD.cpp:153-198, at the scale of devices) ----------------------------------------------------------------------
 * The rows are cut into n_devices contiguous parts with equal candidate-pair counts; part k runs on devices[k] from its
 * own host thread and holds only the sites its rows pair with.  Pairs are independent, so nothing is exchanged while
 * computing; the records of the parts, in part order, are the single-device run bit for bit. */

/* Cut rows [0, n_sites) into n_parts parts: parts[k] = {row_begin, row_end, site_end} -- part k computes the rows
 * [row_begin, row_end) and needs the sites [row_begin, site_end).  Host only. */
int ngsld_plan_parts(const double *pos_dist, uint64_t n_sites, const ngsld_params *params, int n_parts, ngsld_slab *parts);

/* Sink of a multi-device run: called on part `part`'s own thread -- the batches of one part arrive in (s1, s2) order,
 * different parts call concurrently.  Site indices in the batch are global. */
typedef int (*ngsld_multi_sink_fn)(void *user, int part, const ngsld_batch *batch);

/* The whole job: gl_raw = the matrix in host memory ([site][ind][3], as ngsld_set_geno_raw_opts takes it), or NULL and
 * `read` delivers the raw values of any site range (it is called from several threads at once).  A windowed run uploads
 * every part's slab from host memory over the part's own PCIe link; an all-pairs run on >= 2 distinct devices puts the
 * matrix on the first device once and hands it to the others with ONE ncclBroadcast (RCCL over xGMI, loaded on demand).
 * maf_out (n_sites doubles, may be NULL) receives est_maf; it is complete before the first batch reaches the sink.
 * labels / text_output as in ngsld_run_streamed_text.  pairs_per_part (n_devices entries, may be NULL) receives the
 * pairs each part computed.  Every part must fit its device (a job that does not is for ngsld_run_streamed). */
int ngsld_run_multi(const int *devices, int n_devices, uint64_t n_sites, uint64_t n_ind, const double *pos_dist,
                    const ngsld_params *params, const ngsld_geno_opts *opts, const double *gl_raw,
                    ngsld_read_sites_fn read, void *read_user, double *maf_out, ngsld_multi_sink_fn sink, void *sink_user,
                    const char *const *labels, int text_output, uint64_t *pairs_per_part, char *err, size_t errlen);

/* How the last ngsld_run_multi of this process handed the matrix to its devices (the one collective of the
 * design is this broadcast): uploaded slab by slab over each part's own PCIe link, copied device to device from the first
 * device, or ONE ncclBroadcast over RCCL / xGMI. */
enum { NGSLD_DIST_NONE = 0, NGSLD_DIST_UPLOAD = 1, NGSLD_DIST_PEER_COPY = 2, NGSLD_DIST_RCCL = 3 };
int ngsld_multi_last_distribution(void);

/* The RCCL calls of ngsld_run_multi's broadcast -- dlopen of librccl, ncclCommInitAll, ncclGroupStart / ncclBroadcast /
 * ncclGroupEnd, ncclCommDestroy -- on a communicator of ONE device: `bytes` of a known pattern go to the device, through an
 * in-place broadcast, and back.  What a one-GPU box can prove about that path; NGSLD_OK, or NGSLD_ERR_DEVICE with the
 * reason in err. */
int ngsld_rccl_selftest(int device, uint64_t bytes, char *err, size_t errlen);

/* ---- LD pruning on the device (PRUNE.md) ------------------------------------------------------------------------------
 * The sites the reference's scripts/prune_graph.pl keeps (its prune_graph_idx path) for the TSV this context's plan would
 * print -- without the TSV: the pairs run again chunk by chunk into device records (every pair kernel, the exact-order replay
 * included), the edges are taken from them on the device, the graph is built and pruned there, a small remainder on the host.
 * A site is a node iff it is one end of a planned pair (and in the subset, when one is given); edge weights are the chosen
 * field as printed ("%f" read back), the rule and its deviations are in PRUNE.md.  Both structs start with struct_size: set it
 * to sizeof(the struct) of your header (params: must equal this library's; stats: up to that many bytes are written). */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_prune_params) */
  int32_t field;              /* TSV column of the weight: 4 r2_ExpG, 5 D, 6 D', 7 r2 (the script's --field_weight, default 7) */
  double max_kb_dist;         /* an edge needs dist <= max_kb_dist * 1000 (INFINITY: no limit) */
  double min_weight;          /* an edge needs weight >= min_weight (default 0) */
  int32_t weight_type;        /* 'a' |weight| (default), 'e' weight as it is, 'n' every edge counts 1 */
  int32_t keep_heavy;         /* != 0: the heaviest node stays and its neighbours go */
  int32_t precision;          /* edge label = trunc(weight * 10^precision), 0..15 (default 4) */
  int32_t reserved;           /* 0 */
  const char *const *subset;  /* NULL: every site; else n_subset labels -- only those sites are nodes */
  uint64_t n_subset;
} ngsld_prune_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_prune_stats) */
  uint32_t reserved;
  uint64_t pairs;             /* pairs computed */
  uint64_t nodes, edges;      /* of the graph */
  uint64_t kept, excluded;    /* nodes == kept + excluded */
  uint64_t rounds;            /* parallel rounds on the device */
  uint64_t host_nodes, host_edges, host_steps;  /* the remainder finished on the host, and its heaviest-node steps */
  double pairs_ms, edges_ms, graph_ms, rounds_ms, host_ms, total_ms;  /* phases: pair kernels + replay, edge extraction
                                                 (kernel time), CSR build, device rounds, host finish, the whole call */
} ngsld_prune_stats;

/* Prune after ngsld_plan.  labels = n_sites C strings, the TSV's first two columns (NULL: every label is "(null)").
 * site_state[n_sites] receives 0 (not a node), 1 (kept) or 2 (excluded).  stats may be NULL.  Two node sites with the same
 * label: NGSLD_ERR_INVALID naming it; an edge label of 2^62 or more: NGSLD_ERR_UNSUPPORTED naming the pair. */
int ngsld_prune(ngsld_ctx *ctx, const ngsld_prune_params *params, const char *const *labels, uint8_t *site_state,
                ngsld_prune_stats *stats);

/* ---- LD decay on the device (DECAY.md) -----------------------------------------------------------------------------------
 * The bins the reference's scripts/fit_LDdecay.R averages (its default mean, --fit_bin_size > 1) for the TSV this context's
 * plan would print -- without the TSV: the pairs run again chunk by chunk into device records (every pair kernel, the
 * exact-order replay included) and a kernel bins them.  A row counts iff both printed maf >= min_maf, dist (as printed) is finite
 * and < max_kb_dist * 1000, and every chosen field is finite; it goes to the right-closed bin (k*B, (k+1)*B], reported at k*B.
 * A bin's mean is the double nearest to the exact mean of the printed ("%f") values: the sums are exact integers.  The rule
 * and its deviations are in DECAY.md.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_decay_params) */
  uint32_t fields;            /* mask of the TSV columns binned: 1 r2_ExpG, 2 D, 4 D' (the script's Dp), 8 r2 (its default) */
  double bin_size;            /* B > 1 (the script's --fit_bin_size, default 250) */
  double max_kb_dist;         /* a row needs dist < max_kb_dist * 1000 (INFINITY: no limit, the script's default) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
} ngsld_decay_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_decay_stats) */
  uint32_t lds;               /* 1: the bins were accumulated per workgroup in LDS, 0: in global memory */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows in some bin */
  uint64_t bins;              /* non-empty bins (what ngsld_decay_bins returns) */
  uint64_t bin_slots;         /* bins sized from the plan */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, bin_ms, total_ms;  /* pair kernels + replay, the bin kernel (kernel time), the whole call */
} ngsld_decay_stats;

/* Bin after ngsld_plan; the context keeps the bins until the next ngsld_decay.  stats may be NULL.  NGSLD_ERR_UNSUPPORTED for a
 * value of 2^38 micro-units or more (|x| >= 274877.906944, naming the pair), a finite max_kb_dist with non-integer position
 * gaps, or more than 2^22 bins. */
int ngsld_decay(ngsld_ctx *ctx, const ngsld_decay_params *params, ngsld_decay_stats *stats);
/* The last ngsld_decay's non-empty bins in increasing distance: up to cap of them into dist[] (the bin's lower break),
 * count[] (rows) and mean[] (one value per chosen field, in TSV column order: mean[i * n_fields + f]).  Any pointer may be
 * NULL; *n_bins (may be NULL) receives the number of bins. */
int ngsld_decay_bins(ngsld_ctx *ctx, uint64_t cap, double *dist, uint64_t *count, double *mean, uint64_t *n_bins);

/* ---- LD blocks on the device (BLOCKS.md) ----------------------------------------------------------------------------------
 * The square matrices the reference's scripts/LD_blocks.sh hands to LDheatmap for one region CHR:START-END, for the TSV this
 * context's plan would print -- without the TSV: only the rows of the region's sites run again (chunk by chunk into device
 * records, every pair kernel and the exact-order replay included), a kernel scatters their pairs into dense matrices and a
 * formatter writes them as text.  A site is a member iff its label (up to the first TAB) is CHR ":" p with START <= p <= END;
 * the matrix holds the members that are one end of an in-region pair, ordered by p.  Cell [a][b] is the pair (a, b) with a
 * the earlier site of the file, NA elsewhere (the diagonal included); a cell's text is what the TSV prints for that pair.
 * Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_blocks_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (the script's pair: 4 | 8) */
  const char *chr;            /* CHR */
  uint64_t start, end;        /* START < END, both inclusive */
} ngsld_blocks_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_blocks_stats) */
  uint32_t reserved;
  uint64_t members, sites;    /* region members; matrix sites (members that are one end of an in-region pair) */
  uint64_t pairs, pairs_in_region;  /* pairs computed (the members' rows only); of them in the region */
  uint64_t cells_na, host_rows, chunks;  /* NA cells of a matrix; text rows formatted on the host; chunks of rows the pairs
                                            ran in */
  double pairs_ms, scatter_ms, format_ms, total_ms;  /* pair kernels + replay, the scatter and site kernels (kernel time),
                                                 text (ngsld_blocks_text), the whole ngsld_blocks call */
} ngsld_blocks_stats;

/* Block matrices after ngsld_plan; the context keeps them until the next ngsld_blocks, ngsld_plan or ngsld_set_*.  labels =
 * n_sites C strings, the TSV's first two columns (NULL or "(null)" labels: NGSLD_ERR_INVALID, blocks need positions).  No
 * in-region pair: NGSLD_OK with sites == 0.  NGSLD_ERR_UNSUPPORTED, naming the label, for a site of CHR whose position is not
 * plain decimal digits or two members at one position; also for more than 2^15 members or matrices the device has no room
 * for (fields x members^2 x 8 + members^2 bytes).  stats may be NULL. */
int ngsld_blocks(ngsld_ctx *ctx, const ngsld_blocks_params *params, const char *const *labels, ngsld_blocks_stats *stats);
/* The matrix sites of the last ngsld_blocks in matrix order (increasing position): up to cap site indices into site[];
 * *n_sites (may be NULL) receives their number. */
int ngsld_blocks_sites(ngsld_ctx *ctx, uint64_t cap, uint64_t *site, uint64_t *n_sites);
/* One chosen statistic's matrix (field = TSV column 4..7), sites x sites in matrix order, row-major: values[] the records'
 * doubles (NaN where no pair is), present[] 1 where a pair is; either pointer may be NULL. */
int ngsld_blocks_matrix(ngsld_ctx *ctx, int field, double *values, uint8_t *present);
/* One chosen statistic's matrix as a file (BLOCKS.md: a label row, then a label and sites cells per row), handed to sink in
 * order, in chunks; a sink that returns non-zero stops it (NGSLD_ERR_SINK).  stats (may be NULL): the call's format_ms (its
 * time outside the sink) and host_rows are added to it. */
typedef int (*ngsld_text_fn)(void *user, const char *text, uint64_t len);
int ngsld_blocks_text(ngsld_ctx *ctx, int field, ngsld_text_fn sink, void *user, ngsld_blocks_stats *stats);

/* ---- Per-site LD summaries on the device (SITES.md) -------------------------------------------------------------------------
 * The TSV this context's plan would print, collapsed per site -- without the TSV: the pairs run again chunk by chunk into
 * device records (every pair kernel, the exact-order replay included) and a kernel adds every counted row to BOTH of its
 * sites.  A row counts iff dist (as printed) is finite and <= max_kb_dist * 1000, both printed maf >= min_maf, and every chosen
 * field is finite.  Per site: the counted rows it is in, and per chosen field the sum (its LD score, the site itself not
 * included), the maximum and the mean of the printed ("%f") values -- |value| with abs_value -- and the rows whose value is
 * >= linked_min.  Sums and maxima are exact integers in micro-units (value * 10^6); the mean is the double nearest to the
 * exact mean.  The rule and its deviations are in SITES.md.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_site_ld_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (default) */
  double max_kb_dist;         /* a row needs dist <= max_kb_dist * 1000 (INFINITY: no limit, the default) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  double linked_min;          /* a row is linked in a field iff its value >= linked_min (default 0.5) */
  int32_t abs_value;          /* != 0 (default): |value|, as pruning's weight type 'a'; 0: the signed value */
  int32_t reserved;           /* 0 */
} ngsld_site_ld_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_site_ld_stats) */
  uint32_t lds;               /* 1: accumulated per tile of rows in LDS, 0: in global memory */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows that count */
  uint64_t sites_with_pairs;  /* sites in at least one counted row */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, site_ms, total_ms;  /* pair kernels + replay, the site kernel (kernel time), the whole call */
} ngsld_site_ld_stats;

/* Summaries after ngsld_plan; the context keeps them until the next ngsld_site_ld, ngsld_plan or ngsld_set_*.  stats may be
 * NULL.  NGSLD_ERR_UNSUPPORTED for a value of 2^38 micro-units or more (|x| >= 274877.906944, naming the pair), a site whose
 * sum could pass 2^63 micro-units, or a finite max_kb_dist with non-integer position gaps. */
int ngsld_site_ld(ngsld_ctx *ctx, const ngsld_site_ld_params *params, ngsld_site_ld_stats *stats);
/* The last ngsld_site_ld's arrays of one chosen statistic (field = TSV column 4..7), n_sites entries each, any pointer may be
 * NULL: n[] counted rows (the same for every field), sum_micro[] and max_micro[] in micro-units, linked[], mean[].  Where
 * n[s] == 0: sum 0, linked 0, max_micro INT64_MIN, mean NaN. */
int ngsld_site_ld_get(ngsld_ctx *ctx, int field, uint64_t *n, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked,
                      double *mean);

/* ---- LD clusters on the device (CLUSTERS.md) --------------------------------------------------------------------------------
 * The connected components of the graph ngsld_prune prunes -- without the TSV and without an edge list: the pairs run again
 * chunk by chunk into device records (every pair kernel, the exact-order replay included) and a kernel unites the two sites of
 * every edge in a lock-free union-find of one word per site.  A site is a node iff it is one end of an emitted pair.  An
 * emitted pair is an edge iff dist (as printed) is finite and <= max_kb_dist * 1000, both printed maf >= min_maf, the chosen
 * field is finite and its printed ("%f") value -- |value| with abs_value -- is >= min_weight.  Clusters are numbered 1, 2, ...
 * in increasing order of their smallest site, singletons included; a site that is not a node has cluster 0.  The rule and its
 * deviations are in CLUSTERS.md.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_clusters_params) */
  int32_t field;              /* TSV column of the edge value: 4 r2_ExpG, 5 D, 6 D', 7 r2 (default) */
  double max_kb_dist;         /* an edge needs dist <= max_kb_dist * 1000 (INFINITY: no limit, the default) */
  double min_maf;             /* an edge needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  double min_weight;          /* an edge needs value >= min_weight (default 0.5; a value equal to it is an edge) */
  int32_t abs_value;          /* != 0 (default): |value|, as pruning's weight type 'a'; 0: the signed value */
  int32_t reserved;           /* 0 */
} ngsld_clusters_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_clusters_stats) */
  uint32_t reserved;          /* 0 */
  uint64_t pairs;             /* pairs computed */
  uint64_t nodes;             /* sites that are one end of an emitted pair */
  uint64_t edges;             /* pairs that are edges */
  uint64_t clusters;          /* clusters, singletons included */
  uint64_t clusters_multi;    /* clusters of two sites or more */
  uint64_t largest;           /* sites of the largest cluster */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  uint64_t union_launches;    /* launches of the union kernel: one per chunk (per 2^24 work items of it), whatever the diameter */
  double pairs_ms, union_ms, finish_ms, total_ms;  /* pair kernels + replay, the union kernel (kernel time), flatten + copy
                                                      back + the host's pass over the sites, the whole call */
} ngsld_clusters_stats;

/* Clusters after ngsld_plan; the context keeps them until the next ngsld_clusters, ngsld_plan or ngsld_set_*.  stats may be
 * NULL.  NGSLD_ERR_UNSUPPORTED for non-integer position gaps (the limit and the spans come from the positions' prefix sums), a
 * value of 2^38 micro-units or more (|x| >= 274877.906944, naming the pair), or a cluster whose sum could pass 2^63
 * micro-units. */
int ngsld_clusters(ngsld_ctx *ctx, const ngsld_clusters_params *params, ngsld_clusters_stats *stats);
/* The last ngsld_clusters' cluster id of every site: n_sites entries, 0 for a site that is not a node. */
int ngsld_clusters_sites(ngsld_ctx *ctx, uint32_t *cluster);
/* The last ngsld_clusters' table: one row per cluster of at least min_size sites, in id order, up to cap rows into each array
 * that is not NULL; *n (may be NULL) receives the number of such clusters.  first[] and last[] are the smallest and largest
 * site index, span[] the dist the TSV would print for that pair (0 for a singleton), sum_micro[] the sum of the edges' values
 * in micro-units (value * 10^6), mean[] the double nearest to sum / (10^6 * edges) (NaN without edges), density[] the double
 * nearest to edges / (size * (size - 1) / 2) (NaN for a singleton). */
int ngsld_clusters_table(ngsld_ctx *ctx, uint64_t min_size, uint64_t cap, uint32_t *id, uint32_t *size, uint32_t *first,
                         uint32_t *last, uint64_t *span, uint64_t *edges, int64_t *sum_micro, double *mean, double *density,
                         uint64_t *n);

/* ---- LD tree on the device (TREE.md) ----------------------------------------------------------------------------------------
 * The single-linkage tree of the sites: the maximum spanning forest of the graph ngsld_clusters unites, kept on the device while
 * the rows stream past -- without the TSV and without the graph's edge list.  Nodes and edges are those of ngsld_clusters.  Edge
 * e comes before edge f iff q_e > q_f (the printed value in micro-units, |q| with abs_value), or the q are equal and
 * s1_e < s1_f, or those are equal too and s2_e < s2_f; the edges taken in that order, an edge is kept iff its two ends lie in
 * different trees so far.  The kept edges, in that order, are the merges 1..M, M = nodes - clusters at the floor min_weight; every
 * cut of them at a floor t >= min_weight is what ngsld_clusters gives at min_weight = t (ngsld_ld_tree_cut).  The rule is in
 * TREE.md.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_ld_tree_params) */
  int32_t field;              /* TSV column of the edge value: 4 r2_ExpG, 5 D, 6 D', 7 r2 (default) */
  double max_kb_dist;         /* an edge needs dist <= max_kb_dist * 1000 (INFINITY: no limit, the default) */
  double min_maf;             /* an edge needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  double min_weight;          /* an edge needs value >= min_weight (default 0.1; a value equal to it is an edge): the lowest cut */
  int32_t abs_value;          /* != 0 (default): |value|; 0: the signed value */
  int32_t reserved;           /* 0 */
} ngsld_ld_tree_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_ld_tree_stats) */
  uint32_t reserved;          /* 0 */
  uint64_t pairs;             /* pairs computed */
  uint64_t nodes;             /* sites that are one end of an emitted pair */
  uint64_t edges;             /* pairs that are edges: the candidates that passed */
  uint64_t merges;            /* edges of the forest */
  uint64_t clusters;          /* clusters at the floor, singletons included: nodes - merges */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  uint64_t rounds;            /* rounds of all the reduces (a chunk without a candidate has no reduce) */
  uint64_t max_rounds;        /* the most rounds of one reduce: at most ceil(log2(n_sites)) + 1, whatever the diameter */
  uint64_t displaced;         /* forest edges that a later chunk's reduce dropped */
  double pairs_ms, edges_ms, reduce_ms, finish_ms, total_ms;  /* pair kernels + replay, the candidates kernel (kernel time), the
                                                                 reduces (wall time), copy back + the host's pass, the whole call */
} ngsld_ld_tree_stats;

/* The tree after ngsld_plan; the context keeps it until the next ngsld_ld_tree, ngsld_plan or ngsld_set_*.  stats may be NULL.
 * NGSLD_ERR_UNSUPPORTED for non-integer position gaps or a value of 2^38 micro-units or more (|x| >= 274877.906944, naming the
 * pair); nothing is summed, so no sum can wrap. */
int ngsld_ld_tree(ngsld_ctx *ctx, const ngsld_ld_tree_params *params, ngsld_ld_tree_stats *stats);
/* The last ngsld_ld_tree's merges in rule order, up to cap rows into each array that is not NULL; *n (may be NULL) receives the
 * number of merges.  Merge k (from 1) joins the clusters that held s1[k-1] and s2[k-1] through the edge of q_micro[k-1]
 * micro-units and dist[k-1] bp (what the TSV prints); left[] and right[] name those two clusters as R's hclust$merge does --
 * -(site index + 1) for a single site, the number of the merge that made it otherwise --; size[] is the number of sites after
 * the merge, first[] and last[] the smallest and largest site index of the merged cluster. */
int ngsld_ld_tree_merges(ngsld_ctx *ctx, uint64_t cap, uint32_t *s1, uint32_t *s2, int64_t *q_micro, uint64_t *dist, int64_t *left,
                         int64_t *right, uint32_t *size, uint32_t *first, uint32_t *last, uint64_t *n);
/* The clusters of the last ngsld_ld_tree at the floor t: cluster[] (n_sites entries, may be NULL) and *n_clusters (may be NULL)
 * are what ngsld_clusters_sites and its stats give at min_weight = t with the other parameters equal -- ids 1, 2, ... in
 * increasing order of the smallest site, singletons included, 0 for a site that is not a node.  A host pass over the stored
 * merges: no device work.  NGSLD_ERR_INVALID for a NaN or a t below the tree's min_weight. */
int ngsld_ld_tree_cut(ngsld_ctx *ctx, double t, uint32_t *cluster, uint64_t *n_clusters);

/* ---- LD grid on the device (GRID.md) ----------------------------------------------------------------------------------------
 * The TSV this context's plan would print, binned into a heat map along each chromosome -- without the TSV: the pairs run again
 * chunk by chunk into device records (every pair kernel, the exact-order replay included) and a kernel adds every counted row to
 * ONE cell.  A site's position p and chromosome come from its label (up to the first TAB: CHR ":" p); its bin is p / bin_size in
 * integer division; a counted row (s1, s2) belongs to the cell (chromosome, bin(s1), bin(s2)).  A row counts iff dist (as
 * printed) is finite and <= max_kb_dist * 1000, both printed maf >= min_maf, and every chosen field is finite.  Per cell: the
 * counted rows, and per chosen field the sum, the maximum and the mean of the printed ("%f") values -- |value| with abs_value --
 * and the rows whose value is >= linked_min.  Sums and maxima are exact integers in micro-units (value * 10^6); the mean is the
 * double nearest to the exact mean.  The rule and its refusals are in GRID.md.  Both structs start with struct_size, as the
 * pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_grid_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (default) */
  uint64_t bin_size;          /* B: the window in bp, 1 <= B < 2^31 */
  double max_kb_dist;         /* a row needs dist <= max_kb_dist * 1000 (INFINITY: no limit, the default) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  double linked_min;          /* a row is linked in a field iff its value >= linked_min (default 0.5) */
  int32_t abs_value;          /* != 0 (default): |value|, as pruning's weight type 'a'; 0: the signed value */
  int32_t reserved;           /* 0 */
} ngsld_grid_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_grid_stats) */
  uint32_t lds;               /* 1: accumulated per tile of rows in LDS, 0: in global memory */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows that count: the sum of n over the cells */
  uint64_t cells;             /* cells with rows (what ngsld_grid_cells returns) */
  uint64_t bins;              /* bins between the first and the last site of every chromosome */
  uint64_t band;              /* K: the bins a row's candidates reach, from the plan; the accumulators hold bins x K cells */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, grid_ms, total_ms;  /* pair kernels + replay, the grid kernel (kernel time), the whole call */
} ngsld_grid_stats;

/* The grid after ngsld_plan; the context keeps it until the next ngsld_grid, ngsld_plan or ngsld_set_*.  labels = n_sites C
 * strings, the TSV's first two columns (NULL or "(null)" labels: NGSLD_ERR_INVALID, the grid needs positions).  stats may be
 * NULL.  NGSLD_ERR_UNSUPPORTED, naming the site, for a position that is not plain decimal digits, positions that decrease
 * inside a chromosome, a chromosome name that begins two runs of sites, or label chromosomes that disagree with pos_dist (a
 * chromosome changes exactly where the gap is +inf); also for a value of 2^38 micro-units or more (|x| >= 274877.906944, naming
 * the pair), a cell whose sum could pass 2^63 micro-units, a finite max_kb_dist with non-integer position gaps, or accumulators
 * of more than 2 GiB ((1 + 3 x fields) x bins x band x 8 B: a larger bin_size is needed). */
int ngsld_grid(ngsld_ctx *ctx, const ngsld_grid_params *params, const char *const *labels, ngsld_grid_stats *stats);
/* The last ngsld_grid's cells with rows, ordered by chromosome (file order), bin1, bin2: up to cap of them into chr[] (index
 * into ngsld_grid_chromosomes' names), bin1[] and bin2[] (the bins b = p / bin_size of the pair's first and second site; the
 * window is [b * bin_size, (b + 1) * bin_size)) and n[] (rows).  Any pointer may be NULL; *n_cells (may be NULL) receives the
 * number of cells. */
int ngsld_grid_cells(ngsld_ctx *ctx, uint64_t cap, uint32_t *chr, uint64_t *bin1, uint64_t *bin2, uint64_t *n, uint64_t *n_cells);
/* The chromosomes of the last ngsld_grid in file order: up to cap names into name[] (the context's strings: valid while the
 * result is); *n_chr (may be NULL) receives their number. */
int ngsld_grid_chromosomes(ngsld_ctx *ctx, uint64_t cap, const char **name, uint64_t *n_chr);
/* The last ngsld_grid's arrays of one chosen statistic (field = TSV column 4..7), in the order of ngsld_grid_cells, up to cap
 * entries each, any pointer may be NULL: sum_micro[] and max_micro[] in micro-units, linked[], mean[]. */
int ngsld_grid_get(ngsld_ctx *ctx, int field, uint64_t cap, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked, double *mean);

/* ---- Linked pairs on the device (LINKED.md) ---------------------------------------------------------------------------------
 * The rows of the TSV this context's plan would print that pass a filter, in the table's own order -- without the TSV: the pairs
 * run again chunk by chunk into device records (every pair kernel, the exact-order replay included), a kernel applies the filter
 * and measures the surviving rows, two prefix sums place them, and a second kernel stores them compactly: the two sites and the
 * record(s) of every linked row, and (or) its text, byte for byte the row of the full table.  An emitted pair is a linked row iff
 * the chosen field is finite and its printed ("%f") value -- |value| with abs_value -- is >= min_weight, both printed maf >=
 * min_maf, and -- only with a finite max_kb_dist -- dist (as printed) is finite and <= max_kb_dist * 1000.  With the default
 * INFINITY there is no condition on dist at all: rows across chromosomes and rows without positions pass.  The rule and its
 * deviations are in LINKED.md.  Both structs start with struct_size, as the pruning structs do. */
enum {
  NGSLD_LINKED_RECORDS = 1,   /* s1, s2, std (and ext where the plan has extend_out) */
  NGSLD_LINKED_TEXT = 2       /* the rows' text */
};

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_linked_params) */
  int32_t field;              /* TSV column of the value: 4 r2_ExpG, 5 D, 6 D', 7 r2 (default) */
  double min_weight;          /* a row needs value >= min_weight (default 0.5; a value equal to it passes; -INFINITY allowed) */
  double max_kb_dist;         /* finite: a row needs dist <= max_kb_dist * 1000; INFINITY (default): no condition on dist */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  int32_t abs_value;          /* != 0 (default): |value|, as pruning's weight type 'a'; 0: the signed value */
  int32_t want;               /* NGSLD_LINKED_RECORDS | NGSLD_LINKED_TEXT, at least one */
} ngsld_linked_params;

/* The linked rows of one chunk of the table's rows, in the table's order.  Pointers are valid only during the callback; the
 * arrays that were not asked for are NULL (text_len 0). */
typedef struct {
  uint64_t n;                 /* linked rows in this batch (> 0) */
  const uint32_t *s1, *s2;    /* [n] the two sites */
  const ngsld_rec_std *std;   /* [n] */
  const ngsld_rec_ext *ext;   /* [n], NULL unless the plan has extend_out */
  const char *text;           /* the n rows, each as the full table prints it */
  uint64_t text_len;
} ngsld_linked_batch;

typedef int (*ngsld_linked_fn)(void *user, const ngsld_linked_batch *b);

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_linked_stats) */
  uint32_t reserved;          /* 0 */
  uint64_t pairs;             /* pairs computed */
  uint64_t rows;              /* linked rows handed to the sink */
  uint64_t text_bytes;        /* bytes of text handed to the sink */
  uint64_t host_rows;         /* rows the host formatter wrote (a value beyond the device formatter's range in their chunk) */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, kernel_ms, total_ms;  /* pair kernels + replay, the count + scan + write kernels (kernel time), the whole call */
  double count_ms, scan_ms, write_ms;    /* kernel_ms by kernel */
} ngsld_linked_stats;

/* The linked rows after ngsld_plan, streamed: the sink is called once per chunk of the table's rows that has linked rows, in
 * order, on the calling thread.  A non-zero return of the sink ends the call with that value; the context stays usable.  labels
 * = n_sites C strings, the TSV's first two columns (NULL: every label prints "(null)"); read only when text is wanted.  The
 * extended columns are in the text iff the plan has extend_out.  stats may be NULL.  NGSLD_ERR_INVALID for a field outside 4..7,
 * a NaN min_weight, a max_kb_dist that is NaN or below 0, a min_maf that is NaN, negative or infinite, or want == 0;
 * NGSLD_ERR_UNSUPPORTED for a finite max_kb_dist with non-integer position gaps. */
int ngsld_linked_pairs(ngsld_ctx *ctx, const ngsld_linked_params *params, const char *const *labels, ngsld_linked_fn sink,
                       void *user, ngsld_linked_stats *stats);

/* ---- LD partners on the device (PARTNERS.md) --------------------------------------------------------------------------------
 * For every site -- or every site of a query -- the k sites that tag it best, without the TSV: the pairs run again chunk by chunk
 * into device records (every pair kernel, the exact-order replay included) and a kernel keeps, per site, the k largest of its
 * partner rows.  An emitted pair (s1, s2) is a partner row iff it is a linked row of ngsld_linked_pairs under the same field,
 * min_weight, abs_value, max_kb_dist and min_maf; it makes s2 a partner of s1 and s1 a partner of s2.  A site's partners are
 * ranked by (printed value in micro-units descending -- |value| with abs_value --, partner index ascending): a total order, so
 * every launch shape gives the same lists.  The rule and its deviations are in PARTNERS.md.  Both structs start with
 * struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_partners_params) */
  uint32_t k;                 /* partners kept per site, 1..64 */
  int32_t field;              /* TSV column of the value: 4 r2_ExpG, 5 D, 6 D', 7 r2 (default) */
  int32_t abs_value;          /* != 0 (default): |value| is compared and ranked; 0: the signed value */
  double min_weight;          /* a row needs value >= min_weight (default 0.5; a value equal to it passes; -INFINITY allowed) */
  double max_kb_dist;         /* finite: a row needs dist <= max_kb_dist * 1000; INFINITY (default): no condition on dist */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
} ngsld_partners_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_partners_stats) */
  uint32_t reserved;          /* 0 */
  uint64_t pairs;             /* pairs computed */
  uint64_t rows_counted;      /* partner rows (whether or not an end of theirs collects) */
  uint64_t sites_with_partners;  /* collecting sites with a partner row */
  uint64_t entries;           /* partners kept, over all sites */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, kernel_ms, total_ms;  /* pair kernels + replay, the partners kernel (kernel time), the whole call */
} ngsld_partners_stats;

/* The lists after ngsld_plan; the context keeps them until the next ngsld_partners, ngsld_plan or ngsld_set_*, and a call that
 * fails leaves none.  query = n_sites bytes, a site collects partners iff its byte is not 0 (any site can be a partner); NULL:
 * every site.  stats may be NULL.  A plan without pairs gives empty lists.  NGSLD_ERR_INVALID for a k outside 1..64, a field
 * outside 4..7, a NaN min_weight or min_maf, a max_kb_dist that is NaN or below 0; NGSLD_ERR_UNSUPPORTED for a finite max_kb_dist
 * with non-integer position gaps, and for a finite value of 2^31 micro-units or more (|x| >= 2147.483648, naming the pair) in a
 * row that passes the maf and distance tests: nothing is wrapped or clamped. */
int ngsld_partners(ngsld_ctx *ctx, const ngsld_partners_params *params, const uint8_t *query, ngsld_partners_stats *stats);
/* The shape of the last ngsld_partners' lists (any pointer may be NULL); NGSLD_ERR_INVALID when there is none. */
int ngsld_partners_info(ngsld_ctx *ctx, uint32_t *k, uint64_t *n_sites, uint32_t *field);
/* The last ngsld_partners' lists, any pointer may be NULL: rows[n_sites] the site's partner rows before the cut to k,
 * partner[n_sites * k] site indices in rank order (0xFFFFFFFF: none, from min(k, rows) on), value_micro[n_sites * k] the
 * partner row's printed value * 10^6, signed as in the table unless abs_value (0 where there is no partner). */
int ngsld_partners_get(ngsld_ctx *ctx, uint64_t *rows, uint32_t *partner, int64_t *value_micro);

/* ---- LD scan on the device (SCAN.md) ----------------------------------------------------------------------------------------
 * The TSV this context's plan would print, scanned with a window centred on every site -- without the TSV: the pairs run again
 * chunk by chunk into device records (every pair kernel, the exact-order replay included) and a kernel adds every counted row
 * to the windows it is in.  The window of a site c holds the sites of its chromosome within half_window bp of it: an index
 * range [win_first, win_last]; its left flank is [win_first, c], its right flank [c + 1, win_last].  A row counts iff dist (as
 * printed) is finite and <= max_kb_dist * 1000, both printed maf >= min_maf, and every chosen field is finite; a counted row
 * (s1, s2) is in window c iff win_first <= s1 and s2 <= win_last, and there it is LL (s2 <= c), RR (s1 > c) or LR (across c).
 * Per site: the rows of each class, and per chosen field the sums of |printed ("%f") value| of each class in micro-units
 * (value * 10^6), zns = the double nearest to the mean over all three classes (Kelly's ZnS), omega = the double nearest to
 * ((S_LL + S_RR) * n_LR) / ((n_LL + n_RR) * S_LR) (Kim and Nielsen's omega).  The rule and its refusals are in SCAN.md.  Both
 * structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_scan_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (default) */
  uint64_t half_window;       /* H: a window reaches H bp to either side of its site, 0 <= H < 2^31 */
  double max_kb_dist;         /* a row needs dist <= max_kb_dist * 1000 (INFINITY: no limit, the default) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  uint64_t reserved;          /* 0 */
} ngsld_scan_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_scan_stats) */
  uint32_t reserved;          /* 0 */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows that count (in a window or not) */
  uint64_t largest_window;    /* sites of the largest window */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, scan_ms, total_ms;  /* pair kernels + replay, the scan kernel and the prefix sums (kernel time), the whole call */
} ngsld_scan_stats;

/* The scan after ngsld_plan; the context keeps it until the next ngsld_scan, ngsld_plan or ngsld_set_*.  stats may be NULL.
 * NGSLD_ERR_INVALID for a plan whose distance window (ngsld_params.max_kb_dist > 0) is below 2 * half_window bp: a window would
 * hold site pairs the table never had.  NGSLD_ERR_UNSUPPORTED for non-integer position gaps (the windows come from the
 * positions' prefix sums), a value of 2^38 micro-units or more (|x| >= 274877.906944, naming the pair), or a window whose sum
 * could pass 2^63 micro-units. */
int ngsld_scan(ngsld_ctx *ctx, const ngsld_scan_params *params, ngsld_scan_stats *stats);
/* The last ngsld_scan's arrays, n_sites entries each, any pointer may be NULL: win_first[] and win_last[] (site indices), the
 * rows n_ll[], n_rr[], n_lr[] (the same for every field), and of one chosen statistic (field = TSV column 4..7) the sums
 * sum_ll[], sum_rr[], sum_lr[] in micro-units, zns[] (NaN where the window has no row) and omega[] (NaN where n_ll + n_rr,
 * n_lr or sum_lr is 0). */
int ngsld_scan_get(ngsld_ctx *ctx, int field, uint32_t *win_first, uint32_t *win_last, uint64_t *n_ll, uint64_t *n_rr,
                   uint64_t *n_lr, int64_t *sum_ll, int64_t *sum_rr, int64_t *sum_lr, double *zns, double *omega);

/* ---- several analyses over one run of the pair kernels ----
 * ngsld_prune, ngsld_decay, ngsld_site_ld, ngsld_clusters, ngsld_grid and ngsld_scan each run every planned pair through the pair
 * kernels.  ngsld_analyze runs the pairs once, chunk of rows by chunk, and every listed analysis reads each chunk's records in
 * list order; the results are the single calls' bit for bit and are read through the single calls' getters (pruning's through
 * site_state).  ANALYZE.md has the rule.  ngsld_blocks, ngsld_linked_pairs and ngsld_partners stay calls of their own. */
enum { NGSLD_AN_PRUNE = 1, NGSLD_AN_DECAY, NGSLD_AN_SITE_LD, NGSLD_AN_CLUSTERS, NGSLD_AN_GRID, NGSLD_AN_SCAN };

typedef struct ngsld_analysis {
  uint32_t struct_size;         /* sizeof(ngsld_analysis) */
  uint32_t kind;                /* NGSLD_AN_* */
  const void *params;           /* the kind's own ngsld_*_params */
  void *stats;                  /* the kind's own ngsld_*_stats, filled as by its single call (pairs_ms is the shared figure); may be NULL */
  const char *const *labels;    /* prune, grid: as in the single call; NULL otherwise */
  uint8_t *site_state;          /* prune: as in ngsld_prune; NULL otherwise */
} ngsld_analysis;

typedef struct ngsld_analyze_stats {
  uint32_t struct_size;         /* sizeof(ngsld_analyze_stats) */
  uint32_t n_analyses;          /* the length of the list */
  uint64_t pairs;               /* planned pairs */
  uint64_t pairs_run;           /* pairs handed to the pair kernels in this call: == pairs says they ran once (0 after a refusal
                                   made before they start, and when no listed analysis has anything to read) */
  uint64_t chunks;              /* chunks of rows the pairs ran in */
  double pairs_ms, kernels_ms, total_ms;  /* pair kernels + replay (shared), the analyses' kernels over the chunks, the whole call */
} ngsld_analyze_stats;

/* After ngsld_plan.  Before any device work: NGSLD_ERR_INVALID for n == 0, an unknown kind, a kind listed twice (a context keeps
 * one result per kind) or a wrong struct_size, and every entry's parameters are checked with its single call's code and message.
 * The stores of the listed kinds are emptied on entry; on any failure -- a refusal that a single call would make, with its
 * message, at whatever chunk it arrives -- every listed store is left empty and the context stays usable; kinds not listed keep
 * what they held.  The chunk is that of the single calls (2^24 records): with pruning listed a row longer than the chunk is
 * refused as by ngsld_prune, without it the buffer fits the longest row.  All listed analyses hold their device state at once.
 * stats may be NULL. */
int ngsld_analyze(ngsld_ctx *ctx, ngsld_analysis *list, uint32_t n, ngsld_analyze_stats *stats);

/* ---- LD decay map on the device (DECAY_MAP.md) ------------------------------------------------------------------------------
 * ngsld_decay's bins kept per group instead of pooled: a group is a chromosome (window == 0) or the window of `window` bp of a
 * chromosome that holds the midpoint of the pair, w = (p1 + p2) / (2 * window) in integer division.  Chromosomes are the runs of
 * sites between the non-finite gaps of pos_dist, as for ngsld_grid; a pair across chromosomes is never counted.  For each group
 * the bins are what ngsld_decay gives for a TSV that holds only that group's rows: the same filters, right-closed bins and exact
 * means (DECAY.md rules 1-6).  The fit is not run here: ngsld_host_decay_fit takes a group's bins.  It is a call of its own, not
 * a kind of ngsld_analyze.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_decay_map_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (default) */
  double bin_size;            /* B > 1, as ngsld_decay_params.bin_size */
  double max_kb_dist;         /* a row needs dist < max_kb_dist * 1000 (INFINITY: no limit) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  uint64_t window;            /* 0: a group per chromosome; W in [1, 2^31): a group per window of W bp (the labels give the positions) */
} ngsld_decay_map_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_decay_map_stats) */
  uint32_t lds;               /* 1: a workgroup kept its home group's bins in LDS, 0: every add went to global memory */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows in some bin of some group */
  uint64_t groups;            /* groups with a non-empty bin (what ngsld_decay_map_groups returns) */
  uint64_t bins;              /* non-empty bins over all groups (what ngsld_decay_map_bins returns) */
  uint64_t group_slots;       /* groups sized from the plan: chromosomes, or per chromosome the windows from its first to its last site */
  uint64_t bin_slots;         /* bins per group sized from the plan */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  double pairs_ms, kernel_ms, total_ms;  /* pair kernels + replay, the map kernel (kernel time), the whole call */
} ngsld_decay_map_stats;

/* The map after ngsld_plan; the context keeps it until the next ngsld_decay_map, ngsld_plan or ngsld_set_*.  labels = n_sites C
 * strings as ngsld_grid takes them, CHR ":" pos up to the first TAB.  window == 0: labels may be NULL (the groups are then named
 * by their 1-based ordinal), otherwise a group is named by its first site's label up to the first ':'.  window > 0: NULL or
 * "(null)" labels are NGSLD_ERR_INVALID; a position that is not plain decimal digits or is >= 2^62, and positions that decrease
 * inside a chromosome, are NGSLD_ERR_UNSUPPORTED.  Also NGSLD_ERR_UNSUPPORTED: a value of 2^38 micro-units or more (naming the
 * pair), sums that could pass 2^63 micro-units (max |value| x planned pairs), a finite max_kb_dist with non-integer position gaps,
 * or accumulators of more than 1 GiB ((1 + fields) x group slots x bin slots x 8 B: a larger window or bin_size is needed;
 * this stands in for ngsld_decay's limit of 2^22 bins).  Every refusal leaves the store empty and the context usable.  stats may be NULL. */
int ngsld_decay_map(ngsld_ctx *ctx, const ngsld_decay_map_params *params, const char *const *labels, ngsld_decay_map_stats *stats);
/* The chromosomes of the last ngsld_decay_map in file order: up to cap names into name[] (the context's strings: valid while the
 * result is); *n_chr (may be NULL) receives their number. */
int ngsld_decay_map_chromosomes(ngsld_ctx *ctx, uint64_t cap, const char **name, uint64_t *n_chr);
/* The last ngsld_decay_map's groups with a non-empty bin, by chromosome (file order), then window: up to cap of them into chr[]
 * (index into ngsld_decay_map_chromosomes' names), win_start[] (w * window; 0 per chromosome), first_bin[] and n_bins[] (the
 * group's bins are entries first_bin .. first_bin + n_bins - 1 of ngsld_decay_map_bins).  Any pointer may be NULL; *n_groups (may
 * be NULL) receives the number of groups. */
int ngsld_decay_map_groups(ngsld_ctx *ctx, uint64_t cap, uint32_t *chr, uint64_t *win_start, uint64_t *first_bin, uint64_t *n_bins,
                           uint64_t *n_groups);
/* The non-empty bins of all groups back to back, each group's in increasing distance, as ngsld_decay_bins gives them: dist[],
 * count[], mean[i * n_fields + f].  Any pointer may be NULL; *n_bins (may be NULL) receives the number of bins. */
int ngsld_decay_map_bins(ngsld_ctx *ctx, uint64_t cap, double *dist, uint64_t *count, double *mean, uint64_t *n_bins);

/* ---- LD across chromosomes on the device (CROSS.md) -------------------------------------------------------------------------
 * The whole-genome form of ngsld_grid: the rows of the TSV this context's plan would print, those across two chromosomes (dist
 * not finite) included, binned by the chromosome and window of both sites -- without the TSV.  Chromosomes are the runs of sites
 * between the non-finite gaps of pos_dist; a site's bin is p / bin_size in integer division (bin_size == 0: one bin per
 * chromosome), the bins numbered consecutively over the chromosomes.  A row (s1 < s2) counts iff both printed maf >= min_maf,
 * every chosen field is finite, and either the sites lie on two chromosomes or within != 0 and dist (as printed) >=
 * min_kb_dist * 1000.  It belongs to the cell (chr, bin of s1; chr, bin of s2).  Per cell: what ngsld_grid keeps per cell, as
 * exact integers in micro-units, and the mean as the double nearest to the exact mean.  It is a call of its own, not a kind of
 * ngsld_analyze.  Both structs start with struct_size, as the pruning structs do. */
typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_cross_ld_params) */
  uint32_t fields;            /* mask as ngsld_decay_params.fields: 1 r2_ExpG, 2 D, 4 D', 8 r2 (default) */
  uint64_t bin_size;          /* B: 0 = one bin per chromosome; else the window in bp, 1 <= B < 2^31 (the labels give the positions) */
  double min_maf;             /* a row needs maf1 >= min_maf and maf2 >= min_maf, as printed (default 0) */
  double linked_min;          /* a row is linked in a field iff its value >= linked_min (default 0.5) */
  double min_kb_dist;         /* a row inside one chromosome needs dist >= min_kb_dist * 1000 (default 0) */
  int32_t abs_value;          /* != 0 (default): |value|; 0: the signed value */
  int32_t within;             /* != 0 (default): rows inside one chromosome count too; 0: only rows across two chromosomes */
} ngsld_cross_ld_params;

typedef struct {
  uint32_t struct_size;       /* sizeof(ngsld_cross_ld_stats) */
  uint32_t lds;               /* 0: every add that leaves a wavefront goes to global memory (there is no LDS form) */
  uint64_t pairs;             /* pairs computed */
  uint64_t pairs_counted;     /* rows that count: the sum of n over the cells */
  uint64_t pairs_cross;       /* ... of them across two chromosomes */
  uint64_t cells;             /* cells with rows (what ngsld_cross_ld_cells returns) */
  uint64_t bins;              /* bins between the first and the last site of every chromosome; the accumulators hold bins * (bins + 1) / 2 cells */
  uint64_t chunks;            /* chunks of rows the pairs ran in */
  uint64_t span_items;        /* M: consecutive work items a wavefront carries its current cell over */
  double pairs_ms, cross_ms, total_ms;  /* pair kernels + replay, the cross kernel (kernel time), the whole call */
} ngsld_cross_ld_stats;

/* The cells after ngsld_plan; the context keeps them until the next ngsld_cross_ld, ngsld_plan or ngsld_set_*.  labels = n_sites
 * C strings as ngsld_grid takes them, CHR ":" pos up to the first TAB.  bin_size == 0: labels may be NULL (the chromosomes are
 * then named by their 1-based ordinal); bin_size > 0: NULL or "(null)" labels are NGSLD_ERR_INVALID.  NGSLD_ERR_INVALID too
 * where pos_dist holds no finite gap at all.  NGSLD_ERR_UNSUPPORTED as for ngsld_grid: labels that disagree with pos_dist, a
 * chromosome name that begins two runs, positions that are not plain decimal digits or that decrease, a value of 2^38
 * micro-units or more (naming the pair), a cell whose sum could pass 2^63 micro-units, min_kb_dist > 0 with non-integer position
 * gaps, or accumulators of more than 2 GiB ((1 + 3 x fields) x bins x (bins + 1) / 2 x 8 B: a larger bin_size is needed).  Every
 * refusal leaves the store empty and the context usable.  stats may be NULL. */
int ngsld_cross_ld(ngsld_ctx *ctx, const ngsld_cross_ld_params *params, const char *const *labels, ngsld_cross_ld_stats *stats);
/* The last ngsld_cross_ld's cells with rows, ordered by the consecutive bin of the first site, then of the second: up to cap of
 * them into chr1[] and chr2[] (indices into ngsld_cross_ld_chromosomes' names), bin1[] and bin2[] (the bins b = p / bin_size; 0
 * with bin_size 0) and n[] (rows).  Any pointer may be NULL; *n_cells (may be NULL) receives the number of cells. */
int ngsld_cross_ld_cells(ngsld_ctx *ctx, uint64_t cap, uint32_t *chr1, uint64_t *bin1, uint32_t *chr2, uint64_t *bin2, uint64_t *n,
                         uint64_t *n_cells);
/* The chromosomes of the last ngsld_cross_ld in file order: up to cap names into name[] (the context's strings: valid while the
 * result is); *n_chr (may be NULL) receives their number. */
int ngsld_cross_ld_chromosomes(ngsld_ctx *ctx, uint64_t cap, const char **name, uint64_t *n_chr);
/* The last ngsld_cross_ld's arrays of one chosen statistic (field = TSV column 4..7), in the order of ngsld_cross_ld_cells, up
 * to cap entries each, any pointer may be NULL: sum_micro[] and max_micro[] in micro-units, linked[], mean[]. */
int ngsld_cross_ld_get(ngsld_ctx *ctx, int field, uint64_t cap, int64_t *sum_micro, int64_t *max_micro, uint64_t *linked, double *mean);

#ifdef __cplusplus
}
#endif
#endif
