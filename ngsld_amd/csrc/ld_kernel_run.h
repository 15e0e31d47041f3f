// ld_kernel_run.h -- pair_ld_run_kernel: one wavefront per pair, the row vector shared in LDS, runs of items (the headline's
// kernel at eight slots; the pipeline is described in ld_run_pipeline.h); instantiated in ld_pair_w1.hip.
#pragma once

#include "ld_run_pipeline.h"

namespace ngsld {

// SKIP (a launch over a matrix with degenerate sites, PairArgs::skip_degenerate): a pair with such a site -- marked in
// sc4[.][3] by site_skip_kernel, ld_prep.hip -- is staged for its Pearson moment only; its frequencies are left NaN, which
// write_pair flags, and the exact-order replay is the pair's one evaluation (it was going to start the pair over anyway).  A
// variant of its own so that launches over SNP-called matrices keep the instruction stream they had.
//
// FIRST STEP FROM DOSAGES (kFirst: every individual counts, two to eight slots; on where PairArgs::dose_sum is set).  Every
// pair starts at linkage equilibrium, f = (1-m1, m1) x (1-m2, m2), where the two-locus genotype weights factorise: an
// individual's posterior over the nine genotype pairs is alpha_g beta_h, with alpha_g = u_g a_g / (u . a),
// u = ((1-m)^2, 2m(1-m), m^2), a matter of site 1 alone, and a double heterozygote is cis or trans with probability 1/2.
// With the posterior dosage d = alpha_1 + 2 alpha_2 the expected count of haplotype (1,1) is d1 d2 / 2, so iteration 0 is
//   f3' = S12 / (4n),  f2' = S1 / (2n) - f3',  f1' = S2 / (2n) - f3',  f0' = 1 - ((f1' + f2') + f3'),   S12 = sum d1 d2, S = sum d.
// S is a per-site scalar, summed once per matrix by site_dose_kernel (ld_prep.hip), which also says whether the site may
// take part (dose_ok).  S12 -- and the Pearson cross moment sum e1 e2, e = a1 + 2 a2 -- are sums over the individuals of
// products of two PER-SITE vectors (each site's labels depend on its own frequency only: Relabel): over a launch they are the
// band of X X^T, the one contraction of the workload that IS shared across pairs.  pair_ld_moments_kernel
// (ld_pair_moments.hip) forms them on the f64 matrix pipe in front of every launch, 16 bytes a pair (PairArgs::moments,
// mom_on; every individual counting, any slot count); they come in with the candidate's site copy (lane 2's 16 bytes beside
// its scalars) and are read behind stage_pair: no dosage, no reciprocal tree, no wavefront reduction in front of the EM.
// The centring fma(-n mean1, mean2, sum e1 e2), have0 / dose_ok / skip and em_pair's FIRST bookkeeping are what they were.
//
// A pair with a site that is not dose_ok by itself keeps the in-kernel moment: its records do not depend on the pass.
// PairArgs::moments == nullptr (NGSLD_TEST_PAIR_MOMENTS=0: tests, A/B) is the kernel as it was before that pass, the same
// records bit for bit (but for a row whose lane product of dens underflows, which site_dose_kernel now keeps out of the
// step as it kept such a candidate: ld_prep.hip): the row's dosages are formed once per run, from its planes in LDS, and stay in LDS (4 KB at eight
// slots); the candidate's are formed from its planes right before stage_pair turns them into P -- den and num per slot, ONE
// reciprocal per lane for all its slots (RcpTree), one FMA per slot into S12, a wave_sum1_bcast of its own (the lane's share
// of S12 is complete before P exists, that of the moment only after it; carried across stage_pair the cross-compile spills) --
// and the moment is read off P and reduced behind stage_pair.  (Both paths live in ONE kernel, chosen by a wavefront-uniform
// argument like first_on: the row's 4 KB of LDS stay allocated.  HISTORY.md has what else was tried for the in-kernel form.)
// The candidate's S comes through the scalar cache, behind stage_pair (see there).  Everything is formed under the
// kernel's labels (Relabel), so no sum needs turning round.  A pair with a site that is not dose_ok, or whose given
// frequencies fail em_pair's sanity test (a product of dens that underflowed: NaN), starts at iteration 0 as before; the
// choice is wavefront-uniform.  Nine and ten slots spill already: they keep the per-individual first step (and take the
// moment from the pass).  The SKIP variant takes the step like
// the plain one: which of the two a launch gets depends on the context (marks on or off, a replay that can take the marked
// pairs), and the pairs both compute must come out the same bits in both (tests/test_gpu_replay_lkl.py,
// tests/test_gpu_multi_native.py).
template <int SLOTS, bool MASKED, bool SKIP = false>
__global__ __launch_bounds__(256, 2) void pair_ld_run_kernel(PairArgs A) {
  constexpr int kSiteBytes = SLOTS * 64 * 3 * 8;
  constexpr int kBuf = kSiteBytes + 48;  // a site's planes, its four scalars, the pair's two sums (mom_on)
  constexpr uint32_t kNp = SLOTS * 64;
  // (ten slots: five site buffers of 15 KB leave 5 KB for rings and list under the 80 KB that let two workgroups share a CU)
  constexpr uint32_t kRing = SLOTS <= 9 ? 32 : 8;
  constexpr int kRingOff = kSiteBytes + 4 * kBuf;
  constexpr int kListOff = kRingOff + 4 * (int)(kRing * sizeof(RunResult));
  constexpr bool kFirst = !MASKED && SLOTS >= 2 && SLOTS <= 8;
  constexpr int kDoseOff = kListOff + (int)sizeof(RunList);  // (kFirst) the row's dosages, [kNp] doubles
  static_assert(sizeof(RunList) % 8 == 0, "run kernel: doubles behind the run list");
  __shared__ __attribute__((aligned(16))) char smem[kDoseOff + (kFirst ? (int)kNp * 8 : 0)];
  static_assert(sizeof(smem) <= 81920, "run kernel: two workgroups per CU need <= 80 KB of LDS each");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // (An XCD-aware order -- each XCD taking 64 consecutive runs of every 512 -- was measured and dropped: neighbouring
  // rows drift apart by more pairs than the 4 MB L2 bridges, L2-miss traffic rose 35 % and the kernel lost 0.7 %.)
  const Run run = A.runs[blockIdx.x];
  const Item *g_items = A.items_all + run.first_item;
  const uint32_t s1 = g_items[0].s1;
  const double m1 = A.sc4[4 * (uint64_t)s1], mean1 = A.sc4[4 * (uint64_t)s1 + 1];
  const double rsx1 = uniform(A.sc4[4 * (uint64_t)s1 + 2]);  // (only the flushes read it: in SGPRs, or their spill lanes, it holds no VGPR through the pairs)
  const bool skip1 = SKIP && A.sc4[4 * (uint64_t)s1 + 3] != 0.0;
  char *lds_a = smem;
  char *lds_b = smem + kSiteBytes + wave * kBuf;
  RunResult *ring = reinterpret_cast<RunResult *>(smem + kRingOff) + wave * kRing;
  RunList *L = reinterpret_cast<RunList *>(smem + kListOff);

  dma_site_to_lds<SLOTS>(A.planes + (uint64_t)s1 * A.site_stride, lds_a, lane, wave, 4);  // a quarter per wavefront
  build_run_list(L, g_items, run.n_items);  // its last barrier: row vector and list in place
  const uint32_t n_kept = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->base[run.n_items]);
  const uint32_t s2_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->items[0].s2_begin);
  const uint64_t rec_base = g_items[0].first_record - A.out_base;
  const bool first_on = kFirst && A.dose_sum != nullptr;  // (a kernel argument: wavefront-uniform)
  const bool mom_on = !MASKED && A.moments != nullptr;    // (likewise) both sums come from pair_ld_moments_kernel
  const bool has_ok = kFirst && A.dose_ok != nullptr;      // (likewise) the sites' dosage sums are there, if only for their signs
  double S1 = -1.0;
  if (has_ok) {
    S1 = uniform(A.dose_ok[s1]);
    S1 = uniform(S1 < 0.0 ? S1 : 0.5 * S1);  // half the sum is what the pairs use (in SGPRs)
  }
  if (first_on && !mom_on) {  // the row's dosages, for the sums formed per pair
    const bool flip1 = m1 > 0.5;  // (Relabel: the row's labels are the same for all its pairs)
    const DoseWeights u = dose_weights(flip1 ? 1.0 - m1 : m1);
    const double *pa = reinterpret_cast<const double *>(lds_a);
    double *d1 = reinterpret_cast<double *>(smem + kDoseOff);
    for (uint32_t i = threadIdx.x; i < kNp; i += 256) {
      double den, num;
      dose_terms(u, pa[(flip1 ? 2 * kNp : 0u) + i], pa[kNp + i], pa[(flip1 ? 0u : 2 * kNp) + i], den, num);
      d1[i] = i < A.n_ind ? num / den : 0.0;  // (a row that is not dose_ok: whatever this gives is never used)
    }
    __syncthreads();
  }

  // one computed pair of the run: site and record index
  struct Cand {
    uint32_t s2;
    uint64_t rec;
    bool ok;
  };
  auto claim_next = [&]() -> Cand {  // (the maf[s2] / sub-sampling filters, ngsLD.cpp:270-282, already shaped the list)
    uint32_t j = 0;
    if (lane == 0) j = atomicAdd(&L->claim, 1u);
    j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
    if (j >= n_kept) return Cand{0u, 0ull, false};
    const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)L->cand[j]);
    return Cand{s2_base + off, rec_base + j, true};
  };
  // (mom_on: the pair's two sums travel with the site like its scalars -- lane 2's 16 bytes of the same copy, a pair ahead of
  // their use, behind no wait of their own)
  auto dma_site = [&](const Cand &c) {
    dma_site_to_lds<SLOTS>(A.planes + (uint64_t)c.s2 * A.site_stride, lds_b, lane, 0, 1);
    if (lane < (mom_on ? 3 : 2)) {
      const char *src = reinterpret_cast<const char *>(A.sc4 + 4 * (uint64_t)c.s2) + lane * 16;
      if (!MASKED && lane == 2) src = reinterpret_cast<const char *>(A.moments + 2 * c.rec);
      __builtin_amdgcn_global_load_lds((glb_void_t *)src, (lds_void_t *)(lds_b + kSiteBytes), 16, 0, 0);
    }
  };
  auto flush = [&](uint32_t n) {  // lane t derives and writes the record of ring entry t
    if ((uint32_t)lane < n) {
      const RunResult r = ring[lane];
      write_pair(A, r.rec, r.f[0], r.f[1], r.f[2], r.f[3], r.sxy, rsx1, r.rsx2, r.x, r.n_iter);
    }
  };

  Cand cur = claim_next();
  if (cur.ok) dma_site(cur);
  uint32_t held = 0;
  while (cur.ok) {
    const Cand nxt = claim_next();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's site copy (issued a pair ago) has landed
    const double *sc = reinterpret_cast<const double *>(lds_b + kSiteBytes);
    const double m2 = uniform(sc[0]), mean2 = uniform(sc[1]), rsx2 = uniform(sc[2]);
    const bool skip = SKIP && (skip1 || uniform(sc[3]) != 0.0);  // (read here: the next site's copy is about to land on sc)
    double P[SLOTS][9];
    uint32_t vbits;
    double sxy;
    const Relabel rl = relabel(m1, m2, mean1, mean2);
    double s12 = 0.0;
    const bool ok1 = has_ok && !skip && S1 >= 0.0;  // (wavefront-uniform) the row is dose_ok
    const bool dose1 = first_on && ok1;
    const bool bad1 = has_ok && S1 == -1.0;  // not dose_ok by itself (-2: by site_skip_kernel's mark alone, ld_prep.hip)
    const bool want2 = (dose1 || (mom_on && has_ok && !bad1));  // the candidate's sum: for the step, or to tell what it is
    if (dose1 && !mom_on) {  // this lane's share of sum d1 d2, before P takes the registers
      const DoseWeights u = dose_weights(rl.m2);
      const double *d1 = reinterpret_cast<const double *>(smem + kDoseOff) + lane;
      const double *pb = reinterpret_cast<const double *>(lds_b) + lane;
      double den[SLOTS], numd[SLOTS], rv[SLOTS];
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) {
        double num;
        dose_terms(u, pb[(rl.flip2 ? 2 * kNp : 0u) + 64 * j], pb[kNp + 64 * j], pb[(rl.flip2 ? 0u : 2 * kNp) + 64 * j], den[j], num);
        if (j == SLOTS - 1 && (uint32_t)lane + 64u * j >= A.n_ind) den[j] = 1.0;  // a padding lane: planes and d1 are 0
        numd[j] = num * d1[64 * j];
      }
      RcpTree<SLOTS>::down(den, rcp_refined(RcpTree<SLOTS>::prod(den)), rv);  // one reciprocal for the lane's slots
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) s12 = fma(numd[j], rv[j], s12);  // in slot order
      s12 = wave_sum1_bcast(s12);
    }
    stage_pair<SLOTS, MASKED, !MASKED, true>(reinterpret_cast<const double *>(lds_a), kNp, (uint32_t)lane,
                                             reinterpret_cast<const double *>(lds_b), kNp, (uint32_t)lane, (uint32_t)lane,
                                             A.n_ind, rl.mean1, rl.mean2, P, vbits, sxy, rl.flip1, rl.flip2);
    // stage_pair's own moment, in its operations and order (this call's is dead code then): the lane's share
    auto moment_of_P = [&]() -> double {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) t += fma(4.0, P[j][8], fma(2.0, P[j][5] + P[j][7], P[j][4]));
      return t;
    };
    if (!MASKED && !mom_on) sxy = moment_of_P();
    // (the same for the rare pair below, behind an empty statement per slot: left to itself the compiler forms ONE lane share
    // for both uses, in front of the branches -- 32 VALU instructions and a VGPR pair on every pair of the launch)
    auto moment_of_P_apart = [&]() -> double {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) {
        double p8 = P[j][8];
        asm volatile("" : "+v"(p8));
        t += fma(4.0, p8, fma(2.0, P[j][5] + P[j][7], P[j][4]));
      }
      return t;
    };
    if (!MASKED && mom_on) {  // {sum e1 e2, sum d1 d2}, the same in every lane: the last reads of the buffer
      sxy = sc[4];
      if (dose1) s12 = sc[5];
    }
    // all ds_reads of the buffer are consumed (P is computed): start the copy of the next site over it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (nxt.ok) dma_site(nxt);
    const uint32_t x = MASKED ? count_valid<SLOTS>(vbits) : A.n_ind;
    const double inv_x = MASKED ? 1.0 / (double)x : A.inv_n;
    // The candidate's dosage sum, through the SCALAR cache: the address is wavefront-uniform, and a vector load here would
    // come back behind the 12 KB of the next site's copy just issued (loads return in order) and have that copy -- meant to
    // fly through the whole EM loop -- waited for as well.  Assembly, because the compiler makes a vector load of it (the
    // kernel writes global memory); issued here, waited for after the Pearson moment's reduction.
    // (The empty statement pins the lane's share of the moment in front of the load: the compiler's own wait for
    // stage_pair's LDS reads, which it places at their first use, would otherwise come right behind the load.)
    double S2 = -2.0;  // (not asked for: no step, and nothing said about the site)
    if constexpr (kFirst) {
      if (!mom_on) asm volatile("" : "+v"(sxy));
      if (want2) asm volatile("s_load_dwordx2 %0, %1, 0x0" : "=s"(S2) : "s"(A.dose_ok + cur.s2) : "memory");
    }
    if (MASKED || !mom_on) sxy = wave_sum1_bcast(sxy);
    if constexpr (kFirst) {
      if (want2) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(S2)::"memory");
      // A pair with a site that by itself takes no part in the first step (not dose_ok: -1) keeps the in-kernel moment: its
      // records are the same bits whether the pass ran or not, whether the step is on or not, and -- a marked site is -2 or a
      // sum, never -1 -- whether the marks are on or not (tests/test_gpu_pair_moments.py, tests/test_gpu_first_step.py,
      // tests/test_gpu_replay_lkl.py).  Wavefront-uniform, rare.
      if (mom_on && has_ok && (bad1 || S2 == -1.0)) sxy = wave_sum1_bcast(moment_of_P_apart());
    }
    sxy = fma(-(double)A.n_ind * rl.mean1, rl.mean2, sxy);  // centred: sum e1 e2 - n mean1 mean2
    double f0, f1, f2, f3;
    uint32_t n_iter = 0;
    if (skip) {  // (wavefront-uniform)
      f0 = f1 = f2 = f3 = __builtin_nan("");
    } else if constexpr (kFirst) {
      bool have0 = false;
      double g1 = 0.0, g2 = 0.0, g3 = 0.0;
      if (dose1) {
        have0 = S2 >= 0.0;  // both sites dose_ok
        // (written so that nothing here is invariant over the run's pairs: a hoisted product is a VGPR pair held through every
        // EM loop, and the kernel has none to give)
        g3 = (0.25 * s12) * inv_x;
        g2 = S1 * inv_x - g3;
        g1 = (0.5 * S2) * inv_x - g3;
      }
      n_iter = em_pair<SLOTS, 1, true>(P, vbits, inv_x, rl.m1, rl.m2, f0, f1, f2, f3, (double (*)[1][4]) nullptr, 0, lane,
                                       A.status, nullptr, have0, g1, g2, g3);
      unrelabel(rl.flip1, rl.flip2, f0, f1, f2, f3);
    } else {
      n_iter = em_pair<SLOTS, 1>(P, vbits, inv_x, rl.m1, rl.m2, f0, f1, f2, f3, (double (*)[1][4]) nullptr, 0, lane, A.status);
      unrelabel(rl.flip1, rl.flip2, f0, f1, f2, f3);
    }
    if (lane == 0) {
      RunResult &r = ring[held];
      r.f[0] = f0; r.f[1] = f1; r.f[2] = f2; r.f[3] = f3;
      r.sxy = sxy;
      r.rsx2 = rsx2;
      r.x = x;
      r.n_iter = n_iter;
      r.rec = cur.rec;
    }
    if (++held == kRing) {
      flush(held);
      held = 0;
    }
    cur = nxt;
  }
  flush(held);
}

}  // namespace ngsld
