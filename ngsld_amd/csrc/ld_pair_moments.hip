// ld_pair_moments.hip -- pair_ld_moments_kernel: the two sums of a pair that ARE shared across pairs, as a banded matrix product
// on the f64 matrix pipe, in front of pair_ld_run_kernel (ld_kernel_run.h).
//
// Under the kernels' labels (Relabel: a site's labels depend on its own frequency only) the expected genotype e = a1 + 2 a2 and
// the posterior dosage d = num / den (dose_weights / dose_terms, ld_common.h) are per-SITE vectors over the individuals, so a
// launch's Pearson cross moments sum e1 e2 and first-step sums S12 = sum d1 d2 are the band of X X^T, X = sites x individuals.
// One workgroup (eight wavefronts) takes a tile of 128 rows x 64 candidates, a wavefront 32 x 32 of it as 2 x 2 results of
// v_mfma_f64_16x16x4_f64 per sum.  K runs over the padded individuals in chunks of 16: the loader threads bring the chunk's
// planes into registers a chunk ahead, form e and d and put them into LDS [k][site]; the wavefronts read their operands from
// there (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[i = (lane >> 4) + 4 reg][j = lane & 15]).
//
// SUMMATION ORDER, one for every output element whatever tile or launch holds it: a chunk's four MFMA steps accumulate from
// zero (16 individuals, in order), and the chunks' partial sums are added in order to the element's total.  A term passes at
// most 16 + np / 16 roundings (48 at np = 512, 56 at 640) instead of the np / 4 MFMA steps x 4 of one long chain: that is the
// number write_pair's text margin for r2_ExpG is sized with (ld_em.h).  No split of K across wavefronts, no atomics.
//
// A site that is not dose_ok may give a non-finite d: it reaches the results of that site's own row / column only, pairs whose
// first step the run kernel does not take.  Padding individuals hold zero planes: e = 0, and d is set to 0.
// Results go to out[first_record + j - rec0] = {sum e1 e2, sum d1 d2} for the KEPT pairs of the plan's items; tiles beyond the
// band and 16 x 16 results without a candidate are skipped.
#include <algorithm>

#include "ld_dispatch.h"

namespace ngsld {

namespace {
constexpr uint32_t kTR = 128, kTC = 64, kKc = 16;
constexpr uint32_t kSites = kTR + kTC;  // 192 sites' values per chunk
constexpr uint32_t kLd = kSites + 16;   // row stride in doubles: k and k + 1 sit 128 B (mod 256) apart -- no bank conflict
typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
}  // namespace

template <bool DOSE>
__global__ __launch_bounds__(512) void pair_ld_moments_kernel(MomentArgs A) {
  __shared__ double sE[kKc * kLd];
  __shared__ double sD[DOSE ? kKc * kLd : 1];
  __shared__ uint64_t s_ioff[kTR];
  __shared__ uint32_t s_end[kTR];
  __shared__ uint32_t s_cmax;
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
  const uint32_t rb = A.row0 + blockIdx.y * kTR;                       // first row of the tile (< row1 by the grid)
  const uint64_t c0 = (uint64_t)rb + 1u + (uint64_t)blockIdx.x * kTC;  // first candidate of the tile
  if (t == 0) s_cmax = 0;
  __syncthreads();
  if (t < kTR) {
    const uint32_t row = rb + t;
    const bool in = row < A.row1;
    const uint32_t e = in ? A.row_end[row] : 0u;
    s_end[t] = e;
    s_ioff[t] = in ? A.item_off[row] : 0ull;
    atomicMax(&s_cmax, e);
  }
  __syncthreads();
  const uint32_t cmax = s_cmax;
  if (c0 >= cmax) return;  // (workgroup-uniform) the tile lies beyond the band

  // loader threads: site sl of the tile's 192 (rows first), individuals half * 8 .. + 8 of each chunk
  const bool loader = t < 2 * kSites;
  const uint32_t sl = t < kSites ? t : (loader ? t - kSites : 0u), half = t < kSites ? 0u : 1u;
  uint64_t site = sl < kTR ? (uint64_t)rb + sl : c0 + (sl - kTR);
  if (site >= A.n_sites) site = A.n_sites - 1;  // (beyond the matrix: a copy of its last site, never written out)
  const double m = A.maf[site];
  const bool flip = m > 0.5;
  const DoseWeights u = dose_weights(flip ? 1.0 - m : m);
  const double *pl = A.planes + site * A.site_stride + half * 8u;
  const double *p0 = pl + (flip ? 2u * A.np : 0u), *p1 = pl + A.np, *p2 = pl + (flip ? 0u : 2u * A.np);
  v2d q0[4], q1[4], q2[4];
  auto fetch = [&](uint32_t kc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      q0[i] = reinterpret_cast<const v2d *>(p0 + kc * kKc)[i];
      q1[i] = reinterpret_cast<const v2d *>(p1 + kc * kKc)[i];
      q2[i] = reinterpret_cast<const v2d *>(p2 + kc * kKc)[i];
    }
  };
  auto stage = [&](uint32_t kc) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double a0 = q0[i >> 1][i & 1], a1 = q1[i >> 1][i & 1], a2 = q2[i >> 1][i & 1];
      const uint32_t k = half * 8u + (uint32_t)i;
      sE[k * kLd + sl] = fma(2.0, a2, a1);
      if (DOSE) {
        double den, num;
        dose_terms(u, a0, a1, a2, den, num);
        sD[k * kLd + sl] = kc * kKc + k < A.n_ind ? num / den : 0.0;
      }
    }
  };

  // this wavefront's 32 x 32 results: rows wr * 32, candidates wc * 32 of the tile, 2 x 2 MFMA results of 16 x 16
  const uint32_t wr = wave & 3u, wc = wave >> 2;
  bool live[2][2];
#pragma unroll
  for (int ri = 0; ri < 2; ++ri)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) {
      const uint64_t r_lo = (uint64_t)rb + wr * 32u + ri * 16u, c_lo = c0 + wc * 32u + cj * 16u;
      live[ri][cj] = r_lo < A.row1 && c_lo + 15u > r_lo && c_lo < cmax;  // (wavefront-uniform)
    }
  v4d totE[2][2], totD[2][2];
#pragma unroll
  for (int ri = 0; ri < 2; ++ri)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) totE[ri][cj] = totD[ri][cj] = v4d{0.0, 0.0, 0.0, 0.0};
  const uint32_t oa = (lane >> 4) * kLd + wr * 32u + (lane & 15u);        // A operand: [k][row site]
  const uint32_t ob = (lane >> 4) * kLd + kTR + wc * 32u + (lane & 15u);  // B operand: [k][candidate site]

  const uint32_t nk = A.np / kKc;
  if (loader) fetch(0);
  for (uint32_t kc = 0; kc < nk; ++kc) {
    lds_barrier();  // the last chunk's operands are read (LDS only: the planes fetched below fly through the MFMA steps)
    if (loader) {
      stage(kc);
      if (kc + 1 < nk) fetch(kc + 1);
    }
    lds_barrier();
    v4d inE[2][2], inD[2][2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      double ae[2], be[2], ad[2], bd[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        ae[x] = sE[ks * 4 * kLd + oa + x * 16];
        be[x] = sE[ks * 4 * kLd + ob + x * 16];
        if (DOSE) {
          ad[x] = sD[ks * 4 * kLd + oa + x * 16];
          bd[x] = sD[ks * 4 * kLd + ob + x * 16];
        }
      }
#pragma unroll
      for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int cj = 0; cj < 2; ++cj) {
          if (!live[ri][cj]) continue;
          const v4d z = {0.0, 0.0, 0.0, 0.0};
          inE[ri][cj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ae[ri], be[cj], ks == 0 ? z : inE[ri][cj], 0, 0, 0);
          if (DOSE) inD[ri][cj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ri], bd[cj], ks == 0 ? z : inD[ri][cj], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
      for (int cj = 0; cj < 2; ++cj) {
        if (!live[ri][cj]) continue;
        totE[ri][cj] += inE[ri][cj];
        if (DOSE) totD[ri][cj] += inD[ri][cj];
      }
  }

  // results -> the kept pairs' slots, through the plan's items (64 candidates each from s1 + 1 on)
#pragma unroll
  for (int ri = 0; ri < 2; ++ri)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) {
      if (!live[ri][cj]) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t lr = wr * 32u + ri * 16u + (lane >> 4) + 4u * r;
        const uint64_t s1 = (uint64_t)rb + lr, s2 = c0 + wc * 32u + cj * 16u + (lane & 15u);
        if (s1 >= A.row1 || s2 <= s1 || s2 >= s_end[lr]) continue;
        const uint64_t off = s2 - s1 - 1;
        const Item *it = A.items_all + s_ioff[lr] + (off >> 6);
        const uint64_t mask = it->mask, bit = 1ull << (off & 63u);
        if (!(mask & bit)) continue;  // the filters dropped the pair
        const uint64_t idx = it->first_record + (uint64_t)__popcll(mask & (bit - 1)) - A.rec0;
        reinterpret_cast<v2d *>(A.out)[idx] = v2d{totE[ri][cj][r], DOSE ? totD[ri][cj][r] : 0.0};
      }
    }
}

hipError_t launch_pair_moments(const MomentArgs &a, const uint32_t *h_row_end, hipStream_t stream) {
  if (a.row1 <= a.row0) return hipSuccess;
  uint64_t most = 0;  // candidate tiles of the widest row block
  for (uint32_t rb = a.row0; rb < a.row1; rb += kTR) {
    uint32_t end = 0;
    for (uint32_t r = rb; r < a.row1 && r < rb + kTR; ++r) end = std::max(end, h_row_end[r]);
    if (end > rb + 1) most = std::max<uint64_t>(most, ((uint64_t)end - rb - 1 + kTC - 1) / kTC);
  }
  if (most == 0) return hipSuccess;
  if (most > (1ull << 22)) return hipErrorInvalidValue;  // (rows of more than 2^28 candidates)
  // at most 2^22 workgroups a grid (gridDim x blockDim stays below 2^32, see launch_pair_kernel) and 65,535 row blocks
  const uint64_t blocks_y = std::min<uint64_t>(65535, std::max<uint64_t>(1, (1ull << 22) / most));
  for (uint64_t r0 = a.row0; r0 < a.row1; r0 += blocks_y * kTR) {
    MomentArgs b = a;
    b.row0 = (uint32_t)r0;  // (row1 stays: the last grid's last tile ends there)
    const uint64_t by = std::min<uint64_t>(blocks_y, ((uint64_t)a.row1 - r0 + kTR - 1) / kTR);
    const dim3 grid((unsigned)most, (unsigned)by), block(512);
    if (a.dose)
      hipLaunchKernelGGL((pair_ld_moments_kernel<true>), grid, block, 0, stream, b);
    else
      hipLaunchKernelGGL((pair_ld_moments_kernel<false>), grid, block, 0, stream, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ngsld
