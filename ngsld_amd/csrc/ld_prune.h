// ld_prune.h -- the edge weight of LD pruning, shared by the device's edge extraction (prune.hip) and the host
// (prune_host.cpp: ngsld_host_prune_label, ngsld_host_prune_graph), and the printed value in micro-units that LD decay's bins
// sum (decay.hip).  Not part of the ld_device.h umbrella: the pair kernels
// never see it.
//
// A pruner that reads the TSV sees every value "as printed": the double nearest to its "%f" text.  Both glibc and the
// device formatter (ld_text.hip, put_fixed) round the EXACT binary value half-to-even at the sixth decimal, so for |x| < 2^33
// that text is m / 10^6 with m = round_half_even(x * 10^6) computed exactly (below 2^53, in 128-bit integers as put_fixed does),
// and (double)m / 1e6 -- one correctly rounded IEEE division of exact operands -- is what strtod makes of it.  From 2^33 on the
// ulp of x exceeds 10^-6 and the text reads back as x itself.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define NGSLD_PRUNE_HD __host__ __device__
#else
#define NGSLD_PRUNE_HD
#endif

namespace ngsld {

// round_half_even(|x| * 10^6) computed exactly: the digits of "%f" of |x| without the point, for a finite |x| < 2^33
NGSLD_PRUNE_HD inline uint64_t printed_micro_abs(double x) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  const int ebits = (int)((bits >> 52) & 0x7ff);
  uint64_t m = bits & 0xfffffffffffffull;
  int ex;  // |x| = m * 2^ex, ex <= -20 here
  if (ebits == 0) {
    ex = -1074;
  } else {
    m |= 1ull << 52;
    ex = ebits - 1075;
  }
  const int k = -ex;
  const unsigned __int128 M = (unsigned __int128)m * 1000000u;  // < 2^73
  uint64_t q = 0;
  if (k < 127) {  // (k >= 127: M is below half a unit, q = 0)
    const unsigned __int128 quo = M >> k;
    q = (uint64_t)quo;
    const unsigned __int128 rem = M - (quo << k), half = (unsigned __int128)1 << (k - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
  }
  return q;
}

// the double a reader gets back from "%f" of a finite x
NGSLD_PRUNE_HD inline double prune_printed(double x) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  if ((int)((bits >> 52) & 0x7ff) >= 1023 + 33) return x;  // |x| >= 2^33 (and inf / NaN, which the callers have sorted out)
  const double p = (double)printed_micro_abs(x) / 1e6;
  return (bits >> 63) ? -p : p;
}

// LD decay's exact accumulator (decay.hip): q = round_half_even(x * 10^6), the printed value in integer micro-units, for a
// finite x.  false when |q| would reach 2^38 (|x| >~ 2.7 * 10^5): never wrapped.
NGSLD_PRUNE_HD inline bool printed_micro(double x, int64_t *q) {
  uint64_t bits;
  __builtin_memcpy(&bits, &x, sizeof(bits));
  if ((int)((bits >> 52) & 0x7ff) >= 1023 + 19) return false;  // |x| >= 2^19: |q| > 5 * 10^11 > 2^38
  const uint64_t a = printed_micro_abs(x);
  if (a >= (1ull << 38)) return false;
  *q = (bits >> 63) ? -(int64_t)a : (int64_t)a;
  return true;
}

// 10^prec as a double (exact for the supported 0 <= prec <= 15)
NGSLD_PRUNE_HD inline double prune_scale(int prec) {
  double s = 1.0;
  for (int i = 0; i < prec; ++i) s *= 10.0;
  return s;
}

enum { kPruneEdge = 0, kPruneSkip = 1, kPruneTooLarge = 2 };

// The weight filter of one pair whose distance and subset tests have passed: w = the printed value, |w| for type 'a', skipped
// below min_weight, 1 for type 'n', label = trunc(w * 10^prec).  kPruneSkip for NaN / inf or w < min_weight, kPruneTooLarge
// when |w * 10^prec| >= 2^62 (never wrapped).
NGSLD_PRUNE_HD inline int prune_label(double x, double min_weight, char type, double scale, int64_t *label) {
  if (!(x - x == 0.0)) return kPruneSkip;  // NaN or +-inf
  double w = prune_printed(x);
  if (type == 'a') w = w < 0 ? -w : w;
  if (w < min_weight) return kPruneSkip;
  if (type == 'n') w = 1.0;
  const double t = w * scale;
  if (!(t < 4611686018427387904.0 && t > -4611686018427387904.0)) return kPruneTooLarge;
  *label = (int64_t)t;
  return kPruneEdge;
}

}  // namespace ngsld
