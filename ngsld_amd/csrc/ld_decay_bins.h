// ld_decay_bins.h -- the bins of LD decay (DECAY.md rules 4 and 5), shared by ngsld_decay (decay.hip) and ngsld_decay_map
// (decay_map.hip): dist as the TSV prints it, the right-closed bin of a dist, a bin's lower break as R labels it.
#pragma once

#include <cstdio>
#include <cstdlib>

// dist as the TSV prints it ("%.0f", read back): the exact binary value rounded half-to-even (exact for integer gaps)
__host__ __device__ inline double printed_dist(double x) { return __builtin_rint(x); }

// the right-closed bin (k*B, (k+1)*B] of d, with the breaks computed as R's seq(0, ., B) does (k * B); -1 for d <= 0
__host__ __device__ inline long long bin_of(double d, double B) {
  if (!(d > 0.0)) return -1;
  long long k = (long long)__builtin_ceil(d / B) - 1;
  if (k < 0) k = 0;
  while (k > 0 && !(d > (double)k * B)) --k;
  while (d > (double)(k + 1) * B) ++k;
  return k;
}

// R's as.character of a break (15 significant digits) read back
inline double break_value(uint64_t k, double B) {
  char buf[64];
  std::snprintf(buf, sizeof(buf), "%.15g", (double)k * B);
  return std::strtod(buf, nullptr);
}
