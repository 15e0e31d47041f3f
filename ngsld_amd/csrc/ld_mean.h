// ld_mean.h -- the one rounding of an exact mean: the means of ngsld_decay's and ngsld_decay_map's bins (decay.hip, decay_map.hip:
// append_bin_means) and of ngsld_site_ld's sites (site_ld.hip), of ngsld_clusters' clusters (cluster.hip) and of ngsld_grid's cells
// (grid.hip) are sums of integer micro-units over counts, divided once.  Host code, no HIP: tests/test_div_nearest.py
// compiles it alone.  ngsld_scan's omega (scan.hip) is a ratio of two such products, rounded once by ratio_nearest.
#pragma once

#include <stdint.h>

#include <cmath>
#include <vector>

namespace ngsld {
namespace eng {

// the double nearest to a / b (round half to even) for a >= 0, 0 < b < 2^126 and a / b < 2^54 (a mean below 2^38 / 10^6):
// long division to 55 significant bits, then the round bit and the sticky remainder
inline double div_nearest(unsigned __int128 a, unsigned __int128 b) {
  if (a == 0) return 0.0;
  unsigned __int128 q = a / b, r = a % b;
  int sh = 0;  // a / b = (q + r / b) * 2^-sh
  while (q < ((unsigned __int128)1 << 54)) {
    r <<= 1;
    q <<= 1;
    if (r >= b) {
      r -= b;
      q |= 1;
    }
    ++sh;
  }
  bool sticky = r != 0;
  const unsigned low = (unsigned)(q & 3);
  uint64_t m = (uint64_t)(q >> 2);
  sticky = sticky || (low & 1);
  if ((low & 2) && (sticky || (m & 1))) ++m;
  return std::ldexp((double)m, 2 - sh);
}

// div_nearest where a group map divides tens of thousands of means (append_bin_means): operands below 2^53 are exact doubles, and
// the IEEE quotient of two exact doubles is the double nearest to a / b, ties to even -- div_nearest's answer without its long
// division (the build keeps -ffp-contract=off and no fast-math; tests/test_div_nearest_small.py holds the two to each other)
inline double div_nearest_small(unsigned __int128 a, unsigned __int128 b) {
  if ((a >> 53) == 0 && (b >> 53) == 0) return (double)(uint64_t)a / (double)(uint64_t)b;
  return div_nearest(a, b);
}

// the double nearest to num / den (round half to even) for any num < 2^128 and 0 < den < 2^127, whatever the quotient: ngsld_scan's
// omega (scan.hip) is a ratio of two products of a sum and a count, which can lie far beyond the 2^54 of div_nearest and far
// below 1.  Where both operands are below 2^53 they are doubles, and one IEEE division is that one rounding.  Elsewhere the
// integer quotient is cut down to, or carried on by long division up to, 55 significant bits: 53 of the result, the round bit and
// one more that joins the sticky remainder.  tests/test_ratio_nearest.py holds both branches to the exact quotient.
inline double ratio_nearest(unsigned __int128 num, unsigned __int128 den) {
  if (num == 0) return 0.0;
  if (num < ((unsigned __int128)1 << 53) && den < ((unsigned __int128)1 << 53)) return (double)(uint64_t)num / (double)(uint64_t)den;
  unsigned __int128 q = num / den, r = num % den;
  int e = 0;  // num / den = (q + (what was cut off)) * 2^e
  bool sticky = false;
  while (q >= ((unsigned __int128)1 << 55)) {
    sticky = sticky || (q & 1);
    q >>= 1;
    ++e;
  }
  if (e == 0)
    while (q < ((unsigned __int128)1 << 54)) {
      r <<= 1;
      q <<= 1;
      if (r >= den) {
        r -= den;
        q |= 1;
      }
      --e;
    }
  sticky = sticky || r != 0;
  const unsigned low = (unsigned)(q & 3);
  uint64_t m = (uint64_t)(q >> 2);
  sticky = sticky || (low & 1);
  if ((low & 2) && (sticky || (m & 1))) ++m;
  return std::ldexp((double)m, e + 2);
}

// the double nearest to sum / (10^6 * rows): the mean of `rows` printed values whose micro-units add up to `sum` (ngsld_grid's
// cells, up to a million of them a field, and ngsld_site_ld's sites: field_summary, record_pass.h).  Where sum < 2^53 and rows < 2^33 both operands are doubles, and one IEEE
// division is that one rounding: the operands are exact, and a quotient of two integers below 2^53 never lies on a tie between
// two doubles (a tie has 54 significant bits, hence a numerator of at least 2^53).  Elsewhere the long division.
// tests/test_mean_nearest.py holds both branches to the exact quotient; GRID.md has what the short one saves.
inline double mean_nearest(uint64_t sum, uint64_t rows) {
  if (sum < (1ull << 53) && rows < (1ull << 33)) return (double)sum / (double)(rows * 1000000u);
  return div_nearest((unsigned __int128)sum, (unsigned __int128)rows * 1000000u);
}

// One group's non-empty bins of LD decay, appended to dist, count and mean ([bin][field]): bin k holds rows[k] rows, sum(v, k) is the
// signed sum of their micro-units of field v (an __int128 holds decay's totals over every chunk), lower(k) the bin's label.  A mean
// is the double nearest to sum / (10^6 * rows) (100 groups x 400 bins x 4 statistics: 160,000 of them).  Returns the rows appended.
template <class Sum, class Lower>
uint64_t append_bin_means(uint64_t n_bins, const uint64_t *rows, int ns, Sum sum, Lower lower, std::vector<double> &dist,
                          std::vector<uint64_t> &count, std::vector<double> &mean) {
  uint64_t appended = 0;
  for (uint64_t k = 0; k < n_bins; ++k) {
    if (rows[k] == 0) continue;
    dist.push_back(lower(k));
    count.push_back(rows[k]);
    appended += rows[k];
    for (int v = 0; v < ns; ++v) {
      const __int128 s = sum(v, k);
      const double m = div_nearest_small((unsigned __int128)(s < 0 ? -s : s), (unsigned __int128)rows[k] * 1000000u);
      mean.push_back(s < 0 ? -m : m);
    }
  }
  return appended;
}

}  // namespace eng
}  // namespace ngsld
