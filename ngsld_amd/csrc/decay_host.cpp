// decay_host.cpp -- the LD decay fit of scripts/fit_LDdecay.R on the bin means (include/ngsld_host.h: ngsld_host_decay_fit).
// The script runs optim (BFGS) from random starts and keeps a run that converged inside its bounds; this returns the global
// minimum of the same sum of squares over the same region, deterministically (DECAY.md, "The fit"):
//   * for a fixed rate (C, or t for D') both three-parameter models are linear in (h, l): the 2-variable QP over the triangle
//     0 <= l <= h <= 1 is solved exactly by active sets (the interior optimum, else the best of the three edges);
//   * the rate minimises the resulting profile: a log grid (kPerDecade points a decade over kDecades decades below the top of
//     the range, and the rate 0), then golden-section refinement of the grid's local minima.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ngsld_host.h"

namespace {

constexpr int kPerDecade = 60, kDecades = 15, kRefine = 8;

enum Model { kR2, kR2Nind, kDp };

struct Data {
  const double *d, *y;
  uint64_t n;
  Model model;
  double n_ind, rr;
};

// the script's model (ld_exp), term by term as R evaluates it
inline double model_at(const Data &D, double rate, double h, double l, double d) {
  if (D.model == kDp) return l + (h - l) * 1.0 * std::pow(1.0 - d * D.rr / 1e6, rate);
  const double C = rate * d;
  if (D.model == kR2Nind)
    return ((10 + C) / ((2 + C) * (11 + C))) * (1 + ((3 + C) * (12 + 12 * C + C * C)) / (D.n_ind * (2 + C) * (11 + C)));
  return (h - l) / (1 + C) + l;
}

double sse_at(const Data &D, double rate, double h, double l) {
  double s = 0.0;
  for (uint64_t i = 0; i < D.n; ++i) {
    const double r = model_at(D, rate, h, l, D.d[i]) - D.y[i];
    s += r * r;
  }
  return s;
}

// the h coefficient of the linear form h u + l (1 - u) at a rate
inline double basis(const Data &D, double rate, double d) {
  return D.model == kDp ? std::pow(1.0 - d * D.rr / 1e6, rate) : 1.0 / (1.0 + rate * d);
}

struct Fit {
  double rate, h, l, sse;
};

// min over 0 <= l <= h <= 1 of sum (h u_i + l (1 - u_i) - y_i)^2 for one rate
Fit solve_hl(const Data &D, double rate, std::vector<double> &u) {
  double Saa = 0, Sab = 0, Sbb = 0, Say = 0, Sby = 0, Sy = 0;
  u.resize(D.n);
  for (uint64_t i = 0; i < D.n; ++i) {
    const double a = basis(D, rate, D.d[i]), b = 1.0 - a, y = D.y[i];
    u[i] = a;
    Saa += a * a;
    Sab += a * b;
    Sbb += b * b;
    Say += a * y;
    Sby += b * y;
    Sy += y;
  }
  auto q = [&](double h, double l) {  // the quadratic part, for choosing among the candidates
    return Saa * h * h + 2 * Sab * h * l + Sbb * l * l - 2 * Say * h - 2 * Sby * l;
  };
  auto clamp01 = [](double t) { return t < 0 ? 0.0 : t > 1 ? 1.0 : t; };
  double bh = 0, bl = 0, bq = INFINITY;
  auto consider = [&](double h, double l) {
    const double v = q(h, l);
    if (v < bq) {
      bq = v;
      bh = h;
      bl = l;
    }
  };
  const double det = Saa * Sbb - Sab * Sab;
  if (det > 1e-12 * Saa * Sbb) {  // (a singular system has a line of optima: it meets the boundary, which is searched below)
    const double h = (Say * Sbb - Sby * Sab) / det, l = (Sby * Saa - Say * Sab) / det;
    if (l >= 0 && h <= 1 && h >= l) consider(h, l);
  }
  if (bq == INFINITY) {
    consider(Saa > 0 ? clamp01(Say / Saa) : 0.0, 0.0);                              // l = 0
    consider(1.0, Sbb > 0 ? clamp01((Sby - Sab) / Sbb) : 0.0);                      // h = 1
    const double t = clamp01(Sy / (double)D.n);                                     // h = l
    consider(t, t);
  }
  double s = 0.0;
  for (uint64_t i = 0; i < D.n; ++i) {
    const double r = bh * u[i] + bl * (1.0 - u[i]) - D.y[i];
    s += r * r;
  }
  return Fit{rate, bh, bl, s};
}

// the profile: the best (h, l) of a rate (the n_ind model has none to choose)
Fit profile(const Data &D, double rate, std::vector<double> &u) {
  if (D.model == kR2Nind) return Fit{rate, 0.0, 0.0, sse_at(D, rate, 0.0, 0.0)};
  return solve_hl(D, rate, u);
}

Fit minimise(const Data &D, double hi) {
  std::vector<double> u;
  const int N = kPerDecade * kDecades;
  std::vector<double> r(N + 2);
  r[0] = 0.0;
  for (int j = 0; j <= N; ++j) r[j + 1] = hi * std::pow(10.0, -(double)(N - j) / kPerDecade);
  r[N + 1] = hi;
  std::vector<Fit> g(r.size());
  for (size_t j = 0; j < r.size(); ++j) g[j] = profile(D, r[j], u);
  Fit best = g[0];
  for (const Fit &f : g)
    if (f.sse < best.sse) best = f;
  // the grid's local minima, best first
  std::vector<size_t> loc;
  for (size_t j = 0; j < g.size(); ++j)
    if ((j == 0 || g[j].sse <= g[j - 1].sse) && (j + 1 == g.size() || g[j].sse <= g[j + 1].sse)) loc.push_back(j);
  std::stable_sort(loc.begin(), loc.end(), [&](size_t a, size_t b) { return g[a].sse < g[b].sse; });
  if (loc.size() > (size_t)kRefine) loc.resize(kRefine);
  const double phi = 0.5 * (std::sqrt(5.0) - 1.0);
  for (size_t j : loc) {
    const size_t lo = j == 0 ? 0 : j - 1, up = j + 1 == g.size() ? j : j + 1;
    if (up == lo) continue;
    // log scale inside the grid, linear on the segment that starts at 0
    const bool lin = r[lo] == 0.0;
    auto to_r = [&](double x) { return lin ? x : std::exp(x); };
    double a = lin ? r[lo] : std::log(r[lo]), b = std::log(r[up]);
    if (lin) b = r[up];
    double x1 = b - phi * (b - a), x2 = a + phi * (b - a);
    Fit f1 = profile(D, to_r(x1), u), f2 = profile(D, to_r(x2), u);
    for (int it = 0; it < 200 && (b - a) > 1e-15 * std::max(std::fabs(a), std::fabs(b)) + (lin ? 1e-300 : 0.0); ++it) {
      if (f1.sse <= f2.sse) {
        b = x2;
        x2 = x1;
        f2 = f1;
        x1 = b - phi * (b - a);
        f1 = profile(D, to_r(x1), u);
      } else {
        a = x1;
        x1 = x2;
        f1 = f2;
        x2 = a + phi * (b - a);
        f2 = profile(D, to_r(x2), u);
      }
    }
    for (const Fit &f : {f1, f2})
      if (f.sse < best.sse) best = f;
  }
  return best;
}

}  // namespace

extern "C" {

int ngsld_host_decay_fit(uint64_t n_bins, const double *dist, const double *value, int field, double n_ind, double recomb_rate,
                         ngsld_decay_fit_result *out) try {
  if (out == nullptr || dist == nullptr || value == nullptr || n_bins == 0) return NGSLD_ERR_INVALID;
  if (field != 4 && field != 6 && field != 7) return NGSLD_ERR_INVALID;  // (5, D: the script has no model)
  if (!(n_ind >= 0) || !std::isfinite(n_ind)) return NGSLD_ERR_INVALID;
  if (!(recomb_rate > 0) || !std::isfinite(recomb_rate)) return NGSLD_ERR_INVALID;
  if (field == 6 && n_ind > 0) return NGSLD_ERR_INVALID;
  for (uint64_t i = 0; i < n_bins; ++i) {
    if (!std::isfinite(dist[i]) || dist[i] < 0 || !std::isfinite(value[i])) return NGSLD_ERR_INVALID;
    if (field == 6 && dist[i] * recomb_rate / 1e6 > 1) return NGSLD_ERR_INVALID;  // (the script's curve is NaN there)
  }
  Data D{dist, value, n_bins, field == 6 ? kDp : n_ind > 0 ? kR2Nind : kR2, n_ind, recomb_rate};
  double hi = 1.0;  // C in [0, 1]
  if (D.model == kDp) {
    // t in [0, 50 / g], g = -ln(1 - d rr / 10^6) at the smallest d > 0 whose base is not 0: beyond it every term with d > 0
    // is below e^-50 of (h - l), and the sum of squares is flat to rounding
    double g = INFINITY;
    for (uint64_t i = 0; i < n_bins; ++i) {
      const double x = 1.0 - dist[i] * recomb_rate / 1e6;
      if (x < 1.0 && x > 0.0) g = std::min(g, -std::log(x));
    }
    hi = std::isfinite(g) ? 50.0 / g : 1.0;
  }
  const Fit f = minimise(D, hi);
  out->rate = f.rate;
  out->ld_max = D.model == kR2Nind ? 0.0 : f.h;
  out->ld_min = D.model == kR2Nind ? 0.0 : f.l;
  out->sse = sse_at(D, f.rate, f.h, f.l);
  out->n_bins = n_bins;
  return NGSLD_OK;
} catch (...) {
  return NGSLD_ERR_NOMEM;
}

}  // extern "C"
