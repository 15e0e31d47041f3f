// ld_text_row.h -- one TSV row on the device, for any of ld_fmt.h's emitters: the rows of a batch (ld_text.hip) and the linked
// pairs (linked.hip) print a pair with the same code, so a linked row is byte for byte the row of the full table.
#pragma once

#include "ld_fmt.h"
#include "ld_text.h"

namespace ngsld {

template <class E>
__device__ __forceinline__ void put_label(E &e, const TextArgs &A, uint32_t s) {
  if (A.labels == nullptr) {  // glibc prints "(null)" for the reference's NULL labels (ngsLD.cpp:135)
    e.put('('); e.put('n'); e.put('u'); e.put('l'); e.put('l'); e.put(')');
    return;
  }
  const uint64_t b = A.label_off[s], n = A.label_off[s + 1] - b;
  for (uint64_t i = 0; i < n; ++i) e.put(A.labels[b + i]);
}

// host_io.cpp format_row
template <class E>
__device__ __forceinline__ bool format_row(E &e, const TextArgs &A, uint32_t s1, uint32_t s2, uint64_t k) {
  bool ok = true;
  put_label(e, A, s1);
  e.put('\t');
  put_label(e, A, s2);
  e.put('\t');
  // ngsLD.cpp:241: dist is the running sum of pos_dist over (s1, s2]; INFINITY once a chromosome change is passed
  const double dist = A.infc[s2] != A.infc[s1] ? __builtin_inf() : A.cum[s2] - A.cum[s1];
  ok &= put_fixed<0>(e, dist);
  e.put('\t');
  const ngsld_rec_std sr = A.std_rec[k];
  ok &= put_fixed<6>(e, sr.r2_ExpG); e.put('\t');
  ok &= put_fixed<6>(e, sr.D);       e.put('\t');
  ok &= put_fixed<6>(e, sr.Dp);      e.put('\t');
  ok &= put_fixed<6>(e, sr.r2);
  if (A.ext_rec != nullptr) {
    const ngsld_rec_ext er = A.ext_rec[k];
    const double *h = er.hap;
    const double hm0 = 1 - (h[0] + h[1]);  // ngsLD.cpp:297-298
    const double hm1 = 1 - (h[0] + h[2]);
    float chi2 = 0;  // ngsLD.cpp:328-333, float arithmetic as there
    const float freq_A = (float)(h[0] + h[1]);
    const float freq_B = (float)(h[0] + h[2]);
    const float exp_hap[4] = {freq_A * freq_B, freq_A * (1 - freq_B), (1 - freq_A) * freq_B,
                              (1 - freq_A) * (1 - freq_B)};
    for (int i = 0; i < 4; i++) {
      const double d = h[i] - (double)exp_hap[i];
      chi2 = (float)((double)chi2 + d * d / (double)exp_hap[i]);
    }
    e.put('\t');
    put_u64(e, er.n_ind_data);  // ngsLD.cpp:336-349
    e.put('\t');
    ok &= put_fixed<6>(e, A.maf[s1]); e.put('\t');
    ok &= put_fixed<6>(e, A.maf[s2]); e.put('\t');
    for (int i = 0; i < 4; i++) {
      ok &= put_fixed<6>(e, h[i]);
      e.put('\t');
    }
    ok &= put_fixed<6>(e, hm0); e.put('\t');
    ok &= put_fixed<6>(e, hm1); e.put('\t');
    ok &= put_fixed<6>(e, (double)chi2);
    const char lit[] = "\t0.000000\t";  // loglike is the literal 0.0 (ngsLD.cpp:347)
    for (int i = 0; i < 10; ++i) e.put(lit[i]);
    put_u64(e, er.n_iter);
  }
  e.put('\n');
  return ok;
}

}  // namespace ngsld
