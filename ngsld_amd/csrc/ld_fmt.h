// ld_fmt.h -- the device's "%f" digit generator and its byte writers, shared by the TSV rows (ld_text.hip) and the LD block
// matrices (blocks.hip): a cell of a block matrix is byte for byte the text the TSV prints for that pair and column.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngsld {

struct Counter {
  uint64_t n = 0;
  __device__ __forceinline__ void put(char) { ++n; }
};
struct Writer {
  char *p;
  __device__ __forceinline__ void put(char c) { *p++ = c; }
};
// A row goes out in aligned 8-byte words: the characters collect in a register and every eighth is one store (a thread's
// row is ~150 bytes of its own, so a byte store is a whole memory request for one byte -- and the 64 lanes of a wave-wide
// store hit 64 different cache lines either way).  The partial words at the two ends of the row, which it shares with the
// neighbouring rows, go out byte by byte.
// (Tried first: rows composed in LDS, the wavefront's contiguous piece copied out 16 bytes per lane.  Its 49 KB of LDS per
// workgroup cannot sit beside the pair kernel's two 72 KB workgroups on a CU, so the write pass, which runs beside the next
// batch's pair kernel, starved: 332 ms against 96 ms for the plain byte stores over configs[2].)
struct WordWriter {
  char *p;        // aligned address of the word being filled
  uint64_t acc;
  uint32_t cnt;   // bytes of the word filled so far (counting the leading bytes that are not this row's)
  uint32_t head;  // leading bytes of the FIRST word that belong to the previous row
  __device__ __forceinline__ explicit WordWriter(char *dst) {
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 7u);
    p = dst - mis;
    acc = 0;
    cnt = head = mis;
  }
  __device__ __forceinline__ void put(char c) {
    acc |= (uint64_t)(unsigned char)c << (8 * cnt);
    if (++cnt == 8) {
      if (head) {
        for (uint32_t b = head; b < 8; ++b) p[b] = (char)(acc >> (8 * b));
        head = 0;
      } else {
        *reinterpret_cast<uint64_t *>(p) = acc;
      }
      p += 8;
      acc = 0;
      cnt = 0;
    }
  }
  __device__ __forceinline__ void finish() {
    for (uint32_t b = head; b < cnt; ++b) p[b] = (char)(acc >> (8 * b));
  }
};

template <class E>
__device__ __forceinline__ void put_u64(E &e, uint64_t v) {
  char tmp[24];
  int n = 0;
  do {
    tmp[n++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  while (n) e.put(tmp[--n]);
}

// host_io.cpp put_fixed<DECIMALS>, minus its snprintf fallback: returns false where that would be taken
template <int DECIMALS, class E>
__device__ __forceinline__ bool put_fixed(E &e, double v) {
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  const bool neg = bits >> 63;
  const int ebits = (int)((bits >> 52) & 0x7ff);
  uint64_t m = bits & 0xfffffffffffffull;
  if (ebits == 0x7ff) {
    if (m) {
      e.put('-'); e.put('n'); e.put('a'); e.put('n');
      return true;
    }
    if (neg) e.put('-');
    e.put('i'); e.put('n'); e.put('f');
    return true;
  }
  int ex;  // value = m * 2^ex
  if (ebits == 0) {
    ex = -1074;
  } else {
    m |= 1ull << 52;
    ex = ebits - 1075;
  }
  constexpr uint64_t kScale = DECIMALS == 6 ? 1000000ull : 1ull;
  uint64_t q;
  if (ex >= 0) {
    if (ex > 10 || (DECIMALS == 6 && ex > -1)) return false;
    q = (m << ex) * kScale;
  } else {
    const int k = -ex;
    const unsigned __int128 M = (unsigned __int128)m * kScale;
    if (k >= 127) {
      q = 0;
    } else {
      const unsigned __int128 quo = M >> k;
      if (quo >> 63) return false;
      q = (uint64_t)quo;
      const unsigned __int128 rem = M - (quo << k), half = (unsigned __int128)1 << (k - 1);
      if (rem > half || (rem == half && (q & 1))) ++q;
    }
  }
  if (neg) e.put('-');
  if (DECIMALS == 0) {
    put_u64(e, q);
    return true;
  }
  put_u64(e, q / 1000000ull);
  uint32_t f = (uint32_t)(q % 1000000ull);
  char d[6];
  for (int i = 5; i >= 0; --i) {
    d[i] = (char)('0' + f % 10);
    f /= 10;
  }
  e.put('.');
  for (int i = 0; i < 6; ++i) e.put(d[i]);
  return true;
}

}  // namespace ngsld
