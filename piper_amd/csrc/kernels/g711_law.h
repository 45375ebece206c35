// The G.711 law itself, one sample at a time: the encoder the device kernels (g711.h) and the host twins share, and the
// expanders. Included by host code too (pe_g711_encode / pe_g711_decode, the host conversion of pe_stream_next); the
// formulas and their source are in g711.h and DESIGN.md 4.10.
#pragma once
#include "params.h"

namespace pe {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PE_G711_FN __host__ __device__ __forceinline__
#else
#define PE_G711_FN inline
#endif

PE_G711_FN unsigned g711_ulaw(int lin) {
  const int m = lin >> 15;                               // 0 or -1: lin ^ m is lin or ~lin
  int a = ((lin ^ m) >> 2) + 33;
  a = a > 0x1FFF ? 0x1FFF : a;
  const int seg = 27 - __builtin_clz((unsigned)a);       // a in [33, 8191]: bit length in [6, 13], seg in [1, 8]
  return (unsigned)((((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF))) | (~m & 0x80));
}

PE_G711_FN unsigned g711_alaw(int lin) {
  const int m = lin >> 15;
  const int ix = (lin ^ m) >> 4;                         // [0, 2047]
  int e = 28 - __builtin_clz((unsigned)(ix | 1));        // bit length less 4: <= 0 on the linear segment
  e = e < 0 ? 0 : e;
  const int sh = e > 0 ? e - 1 : 0;
  return (unsigned)(((((ix >> sh) & 0xF) | (e << 4)) | (~m & 0x80)) ^ 0x55);
}

PE_G711_FN unsigned g711_code(int law, int lin) { return law == G711_ALAW ? g711_alaw(lin) : g711_ulaw(lin); }

// the expanders of the same tools (host only: nothing on the device decodes)
inline int g711_ulaw_expand(unsigned code) {
  const int mant = ~(int)code, exponent = (mant >> 4) & 7, step = 4 << (exponent + 1);
  const int v = (0x80 << exponent) + step * (mant & 0xF) + step / 2 - 4 * 33;
  return code < 0x80 ? -v : v;
}
inline int g711_alaw_expand(unsigned code) {
  const int ix = (int)(code ^ 0x55) & 0x7F, iexp = ix >> 4;
  int mant = ix & 0xF;
  if (iexp > 0) mant += 16;
  mant = (mant << 4) + 8;
  if (iexp > 1) mant <<= iexp - 1;
  return code > 127 ? mant : -mant;
}

}  // namespace pe
