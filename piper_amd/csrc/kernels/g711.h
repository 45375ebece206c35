// G.711 companding of the delivered int16: 8-bit mu-law (PCMU) or A-law (PCMA), the last stage of the delivery chain
// (DESIGN.md 4.10). The law is that of the ITU-T G.191 software tools; with `lin` an int16, >> arithmetic, ~ one's complement:
//   mu-law:  a = min((lin < 0 ? ~lin >> 2 : lin >> 2) + 33, 0x1FFF); seg = 1 + bit length of (a >> 6);
//            code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)), | 0x80 for lin >= 0
//   A-law:   ix = lin < 0 ? ~lin >> 4 : lin >> 4; ix > 15: e = 1, while (ix > 31) { ix >>= 1; e++; }, ix = ix - 16 + (e << 4);
//            code = (ix | 0x80 for lin >= 0) ^ 0x55
// Here both are branch-free: the segment is a count of leading zeros (a >= 33, so seg = bit length of a, less 5), no table.
// The per-sample functions live in g711_law.h: they are also the host twins (pe_g711_encode) and what pe_stream_next uses
// for its host-side conversion.
#pragma once
#include "g711_law.h"

namespace pe {

// A workgroup converts G711_SPAN samples: G711_TPB threads of 8, one 16-byte load and one 8-byte store each where the
// alignment allows. The kernel is bound by its store instructions, not by the arithmetic.
struct alignas(16) G711In { short v[8]; };
struct alignas(8) G711Out { unsigned lo, hi; };

__device__ __forceinline__ unsigned g711_pack4(int law, const short* s) {
  return g711_code(law, s[0]) | (g711_code(law, s[1]) << 8) | (g711_code(law, s[2]) << 16) | (g711_code(law, s[3]) << 24);
}

// One row of L int16 at `src` -> L codes at out[off, off + L); the caller has cut [off, off + L) to the output buffer. `out`
// is 4-byte aligned, `off` has any residue mod 4, and the dword that holds the row's first or last bytes may also hold a
// neighbouring row's, written by another workgroup: such a dword is never stored whole and never read back. The head
// (up to the first destination-aligned dword) and the tail (from the last) go out as byte stores from the row's first
// workgroup, only the interior as dwords. Rows of 0 to 3 samples have no interior.
__device__ __forceinline__ void g711_row(int law, const short* src, long L, unsigned char* out, long off, int tile) {
  if (L <= 0) return;
  const long h = (4 - (off & 3)) & 3;                    // head bytes
  const long I = L > h ? ((L - h) & ~3L) : 0;            // interior samples: whole destination dwords
  const int t = threadIdx.x;
  if (tile == 0) {
    if (t < 4) {
      if (t < h && t < L) out[off + t] = (unsigned char)g711_code(law, src[t]);
    } else if (t < 8) {
      const long i = h + I + (t - 4);
      if (L > h && i < L) out[off + i] = (unsigned char)g711_code(law, src[i]);
    }
  }
  const long i0 = (long)tile * G711_SPAN + 8L * t;       // of the interior
  if (i0 >= I) return;
  const short* s = src + h + i0;
  unsigned char* d = out + off + h + i0;                 // 4-byte aligned
  if (i0 + 8 <= I) {
    G711In x;
    if ((reinterpret_cast<unsigned long long>(s) & 15) == 0) {
      __builtin_memcpy(&x, __builtin_assume_aligned(s, 16), 16);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x.v[j] = s[j];
    }
    const unsigned lo = g711_pack4(law, x.v), hi = g711_pack4(law, x.v + 4);
    if ((reinterpret_cast<unsigned long long>(d) & 7) == 0) {
      const G711Out o{lo, hi};
      __builtin_memcpy(__builtin_assume_aligned(d, 8), &o, 8);
    } else {
      __builtin_memcpy(__builtin_assume_aligned(d, 4), &lo, 4);
      __builtin_memcpy(__builtin_assume_aligned(d + 4, 4), &hi, 4);
    }
  } else {                                               // (I is a multiple of 4: exactly one dword is left)
    short v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = s[j];
    const unsigned w = g711_pack4(law, v);
    __builtin_memcpy(__builtin_assume_aligned(d, 4), &w, 4);
  }
}

// Rows form (whole utterances): grid = (spans of the longest row, rows). Row b holds lens[b] * len_mul int16 at
// pcm + b * p_bs, cut to the row; its codes start at the sum of the lengths before it, as pcm16_body (post.h) computes the
// packed host offset -- in the kernel, because inside the one-graph form of a call the host does not know the lengths yet.
// Everything is cut to the out_cap bytes of `out`.
__global__ __launch_bounds__(G711_TPB) void g711_kernel(const int* lens, int len_mul, const short* pcm, long p_bs,
                                                        unsigned char* out, long out_cap, int law) {
  PE_KTRACE(43);
  const int b = blockIdx.y;
  long off = 0;
  for (int u = 0; u < b; ++u) {
    const long n = (long)lens[u] * len_mul;
    off += n < 0 ? 0 : (n > p_bs ? p_bs : n);
  }
  long L = (long)lens[b] * len_mul;
  L = L < 0 ? 0 : (L > p_bs ? p_bs : L);
  if (off >= out_cap) return;
  if (L > out_cap - off) L = out_cap - off;
  if ((long)blockIdx.x * G711_SPAN >= L) return;         // (span 0 of a row also carries its head and tail)
  g711_row(law, pcm + (long)b * p_bs, L, out, off, (int)blockIdx.x);
}

// Flat form (stream chunks): n contiguous int16 at a 16-byte aligned base -> n codes; grid = spans of n. The caller has
// cut n to both buffers.
__global__ __launch_bounds__(G711_TPB) void g711_flat_kernel(const short* pcm, long n, unsigned char* out, int law) {
  PE_KTRACE(43);
  if ((long)blockIdx.x * G711_SPAN >= n) return;
  g711_row(law, pcm, n, out, 0, (int)blockIdx.x);
}

}  // namespace pe
