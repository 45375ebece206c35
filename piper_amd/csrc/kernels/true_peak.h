// True peak of whole utterances: the largest |sample| of the delivered float waveform interpolated Q times, Q the
// oversampling ITU-R BS.1770-4 Annex 2 asks for (4 at 48 kHz, proportionally more below). Nothing is stored per sample:
// one word per row. (gfx950 / CDNA4 device code. The reference has no such stage: its ceiling is the sample peak of
// pcm16_kernel's rule, src/cpp/piper.cpp:410-431. The arithmetic is DESIGN.md 4.6.)
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// The interpolator is the resampler's filter for the pair fs -> Q fs (L = Q, M = 1: resample.h), so native position c has
// the Q outputs
//   y[c Q + ph] = sum_k coef[ph][k] * x[c - K + 1 + k],   k = 0 .. 2 K - 1,   ph = 0 .. Q - 1
// with x = 0 outside [0, n) and K = TP_K whatever fs is (the cutoff follows fs). A dedicated kernel, not resample_kernel
// with its store taken out: with M = 1 the 2 K native samples of a position serve all Q phases from registers and the
// table rows are read wave-uniformly out of LDS, where resample_kernel's walk over OUTPUTS would read every native sample
// Q times more often and form a phase by division per output.
// grid = (tiles of TP_TILE native samples of the bucket, rows); a workgroup whose tile starts behind the row's end returns.
// The tile and K samples on either side are staged into LDS -- 16-byte loads from the 16-byte boundary below the first one
// where the row is aligned, zeros outside [0, n) -- and so is the table. Every thread walks native positions tile-local
// i = thread, thread + 256, ...; the taps of a phase are summed first to last with one fma each, so a run repeats bit for
// bit. max |y| meets across the lanes, then across the four waves through LDS, and goes to the row's word with one
// atomicMax on the bit pattern per workgroup (non-negative floats order like their bit patterns). The word was zeroed by
// loudness_seg_kernel, which is stream-ordered before this launch.
// STORE (true_peak_v_kernel, the look-ahead limiter under the true-peak ceiling): the per-position maximum over the phases
// goes to p.v as well. The default instantiation is the kernel as it was: nothing of the store is in it.
template <bool STORE>
__device__ __forceinline__ void true_peak_body(const TpP& p) {
  __shared__ __attribute__((aligned(16))) float xs[TP_SPAN];
  __shared__ __attribute__((aligned(16))) float cs[TP_MAXQ * TP_TAPS];
  __shared__ float wmax[4];
  const int b = blockIdx.y;
  long nl = (long)p.lens[b] * p.len_mul;
  nl = nl < 0 ? 0 : (nl > p.x_cap ? p.x_cap : nl);
  const int n = (int)nl;
  const long t0l = (long)blockIdx.x * TP_TILE;
  if (t0l >= n) return;
  const int t0 = (int)t0l;
  const int nt = n - t0 < TP_TILE ? n - t0 : TP_TILE;
  const int Q = p.Q < 1 ? 1 : (p.Q > TP_MAXQ ? TP_MAXQ : p.Q);
  // buffer element of the first tap of the tile's first position, the 16-byte boundary below it, the span from there
  const int r = t0 - TP_K + 1, rs = r & ~3, lead = r - rs;
  const int span = lead + nt - 1 + TP_TAPS;            // <= 3 + TP_TILE - 1 + TP_TAPS <= TP_SPAN
  const float* xb = p.x + (long)b * p.x_bs;
  if ((reinterpret_cast<size_t>(xb) & 15) == 0) {
    for (int q = threadIdx.x * 4; q < span; q += 1024) {
      const int i = rs + q;
      f32x4 v;
      if (i >= 0 && i + 4 <= n) {
        v = *reinterpret_cast<const f32x4*>(xb + i);
      } else {
        for (int k = 0; k < 4; ++k) v[k] = (i + k >= 0 && i + k < n) ? xb[i + k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(xs + q) = v;
    }
  } else {
    for (int q = threadIdx.x; q < span; q += 256) {
      const int i = rs + q;
      xs[q] = (i >= 0 && i < n) ? xb[i] : 0.f;
    }
  }
  for (int q = threadIdx.x; q < Q * TP_TAPS; q += 256) cs[q] = p.coef[q];
  __syncthreads();
  float m = 0.f;
  for (int i = threadIdx.x; i < nt; i += 256) {
    float xv[TP_TAPS];
    float vm = 0.f;
    (void)vm;
#pragma unroll
    for (int k = 0; k < TP_TAPS; ++k) xv[k] = xs[lead + i + k];
    for (int ph = 0; ph < Q; ++ph) {
      const float* cf = cs + ph * TP_TAPS;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < TP_TAPS; k += 4) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cf + k);
        acc = fmaf(c[0], xv[k], acc);
        acc = fmaf(c[1], xv[k + 1], acc);
        acc = fmaf(c[2], xv[k + 2], acc);
        acc = fmaf(c[3], xv[k + 3], acc);
      }
      m = fmaxf(m, fabsf(acc));
      if constexpr (STORE) vm = fmaxf(vm, fabsf(acc));
    }
    if constexpr (STORE) p.v[(long)b * p.x_bs + t0 + i] = vm;
  }
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(p.tpeak + b, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}
__global__ __launch_bounds__(256) void true_peak_kernel(TpP p) {
  PE_KTRACE(35);
  true_peak_body<false>(p);
}
__global__ __launch_bounds__(256) void true_peak_v_kernel(TpP p) {
  PE_KTRACE(37);
  true_peak_body<true>(p);
}

}  // namespace pe
