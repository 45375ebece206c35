// Output-rate conversion: a polyphase Kaiser-windowed sinc on the float waveform, before the int16 conversion.
// (gfx950 / CDNA4 device code. The reference's runtime never resamples; what it fixes is the rule the int16 conversion
// follows afterwards -- scale by the maximum of what is delivered, src/cpp/piper.cpp:410-431.)
#pragma once
#include "../pe_rt.h"
#include "params.h"
#include "post.h"

namespace pe {

// With g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g, output n of an utterance sits at native position n * M / L:
//   y[n] = sum_k coef[(n * M) mod L][k] * x[floor(n * M / L) - K + 1 + k],   k = 0 .. Tp - 1
// with x = 0 outside the utterance. The table holds the windowed sinc sampled at (phase + (K - 1 - k) * L) / (L * fs_in)
// seconds, built in f64 on the host and rounded once to f32 (engine.cpp: set_output_rate); entries past the window's
// support, the padding up to Tp included, are exact zeros.

// First launch of the stage: the device row block (params.h: rs_*), one thread per row. hst != null: the rows a stream
// filled in pinned host memory, read in place; null: whole utterances of lens[b] * len_mul native samples from index 0.
// Lengths are cut to the buffers (x_cap / y_cap elements per row) so that nothing outside a row is ever read or written.
__global__ __launch_bounds__(64) void resample_rows_kernel(const int* hst, const int* lens, int len_mul, int* rows, int cap,
                                                           int B, long x_cap, long y_cap, int L, int M) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || b >= cap) return;
  long long n0 = 0, org = 0;
  long vlen, count;
  if (hst) {
    n0 = reinterpret_cast<const long long*>(hst)[b];
    org = reinterpret_cast<const long long*>(hst + rs_o_org(cap))[b];
    count = hst[rs_o_count(cap) + b];
    vlen = hst[rs_o_vlen(cap) + b];
    vlen = vlen < 0 ? 0 : (vlen > x_cap ? x_cap : vlen);
  } else {
    vlen = (long)lens[b] * len_mul;
    vlen = vlen < 0 ? 0 : (vlen > x_cap ? x_cap : vlen);
    count = (vlen * L + M - 1) / M;
  }
  count = count < 0 ? 0 : (count > y_cap ? y_cap : count);
  reinterpret_cast<long long*>(rows)[b] = n0 < 0 ? 0 : n0;
  reinterpret_cast<long long*>(rows + rs_o_org(cap))[b] = org;
  rows[rs_o_count(cap) + b] = (int)count;
  rows[rs_o_vlen(cap) + b] = (int)vlen;
  rows[rs_o_peak(cap) + b] = 0;
}

// grid = (tiles of p.tile output samples, rows). Traffic is small (4 bytes in per native sample, 4 out per output, the
// table stays in cache); what it costs is the taps -- 2.7 - 3.7 x 10^12 per second measured, profiles/resample.md.
// A workgroup stages the native span of its tile into LDS -- 16-byte loads from the 16-byte boundary below the span's first sample, zeros outside the row's valid range -- then every thread walks outputs
// tile-local i = thread, thread + 256, ...: n * M is formed in 64 bits once per workgroup (33 M outputs x M = 147 pass
// 2^32) and i * M in 32 (tile <= 1024, M < 2^20). Taps are summed first to last with one fma each, so a run repeats bit
// for bit. max |y| goes to the row's peak word with one atomicMax on the bit pattern per workgroup (non-negative floats
// order like their bit patterns).
__global__ __launch_bounds__(256) void resample_kernel(RsP p) {
  PE_KTRACE(27);
  __shared__ __attribute__((aligned(16))) float xs[RS_SPAN];
  __shared__ float wmax[4];
  const int b = blockIdx.y, cap = p.cap;
  const int count = p.rows[rs_o_count(cap) + b];
  const long t0 = (long)blockIdx.x * p.tile;
  if (t0 >= count) return;
  const int nt = count - t0 < p.tile ? (int)(count - t0) : p.tile;
  const int vlen = p.rows[rs_o_vlen(cap) + b];
  const long long n0 = reinterpret_cast<const long long*>(p.rows)[b] + t0;
  const long long org = reinterpret_cast<const long long*>(p.rows + rs_o_org(cap))[b];
  const long long pos = n0 * p.M, c0 = pos / p.L;
  const unsigned ph0 = (unsigned)(pos - c0 * p.L);
  // buffer element of the first tap of the tile's first output, the 16-byte boundary below it, the span from there
  const long long r = c0 - p.K + 1 - org, rs = r & ~3LL;
  const int lead = (int)(r - rs);
  const long span = lead + (long)((ph0 + (unsigned)(nt - 1) * (unsigned)p.M) / (unsigned)p.L) + p.Tp;
  if (span > RS_SPAN) return;          // (the host sizes the tile so that it fits)
  const float* xb = p.x + (long)b * p.x_bs;
  if ((reinterpret_cast<size_t>(xb) & 15) == 0) {
    for (int q = threadIdx.x * 4; q < span; q += 1024) {
      const long long i = rs + q;
      f32x4 v;
      if (i >= 0 && i + 4 <= vlen) {
        v = *reinterpret_cast<const f32x4*>(xb + i);
      } else {
        for (int k = 0; k < 4; ++k) v[k] = (i + k >= 0 && i + k < vlen) ? xb[i + k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(xs + q) = v;
    }
  } else {
    for (int q = threadIdx.x; q < span; q += 256) {
      const long long i = rs + q;
      xs[q] = (i >= 0 && i < vlen) ? xb[i] : 0.f;
    }
  }
  __syncthreads();
  float* yb = p.y + (long)b * p.y_bs + t0;
  float m = 0.f;
  for (int i = threadIdx.x; i < nt; i += 256) {
    const unsigned q = ph0 + (unsigned)i * (unsigned)p.M, dc = q / (unsigned)p.L, ph = q - dc * (unsigned)p.L;
    const float* cf = p.coef + (long)ph * p.Tp;
    const float* xp = xs + lead + dc;
    float acc = 0.f;
    for (int k = 0; k < p.Tp; k += 4) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(cf + k);
      acc = fmaf(c[0], xp[k], acc);
      acc = fmaf(c[1], xp[k + 1], acc);
      acc = fmaf(c[2], xp[k + 2], acc);
      acc = fmaf(c[3], xp[k + 3], acc);
    }
    yb[i] = acc;
    m = fmaxf(m, fabsf(acc));
  }
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<unsigned*>(p.rows) + rs_o_peak(cap) + b,
              __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}

// Chunk delivery of a batch stream at a converted rate: chunk_pcm_kernel (post.h) on the resampled rows. The chunk is
// y[b][0 .. count_b) of the row block, its peak the one resample_kernel folded; where it goes in the packed pinned host
// output comes from the window state block `st` (params.h: sb_*), whose offsets the host wrote in output samples.
// GAIN (chunk_pcm_rs_gain_kernel): the stream-wide levels, as chunk_pcm_gain_kernel (post.h) -- the operands come from the
// device gain block `gq` (params.h: sgd_*, at the window state's cap), the ramp counts in output samples.
template <bool GAIN>
__device__ __forceinline__ void chunk_pcm_rs_body(const float* y, long y_bs, const int* rows, int rcap, const int* st, int cap,
                                                  const int* gq) {
  const int b = blockIdx.y;
  int count = rows[rs_o_count(rcap) + b];
  count = count < 0 ? 0 : (count > y_bs ? (int)y_bs : count);
  if ((long)blockIdx.x * CHUNK_SPB >= count) return;
  const float* a = y + (long)b * y_bs;
  const long off = reinterpret_cast<const long long*>(st + sb_o_off(cap))[b];
  short* pcm = reinterpret_cast<short* const*>(st + sb_o_ptrs(cap))[0] + off;
  float* fout = reinterpret_cast<float* const*>(st + sb_o_ptrs(cap))[1];
  float scale, dg = 0.f, Rf = 1.f;
  int R = 0;
  if constexpr (GAIN) {
    scale = __uint_as_float(reinterpret_cast<const unsigned*>(gq)[sgd_o_g1(cap) + b]);
    dg = __uint_as_float(reinterpret_cast<const unsigned*>(gq)[sgd_o_g0(cap) + b]) - scale;
    R = gq[sgd_o_ramp(cap) + b];
    R = R < 0 ? 0 : (R > count ? count : R);
    Rf = (float)(R > 0 ? R : 1);
  } else {
    const float peak = fmaxf(0.01f, __uint_as_float(reinterpret_cast<const unsigned*>(rows)[rs_o_peak(rcap) + b]));
    scale = 32767.0f / peak;
  }
  for (long base = (long)blockIdx.x * CHUNK_SPB; base < count; base += (long)gridDim.x * CHUNK_SPB)
#pragma unroll
    for (int j = 0; j < CHUNK_SPB / 256; ++j) {
      const long i = base + j * 256 + threadIdx.x;
      if (i < count) {
        const float x = a[i];
        float v = x * chunk_gain_at<GAIN>(scale, dg, R, Rf, i);
        v = fminf(fmaxf(v, -32768.0f), 32767.0f);
        pcm[i] = (short)v;
        if (fout) fout[off + i] = x;
      }
    }
}
__global__ __launch_bounds__(256) void chunk_pcm_rs_kernel(const float* y, long y_bs, const int* rows, int rcap, const int* st,
                                                           int cap) {
  PE_KTRACE(28);
  chunk_pcm_rs_body<false>(y, y_bs, rows, rcap, st, cap, nullptr);
}
__global__ __launch_bounds__(256) void chunk_pcm_rs_gain_kernel(const float* y, long y_bs, const int* rows, int rcap,
                                                                const int* st, int cap, const int* gq) {
  PE_KTRACE(31);
  chunk_pcm_rs_body<true>(y, y_bs, rows, rcap, st, cap, gq);
}

}  // namespace pe
