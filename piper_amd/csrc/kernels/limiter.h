// Look-ahead limiter of the target loudness: a row whose peak would have lowered the whole utterance (LIMITED) keeps the
// gain of its loudness target instead, and only the neighbourhood of its peaks is turned down, by a zero-phase envelope.
// (gfx950 / CDNA4 device code. The reference has no such stage: its level follows the peak alone, src/cpp/piper.cpp:410-431.
// The arithmetic is DESIGN.md 4.6.)
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// The int16 conversion of one sample, as pcm16_body (post.h) stores it: the device row and the packed pinned host copy.
__device__ __forceinline__ void lim_store(const LimP& p, int b, int t, float v, long host_off) {
  p.pcm[(long)b * p.p_bs + t] = (short)v;
  if (p.host) p.host[host_off + t] = (short)v;
}

// The tile body shared with stream_limiter_kernel (stream_limiter.h). ms[0 .. span) holds r on entry (and a barrier has
// passed); on return ms[q] = d[q] = 1 - min r[q - W .. q + W] for the q whose window lies in the span, 0 for the others.
__device__ __forceinline__ void lim_window_d(float* ms, int span, int W, int tid) {
  float v[LIM_PER];
  int run = 1;
  for (; 2 * run <= 2 * W + 1; run *= 2) {
#pragma unroll
    for (int j = 0; j < LIM_PER; ++j) {
      const int q = tid + 256 * j;
      v[j] = q < span ? fminf(ms[q], q + run < span ? ms[q + run] : 1.0f) : 1.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LIM_PER; ++j) {
      const int q = tid + 256 * j;
      if (q < span) ms[q] = v[j];
    }
    __syncthreads();
  }
  // ms[q] = min r[q .. q + run - 1]; d[q] = 1 - min(ms[q - W], ms[q + W - run + 1]) for the q whose window lies in the span
#pragma unroll
  for (int j = 0; j < LIM_PER; ++j) {
    const int q = tid + 256 * j;
    v[j] = (q >= W && q + W < span) ? 1.0f - fminf(ms[q - W], ms[q + W - run + 1]) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LIM_PER; ++j) {
    const int q = tid + 256 * j;
    if (q < span) ms[q] = v[j];
  }
  __syncthreads();
}
// e of the span element q from d (ms), r (rs) and the weights: the taps first to last, one fma each; skipped where every d
// of the sum is 0 (the minimum over +-2 W is 1).
__device__ __forceinline__ float lim_env_at(const float* ms, const float* rs, const float* hs, int q, int W) {
  float e = 1.0f;
  if (ms[q - W] != 0.f || ms[q + W] != 0.f) {
    const float* d = ms + q - W;
    float acc = 0.f;
    for (int k = 0; k <= 2 * W; ++k) acc = fmaf(hs[k], d[k], acc);
    e = fminf(rs[q], 1.0f - acc);
  }
  return e;
}

// With x[0 .. n) a row, g = scale / 32767 its loudness gain, C the ceiling and W the window (all f32 unless said):
//   r[i] = min(1, C / (g |x[i]|)), 1 where x[i] = 0 and outside [0, n): the gain that alone would hold sample i
//   m[j] = min r[j - W .. j + W],  d = 1 - m
//   e[i] = min(r[i], 1 - sum_{k = -W .. W} h[k] d[i + k]),  h >= 0, sum h = 1
//   pcm[i] = trunc(clamp((x[i] e[i]) scale, +-floor(32767 C)))
// Every m[i + k] of the sum is at most r[i], so the smoothed envelope lies under r already and the outer min only catches
// rounding; where no sample within 2 W passes the ceiling every d of the sum is 0 and e is exactly 1. Nothing is recursive:
// a workgroup needs 2 W samples of halo on either side of its tile and no state from its neighbours, so e is continuous
// across tile seams by construction.
// grid = (tiles of LIM_TILE samples of the bucket, rows); a workgroup whose tile starts behind the row's end returns, one of
// a row that is not SHAPED does pcm16_gain_kernel's work for its tile. Otherwise: the tile and its halo are staged into LDS
// (16-byte loads from the 16-byte boundary below the first sample where the row is aligned, zeros outside [0, n)); r; the
// sliding minimum by doubling steps -- after log2(P) steps an entry holds the minimum of P = 2^k <= 2 W + 1 < 2 P entries
// from itself on, and min being idempotent the window of 2 W + 1 is the min of two such runs, exact whatever the schedule
// (every step reads into registers, meets, writes, meets); the taps summed first to last with one fma each out of LDS, so a
// run repeats bit for bit, and skipped where the minimum over +-2 W (the min of m[i - W] and m[i + W]) is 1. LDS: three
// spans and the weights, 51.6 KB static. The row's report -- the largest 1 - e and the count of e < 1 -- goes out with one
// atomicMax on the bit pattern and one atomicAdd per workgroup into words loudness_seg_kernel cleared.
// (The row length is cut to x_cap, which pcm16_body does not do: the pass-through is that kernel's work while
// lens * len_mul <= x_cap, which holds for every caller -- x_cap is the row stride.)
// TRUE_PEAK (limiter_true_kernel, the true-peak ceiling): |x[i]| is replaced by a[i] = max(|x[i]|, v[i - 1], v[i]), v the
// per-position maxima of the interpolation that true_peak_v_kernel stored (v[-1] = 0), read from global memory while r is
// formed; instead of the int16 the kernel writes z = x e (x on rows that are not shaped) and folds max |z| into the row's
// p_z word. true_peak_kernel then runs on z and pcm16_trim_kernel converts.
template <bool TRUE_PEAK>
__device__ __forceinline__ void limiter_body(const LimP& p) {
  __shared__ __attribute__((aligned(16))) float xs[LIM_SPAN];
  __shared__ float rs[LIM_SPAN];
  __shared__ float ms[LIM_SPAN];
  __shared__ float hs[2 * LIM_MAXW + 1];
  __shared__ float wred[4];
  __shared__ int wcnt[4];
  __shared__ long s_off;
  const int b = blockIdx.y, tid = threadIdx.x;
  long nl = (long)p.lens[b] * p.len_mul;
  nl = nl < 0 ? 0 : (nl > p.x_cap ? p.x_cap : nl);
  const int n = (int)nl;
  const long t0l = (long)blockIdx.x * LIM_TILE;
  if (t0l >= n) return;
  const int t0 = (int)t0l;
  const int nt = n - t0 < LIM_TILE ? n - t0 : LIM_TILE;
  const float scale = __uint_as_float(reinterpret_cast<const unsigned*>(p.gq)[ld_o_scale(p.gcap) + b]);
  const int flags = p.gq[ld_o_flags(p.gcap) + b];
  const float* xb = p.x + (long)b * p.x_bs;
  // (the row's offset in the packed host buffer: one walk over the rows in front per workgroup)
  if (tid == 0) {
    long off = 0;
    if (!TRUE_PEAK && p.host)
      for (int u = 0; u < b; ++u) off += (long)p.lens[u] * p.len_mul;
    s_off = off;
  }
  __syncthreads();
  const long host_off = s_off;
  if (!(flags & LOUD_SHAPED)) {
    float zm = 0.f;
    for (int i = tid; i < nt; i += 256) {
      const float xv = xb[t0 + i];
      if constexpr (TRUE_PEAK) {
        p.z[(long)b * p.x_bs + t0 + i] = xv;
        zm = fmaxf(zm, fabsf(xv));
      } else {
        float v = xv * scale;
        v = fminf(fmaxf(v, -32768.0f), 32767.0f);
        lim_store(p, b, t0 + i, v, host_off);
      }
      if (p.env) p.env[(long)b * p.e_bs + t0 + i] = 1.0f;
    }
    if constexpr (TRUE_PEAK) {
      for (int o = 32; o >= 1; o >>= 1) zm = fmaxf(zm, __shfl_xor(zm, o));
      if ((tid & 63) == 0) wred[tid >> 6] = zm;
      __syncthreads();
      if (tid == 0)
        atomicMax(reinterpret_cast<unsigned*>(p.rep) + lim_o_pz(p.rcap) + b,
                  __float_as_uint(fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]))));
    }
    return;
  }
  const int W = p.W < 1 ? 1 : (p.W > LIM_MAXW ? LIM_MAXW : p.W);
  const float C = __uint_as_float(reinterpret_cast<const unsigned*>(p.ctl)[1]);
  const float g = (float)((double)scale / 32767.0);
  const float cq = (float)floor(32767.0 * (double)C);
  // buffer element of the first halo sample, the 16-byte boundary below it, the span from there
  const int r0 = t0 - 2 * W, s0 = r0 & ~3, lead = r0 - s0;
  const int span = lead + nt + 4 * W;                  // <= 3 + LIM_TILE + 4 LIM_MAXW < LIM_SPAN
  if ((reinterpret_cast<size_t>(xb) & 15) == 0) {
    for (int q = tid * 4; q < span; q += 1024) {
      const int i = s0 + q;
      f32x4 v;
      if (i >= 0 && i + 4 <= n) {
        v = *reinterpret_cast<const f32x4*>(xb + i);
      } else {
        for (int k = 0; k < 4; ++k) v[k] = (i + k >= 0 && i + k < n) ? xb[i + k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(xs + q) = v;
    }
  } else {
    for (int q = tid; q < span; q += 256) {
      const int i = s0 + q;
      xs[q] = (i >= 0 && i < n) ? xb[i] : 0.f;
    }
  }
  for (int q = tid; q < 2 * W + 1; q += 256) hs[q] = p.h[q];
  __syncthreads();
  for (int q = tid; q < span; q += 256) {
    float a = fabsf(xs[q]);
    if constexpr (TRUE_PEAK) {
      const int i = s0 + q;
      if (i >= 0 && i < n) {
        const float* vb = p.v + (long)b * p.x_bs;
        a = fmaxf(a, vb[i]);
        if (i > 0) a = fmaxf(a, vb[i - 1]);
      }
    }
    const float r = a > 0.f ? fminf(1.0f, C / (g * a)) : 1.0f;
    rs[q] = r;
    ms[q] = r;
  }
  __syncthreads();
  lim_window_d(ms, span, W, tid);
  float red = 0.f, zm = 0.f;
  int cnt = 0;
  for (int i = tid; i < nt; i += 256) {
    const int q = lead + 2 * W + i;
    const float e = lim_env_at(ms, rs, hs, q, W);
    const float z = xs[q] * e;
    if constexpr (TRUE_PEAK) {
      p.z[(long)b * p.x_bs + t0 + i] = z;
      zm = fmaxf(zm, fabsf(z));
    } else {
      float o = z * scale;
      o = fminf(fmaxf(o, -cq), cq);
      lim_store(p, b, t0 + i, o, host_off);
    }
    if (p.env) p.env[(long)b * p.e_bs + t0 + i] = e;
    red = fmaxf(red, 1.0f - e);
    cnt += e < 1.0f ? 1 : 0;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    red = fmaxf(red, __shfl_xor(red, o));
    cnt += __shfl_xor(cnt, o);
    if constexpr (TRUE_PEAK) zm = fmaxf(zm, __shfl_xor(zm, o));
  }
  if constexpr (TRUE_PEAK) {
    // (wmin of the p_z fold: the rs span is dead by now, its first four floats carry the waves' maxima)
    __syncthreads();
    if ((tid & 63) == 0) rs[tid >> 6] = zm;
  }
  if ((tid & 63) == 0) { wred[tid >> 6] = red; wcnt[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    if constexpr (TRUE_PEAK)
      atomicMax(reinterpret_cast<unsigned*>(p.rep) + lim_o_pz(p.rcap) + b,
                __float_as_uint(fmaxf(fmaxf(rs[0], rs[1]), fmaxf(rs[2], rs[3]))));
    atomicMax(reinterpret_cast<unsigned*>(p.rep) + lim_o_maxred(p.rcap) + b,
              __float_as_uint(fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]))));
    atomicAdd(p.rep + lim_o_count(p.rcap) + b, wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
  }
}
__global__ __launch_bounds__(256) void limiter_kernel(LimP p) {
  PE_KTRACE(36);
  limiter_body<false>(p);
}
__global__ __launch_bounds__(256) void limiter_true_kernel(LimP p) {
  PE_KTRACE(38);
  limiter_body<true>(p);
}

// The conversion behind the second true-peak pass (true-peak ceiling with the limiter), grid and threads as
// pcm16_gain_kernel. For a SHAPED row, with p_z = max |z| and t_z the true peak of z: the gain's two terms are the target's
// g1 = scale / 32767 and g2 = C / max(p_z, t_z); scale' = 32767 min(g1, g2), lowered by one ulp where its rounding would lift
// the peak over the ceiling, trim = min(1, g2 / g1), products clamped to +-floor(32767 C). The second term is a guarantee,
// not the mechanism: the envelope already holds a under C. Every other row is pcm16_gain_kernel's conversion of z = x.
// Thread 0 of a row's first workgroup leaves the trim in the report words and the scale that was used in the control
// block's report.
__global__ __launch_bounds__(256) void pcm16_trim_kernel(TrimP p) {
  PE_KTRACE(39);
  const int b = blockIdx.y, L = p.lens[b] * p.len_mul;
  const int t = blockIdx.x * 256 + threadIdx.x;
  float scale = __uint_as_float(reinterpret_cast<const unsigned*>(p.gq)[ld_o_scale(p.gcap) + b]);
  const int flags = p.gq[ld_o_flags(p.gcap) + b];
  float lo = -32768.0f, hi = 32767.0f, trim = 1.0f;
  if (flags & LOUD_SHAPED) {
    const float C = __uint_as_float(reinterpret_cast<const unsigned*>(p.ctl)[1]);
    const float pz = __uint_as_float(reinterpret_cast<const unsigned*>(p.rep)[lim_o_pz(p.rcap) + b]);
    const float tz = __uint_as_float(reinterpret_cast<const unsigned*>(p.rep)[lim_o_tz(p.rcap) + b]);
    const float P = fmaxf(pz, tz);
    const float cq = (float)floor(32767.0 * (double)C);
    lo = -cq; hi = cq;
    const double g1 = (double)scale / 32767.0;
    if (P > 0.f && (double)C / (double)P < g1) {
      const double g2 = (double)C / (double)P;
      trim = (float)(g2 / g1);
      scale = (float)(32767.0 * g2);
      if ((double)scale * (double)P > 32767.0 * (double)C) scale = __uint_as_float(__float_as_uint(scale) - 1u);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<float*>(p.rep)[lim_o_trim(p.rcap) + b] = trim;
    if (flags & LOUD_SHAPED) reinterpret_cast<float*>(p.ctl)[ldc_o_report(p.gcap) + ld_o_scale(p.gcap) + b] = scale;
  }
  if (t >= L) return;
  float v = p.z[(long)b * p.z_bs + t] * scale;
  v = fminf(fmaxf(v, lo), hi);
  p.pcm[(long)b * p.p_bs + t] = (short)v;
  if (p.host) {
    long off = 0;
    for (int u = 0; u < b; ++u) off += (long)p.lens[u] * p.len_mul;
    p.host[off + t] = (short)v;
  }
}

}  // namespace pe
