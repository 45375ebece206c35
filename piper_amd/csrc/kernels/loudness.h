// Target loudness of whole utterances: ITU-R BS.1770-4 gated integrated loudness (mono) of the float waveform a call
// delivers, and from it the scale of the int16 conversion. (gfx950 / CDNA4 device code. The reference has no such stage:
// its rule is the peak rule of pcm16_kernel, src/cpp/piper.cpp:410-431. The arithmetic is DESIGN.md 4.6.)
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// One sample through the K-weighting cascade, both biquads in the transposed direct form II on f64 states
// z = {shelf s1, shelf s2, high-pass s1, high-pass s2}: y = b0 x + s1, s1' = b1 x - a1 y + s2, s2' = b2 x - a2 y.
__device__ __forceinline__ double loud_step(const double (&c)[10], double x, double (&z)[4]) {
  const double ya = fma(c[0], x, z[0]);
  z[0] = fma(-c[3], ya, fma(c[1], x, z[1]));
  z[1] = fma(-c[4], ya, c[2] * x);
  const double yb = fma(c[5], ya, z[2]);
  z[2] = fma(-c[8], yb, fma(c[6], ya, z[3]));
  z[3] = fma(-c[9], yb, c[7] * ya);
  return yb;
}

// Segment sums s_j = sum of y^2 over [j h, (j + 1) h) cut to the row, y = the K-weighted row. grid = (segments of the
// bucket, rows), one workgroup per 100 ms segment; a workgroup whose segment starts behind the row's end returns.
// The workgroup filters [max(0, j h - W), segment end): W samples of warm-up from zero state stand for the row's past
// (the slowest pole pair, the 38 Hz high-pass, has decayed below 1e-4 of its start by then; a segment that starts within
// W of sample 0 is exact). That span is cut into LOUD_TPB runs of R samples, one per thread, so nobody walks more than
// 2 R samples (58 at 48000 Hz) however long the utterance is:
//   1. every thread filters its run from ZERO state: v_t = the four states behind it;
//   2. the states the runs really start from follow from v by linearity, in_(t+1) = A^R in_t + v_t: an inclusive scan over
//      the threads in LOUD_LEVELS doubling steps through LDS, step k adding A^(R 2^k) times the value 2^k threads below
//      (the matrices come from the host in f64);
//   3. the threads whose runs reach into the segment filter them again from the right state and sum y^2.
// The partial sums meet in LDS and are added as a fixed tree: no floating-point atomics, a run repeats bit for bit.
// Samples outside [0, n) read as zero through the row descriptor.
__global__ __launch_bounds__(LOUD_TPB) void loudness_seg_kernel(LoudP p) {
  PE_KTRACE(32);
  __shared__ double sv[2][LOUD_TPB][4];
  __shared__ double red[LOUD_TPB];
  const int b = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
  // (true-peak ceiling: the row's word is cleared here, stream-ordered before true_peak_kernel folds into it)
  if (p.tpeak && j == 0 && t == 0) p.tpeak[b] = 0u;
  // (limiter: so are the row's report words, before limiter_kernel folds into them)
  if (p.limrep && j == 0 && t == 0 && b < p.limcap) {
    p.limrep[lim_o_maxred(p.limcap) + b] = 0; p.limrep[lim_o_count(p.limcap) + b] = 0;
    p.limrep[lim_o_pz(p.limcap) + b] = 0; p.limrep[lim_o_tz(p.limcap) + b] = 0;
    reinterpret_cast<float*>(p.limrep)[lim_o_trim(p.limcap) + b] = 1.0f;
  }
  long nl = (long)p.lens[b] * p.len_mul;
  nl = nl < 0 ? 0 : (nl > p.x_cap ? p.x_cap : nl);
  const int n = (int)nl;
  const long s0l = (long)j * p.h;
  if (s0l >= n || j >= p.nseg_cap) return;
  const int s0 = (int)s0l;
  const int e = n - s0 < p.h ? n : s0 + p.h;
  const int start = s0 > p.W ? s0 - p.W : 0;
  // (start + t R <= s0 + h + W + R: far inside an int for every row a descriptor can address)
  const int r0 = start + t * p.R < e ? start + t * p.R : e;
  const int r1 = e - r0 < p.R ? e : r0 + p.R;
  const pe_rowsrc row = pe_make_row(p.x + (long)b * p.x_bs, n);
  double c[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) c[k] = p.coef[k];
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = r0; i < r1; ++i) loud_step(c, (double)pe_row_load(row, i), z);
#pragma unroll
  for (int q = 0; q < 4; ++q) sv[0][t][q] = z[q];
  __syncthreads();
  for (int k = 0; k < LOUD_LEVELS; ++k) {
    const int d = 1 << k, cur = k & 1;
    double own[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) own[q] = sv[cur][t][q];
    if (t >= d) {
      const double* m = p.coef + 10 + 16 * k;
      double o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = sv[cur][t - d][q];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        own[q] += fma(m[4 * q + 3], o[3], fma(m[4 * q + 2], o[2], fma(m[4 * q + 1], o[1], m[4 * q] * o[0])));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) sv[cur ^ 1][t][q] = own[q];
    __syncthreads();
  }
  // (LOUD_LEVELS is even: the scanned states are back in sv[0])
  static_assert((LOUD_LEVELS & 1) == 0 && (1 << LOUD_LEVELS) == LOUD_TPB, "the scan covers the workgroup and ends in sv[0]");
  double acc = 0.0;
  if (r1 > s0 && r1 > r0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) z[q] = t > 0 ? sv[0][t - 1][q] : 0.0;
    for (int i = r0; i < r1; ++i) {
      const double y = loud_step(c, (double)pe_row_load(row, i), z);
      if (i >= s0) acc = fma(y, y, acc);
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int o = LOUD_TPB / 2; o >= 1; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) p.seg[(long)b * p.nseg_cap + j] = red[0];
}

// Blocks, gates, loudness, scale and flags of every row; grid = rows, one wave each. Block j is segments j .. j + 3
// (400 ms, 75 % overlap), z_j their mean square, l_j = -0.691 + 10 log10 z_j, for every j with (j + 4) h <= n. The lanes
// walk the blocks in steps of 64 and their partial sums are added lane 0 to 63 by one thread: a fixed order.
//   absolute gate l_j > -70; relative gate G = -0.691 + 10 log10(mean z over the absolute-gated blocks) - 10;
//   L = -0.691 + 10 log10(mean z over blocks with l_j > -70 and l_j > G).
//   n < 4 h (SHORT): one block over the whole row, mean of y^2 over n, kept when it passes the absolute gate.
//   nothing kept, or n == 0 (UNMEASURABLE): scale = 32767, L = -inf.
//   else scale = 32767 min(10^((T - L) / 20), C / P), LIMITED when the second term is the smaller; P = p, the row's
//   sample-peak word, or with a true-peak ceiling (tpeaks != null) max(p, t), t = the word of true_peak_kernel
//   (true_peak.h): phase 0 of its interpolator has gain 0.92, so t alone can read below p.
// T and C are read in place from the pinned control block `ctl`; {L, scale, p, flags} go to the device block `gd` for the
// conversion and into the control block's report for pe_last_loudness, t behind it for pe_last_true_peak. Every index is
// cut to its block. limiter != 0 (the look-ahead limiter, limiter.h): a LIMITED row is SHAPED as well and its scale is the
// first term, 32767 10^((T - L) / 20), whatever the peak is.
__global__ __launch_bounds__(64) void loudness_gain_kernel(const double* seg, int nseg_cap, const int* lens, int len_mul,
                                                           long x_cap, int h, const unsigned* peaks, const unsigned* tpeaks, int* ctl, int* gd,
                                                           int cap, int limiter) {
  PE_KTRACE(33);
  __shared__ double ps[64];
  __shared__ int pc[64];
  __shared__ double gate;
  const int b = blockIdx.x, t = threadIdx.x;
  if (b >= cap) return;
  long nl = (long)lens[b] * len_mul;
  nl = nl < 0 ? 0 : (nl > x_cap ? x_cap : nl);
  const int n = (int)nl;
  const double* s = seg + (long)b * nseg_cap;
  const bool is_short = n < 4 * h;
  int nseg = (n + h - 1) / h;                            // segments the first kernel wrote
  nseg = nseg > nseg_cap ? nseg_cap : nseg;
  const int nb = is_short ? 0 : (n / h - 3 < nseg - 3 ? n / h - 3 : nseg - 3);
  const double inv = 1.0 / (4.0 * (double)h);
  double L = 0.0;
  bool ok = false;
  if (is_short) {
    if (t == 0 && n > 0) {
      double sum = 0.0;
      for (int j = 0; j < nseg; ++j) sum += s[j];
      L = -0.691 + 10.0 * log10(sum / (double)n);
      ok = L > -70.0;
    }
  } else {
    for (int pass = 0; pass < 2; ++pass) {
      const double g = pass ? gate : -70.0;
      double sum = 0.0;
      int cnt = 0;
      for (int j = t; j < nb; j += 64) {
        const double zj = (((s[j] + s[j + 1]) + s[j + 2]) + s[j + 3]) * inv;
        const double lj = -0.691 + 10.0 * log10(zj);
        if (lj > -70.0 && lj > g) { sum += zj; ++cnt; }
      }
      ps[t] = sum;
      pc[t] = cnt;
      __syncthreads();
      if (t == 0) {
        double tot = 0.0;
        int ct = 0;
        for (int q = 0; q < 64; ++q) { tot += ps[q]; ct += pc[q]; }
        ok = ct > 0;
        L = ok ? -0.691 + 10.0 * log10(tot / (double)ct) : 0.0;
        gate = ok ? L - 10.0 : 1.0e300;                  // (nothing passed: the second pass keeps nothing either)
      }
      __syncthreads();
    }
  }
  if (t != 0) return;
  const float T = __uint_as_float(reinterpret_cast<const unsigned*>(ctl)[0]);
  const float C = __uint_as_float(reinterpret_cast<const unsigned*>(ctl)[1]);
  const float p = __uint_as_float(peaks[b]);
  const float tp = tpeaks ? __uint_as_float(tpeaks[b]) : 0.f;
  const float P = fmaxf(p, tp);
  int flags = is_short ? LOUD_SHORT : 0;
  float scale = 32767.0f, Lf = -__builtin_inff();
  if (ok && P > 0.f) {
    const double g1 = exp(((double)T - L) * 0.11512925464970228), g2 = (double)C / (double)P;      // 10^(x / 20) = e^(x ln 10 / 20)
    if (g2 < g1) flags |= LOUD_LIMITED;
    scale = (float)(32767.0 * (g2 < g1 ? g2 : g1));
    // (the rounding to f32 must not lift the row's peak over the ceiling)
    if ((flags & LOUD_LIMITED) && (double)scale * (double)P > 32767.0 * (double)C) scale = __uint_as_float(__float_as_uint(scale) - 1u);
    // (look-ahead limiter, limiter.h: the row keeps the gain of its target and limiter_kernel shapes its peaks under C)
    if (limiter && (flags & LOUD_LIMITED)) { flags |= LOUD_SHAPED; scale = (float)(32767.0 * g1); }
    Lf = (float)L;
  } else {
    flags |= LOUD_UNMEASURABLE;
  }
  float* gf = reinterpret_cast<float*>(gd);
  float* rf = reinterpret_cast<float*>(ctl + ldc_o_report(cap));
  gf[b] = Lf; rf[b] = Lf;
  gf[ld_o_scale(cap) + b] = scale; rf[ld_o_scale(cap) + b] = scale;
  gf[ld_o_peak(cap) + b] = p; rf[ld_o_peak(cap) + b] = p;
  gd[ld_o_flags(cap) + b] = flags; ctl[ldc_o_report(cap) + ld_o_flags(cap) + b] = flags;
  if (tpeaks) reinterpret_cast<float*>(ctl)[ldc_o_tpeak(cap) + b] = tp;
}

}  // namespace pe
