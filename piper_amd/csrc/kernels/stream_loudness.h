// Target loudness of streams (pe_set_stream_loudness, mode PE_GAIN_LOUDNESS): the running ITU-R BS.1770-4 gated loudness
// of what a stream has delivered so far, carried on the device from chunk to chunk, and from it every chunk's gain toward a
// target under a peak ceiling. (gfx950 / CDNA4 device code; the arithmetic is DESIGN.md 4.9. The filter, the segments and
// the gates are those of loudness.h; the conversion is chunk_pcm_gain_kernel / chunk_pcm_rs_gain_kernel, unchanged.)
#pragma once
#include "../pe_rt.h"
#include "params.h"
#include "loudness.h"
#include "post.h"

#include "stream_loudness_rule.h"

namespace pe {

// Row b's chunk (SlChunkP, params.h): n samples at the returned pointer, c = the chunk's peak word.
__device__ __forceinline__ const float* sl_chunk(const SlChunkP& q, int b, int& n, float& c) {
  if (q.rows) {
    if (b >= q.rcap) { n = 0; c = 0.f; return q.x; }
    const long cnt = q.rows[rs_o_count(q.rcap) + b];
    n = (int)(cnt < 0 ? 0 : (cnt > q.y_cap ? q.y_cap : cnt));
    c = __uint_as_float(reinterpret_cast<const unsigned*>(q.rows)[rs_o_peak(q.rcap) + b]);
    return q.x + (long)b * q.x_bs;
  }
  int first;
  chunk_range(q.st, q.cap, b, q.hop, first, n);
  c = __uint_as_float(reinterpret_cast<const unsigned*>(q.st)[sb_o_peak(q.cap) + b]);
  return q.x + (long)b * q.x_bs + first;
}

// Stream sample i of a row whose chunk starts at stream sample N: the chunk's floats from N on, the resident tail (the W
// floats in front of N, tail[k] = X[N - W + k]) below. The callers never ask outside [max(0, N - W), N + n).
__device__ __forceinline__ float sl_sample(const float* chunk, const float* tail, int N, int W, int i) {
  return i >= N ? chunk[i - N] : tail[i - (N - W)];
}

// Segment sums of the stream's K-weighted samples, added to across chunks. grid = (segments a chunk can touch, rows): the
// workgroup q of row b owns STREAM segment j = N / h + q, N = the samples the row's stream delivered before this chunk (0
// when the control block marks the row `first`), and filters the part [lo, e) of [j h, (j + 1) h) that lies in this chunk
// [N, N + n), from zero state at max(0, lo - W): what lies in front of the chunk comes from the row's tail, so the filter
// runs through chunk boundaries to the accuracy loudness_seg_kernel has inside a row. The body is that kernel's (runs, scan,
// fixed tree); the span is at most h + W, so its R holds here too. A segment that began in an earlier chunk (lo > j h) is
// added to, one that begins here is overwritten: a join needs no clearing, and one workgroup writes any (row, segment).
// Workgroup 0 of a row with n > 0 also writes the row's NEXT tail, the last W floats of the stream up to N + n, into the other
// of the two tail buffers (parity word in the state block; stream_loudness_gain_kernel flips it) -- a chunk shorter than W
// shifts the old tail. Nothing of the state is written when n == 0.
__global__ __launch_bounds__(LOUD_TPB) void stream_loudness_seg_kernel(SlP p, SlChunkP cq) {
  PE_KTRACE(40);
  __shared__ double sv[2][LOUD_TPB][4];
  __shared__ double red[LOUD_TPB];
  const int b = blockIdx.y, q = blockIdx.x, t = threadIdx.x;
  if (b >= p.cap) return;
  int n;
  float cpk;
  const float* chunk = sl_chunk(cq, b, n, cpk);
  if (n <= 0) return;
  const bool first = p.ctl[slc_o_first(p.cap) + b] != 0;
  int N = first ? 0 : p.dev[sld_o_n(p.cap) + b];
  N = N < 0 ? 0 : N;
  const int par = first ? 0 : (p.dev[sld_o_par(p.cap) + b] & 1);
  const int W = p.W;
  const float* tail = p.tail + ((long)b * 2 + par) * W;
  if (q == 0) {
    float* nt = p.tail + ((long)b * 2 + (par ^ 1)) * W;
    const int end = N + n;
    for (int k = t; k < W; k += LOUD_TPB) {
      const int i = end - W + k;
      // (below stream sample 0, or below what the old tail holds: never read, kept defined)
      nt[k] = (i >= 0 && i >= N - W) ? sl_sample(chunk, tail, N, W, i) : 0.f;
    }
  }
  const long jl = (long)(N / p.h) + q;
  if (jl >= p.nseg_cap) return;
  const int j = (int)jl;
  const long s0l = jl * p.h;
  if (s0l >= (long)N + n) return;
  const int s0 = (int)s0l;
  const int lo = s0 > N ? s0 : N;
  const int e = (long)N + n - s0 < p.h ? N + n : s0 + p.h;
  int start = lo > W ? lo - W : 0;
  if (start < N - W) start = N - W;            // (lo >= N: never taken; the tail holds nothing older)
  const int r0 = start + t * p.R < e ? start + t * p.R : e;
  const int r1 = e - r0 < p.R ? e : r0 + p.R;
  double c[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) c[k] = p.coef[k];
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = r0; i < r1; ++i) loud_step(c, (double)sl_sample(chunk, tail, N, W, i), z);
#pragma unroll
  for (int k = 0; k < 4; ++k) sv[0][t][k] = z[k];
  __syncthreads();
  for (int k = 0; k < LOUD_LEVELS; ++k) {
    const int d = 1 << k, cur = k & 1;
    double own[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) own[u] = sv[cur][t][u];
    if (t >= d) {
      const double* m = p.coef + 10 + 16 * k;
      double o[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = sv[cur][t - d][u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        own[u] += fma(m[4 * u + 3], o[3], fma(m[4 * u + 2], o[2], fma(m[4 * u + 1], o[1], m[4 * u] * o[0])));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) sv[cur ^ 1][t][u] = own[u];
    __syncthreads();
  }
  double acc = 0.0;
  if (r1 > lo && r1 > r0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) z[u] = t > 0 ? sv[0][t - 1][u] : 0.0;
    for (int i = r0; i < r1; ++i) {
      const double y = loud_step(c, (double)sl_sample(chunk, tail, N, W, i), z);
      if (i >= lo) acc = fma(y, y, acc);
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int o = LOUD_TPB / 2; o >= 1; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) {
    double* s = p.seg + (long)b * p.nseg_cap + j;
    *s = lo > s0 ? *s + red[0] : red[0];
  }
}

// The running loudness and the chunk's gain of every row; grid = rows, one wave each. loudness_gain_kernel's block walk and
// both gates over the segments of the prefix [0, N + n) -- SHORT below 4 h -- then sl_rule. The setting {T, C, prior, R0} and
// the row's `first` flag are read in place from the pinned control block; {r, G, N, last Lu, tail parity} move in the device
// block; {g0, g1, R} go to the sgd_* words the conversions read; {L, g1, r', flags, g0, R} into the control block's report.
// A row with n == 0 moves nothing: its report words keep what its last chunk wrote (a `first` row: -inf, 0, 0, UNMEASURABLE),
// and its sgd_* words are left as they are (the conversion returns at once on an empty chunk).
// limrep (the look-ahead limiter on streams, stream_limiter.h; null: off): the rule runs with its `lim` flag, and the row's two
// report words are cleared for stream_limiter_kernel, whatever n is.
__global__ __launch_bounds__(64) void stream_loudness_gain_kernel(SlP p, SlChunkP cq, int* gq, int* limrep) {
  PE_KTRACE(41);
  __shared__ double ps[64];
  __shared__ int pc[64];
  __shared__ double gate;
  const int b = blockIdx.x, t = threadIdx.x;
  if (b >= p.cap) return;
  int n;
  float cpk;
  (void)sl_chunk(cq, b, n, cpk);
  const bool first = p.ctl[slc_o_first(p.cap) + b] != 0;
  float* rf = reinterpret_cast<float*>(p.ctl);
  if (limrep && t == 0) {
    limrep[lim_o_maxred(p.cap) + b] = 0;
    limrep[lim_o_count(p.cap) + b] = 0;
  }
  if (n <= 0) {
    if (first && t == 0) {
      rf[slc_o_lufs(p.cap) + b] = -__builtin_inff();
      rf[slc_o_gain(p.cap) + b] = 0.f;
      rf[slc_o_peak(p.cap) + b] = 0.f;
      p.ctl[slc_o_flags(p.cap) + b] = LOUD_SHORT | LOUD_UNMEASURABLE;
      rf[slc_o_g0(p.cap) + b] = 0.f;
      p.ctl[slc_o_ramp(p.cap) + b] = 0;
    }
    return;
  }
  int N0 = first ? 0 : p.dev[sld_o_n(p.cap) + b];
  N0 = N0 < 0 ? 0 : N0;
  const long Nl = (long)N0 + n;
  const int N = (int)(Nl > (long)p.nseg_cap * p.h ? (long)p.nseg_cap * p.h : Nl);      // (what the segment block can hold)
  const int h = p.h;
  const double* s = p.seg + (long)b * p.nseg_cap;
  const bool is_short = N < 4 * h;
  int nseg = (N + h - 1) / h;
  nseg = nseg > p.nseg_cap ? p.nseg_cap : nseg;
  const int nb = is_short ? 0 : (N / h - 3 < nseg - 3 ? N / h - 3 : nseg - 3);
  const double inv = 1.0 / (4.0 * (double)h);
  double L = 0.0;
  bool ok = false;
  if (is_short) {
    if (t == 0) {
      double sum = 0.0;
      for (int j = 0; j < nseg; ++j) sum += s[j];
      L = -0.691 + 10.0 * log10(sum / (double)N);
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
        for (int u = 0; u < 64; ++u) { tot += ps[u]; ct += pc[u]; }
        ok = ct > 0;
        L = ok ? -0.691 + 10.0 * log10(tot / (double)ct) : 0.0;
        gate = ok ? L - 10.0 : 1.0e300;                  // (nothing passed: the second pass keeps nothing either)
      }
      __syncthreads();
    }
  }
  if (t != 0) return;
  const float T = rf[0], C = rf[1], prior = rf[2];
  int R0 = p.ctl[3];
  R0 = R0 < 0 ? 0 : (R0 > GAIN_MAX_RAMP ? GAIN_MAX_RAMP : R0);
  float* df = reinterpret_cast<float*>(p.dev);
  const float r = first ? 0.f : df[sld_o_r(p.cap) + b];
  const float rp = fmaxf(r >= 0.f ? r : 0.f, cpk);
  float lu = first ? __builtin_nanf("") : df[sld_o_lu(p.cap) + b];
  const float G = first ? 0.f : df[sld_o_g(p.cap) + b];
  const SlRule o = sl_rule(ok, is_short, L, T, C, prior, rp, G, first, lu, limrep != nullptr);
  const int R = R0 < n ? R0 : n;
  df[sld_o_r(p.cap) + b] = rp;
  df[sld_o_g(p.cap) + b] = o.g1;
  p.dev[sld_o_n(p.cap) + b] = (int)(Nl > 0x7fffffffL ? 0x7fffffffL : Nl);
  df[sld_o_lu(p.cap) + b] = lu;
  p.dev[sld_o_par(p.cap) + b] = first ? 1 : ((p.dev[sld_o_par(p.cap) + b] & 1) ^ 1);
  float* gf = reinterpret_cast<float*>(gq);
  gf[sgd_o_g0(p.cap) + b] = o.g0;
  gf[sgd_o_g1(p.cap) + b] = o.g1;
  gq[sgd_o_ramp(p.cap) + b] = R;
  rf[slc_o_lufs(p.cap) + b] = ok ? (float)L : -__builtin_inff();
  rf[slc_o_gain(p.cap) + b] = o.g1;
  rf[slc_o_peak(p.cap) + b] = rp;
  p.ctl[slc_o_flags(p.cap) + b] = o.flags;
  rf[slc_o_g0(p.cap) + b] = o.g0;
  p.ctl[slc_o_ramp(p.cap) + b] = R;
}

}  // namespace pe
