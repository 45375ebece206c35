// The look-ahead limiter of a stream delivered at a target loudness, the per-sample arithmetic written once:
// for stream_limiter_kernel (stream_limiter.h) and for the one-utterance stream, whose conversion runs on the host.
#pragma once
#include <cmath>
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// The scale of sample j of a chunk with the gains {g0, g1} and a ramp of R samples (chunk_gain_at of post.h, step 7 of 4.9).
__host__ __device__ __forceinline__ float slm_scale_at(float g1, float dg, int R, float Rf, int j) {
  return j < R ? fmaf(dg, (float)(R - 1 - j) / Rf, g1) : g1;
}

// r of one sample: the gain that alone would hold it under the ceiling C at its own scale s; 1 for a zero sample.
__host__ __device__ __forceinline__ float slm_r(float x, float s, float C) {
  const float a = fabsf(x);
  const float g = (float)((double)s / 32767.0);
  return a > 0.f ? fminf(1.0f, C / (g * a)) : 1.0f;
}

// The int16 of one sample from its float, its envelope, its scale and cq = floor(32767 C).
__host__ __device__ __forceinline__ short slm_pcm(float x, float e, float s, float cq) {
  float o = (x * e) * s;
  o = fminf(fmaxf(o, -cq), cq);
  return (short)o;
}

// How far a stream has been handed out once N of its samples exist: everything when the row has ended, else all but D.
static inline long long slm_delivered(long long N, int D, bool ended) { return ended ? N : (N > D ? N - D : 0); }

// Host: e of the stream samples [lo, hi) from r over [lo - 2 W, hi + 2 W), given as rr[i - (lo - 2 W)] (1 outside the
// stream), with the f32 weights h[2 W + 1]: the arithmetic of the kernel's tile body, serial.
// (d: scratch of count + 2 W floats. Where every d of a sum is 0 the sum is 0 and r is 1: the kernel's skip gives the same e.)
static inline void slm_host_env(const float* rr, int count, int W, const float* h, float* d, float* e) {
  for (int j = 0; j < count + 2 * W; ++j) {              // d of stream sample lo - W + j: the window rr[j .. j + 2 W]
    float m = 1.0f;
    for (int u = 0; u <= 2 * W; ++u) m = fminf(m, rr[j + u]);
    d[j] = 1.0f - m;
  }
  for (int i = 0; i < count; ++i) {
    float acc = 0.f;
    for (int k = 0; k <= 2 * W; ++k) acc = fmaf(h[k], d[i + k], acc);
    e[i] = fminf(rr[i + 2 * W], 1.0f - acc);
  }
}

}  // namespace pe
