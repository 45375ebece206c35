// Timing plan: per-id rates, forced durations and a target frame count, in the place of duration_kernel.
// (gfx950 / CDNA4 device code; beyond the reference, which only knows one length_scale per utterance.)
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {

static constexpr int PLAN_MAXPER = 32;        // ids per thread: 8192 ids / 256 threads

// Sum of v over the 256 threads of the workgroup, the same value in every thread. sh: 272 words of LDS, free again on return.
__device__ __forceinline__ long long plan_block_sum(long long v, long long* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  if (tid < 16) {
    long long s = 0;
    for (int i = 0; i < 16; ++i) s += sh[tid * 16 + i];
    sh[256 + tid] = s;
  }
  __syncthreads();
  long long s = 0;
  for (int i = 0; i < 16; ++i) s += sh[256 + i];
  __syncthreads();
  return s;
}

// One workgroup per utterance, ids dealt to the threads as in duration_kernel (thread t owns ids [t * per, t * per + per)).
//   w_i = (exp(logw_i) * length_scale) * rate_i                                  (f32, in this order)
//   no target:  d_i = forced_i >= 0 ? forced_i : clamp(ceil(w_i), 0, 1e6)        (duration_kernel's rule)
//   target N:   forced ids keep forced_i; the n free ids get one frame each and share R = N - sum(forced) - n more by
//               largest remainder on the integer weights q_i = w_i > 0 ? max(1, (int64)(min(w_i, 1e6) * 2^20)) : 1:
//               a_i = q_i R / Q, r_i = q_i R % Q (Q = sum q_i), L = R - sum a_i; the L ids with the largest r_i -- ties to
//               the lower index -- get one more. sum d_i == N.
// The L-th largest remainder is found by a search over its bits from the top one of Q down: one count over the workgroup
// per bit (wave shuffles + four LDS words), so the cost is O(T / 256 * bits(Q)), not O(T^2). The remainders stay in
// registers (PLAN_MAXPER per thread, loops unrolled). Then cum / frames / frames_host / frames_clamped by duration_kernel's
// protocol: 64-bit running sums, clamped to MAX_FRAMES + 1, frames = max(sum, 1).
// p.d.z0 == null: the duration predictor did not run -- every id is forced (the host checked it), nothing reads logw.
__global__ __launch_bounds__(256) void duration_plan_kernel(PlanP p) {
  PE_KTRACE(32);
  __shared__ long long sh[272];
  __shared__ int wcnt[2][4];
  const DurP& d = p.d;
  const int b = blockIdx.x;
  const int T = d.lens[b], tid = threadIdx.x;
  const int per = (T + 255) / 256;
  const int lo = tid * per < T ? tid * per : T, hi = (lo + per < T) ? lo + per : T;
  const float* rate = p.rate + (long)b * p.pl_bs;
  const int* forced = p.forced + (long)b * p.pl_bs;
  const int N = p.target[b];
  int* dur = d.dur + (long)b * d.d_bs;

  // ---- phase 1: w, q, the forced and the plain durations
  long long q[PLAN_MAXPER];
  long long sq = 0, sf = 0, nfree = 0;
  if (d.z0) {
    const float length_scale = d.scales[3 * b + 1];
#pragma unroll
    for (int k = 0; k < PLAN_MAXPER; ++k) {
      const int t = lo + k;
      q[k] = -1;                               // -1: not a free id of this thread
      if (t < hi) {
        const float zv = d.z0[(long)b * d.z_bs + t];
        const float logw = (zv - d.m0) * d.es0;
        const float w = (expf(logw) * length_scale) * rate[t];
        if (d.logw_out) d.logw_out[(long)b * d.d_bs + t] = logw;
        if (p.w_out) p.w_out[(long)b * d.d_bs + t] = w;
        const int fv = forced[t];
        int dv;
        if (fv >= 0) {
          dv = fv;
          sf += fv;
        } else {
          float c = ceilf(w);
          c = c < 0.f ? 0.f : (c > 1.0e6f ? 1.0e6f : c);
          dv = (int)c;
          long long qi = 1;
          if (w > 0.f) {
            qi = (long long)((w < 1.0e6f ? w : 1.0e6f) * 1048576.f);
            if (qi < 1) qi = 1;
          }
          q[k] = qi;
          sq += qi;
          ++nfree;
        }
        dur[t] = dv;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PLAN_MAXPER; ++k) {
      const int t = lo + k;
      q[k] = -1;
      if (t < hi) {
        const int fv = forced[t];
        dur[t] = fv > 0 ? fv : 0;
        sf += fv > 0 ? fv : 0;
      }
    }
  }

  // ---- phase 2: a target shares its frames among the free ids
  if (N > 0) {                                 // (uniform: one utterance per workgroup)
    const long long Q = plan_block_sum(sq, sh);
    const long long F = plan_block_sum(sf, sh);
    const long long n = plan_block_sum(nfree, sh);
    long long R = (long long)N - F - n;
    if (R < 0) R = 0;                          // (the host refused such a plan)
    if (n > 0) {
      long long sa = 0;
#pragma unroll
      for (int k = 0; k < PLAN_MAXPER; ++k)
        if (q[k] >= 0) {
          const long long m = q[k] * R;        // q < 2^40, R < 2^16
          const long long a = m / Q;
          dur[lo + k] = 1 + (int)a;
          sa += a;
          q[k] = m - a * Q;                    // from here on: the remainder r
        }
      const long long Lx = R - plan_block_sum(sa, sh);      // 0 <= Lx < n
      if (Lx > 0) {
        // the Lx-th largest remainder v: the largest value with count(r >= v) >= Lx, built bit by bit (r < Q)
        int top = 0;
        while (top < 62 && (Q >> (top + 1)) != 0) ++top;
        long long v = 0;
        int step = 0;
        for (int bit = top; bit >= 0; --bit, ++step) {
          const long long cand = v | (1LL << bit);
          int c = 0;
#pragma unroll
          for (int k = 0; k < PLAN_MAXPER; ++k) c += q[k] >= cand ? 1 : 0;
          for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
          // two sets of wave words used in turn: a wave that runs ahead writes the other set, and cannot get two steps
          // ahead because the next barrier waits for everybody
          if ((tid & 63) == 0) wcnt[step & 1][tid >> 6] = c;
          __syncthreads();
          const int tot = wcnt[step & 1][0] + wcnt[step & 1][1] + wcnt[step & 1][2] + wcnt[step & 1][3];
          if (tot >= Lx) v = cand;
        }
        // every r > v gets a frame; the rest of the Lx go to the ids with r == v, lowest index first
        int cg = 0, ce = 0;
#pragma unroll
        for (int k = 0; k < PLAN_MAXPER; ++k) { cg += q[k] > v ? 1 : 0; ce += q[k] == v ? 1 : 0; }
        __syncthreads();                       // (the last step's wcnt reads are done; sh is free)
        sh[tid] = ((long long)cg << 32) | (long long)ce;
        __syncthreads();
        long long G = 0, before = 0;           // r > v in the workgroup; r == v in the threads in front of this one
        for (int i = 0; i < 256; ++i) {
          const long long e = sh[i];
          G += e >> 32;
          if (i < tid) before += e & 0xffffffffLL;
        }
        long long left = Lx - G - before;      // extras still to hand out when this thread's first id comes up
#pragma unroll
        for (int k = 0; k < PLAN_MAXPER; ++k)
          if (q[k] >= 0) {
            if (q[k] > v) dur[lo + k] += 1;
            else if (q[k] == v) {
              if (left > 0) dur[lo + k] += 1;
              --left;
            }
          }
      }
    }
  }

  // ---- phase 3: the running sum of the durations, duration_kernel's protocol
  long long s = 0;
  for (int t = lo; t < hi; ++t) s += dur[t];
  __syncthreads();
  sh[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 256; ++i) { const long long v = sh[i]; sh[i] = run; run += v; }
    const int f = run < 1 ? 1 : (run > MAX_FRAMES ? MAX_FRAMES + 1 : (int)run);
    d.frames[b] = f;
    if (d.frames_host) d.frames_host[b] = f;
    d.frames_clamped[b] = f < d.frame_cap ? f : d.frame_cap;
  }
  __syncthreads();
  long long run = sh[tid];
  int* cum = d.cum + (long)b * d.d_bs;
  for (int t = lo; t < hi; ++t) {
    run += dur[t];
    cum[t] = run > MAX_FRAMES ? MAX_FRAMES + 1 : (int)run;
  }
}

}  // namespace pe
