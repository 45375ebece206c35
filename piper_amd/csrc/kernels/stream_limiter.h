// Look-ahead limiter on streams at a target loudness (pe_set_stream_limiter, mode PE_GAIN_LOUDNESS): the conversion of a chunk
// call when the limiter is on, in chunk_pcm_gain_kernel's / chunk_pcm_rs_gain_kernel's place. (gfx950 / CDNA4 device code; the
// arithmetic is DESIGN.md 4.9.1, the envelope is limiter.h's, the sample source stream_loudness.h's.)
#pragma once
#include "../pe_rt.h"
#include "params.h"
#include "limiter.h"
#include "stream_loudness.h"
#include "stream_limiter_rule.h"

namespace pe {

// With X the stream's floats, s its per-sample scales (step 7 of 4.9 from every chunk's {g0, g1, R}), C the ceiling, W the window:
//   r[i] = min(1, C / (g_i |X_i|)), g_i = (float)((double)s_i / 32767); 1 where X_i = 0 and outside the stream
//   m, d, e as limiter_kernel's;  pcm_i = trunc(clamp((X_i e_i) s_i, +-floor(32767 C)))
// e[i] depends on r[i - 2 W .. i + 2 W] only, so a stream that holds back D = 2 W samples hands out exactly the envelope of the
// whole stream: this call delivers the stream samples [b0, b0 + cnt) of row b (the host's limiter control block), which end
// D short of the chunk's end N + n unless the row has ended, and reach back to b0 - 2 W >= N - 4 W. grid = (tiles of LIM_TILE
// samples of the delivered range, rows). Stream sample i comes from the chunk where i >= N, below it from the row's float tail
// (the buffer the seg kernel READ: the gain kernel has flipped the parity word since) and its scale from the scale tail of the
// same parity; beyond N + n and below 0 r is 1. The tile and 2 W of halo a side are staged into LDS as x, s and r; a tile
// whose span holds no r < 1 converts with e = 1, every other one goes through the doubling sliding minimum and the taps of
// limiter.h (lim_window_d, lim_env_at), so e is a function of the stream index alone -- whatever the chunking. LDS: three
// spans and the weights, 51.6 KB static, as limiter_kernel (the tile's scales wait in registers while the third span turns
// from s into m).
// Workgroup 0 of a row with n > 0 writes the row's NEXT scale tail, the scales of the stream's last SLM_TAIL samples up to
// N + n, into the buffer of the new parity, whether or not the call delivers anything for the row. The report -- the largest
// 1 - e and the count of e < 1 over what was delivered -- goes out with one atomicMax / atomicAdd per workgroup into the words
// stream_loudness_gain_kernel cleared.
__global__ __launch_bounds__(256) void stream_limiter_kernel(SlmP p, SlChunkP cq) {
  PE_KTRACE(42);
  __shared__ float xs[LIM_SPAN];
  __shared__ float rs[LIM_SPAN];
  __shared__ float ms[LIM_SPAN];
  __shared__ float hs[2 * LIM_MAXW + 1];
  __shared__ float wred[4];
  __shared__ int wcnt[4];
  __shared__ int s_any;
  const int b = blockIdx.y, tid = threadIdx.x;
  if (b >= p.cap) return;
  int n;
  float cpk;
  const float* chunk = sl_chunk(cq, b, n, cpk);
  if (n <= 0) return;                                    // (nothing moved: nothing is delivered either)
  int N = p.mctl[b];
  N = N < 0 ? 0 : N;
  const int par = p.ldev[sld_o_par(p.cap) + b] & 1;      // the NEW parity: the old tails lie in the other buffers
  const int TW = p.TW;
  const float* tail = p.tail + ((long)b * 2 + (par ^ 1)) * TW;
  const float* st_old = p.stail + ((long)b * 2 + (par ^ 1)) * SLM_TAIL;
  const float g1 = __uint_as_float(reinterpret_cast<const unsigned*>(p.gq)[sgd_o_g1(p.cap) + b]);
  const float dg = __uint_as_float(reinterpret_cast<const unsigned*>(p.gq)[sgd_o_g0(p.cap) + b]) - g1;
  int R = p.gq[sgd_o_ramp(p.cap) + b];
  R = R < 0 ? 0 : (R > n ? n : R);
  const float Rf = (float)(R > 0 ? R : 1);
  const long endl = (long)N + n;
  const int end = (int)(endl > 0x7fffffffL ? 0x7fffffffL : endl);
  // the scale of stream sample i in [max(0, N - SLM_TAIL), end)
  auto scale_at = [&](int i) -> float { return i >= N ? slm_scale_at(g1, dg, R, Rf, i - N) : st_old[i - (N - SLM_TAIL)]; };
  if (blockIdx.x == 0) {
    float* st_new = p.stail + ((long)b * 2 + par) * SLM_TAIL;
    for (int k = tid; k < SLM_TAIL; k += 256) {
      const int i = end - SLM_TAIL + k;
      // (below stream sample 0, or below what the old tail holds: never read, kept defined)
      st_new[k] = (i >= 0 && i >= N - SLM_TAIL) ? scale_at(i) : 0.f;
    }
  }
  const int b0h = p.mctl[slm_o_b0(p.cap) + b];
  int b0 = b0h, cnt = p.mctl[slm_o_cnt(p.cap) + b];
  const int W = p.W < 1 ? 1 : (p.W > LIM_MAXW ? LIM_MAXW : p.W);
  // (what the tails and the chunk can serve: the host's ranges lie inside it)
  const int reach = TW < SLM_TAIL ? TW : SLM_TAIL;
  const int lo_ok = N - reach + 2 * W > 0 ? N - reach + 2 * W : 0;
  if (b0 < lo_ok) { cnt -= lo_ok - b0; b0 = lo_ok; }
  if (cnt > end - b0) cnt = end - b0;
  const long t0l = (long)b0 + (long)blockIdx.x * LIM_TILE;
  if (cnt <= 0 || t0l >= (long)b0 + cnt) return;
  const int t0 = (int)t0l;
  const int nt = b0 + cnt - t0 < LIM_TILE ? b0 + cnt - t0 : LIM_TILE;
  const float C = __uint_as_float(reinterpret_cast<const unsigned*>(p.lctl)[1]);
  const float cqv = (float)floor(32767.0 * (double)C);
  const int r0 = t0 - 2 * W, span = nt + 4 * W;          // <= LIM_TILE + 4 LIM_MAXW < LIM_SPAN
  if (tid == 0) s_any = 0;
  __syncthreads();
  // x and r over the span; ms carries the scales until r takes its place (the scales of the tile are read back first)
  for (int q = tid; q < span; q += 256) {
    const int i = r0 + q;
    float x = 0.f, s = 0.f, r = 1.0f;
    if (i >= 0 && i < end) {
      x = sl_sample(chunk, tail, N, TW, i);
      s = scale_at(i);
      r = slm_r(x, s, C);
    }
    xs[q] = x;
    rs[q] = r;
    ms[q] = s;
    if (r < 1.0f) s_any = 1;
  }
  for (int q = tid; q < 2 * W + 1; q += 256) hs[q] = p.h[q];
  __syncthreads();
  const bool shaped = s_any != 0;
  float sc[LIM_TILE / 256];
#pragma unroll
  for (int j = 0; j < LIM_TILE / 256; ++j) {
    const int i = tid + 256 * j;
    sc[j] = i < nt ? ms[2 * W + i] : 0.f;
  }
  __syncthreads();
  if (shaped) {
    for (int q = tid; q < span; q += 256) ms[q] = rs[q];
    __syncthreads();
    lim_window_d(ms, span, W, tid);
  }
  const long off = reinterpret_cast<const long long*>(p.st + sb_o_off(p.cap))[b] + (t0 - b0h);
  short* pcm = reinterpret_cast<short* const*>(p.st + sb_o_ptrs(p.cap))[0] + off;
  float* fout = reinterpret_cast<float* const*>(p.st + sb_o_ptrs(p.cap))[1];
  float red = 0.f;
  int c = 0;
#pragma unroll
  for (int j = 0; j < LIM_TILE / 256; ++j) {
    const int i = tid + 256 * j;
    if (i < nt) {
      const int q = 2 * W + i;
      const float e = shaped ? lim_env_at(ms, rs, hs, q, W) : 1.0f;
      const float x = xs[q];
      pcm[i] = slm_pcm(x, e, sc[j], cqv);
      if (fout) fout[off + i] = x;
      if (p.env) p.env[(long)b * p.e_bs + t0 + i] = e;
      red = fmaxf(red, 1.0f - e);
      c += e < 1.0f ? 1 : 0;
    }
  }
  if (!shaped) return;
  for (int o = 32; o >= 1; o >>= 1) {
    red = fmaxf(red, __shfl_xor(red, o));
    c += __shfl_xor(c, o);
  }
  if ((tid & 63) == 0) { wred[tid >> 6] = red; wcnt[tid >> 6] = c; }
  __syncthreads();
  if (tid == 0) {
    atomicMax(reinterpret_cast<unsigned*>(p.rep) + lim_o_maxred(p.cap) + b,
              __float_as_uint(fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]))));
    atomicAdd(p.rep + lim_o_count(p.cap) + b, wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]);
  }
}

}  // namespace pe
