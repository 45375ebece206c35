// Generator tail: conv_post + tanh + peak, int16 conversion; small glue kernels.
// (gfx950 / CDNA4 device code; reference arithmetic cited per kernel, paths relative to
// /root/reference/src/python/piper_train/vits/.)
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {

// ------------------------------------------------------------------------------------------------
// Generator tail (models.py:364-366): leaky_relu(0.01) -> conv_post (k=7, no bias, 1 output channel)
// -> tanh, fused with the per-utterance max|x| that the int16 conversion needs (piper.cpp:410-418).
// HBM-bound (4*Cin bytes in, 4 out per sample), and at batch 1 a latency chain: a workgroup = 256 samples x 4 channel
// groups (one wave each); a thread owns POST_OPT consecutive samples of POST_CU channels per pass (one pass for
// Cin <= 32) and requests all its POST_CU * (POST_OPT + 6) inputs at once through row descriptors (zero padding = range
// check; neighbouring threads' overlap is served by L1). The weights are wave-uniform scalars. The channel-group
// partials meet in LDS and are summed in a fixed order; one peak atomic per workgroup. (A first version walked all channels in one thread: 8 dependent memory round
// trips and 104 workgroups for a 4.8 s utterance, 22.9 us; profiles/r02_notes.md.)
__global__ __launch_bounds__(256) void conv_post_kernel(const float* x, long x_bs, int x_cs, const float* __restrict__ w,
                                                        int Cin, float slope, const int* lens,
                                                        int len_mul, float* audio, long a_bs,
                                                        unsigned* absmax) {
  PE_KTRACE(17);
  constexpr int NIN = POST_OPT + POST_K - 1;
  __shared__ float part[POST_CG][POST_SPB];
  PE_STAMP(4, 0);
  const int b = blockIdx.y, L = lens[b] * len_mul;
  if (blockIdx.x * POST_SPB >= L) return;
  const int sg = threadIdx.x & 63, cg = PE_UNIFORM(threadIdx.x >> 6);
  const int t0 = blockIdx.x * POST_SPB + sg * POST_OPT;
  const float* xb = x + (long)b * x_bs;
  float acc[POST_OPT];
#pragma unroll
  for (int o = 0; o < POST_OPT; ++o) acc[o] = 0.f;
  for (int c0 = cg * POST_CU; c0 < Cin; c0 += POST_CG * POST_CU) {
    float v[POST_CU][NIN];
#pragma unroll
    for (int cc = 0; cc < POST_CU; ++cc) {
      const pe_rowsrc row = pe_make_row(xb + (long)(c0 + cc) * x_cs, c0 + cc < Cin ? L : 0);
#pragma unroll
      for (int j = 0; j < NIN; ++j) v[cc][j] = pe_row_load(row, t0 - (POST_K - 1) / 2 + j);
    }
#pragma unroll
    for (int cc = 0; cc < POST_CU; ++cc) {
      const float* wc = w + (c0 + cc < Cin ? c0 + cc : 0) * POST_K;
#pragma unroll
      for (int j = 0; j < NIN; ++j) v[cc][j] = pe_lrelu(v[cc][j], slope);
#pragma unroll
      for (int k = 0; k < POST_K; ++k) {
        const float wk = wc[k];
#pragma unroll
        for (int o = 0; o < POST_OPT; ++o) acc[o] = fmaf(wk, v[cc][o + k], acc[o]);   // channel-major, tap-minor
      }
    }
  }
#pragma unroll
  for (int o = 0; o < POST_OPT; ++o) part[cg][sg * POST_OPT + o] = acc[o];
  __shared__ float wmax[4];
  PE_STAMP(4, 1);
  __syncthreads();
  PE_STAMP(4, 2);
  const int t = blockIdx.x * POST_SPB + threadIdx.x;
  float sum = 0.f;
#pragma unroll
  for (int g = 0; g < POST_CG; ++g) sum += part[g][threadIdx.x];
  const float y = tanhf(sum);
  float m = 0.f;
  if (t < L) {
    audio[(long)b * a_bs + t] = y;
    m = fabsf(y);
  }
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  PE_STAMP(4, 3);
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(absmax + b, __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
  PE_STAMP(4, 4);
}

// float -> int16 exactly as piper.cpp:420-431 (scale 32767/max(0.01,peak), clamp, truncate)
// `host`: pinned host memory that also receives the samples, utterances packed back to back (zero-copy delivery), or null
// Kernel entry: the parameters arrive in SGPRs in the order the kernel needs them (the two data-dependent scalars' pointers
// first), and the block size is a constant instead of the hidden blockDim argument.
constexpr int PCM16_TPB = 256;
// GAIN (pcm16_gain_kernel, the target-loudness setting): the scale is the one loudness_gain_kernel (loudness.h) left in the
// device block `gq` (params.h: ld_*) instead of 32767 / max(0.01, peak). The default instantiation is the kernel as it was:
// nothing of the gain path is in it.
template <bool GAIN>
__device__ __forceinline__ void pcm16_body(const int* lens, int len_mul, const unsigned* absmax, const float* audio, long a_bs,
                                           short* pcm, long p_bs, short* host, const int* gq, int gcap) {
  const int b = blockIdx.y, L = lens[b] * len_mul;
  const int t = blockIdx.x * PCM16_TPB + threadIdx.x;
  if (t >= L) return;
  float scale;
  if constexpr (GAIN) {
    scale = __uint_as_float(reinterpret_cast<const unsigned*>(gq)[ld_o_scale(gcap) + b]);
  } else {
    const float peak = fmaxf(0.01f, __uint_as_float(absmax[b]));
    scale = 32767.0f / peak;
  }
  float v = audio[(long)b * a_bs + t] * scale;
  v = fminf(fmaxf(v, -32768.0f), 32767.0f);
  pcm[(long)b * p_bs + t] = (short)v;
  if (host) {
    // the utterances are packed back to back in the host buffer, as pe_result.sample_offsets describes them
    long off = 0;
    for (int u = 0; u < b; ++u) off += (long)lens[u] * len_mul;
    host[off + t] = (short)v;
  }
}
__global__ __launch_bounds__(PCM16_TPB) void pcm16_kernel(const int* lens, int len_mul, const unsigned* absmax, const float* audio,
                                                          long a_bs, short* pcm, long p_bs, short* host) {
  PE_KTRACE(18);
  pcm16_body<false>(lens, len_mul, absmax, audio, a_bs, pcm, p_bs, host, nullptr, 0);
}
__global__ __launch_bounds__(PCM16_TPB) void pcm16_gain_kernel(const int* lens, int len_mul, const int* gq, int gcap, const float* audio,
                                                               long a_bs, short* pcm, long p_bs, short* host) {
  PE_KTRACE(34);
  pcm16_body<true>(lens, len_mul, nullptr, audio, a_bs, pcm, p_bs, host, gq, gcap);
}

// Streaming decode: copy frames [win[0], win[0]+win[1]) of z [C][zs] into the window buffer [C][ws]
// (window bounds live in device memory so one captured graph serves every chunk).
__global__ void window_copy_kernel(const float* z, int zs, const int* win, float* out, int ws, int C) {
  const int c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C && t < win[1]) out[(long)c * ws + t] = z[(long)c * zs + win[0] + t];
}

// Batch streaming (pe_stream_next_batch), first launch of the window stage: frames [start_b, start_b + len_b) of z[b] into
// window buffer [b]; grid = (64-frame tiles over the window bucket `wg`, channels, utterances). Columns [len_b, wg) are
// zeroed: the buffer held other data before (the prior noise), and not every consumer of the generator's input masks by
// `lens` before it multiplies. The window bounds come from the pinned host block `hst` (params.h: sb_*), cut to the row so
// that nothing outside z[b] is ever read; workgroup (0, 0, b) publishes utterance b's state to the device block `dst` and
// clears its chunk peak there.
__global__ void window_gather_kernel(const float* z, long z_bs, int zs, const int* hst, int* dst, int cap, float* out,
                                     long o_bs, int ws, int wg) {
  PE_KTRACE(23);
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  int start = hst[b], len = hst[sb_o_len(cap) + b];
  start = start < 0 ? 0 : (start > zs ? zs : start);
  const int room = zs - start < wg ? zs - start : wg;
  len = len < 0 ? 0 : (len > room ? room : len);
  if (blockIdx.x == 0 && c == 0 && threadIdx.x == 0) {
    dst[b] = start;
    dst[sb_o_len(cap) + b] = len;
    dst[sb_o_first(cap) + b] = hst[sb_o_first(cap) + b];
    dst[sb_o_count(cap) + b] = hst[sb_o_count(cap) + b];
    dst[sb_o_off(cap) + 2 * b] = hst[sb_o_off(cap) + 2 * b];
    dst[sb_o_off(cap) + 2 * b + 1] = hst[sb_o_off(cap) + 2 * b + 1];
    dst[sb_o_peak(cap) + b] = 0;
    if (b == 0)
      for (int k = 0; k < 4; ++k) dst[sb_o_ptrs(cap) + k] = hst[sb_o_ptrs(cap) + k];
  }
  if (t >= wg || t >= ws) return;
  out[(long)b * o_bs + (long)c * ws + t] = t < len ? z[(long)b * z_bs + (long)c * zs + start + t] : 0.f;
}

// Chunk delivery of a batch stream, two launches over grid = (steps of CHUNK_SPB samples, utterances): the chunk is samples
// [first_b, first_b + count_b) of utterance b's window waveform -- the window minus its halo, so conv_post_kernel's peak
// (which covers the halo) is not the chunk's. A workgroup walks its steps (the chunk length is the caller's), and a
// finished utterance (count 0) costs an early return.
// 1. max |sample| over the chunk: one atomicMax on the float's bit pattern per workgroup (non-negative floats order like
//    their bit patterns; the maximum does not depend on the order of the updates).
__device__ __forceinline__ void chunk_range(const int* st, int cap, int b, int hop, int& first, int& count) {
  const int L = st[sb_o_len(cap) + b] * hop;
  first = st[sb_o_first(cap) + b];
  count = st[sb_o_count(cap) + b];
  first = first < 0 ? 0 : (first > L ? L : first);
  count = count < 0 ? 0 : (count > L - first ? L - first : count);
}
__global__ __launch_bounds__(256) void chunk_peak_kernel(const float* audio, long a_bs, int* st, int cap, int hop) {
  PE_KTRACE(24);
  __shared__ float wmax[4];
  const int b = blockIdx.y;
  int first, count;
  chunk_range(st, cap, b, hop, first, count);
  if ((long)blockIdx.x * CHUNK_SPB >= count) return;
  const float* a = audio + (long)b * a_bs + first;
  float m = 0.f;
  for (long base = (long)blockIdx.x * CHUNK_SPB; base < count; base += (long)gridDim.x * CHUNK_SPB)
#pragma unroll
    for (int j = 0; j < CHUNK_SPB / 256; ++j) {
      const long i = base + j * 256 + threadIdx.x;
      if (i < count) m = fmaxf(m, fabsf(a[i]));
    }
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<unsigned*>(st) + sb_o_peak(cap) + b,
              __float_as_uint(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
}
// 2. float -> int16 as pcm16_kernel, with the chunk's own peak (the reference's streaming script normalises every chunk
//    by itself, infer_onnx_streaming.py:122), stored packed back to back into pinned host memory at the utterance's
//    offset; the floats go next to them when the caller wants them.
//    GAIN (chunk_pcm_gain_kernel, the stream-wide levels): the scale of sample i of the chunk is g1 behind the ramp and
//    g1 + (g0 - g1) * ((R - 1 - i) / R) inside it (i < R), from the block stream_gain_kernel wrote (params.h: sgd_*). The
//    default instantiation is the kernel as it was: nothing of the gain path is in it.
template <bool GAIN>
__device__ __forceinline__ float chunk_gain_at(float g1, float dg, int R, float Rf, long i) {
  if constexpr (GAIN) {
    if (i < R) return fmaf(dg, (float)(R - 1 - (int)i) / Rf, g1);
  }
  return g1;
}
template <bool GAIN>
__device__ __forceinline__ void chunk_pcm_body(const float* audio, long a_bs, const int* st, int cap, int hop, const int* gq) {
  const int b = blockIdx.y;
  int first, count;
  chunk_range(st, cap, b, hop, first, count);
  if ((long)blockIdx.x * CHUNK_SPB >= count) return;
  const float* a = audio + (long)b * a_bs + first;
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
    const float peak = fmaxf(0.01f, __uint_as_float(reinterpret_cast<const unsigned*>(st)[sb_o_peak(cap) + b]));
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
__global__ __launch_bounds__(256) void chunk_pcm_kernel(const float* audio, long a_bs, const int* st, int cap, int hop) {
  PE_KTRACE(25);
  chunk_pcm_body<false>(audio, a_bs, st, cap, hop, nullptr);
}
__global__ __launch_bounds__(256) void chunk_pcm_gain_kernel(const float* audio, long a_bs, const int* st, int cap, int hop,
                                                             const int* gq) {
  PE_KTRACE(30);
  chunk_pcm_body<true>(audio, a_bs, st, cap, hop, gq);
}

// Stream-wide gain (pe_set_stream_gain, modes running and fixed), one thread per row, between the chunk's peak and its
// conversion. Row b's chunk has n samples and peak c: of the window state block `st` at the native rate (chunk_range,
// sb_o_peak), of the resampling row block `rows` when a rate is set (count cut to y_cap as the conversion cuts it). The
// setting's numbers and the row's "nothing delivered yet" flag come from the pinned control block `ctl`, read in place;
// the running peak r lives in the device block `gb` (params.h: sg_*, sgd_*).
//   running: first -> r = max(0.01, P). n > 0: r' = max(r, c), g1 = 32767 / r', g0 = g1 on the first chunk, else 32767 / r;
//            the chunk's ramp is R = min(R0, n) samples. n == 0: nothing moves. r never falls, so the gain never rises.
//   fixed:   g0 = g1 = 32767 / max(0.01, P), no state.
// {g0, g1, R} go to `gb` for the conversion, {g1, the level it came from} into the control block for pe_stream_last_gains
// (rows with nothing delivered: the stored state when running, 0 when fixed). Every index is cut to its block.
__global__ __launch_bounds__(64) void stream_gain_kernel(int* ctl, int* gb, int cap, int B, int mode, const int* st, int hop,
                                                         const int* rows, int rcap, long y_cap) {
  PE_KTRACE(29);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || b >= cap) return;
  int n = 0;
  float c = 0.f;
  if (rows) {
    if (b >= rcap) return;
    const long cnt = rows[rs_o_count(rcap) + b];
    n = (int)(cnt < 0 ? 0 : (cnt > y_cap ? y_cap : cnt));
    c = __uint_as_float(reinterpret_cast<const unsigned*>(rows)[rs_o_peak(rcap) + b]);
  } else {
    int first;
    chunk_range(st, cap, b, hop, first, n);
    c = __uint_as_float(reinterpret_cast<const unsigned*>(st)[sb_o_peak(cap) + b]);
  }
  const float P = __uint_as_float(reinterpret_cast<const unsigned*>(ctl)[0]);
  int R0 = ctl[1];
  R0 = R0 < 0 ? 0 : (R0 > GAIN_MAX_RAMP ? GAIN_MAX_RAMP : R0);
  float* gf = reinterpret_cast<float*>(gb);
  float* cf = reinterpret_cast<float*>(ctl);
  float g0, g1, level;
  int R = 0;
  if (mode == GAIN_FIXED) {
    level = fmaxf(0.01f, P);
    g0 = g1 = 32767.0f / level;
    cf[sg_o_rgain(cap) + b] = n > 0 ? g1 : 0.f;
    cf[sg_o_rpeak(cap) + b] = n > 0 ? level : 0.f;
  } else {
    const bool first = ctl[sg_o_first(cap) + b] != 0;
    float r = first ? fmaxf(0.01f, P) : gf[b];
    if (!(r >= 0.01f)) r = 0.01f;                        // (a row that never began: the floor, not a division by zero)
    level = n > 0 ? fmaxf(r, c) : r;
    g1 = 32767.0f / level;
    g0 = first ? g1 : 32767.0f / r;
    R = R0 < n ? R0 : n;
    gf[b] = level;
    cf[sg_o_rgain(cap) + b] = g1;
    cf[sg_o_rpeak(cap) + b] = level;
  }
  gf[sgd_o_g0(cap) + b] = g0;
  gf[sgd_o_g1(cap) + b] = g1;
  gb[sgd_o_ramp(cap) + b] = R;
}

// Stream pool (pe_stream_pool_join): the newcomers' latents move from the stage-B workspace, which the next upload
// overwrites, into the pool's resident rows; grid = (64-frame tiles over the newcomers' frame bucket, channels, newcomers).
// Newcomer j goes to row slot[j] (join block `join`, pinned host memory read in place; params.h: sj_*): frames [0, F_j) of
// z[j][c] are copied, [F_j, ps) of the pool row are zeroed -- the row is ps frames wide, whatever the bucket is, and a
// reused slot must not keep its previous tenant's tail -- so a workgroup walks from its tile in steps of the grid's width.
// Workgroups (., 0, j) also copy the newcomer's decoder conditioning row (cond null: a single-speaker voice). Slot and
// frame count are cut to the pool, so that nothing outside a row is read or written. With rows that start on 16-byte
// boundaries -- every row the engine allocates does -- and the 64 threads it is launched with, a quarter wave owns a tile
// and moves four frames per lane; anything else takes the one-frame-per-lane loop.
__global__ __launch_bounds__(64) void stream_adopt_kernel(const float* z, long z_bs, int zs, const float* cond, int cond_bs,
                                                          int cond_rows, const int* join, int cap, float* pool, long p_bs,
                                                          int ps, float* pcond, int slots) {
  PE_KTRACE(26);
  const int j = blockIdx.z, c = blockIdx.y;
  if (j >= cap || j >= join[0]) return;
  const int slot = join[sj_o_slot(cap) + j];
  if (slot < 0 || slot >= slots) return;
  int F = join[sj_o_frames(cap) + j];
  const int room = zs < ps ? zs : ps;
  F = F < 0 ? 0 : (F > room ? room : F);
  if (c == 0 && cond)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cond_rows; i += gridDim.x * blockDim.x)
      pcond[(long)slot * cond_rows + i] = cond[(long)j * cond_bs + i];
  const float* src = z + (long)j * z_bs + (long)c * zs;
  float* dst = pool + (long)slot * p_bs + (long)c * ps;
  const bool v4 = blockDim.x == 64 && ((zs | ps | (int)(z_bs & 3) | (int)(p_bs & 3)) & 3) == 0 &&
                  ((reinterpret_cast<size_t>(z) | reinterpret_cast<size_t>(pool)) & 15) == 0;
  if (v4) {
    const int q = threadIdx.x & 15, r = threadIdx.x >> 4;
    for (long tile = blockIdx.x + (long)r * gridDim.x; tile * 64 < ps; tile += 4L * gridDim.x) {
      const int t = (int)(tile * 64) + q * 4;
      if (t >= ps) continue;
      f32x4 v;
      if (t + 4 <= F) {
        v = *reinterpret_cast<const f32x4*>(src + t);
      } else {
        for (int k = 0; k < 4; ++k) v[k] = t + k < F ? src[t + k] : 0.f;
      }
      *reinterpret_cast<f32x4*>(dst + t) = v;
    }
  } else {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < ps; t += (long)gridDim.x * blockDim.x)
      dst[t] = t < F ? src[t] : 0.f;
  }
}

// MRF combine for the parallel-branch schedule: out = ((r0 + r1) + r2) * scale  (models.py:356-363)
__global__ void mrf_sum_kernel(const float* r0, const float* r1, const float* r2, float* out, long bs, int cs,
                               const int* lens, int len_mul, float scale) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lens[b] * len_mul) return;
  const long i = (long)b * bs + (long)c * cs + t;
  float v = r0[i] + r1[i];
  if (r2) v += r2[i];
  out[i] = v * scale;
}

}  // namespace pe
