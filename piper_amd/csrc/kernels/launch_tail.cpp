// Launchers of the fused MRF stage kernel and the generator tail: one translation unit of the library build.
#include "launch.h"

#include "mrf.h"
#include "post.h"
#include "resample.h"
#include "loudness.h"
#include "true_peak.h"
#include "limiter.h"
#include "stream_loudness.h"
#include "stream_limiter.h"
#include "g711.h"

#include <algorithm>

namespace pe {
namespace launch {

void init_tail() {
#ifndef PE_EMU
  const int lim = 160 * 1024;
  const void* ks[] = {(const void*)mrf_kernel<32, 1, 1>, (const void*)mrf_kernel<32, 2, 1>, (const void*)mrf_kernel<32, 3, 1>, (const void*)mrf_kernel<32, 4, 1>,
                      (const void*)mrf_kernel<64, 1, 2>, (const void*)mrf_kernel<64, 2, 2>, (const void*)mrf_kernel<64, 3, 2>};
  for (const void* k : ks) PE_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
#endif
}

// cp = padded channels (32: one row group of 8 column groups, 1 halo unit per wave; 64: two row groups of 4 column
// groups, 2 halo units per wave); ou = output units per wave (N = 16 * column groups * ou)
void mrf(int cp, int ou, dim3 grid, hipStream_t stream, const MrfP& p) {
  const size_t smem = mrf_smem_bytes(cp, ou);
#define PE_MRF(CP_, OU_, HU_) \
  PE_LAUNCH((mrf_kernel<CP_, OU_, HU_>), grid, dim3(64 * MRF_NW), smem, stream, p.lens, p.wstream, p.phases, p.x, p.len_mul, p.stride, p.n0off, p.hxa, \
            p.wfloats, p.nphases, p)
  if (cp == 32) {
    if (ou == 1) PE_MRF(32, 1, 1); else if (ou == 2) PE_MRF(32, 2, 1); else if (ou == 3) PE_MRF(32, 3, 1); else PE_MRF(32, 4, 1);
  } else {
    if (ou == 1) PE_MRF(64, 1, 2); else if (ou == 2) PE_MRF(64, 2, 2); else PE_MRF(64, 3, 2);
  }
#undef PE_MRF
}

void mrf_sum(dim3 grid, hipStream_t stream, const float* r0, const float* r1, const float* r2, float* out, long bs, int cs,
             const int* lens, int len_mul, float scale) {
  PE_LAUNCH(mrf_sum_kernel, grid, dim3(256), 0, stream, r0, r1, r2, out, bs, cs, lens, len_mul, scale);
}

void conv_post(dim3 grid, hipStream_t stream, const float* x, long x_bs, int x_cs, const float* w, int Cin, float slope,
               const int* lens, int len_mul, float* audio, long a_bs, unsigned* absmax) {
  PE_LAUNCH(conv_post_kernel, grid, dim3(256), 0, stream, x, x_bs, x_cs, w, Cin, slope, lens, len_mul, audio, a_bs, absmax);
}

void pcm16(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const unsigned* absmax, const int* lens,
           int len_mul, short* pcm, long p_bs, short* host) {
  PE_LAUNCH(pcm16_kernel, grid, dim3(PCM16_TPB), 0, stream, lens, len_mul, absmax, audio, a_bs, pcm, p_bs, host);
}

void window_copy(dim3 grid, hipStream_t stream, const float* z, int zs, const int* win, float* out, int ws, int C) {
  PE_LAUNCH(window_copy_kernel, grid, dim3(64), 0, stream, z, zs, win, out, ws, C);
}

void window_gather(dim3 grid, hipStream_t stream, const float* z, long z_bs, int zs, const int* hst, int* dst, int cap,
                   float* out, long o_bs, int ws, int wg) {
  PE_LAUNCH(window_gather_kernel, grid, dim3(64), 0, stream, z, z_bs, zs, hst, dst, cap, out, o_bs, ws, wg);
}

void chunk_peak(dim3 grid, hipStream_t stream, const float* audio, long a_bs, int* st, int cap, int hop) {
  PE_LAUNCH(chunk_peak_kernel, grid, dim3(256), 0, stream, audio, a_bs, st, cap, hop);
}

void chunk_pcm(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* st, int cap, int hop) {
  PE_LAUNCH(chunk_pcm_kernel, grid, dim3(256), 0, stream, audio, a_bs, st, cap, hop);
}

void chunk_pcm_gain(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* st, int cap, int hop, const int* gq) {
  PE_LAUNCH(chunk_pcm_gain_kernel, grid, dim3(256), 0, stream, audio, a_bs, st, cap, hop, gq);
}

void stream_gain(hipStream_t stream, int* ctl, int* gb, int cap, int B, int mode, const int* st, int hop, const int* rows,
                 int rcap, long y_cap) {
  PE_LAUNCH(stream_gain_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, ctl, gb, cap, B, mode, st, hop, rows, rcap, y_cap);
}

void stream_loudness_seg(hipStream_t stream, int nseg, int B, const SlP& p, const SlChunkP& q) {
  PE_LAUNCH(stream_loudness_seg_kernel, dim3(nseg, B), dim3(LOUD_TPB), 0, stream, p, q);
}

void stream_loudness_gain(hipStream_t stream, int B, const SlP& p, const SlChunkP& q, int* gq, int* limrep) {
  PE_LAUNCH(stream_loudness_gain_kernel, dim3(B), dim3(64), 0, stream, p, q, gq, limrep);
}

void stream_limiter(hipStream_t stream, int tiles, int B, const SlmP& p, const SlChunkP& q) {
  PE_LAUNCH(stream_limiter_kernel, dim3(tiles, B), dim3(256), 0, stream, p, q);
}

void stream_adopt(dim3 grid, hipStream_t stream, const float* z, long z_bs, int zs, const float* cond, int cond_bs,
                  int cond_rows, const int* join, int cap, float* pool, long p_bs, int ps, float* pcond, int slots) {
  PE_LAUNCH(stream_adopt_kernel, grid, dim3(64), 0, stream, z, z_bs, zs, cond, cond_bs, cond_rows, join, cap, pool, p_bs, ps,
            pcond, slots);
}

void resample_rows(hipStream_t stream, const int* hst, const int* lens, int len_mul, int* rows, int cap, int B, long x_cap,
                   long y_cap, int L, int M) {
  PE_LAUNCH(resample_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, hst, lens, len_mul, rows, cap, B, x_cap, y_cap, L, M);
}

void resample(dim3 grid, hipStream_t stream, const RsP& p) {
  PE_LAUNCH(resample_kernel, grid, dim3(256), 0, stream, p);
}

void chunk_pcm_rs(dim3 grid, hipStream_t stream, const float* y, long y_bs, const int* rows, int rcap, const int* st, int cap) {
  PE_LAUNCH(chunk_pcm_rs_kernel, grid, dim3(256), 0, stream, y, y_bs, rows, rcap, st, cap);
}

void chunk_pcm_rs_gain(dim3 grid, hipStream_t stream, const float* y, long y_bs, const int* rows, int rcap, const int* st, int cap,
                       const int* gq) {
  PE_LAUNCH(chunk_pcm_rs_gain_kernel, grid, dim3(256), 0, stream, y, y_bs, rows, rcap, st, cap, gq);
}

void loudness_seg(dim3 grid, hipStream_t stream, const LoudP& p) {
  PE_LAUNCH(loudness_seg_kernel, grid, dim3(LOUD_TPB), 0, stream, p);
}

void true_peak(dim3 grid, hipStream_t stream, const TpP& p) {
  PE_LAUNCH(true_peak_kernel, grid, dim3(256), 0, stream, p);
}

void loudness_gain(hipStream_t stream, int B, const double* seg, int nseg_cap, const int* lens, int len_mul, long x_cap, int h,
                   const unsigned* peaks, const unsigned* tpeaks, int* ctl, int* gd, int cap, int limiter) {
  PE_LAUNCH(loudness_gain_kernel, dim3(B), dim3(64), 0, stream, seg, nseg_cap, lens, len_mul, x_cap, h, peaks, tpeaks, ctl, gd, cap, limiter);
}

void limiter(dim3 grid, hipStream_t stream, const LimP& p) {
  PE_LAUNCH(limiter_kernel, grid, dim3(256), 0, stream, p);
}

void true_peak_v(dim3 grid, hipStream_t stream, const TpP& p) {
  PE_LAUNCH(true_peak_v_kernel, grid, dim3(256), 0, stream, p);
}

void limiter_true(dim3 grid, hipStream_t stream, const LimP& p) {
  PE_LAUNCH(limiter_true_kernel, grid, dim3(256), 0, stream, p);
}

void pcm16_trim(dim3 grid, hipStream_t stream, const TrimP& p) {
  PE_LAUNCH(pcm16_trim_kernel, grid, dim3(256), 0, stream, p);
}

void pcm16_gain(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* gq, int gcap, const int* lens,
                int len_mul, short* pcm, long p_bs, short* host) {
  PE_LAUNCH(pcm16_gain_kernel, grid, dim3(PCM16_TPB), 0, stream, lens, len_mul, gq, gcap, audio, a_bs, pcm, p_bs, host);
}

void g711_rows(hipStream_t stream, int B, long max_n, const int* lens, int len_mul, const short* pcm, long p_bs,
               unsigned char* out, long out_cap, int law) {
  const unsigned spans = (unsigned)((std::max<long>(max_n, 1) + G711_SPAN - 1) / G711_SPAN);
  PE_LAUNCH(g711_kernel, dim3(spans, B), dim3(G711_TPB), 0, stream, lens, len_mul, pcm, p_bs, out, out_cap, law);
}

void g711_flat(hipStream_t stream, const short* pcm, long n, unsigned char* out, int law) {
  const unsigned spans = (unsigned)((std::max<long>(n, 1) + G711_SPAN - 1) / G711_SPAN);
  PE_LAUNCH(g711_flat_kernel, dim3(spans), dim3(G711_TPB), 0, stream, pcm, n, out, law);
}

}  // namespace launch
}  // namespace pe

#ifdef PE_STAMPS
PE_TRACE_FETCHER(tail)
#endif
