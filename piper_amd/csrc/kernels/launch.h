// Host-side launchers of the kernels, one translation unit per kernel family (launch_conv.cpp, launch_front.cpp,
// launch_tail.cpp) so that the library builds in parallel: the engine (engine_launch.cpp) sees only the parameter structs (params.h) and
// these prototypes. A launcher picks the template instantiation for its runtime arguments and issues ONE launch on
// `stream` (counted in pe::g_launches). `init()` of a family raises the dynamic-LDS limit of its kernels (160 KiB per
// workgroup on gfx950) and must run once per process before the first launch.
#pragma once
#include "../pe_rt.h"
#include "params.h"

namespace pe {
namespace launch {

// ---- conv GEMM family (launch_conv.cpp)
void init_conv();
// tiled implicit GEMM: cfg = tile configuration id (engine_internal.h CFG_*), halo = 64 | 128 columns of staging slack
void conv_tile(int cfg, bool gate, int halo, dim3 grid, size_t smem, hipStream_t stream, const ConvP& p);
// one-tap convs of a batched call, B operand straight from global memory (conv1x1.h):
// grid = (64-column tiles, blocks of 64 rows, utterances)
void conv1x1(dim3 grid, hipStream_t stream, const ConvP& p);
// split-K forms: nw = 4 | 8 | 12 waves
void conv_splitk(bool gate, int nw, dim3 grid, size_t smem, hipStream_t stream, const ConvP& p);
// half (gate only): half a 32-channel group per workgroup on six waves with the whole K range in flight (conv_splitk.h GT = 2)
void conv_splitk16(bool gate, dim3 grid, size_t smem, hipStream_t stream, const ConvP& p, bool half = false);
// WN gate conv of short calls on 64-row x 12-column workgroups (gate4.h): grid = (12-column tiles, 32-channel groups, utterances)
void gate4(dim3 grid, size_t smem, hipStream_t stream, const ConvP& p);
// ... with the coupling layer's pre composed into it: K = 96 channels of x0, `tapb` = the per-tap bias table (gate4.h)
void gate4pre(dim3 grid, size_t smem, hipStream_t stream, const ConvP& p, const float* tapb);
void conv_group(bool wide, dim3 grid, size_t smem, hipStream_t stream, const ConvG& g);
// the tiled kernel on up to three sibling convs of one tile configuration (conv_mfma.h: conv_mfma_group_kernel)
void conv_tile_group(int cfg, int halo, dim3 grid, size_t smem, hipStream_t stream, const ConvG& g);
void conv_group_sum(dim3 grid, size_t smem, hipStream_t stream, const ConvP& p);

// ---- split-bf16 tiled conv GEMM (launch_bf3.cpp; opt-in matrix mode PIPER_HIP_MATRIX=bf16x3)
void init_bf3();
// cfg: 0 = 128 x 128 tile, 1 = 64 x 128, 2 = 32 x 256 (engine_launch.cpp BF3_BM / BF3_BN); gate needs cfg 0 or 1
// sm: split mode of conv_split_kernel (0 bf16x3, 1 f16x3, 2 bf16x6)
void conv_bf3(int sm, int cfg, bool gate, int halo, dim3 grid, size_t smem, hipStream_t stream, const ConvP& p);
// the fused MRF stage on the 16-bit pipe (mrf_split.h): sm = 0 (bf16x3) or 1 (f16x3); cp / ou as launch::mrf
void mrf_split(int sm, int cp, int ou, dim3 grid, hipStream_t stream, const MrfP& p);

// ---- text encoder / duration predictor / flow glue (launch_front.cpp)
void init_front();
void embed(dim3 grid, hipStream_t stream, const EmbedP& p);
void attention(int dk, dim3 grid, size_t smem, hipStream_t stream, const AttnP& p);
void attno(dim3 grid, size_t smem, hipStream_t stream, const AttnOP& p);        // attention + conv_o + LN, dk = 96 x 2 heads (attno.h)
void attn4(bool long_rows, dim3 grid, size_t smem, hipStream_t stream, const AttnOP& p);   // the same on 4-query workgroups (attn4.h); long_rows: more than 128 ids per utterance
void layer_norm(dim3 grid, hipStream_t stream, const LnP& p);
void dds_layer(int nchunks, dim3 grid, size_t smem, hipStream_t stream, const DdsP& p);
void dds_layer4(dim3 grid, size_t smem, hipStream_t stream, const DdsP& p);      // 4-column form, 192 channels (dds4.h)
void colchain(dim3 grid, size_t smem, hipStream_t stream, const ColP& p);
void colchain4(dim3 grid, size_t smem, hipStream_t stream, const ColP& p);     // 4-column forms (col4.h): weights in pack4 order
void lngemm(dim3 grid, size_t smem, hipStream_t stream, const LnGemmP& p);
void lngemm4(dim3 grid, size_t smem, hipStream_t stream, const LnGemmP& p);
void ffn(dim3 grid, size_t smem, hipStream_t stream, const FfnP& p);            // fused small-call FFN (ffn.h)
void cf_pre(dim3 grid, hipStream_t stream, const float* z0, long z_bs, const float* w, const float* bias, const float* xg,
            long g_bs, int g_cs, float* out, long o_bs, int o_cs, const int* lens, int H);
void spline_inverse(dim3 grid, hipStream_t stream, const float* hproj, long h_bs, int h_cs, float* z1, long z_bs,
                    const int* lens, float inv_sqrt_h);
void scale(dim3 grid, hipStream_t stream, const float* in, float* out, long n, const float* s, long per_utt);
void duration(dim3 grid, hipStream_t stream, const DurP& p);
void duration_plan(dim3 grid, hipStream_t stream, const PlanP& p);      // duration_kernel's place under a timing plan (timing.h)
// keys / use / ch: the per-utterance seed table and the rows per utterance (rng.h); keys null: no utterance is seeded
void randn(hipStream_t stream, float* out, long rows, int cols, long stride, long row0, const unsigned long long* state,
           int site, const unsigned long long* keys = nullptr, const int* use = nullptr, int ch = 1);
void regulate(dim3 grid, hipStream_t stream, const RegP& p);
void xcc_probe(hipStream_t stream, int* out64);       // 64 workgroups, out64[i] = XCC id of workgroup i
void cond(dim3 grid, hipStream_t stream, const float* emb_g, int gin, const int* sids, const float* w, const float* bias,
          int rows, float* out, int o_bs);
// g[batch][gin] of a call that carries a blend (glue.h): 64 lanes along gin per workgroup, one grid row per utterance
void speaker_blend(hipStream_t stream, int batch, const BlendP& p);

// ---- vocoder stage kernels and the generator tail (launch_tail.cpp)
void init_tail();
void mrf(int cp, int ou, dim3 grid, hipStream_t stream, const MrfP& p);
void mrf_sum(dim3 grid, hipStream_t stream, const float* r0, const float* r1, const float* r2, float* out, long bs, int cs,
             const int* lens, int len_mul, float scale);
void conv_post(dim3 grid, hipStream_t stream, const float* x, long x_bs, int x_cs, const float* w, int Cin, float slope,
               const int* lens, int len_mul, float* audio, long a_bs, unsigned* absmax);
void pcm16(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const unsigned* absmax, const int* lens,
           int len_mul, short* pcm, long p_bs, short* host);
void window_copy(dim3 grid, hipStream_t stream, const float* z, int zs, const int* win, float* out, int ws, int C);
// batch streaming (params.h: sb_*): grid = (64-frame tiles of the window bucket wg, channels, utterances)
void window_gather(dim3 grid, hipStream_t stream, const float* z, long z_bs, int zs, const int* hst, int* dst, int cap,
                   float* out, long o_bs, int ws, int wg);
// ... and the chunk delivery: grid = (steps of CHUNK_SPB samples, utterances), peak first, conversion second
void chunk_peak(dim3 grid, hipStream_t stream, const float* audio, long a_bs, int* st, int cap, int hop);
void chunk_pcm(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* st, int cap, int hop);
// stream-wide gain (params.h: sg_*, sgd_*): one thread per row between the peak and the conversion; rows null: the chunk's
// range and peak from the window state block `st`, else from the resampling row block. chunk_pcm_gain / chunk_pcm_rs_gain =
// the conversions with the operands stream_gain wrote to `gq`
void stream_gain(hipStream_t stream, int* ctl, int* gb, int cap, int B, int mode, const int* st, int hop, const int* rows,
                 int rcap, long y_cap);
void chunk_pcm_gain(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* st, int cap, int hop, const int* gq);
// target loudness of streams (params.h: sl*, SlP, SlChunkP), in stream_gain's place: grid = (nseg segments a chunk can touch,
// B rows), then one wave per row; `gq` = the rows' gain block, whose sgd_* words the conversions read
void stream_loudness_seg(hipStream_t stream, int nseg, int B, const SlP& p, const SlChunkP& q);
void stream_loudness_gain(hipStream_t stream, int B, const SlP& p, const SlChunkP& q, int* gq, int* limrep = nullptr);
// the look-ahead limiter on streams in the gain conversion's place: grid = (tiles of LIM_TILE delivered samples, rows)
void stream_limiter(hipStream_t stream, int tiles, int B, const SlmP& p, const SlChunkP& q);
// stream pool (params.h: sj_*): grid = (64-frame tiles of the newcomers' frame bucket, channels, newcomers)
void stream_adopt(dim3 grid, hipStream_t stream, const float* z, long z_bs, int zs, const float* cond, int cond_bs,
                  int cond_rows, const int* join, int cap, float* pool, long p_bs, int ps, float* pcond, int slots);
// output-rate conversion (params.h: rs_*): the row block first (one thread per row), then grid = (tiles of p.tile output
// samples, rows); chunk_pcm_rs = chunk_pcm on the resampled rows, grid = (steps of CHUNK_SPB samples, rows)
void resample_rows(hipStream_t stream, const int* hst, const int* lens, int len_mul, int* rows, int cap, int B, long x_cap,
                   long y_cap, int L, int M);
void resample(dim3 grid, hipStream_t stream, const RsP& p);
void chunk_pcm_rs(dim3 grid, hipStream_t stream, const float* y, long y_bs, const int* rows, int rcap, const int* st, int cap);
void chunk_pcm_rs_gain(dim3 grid, hipStream_t stream, const float* y, long y_bs, const int* rows, int rcap, const int* st, int cap,
                       const int* gq);
// target loudness (params.h: ld_*, LoudP): grid = (100 ms segments of the bucket, rows), then one wave per row; pcm16_gain =
// pcm16 with the scale loudness_gain wrote to `gq`. True-peak ceiling (TpP): true_peak between the two, grid = (tiles of
// TP_TILE native samples, rows), and its words as `tpeaks` (null: the sample-peak ceiling)
void loudness_seg(dim3 grid, hipStream_t stream, const LoudP& p);
void true_peak(dim3 grid, hipStream_t stream, const TpP& p);
void loudness_gain(hipStream_t stream, int B, const double* seg, int nseg_cap, const int* lens, int len_mul, long x_cap, int h,
                   const unsigned* peaks, const unsigned* tpeaks, int* ctl, int* gd, int cap, int limiter);
// look-ahead limiter (LimP): in pcm16_gain's place, grid = (tiles of LIM_TILE samples, rows); loudness_gain's `limiter` != 0
// marks the rows it shapes
void limiter(dim3 grid, hipStream_t stream, const LimP& p);
// the limiter under the true-peak ceiling: true_peak_v = true_peak that also stores the per-position maxima (p.v),
// limiter_true writes z and max |z| instead of the int16, true_peak runs on z, pcm16_trim converts (grid as pcm16_gain)
void true_peak_v(dim3 grid, hipStream_t stream, const TpP& p);
void limiter_true(dim3 grid, hipStream_t stream, const LimP& p);
void pcm16_trim(dim3 grid, hipStream_t stream, const TrimP& p);
void pcm16_gain(dim3 grid, hipStream_t stream, const float* audio, long a_bs, const int* gq, int gcap, const int* lens,
                int len_mul, short* pcm, long p_bs, short* host);
// G.711 codes of the delivered int16 (g711.h; law = G711_ULAW / G711_ALAW). Rows form: grid = (spans of G711_SPAN samples
// of max_n, rows), row b = lens[b] * len_mul int16 at pcm + b * p_bs, codes packed back to back into out[0, out_cap).
// Flat form: n contiguous int16 at a 16-byte aligned base -> n codes (n == 0: one idle workgroup, so that a chunk's launch count does not depend on what it delivers)
void g711_rows(hipStream_t stream, int B, long max_n, const int* lens, int len_mul, const short* pcm, long p_bs,
               unsigned char* out, long out_cap, int law);
void g711_flat(hipStream_t stream, const short* pcm, long n, unsigned char* out, int law);

}  // namespace launch
}  // namespace pe
