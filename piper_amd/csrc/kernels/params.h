// Launch parameters and host-visible constants of every kernel (what engine_launch.cpp fills in and the launch translation
// units kernels/launch_*.cpp pass on). Device code lives in the per-kernel headers next to this file; each struct's
// fields are documented there where the kernel uses them.
#pragma once
#include <cstddef>

namespace pe {

// ---- conv GEMM kernels (conv_common.h)
static constexpr int KC = 32;           // input channels staged per K-chunk of the conv GEMM
enum Epi { EPI_STORE = 0, EPI_RESADD = 1, EPI_GATE = 2, EPI_WNRS = 3, EPI_SUBFROM = 4,
           EPI_ACCUM = 5, EPI_CONVT = 6 };
enum Act { ACT_NONE = 0, ACT_RELU = 1 };
struct ConvP {
  const float* x; long x_bs; int x_cs;          // input  x[b][ci][t]
  const float* wp;                              // packed weights (engine_pack.cpp: pack_conv)
  const float* wp16;                            // conv_splitk16_kernel: the same in 16x16x4 fragment order, or null
  const float* wpb;                             // conv_split_kernel: 16-bit split-term fragments of the matrix mode (engine_pack.cpp pack_matrix), or null
  const float* wunscale;                        // conv_split_kernel, mode f16x3: the weights were packed times 1 / *wunscale (a power of two)
  const float* wpg4;                            // gate4_kernel: the gate conv in [group][tap][k quad][lane][4] order (192 input channels), or null
  const float* bias;                            // per output channel or null
  const float* bias2; int bias2_bs;             // per-utterance extra bias (speaker cond) or null
  float* out; long o_bs; int o_cs;
  const float* res; long r_bs; int r_cs;        // residual input (may alias out)
  float* out2; long o2_bs; int o2_cs;           // second output (WN skip accumulator)
  const int* lens; int len_mul;                 // valid input length = lens[b]*len_mul
  int Cin, rows;                                // real input channels; GEMM rows (Cout, or Cout*up)
  int nchunks;                                  // ceil(Cin/KC)
  int ntaps, dil, padl;                         // tap k reads x[t + k*dil - padl]
  int xhalo;                                    // (ntaps-1)*dil
  float in_slope;                               // leaky-relu slope applied to x while staging (1 = none)
  int epi, act;
  int split;                                    // GATE: H ; WNRS: rows < split go to h, rest to skip
  int up, padT;                                 // CONVT: stride and padding
  unsigned up_magic;                            // CONVT: ceil(2^32 / up): row / up == (row * up_magic) >> 32 for row < 2^16
  int up_vec;                                   // CONVT, conv_mfma_kernel: a lane's four accumulator rows are consecutive output samples of ONE
                                                // channel when up is a multiple of 4 (4: one 16-byte store) or both phases of two channels when
                                                // up == 2 (2: two 8-byte stores); 0: one by one
  int mode;                                     // ACCUM: 0 first,1 middle,2 last,3 only ; WNRS: 1 = first layer
  float alpha;                                  // ACCUM last/only: scale
  int tpb;                                      // conv_mfma_kernel: column tiles walked by one workgroup
  int tgroups;                                  // conv_splitk_kernel: 1, or 2 = two halves of the waves split the taps
  // conv_splitk_body<..., MS = true> only: K = the concatenation of nseg convs of one shape whose outputs are summed
  // (segment 0 repeats x / wp / ntaps / dil / padl); res2 / res3 = the residual tensors of segments 1 / 2
  int nseg;
  const float* seg_x[3]; const float* seg_wp[3];
  int seg_ntaps[3], seg_dil[3], seg_padl[3];
  const float* res2; const float* res3;
};

// ---- grouped split-K launches (conv_splitk.h)
struct ConvG {
  ConvP c[3];
  int n, B;
};

// ---- relative-position attention (attention.h)
struct AttnP {
  const float* qkv; long q_bs; int q_cs;
  const float* relk; const float* relv;     // [2w+1][dk]
  float* out; long o_bs; int o_cs;
  const int* lens;
  int H, dk, window;
  int SP;                                   // score row stride in LDS: odd, >= round_up(max len, 64)
  float qscale;
  float* sglobal;                           // attn_long_kernel: [utterance][head][query block][32][SP] score slabs (null: LDS)
};
// attno_kernel (attno.h): attention + conv_o + residual + norm_layers_1 of an encoder layer in one launch
struct AttnOP {
  const float* qkv; long q_bs; int q_cs;
  const float* relk; const float* relv;     // [2w+1][dk]
  const int* lens;
  int window;
  int SP;                                   // score row stride in LDS: round_up(max len, 64) + 2 (== 2 mod 32)
  float qscale;
  const float* wo16; const float* bo;       // conv_o in pack16 order, bias [H]
  const float* gamma; const float* beta;    // norm_layers_1
  float* x; long x_bs; int x_cs;            // residual in, LayerNorm output (in place)
  const float* wo4;                         // attn4_kernel: conv_o in pack4 order; SP = round_up(max len, 64) + 4 there
  const float* kT; long kt_bs;              // attn4_kernel: K as [utterance][channel quad][column stride q_cs][4] (written by the q/k/v launch)
  const float* vQ;                          // attn4_kernel: V as [utterance][column quad][192][4] (same batch stride)
  int xcd;                                  // attn4_kernel: XCD-contiguous column tiles (col4.h c4_tile)
};
static constexpr int ATT_QB = 32;           // queries per workgroup (one MFMA tile)
static constexpr int ATT_KCH = 64;          // keys staged per V chunk
static constexpr int ATT_MAXDK = 128;

// ---- LayerNorm (layernorm.h)
struct LnP {
  const float* in; long i_bs; int i_cs;
  float* out; long o_bs; int o_cs;
  const float* gamma; const float* beta;
  const int* lens;
  int C;
};
static constexpr int LN_COLS = 8, LN_NV = 8;

// ---- spline (spline.h)
static constexpr int SPL_NB = 10;

// ---- DDSConv layer (dds.h)
struct DdsP {
  const float* x; long x_bs; int x_cs;
  float* out; long o_bs; int o_cs;
  const float* dw_w; const float* dw_b; int dw_k, dw_dil;
  const float* g1; const float* b1; const float* g2; const float* b2;
  const float* bias;                        // 1x1 conv bias
  const float* wp16;                        // 1x1 conv weights in the 16x16x4 fragment order (engine_pack.cpp)
  const float* wp4;                         // the same in the 4x4x1 fragment order (dds_layer4_kernel; null: not packed)
  int nchunks;                              // ceil(H / 32)
  const int* lens;
  int H;
  // Optional fold of ConvFlow.pre + DDSConv's "x = x + g" into the layer input (modules.py:504-505, 118-119), first
  // layer of a ConvFlow: the input is  pre_w[c] * (z0[t] * z_scale) + pre_b[c] + x[c][t]  with x = the conditioning g.
  const float* pre_z; long pre_z_bs;        // z0 row of utterance b (null: no fold)
  const float* pre_w; const float* pre_b;
  // noise_scale_w of utterance b at z_scale[3 b] on the first flow (z is still the raw N(0,1) draw: &scales[0][2] of the
  // per-utterance [B][3] array); null: 1
  const float* z_scale;
  // Optional second 1x1 conv on the layer's output columns (last layer of a DDSConv: dp.proj / ConvFlow.proj,
  // models.py:65, modules.py:507), weights in the 16x16x4 fragment order; the layer output itself is then not stored.
  const float* post_w16; const float* post_w4; const float* post_bias; int post_rows;
  float* post_out; long po_bs; int po_cs;   // plain store of the post conv (dp.proj), or null
  // Optional spline epilogue (ConvFlow, modules.py:508-526): the post conv's 29 rows are the per-position parameters;
  // z1 <- rq_spline_inverse(z1 * z_scale), z0 <- z0 * z_scale (pass-through), both [2][Ts] tensors may alias.
  const float* zin; long zin_bs; int z_cs; int c0, c1;
  float* zout; long zout_bs;
  float inv_sqrt_h;
  int xcd;                                  // dds_layer4_kernel: XCDs the dispatch round-robins over (0: unknown), col4.h c4_tile
};

// ---- 1x1 conv chains (colchain.h)
struct ColP {
  const float* in1; long in1_bs; int in1_cs; int K1;
  const float* w1; const float* b1; int rows1;
  int mode;
  const float* res; long res_bs; int res_cs;            // mode 0
  const float* gamma; const float* beta;
  float* out; long out_bs; int out_cs;
  float* x1; long x1_bs; int x1_cs;                     // mode 1 (updated in place)
  const float* w2; const float* b2; int rows2;          // w2 == null: no second GEMM (last coupling layer)
  float* out2; long o2_bs; int o2_cs;
  const int* lens;
  int first;                                            // mode 2 (colchain4_kernel): first WN layer -- the skip sum is not read
  int xcd;                                              // colchain4_kernel: XCDs the dispatch round-robins over (0: unknown)
  // colchain4_kernel<true> (mode 1): the last WN layer's res/skip conv in front -- GEMM 1 reads (w0.in0 + b0) + in1
  const float* in0; long in0_bs; int in0_cs;
  const float* w0; const float* b0;
  float* kT; long kt_bs;                                // mode 3, optional: row part 1 also as [channel quad][column][4] (see LnGemmP)
  float* vQ;                                            // ... and row part 2 as [column quad][192][4]
};
// ---- fused FFN (ffn.h): partial outputs per 48-row slice of the hidden dimension
struct FfnP {
  const float* x; long x_bs; int x_cs;           // norm_layers_1 output [192][T]
  const float* w1p; const float* b1;             // conv_1: pack_ffn order per slice, bias [FC]
  const float* w2p;                              // conv_2: pack_ffn order per slice (its bias is added by the consumer)
  float* parts; long p_bs; int nslices;          // [utterance][4-column tile][slice][192][4], p_bs floats per utterance
  const int* lens;
  int xcd;                                       // XCDs the dispatch round-robins over -> (column tile, slice) by pe_xcd_xy; 0 / 1: blockIdx
};
struct LnGemmP {
  const float* in; long in_bs; int in_cs;        // y = x + ffn(x)  (parts != null: the residual x alone)
  // lngemm4_kernel only: y = in + pbias + sum of the nparts partial FFN outputs (ffn_kernel), in slice order
  const float* parts; long p_bs; int nparts;     // [utterance][4-column tile][slice][192][4]
  const float* pbias;
  int xcd;                                       // lngemm4_kernel: XCDs the dispatch round-robins over (0: unknown)
  const float* gamma; const float* beta;
  float* xout; long x_bs; int x_cs;              // LN(y)
  const float* w16; const float* bias; int rows; // pack16 order, all parts; part z owns rows [32 NVT z, 32 NVT (z + 1))
  float* out; long o_bs; int o_cs;
  const int* lens;
  // lngemm4_kernel, optional: rows >= split belong to a SECOND conv over the same LN(y) (enc_p.proj stacked with dp.pre):
  // they go to out2 (row 0 = GEMM row split) and take the per-utterance bias vector bias2 (speaker conditioning) as well
  int split; float* out2; long o2_bs; int o2_cs; const float* bias2; long bias2_bs;
  // lngemm4_kernel, optional (q/k/v conv in front of attn4_kernel): row part 1 (the K rows) is ALSO written as
  // kT[utterance][channel quad 48][column stride][4], so that the attention kernel takes four channel steps of a key as ONE
  // 16-byte load that is contiguous across the lanes (= keys) of a wave
  float* kT; long kt_bs;
  // ... and row part 2 (the V rows) as vQ[utterance][column quad][192][4]: four keys of a channel per 16-byte load,
  // contiguous across the lanes (= channels) of a wave (same batch stride kt_bs)
  float* vQ;
};

// ---- text embedding = the first kernel of every run (attention.h: embed_kernel)
struct EmbedP {
  const int* ids; int ids_bs;                  // [B][Ts] phoneme ids
  const int* lens;                             // [B]
  const float* emb; int H; float scale;
  float* out; long o_bs; int o_cs;
  unsigned long long* rng;                     // device {seed, runs so far, last ingested upload, -}
  // Zero-copy inputs (null: upload() copied the input block to the device). The pinned host mirror of the block is read
  // in place: ids and lengths by every workgroup that needs them, lengths / speaker ids / {seed, counter} published to
  // device memory for the kernels behind this one.
  const unsigned long long* h_rng; const int* h_lens; const int* h_sids; const float* h_scales; const int* h_ids;
  int* d_lens; int* d_sids; float* d_scales;   // (scales: [B][3] per utterance {noise_scale, length_scale, noise_w})
  // Optional (small calls): the duration noise of models.py:111 -- rows 2 b, 2 b + 1 of the site-0 stream, draw_cols columns,
  // exactly the values randn_kernel writes -- drawn by workgroup (0, 0, 0), the one that advances the generator state, with
  // the state it publishes; null: randn_kernel draws it in a launch of its own.
  float* draw_out; long draw_stride; int draw_rows, draw_cols;
  // Per-utterance seeds (rng.h; null: the call carries none): the device table keys[B] / use[B] of the input block, and on
  // the zero-copy path its pinned mirror, which the kernel publishes to the device table like lengths and scales.
  unsigned long long* keys; int* use;
  const unsigned long long* h_keys; const int* h_use;
};

// ---- speaker vectors of a blended call (glue.h: speaker_blend_kernel)
static constexpr int BLEND_MAX = 8;            // components per utterance (include/piper_hip.h: PE_BLEND_MAX)
struct BlendP {
  const float* emb_g; int gin;                 // the speaker table [num_speakers][gin]
  const int* sids;                             // [B] device speaker ids (count 0)
  const int* count;                            // [B]  0 plain id, 1..BLEND_MAX components, -1 row b of vec
  const int* csid; const float* cw;            // [B][BLEND_MAX] components, the first count[b] of a row are used
  const float* vec;                            // [B][gin] caller-supplied vectors
  float* g;                                    // out [B][gin]
  int* rows;                                   // out [B] rows[b] = b: cond_kernel's index into g (null: not written)
};

// ---- durations, N(0,1) generator, length regulator (duration.h)
static constexpr int MAX_FRAMES = 60000;      // per-utterance activations stay below the 2 GiB descriptor range
struct DurP {
  const float* z0; long z_bs; float m0, es0;
  const float* scales;                         // [B][3] per utterance {noise_scale, length_scale, noise_w} (device)
  const int* lens; int* dur; int* cum; int d_bs; int* frames; float* logw_out;
  int* frames_host; int* frames_clamped; int frame_cap;
};
// ---- timing plan (timing.h). The plan block, device and pinned host alike: [target Bc | per utterance: rate T floats,
// forced T ints], so that the rows of a call's B utterances are one contiguous piece behind the targets.
struct PlanP {
  DurP d;                                      // duration_kernel's fields; d.z0 null: every id is forced, no logw exists
  const int* target;                           // [B]: > 0 the utterance's frame count, 0 none
  const float* rate; const int* forced; long pl_bs;      // row b at + b * pl_bs: multiplier of the id's duration; >= 0 forced frames, -1 predicted
  float* w_out;                                // [B][d.d_bs] w_i ("plan_w"), or null
};
static inline size_t plan_words(size_t Bc, size_t T) { return Bc + 2 * Bc * T; }
static constexpr int RNG_PITCH = 65536;       // >= MAX_FRAMES and >= the longest id sequence
static inline unsigned randn_blocks(long rows, int cols) { return (unsigned)(rows * ((cols + 1023) / 1024)); }
struct RegP {
  const float* stats; long s_bs; int s_cs;     // [B][2C][Ts]: m_p rows [0,C), logs_p rows [C,2C)
  const int* cum; int d_bs;
  const int* tlens; const int* frames;
  float* noise; long n_bs; int n_cs;           // [B][C][>=F]: read (injected noise), or written by the kernel's own draws (gen)
  const float* scales;                         // [B][3] per utterance {noise_scale, length_scale, noise_w} (device)
  float* out; long o_bs; int o_cs;
  int C;
  unsigned* absmax;                            // per-utterance peak accumulator of conv_post_kernel: zeroed here
  const unsigned long long* rng; int gen;      // gen: the prior noise (site 1) is drawn here and stored to `noise`
  DurP dur; int fold;                          // fold: the durations are computed here too (duration_kernel's fields)
  const unsigned long long* keys; const int* use;      // per-utterance seeds (rng.h), device table; keys null: none
};
static constexpr int REG_MAXT = 4096;          // ids whose cumulative durations fit the LDS copy; longer: search in global memory

// ---- generator tail (post.h)
static constexpr int POST_K = 7, POST_OPT = 4, POST_CU = 8, POST_CG = 4, POST_SPB = 64 * POST_OPT;

// ---- batch streaming (post.h: window_gather_kernel, chunk_peak_kernel, chunk_pcm_kernel)
// The per-chunk state of a batch stream is DATA, so that one captured graph serves every chunk: a block of 32-bit words
// for `cap` utterances (cap even, the block 8-byte aligned) that the host fills in pinned memory before each chunk.
// window_gather_kernel, the first launch of the window stage, reads it in place and publishes it to a device block of the
// same layout for the launches behind it (the generator reads `len` as its contiguous int[B] frame counts).
//   start[cap] len[cap]    window of z in frames: [start, start + len)
//   first[cap] count[cap]  the chunk's own samples inside the window's waveform (the window minus its halo)
//   off[cap] (64-bit)      where the chunk goes in the packed host output
//   pcm, audio (pointers)  pinned host output of this chunk; audio null: no floats wanted
//   peak[cap]              device block only: max |sample| of the chunk as a float's bit pattern, cleared by the gather
static constexpr int sb_o_len(int cap) { return cap; }
static constexpr int sb_o_first(int cap) { return 2 * cap; }
static constexpr int sb_o_count(int cap) { return 3 * cap; }
static constexpr int sb_o_off(int cap) { return 4 * cap; }
static constexpr int sb_o_ptrs(int cap) { return 6 * cap; }
static constexpr int sb_o_peak(int cap) { return 6 * cap + 4; }
static constexpr int sb_words(int cap) { return 7 * cap + 4; }
static constexpr int CHUNK_SPB = 1024;         // samples one workgroup of the delivery kernels covers per step

// ---- stream-wide gain (post.h: stream_gain_kernel, chunk_pcm_gain_kernel; resample.h: chunk_pcm_rs_gain_kernel)
// The int16 level of a stream outside the default per-chunk rule. The setting's numbers are DATA like the window state: a
// pinned host control block for `cap` rows that the host fills before each chunk and stream_gain_kernel reads in place,
// and into which the kernel writes what pe_stream_last_gains reports; the running peaks and the conversion's operands
// live in a device block.
//   control (pinned host)  P (float bits), R0, first[cap] (1: the row's stream has delivered nothing yet: its state is
//                          reset to P), report gain[cap] (g1), report peak[cap] (the level g1 came from)
//   gain (device)          r[cap] running peak (f32), then for the conversion g0[cap], g1[cap] (f32) and R[cap] (ramp
//                          samples of this chunk: min(R0, chunk length))
enum { GAIN_CHUNK = 0, GAIN_RUNNING = 1, GAIN_FIXED = 2 };
static constexpr int GAIN_MAX_RAMP = 65536;
static constexpr int sg_o_first(int cap) { (void)cap; return 2; }
static constexpr int sg_o_rgain(int cap) { return 2 + cap; }
static constexpr int sg_o_rpeak(int cap) { return 2 + 2 * cap; }
static constexpr int sg_words(int cap) { return 2 + 3 * cap; }
static constexpr int sgd_o_g0(int cap) { return cap; }
static constexpr int sgd_o_g1(int cap) { return 2 * cap; }
static constexpr int sgd_o_ramp(int cap) { return 3 * cap; }
static constexpr int sgd_words(int cap) { return 4 * cap; }

// ---- target loudness of streams (stream_loudness.h: stream_loudness_seg_kernel, stream_loudness_gain_kernel; mode
// GAIN_LOUDNESS of the stream-wide gain). The setting's numbers are DATA like the other modes': a pinned host
// control block of its own for `cap` rows, which the gain kernel reads in place and writes its report into; what a stream
// carries from chunk to chunk lives on the device: a state block, the segment sums seg[cap][nseg_cap] (f64) and two tail
// buffers of W floats per row, tail[cap][2][W] (the kernels alternate between them: the seg kernel reads one and writes the
// other). The conversion's operands go to the sgd_* words of the rows' gain block.
//   control (pinned host)  T (LUFS), C (ceiling as a peak ratio), prior (LUFS; NaN: none) as f32, R0, first[cap], then the
//                          report: L[cap] (f32 LUFS, -inf: not measurable), g1[cap], r'[cap] (f32), flags[cap], g0[cap], R[cap]
//   state (device)         r[cap] running peak, G[cap] last end-of-chunk gain, lu[cap] last loudness used (NaN: none) as
//                          f32, N[cap] samples delivered, par[cap] which tail buffer holds the stream's last W samples
static constexpr int GAIN_LOUDNESS = 3;
static constexpr int LOUD_PRIOR = 16;          // (beside LOUD_SHAPED = 8 of the whole-utterance flags, below)
static constexpr int slc_o_first(int cap) { (void)cap; return 4; }
static constexpr int slc_o_lufs(int cap) { return 4 + cap; }
static constexpr int slc_o_gain(int cap) { return 4 + 2 * cap; }
static constexpr int slc_o_peak(int cap) { return 4 + 3 * cap; }
static constexpr int slc_o_flags(int cap) { return 4 + 4 * cap; }
static constexpr int slc_o_g0(int cap) { return 4 + 5 * cap; }
static constexpr int slc_o_ramp(int cap) { return 4 + 6 * cap; }
static constexpr int slc_words(int cap) { return 4 + 7 * cap; }
static constexpr int sld_o_r(int cap) { (void)cap; return 0; }
static constexpr int sld_o_g(int cap) { return cap; }
static constexpr int sld_o_lu(int cap) { return 2 * cap; }
static constexpr int sld_o_n(int cap) { return 3 * cap; }
static constexpr int sld_o_par(int cap) { return 4 * cap; }
static constexpr int sld_words(int cap) { return 5 * cap; }
struct SlP {
  int* ctl; int* dev; int cap;                 // control and state blocks for cap rows
  const double* coef;                          // filter block (LOUD_COEF_DOUBLES, as LoudP's)
  int h, W, R;                                 // samples of a 100 ms segment, of the tail (50 ms), of one thread's run
  double* seg; int nseg_cap;                   // segment sums seg[cap][nseg_cap], indexed by STREAM segment
  float* tail;                                 // tail[cap][2][W]
};
// Row b's chunk: n samples at x. Native rate (rows null): [first, first + count) of the row's window waveform, by the
// window state block; converted rate: the first count outputs of the row's resampled waveform, by the resampling row block,
// cut to y_cap as the conversion cuts it. c = the chunk's peak word.
struct SlChunkP {
  const float* x; long x_bs;                   // audio_ [rows][x_bs], or raudio_ [rows][y_cap ..]
  const int* st; int cap; int hop;             // window state block (device)
  const int* rows; int rcap; long y_cap;       // resampling row block (device), or null
};

// ---- stream pool (post.h: stream_adopt_kernel). The join block, pinned host memory for `cap` newcomers that the kernel
// reads in place: which slot every newcomer of a join takes and how many frames it has -- data, not kernel arguments.
//   n, (pad)               newcomers of this join
//   slot[cap] frames[cap]  newcomer j goes to pool row slot[j] with frames[j] frames
static constexpr int sj_o_slot(int cap) { (void)cap; return 2; }
static constexpr int sj_o_frames(int cap) { return 2 + cap; }
static constexpr int sj_words(int cap) { return 2 + 2 * cap; }

// ---- output-rate conversion (resample.h: resample_rows_kernel, resample_kernel, chunk_pcm_rs_kernel)
// What a row of a resampling launch covers is DATA, like the window state above: a block of 32-bit words for `cap` rows
// (cap even, the block 8-byte aligned). resample_rows_kernel fills the device block -- from the frame counts of a whole-
// utterance call, or from a pinned host block of the same layout that a stream fills before each chunk -- and clears the peaks.
//   n0[cap] (64-bit)       index of the row's first output sample within its utterance
//   org[cap] (64-bit)      native index, within the utterance, of element 0 of the buffer the row reads
//   count[cap]             output samples of the row
//   vlen[cap]              elements [0, vlen) of that buffer are the utterance's samples; everything else reads as zero
//   peak[cap]              device block only: max |output| as a float's bit pattern
static constexpr int rs_o_org(int cap) { return 2 * cap; }
static constexpr int rs_o_count(int cap) { return 4 * cap; }
static constexpr int rs_o_vlen(int cap) { return 5 * cap; }
static constexpr int rs_o_peak(int cap) { return 6 * cap; }
static constexpr int rs_words(int cap) { return 7 * cap; }
static constexpr int RS_TILE = 1024;           // output samples per workgroup, fewer where the native span would not fit
static constexpr int RS_SPAN = 3072;           // floats of LDS that hold a tile's native span (12 KB)
struct RsP {
  const float* x; long x_bs;                   // native rows x[b][.]
  float* y; long y_bs;                         // resampled rows y[b][0 .. count_b)
  const float* coef;                           // [L][Tp] polyphase table, row = phase (n * M) mod L, 16-byte aligned rows
  int L, M, K, Tp;                             // fs_out / g, fs_in / g, half-width in native samples, taps per row (2K rounded up to 4)
  int* rows; int cap;                          // device row block
  int tile;                                    // output samples per workgroup: its native span fits RS_SPAN
};

// ---- target loudness of whole utterances (loudness.h: loudness_seg_kernel, loudness_gain_kernel; post.h: pcm16_gain_kernel)
// The setting's numbers are DATA, like the stream gain's: a pinned host control block for `cap` rows that
// loudness_gain_kernel reads in place and into which it writes what pe_last_loudness reports; the conversion's operand
// lives in a device block of the report's layout.
//   control (pinned host)  T (target, LUFS), C (ceiling as a peak ratio) as f32, then the report, then the true peaks
//   report / device block  L[cap] (f32 LUFS, -inf: not measurable), scale[cap] (f32), peak[cap] (f32), flags[cap]
// The filter block (device, f64): shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2}, then LOUD_LEVELS 4 x 4
// matrices A^(R 2^k), k = 0 .. LOUD_LEVELS - 1, row-major: what R samples of silence make of the cascade's four states.
enum { LOUD_SHORT = 1, LOUD_UNMEASURABLE = 2, LOUD_LIMITED = 4, LOUD_SHAPED = 8 };      // (SHAPED: the look-ahead limiter, below)
static constexpr int LOUD_TPB = 256;           // threads (= runs) of a segment's workgroup
static constexpr int LOUD_LEVELS = 8;          // log2(LOUD_TPB)
static constexpr int LOUD_COEF_DOUBLES = 10 + 16 * LOUD_LEVELS;
static constexpr int ld_o_scale(int cap) { return cap; }
static constexpr int ld_o_peak(int cap) { return 2 * cap; }
static constexpr int ld_o_flags(int cap) { return 3 * cap; }
static constexpr int ld_words(int cap) { return 4 * cap; }
static constexpr int ldc_o_report(int cap) { (void)cap; return 2; }
static constexpr int ldc_words(int cap) { return 2 + 5 * cap; }      // (the report, then the true peaks: ldc_o_tpeak)
struct LoudP {
  const float* x; long x_bs;                   // delivered rows x[b][0 .. n_b), n_b = lens[b] * len_mul cut to x_cap
  const int* lens; int len_mul; long x_cap;
  const double* coef;                          // filter block
  int h, W, R;                                 // samples of a 100 ms segment, of the warm-up in front of it, of one thread's run
  double* seg; int nseg_cap;                   // segment sums seg[b][nseg_cap]
  unsigned* tpeak;                             // true-peak words [rows] to clear for true_peak_kernel, or null (sample-peak ceiling)
  int* limrep; int limcap;                     // limiter report words (lim_o_*) to clear for limiter_kernel, or null (limiter off)
};

// ---- true-peak ceiling of the target loudness (true_peak.h: true_peak_kernel)
// The kind of ceiling picks the launches (PEAK_TRUE: one more, between the segment sums and the gain) and is part of the
// graph keys. The table is the resampler's for the pair fs -> Q fs, Q = ceil(192000 / fs): its half-width is TP_K native
// samples at every fs in [8000, 48000], where Q <= TP_MAXQ. One word per row (max |interpolated sample| as a float's bit
// pattern) in a device allocation of its own; loudness_gain_kernel copies it into the control block's report behind the
// flags: tpeak[cap] at ldc_o_tpeak.
enum { PEAK_SAMPLE = 0, PEAK_TRUE = 1 };
static constexpr int TP_K = 18;                // ceil(16 / 0.92)
static constexpr int TP_TAPS = 2 * TP_K;       // taps of a phase (a multiple of 4: the table needs no padding)
static constexpr int TP_MAXQ = 24;             // Q at 8000 Hz
static constexpr int TP_TILE = 1024;           // native samples per workgroup
static constexpr int TP_SPAN = TP_TILE + TP_TAPS + 4;      // floats of LDS: the tile, its halo, alignment slack
static constexpr int ldc_o_tpeak(int cap) { return 2 + 4 * cap; }
struct TpP {
  const float* x; long x_bs;                   // delivered rows x[b][0 .. n_b), n_b = lens[b] * len_mul cut to x_cap
  const int* lens; int len_mul; long x_cap;
  const float* coef; int Q;                    // [Q][TP_TAPS] polyphase table
  unsigned* tpeak;                             // [rows], zero before the launch
  float* v;                                    // true_peak_v_kernel only: v[b][c] = max over ph of |y[c Q + ph]|, row stride x_bs
};

// ---- look-ahead limiter of the target loudness (limiter.h: limiter_kernel)
// On / off picks the launches (limiter_kernel in pcm16_gain_kernel's place) and is part of the graph keys; W, the window in
// samples of the delivered rate, is a kernel argument. A row is SHAPED when the ceiling would have won (LIMITED) and the
// loudness is measurable: loudness_gain_kernel then leaves scale = 32767 g, g = 10^((T - L) / 20), and the flag, and
// limiter_kernel multiplies the row by an envelope e <= 1 that holds g |x| e under the ceiling. The weights h[2 W + 1]
// (raised cosine, sum 1, computed in f64 and rounded once) live in a device table. The report block (device ints, copied to
// pinned host memory with the call's samples): the largest 1 - e of a row as a float's bit pattern, then the count of
// samples with e < 1.
static constexpr int LIM_TILE = 2048;          // samples of a row per workgroup
static constexpr int LIM_MAXW = 480;           // 10 ms at 48000 Hz
static constexpr int LIM_SPAN = LIM_TILE + 4 * LIM_MAXW + 4;      // floats of LDS: the tile, 2 W of halo a side, alignment slack
static constexpr int LIM_PER = (LIM_SPAN + 255) / 256;            // span elements per thread
static constexpr int lim_o_maxred(int cap) { (void)cap; return 0; }
static constexpr int lim_o_count(int cap) { return cap; }
// true-peak ceiling: max |z| and the true peak of z = x e as bit patterns (folded by atomicMax), the final trim as f32
static constexpr int lim_o_pz(int cap) { return 2 * cap; }
static constexpr int lim_o_tz(int cap) { return 3 * cap; }
static constexpr int lim_o_trim(int cap) { return 4 * cap; }
static constexpr int lim_words(int cap) { return 5 * cap; }
static inline int limiter_window_samples(int fs, double window_ms) {
  const int W = (int)(window_ms * (double)fs / 1000.0 + 0.5);
  return W < 1 ? 1 : W;
}
struct LimP {
  const float* x; long x_bs;                   // delivered rows x[b][0 .. n_b), n_b = lens[b] * len_mul cut to x_cap
  const int* lens; int len_mul; long x_cap;
  const int* gq; int gcap;                     // device block of loudness_gain_kernel (ld_*): scale and flags per row
  const int* ctl;                              // control block: C at word 1
  const float* h; int W;                       // [2 W + 1] weights, W <= LIM_MAXW
  short* pcm; long p_bs; short* host;          // as pcm16_kernel's
  int* rep; int rcap;                          // report words (lim_o_*), cleared before the launch
  float* env; long e_bs;                       // test hook: e[b][0 .. n_b), or null
  // true-peak ceiling (limiter_kernel<true>): v[b][c] = max over the phases of |y[c Q + ph]| from true_peak_v_kernel, row
  // stride x_bs; z[b][i] = x e (x on rows that are not shaped), row stride x_bs, in the int16's place
  const float* v; float* z;
};
// pcm16_trim_kernel: the conversion of z behind the second true-peak pass
struct TrimP {
  const float* z; long z_bs;
  const int* lens; int len_mul;
  const int* gq; int gcap;                     // scale and flags per row
  int* ctl;                                    // control block: C at word 1; the report's scale is rewritten for shaped rows
  int* rep; int rcap;                          // pz, tz in; trim out
  short* pcm; long p_bs; short* host;
};

// ---- look-ahead limiter on streams (stream_limiter.h: stream_limiter_kernel; mode GAIN_LOUDNESS with pe_set_stream_limiter,
// DESIGN.md 4.9.1). A stream holds back D = 2 W samples so that what it hands out carries the envelope a whole-stream
// computation would give. What a call delivers is DATA like the window state: a pinned host block for `cap` rows that the
// kernel reads in place; the per-sample scales of the last SLM_TAIL samples of every stream live next to the float tails,
// stail[cap][2][SLM_TAIL], in the same two parities (stream_loudness_gain_kernel flips the word, one workgroup per row
// writes the other buffer). The report words (device; lim_o_maxred, lim_o_count) are cleared by the gain kernel.
//   control (pinned host)  nprev[cap] stream samples in front of this chunk (N of the call before), b0[cap] first stream
//                          sample this call delivers, cnt[cap] how many
static constexpr int SLM_TAIL = 4 * LIM_MAXW;  // scales kept per stream: the 4 W samples of past a delivery looks at
static constexpr int slm_o_b0(int cap) { return cap; }
static constexpr int slm_o_cnt(int cap) { return 2 * cap; }
static constexpr int slm_words(int cap) { return 3 * cap; }
static constexpr int slm_rep_words(int cap) { return 2 * cap; }
struct SlmP {
  const int* mctl;                             // limiter control block (pinned host)
  const int* lctl;                             // loudness control block: C at word 1
  const int* ldev;                             // loudness state block: the tail parity, flipped by the gain kernel
  const int* gq;                               // sgd_* words: g0, g1, R of this chunk
  int cap;
  const float* tail; int TW;                   // float tails tail[cap][2][TW] (SlP's)
  float* stail;                                // scale tails stail[cap][2][SLM_TAIL]
  const float* h; int W;                       // [2 W + 1] weights, W <= LIM_MAXW
  const int* st;                               // window state block (device): packed offsets and the host output pointers
  int* rep;                                    // report words [slm_rep_words(cap)]
  float* env; long e_bs;                       // test hook: e[b][stream sample], or null
};

// ---- G.711 companding of the delivered int16 (g711.h: g711_kernel, g711_flat_kernel; pe_set_sample_format).
// The format is part of the 'B' and 'C' graph keys; a stream chunk's encoder is launched outside the window stage's graph.
enum { G711_S16 = 0, G711_ULAW = 1, G711_ALAW = 2 };
static constexpr int G711_TPB = 256, G711_SPAN = 8 * G711_TPB;      // threads of 8 samples: samples per workgroup

// ---- fused MRF stage (mrf.h)
enum { MRF_RES = 1, MRF_KEEP = 2, MRF_FINAL = 4, MRF_INIT = 8, MRF_RESTAGE = 16 };
struct MrfPhase {        // one conv of one resblock chain; 12 ints wide (the kernel copies the table to LDS as ints)
  const float* bias;
  int ntaps, dil;
  int e;                 // columns of halo its OUTPUT still needs (0 for the last conv of a resblock)
  int src, dst;          // LDS activation buffers (0 = stage input window, 1 = chain buffer); dst < 0: none
  int flags;             // RES: + running x (registers); KEEP: result becomes the running x; FINAL: add to the MRF sum;
                         // INIT: running x = stage input (first conv of a resblock); RESTAGE: reload buffer 0 first
  int pad[4];
};
static_assert(sizeof(MrfPhase) == 48, "MrfPhase is read as 12 ints");
struct MrfP {
  const float* x; long x_bs; int x_cs;
  float* out; long o_bs; int o_cs;
  const int* lens; int len_mul;
  const MrfPhase* phases; int nphases;
  const float* wstream; int wfloats;
  const float* wunscale; // mrf_split_kernel, mode f16x3: per phase, the power of two that undoes the packing scale of its weights
  int C;                 // real channels (<= CP)
  int N;                 // output columns per workgroup (16 * NCG * OU)
  int wcols;             // window columns in use: hxa + N + the stage's halo (<= the row stride)
  int hxa;               // window column of the first output column (halo rounded up to 16)
  int cu_lo, cu_hi;      // 16-column units any phase needs: [cu_lo, cu_hi)
  int nleft, nhalo;      // halo units left of the output columns / in total
  float slope, alpha;
  int stride, n0off;     // workgroup bx owns window output columns [bx * stride - n0off, ... + N): (N, 0) without the tail
  // generator tail fused into the last stage (post_w != nullptr; out is not written): conv_post weights [C][7], waveform,
  // per-utterance peak (post.h: conv_post_kernel); stride = N - 6, n0off = 3
  const float* post_w; float* audio; long a_bs; unsigned* absmax; float post_slope;
};
static constexpr int MRF_NW = 8, MRF_PAD = 128, MRF_MAXPH = 24;
// row stride of the LDS window (== 16 mod 32). 32 channels with 4 output units per wave (N = 512, one utterance's last
// stage in ONE round over the chip) take the whole 160 KB: 2 x 32 x 624 floats + pads + table = 161 920 B
static constexpr int mrf_ws(int cp, int ou = 1) { return cp == 32 ? (ou >= 4 ? 624 : 528) : 304; }
static constexpr size_t mrf_smem_bytes(int cp, int ou = 1) {
  return ((size_t)2 * MRF_PAD + (size_t)2 * cp * mrf_ws(cp, ou) + MRF_MAXPH * 12) * sizeof(float);
}

}  // namespace pe
