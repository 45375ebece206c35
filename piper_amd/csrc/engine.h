// Host engine: owns the packed voice weights in HBM, the workspaces, one HIP stream, and issues the
// kernel sequence that replaces Ort::Session::Run() inside piper::synthesize
// (reference src/cpp/piper.cpp:386-388).
#pragma once
#include <cstdint>
#include <deque>
#include <limits>
#include <list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "pe_rt.h"
#include "engine_buffers.h"
#include "kernels/params.h"
#include "policy.h"
#include "weights.h"

namespace pe {

struct PackedConv {
  float* wp = nullptr;      // device, packed for conv_mfma_kernel
  float* wp16 = nullptr;    // device, the same in 16x16x4 fragment order (conv_splitk16_kernel), long-K convs only
  float* wpb = nullptr;     // device, 16-bit split-term fragments (conv_split_kernel), split matrix modes only
  const float* wunscale = nullptr;   // device: wpb holds the weights times 1 / *wunscale (a power of two; 1 except in mode f16x3)
  float* wpg4 = nullptr;    // device, gate convs over 192 channels in the 4x4x1 MFMA's order (gate4_kernel), or null
  float* bias = nullptr;    // device or null
  int rows = 0;             // GEMM rows (real)
  int mtiles = 0;           // packed 32-row tiles (padded to the block tile)
  int Cin = 0, nchunks = 0, ntaps = 1, dil = 1, padl = 0;
  int cfg = 0;              // tile configuration id
  bool gate = false;
  int split = 0;
  int up = 0, padT = 0;     // conv-transpose
  double macs_per_col = 0;  // algorithmic MACs per output column (for roofline accounting)
};

struct DdsW {               // one DDSConv (modules.py:81-129)
  std::vector<float*> dw_w, dw_b, g1, b1, g2, b2;
  std::vector<PackedConv> c1x1;
  std::vector<float*> w16;           // 1x1 weights in the 16x16x4 fragment order (dds_layer16_kernel)
};

struct ProfileRow {
  const char* name;
  double ms = 0;
  double flops = 0;
  long launches = 0;
  double bytes = 0;         // algorithmic HBM bytes (activations in + out + residual operands + weights), level 2 rows
};

struct NoiseIn {            // optional injected N(0,1) draws (parity tests); host pointers
  const float* noise_w = nullptr;  // [B][2][w_stride]
  int64_t w_stride = 0;
  const float* noise_z = nullptr;  // [B][inter][z_stride]
  int64_t z_stride = 0;
};

// A timing plan (include/piper_hip.h: pe_timing). Host pointers, any of them null: rate and forced per id,
// concatenated like the ids; target per utterance.
struct TimingIn {
  const float* rate = nullptr;
  const int32_t* forced = nullptr;
  const int32_t* target = nullptr;
};

// Per-utterance noise seeds (include/piper_hip.h: pe_seeds). Host pointers: seed[B]; use[B], null = every
// utterance of the call is seeded.
struct SeedsIn {
  const uint64_t* seed = nullptr;
  const uint8_t* use = nullptr;
};

// Per-utterance speaker blends and caller-supplied speaker vectors (include/piper_hip.h: pe_blend). Host
// pointers: count[B]; sid / weight, the components of all utterances concatenated in utterance order; vector[B][gin].
struct BlendIn {
  const int32_t* count = nullptr;
  const int64_t* sid = nullptr;
  const float* weight = nullptr;
  const float* vector = nullptr;
};

// Where the packed voice weights live. Default: one device allocation owned by the engine. A caller-provided arena
// (multi-GPU: a device buffer the host framework can hand to RCCL) receives them instead; with `skeleton` the engine only
// lays the arena out (same offsets as on the packing rank, derived from tensor shapes alone) and waits for its content
// to be broadcast into it -- no parsing of weight data, no packing, no upload on that rank.
struct ArenaSpec {
  void* base = nullptr;
  size_t bytes = 0;
  bool skeleton = false;
};

class Engine {
 public:
  Engine(const WeightSet& ws, int device, ArenaSpec arena = ArenaSpec{});
  ~Engine();
  // upper bound of the packed-weight arena for a voice (from tensor shapes), and what the engine actually used
  static size_t arena_bound(const WeightSet& ws);
  size_t arena_used() const { return arena_off_; }
  const void* arena_base() const { return arena_; }

  // Phase 1: copy inputs to HBM. ids: concatenated phoneme ids, offsets[B+1]. scales: one {noise_scale, length_scale,
  // noise_w} triple for every utterance, or (per_utt) [B][3], one triple per utterance. The triples are call inputs in
  // device memory like the ids: no captured graph depends on their values.
  // timing: the call's plan, checked before anything of the engine changes (a refused plan leaves a live stream alone). It
  // stays with the uploaded inputs -- every run() on them follows it -- and goes with the next upload.
  // seeds: per-utterance noise seeds, checked like the plan. They stay with the uploaded inputs -- every run() on them draws
  // the same noise again -- and go with the next upload of any kind.
  // blend: per-utterance speaker blends / vectors, checked like the plan (check_blend); they stay with the uploaded inputs
  // and go with the next upload of any kind.
  void upload(const int64_t* ids, const int64_t* offsets, int B, const float* scales,
              const int64_t* sids, const NoiseIn* noise, bool per_utt = false, const TimingIn* timing = nullptr,
              const SeedsIn* seeds = nullptr, const BlendIn* blend = nullptr);
  bool timed() const { return plan_on_; }
  bool seeded() const { return seeded_; }
  bool blended() const { return blended_; }
  // Refuses a blend the law does not cover -- a single-speaker voice, a count outside [-1, PE_BLEND_MAX], a component id
  // outside [0, num_speakers), a weight or vector element that is not finite, a missing array -- naming the utterance and
  // the component. Changes nothing of the engine.
  void check_blend(const BlendIn& blend, int B) const;
  int speaker_dim() const { return nspk_ > 1 ? gin_ : 0; }
  void speaker_embedding(int64_t sid, float* out, int64_t capacity);
  // test hook: speaker_blend_kernel alone, out[batch][gin] (sids may be null: 0)
  void debug_blend(const BlendIn& blend, int batch, const int64_t* sids, float* out);
  // test hook: duration_plan_kernel alone on caller-given logw rows (concatenated like ids, offsets[batch + 1]) with one
  // scales triple per utterance: the durations and w (concatenated) and the frame counts
  void debug_timing(const float* logw, const int64_t* offsets, int batch, const float* scales, const TimingIn* timing,
                    int32_t* dur_out, int32_t* frames_out, float* w_out);
  // Phase 2: the whole device pipeline (one host read-back of B frame counts in the middle).
  void run();
  // Phase 3: results to host (pinned buffers owned by the engine, valid until the next upload()).
  void download(bool want_audio, bool want_pcm);

  // Streaming decode of ONE utterance (BASELINE configs[4]; reference infer_onnx_streaming.py:76-124):
  // stream_begin runs everything up to the latent z (encoder, durations, flow) and returns the frame
  // count; every stream_next decodes the next `chunk_frames` frames through HiFiGAN on a window padded
  // with the generator's exact receptive half-width, so the concatenated chunks equal the unchunked
  // waveform (the reference pads by a heuristic 5-10 frames and does not). Returns false when done.
  int stream_begin(const int64_t* ids, int64_t n, const float scales[3], int64_t sid, const NoiseIn* noise,
                   const TimingIn* timing = nullptr, const SeedsIn* seeds = nullptr, const BlendIn* blend = nullptr);
  bool stream_next(int chunk_frames, const float** audio, const int16_t** pcm, int64_t* nsamples);
  // halo of a stream window in frames: the generator's receptive half-width, plus one frame while an output rate is set
  // (the resampler needs exact native samples up to K <= hop beyond a chunk's edges)
  int decoder_halo_frames() const { return halo_frames_ + (rs_on_ ? 1 : 0); }

  // Output-rate conversion on the device (kernels/resample.h): every waveform the engine delivers -- whole utterances and
  // stream chunks -- is resampled from the voice's rate to `output` by a polyphase Kaiser-windowed sinc before the int16
  // conversion, whose peak is then the RESAMPLED waveform's. native == 0: the rate of the voice's header (an .onnx has
  // none: the caller passes the value of its .onnx.json); output == 0 or == native: off, the engine is exactly the
  // native-rate engine. Throws, and changes nothing, for a rate pair outside the supported set (8000 <= output <= 48000,
  // L = output / gcd <= 640, half-width K <= hop), a native rate that contradicts the header, or while a stream, a batch
  // stream or a stream pool is live. A change drops every captured graph.
  void set_output_rate(int native, int output);
  // host only: geometry and (table != null) the f64 polyphase table of a rate pair; the one place the filter is built
  static void resample_filter(int native, int output, int& L, int& M, int& K, int& Tp, std::vector<double>* table);
  int native_rate() const { return rs_native_ ? rs_native_ : arch_[A_SR]; }
  int output_rate() const { return rs_on_ ? rs_out_ : native_rate(); }
  int resample_half_width() const { return rs_on_ ? rs_K_ : 0; }
  // output samples of s native ones: ceil(s * L / M) (s itself at the native rate)
  int64_t out_samples(int64_t s) const { return rs_on_ ? (s * rs_L_ + rs_M_ - 1) / rs_M_ : s; }
  // test hook: resample_kernel with the current rate pair on host rows x[batch][stride]: row b holds vlen[b] native samples
  // whose first one has native index origin[b]; outputs n0[b] .. n0[b] + count[b] - 1 go to out[b][out_stride]
  void debug_resample(const float* x, int batch, int64_t stride, const int32_t* vlen, const int64_t* n0, const int32_t* count,
                      const int64_t* origin, float* out, int64_t out_stride);

  // Target loudness of whole utterances (kernels/loudness.h). Off, the default, is the reference's rule: every
  // utterance scaled by 32767 / max(0.01, its peak). On: every whole-utterance call -- synthesize, the batch calls, run /
  // fetch -- measures the gated integrated loudness L (ITU-R BS.1770-4, mono) of each float waveform it delivers, at the
  // delivered rate, on the device, and converts with scale = 32767 min(10^((target - L) / 20), C / peak),
  // C = 10^(ceiling_db / 20) a ceiling on the sample peak, or with set_loudness_ceiling(PEAK_TRUE) on the true peak (below:
  // `peak` is then max(sample peak, true peak)); an utterance whose loudness cannot be measured (silence) keeps
  // scale 32767. The delivered floats are not touched and stream chunks keep their own rules. Throws, and changes nothing,
  // for a target outside [-40, -5] LUFS, a ceiling outside [-20, 0] dB, values that are not finite, or a voice whose
  // delivered rate is unknown or outside [4000, 192000] Hz. target and ceiling are data the kernels read in place; on / off
  // is part of the graph keys of the stages that end in the conversion.
  void set_loudness(bool on, float target_lufs, float ceiling_db);
  bool loudness_on() const { return ld_on_; }
  float loudness_target() const { return ld_T_; }
  float loudness_ceiling_db() const { return ld_cdb_; }
  // per utterance of the last fetched call: loudness (LUFS, -inf: not measurable), scale, peak, LOUD_* flags; returns the
  // utterances (0: that call ran with the setting off)
  int last_loudness(float* lufs, float* scale, float* peak, int32_t* flags, int64_t capacity);
  // host only: the K-weighting biquads at rate fs, shelf {b0, b1, b2, a1, a2} then high-pass {b0, b1, b2, a1, a2}
  static void loudness_filter(int fs, double coef[10]);
  // What the ceiling of the target loudness holds (kernels/true_peak.h). PEAK_SAMPLE, the default: the
  // largest |sample|. PEAK_TRUE: the true peak of ITU-R BS.1770-4 Annex 2 as well -- the largest |sample| of the delivered
  // floats interpolated Q = ceil(192000 / fs) times by the resampler's own filter for the pair fs -> Q fs, measured on the
  // device by one more launch per call. The kind may be set with the loudness off (it is remembered) and while a stream is
  // live (streams do not see it). Throws, and changes nothing, for an unknown kind, or for PEAK_TRUE while the loudness is on
  // at a delivered rate outside [8000, 48000] Hz; set_loudness and set_output_rate refuse what would make that true. The
  // kind is part of the graph keys next to on / off: the three sets of graphs stay cached.
  void set_loudness_ceiling(int kind);
  int loudness_ceiling_kind() const { return ld_kind_; }
  static int true_peak_oversample(int fs) { return fs > 0 ? (192000 + fs - 1) / fs : 0; }
  // per utterance of the last fetched call: the true peak t; returns the utterances (0: that call did not run with PEAK_TRUE)
  int last_true_peak(float* t, int64_t capacity);
  // host only: the interpolator at rate fs in f64, coef[ph * 2 K + k] (kernels/true_peak.h); throws outside [8000, 48000]
  static void true_peak_filter(int fs, int& Q, int& K, std::vector<double>& coef);
  // test hook: true_peak_kernel alone on host rows x[batch][stride], row b holding valid[b] samples at rate fs
  void debug_true_peak(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float* t);
  // Look-ahead limiter of the target loudness (kernels/limiter.h). Off, the default: a row whose peak would
  // pass the ceiling at the gain of its target is lowered as a whole (LIMITED). On: such a row keeps that gain and a
  // zero-phase envelope of window_ms (in [1, 10], W = round(window_ms fs / 1000) samples a side) turns down the
  // neighbourhood of its peaks only (SHAPED); every other row is delivered bit for bit as without it. The floats a call
  // returns are never shaped, only the int16. Whole-utterance calls only. The setting is remembered while the loudness is
  // off. With PEAK_TRUE the envelope is formed from max(|x[i]|, v[i - 1], v[i]), v the per-position maxima of the
  // true-peak interpolation, the shaped floats z = x e get a true-peak pass of their own and a last conversion kernel trims
  // the scale to C / max(p_z, t_z) where that is the smaller term (three launches more; the existing rate refusals of
  // PEAK_TRUE hold). Throws, and changes nothing, for a window outside [1, 10] ms or not finite. On / off is part of the
  // graph keys; W is a kernel argument, so a new window drops the graphs.
  void set_loudness_limiter(bool on, float window_ms);
  bool loudness_limiter_on() const { return lim_on_; }
  float loudness_limiter_ms() const { return lim_ms_; }
  int loudness_limiter_window() const { return output_rate() > 0 ? limiter_window_samples(output_rate(), lim_ms_) : 0; }
  // per utterance of the last fetched call: 1 - min e, the count of samples with e < 1, the final trim (1: the sample-peak
  // ceiling needs none: 1); returns the utterances (0: that call did not run with the limiter)
  int last_limiter(float* max_reduction, int32_t* shaped_samples, float* trim, int64_t capacity);
  // host only: W and the 2 W + 1 weights in f64, before the rounding to f32; throws outside [1, 10] ms or fs outside the
  // loudness's rates
  static void limiter_window(int fs, float window_ms, int& W, std::vector<double>& coef);
  // test hook: limiter_kernel alone on host rows x[batch][stride], row b holding valid[b] samples at rate fs with the gain
  // g[b] (scale = 32767 g[b] in f32; the row is shaped iff C / max |x| < g[b]); env[batch][stride] receives e and
  // pcm[batch][stride] the int16 (entries behind a row's end are left alone)
  void debug_limiter(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, const float* g, float ceiling_db,
                     int kind, float window_ms, float* env, int16_t* pcm);
  // test hook: the two loudness kernels alone on host rows x[batch][stride], row b holding valid[b] samples at rate fs
  void debug_loudness(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float target, float ceiling_db,
                      float* lufs, float* scale, int32_t* flags);

  // The sample format of what is delivered (kernels/g711.h). G711_S16, the default: int16 and floats, as ever.
  // G711_ULAW / G711_ALAW: every whole-utterance call and every chunk of every kind of stream ALSO delivers one G.711 code
  // per delivered int16 sample, packed under the same sample offsets (last_codes); the int16 and the floats stay bit for bit
  // what they are without it. Whole utterances: g711_kernel is the last launch of the delivery stage on every route, one
  // launch more per call, the codes fetched by one copy in download. Batch stream and pool: the chunk's int16 go to a device
  // staging buffer and reach the host by one copy, g711_flat_kernel behind the stage writes the codes, one launch more per
  // chunk. The one-utterance stream converts on the host, as it does its int16. Throws, and changes nothing, for an unknown
  // value, or while a stream is live / a pool is open on the handle (set_output_rate's rule). The format is part of the
  // 'B' and 'C' graph keys: nothing is dropped, the sets of graphs stay cached side by side.
  void set_sample_format(int format);
  int sample_format() const { return fmt_; }
  // which = 0: the codes of the last fetched whole-utterance call; 1: of the last chunk of any kind of stream. Returns the
  // rows (offsets[rows + 1]); 0, with null views, when that call ran with G711_S16. Views are valid until the next call.
  int last_codes(int which, const uint8_t** codes, const int64_t** offsets);
  // test hook: the rows form (x[batch][stride], row b holding valid[b] samples) or the flat form (batch 1) of the encoder
  // alone; out[out_capacity] is uploaded, written by the kernel and read back whole
  void debug_g711(int format, bool flat, const int16_t* x, int batch, int64_t stride, const int32_t* valid, uint8_t* out,
                  int64_t out_capacity);

  // The int16 level of stream chunks (kernels/params.h: GAIN_*). GAIN_CHUNK, the default, is the
  // reference's rule: every chunk scaled by 32767 / max(0.01, its own peak). GAIN_FIXED: 32767 / max(0.01, peak) for every
  // sample. GAIN_RUNNING: every stream -- the one-utterance stream, a batch-stream row, a pool slot -- carries a running
  // peak r that starts at max(0.01, peak) and only grows: a chunk with peak c is scaled by 32767 / max(r, c), reached from
  // the previous chunk's gain over the chunk's first ramp_samples samples. The delivered floats are not touched. Throws,
  // and changes nothing, for an unknown mode, a peak that is not finite (or < 0; fixed: <= 0), a ramp outside [0, 65536],
  // or while a stream, a batch stream or a pool with an occupied slot is live. peak and ramp are data; the mode is part
  // of the window stage's graph key.
  void set_stream_gain(int mode, float peak, int ramp_samples);
  int stream_gain_mode() const { return gain_mode_; }
  float stream_gain_peak() const { return gain_peak_; }
  int stream_gain_ramp() const { return gain_ramp_; }
  // Streams at a target loudness (mode GAIN_LOUDNESS): a running BS.1770-4 loudness per stream sets every
  // chunk's gain toward target_lufs under the peak ceiling; prior_lufs NaN: none. Refused, with nothing changed, for values
  // out of range, an unknown delivered rate, or while a stream is live / a pool slot occupied.
  void set_stream_loudness(float target_lufs, float ceiling_db, float prior_lufs, int ramp_samples);
  float stream_loudness_target() const { return sl_T_; }
  float stream_loudness_ceiling() const { return sl_cdb_; }
  float stream_loudness_prior() const { return sl_prior_; }
  // the report of the last chunk call in that mode: per row the running loudness (-inf: not measurable), the gain at the
  // chunk's end, the running peak and the flags; rows that delivered nothing report their stream's last state
  int stream_last_loudness(float* lufs, float* gain, float* peak, int32_t* flags, int64_t capacity);
  // test hook: the two stream loudness kernels and chunk_pcm_gain_kernel chunk after chunk on caller-given rows
  // x[batch][stride] at rate fs; chunks[n_chunks][batch] = the chunk lengths (zeros allowed, a row's sum <= stride). Out per
  // chunk and row lufs / g0 / g1 / flags [n_chunks][batch], and the int16 pcm[batch][stride].
  void debug_stream_loudness(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                             float ceiling_db, float prior_lufs, int ramp_samples, float* lufs, float* g0, float* g1, int32_t* flags,
                             int16_t* pcm);
  // end-of-chunk gain and the level it came from, per row of the last chunk call of any kind; returns the rows
  int stream_last_gains(float* gain, float* peak, int64_t capacity);
  // Look-ahead limiter on streams at a target loudness (kernels/stream_limiter.h). Acts in GAIN_LOUDNESS
  // only (remembered otherwise): a chunk whose cap is under its target gain keeps that gain (LIMITED | SHAPED) and the
  // envelope of 4.6.1, formed over the WHOLE stream, turns down the neighbourhood of the peaks; every stream holds back
  // D = 2 W samples for it, W = round(window_ms fs / 1000) at the delivered rate, and hands them out with the chunk that
  // consumes its last frame. Refused, with nothing changed, for a window outside [1, 10] ms or not finite, an unknown
  // delivered rate, or while a stream is live / a pool slot occupied. On / off and W are part of the window stages' graph keys.
  void set_stream_limiter(bool on, float window_ms);
  bool stream_limiter_on() const { return slim_on_; }
  float stream_limiter_ms() const { return slim_ms_; }
  int stream_limiter_window() const { return output_rate() > 0 ? limiter_window_samples(output_rate(), slim_ms_) : 0; }
  // per row of the last chunk call with the limiter: 1 - min e and the count of e < 1 over the samples that call delivered;
  // returns the rows (0: that call did not run with the limiter)
  int stream_last_limiter(float* max_reduction, int32_t* shaped_samples, int64_t capacity);
  // test hook: debug_stream_loudness with the limiter of window_ms on -- the production kernels chunk after chunk; a row ends
  // with its last chunk of length > 0. Also out: delivered[n_chunks][batch] samples handed out per call and row,
  // env[batch][stride] = e per stream sample; pcm[batch][stride] holds the int16 in delivery order.
  void debug_stream_limiter(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                            float ceiling_db, float prior_lufs, int ramp_samples, float window_ms, float* lufs, float* g0, float* g1,
                            int32_t* flags, int32_t* delivered, float* env, int16_t* pcm);

  // Streaming decode of a whole BATCH in lock step: stream_begin_batch is upload (one scales triple per utterance) + text
  // encoder + durations + flow for B utterances, once; the latent stays resident. Every stream_next_batch decodes the
  // next `chunk_frames` frames of every utterance that has frames left as ONE batched generator pass on exact-halo
  // windows and delivers each utterance's chunk, peak-normalised over its own samples on the device, packed back to
  // back in pinned host memory. Utterances finish at different calls: a finished one keeps a one-frame window whose
  // output is not delivered (the generator's kernels have only ever seen lengths >= 1). Any other call that uploads
  // inputs ends the stream. Views are valid until the next call.
  struct StreamChunk {
    int batch = 0;
    const int64_t* sample_offsets = nullptr;    // [batch + 1] of THIS chunk
    const int16_t* pcm = nullptr;
    const float* audio = nullptr;               // null unless wanted
    const int32_t* frames_done = nullptr;       // [batch]
  };
  const std::vector<int32_t>& stream_begin_batch(const int64_t* ids, const int64_t* offsets, int B, const float* scales,
                                                 const int64_t* sids, const NoiseIn* noise, const TimingIn* timing = nullptr,
                                                 const SeedsIn* seeds = nullptr, const BlendIn* blend = nullptr);
  void stream_next_batch(int chunk_frames, bool want_audio, StreamChunk& out);

  // Stream pool: a fixed number of slots whose latents and decoder conditioning rows live in storage OWNED BY THE POOL,
  // outside both stage workspaces, so that listeners join and leave while others are in mid-stream. stream_pool_join is
  // stream_begin_batch's front half for n newcomers (upload, text encoder, durations, flow -- it may overwrite every
  // workspace) plus stream_adopt_kernel, which moves their latents into the lowest free slots in input order.
  // stream_pool_next is ONE batched window stage over all slots: every live slot advances from its own position by
  // chunk_frames, or by per_slot[s] where that is > 0; an empty, finished or left slot keeps the one-frame window of its
  // own (zeroed or stale) row with nothing delivered. A slot whose last frame has been delivered is free from the next
  // call on; its frames_done stays readable until it is reused. The pool survives every other call on the handle --
  // nothing it needs between two next calls lives in a workspace -- and is freed by stream_pool_close and the destructor.
  // A join that fails (too few free slots, an utterance over max_frames, an upload error) leaves the pool as it was.
  int stream_pool_open(int slots, int max_frames);                 // returns the halo in frames
  void stream_pool_join(const int64_t* ids, const int64_t* offsets, int n, const float* scales, const int64_t* sids,
                        const NoiseIn* noise, int32_t* slot_of, int32_t* total_frames, const TimingIn* timing = nullptr,
                        const SeedsIn* seeds = nullptr, const BlendIn* blend = nullptr);
  void stream_pool_next(int chunk_frames, const int32_t* per_slot, bool want_audio, StreamChunk& out);   // out.batch == slots
  void stream_pool_leave(int slot);
  void stream_pool_close();
  // host view: slots (0: no pool; then the arrays are not touched), per slot total frames, frames delivered, 1 = occupied
  int stream_pool_state(int32_t* frames, int32_t* frames_done, int32_t* live) const;
  void stream_pool_require() const;                                // throws "no stream pool"

  int batch() const { return B_; }
  const std::vector<int64_t>& sample_offsets() { finish_run(); return sample_off_; }
  const float* audio_host() const { return h_audio_.get(); }
  const int16_t* pcm_host() const { return pcm_zc_live_ ? h_pcm_zc_.get() : h_pcm_.get(); }
  const std::vector<int32_t>& durations_host();   // concatenated per id, same offsets as ids
  const std::vector<int32_t>& frames_host() { finish_run(); return frames_h_; }
  void debug_tensor(const std::string& name, int b, std::vector<float>& out, int* rows, int* cols);
  // test hook: n draws of the engine's N(0,1) generator (randn_kernel) at sampling site 0/1 with the engine's
  // seed and the given call counter, starting at logical row `row` of the site's stream: exactly what run() would draw
  // at that counter for (utterance, channel) = row, columns 0 .. n-1
  void debug_randn(int site, uint64_t call, int64_t row, int64_t n, float* out);
  uint64_t rng_call() const { return call_; }
  long run_launches() const { return run_launches_; }          // kernel launches (graph nodes) of the last run()
  // speculative stage-B sizing (see below): runs issued with a guessed frame bucket / guesses that were too small and
  // cost a second pass of stage B, since the engine was created
  long speculation_runs() const { return spec_runs_; }
  long speculation_misses() const { return spec_misses_; }
  // XCC id of workgroups 0..63 of a 1-D launch as seen at engine creation, and the round-robin period (0: not a round-robin)
  const int* xcc_pattern(int* period) const { if (period) *period = xcd_period_; return xcc_of_; }

  void set_seed(uint64_t s) { seed_ = s; }
  uint64_t seed() const { return seed_; }
  void set_use_graphs(bool on) { use_graphs_ = on; }
  // level 0 off; 1 = one HIP-event pair per pipeline stage; 2 = additionally one pair around every
  // conv/attention/layer-norm launch (per-kernel rows after the five stage rows)
  void set_profile(int level);
  const std::vector<ProfileRow>& profile();
  void reset_profile();
  hipStream_t stream() const { return stream_; }
  const int32_t* arch() const { return arch_; }
  int sample_rate() const { return arch_[A_SR]; }
  int hop() const { return hop_; }
  size_t weight_bytes() const { return weight_bytes_; }

 private:
  // every threshold and A/B knob that picks a kernel form (policy.h; read from the environment at engine creation)
  LaunchPolicy pol_;
  // ---- setup
  void init(const WeightSet& ws);
  float* dev_copy(const std::vector<float>& v);
  float* dev_alloc(size_t nfloats, const float* src);   // bump allocation in the weight arena (+ upload unless skeleton)
  char* arena_ = nullptr; size_t arena_bytes_ = 0, arena_off_ = 0;
  bool arena_owned_ = false, skeleton_ = false;
  float* dev_tensor(const WeightSet& ws, const std::string& name);
  PackedConv pack_conv(const WeightSet& ws, const std::string& wname, const std::string& bname, int dil,
                       int padl_override, bool gate, int in_rev, int out_rev);
  PackedConv pack_qkv(const WeightSet& ws, const std::string& prefix, float** out16 = nullptr);
  PackedConv pack_convT(const WeightSet& ws, const std::string& prefix, int stride);
  PackedConv pack_matrix(const std::vector<float>& W, int rows, int Cin, int ntaps,
                         const std::vector<float>* bias, int nbias, int dil, int padl, bool gate, int split);
  DdsW load_dds(const WeightSet& ws, const std::string& prefix);
  // A side buffer (engine_buffers.h) replaced by one of exactly n elements, then filled. idle: first wait for the stream
  // and, where the buffer exists -- its address may sit inside a captured graph --, drop the graphs; false: the caller has
  // seen to both. what / what_bytes: Buffer::grow's out-of-memory text. (engine_internal.h)
  enum Fill { FILL_NONE, FILL_ZERO, FILL_POISON, FILL_POISON_OR_ZERO };      // POISON: under LaunchPolicy::debug_poison only
  template <class Buf>
  void side_alloc(Buf& b, size_t n, bool idle, Fill fill, const char* what = nullptr, size_t what_bytes = 0);
  void ensure_stage_a(int B, int Tmax);
  void ensure_stage_b(int Fmax, int batch = 0);

  // ---- launches
  struct View { float* p; long bs; int cs; };
  // what a conv launch may set beyond its operands: input leaky-relu slope, output activation, residual, second output
  // (WN skip rows), accumulate mode and scale of the MRF epilogues, a per-utterance bias (speaker conditioning)
  struct ConvOpt {
    float in_slope = 1.f; int act = 0; View res{nullptr, 0, 0}; View out2{nullptr, 0, 0}; int mode = 0; float alpha = 1.f;
    const float* bias2 = nullptr; int bias2_bs = 0;
  };
  void conv(const PackedConv& pc, View x, View out, const int* lens, int len_mul, int Lmax, int epi, const ConvOpt& o);
  void conv(const PackedConv& pc, View x, View out, const int* lens, int len_mul, int Lmax, int epi) { conv(pc, x, out, lens, len_mul, Lmax, epi, ConvOpt()); }
  // One conv launch decided once (engine_internal.h: ConvPlan): kernel form, grid, LDS, whether it may ride in a grouped
  // launch. A pure function of the packed conv, the column bound, the epilogue, B_, the policy and the matrix mode.
  struct ConvPlan plan_conv(const PackedConv& pc, int Lmax, int epi, bool stage_tiled) const;
  // Grouped launches (conv_splitk_group_kernel): between group_begin() and group_end() conv() records the launch instead
  // of issuing it; group_end() issues all of them (<= 3 independent convs of one launch shape) as one launch.
  bool grouping_ = false;
  bool stage_tiled_ = false;            // the stage being issued keeps the tiled kernel (set for the stage's scope by issue_decoder from its schedule)
  bool group_tiled_ = false;            // the open group goes to the TILED kernel (conv_mfma_group_kernel), cfg = group_cfg_
  int group_cfg_ = 0;
  std::vector<struct ConvP> group_;
  double group_flops_ = 0, group_bytes_ = 0;
  int group_ncols_ = 0;
  void group_begin(bool tiled = false);
  void group_end();
  // the recorded convs as ONE GEMM over their concatenated K, summed: out = (sum_j (res_j + conv_j)) * alpha
  bool can_group_sum() const;
  void group_end_sum(View out, const float* bias_sum, float alpha);
  void layer_norm(View in, View out, const float* g, const float* b, int C, const int* lens, int Lmax);
  // options of one DDSConv run: ConvFlow.pre folded into the first layer, a 1x1 conv (+ spline) fused after the last
  struct DdsOpt {
    const float* pre_z = nullptr; long pre_z_bs = 0; const float* pre_w = nullptr; const float* pre_b = nullptr;
    const float* z_scale = nullptr;   // per-utterance noise_scale_w, stride 3 (&d_scales_[2]); null: 1
    const float* post_w16 = nullptr; const float* post_bias = nullptr; int post_rows = 0;
    View post_out{nullptr, 0, 0};
    const float* zin = nullptr; long zin_bs = 0; int z_cs = 0, c0 = 0, c1 = 1; float* zout = nullptr; long zout_bs = 0;
  };
  void dds(const DdsW& d, View in, View out, View tmp, const DdsOpt* opt = nullptr);
  double dds_bytes(const struct DdsP& p) const;
  double cols_ids_ = 0, cols_frames_ = 0;     // ids / frames of the call being issued (algorithmic byte counts of the profile rows)
  void dds_params(const DdsW& d, View in, View out, View tmp, const DdsOpt* opt, std::vector<struct DdsP>& list);
  float* pack16(const std::vector<float>& W, int rows, int K);    // [16-row tile][q][lane][4] (dds_layer16_kernel)
  // every pack16 matrix with K = 96 / 192 is also packed for the 4x4x1 MFMA of the 4-column kernels (kernels/col4.h):
  // [64-row tile][k quad][lane][4]; looked up by its pack16 pointer (null: not packed)
  float* pack4(const std::vector<float>& W, int rows, int K);
  std::unordered_map<const float*, const float*> w4_of_;
  // fused FFN for small calls (kernels/ffn.h): per-slice weight orders, the partial-output buffer [b][slice][192][Tp]
  // (allocated once for LaunchPolicy::ffn_max_cols columns), and the buffer that holds the encoder output after the last layer (the
  // fused path ping-pongs x_ / y_: lngemm4_kernel must not write LN(y) over the residual other parts still read)
  const float* pack_ffn1(const WeightSet& ws, const std::string& wname);
  const float* pack_ffn2(const WeightSet& ws, const std::string& wname);
  DevBuf<float> ffn_parts_;
  bool stage_a_ffn_fused() const;
  float* stage_a_enc_out() const;
  const float* w4_of(const float* w16) const { auto it = w4_of_.find(w16); return it == w4_of_.end() ? nullptr : it->second; }
  float* dp_proj16_ = nullptr;
  float* dp_pre16_ = nullptr;
  // enc_p.proj and dp.pre stacked for lngemm4_kernel (small calls): pack4 matrix, stacked bias, rows of proj
  float* projpre4_ = nullptr; float* projpre_bias_ = nullptr; int projpre_split_ = 0;
  void colchain(const struct ColP& p, int B, int Lmax, double flops);
  // The route of every coupling layer of a call, decided once per issue_flow (engine_internal.h: FlowLayerPlan): a pure
  // function of the packed layers (Rcl's *_ok flags), the policy and the call's size.
  std::vector<struct FlowLayerPlan> plan_flow(int B, int Fmax, double fsum) const;
  // The three colchain launches that are not plain convs; they alone fill ColP for their mode (engine_launch.cpp).
  struct EncLayer; struct Rcl;
  void conv_o_ln(const EncLayer& e, View att, View x, int B, int T, double tsum);
  void wn_res_skip4(const Rcl& r, int layer, const struct FlowLayerPlan& pl, View x0, View facts, View fh, View fskip, int B, int Fmax, double fsum);
  void coupling_chain(const Rcl& r, const Rcl* next, const struct FlowLayerPlan& pl, View x1, View facts, View fskip, View fh, int B, int Fmax, double fsum);
  bool conv1x1_col4(const float* w16, const float* bias, int rows, View in, View out, const int* lens, int B, int Lmax,
                    double flops, const float* bias2 = nullptr, long bias2_bs = 0, const float* w4direct = nullptr, int kin = 192,
                    long max_cols = 0);
  const float* pack4_conv_pad192(const WeightSet& ws, const std::string& wname, int in_rev, int out_rev);
  void pack_gate4pre(const WeightSet& ws, const std::string& prefix, bool odd, Rcl& r);
  void pack_post4(const WeightSet& ws, const std::string& prefix, bool odd, Rcl& r);
  // the first gate conv of coupling layer `r` with its pre composed in, over x0 (gate4pre_kernel); b2 = the speaker bias or null
  void gate_pre(const Rcl& r, View x0, View out, const int* lens, int Lmax, double cols, const float* b2);
  // second: rows >= split of a STACKED pack4 matrix (w4) are another conv over the same LN(y), written to out2 with the
  // per-utterance bias vector bias2 on top (enc_p.proj + dp.pre of a small call in one launch)
  struct LnSecond { const float* w4 = nullptr; int split = 0; View out2{nullptr, 0, 0}; const float* bias2 = nullptr; long bias2_bs = 0; };
  void lngemm(View y, const float* g, const float* b, View x, const float* w16, const float* bias, int rows, View out,
              int T, double flops, const float* parts = nullptr, int nparts = 0, const float* pbias = nullptr,
              const LnSecond* second = nullptr);
  bool proj_pre_stacked() const;     // this call runs enc_p.proj and dp.pre as one lngemm4_kernel launch
  float* pack16_conv(const WeightSet& ws, const std::string& wname, int in_rev, int out_rev);
  // XCD dispatch pattern of this device (xcc_probe_kernel at engine creation): XCC id of workgroups 0..63 of a 1-D launch,
  // and the period P when it is a round-robin over P XCDs (0: anything else -- the 4-column kernels then use tile = id)
  int xcc_of_[64] = {0};
  int xcd_period_ = 0;
  void probe_xcds();
  // YT | P | red | ZL (kernels/col4.h, dds4.h); with_x0: colchain4_kernel's pre_part keeps x0 as [4][96 + 4] behind them (col4.h: YTP = P + 4 * C4_H * NC + 32 + 64 * 4)
  static size_t col4_smem(bool with_x0 = false) { return ((size_t)4 * 196 + 4 * 192 * 4 + 32 + 64 * 4 + (with_x0 ? 4 * (96 + 4) : 0)) * sizeof(float); }
  void issue_stage_a();
  void issue_stage_b();
  void issue_flow();
  void issue_window();
  // zero_absmax: a window pass (the peaks are cleared here, the PCM is not written to the zero-copy host buffer);
  // with_pcm16 = false additionally leaves out the whole-window pcm16_kernel (batch streaming delivers per chunk)
  // cond / cond_bs: the decoder's conditioning rows and their stride (null: this call's, in cond_)
  void issue_decoder(const float* zsrc, const int* lens, int Fmax, double fsum, bool zero_absmax, bool with_pcm16 = true,
                     const float* cond = nullptr, int cond_bs = 0);
  void run_stage(char which, const std::string& key);
  void dispatch_stage(char which);
  void drop_graphs();
  // Speculative stage B (one to LaunchPolicy::spec_max_batch utterances): the frame count F is the path's only data-dependent
  // shape and normally costs a host round trip in the middle of the pipeline. When a previous run of this engine gives
  // a frames-per-id estimate, stage B is launched right behind stage A for a guessed bucket (kernels read the true
  // lengths from device memory, clamped to the allocated capacity), and the guess is verified when the results are
  // fetched; a wrong guess re-runs stage B with the right size.
  bool finish_run();                 // completes a speculative run; false if stage B had to be re-run
  void finish_stage_b_sizes();
  bool spec_pending_ = false;
  int spec_fg_ = 0;
  int spec_fg_force_ = 0;            // warm-up only: the frame bucket the next speculative run is issued for
  // The guess = (slowly decaying maximum of the frames-per-id ratios seen so far) x margin. The margin adapts: a miss
  // widens it (x 1.15, up to 1.5), 32 hits in a row narrow it again (down to 1.10); four misses within 16 speculative
  // runs switch speculation off for the next 64 calls (texts whose lengths vary too much for the estimate to hold).
  float last_ratio_ = 0.f, spec_margin_ = 1.10f;
  long spec_misses_ = 0, spec_runs_ = 0;
  int spec_hit_streak_ = 0, spec_recent_misses_ = 0, spec_recent_runs_ = 0, spec_cooldown_ = 0;
  int* d_framesc_ = nullptr;
  const int* lens_b_ = nullptr;      // frame counts stage B reads: d_frames_, or d_framesc_ on a speculative run
  void prof_begin();
  void prof_end(int row, double flops);

  int32_t arch_[ARCH_INTS];
  int device_ = 0;
  hipStream_t stream_ = nullptr;
  int H_, C_, FC_, nh_, dk_, nlayers_, ksz_, window_, hop_, U_;
  std::vector<void*> owned_;          // device allocations to free
  size_t weight_bytes_ = 0;

  // weights
  float* emb_ = nullptr;
  float* emb_g_ = nullptr;
  struct EncLayer {
    PackedConv qkv, o, f1, f2;
    float* o16 = nullptr;                        // conv_o in pack16 order (colchain_kernel)
    float* qkv16 = nullptr;                      // the fused q/k/v matrix in pack16 order (lngemm_kernel)
    const float *f1p = nullptr, *f2p = nullptr;   // conv_1 / conv_2 in ffn_kernel's per-slice order (kernels/ffn.h; null: not packed)
    float *relk, *relv, *g1, *b1, *g2, *b2;
  };
  std::vector<EncLayer> enc_;
  PackedConv enc_proj_;
  float* enc_proj16_ = nullptr;                  // pack16 order (lngemm_kernel)
  PackedConv dp_pre_, dp_proj_;
  DdsW dp_dds_;
  struct CFlow {
    float *pre_w, *pre_b;
    DdsW dds;
    PackedConv proj;
    float* proj16 = nullptr;             // proj in the 16x16x4 fragment order (fused after the last DDSConv layer)
  };
  std::vector<CFlow> cflows_;
  float ea_m0_ = 0, ea_es0_ = 1;
  float *ea_dev_m_ = nullptr, *ea_dev_logs_ = nullptr;
 public:
  // skeleton engines: call once the arena content has been broadcast into place (fetches the few host-side scalars)
  void arena_ready();
 private:
  struct Rcl {
    PackedConv pre, post;
    float *pre16 = nullptr, *post16 = nullptr;   // the same two 1x1 convs in pack16 order (colchain_kernel)
    const float* pre4pad = nullptr;               // the first layer's pre in pack4 order, K padded to 192 (colchain4_kernel mode 3)
    std::vector<PackedConv> in, rs;
    std::vector<const float*> rs4;   // the res/skip 1x1 convs in pack4 order (colchain4_kernel mode 2; null: not packed)
    // pre composed into the first gate conv (gate4pre_kernel, kernels/gate4.h; null: shapes it is not built for): the
    // matrix Wg_k . Wp in gate4 order over 96 channels, b_gate + sum_k Wg_k . b_pre, and the per-tap table behind it
    const float* gpre4 = nullptr; const float* gpre_bias = nullptr; const float* gpre_tapb = nullptr;
    // post composed into the skip convs (engine_pack.cpp pack_post4; empty: shapes it is not built for). Per WN layer j the
    // pack4 matrix [Wres_j ; M_j] (288 rows; the last layer: M_j alone, 96 rows) with M_j = Wpost . Wskip_j in post's packed
    // row order, and its bias [bres_j ; c_j], c_j = Wpost . bskip_j (+ bpost for j = 0)
    std::vector<const float*> rsp4, rsp_bias;
    bool front4_ok = false;          // the last res/skip conv, post and the next layer's pre are packed for the 4-column chain launch
    bool compose_pre_ok = false;     // pre is packed into the first gate conv, and the first res/skip launch can write the whole hidden state
    bool compose_post_ok = false;    // post is packed into the skip rows of every res/skip conv
    int in_off, out_off;             // channel offsets of x0 / x1 in the physical (unflipped) layout
  };
  std::vector<Rcl> rcls_;            // in execution order
  PackedConv dec_pre_;
  struct UpStage {
    PackedConv up;
    int rate, ch;
    std::vector<std::vector<PackedConv>> rb;   // [resblock][conv] (ResBlock1: c1_0,c2_0,c1_1,...)
    float* last_bias_sum = nullptr;            // sum over the resblocks of their LAST conv's bias (conv_splitk_sum_kernel)
    // fused MRF stage (mrf_kernel, kernels/mrf.h): device phase table + weight stream, or not ok: the stage runs conv by conv
    struct HostConv { std::vector<float> w; int co = 0, ci = 0, k = 0, dil = 1; const float* bias = nullptr; };
    std::vector<std::vector<HostConv>> rb_host;   // host copies of the resblock convs, dropped after build_mrf
    void* mrf_phases = nullptr; float* mrf_w = nullptr;
    // the same stage for mrf_split_kernel (matrix modes bf16x3 / f16x3): the weight stream as 16-bit term fragments and,
    // per phase, the factor that undoes the f16 packing scale (both in the arena: they travel with the broadcast)
    float* mrf_wsplit = nullptr; float* mrf_unscale = nullptr; int mrf_wsplit_floats = 0;
    int mrf_wfloats = 0, mrf_cp = 0, mrf_hx = 0;  // padded channels (32 / 64), halo of the stage (widest resblock chain)
    std::vector<struct MrfPhase> mrf_ph;          // host copy of the phases (cost model of the geometry choice)
    bool mrf_ok = false, mrf_rb1 = false;
  };
  struct MrfGeo { int ou = 0, N = 0, cu_lo = 0, cu_hi = 0, nleft = 0, nhalo = 0; };
  bool mrf_geo(const UpStage& st, int len_mul, bool tail, MrfGeo& best) const;      // window geometry by the cost model
  void build_mrf(UpStage& st);
  void mrf(const UpStage& st, View x, View out, const int* lens, int len_mul, int Lmax, bool tail = false);
  // How a generator stage's resblocks are issued (engine_launch.cpp, next to the grouping code): one fused launch, sibling
  // convs grouped on the split-K or the tiled kernel, or conv by conv; `tiled`: every conv of the stage keeps the tiled kernel
  enum StageForm { STAGE_FUSED, STAGE_GROUP_SPLITK, STAGE_GROUP_TILED, STAGE_CHAIN };
  struct StageSchedule { StageForm form; bool tiled; };
  StageSchedule stage_schedule(const UpStage& st, int Lmax, double fsum, bool buffers_fit) const;
  // Opt-in split-operand matrix modes PIPER_HIP_MATRIX = bf16x3 | f16x3 | bf16x6 (read at engine creation): the tiled conv
  // GEMMs of the coupling flow and the generator -- and, in the two-term modes, the fused MRF stages -- run on the 16-bit matrix
  // pipe with both f32 operands split into 16-bit terms (kernels/conv_bf3.h, mrf_split.h; 16 / 22 / 24 significand bits per
  // operand, f32 accumulate). The text encoder and the duration predictor stay f32 (the integer durations are those of the
  // f32 path), and so does every latency-bound split-K launch. Default: off, all f32.
  bool matrix_bf3_ = false, pack_bf3_now_ = false;      // a split matrix mode is on / the convs being packed take part in it
  int matrix_sm_ = 0;                                   // ... which: conv_split_kernel's SM (0 bf16x3, 1 f16x3, 2 bf16x6)
  static bool env_bf3();
 public:
  bool matrix_bf3() const { return matrix_bf3_; }
  int matrix_split_mode() const { return matrix_bf3_ ? matrix_sm_ : -1; }
 private:
  std::vector<UpStage> ups_;
  float* post_w_ = nullptr;
  int post_cin_ = 0;
  // speaker conditioning (all per-utterance bias vectors, see cond_kernel)
  struct CondW { float* w; float* b; int rows; };
  CondW cond_dp_{nullptr, nullptr, 0}, cond_dec_{nullptr, nullptr, 0};
  std::vector<CondW> cond_wn_;
  int gin_ = 0, nspk_ = 1;

  // per-call state
  int B_ = 0, Tmax_ = 0, Ts_ = 0, Fmax_ = 0, Fs_ = 0, Tg_ = 0, Fg_ = 0;
  bool use_graphs_ = true;
  // hipGraphExec_t per (stage, shape bucket), least recently used first: a new key beyond graph_cap_ entries
  // evicts ONE graph (the coldest), never the whole cache
  struct GraphEntry { std::string key; void* exec; long launches; };
  std::list<GraphEntry> graphs_;
  std::unordered_map<std::string, std::list<GraphEntry>::iterator> graph_of_;
  long graph_captures_ = 0;                   // captures since the engine was created (pe_graph_stats)
 public:
  long graph_captures() const { return graph_captures_; }
  size_t graphs_cached() const { return graphs_.size(); }
  // Shape buckets of the captured graphs: ids in steps of 32 up to 512, beyond that 8 steps per octave; frames in steps
  // of 64 up to 1024, then 16 per octave. A text of any length maps onto a bounded set of graphs.
  static int id_bucket(int T);
  static int frame_bucket(int F);
  // Pre-size the workspaces (so that no later call grows them -- growth re-creates every graph) and, given a sample
  // utterance, capture the single-utterance graphs of every id bucket up to max_ids by synthesising the sample cut /
  // tiled to each bucket length
  void warmup(int max_batch, int max_ids, float frames_per_id, const float* scales, const int64_t* sample, int64_t n_sample);
 private:
  long run_launches_ = 0;
  unsigned long long* d_rng_ = nullptr;       // {seed, call counter} read by randn_kernel
  float scales_[3] = {0.667f, 1.0f, 0.8f};         // utterance 0's triple of the last upload (pe_warmup's default)
  // utterance b's length_scale relative to the slowest (largest) one of the call, >= 0.5: the speculative guess counts
  // ids x this (1 for every utterance of a uniform call -- today's frames-per-id rule)
  std::vector<float> spec_rel_;
  float spec_rel(int b) const { return (size_t)b < spec_rel_.size() ? spec_rel_[b] : 1.f; }
  bool have_noise_w_ = false, have_noise_z_ = false;
  bool drew_w_ = false;                       // this call's duration noise is drawn by embed_kernel (small calls), not randn_kernel
  // Timing plan of the uploaded inputs. The plan block in the stage-A workspace (kernels/params.h: PlanP) is filled by one
  // copy from a pinned staging block of its own -- not the input block embed_kernel may read in place -- so the plan's values
  // are never kernel arguments: the 'A' graph of a timed call carries the two flags below in its key and nothing else of
  // the plan. A timed call runs as A, frame-count read-back, B; it neither reads nor feeds the speculative sizing.
  bool plan_on_ = false, plan_skip_ = false;      // skip: every id is forced, stage A leaves the duration predictor out
  int* d_plan_ = nullptr; float* plan_w_ = nullptr;
  PinBuf<int> h_plan_;
  // throws the refusal; returns whether every id of the call is forced
  static bool check_timing(const TimingIn& t, const int64_t* offsets, int B);
  void plan_params(PlanP& pp, const DurP& dp) const;
  std::string stage_a_key(int B) const;
  bool fold_dur_ = false;                  // the stage being issued is the one-graph form: regulate_kernel computes the durations
  DurP fold_dp_{};                         // ... from these fields (filled by issue_stage_a)
  std::vector<int64_t> id_off_;
  std::vector<int32_t> tlens_h_, frames_h_, dur_h_;
  std::vector<int64_t> sample_off_;
  uint64_t seed_ = 1234, call_ = 0;
  const float* h_noise_z_ = nullptr;
  int64_t h_noise_z_stride_ = 0;

  // workspaces
  size_t capA_B_ = 0, capA_T_ = 0, capB_B_ = 0, capB_F_ = 0;      // utterances / padded ids of stage A, utterances / frames of stage B
  bool capB_exact_ = false;      // stage B was last sized for exactly one call (memory pressure): it stays while calls fit
  size_t ws_budget_ = 0;             // bytes a stage's workspace may take (a third of the device's memory)
  size_t ws_budget();
  DevBuf<char> wsA_, wsB_;
  int *d_ids_ = nullptr, *d_tlens_ = nullptr, *d_sids_ = nullptr, *d_dur_ = nullptr, *d_cum_ = nullptr,
      *d_frames_ = nullptr;
  float* d_scales_ = nullptr;        // [B][3] per-utterance {noise_scale, length_scale, noise_w}, part of the input block
  static size_t in_scale_slots(size_t Bc) { return (3 * Bc + 3) & ~(size_t)3; }   // its 4-byte slots (ids stay 16-byte aligned)
  // Per-utterance seeds of the uploaded inputs: keys[Bc] (64-bit) and use[Bc] (ints) sit in the input block
  // right behind the generator state, in front of the lengths, so that they travel with the block's one copy -- or are read
  // in place and published by embed_kernel on the zero-copy path. The VALUES are data; whether the call carries seeds at
  // all picks the kernels' key-table arguments (null without) and is part of the graph keys (seed_key), so an unseeded
  // call's graphs are what they always were.
  static size_t in_seed_bytes(size_t Bc) { return (12 * Bc + 15) & ~(size_t)15; }
  static size_t in_head_bytes(size_t Bc) { return 32 + in_seed_bytes(Bc); }
  unsigned long long* d_keys_ = nullptr; int* d_use_ = nullptr;
  bool seeded_ = false;
  const char* seed_key() const { return seeded_ ? "|s" : ""; }
  // The small inputs of a call -- {seed, call}, seeds, lengths, speaker ids, scales, phoneme ids -- are one contiguous block in the stage-A
  // workspace (d_in_) mirrored by a pinned host block (h_in_): upload() fills the host block and enqueues ONE copy, no
  // synchronisation (the pinned block outlives the copy; the call's final synchronisation covers it)
  char* d_in_ = nullptr; PinBuf<char> h_in_; size_t in_bytes_ = 0;
  // Speaker blends of the uploaded inputs lie IN FRONT of that block, in the same allocation and in the same
  // pinned mirror: [count Bc | component ids Bc x 8 | weights Bc x 8 | vectors Bc x gin], padded to 256 bytes, then d_in_
  // (h_in()). A copied call that carries a blend starts its one copy at the area, every other call at d_in_ as ever; a
  // zero-copy call's speaker_blend_kernel reads the pinned area in place. 68 + 4 gin bytes per utterance of the capacity
  // bucket, nothing for a single-speaker voice. The kernel writes g_tab_ [Bc][gin] and g_rows_ [Bc] (rows[b] = b), which
  // cond_kernel reads in place of the table and the ids. The VALUES are data; whether the call carries a blend at all
  // adds a launch and is part of the graph keys (blend_key), so a plain call's graphs are what they always were.
  size_t in_blend_bytes(size_t Bc) const { return nspk_ > 1 ? (Bc * (68 + 4 * (size_t)gin_) + 255) & ~(size_t)255 : 0; }
  char* h_in() const { return h_in_.get() + in_blend_bytes(capA_B_); }
  char* d_blend_ = nullptr;
  float* g_tab_ = nullptr; int* g_rows_ = nullptr;
  bool blended_ = false;
  const char* blend_key() const { return blended_ ? "|g" : ""; }
  BlendP blend_params(const char* area, size_t Bc) const;
  // short calls: no copy at all -- embed_kernel reads the pinned block in place (policy.h: ids_from_host)
  bool ids_zc_ = false;
  unsigned long long upload_serial_ = 0;
  float* att_s_ = nullptr;           // attention score slabs of long utterances (attn_long_kernel); null while every slab fits LDS
  size_t attn_smem(int T, bool global_scores) const;
  bool attn_scores_global(int T) const;
  float* vQ_ = nullptr;
  float* kT_ = nullptr;              // K transposed [utterance][column][H] for attn4_kernel; written by the q/k/v launch while kt_on_
  bool kt_on_ = false, kt_valid_ = false;      // kt_valid_: the last q/k/v launch did write kT
  float *x_ = nullptr, *y_ = nullptr, *qkv_ = nullptr, *att_ = nullptr, *ffh_ = nullptr, *stats_ = nullptr,
        *xg_ = nullptr, *dh_ = nullptr, *dy_ = nullptr, *dy2_ = nullptr, *hproj_ = nullptr, *z2_ = nullptr,
        *logw_ = nullptr, *noise_w_ = nullptr, *cond_ = nullptr;
  int cond_bs_ = 0;
  std::vector<int> cond_off_wn_;
  int cond_off_dp_ = 0, cond_off_dec_ = 0;
  float *zp_ = nullptr, *fh_ = nullptr, *facts_ = nullptr, *fskip_ = nullptr, *noise_z_ = nullptr;
  float* hb_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t ls_ = nullptr;       // stream conv()/layer launches go to
  // per-resblock buffers of the grouped sibling schedule (one-utterance calls)
  DevBuf<float> side_[9];
  size_t side_floats_ = 0;
  float* zwin_ = nullptr;          // streaming: current window of z, [C][Fs]
  int* d_win_ = nullptr;           // streaming: {start, length} of the window in frames
  int halo_frames_ = 0, s_frames_ = 0, s_pos_ = 0, s_wg_ = 0;
  bool s_active_ = false;
  std::vector<int16_t> s_pcm_;
  // Lock-step window stages. ChunkRows is everything such a stage owns for its set of rows -- the batch stream's utterances
  // ('V' graphs), the pool's slots ('P' graphs). The per-chunk state block (kernels/params.h: sb_*) exists twice, pinned
  // host and device; the gain blocks (params.h: sg_*, sgd_*) likewise. All are allocations of their own at `cap` rows,
  // outside both workspaces; their addresses are kernel arguments inside the stage's graphs (growth drops the graphs), their
  // CONTENT -- windows, delivery ranges, the output pointers -- is what changes from chunk to chunk.
  struct ChunkRows {
    char stage;                                    // dispatch_stage's letter, first character of the graph keys
    int cap = 0;                                   // rows the blocks are sized for (even)
    PinBuf<int> host; DevBuf<int> dev;             // state blocks
    PinBuf<int> gctl; DevBuf<int> gdev;            // gain control (pinned) and gain state (device) blocks
    // target loudness of streams (params.h: slc_*, sld_*): control (pinned), state, segment sums [cap][lnseg], tails
    // [cap][2][lW]; allocated with the first chunk in that mode, they live and die with the blocks above
    PinBuf<int> lctl; DevBuf<int> ldev; DevBuf<double> lseg; DevBuf<float> ltail;
    int lnseg = 0, lW = 0;
    // look-ahead limiter on streams (params.h: slm_*): control (pinned), report words (device) and their pinned copy, scale
    // tails [cap][2][SLM_TAIL]; allocated with the first chunk that runs with it, beside the blocks above. Host view per
    // row: stream samples so far and handed out so far (reset with the row's gfirst flag)
    PinBuf<int> mctl, mreph; DevBuf<int> mrep; DevBuf<float> mstail;
    std::vector<int64_t> mN, mB;
    std::vector<char> gfirst;                      // per row: nothing delivered yet (its level starts afresh)
    std::vector<int32_t> pos;                      // frames delivered per row; its size is the number of rows
    std::vector<int64_t> off;                      // sample offsets of the current chunk
    PinBuf<int16_t> pcm; PinBuf<float> audio;      // pinned host output of the current chunk
    // with a G.711 format: the device staging of the chunk's packed int16 (the stage's output pointer), the codes on the
    // device and their pinned host copy; grown with the chunks, never inside a graph (the pointers are data)
    DevBuf<int16_t> pcm_dev; DevBuf<uint8_t> codes_dev; PinBuf<uint8_t> codes;
    int wg = 0;                                    // window bucket of the current chunk
    // what the stage reads the rows from: the latents [row][C][src_cs] and the decoder's conditioning rows (null: cond_)
    const float* src = nullptr; long src_bs = 0; int src_cs = 0;
    const float* cond = nullptr; int cond_bs = 0;
  };
  void rows_free(ChunkRows& r);                    // the blocks released, the state that pointed into them reset
  // one chunk of every row that has frames left (live: null = all rows are) and the positions advanced: row b goes on by
  // per_row[b] where that is > 0, else by `chunk`, at most `clamp` frames. False, with nothing run, when no row delivers.
  bool rows_next(ChunkRows& r, const int32_t* frames, const int32_t* live, int chunk, const int32_t* per_row, int clamp,
                 bool want_audio, StreamChunk& out);
  // the window stage on the rows: gather from r.src by the pinned state block, generator, chunk delivery
  void issue_window_rows(const ChunkRows& r);
  // batch streaming. The window buffer [B][C][Fs] is noise_z_: dead once regulate_kernel has run (debug_tensor refuses
  // "noise_z" while a batch stream is live). The blocks are allocated on the first batch stream for the stage-A batch
  // capacity, the gain blocks with the first chunk outside the default mode; the rows are read from zp_.
  bool sb_active_ = false;
  ChunkRows batch_rows_{'V'};
  void ensure_stream_batch(int B);
  // stream-wide gain. The setting; the one-utterance stream's state (its conversion runs on the host); the report of the
  // last chunk call.
  int gain_mode_ = GAIN_CHUNK, gain_ramp_ = 0;
  float gain_peak_ = 0.f;
  float s_gain_r_ = 0.01f; bool s_gain_first_ = true;
  void gain_blocks_alloc(ChunkRows& r, int cap);   // r's gain blocks for cap rows, zero-filled
  void gain_prepare(int* ctl, int cap, const std::vector<char>& first, int n);
  // after a chunk call over n rows with sample offsets off[n + 1]: the report, and the flags of the rows that delivered.
  // Default mode: the peaks stay on the device (`peaks`, one word per row) and are fetched when the report is asked for.
  void gain_collect(const int* ctl, int cap, int n, std::vector<char>& first, const int64_t* off, const unsigned* peaks);
  void gain_report_idle(const int* ctl, int cap, int n);   // a chunk call that ran nothing: stored state / zeros
  // target loudness of streams: the setting, the filter block of the delivered rate sl_fs_ (h / W / R follow it), the
  // one-utterance stream's state (its filter and conversion run on the host, f64 serial) and the last chunk call's report
  float sl_T_ = -23.f, sl_cdb_ = -1.f, sl_prior_ = std::numeric_limits<float>::quiet_NaN();
  int sl_fs_ = 0, sl_h_ = 0, sl_W_ = 0, sl_R_ = 0;
  DevBuf<double> sl_coef_;
  void sl_upload_filter(int fs);
  // r's blocks for cap rows of streams of up to max_samples delivered samples, at the delivered rate (grown: graphs dropped)
  void sl_ensure(ChunkRows& r, int cap, int64_t max_samples);
  void sl_prepare(ChunkRows& r, int n);
  SlP sl_params(const ChunkRows& r) const;
  void issue_stream_loudness(const ChunkRows& r, int B, long max_n, bool rs);      // (with the limiter on: its launch too)
  void sl_collect(ChunkRows& r, int n, bool ran);
  struct HostLoud {
    double coef[10]; double z[4]; std::vector<double> seg; int64_t N = 0; int h = 1;
    float r = 0.f, G = 0.f, lu = 0.f, L = 0.f; int flags = 0; bool first = true;
    // look-ahead limiter: floats and scales of the stream samples [N - hx.size(), N), what has been handed out, the weights
    std::vector<float> hx, hs, hw; int64_t B = 0; int W = 0;
  } s_sl_;
  // look-ahead limiter on streams: the setting, the weights for the window at the delivered rate (a table of fixed size:
  // its address stays, W is part of the graph keys), the report of the last chunk call
  bool slim_on_ = false;
  float slim_ms_ = 5.f;
  DevBuf<float> slim_h_; int slim_fs_ = 0, slim_W_ = 0; float slim_hms_ = 0.f;
  std::vector<float> lsm_maxred_;
  std::vector<int32_t> lsm_shaped_;
  int lsm_n_ = 0;
  std::vector<float> s_pcm_f_;                             // one-utterance stream: the floats a delayed delivery hands out
  bool slim_active() const { return gain_mode_ == GAIN_LOUDNESS && slim_on_; }
  void slim_ensure(ChunkRows& r, int cap);                 // the table for the rate and the rows' limiter blocks
  SlmP slim_params(const ChunkRows& r) const;
  std::vector<float> lsl_lufs_;
  std::vector<int32_t> lsl_flags_;
  int lsl_n_ = -1;
  std::vector<float> lg_gain_, lg_peak_;
  std::vector<char> lg_got_;
  int lg_n_ = -1;                                          // rows of the last chunk call (-1: none yet)
  const unsigned* lg_dev_peaks_ = nullptr;                 // default mode: where the last chunk's peaks are, until other work runs
  bool lg_lazy_ = false;                                   // the report is still to be fetched from there
  // text encoder, durations and flow of the uploaded batch, the latent left in zp_ (front half of every stream);
  // max_frames > 0: an utterance with more frames is an error, raised before stage B is sized for it
  void stream_front(int B, int max_frames);
  // stream pool (see above). Resident, next to its rows' blocks (cap = slots rounded up to even, all allocated by open): the
  // latent [slots][C][sp_fcap_], the decoder conditioning rows [slots][cond_dec rows] (multi-speaker voices) and the pinned
  // join block (params.h: sj_*). Workspace growth, which frees and poisons both workspaces and drops every graph, does not
  // touch them. stream_pool_close destroys the 'P' graphs.
  int sp_slots_ = 0, sp_fcap_ = 0, sp_maxf_ = 0;           // slots, row width, max_frames
  DevBuf<float> sp_z_, sp_cond_;
  PinBuf<int> sp_join_;
  std::vector<int32_t> sp_frames_, sp_live_;
  ChunkRows pool_rows_{'P'};
  void stream_pool_free();
  // output-rate conversion. The table, the resampled waveform [capB_B_][So_] with its int16 twin and the two row blocks
  // (pinned host + device, params.h: rs_*) are allocations of their own; their addresses are kernel arguments inside the
  // graphs, so (re)allocating them drops every graph. So_ is the row stride of what is delivered: Ss_ at the native rate.
  bool rs_on_ = false;
  int rs_native_ = 0, rs_out_ = 0, rs_L_ = 1, rs_M_ = 1, rs_K_ = 0, rs_Tp_ = 0, rs_tile_ = RS_TILE;
  DevBuf<float> rs_coef_;
  DevBuf<float> raudio_; DevBuf<int16_t> rpcm_;
  long So_ = 0;
  PinBuf<int> rs_host_; DevBuf<int> rs_dev_; int rs_cap_ = 0;
  void ensure_resample();                       // after ensure_stage_b sized the workspace
  // rows + resample launches on B rows of x (row stride x_bs, x_cap valid-capacity per row) into raudio_; hst: the pinned
  // row block, or null with lens: whole utterances; max_out bounds every row's output count (grid)
  void issue_resample(int B, const float* x, long x_bs, const int* hst, const int* lens, long max_out, double native_samples);
  void rs_host_row(int b, int64_t n0, int64_t org, int count, int vlen);
  const unsigned* rs_peaks() const { return reinterpret_cast<const unsigned*>(rs_dev_.get()) + rs_o_peak(rs_cap_); }
  const int* rs_counts() const { return rs_dev_.get() + rs_o_count(rs_cap_); }
  // target loudness. The filter block, the segment sums [rows][ld_nseg_cap_] and the control / gain blocks (params.h: ld_*,
  // pinned host + device) are allocations of their own, outside both workspaces; their addresses are kernel arguments inside
  // the graphs, so (re)allocating them drops every graph. h / W / R follow the delivered rate, which only set_output_rate
  // changes (it drops the graphs itself).
  bool ld_on_ = false;
  float ld_T_ = -23.f, ld_cdb_ = -1.f;
  int ld_fs_ = 0, ld_h_ = 0, ld_W_ = 0, ld_R_ = 0;
  DevBuf<double> ld_coef_;
  DevBuf<double> ld_seg_; size_t ld_seg_rows_ = 0; int ld_nseg_cap_ = 0;
  PinBuf<int> ld_ctl_; DevBuf<int> ld_dev_; int ld_cap_ = 0;
  std::vector<float> ll_lufs_, ll_scale_, ll_peak_;
  std::vector<int32_t> ll_flags_;
  int ll_n_ = -1;                               // utterances of the last fetched call's report (-1: none yet)
  // true-peak ceiling: the interpolator's table [tp_Q_][TP_TAPS] for the delivered rate tp_fs_ and one word per row, device
  // allocations of their own next to the loudness blocks (ensure_loudness; kernel arguments inside the PEAK_TRUE graphs)
  int ld_kind_ = PEAK_SAMPLE;
  bool tp_on() const { return ld_on_ && ld_kind_ == PEAK_TRUE; }
  DevBuf<float> tp_coef_; int tp_fs_ = 0, tp_Q_ = 0;
  DevBuf<unsigned> tp_words_;
  std::vector<float> ll_tpeak_;
  int ll_tn_ = 0;
  static void tp_check_rate(int fs);            // throws the refusal
  void tp_upload_table(int fs);
  // look-ahead limiter: the weights [2 lim_W_ + 1] for the window at the delivered rate lim_fs_, the report words on the
  // device and their pinned host copy (params.h: lim_*), allocations of their own (ensure_loudness; kernel arguments inside
  // the limiter's graphs). The report travels with the call's samples: download enqueues the copy in front of its wait.
  bool lim_on_ = false;
  float lim_ms_ = 5.f;
  DevBuf<float> lim_h_; int lim_fs_ = 0, lim_W_ = 0; float lim_h_ms_ = 0.f;
  DevBuf<int> lim_rep_; PinBuf<int> lim_host_; int lim_cap_ = 0;
  // true-peak ceiling with the limiter: the per-position maxima v and the shaped floats z, [rows][lim_zv_bs_] each
  DevBuf<float> lim_v_, lim_z_;
  // whether the run that is fetched next went through the limiter: noted where a run's graph key is formed and where the
  // stage is issued, so that a setting made between run and fetch does not relabel the report
  mutable bool run_lim_ = false;
  std::vector<float> ll_maxred_, ll_trim_;
  std::vector<int32_t> ll_shaped_;
  int ll_ln_ = 0;
  bool lim_active() const { return ld_on_ && lim_on_; }
  // what the loudness setting adds to the 'B' and 'C' graph keys: off, sample peak, true peak, each with the limiter
  const char* loud_key() const {
    run_lim_ = ld_on_ && lim_on_;
    if (!ld_on_) return "";
    if (lim_on_) return ld_kind_ == PEAK_TRUE ? "|l4" : "|l3";
    return ld_kind_ == PEAK_TRUE ? "|l2" : "|l1";
  }
  static void lim_check(bool on, float window_ms);                // throws the refusal
  void debug_stream_rows(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                         float ceiling_db, float prior_lufs, int ramp_samples, float window_ms, float* lufs, float* g0, float* g1,
                         int32_t* flags, int32_t* delivered, float* env, int16_t* pcm);      // both stream test hooks
  // the delivery chain's other refusals and small formulas, each written once (engine_deliver.cpp)
  static void check_target(float target_lufs);
  static void check_ceiling(float ceiling_db);
  static void check_ceiling_kind(int kind);
  static void check_limiter_window_at(float window_ms, int fs);   // "limiter window ... ms is more than LIM_MAXW samples at fs Hz"
  static int check_row_lengths(const int32_t* valid, int batch, int64_t stride);      // all within [0, stride]; the largest
  static void to_f32(const std::vector<double>& exact, float* out);                 // an f64 filter table rounded once
  int row_block_cap() const;                    // rows of the resampler's / loudness's row blocks: even, >= 64, >= both batch capacities
  // staging of the debug hooks: `batch` host rows of `stride` elements <-> device rows of padded stride xs, on stream_;
  // count: elements of each row that come back (null: stride)
  template <typename T> void rows_to_device(T* dst, long xs, const T* src, int batch, int64_t stride);
  template <typename T> void rows_to_host(T* dst, int64_t stride, const T* src, long xs, int batch, const int32_t* count = nullptr);
  // The limiter's launches behind the gain (kernels/limiter.h): limiter_kernel; or, with the true-peak ceiling,
  // limiter_true_kernel, true_peak_kernel on z and pcm16_trim_kernel. Shared by issue_loudness and debug_limiter.
  struct LimTail {
    const float* x; long x_bs; const int* lens; int len_mul; long x_cap;      // the row view
    int* gq; int gcap; int* ctl; int* rep; int rcap;                          // gain / control / report blocks
    const float* h; int W;                                                    // the window
    float* v; float* z; const float* tp_coef; int Q;                          // true-peak ceiling (v null: sample peak)
    int16_t* pcm; int16_t* zc; float* env;                                    // outputs (zc, env: or null)
  };
  void issue_limiter_tail(const LimTail& t, int B, long max_n, double samples, bool profile_rows);
  void lim_upload_window(int fs);
  void lim_enqueue_report();                    // device report words -> lim_host_, on stream_
  static void loud_check_rate(int fs);          // throws the refusal
  void loud_upload_filter(int fs);              // h / W / R and the filter block for rate fs
  void loud_write_ctl();
  void ensure_loudness();                       // after ensure_stage_b sized the workspace (and ensure_resample the rows)
  void loud_collect();                          // the pinned report of the call just synchronised -> ll_*
  // segment sums, gain and the int16 conversion of B delivered rows x (stride x_bs, lengths lens[b] * len_mul, peak words
  // `peaks`); max_n bounds every row's length (grid)
  void issue_loudness(int B, const float* x, long x_bs, const int* lens, int len_mul, const unsigned* peaks, long max_n,
                      int16_t* pcm, int16_t* zc, double samples);
  // sample format. The codes of a whole-utterance call, packed, [capB_B_ * So_] on the device (an allocation of its own; its
  // address is a kernel argument inside the graphs of its format, so growing it drops the graphs) and their pinned host copy;
  // run_fmt_: the format of the run that is fetched next, noted where its graph key is formed.
  int fmt_ = G711_S16;
  mutable int run_fmt_ = G711_S16;
  DevBuf<uint8_t> codes_; PinBuf<uint8_t> h_codes_;
  int lc_rows_ = 0;                             // rows of the last fetched call's codes (0: s16)
  std::vector<uint8_t> s_codes_;                // one-utterance stream: the chunk's codes (host conversion)
  int64_t s_codes_off_[2] = {0, 0};
  const uint8_t* lc_s_codes_ = nullptr; const int64_t* lc_s_off_ = nullptr; int lc_s_rows_ = 0;      // last chunk of any stream
  const char* fmt_key() const {
    run_fmt_ = fmt_;
    return fmt_ == G711_ULAW ? "|u" : (fmt_ == G711_ALAW ? "|a" : "");
  }
  void ensure_g711();                           // after ensure_stage_b sized the workspace (and So_)
  // the encoder on B delivered int16 rows (stride p_bs, lengths lens[b] * len_mul, max_n bounds them): the call's last launch
  void issue_g711(int B, const int16_t* pcm, long p_bs, const int* lens, int len_mul, long max_n, double samples);
  float* audio_ = nullptr;
  int16_t* pcm_ = nullptr;
  unsigned* absmax_ = nullptr;
  long Ss_ = 0;
  // host pinned
  PinBuf<float> h_audio_;
  PinBuf<int16_t> h_pcm_;
  // pcm16_kernel also writes the samples straight into this pinned host buffer (zero-copy), utterances packed back to
  // back: delivering the PCM costs no copy launches behind the graph (one per utterance before: 1.3 ms at B=64) -- the
  // call ends with one stream synchronisation.
  PinBuf<int16_t> h_pcm_zc_;
  bool pcm_zc_live_ = false;                // the last run's PCM is in h_pcm_zc_
  PinBuf<int> h_frames_;

  // profiling
  bool prof_on_ = false;
  int prof_level_ = 0;
  std::vector<ProfileRow> prof_;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
  // level-2 per-launch timing: event pairs recorded without host syncs, resolved in profile()
  struct KEvent { int row; double flops; double bytes; hipEvent_t a, b; };
  std::vector<KEvent> kev_;
  std::vector<hipEvent_t> ev_pool_;
  int kbegin(int row, double flops, double bytes = 0);
  void kend(int h);
  int krow(const char* name);
  int krow(const std::string& name);
  std::deque<std::string> names_;            // storage of generated profile row names (stable pointers)
  float* zp_keep_ = nullptr;
  void free_all();
};

}  // namespace pe
