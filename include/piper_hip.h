/* piper_hip.h -- C ABI of the MI355X-native VITS synthesis engine (libpiper_hip.so).
 *
 * This is the drop-in boundary for the ONNX Runtime session that the reference's
 * piper::synthesize() drives (reference src/cpp/piper.cpp:337-441). Each entry point names the
 * reference interface it replaces. Plain pointers and sizes only; all functions return 0 on success
 * and a non-zero code on failure, with the message available from pe_last_error() (the reference
 * throws Ort::Exception / std::runtime_error at the same places; the C++ shim in
 * piper_amd/csrc/piper.hpp re-throws std::runtime_error).
 *
 * Threading: like the reference an engine handle is not thread-safe; use one
 * handle per thread / per GPU. Output buffers returned by pe_synthesize* are owned by the engine and
 * stay valid until the next call on the same handle.
 */
#ifndef PIPER_HIP_H_
#define PIPER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pe_engine pe_engine;

/* Optional injected N(0,1) draws for the two sampling sites of the graph (reference
 * vits/models.py:111 and :718; ONNX RandomNormalLike nodes). NULL pointers -> the engine's own
 * counter-based generator (seed: pe_set_seed). Host pointers.
 *   noise_w: [B][2][w_stride]        column t is used for phoneme id t
 *   noise_z: [B][inter][z_stride]    column f is used for frame f (z_stride >= frames) */
typedef struct pe_noise {
  const float* noise_w;
  int64_t w_stride;
  const float* noise_z;
  int64_t z_stride;
} pe_noise;

/* Result views of the last synthesis call (engine-owned host memory). */
typedef struct pe_result {
  int32_t batch;
  const int64_t* sample_offsets; /* [batch+1] prefix offsets into audio / pcm */
  const float* audio;            /* float waveform in [-1,1], what Ort "output" [1,1,1,S] held (piper.cpp:397-400) */
  const int16_t* pcm;            /* peak-normalised int16 as piper.cpp:410-431 / util.py:5-12 produce */
  const int32_t* frames;         /* [batch] spectrogram frames per utterance (S = frames * hop native samples; take lengths from sample_offsets) */
  double infer_seconds;          /* wall time of the device pipeline, the reference's inferSeconds (piper.cpp:385-395) */
} pe_result;

/* Replaces Ort::Env + SessionOptions + Ort::Session(model path) in loadModel()
 * (piper.cpp:262-306): parses the voice .onnx (export_onnx.py graph), packs the weights for the
 * MFMA kernels and uploads them to GPU `device`. `onnx_path` may also name the output of the reference's
 * streaming export (export_onnx_streaming.py: a directory with encoder.onnx + decoder.onnx, or either of
 * the two files): both graphs are read and the voice behaves like the single-file one. */
int pe_create(const char* onnx_path, int device, pe_engine** out);

/* Same from an in-memory weight blob (PEBLOB01, see piper_amd/weights.py). This is also what the
 * other ranks of a multi-GPU job call after the RCCL broadcast of rank 0's blob. */
int pe_create_from_blob(const void* blob, size_t nbytes, int device, pe_engine** out);

/* Multi-GPU loading without a host round trip per rank (one RCCL broadcast of the voice at load).
 * The packed weights of an engine live in ONE device arena whose layout follows from the tensor SHAPES alone:
 *   every rank:  pe_weights_bound(header)            -> arena size to allocate (e.g. a torch / RCCL-registered buffer)
 *   root rank:   pe_create_in_arena(blob, .., arena, bytes, skeleton = 0)   parses, packs, uploads into its arena
 *   other ranks: pe_create_in_arena(header, .., arena, bytes, skeleton = 1) lays the arena out, touches no weight data
 *   all:         broadcast the first pe_weights_used() bytes of the root's arena into the others' arenas (ncclBroadcast)
 *   other ranks: pe_arena_ready()
 * `header` = the first 8 + 4*64 + 8 + n_tensors*136 bytes of a PEBLOB01 (magic, architecture, tensor records).
 * The arena must be 256-byte aligned and outlive the engine. */
int pe_weights_bound(const void* blob_or_header, size_t nbytes, size_t* bound);
int pe_create_in_arena(const void* blob_or_header, size_t nbytes, int device, void* arena, size_t arena_bytes,
                       int skeleton, pe_engine** out);
int pe_weights_used(pe_engine* e, size_t* used);
int pe_arena_ready(pe_engine* e);

/* .onnx -> PEBLOB01 in host memory (no GPU needed). Free with pe_free(). */
int pe_onnx_to_blob(const char* onnx_path, void** blob, size_t* nbytes);
void pe_free(void* p);

/* Replaces session.onnx.Run() for one utterance (piper.cpp:386-388) with the inputs of
 * piper.cpp:342-377: ids = "input"[1,T] (int64), scales = {noise_scale, length_scale, noise_w},
 * sid = "sid" or -1 for single-speaker voices. */
int pe_synthesize(pe_engine* e, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                  const pe_noise* noise, pe_result* result);

/* Batched form: B independent utterances, each computed exactly as a B=1 Run() would (no cross-talk
 * through padding). ids are concatenated; offsets[B+1] delimit them; sids may be NULL. */
int pe_synthesize_batch(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch,
                        const float scales[3], const int64_t* sids, const pe_noise* noise, pe_result* result);

/* The same call in three parts (pe_synthesize_batch = pe_upload + pe_run + pe_fetch(1, 1)): upload = validate and stage the
 * inputs (ids / lengths / speaker ids of calls up to 65 536 padded ids stay in the engine's pinned host block and are read
 * in place by the first kernel -- no copy is enqueued; larger calls and injected noise are copied to HBM), run = the device
 * pipeline (may be repeated on the uploaded inputs: every run draws fresh noise), fetch = wait + result views (the int16 PCM
 * is written straight into pinned host memory by the last kernel; want_audio adds a copy of the float waveform). */
int pe_upload(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float scales[3],
              const int64_t* sids, const pe_noise* noise);

/* Per-utterance scales: the same two calls with one triple per utterance -- scales[batch * 3], laid out as
 * [utterance][noise_scale, length_scale, noise_w] -- so that one batch may mix speaking rates and variability. Utterance b is
 * computed exactly as a call with scales b alone would compute it (the reference's Run() with its own `scales` tensor,
 * piper.cpp:347-365; its batch export shares one tensor, so this goes beyond it). A NULL `scales` or a non-finite value is
 * rejected (the message names the utterance) before anything of the engine changes: the next call works as usual. The
 * one-triple entry points above are these calls with the triple repeated. */
int pe_synthesize_batch_scaled(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch,
                               const float* scales, const int64_t* sids, const pe_noise* noise, pe_result* result);
int pe_upload_scaled(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                     const int64_t* sids, const pe_noise* noise);

/* Timing plan: when things are said (beyond the reference, whose only handle is one length_scale).
 * Host pointers; any member, and the plan itself, may be NULL.
 *   rate           [n_ids], concatenated like ids: multiplies that id's predicted duration; finite and > 0. NULL: all 1.
 *   forced         [n_ids]: >= 0, that id lasts exactly so many frames (0 drops it from the audio); -1, predicted. In
 *                  [-1, 60000]. NULL: all -1. The output of pe_get_durations fits here as it is.
 *   target_frames  [batch]: > 0, the utterance lasts exactly so many frames; 0, no target. In [0, 60000]. NULL: all 0.
 * With logw_i as before, w_i = (exp(logw_i) * length_scale) * rate_i in f32, in this order. Without a target a free id gets
 * d_i = clamp(ceil(w_i), 0, 1e6) as ever and a forced one its value. With a target N the forced ids keep theirs; each of
 * the n free ids gets one frame, and the R = N - sum(forced) - n frames that are left go by largest remainder on the integer
 * weights q_i = w_i > 0 ? max(1, (int64)(min(w_i, 1e6) * 2^20)) : 1 -- a_i = q_i R / Q, r_i = q_i R % Q with Q = sum q_i; the
 * R - sum a_i ids with the largest r_i, ties to the lower index, get one more -- so the frame count is N exactly.
 * Refused, with a message that names the utterance and the id, before anything of the engine changes (a live stream goes on):
 * a rate that is not finite or not > 0; a forced value or a target outside its range; a target below sum(forced) + n (every
 * free id keeps a frame); with every id forced, a target that differs from the sum, or no target and a sum outside
 * [1, 60000].
 * The _timed entry points are the calls they are named after plus the plan; with a NULL plan exactly those calls. pe_run
 * repeated on a timed upload keeps the plan; the next upload of any kind drops it. A timed call always reads the frame counts
 * back between its two halves (it is never issued for a guessed frame bucket and leaves the guess's statistics alone). When
 * every id of the call is forced the duration predictor does not run at all and no duration noise is drawn; the debug tensors
 * logw and plan_w (w_i of the last timed call) are then not available. */
typedef struct pe_timing {
  const float* rate;
  const int32_t* forced;
  const int32_t* target_frames;
} pe_timing;
int pe_upload_timed(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                    const int64_t* sids, const pe_noise* noise, const pe_timing* timing);
int pe_synthesize_batch_timed(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                              const int64_t* sids, const pe_noise* noise, pe_result* result, const pe_timing* timing);
/* Per-utterance noise seeds: a request's audio independent of its batch (the reference's
 * SynthesisConfig / PiperVoice seed, per utterance instead of per process). Host pointers.
 *   seed  [batch]: the utterance's seed. Every 64-bit value is a valid seed, 0 and 2^64 - 1 included.
 *   use   [batch]: != 0, the utterance draws from its seed; 0, from the engine's own stream as ever. NULL: all 1.
 * The law: a seeded utterance with seed S draws, at both sampling sites, element (row = channel, column = id or frame) of the
 * stream documented at pe_debug_randn with key S and run counter 0 -- what pe_debug_randn(site, 0, channel, n) returns under
 * pe_set_seed(S). The engine's own stream starts at counter 1, so a seeded draw never coincides with an unseeded one. Its
 * noise depends on (S, site, channel, column) and on nothing else: not on the engine seed or pe_rng_calls, its index in the
 * batch or the batch size, shape buckets or speculation, the kernel that draws, the entry point, the group member, the
 * coalesced call or the pool slot. An unseeded utterance draws bit for bit what it always did -- (engine seed, counter,
 * row = b * channels + c) -- also beside seeded ones, and the run counter advances as before in every case.
 * Noise injected through pe_noise wins at the site it is given for; the seed covers the other site. pe_run repeated on a
 * seeded upload draws the same noise again (the counter still advances); the next upload of any kind drops the seeds. The
 * seed values are call inputs like the ids: no captured graph depends on them (whether a call carries seeds at all is part
 * of the graph keys, so a server whose calls are all seeded stops capturing like any other).
 * The _seeded entry points are the _timed calls they are named after plus the seeds (pe_stream_begin_seeded: pe_stream_begin
 * plus a plan and the seeds); timing and seeds may each be NULL, and with NULL seeds they are exactly those calls. A non-NULL
 * pe_seeds whose `seed` is NULL is refused, with a message, before anything of the engine changes. */
typedef struct pe_seeds {
  const uint64_t* seed;
  const uint8_t* use;
} pe_seeds;
int pe_upload_seeded(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                     const int64_t* sids, const pe_noise* noise, const pe_timing* timing, const pe_seeds* seeds);
int pe_synthesize_batch_seeded(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                               const int64_t* sids, const pe_noise* noise, pe_result* result, const pe_timing* timing,
                               const pe_seeds* seeds);
/* Blend speakers: weighted embedding mixes and caller-supplied vectors. Host pointers.
 * The law. Every utterance of a call gets one speaker vector g_b[gin]. The choice depends on a per-utterance count:
 *   - count[b] == 0: g_b = emb_g[sids[b]], as ever.
 *   - count[b] == n, with n in 1..8:
 *     - The components (s_0, a_0) .. (s_{n-1}, a_{n-1}) are speaker ids and f32 weights, taken in the order given.
 *     - Per element i, g = a_0 * e_{s_0}[i] as one f32 product.
 *     - Then g = fmaf(a_k, e_{s_k}[i], g) for k = 1 .. n-1.
 *     - The weights are used as given. They are not normalised anywhere, and they may be negative or exceed 1.
 *     - A repeated id is allowed.
 *   - count[b] == -1: g_b is row b of a caller-supplied vector[batch][gin], bit for bit.
 * Everything behind g_b is unchanged: out[b][r] = W[r][:] . g_b + bias[r], with the summation order cond_kernel has today.
 * Two consequences hold bit for bit, audio and durations alike: the blend {(s, 1.0f)} gives what the plain call with
 * sids[b] = s gives, and the vector emb_g[s] gives what the plain call with sids[b] = s gives.
 * An utterance's g_b depends on nothing else: not its components' neighbours, not its row in the batch, the batch size, a
 * shape bucket, the entry point, a group member or a pool slot.
 * sids[b] of an utterance whose count is not 0 is not read. The _blended entry points are the _seeded calls they are named
 * after plus the blend; with a NULL blend they are exactly those calls. pe_run repeated on a blended upload keeps the
 * blend; the next upload of any kind drops it. The blend's values are call inputs like the ids: no captured graph depends
 * on them (whether a call carries a blend at all is part of the graph keys). A call without a blend issues exactly the
 * launches it always did; a blended call issues one more (speaker_blend_kernel).
 * Refused, with a message that names the utterance and the component, before anything of the engine changes (a live stream
 * goes on): a blend on a single-speaker voice; a count outside [-1, 8]; a component id outside [0, num_speakers); a weight
 * or vector element that is not finite; count -1 with a NULL `vector`; NULL `sid` or `weight` while some count is > 0. */
enum { PE_BLEND_MAX = 8 };
typedef struct pe_blend {
  const int32_t* count;   /* [batch]: 0 plain sid, 1..8 components, -1 row b of `vector` */
  const int64_t* sid;     /* components of all utterances, concatenated in utterance order */
  const float*   weight;  /* alike */
  const float*   vector;  /* [batch][gin], may be NULL when no count is -1 */
} pe_blend;
int pe_upload_blended(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                      const int64_t* sids, const pe_noise* noise, const pe_timing* timing, const pe_seeds* seeds,
                      const pe_blend* blend);
int pe_synthesize_batch_blended(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                                const int64_t* sids, const pe_noise* noise, pe_result* result, const pe_timing* timing,
                                const pe_seeds* seeds, const pe_blend* blend);
/* gin, the length of a speaker vector (0 for a single-speaker voice), and row `sid` of the speaker table: callers who do
 * their own arithmetic read rows here and come back with a vector (count -1) */
int pe_get_speaker_dim(pe_engine* e, int32_t* gin);
int pe_get_speaker_embedding(pe_engine* e, int64_t sid, float* out, int64_t capacity);
/* test hook: speaker_blend_kernel alone -- out[batch][gin] for the blend and the plain ids (sids, NULL: all 0) of a call,
 * no synthesis. pe_debug_tensor knows the name "g": the [gin] vector utterance b used in the last call (the table row for
 * a plain one). */
int pe_debug_blend(pe_engine* e, const pe_blend* blend, int32_t batch, const int64_t* sids, float* out);
int pe_run(pe_engine* e);
int pe_fetch(pe_engine* e, int want_audio, int want_pcm, pe_result* result);

/* Streaming decode of one utterance (BASELINE.json configs[4]; reference behaviour:
 * src/python/piper_train/infer_onnx_streaming.py:76-124 -- encoder once, then the decoder on chunks of
 * frames). pe_stream_begin runs the text encoder, duration predictor and flow and reports the frame count;
 * every pe_stream_next returns the samples of the next `chunk_frames` frames (reference default 45),
 * decoded on a window padded by the generator's exact receptive half-width (`halo_frames`), so the chunks
 * concatenate to exactly the unchunked waveform. `pcm` is peak-normalised per chunk, like the reference's
 * streaming script. *n_samples == 0 means the utterance is finished. */
int pe_stream_begin(pe_engine* e, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                    const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames);
/* ... under a timing plan and with the utterance's seed (pe_timing, pe_seeds above; seeds->seed[0]) */
int pe_stream_begin_seeded(pe_engine* e, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                           const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames, const pe_timing* timing,
                           const pe_seeds* seeds);
/* ... and with the utterance's speaker blend or vector (pe_blend above, batch = 1) */
int pe_stream_begin_blended(pe_engine* e, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                            const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames, const pe_timing* timing,
                            const pe_seeds* seeds, const pe_blend* blend);
int pe_stream_next(pe_engine* e, int32_t chunk_frames, const float** audio, const int16_t** pcm, int64_t* n_samples);

/* Streaming decode of a whole batch in lock step: B listeners get their first chunk after the text encoder, the duration
 * predictor, the flow and ONE window decode, instead of after the whole batch (pe_synthesize_batch) or behind each other
 * (pe_stream_begin, one utterance per handle at a time).
 *
 * pe_stream_begin_batch begins B utterances together: text encoder, duration predictor and flow for the whole batch, once.
 * Arguments as pe_upload_scaled (ids concatenated, offsets[batch+1], one scales triple per utterance, sids / noise may be
 * NULL). total_frames[batch] receives every utterance's frame count, *halo_frames the generator's receptive half-width. */
int pe_stream_begin_batch(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                          const int64_t* sids, const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames);

/* ... under a timing plan (pe_timing above) */
int pe_stream_begin_batch_timed(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                                const int64_t* sids, const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames,
                                const pe_timing* timing);
/* ... and with per-utterance seeds (pe_seeds above) */
int pe_stream_begin_batch_seeded(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                                 const int64_t* sids, const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames,
                                 const pe_timing* timing, const pe_seeds* seeds);
/* ... and with per-utterance speaker blends (pe_blend above) */
int pe_stream_begin_batch_blended(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t batch, const float* scales,
                                  const int64_t* sids, const pe_noise* noise, int32_t* total_frames, int32_t* halo_frames,
                                  const pe_timing* timing, const pe_seeds* seeds, const pe_blend* blend);

typedef struct pe_stream_chunk {
  int32_t batch;
  const int64_t* sample_offsets; /* [batch+1] prefix offsets of THIS chunk into pcm / audio; a finished utterance has 0 samples */
  const int16_t* pcm;            /* every utterance's chunk, packed back to back; each peak-normalised over ITS OWN chunk */
  const float* audio;            /* the same samples as floats, or NULL unless want_audio */
  const int32_t* frames_done;    /* [batch] frames delivered so far, this chunk included */
} pe_stream_chunk;

/* The next chunk_frames frames of every utterance that still has frames left, decoded as ONE batched generator pass on
 * exact-halo windows: chunk k of utterance b is what pe_stream_next returns for chunk k of that utterance alone (same frame
 * ranges, same per-chunk peak normalisation; the floats equal up to summation order). The peak, the int16 conversion and
 * the packing run on the device and land in pinned host memory: the call ends with one synchronisation. Utterances finish
 * at different calls; a finished one contributes zero samples and keeps frames_done[b] == total_frames[b].
 * sample_offsets[batch] == 0 means every utterance is finished. chunk_frames may differ from call to call (a short first
 * chunk, longer ones after). Views are engine-owned and valid until the next call on the handle. Any other synthesis call
 * on the handle ends the batch stream: a later pe_stream_next_batch is an error ("no batch stream"), not stale data. */
int pe_stream_next_batch(pe_engine* e, int32_t chunk_frames, int want_audio, pe_stream_chunk* out);

/* Stream pool: listeners join and leave a live batch stream. A fixed number of slots whose latents and decoder
 * conditioning live in storage OWNED BY THE POOL, outside the engine's workspaces; every pe_stream_pool_next is one batched
 * window stage over all slots, each slot advancing from its own position.
 *
 * pe_stream_pool_open allocates and zeroes the pool -- latents [slots][channels][max_frames rounded up to 64], conditioning
 * rows, state blocks -- and sizes the workspaces once for a window stage of `slots` utterances. One pool per handle: a
 * second open is an error. *halo_frames receives the generator's receptive half-width.
 *
 * pe_stream_pool_join begins n utterances (arguments as pe_stream_begin_batch: text encoder, durations and flow for the n
 * newcomers, once) and moves their latents into free slots, lowest free slot first, in input order: slot_of[n] receives the
 * slots, total_frames[n] the frame counts. With fewer than n free slots, or an utterance of more than max_frames frames,
 * the whole join fails and the pool is exactly as it was. Like any other upload a join ends a pe_stream_begin /
 * pe_stream_begin_batch stream on the handle.
 *
 * pe_stream_pool_next delivers the next chunk of every occupied slot: chunk_frames frames, or chunk_frames_per_slot[s]
 * where that array is given and its entry is > 0 (a newcomer's short first chunk next to the residents' long ones). The
 * result is a pe_stream_chunk with batch == slots and every array indexed by slot; a listener that joined before call k
 * gets its frames [0, c) at call k, and every chunk is what pe_stream_next returns for that utterance alone. Free slots
 * contribute zero samples. A slot whose last frame has been delivered is free from the next call on; its frames_done
 * stays readable until the slot is reused. sample_offsets[slots] == 0: no slot has frames left (not an error).
 *
 * pe_stream_pool_leave frees an occupied slot at once (the listener hung up); leaving a free slot is an error.
 *
 * The pool survives every other call on the handle -- pe_synthesize*, pe_upload / pe_run / pe_fetch, pe_stream_begin*,
 * pe_warmup, workspace growth -- because nothing it needs between two next calls lives in a workspace. The device-side
 * results of a pe_run that has not been fetched do not: fetch before the next chunk. pe_stream_pool_close and pe_destroy
 * free it. next, join or leave without an open pool: "no stream pool". */
int pe_stream_pool_open(pe_engine* e, int32_t slots, int32_t max_frames, int32_t* halo_frames);
int pe_stream_pool_join(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t n, const float* scales,
                        const int64_t* sids, const pe_noise* noise, int32_t* slot_of, int32_t* total_frames);
/* ... under a timing plan (pe_timing above); a target beyond max_frames is refused like an utterance that long */
int pe_stream_pool_join_timed(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t n, const float* scales,
                              const int64_t* sids, const pe_noise* noise, int32_t* slot_of, int32_t* total_frames,
                              const pe_timing* timing);
/* ... and with per-utterance seeds (pe_seeds above): a newcomer's audio does not depend on the slot it gets */
int pe_stream_pool_join_seeded(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t n, const float* scales,
                               const int64_t* sids, const pe_noise* noise, int32_t* slot_of, int32_t* total_frames,
                               const pe_timing* timing, const pe_seeds* seeds);
/* ... and with per-utterance speaker blends (pe_blend above): a slot's conditioning row is copied from the newcomer's own, so
 * a slot taken by a blended newcomer and later by a plain one inherits nothing */
int pe_stream_pool_join_blended(pe_engine* e, const int64_t* ids, const int64_t* offsets, int32_t n, const float* scales,
                                const int64_t* sids, const pe_noise* noise, int32_t* slot_of, int32_t* total_frames,
                                const pe_timing* timing, const pe_seeds* seeds, const pe_blend* blend);
int pe_stream_pool_next(pe_engine* e, int32_t chunk_frames, const int32_t* chunk_frames_per_slot, int want_audio,
                        pe_stream_chunk* out);
int pe_stream_pool_leave(pe_engine* e, int32_t slot);
int pe_stream_pool_close(pe_engine* e);
/* Host view of the pool: *slots (0: no pool open, the arrays are not written), and per slot the utterance's frame count,
 * the frames delivered so far and whether the slot is occupied (1) or free (0). Any pointer may be NULL. */
int pe_stream_pool_state(pe_engine* e, int32_t* slots, int32_t* total_frames, int32_t* frames_done, int32_t* occupied);

/* Integer per-id durations (ceil(w), reference models.py:703) of the last call, concatenated like ids. */
int pe_get_durations(pe_engine* e, int32_t* out, int64_t capacity, int64_t* n);

/* Voice facts the caller needs (sample rate from the architecture header of a blob, hop size, ...). */
int pe_get_info(pe_engine* e, int32_t* sample_rate, int32_t* hop, int32_t* n_speakers, int32_t* n_symbols,
                int64_t* weight_bytes);

/* Output sample rate. Everything the engine delivers -- pe_result.audio / pcm of pe_synthesize*, pe_fetch, the groups and
 * the coalescer; the chunks of pe_stream_next, pe_stream_next_batch and pe_stream_pool_next -- comes out at the voice's own
 * rate (16 000 Hz for x_low / low voices, 22 050 Hz for medium / high) unless a rate is set here: then the float waveform is
 * resampled ON THE DEVICE, before the int16 conversion, by a polyphase Kaiser-windowed sinc (pass band
 * to 0.92 of the lower Nyquist within 0.07 dB, images and aliases below -90 dB). The reference never resamples; its rule for
 * the int16 conversion -- scale by the maximum of what is delivered, piper.cpp:410-431 -- is kept: the peak is the RESAMPLED
 * waveform's (whole utterance, or chunk), since a band-limited interpolation can overshoot the native one.
 *   native_rate  the voice's rate; 0 = the rate in the voice's header. An .onnx carries none: pass "audio.sample_rate" of the
 *                voice's .onnx.json. A value that contradicts a header's rate is an error, and so is 0 without one.
 *   output_rate  8000 .. 48000 with output / gcd(native, output) <= 640 and a filter half-width (16 * native / (0.92 * the
 *                lower rate) native samples) of at most one hop: 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100 and
 *                48000 qualify for both voice rates. 0 or == native: off -- the engine is exactly the native-rate engine.
 * With a rate set, pe_result.sample_offsets / audio / pcm are in OUTPUT samples: an utterance of S = frames * hop native
 * samples has ceil(S * output / native) of them; `frames` stays in native frames. A stream chunk that covers native samples
 * [s0, s1) delivers outputs [ceil(s0 * output / native), ceil(s1 * output / native)), so an utterance's chunks add up to
 * its whole length and their floats are the whole utterance's resampling; windows are decoded with one more halo frame on
 * each side (*halo_frames reports it), which keeps every chunk stateless. One rate per handle, not per utterance. Setting
 * a rate while a stream, a batch stream or a stream pool is live is an error that changes nothing; any other failure leaves
 * the previous setting in force too. A change drops the captured graphs (a server at a fixed rate stops capturing, as
 * before). pe_get_info keeps reporting the native rate; pe_get_output_rate reports both and the half-width K in native
 * samples (0 while off). */
int pe_set_output_rate(pe_engine* e, int32_t native_rate, int32_t output_rate);
int pe_get_output_rate(pe_engine* e, int32_t* native_rate, int32_t* output_rate, int32_t* half_width);

/* The int16 level of stream chunks. By default every chunk of pe_stream_next, pe_stream_next_batch and pe_stream_pool_next is
 * scaled by 32767 / max(0.01, its own peak), as the reference's streaming script does (infer_onnx_streaming.py:122): the
 * level a listener hears moves at every chunk boundary, and a chunk that holds a pause is amplified by up to 100. Two
 * stream-wide levels stand beside that rule, computed on the device between the chunk's peak and its conversion, with no host
 * round trip. One stream = one pe_stream_begin utterance, one row of a batch stream, or one pool slot from join to its end.
 * x[0 .. n) are the floats a chunk delivers for the stream (output samples when a rate is set; they never change), c = max |x|.
 *   PE_GAIN_CHUNK    the default rule, bit for bit: g = 32767 / max(0.01, c); launches, graphs and buffers as without this call.
 *   PE_GAIN_FIXED    g = 32767 / max(0.01, peak) for every sample of every chunk; no state. peak must be finite and > 0.
 *   PE_GAIN_RUNNING  the stream carries an f32 running peak r = max(0.01, peak) at begin / join (peak 0: no prior; finite,
 *                    >= 0). A chunk with n > 0: r' = max(r, c), g1 = 32767 / r', g0 = g1 on the stream's first delivered
 *                    chunk and 32767 / r otherwise; with R = min(ramp_samples, n), sample i < R is scaled by
 *                    g1 + (g0 - g1) * ((R - 1 - i) / R) and every later one by g1 (the last ramp sample carries exactly
 *                    g1); then r = r'. A chunk with n == 0 delivers nothing and leaves r alone.
 * Products are clamped to [-32768, 32767] and truncated as before. r never falls within a stream, so the gain never rises; a
 * sample can reach the clamp only inside a ramp that contains the new peak (there the gain is still above 32767 / r'). Once
 * the chunk with the utterance's peak has passed, every later sample has the gain pe_synthesize gives it. A pool slot's
 * level is reset by the join that takes it -- a reused slot inherits nothing -- survives every other call on the handle like
 * the slot's latent, and a failed join changes nothing.
 * ramp_samples: 0 .. 65536 delivered samples. peak and ramp_samples are data the kernels read; only the mode picks launches,
 * and every mode's graphs stay cached, so a steady server stops capturing in any mode. Errors that change nothing: an unknown
 * mode, a peak or ramp out of range, and any call while a stream, a batch stream or a stream pool slot is live / occupied.
 * pe_get_stream_gain reads the setting back (any pointer may be NULL). */
enum { PE_GAIN_CHUNK = 0, PE_GAIN_RUNNING = 1, PE_GAIN_FIXED = 2 };
int pe_set_stream_gain(pe_engine* e, int32_t mode, float peak, int32_t ramp_samples);
int pe_get_stream_gain(pe_engine* e, int32_t* mode, float* peak, int32_t* ramp_samples);
/* The last chunk call on the handle, of any of the three kinds: *n rows (1, batch or slots); gain[r] is the end-of-chunk gain
 * g1 of row r and peak[r] the level it came from -- r' when running, max(0.01, c) in the default mode, max(0.01, peak) when
 * fixed. A row that delivered nothing reports its stored state when running and 0 otherwise. gain / peak may be NULL (then
 * only *n is written); capacity < *n is an error. In the default mode a batch stream's or pool's peaks stay on the device and
 * are fetched by this call: ask before the next call that uploads inputs, which is an error ("no longer on the device")
 * afterwards. */
int pe_stream_last_gains(pe_engine* e, float* gain, float* peak, int64_t capacity, int32_t* n);

/* Streams at a target loudness: a fourth stream level, PE_GAIN_LOUDNESS. A stream cannot know its final integrated loudness
 * before it ends, but the gated loudness of what it has delivered SO FAR is known after every chunk -- the figure a live
 * loudness meter shows -- and equals the final value once the last chunk has passed. Each stream carries that running
 * measure on the device and every chunk's gain follows it toward target_lufs under a peak ceiling, with no host round trip
 * (DESIGN.md section 4.9). One stream as above; x_k[0 .. n_k) the floats chunk k delivers, N_k = n_0 + .. + n_k, fs the
 * delivered rate.
 *   L_k        the integrated loudness pe_set_loudness defines (below), of the prefix X[0 .. N_k): the K-weighting runs from
 *              zero state at stream sample 0 THROUGH the chunk boundaries, segments and blocks lie on stream sample indices,
 *              both gates are re-evaluated over all blocks complete so far; PE_LOUD_SHORT while N_k < 4 h,
 *              PE_LOUD_UNMEASURABLE where nothing passes the absolute gate. L of the last chunk is that of the whole of X.
 *   state      running sample peak r (0 at begin / join), previous end-of-chunk gain G, the last loudness used.
 *   a chunk with n_k > 0:
 *              r' = max(r, max |x_k|). Lu = L_k if measurable and not (SHORT with a prior set), else prior_lufs if set
 *              (PE_LOUD_PRIOR), else the stream's last Lu, else none. a = 10^((target_lufs - Lu) / 20) in f64, 1 when there
 *              is none: a stream that is still silent is delivered as generated. cap = (float)(32767 C / r'),
 *              C = 10^(ceiling_db / 20), one ulp less where the rounding would lift r' over the ceiling; +inf when r' = 0.
 *              g1 = min((float)(32767 a), cap), PE_LOUD_LIMITED when the cap is the smaller. g0 = g1 on the stream's first
 *              delivered chunk, else min(G, cap). With R = min(ramp_samples, n_k), sample i < R is scaled by
 *              fma(g0 - g1, (R - 1 - i) / R, g1), every later one by g1; clamp and truncation as before. Then r = r', G = g1.
 *   n_k == 0   moves nothing.
 * Unlike PE_GAIN_RUNNING the gain may rise as well as fall, and g0 is cut to the cap: |pcm| <= floor(32767 C) outside ramps
 * and <= floor(32767 C) + 1 inside them. Not covered on streams: the true-peak ceiling, a slew limit
 * beyond the ramp, stereo. target_lufs in [-40, -5], ceiling_db in [-20, 0], prior_lufs finite in [-70, 0] or NaN for none,
 * ramp_samples 0 .. 65536. Errors that change nothing, each naming the value: a value out of range or not finite, an unknown
 * delivered rate (a voice without a header rate: pe_set_output_rate(native, ...) first), and any call while a stream, a batch
 * stream or a pool slot is live / occupied. All four numbers are data the kernels read in place: new values replay the
 * captured graphs; the mode is part of the graph keys, and all four modes' graphs stay cached side by side.
 * pe_set_stream_gain with one of the other modes leaves this one; pe_get_stream_gain reports mode 3 while it is set.
 * pe_get_stream_loudness reads the setting back (*on: the mode is set; any pointer may be NULL). */
enum { PE_GAIN_LOUDNESS = 3 };
enum { PE_LOUD_PRIOR = 16 };
int pe_set_stream_loudness(pe_engine* e, float target_lufs, float ceiling_db, float prior_lufs, int32_t ramp_samples);
int pe_get_stream_loudness(pe_engine* e, int32_t* on, float* target_lufs, float* ceiling_db, float* prior_lufs, int32_t* ramp_samples);
/* The last chunk call on the handle in that mode: *n rows; lufs[r] = the running loudness L_k of row r (-inf: not measurable),
 * gain[r] = g1, peak[r] = r', flags[r] = PE_LOUD_* bits. A row that delivered nothing in the call reports the state its
 * stream's last chunk left -- a finished row keeps its end state -- and {-inf, 0, 0, SHORT | UNMEASURABLE} while its stream
 * has delivered nothing yet. pe_stream_last_gains reports the same g1 and r'. Any array may be NULL; capacity < *n is an error. */
int pe_stream_last_loudness(pe_engine* e, float* lufs, float* gain, float* peak, int32_t* flags, int64_t capacity, int32_t* n);
/* Test hook, the counterpart of pe_debug_loudness: the production kernels of the mode chunk after chunk on caller-supplied
 * rows x[batch][stride] (host) at rate fs (8000 .. 48000). chunks[n_chunks][batch]: chunk k of row b holds the row's next
 * chunks[k][b] samples (0 allowed; a row's sum <= stride). Out, [n_chunks][batch] each: lufs, g0, g1, flags as reported after
 * that chunk; pcm[batch][stride]: the int16 of every chunk at its place in the row (what no chunk covers is left alone).
 * Independent of the handle's setting and rate. */
int pe_debug_stream_loudness(pe_engine* e, const float* x, int32_t batch, int64_t stride, int32_t fs, const int32_t* chunks,
                             int32_t n_chunks, float target_lufs, float ceiling_db, float prior_lufs, int32_t ramp_samples,
                             float* lufs, float* g0, float* g1, int32_t* flags, int16_t* pcm);

/* Look-ahead limiter on streams at a target loudness. Step 5 above caps the gain at 32767 C / r', and r'
 * only grows: the first plosive lowers the rest of the stream. With the limiter on the stream keeps the gain of its target and
 * only the neighbourhood of its peaks is turned down, by the zero-phase envelope of pe_set_loudness_limiter formed over the WHOLE
 * stream. window_ms in [1, 10]; W = max(1, floor(window_ms fs / 1000 + 0.5)) at the delivered rate fs, D = 2 W. It acts in
 * PE_GAIN_LOUDNESS only; in the other modes it is remembered and nothing changes.
 *   gain       steps 1 to 4 and 7 to 8 above are unchanged. g1 = (float)(32767 a) always; PE_LOUD_LIMITED | PE_LOUD_SHAPED where
 *              cap < g1 (cap from r' as before). g0 = g1 on the stream's first delivered chunk, else G, not cut to the cap.
 *   envelope   with X the stream's floats, s_i the per-sample scale of step 7 and N_end the stream's total:
 *              g_i = (float)((double)s_i / 32767), r[i] = min(1, C / (g_i |X_i|)), 1 where X_i = 0 and outside [0, N_end);
 *              m, d, h and e exactly as pe_set_loudness_limiter defines them; z_i = X_i e_i in f32;
 *              pcm_i = trunc(clamp(z_i s_i, +-floor(32767 C))). e is exactly 1 wherever no sample within 2 W passes the ceiling:
 *              a stream that is never LIMITED delivers the int16 of the mode without the limiter bit for bit, and
 *              |pcm| <= floor(32767 C) on every sample, ramps included.
 *   delivery   e[i] depends on r[i - 2 W .. i + 2 W] only, so the stream holds back D samples: with N_k the stream's floats after
 *              call k and b_-1 = 0, call k hands out the stream samples [b_k-1, b_k), b_k = N_k if the call consumed the row's
 *              last frame, else max(0, N_k - D). The int16 and, on request, the floats (X unchanged) cover that range, and
 *              sample_offsets / n_samples count it. A call may deliver 0 samples for a row that still has frames: the end of a
 *              stream is decided by its frames (frames_done against total_frames; pe_stream_next: by the frames asked for so
 *              far), not by an empty chunk. The loudness and its report stay on the undelayed prefix N_k.
 *              pe_stream_pool_leave drops what a slot holds back.
 * Refused, with the value named and nothing changed: window_ms out of range or not finite (on != 0), an unknown delivered rate,
 * and any call while a stream, a batch stream or a pool slot is live / occupied. On / off and W are part of the graph keys:
 * both sets of graphs stay cached. pe_get_stream_limiter reads on, window_ms, W and D back (any pointer may be NULL). */
int pe_set_stream_limiter(pe_engine* e, int32_t on, float window_ms);
int pe_get_stream_limiter(pe_engine* e, int32_t* on, float* window_ms, int32_t* window_samples, int32_t* delay_samples);
/* The last chunk call on the handle with the limiter: *n rows (0: it ran without); max_reduction[r] = 1 - min e and
 * shaped_samples[r] = the count of e < 1 over the samples that call delivered for row r. Any array may be NULL; capacity < *n is
 * an error. */
int pe_stream_last_limiter(pe_engine* e, float* max_reduction, int32_t* shaped_samples, int64_t capacity, int32_t* n);
/* Test hook: pe_debug_stream_loudness with the limiter of window_ms on, the production kernels chunk after chunk. A row ends
 * with its last chunk of length > 0. Also out: delivered[n_chunks][batch] = samples handed out per call and row;
 * env[batch][stride] = e per stream sample; pcm[batch][stride] holds the int16 in delivery order, which is stream order. */
int pe_debug_stream_limiter(pe_engine* e, const float* x, int32_t batch, int64_t stride, int32_t fs, const int32_t* chunks,
                            int32_t n_chunks, float target_lufs, float ceiling_db, float prior_lufs, int32_t ramp_samples,
                            float window_ms, float* lufs, float* g0, float* g1, int32_t* flags, int32_t* delivered, float* env,
                            int16_t* pcm);

/* Target loudness of whole utterances. By default every utterance of pe_synthesize*, pe_fetch, the groups and the coalescer
 * is scaled by 32767 / max(0.01, its peak) (the reference's rule, piper.cpp:410-431): the PEAK is fixed, the level is not, and a
 * nearly empty phrase is amplified by up to 100. With on != 0 every whole-utterance call delivers its int16 PCM at a target
 * integrated loudness instead, measured and applied on the device with no host round trip:
 *   x[0 .. n)  the floats the call delivers for the utterance, at the delivered rate fs (output samples when a rate is set).
 *              They never change.
 *   y          x through the K-weighting of ITU-R BS.1770-4 (shelf + 38 Hz high-pass, the coefficients of pe_loudness_filter,
 *              zero state at sample 0), mono.
 *   blocks     h = (fs + 5) / 10 samples; z_j = mean of y^2 over [j h, (j + 4) h) for every j with (j + 4) h <= n;
 *              l_j = -0.691 + 10 log10 z_j. Absolute gate l_j > -70; relative gate G = -0.691 + 10 log10(mean z over the
 *              absolute-gated blocks) - 10; L = -0.691 + 10 log10(mean z over blocks with l_j > -70 and l_j > G).
 *   n < 4 h    PE_LOUD_SHORT: one block over the whole utterance (mean of y^2 over n), no relative gate.
 *   silence    nothing passes the absolute gate, or n == 0: PE_LOUD_UNMEASURABLE, scale = 32767 (the waveform as generated).
 *   scale      32767 * min(10^((target_lufs - L) / 20), C / P), C = 10^(ceiling_db / 20), P = p = max |x|, or with the
 *              true-peak ceiling below P = max(p, t); PE_LOUD_LIMITED when the second term is the smaller. One f32 per
 *              utterance; products are clamped to [-32768, 32767] and truncated.
 * The ceiling holds the sample peak by default and the true peak after the call below. The measurement is mono and covers whole
 * utterances only: pe_stream_next, pe_stream_next_batch and pe_stream_pool_next keep their chunk rule and the
 * pe_set_stream_gain modes -- a stream follows a RUNNING loudness instead, pe_set_stream_loudness above -- and the setting may
 * change while a stream is live. target_lufs in [-40, -5], ceiling_db in [-20, 0], both finite (on == 0: ignored); a voice without
 * a header rate needs pe_set_output_rate(native, ...) first. A refused call names the value and changes nothing. target and
 * ceiling are data the kernels read in place: new values replay the captured graphs; on / off is part of the graph keys.
 * With on == 0 -- the default -- every launch, graph and bit of output is what it is without this call. One setting per
 * handle (the engines of a group: pe_group_engine). pe_get_loudness reads it back (any pointer may be NULL). */
enum { PE_LOUD_SHORT = 1, PE_LOUD_UNMEASURABLE = 2, PE_LOUD_LIMITED = 4 };
int pe_set_loudness(pe_engine* e, int32_t on, float target_lufs, float ceiling_db);
int pe_get_loudness(pe_engine* e, int32_t* on, float* target_lufs, float* ceiling_db);
/* The last fetched whole-utterance call on the handle: *n utterances (0: it ran with the setting off); lufs[i] = L (-inf when
 * not measurable), scale[i], peak[i] = p, flags[i] = PE_LOUD_* bits. Any array may be NULL; capacity < *n is an error. */
int pe_last_loudness(pe_engine* e, float* lufs, float* scale, float* peak, int32_t* flags, int64_t capacity, int32_t* n);
/* Host only: the K-weighting biquads at rate fs (4000 .. 192000), bilinear transforms of the analog prototypes computed in
 * f64: coef = shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2} (a0 = 1). At 48000 Hz the table of BS.1770-4. */
int pe_loudness_filter(int32_t fs, double coef[10]);
/* Test hook: the two loudness kernels alone on caller-supplied rows x[batch][stride] (host), row b holding valid[b] samples at
 * rate fs, with the given target and ceiling: lufs / scale / flags [batch] as pe_last_loudness reports them. Independent of
 * the handle's setting and rate. */
int pe_debug_loudness(pe_engine* e, const float* x, int32_t batch, int64_t stride, const int32_t* valid, int32_t fs,
                      float target_lufs, float ceiling_db, float* lufs, float* scale, int32_t* flags);

/* What the ceiling of the target loudness holds. PE_PEAK_SAMPLE, the default: p, the largest |sample|. PE_PEAK_TRUE: the true
 * peak of ITU-R BS.1770-4 Annex 2 as well, which delivery specifications name (EBU R128: -23 LUFS, at most -1 dBTP). It is
 * measured on the device by one more launch per whole-utterance call, with no host round trip:
 *   Q          ceil(192000 / fs): 4 at 48000 Hz, 5 at 44100, 9 at 22050, 12 at 16000, 24 at 8000.
 *   y[m]       x interpolated Q times, m = 0 .. n Q - 1, x = 0 outside [0, n), by the filter the rate conversion builds for the
 *              pair fs -> Q fs: Kaiser-windowed sinc, cutoff 0.46 fs, 16 zero crossings a side, beta = 8.6, half-width
 *              K = 18 samples of x; computed in f64, rounded once to f32.
 *   t          max |y[m]| (0 for n == 0); P = max(p, t), because phase 0 of that filter has gain 0.92, not 1: a lone
 *              impulse of 1.0 has t = 0.92.
 * The measure is flat within the rate conversion's 0.07 dB up to 0.8 of the Nyquist frequency and under-reads above it
 * (-3.8 dB at 0.9 of Nyquist, computed in f64) -- the compromise Annex 2's own filter makes. Everything else of the loudness
 * setting is unchanged, and pe_last_loudness keeps reporting p. The kind may be set while the loudness is off (it is
 * remembered and takes effect once it is on) and while a stream is live (streams do not see it). An unknown kind is refused
 * with a message that names the value, and so is PE_PEAK_TRUE while the loudness is on at a delivered rate outside
 * [8000, 48000] Hz; pe_set_loudness and pe_set_output_rate refuse what would make that combination true. A refused call
 * changes nothing. The kind is part of the graph keys next to on / off; with PE_PEAK_SAMPLE every launch, graph and bit of
 * output is what it is without this call. The read-back gives the kind, Q at the delivered rate (0 where the rate is unknown
 * or outside the range) and K; any pointer may be NULL. */
enum { PE_PEAK_SAMPLE = 0, PE_PEAK_TRUE = 1 };
int pe_set_loudness_ceiling(pe_engine* e, int32_t kind);
int pe_get_loudness_ceiling(pe_engine* e, int32_t* kind, int32_t* oversample, int32_t* half_width);
/* The last fetched whole-utterance call on the handle: true_peak[i] = t of utterance i, *n utterances (0: it did not run with
 * PE_PEAK_TRUE and the loudness on). true_peak may be NULL; capacity < *n is an error. */
int pe_last_true_peak(pe_engine* e, float* true_peak, int64_t capacity, int32_t* n);
/* Host only: the interpolator at rate fs (8000 .. 48000) in f64, before the rounding to f32: *oversample = Q, *half_width = K,
 * *n = Q * 2 K, and coef[ph * 2 K + k] = the tap of phase ph on x[c - K + 1 + k] for the outputs y[c Q + ph] (coef may be
 * NULL to ask for *n; capacity < *n is an error). */
int pe_true_peak_filter(int32_t fs, int32_t* oversample, int32_t* half_width, double* coef, int64_t capacity, int64_t* n);
/* Test hook: the true-peak kernel alone on caller-supplied rows x[batch][stride] (host), row b holding valid[b] samples at
 * rate fs: t[batch]. Independent of the handle's setting and rate. */
int pe_debug_true_peak(pe_engine* e, const float* x, int32_t batch, int64_t stride, const int32_t* valid, int32_t fs, float* t);

/* Look-ahead limiter of the target loudness. Off, the default: when the ceiling and the target conflict the whole utterance
 * is lowered (PE_LOUD_LIMITED), so one plosive decides the level of a sentence. On: such an utterance keeps the gain of its
 * target, g = 10^((target_lufs - L) / 20), and a zero-phase envelope turns down the neighbourhood of its peaks only
 * (PE_LOUD_SHAPED, set next to PE_LOUD_LIMITED, which keeps its meaning: C / P < g). Every other utterance is delivered bit
 * for bit as with the limiter off. On the device, one launch in the conversion's place:
 *   W          max(1, floor(window_ms fs / 1000 + 0.5)) samples at the delivered rate fs: 8 at 8000 Hz with 1 ms, 480 at
 *              48000 Hz with 10 ms.
 *   r[i]       min(1, C / (g |x[i]|)), 1 where x[i] = 0 and outside [0, n)
 *   m[j], d    m[j] = min r[j - W .. j + W], d = 1 - m
 *   e[i]       min(r[i], 1 - sum_{k = -W .. W} h_k d[i + k]), h_k = H_k / sum H, H_k = (1 + cos(pi k / (W + 1))) / 2; e is
 *              exactly 1 wherever no sample within 2 W passes the ceiling
 *   pcm[i]     trunc(clamp((x[i] e[i]) * scale, +-floor(32767 C))), scale = 32767 g: |pcm| <= 32767 C holds exactly
 * With PE_PEAK_TRUE the rule's P is max(p, t) as before, and in r stands a[i] = max(|x[i]|, v[i - 1], v[i]) for |x[i]|,
 * v[c] = max over ph of |y[c Q + ph]| of the true-peak interpolation (v[-1] = 0); z = x e is kept in f32, its sample peak p_z
 * and true peak t_z are measured by the same kernel that measures t, and scale = 32767 min(g, C / max(p_z, t_z)) with the
 * one-ulp lowering of the ceiling's term: three launches more. The second term is a guarantee, not the mechanism; it is
 * reported as trim = min(1, C / (g max(p_z, t_z))). The rate refusals of PE_PEAK_TRUE hold as without the limiter.
 * The float `audio` a call returns stays x, unchanged: only the int16 is shaped. pe_last_loudness reports the scale that was
 * used and L, the measured loudness of x; the delivered loudness is NOT measured again and there is no make-up gain, so it
 * lies at or below target_lufs (by a few tenths of a dB on speech with 5 ms, the recommended window). window_ms in [1, 10],
 * finite (on == 0: ignored); a value outside is refused with a message that names it, before anything changes, and so is a
 * window of more than 480 samples at the delivered rate. The setting is remembered while the loudness is off. Only whole-utterance calls use it; streams,
 * batch streams and the pool are untouched. On / off is part of the graph keys; a new window_ms or delivered rate drops the
 * captured graphs. The read-back gives on / off, window_ms and W at the delivered rate (0 where the rate is unknown); any
 * pointer may be NULL. */
enum { PE_LOUD_SHAPED = 8 };
int pe_set_loudness_limiter(pe_engine* e, int32_t on, float window_ms);
int pe_get_loudness_limiter(pe_engine* e, int32_t* on, float* window_ms, int32_t* window_samples);
/* The last fetched whole-utterance call on the handle, per utterance: max_reduction[i] = 1 - min e, shaped_samples[i] = the
 * count of samples with e < 1 (both 0 for an utterance that is not shaped), trim[i] = min(1, C / (g max(p_z, t_z))) with
 * PE_PEAK_TRUE and 1 with PE_PEAK_SAMPLE, which holds by construction. *n utterances (0: the call did not run with the limiter and the
 * loudness on). Any array may be NULL; capacity < *n is an error. */
int pe_last_limiter(pe_engine* e, float* max_reduction, int32_t* shaped_samples, float* trim, int64_t capacity, int32_t* n);
/* Host only: *window_samples = W and the weights h_k in f64, before the rounding to f32: coef[k + W], k = -W .. W, *n =
 * 2 W + 1 (coef may be NULL to ask for *n; capacity < *n is an error). */
int pe_limiter_window(int32_t fs, float window_ms, int32_t* window_samples, double* coef, int64_t capacity, int64_t* n);
/* Test hook: the limiter kernel alone on caller-supplied rows x[batch][stride] (host), row b holding valid[b] samples at rate
 * fs with the gain g[b] (scale = 32767 g[b], one f32 product; shaped iff C / max |x| < g[b]). env_out[batch][stride] receives e
 * (1 on rows that are not shaped) and pcm_out[batch][stride] the int16; what lies behind a row's end is left as it was.
 * kind: PE_PEAK_SAMPLE, or PE_PEAK_TRUE (fs in [8000, 48000]; shaped iff C / max(p, t) < g[b]; the four launches of that path).
 * Independent of the handle's setting and rate. */
int pe_debug_limiter(pe_engine* e, const float* x, int32_t batch, int64_t stride, const int32_t* valid, int32_t fs, const float* g,
                     float ceiling_db, int32_t kind, float window_ms, float* env_out, int16_t* pcm_out);

/* Sample format of what the handle delivers. PE_FORMAT_S16, the default: int16 and floats, nothing changes.
 * PE_FORMAT_ULAW / PE_FORMAT_ALAW: every whole-utterance call and every chunk of every kind of stream ALSO delivers one G.711
 * code (8-bit mu-law, RTP payload type 0, or A-law, payload type 8) per delivered int16 sample, companded on the device and
 * packed back to back under the same sample_offsets; pe_last_codes hands them out. The int16 and the floats are delivered
 * exactly as without a format, bit for bit, and pe_result / pe_stream_chunk keep their layouts; a caller that wants the
 * codes only passes want_pcm = 0 to pe_fetch. The law is that of the ITU-T G.191 software tools, with lin an int16,
 * >> arithmetic and ~ one's complement:
 *   mu-law:  a = (lin < 0 ? (~lin) >> 2 : lin >> 2) + 33;  if (a > 0x1FFF) a = 0x1FFF;
 *            seg = 1; for (i = a >> 6; i; i >>= 1) seg++;
 *            code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF));  if (lin >= 0) code |= 0x80;
 *   A-law:   ix = lin < 0 ? (~lin) >> 4 : lin >> 4;
 *            if (ix > 15) { e = 1; while (ix > 31) { ix >>= 1; e++; }  ix = ix - 16 + (e << 4); }
 *            if (lin >= 0) ix |= 0x80;   code = ix ^ 0x55;
 * so code(0) is 0xFF / 0xD5, the byte a caller pads silence with (0x00 is full-scale negative in mu-law). Cost: one launch
 * more per whole-utterance call and per chunk of a batch stream or pool (pe_run_launches); the one-utterance stream converts
 * on the host, as it does its int16. A value outside the enum is refused, and so is any change while a stream is live or a
 * pool is open on the handle, with a message that says which; nothing changes then. The format is part of the graph keys:
 * switching drops nothing. pe_group_* and pe_coalescer_* keep working on handles with a format set, but do NOT hand out
 * codes: their results carry int16 only. */
enum { PE_FORMAT_S16 = 0, PE_FORMAT_ULAW = 1, PE_FORMAT_ALAW = 2 };
int pe_set_sample_format(pe_engine* e, int32_t format);
int pe_get_sample_format(pe_engine* e, int32_t* format);
/* Codes of the last fetched whole-utterance call (which = 0) or of the last chunk of any kind of stream (which = 1):
 * engine-owned views valid until the next call, row i at codes[sample_offsets[i] .. sample_offsets[i + 1]); *codes == NULL
 * and *rows == 0 when the format was PE_FORMAT_S16. */
int pe_last_codes(pe_engine* e, int32_t which, const uint8_t** codes, const int64_t** sample_offsets, int32_t* rows);
/* Host twins, no engine needed: the law above and its expanders (format PE_FORMAT_ULAW or PE_FORMAT_ALAW). */
int pe_g711_encode(int32_t format, const int16_t* pcm, uint8_t* codes, int64_t n);
int pe_g711_decode(int32_t format, const uint8_t* codes, int16_t* pcm, int64_t n);
/* Test hook: the rows form (flat = 0) or the flat form (flat = 1, batch = 1) of the encoder kernel alone on caller-given int16
 * rows x[batch][stride], row b holding valid[b] samples; out receives the packed codes: out_capacity bytes are uploaded first
 * and read back whole, so untouched bytes come back as given. */
int pe_debug_g711(pe_engine* e, int32_t format, int32_t flat, const int16_t* x, int32_t batch, int64_t stride,
                  const int32_t* valid, uint8_t* out, int64_t out_capacity);

/* Test hook: the resampling kernel with the engine's current rate pair on caller-supplied rows. x[batch][stride] (host): row
 * b holds valid[b] native samples of an utterance, the first of which has native index origin[b]; everything outside them
 * counts as zero. out[b][0 .. count[b]) receives outputs n0[b] .. n0[b] + count[b] - 1 of that utterance (out_stride floats
 * per row). Lets a test feed tones and place n0 beyond 2^31 / M without a long utterance. An error while no rate is set. */
int pe_debug_resample(pe_engine* e, const float* x, int32_t batch, int64_t stride, const int32_t* valid, const int64_t* n0,
                      const int32_t* count, const int64_t* origin, float* out, int64_t out_stride);

/* Test hook: the timing-plan kernel alone on caller-supplied logw rows (concatenated, offsets[batch + 1]) with one scales
 * triple per utterance and a plan (NULL: none). dur_out / w_out receive d_i and w_i, concatenated alike (w_out may be NULL),
 * frames_out[batch] the frame counts. Plans of 8192 ids cost no synthesis this way. */
int pe_debug_timing(pe_engine* e, const float* logw, const int64_t* offsets, int32_t batch, const float* scales,
                    const pe_timing* timing, int32_t* dur_out, int32_t* frames_out, float* w_out);

void pe_set_seed(pe_engine* e, uint64_t seed);

/* Timing with HIP events on the engine's stream. level 1: one pair per pipeline stage (rows
 * text_encoder, duration_predictor, regulate+flow, hifigan, post+pcm). level 2: additionally one pair
 * around every conv / attention / layer-norm launch (rows named after the kernel), with the launch's
 * algorithmic FLOPs (the output-rate conversion: row resample_kernel, with its algorithmic bytes). ms/flops/launches accumulate until pe_profile_reset(); 0 switches it off. */
int pe_profile_enable(pe_engine* e, int level);
int pe_profile_reset(pe_engine* e);
int pe_profile_rows(pe_engine* e);
int pe_profile_get(pe_engine* e, int row, const char** name, double* ms, double* flops, int64_t* launches);
/* level 2 rows of the conv kernels also carry the launches' algorithmic HBM bytes (inputs + outputs + residual
 * operands + weights once), the denominator for comparing PMC-measured traffic against */
int pe_profile_bytes(pe_engine* e, int row, double* bytes);

/* The HIP stream (hipStream_t) the engine launches on, for callers that bracket it with their own events. */
void* pe_stream(pe_engine* e);

/* Test hook: copy an internal per-stage tensor of utterance b: x_enc, stats (rows m_p then logs_p, models.py:208),
 * xg, logw, plan_w (w_i of a timed call), z_p (only with PIPER_HIP_DEBUG_KEEP=1 in the environment at pe_create), z, noise_w,
 * noise_z, audio. */
int pe_debug_tensor(pe_engine* e, const char* name, int32_t b, float* out, int64_t capacity, int32_t* rows,
                    int32_t* cols);

/* Test hooks for the N(0,1) generator behind the graph's two RandomNormalLike sites (models.py:111, :718) when no
 * noise is injected. A site's stream is a logical [row][65536] array, row = utterance * channels + channel (2 channels
 * at site 0, inter_channels at site 1), column = phoneme id / frame: the value the pipeline uses there depends on
 * (seed, run counter, site, row, column) only -- not on batch buckets or workspace sizes. pe_debug_randn fills out[n]
 * with draws row * 65536 .. + n of site 0/1 at run counter `call` under the current seed; pe_rng_calls is the number
 * of pipeline runs so far (the counter the next run will use is that + 1). */
int pe_debug_randn(pe_engine* e, int32_t site, uint64_t call, int64_t row, int64_t n, float* out);
uint64_t pe_rng_calls(pe_engine* e);

/* Kernel launches (hipGraph kernel nodes) the last pe_run / pe_synthesize* issued: the length of the dependent
 * launch chain one utterance costs (the latency figure of merit at batch 1). */
int64_t pe_run_launches(pe_engine* e);

/* Calls of <= 4 utterances enqueue the second half of the pipeline (flow + vocoder) for a GUESSED frame bucket right
 * behind the first half -- the frame count is the graph's only data-dependent shape (reference models.py:702-716) and
 * would otherwise cost a host round trip mid-pipeline. The guess (running maximum of frames per id x an adaptive
 * margin) is verified when the results are fetched; a miss re-runs the second half. runs = calls issued that way since
 * pe_create, misses = guesses that were too small (each cost one extra pass of the second half). */
int pe_speculation_stats(pe_engine* e, int64_t* runs, int64_t* misses);

/* Session warm-up -- what loadModel's session creation does for ORT (piper.cpp:262-306: graph optimisation at load), here
 * for the hipGraphs: the kernel sequence of a call is captured once per shape bucket (ids in steps of 32 up to 512, then
 * 8 steps per octave; frames in steps of 64 up to 1024, then 16 per octave) and replayed afterwards; the cache keeps the
 * 256 most recently used graphs (PIPER_HIP_GRAPHS) and evicts one at a time. The scales are not part of a graph (the
 * kernels read each utterance's triple from the call's input block), so one warm-up serves every scale value. pe_warmup
 *   - sizes the workspaces for calls of up to max_batch utterances x max_ids ids and frames_per_id * max_ids frames
 *     (<= 0: 8), so that no later call grows them (growth re-creates every graph), and
 *   - if sample_ids is given (a representative utterance of the voice: its frames-per-id ratio seeds the speculative
 *     sizing), synthesises it cut / tiled to every id bucket up to max_ids with `scales` (NULL: 0.667 / 1 / 0.8), so that
 *     the single-utterance graphs exist before the first real call.
 * pe_graph_stats: graphs currently cached / captures since pe_create (a steady server stops capturing). */
int pe_warmup(pe_engine* e, int32_t max_batch, int32_t max_ids, float frames_per_id, const float scales[3],
              const int64_t* sample_ids, int64_t n_sample);
int pe_graph_stats(pe_engine* e, int64_t* cached, int64_t* captures);

/* Diagnostic: which XCD (accelerator complex of the MI355X) ran workgroups 0..63 of a 1-D probe launch at pe_create
 * (xcc[64]), and *period = P when that was a round-robin over P XCDs (0 otherwise). The small-call kernels order their
 * column tiles by it (piper_amd/csrc/kernels/col4.h); bench.py prints it so that a result line says what the box did. */
int pe_xcc_pattern(pe_engine* e, int32_t xcc[64], int32_t* period);

/* Diagnostic: the PCI bus id ("0000:05:00.0") of HIP device `device` as this process sees it -- what a multi-GPU record
 * lists per rank so that a reader can check that N ranks ran on N DISTINCT devices (bench.py --gpus N). */
int pe_device_pci_bus_id(int device, char* out, int32_t capacity);

/* Diagnostic: the engine's launch-policy knobs -- every environment variable that picks a kernel form, with its default,
 * range and meaning -- as a JSON array of {"env", "default", "lo", "hi", "doc"} objects (piper_amd/csrc/policy.h; a
 * static string, valid for the life of the process). The knobs are read once per engine, at pe_create; the product needs
 * none of them (onnxruntime's session options are the reference's counterpart, src/cpp/piper.cpp:262-306). */
const char* pe_policy_describe(void);

/* In-process multi-GPU synthesis for C / C++ callers (the reference runs the phrases of a text one
 * after the other on one session, src/cpp/piper.cpp:549-582 -- they are independent, so they shard). One engine, one
 * stream and one worker thread per device. The voice is parsed and packed ONCE, on devices[0]; every other device gets an
 * identically laid out arena (pe_create_in_arena, skeleton) and receives the packed weights by ONE RCCL broadcast over
 * xGMI (ncclBroadcast on a communicator of the group's distinct devices; peer copies when librccl cannot be loaded) -- the
 * in-process counterpart of the torch.distributed broadcast in piper_amd/dist.py. A call deals its
 * utterances to the devices in longest-first order onto the least-loaded device (load = phoneme ids), runs the shards
 * concurrently and returns group-owned host views in the CALLER's order: sample_offsets / pcm / frames as in pe_result,
 * `audio` is NULL (fetch floats per engine if needed), infer_seconds = wall time of the whole call. The same device may
 * be listed more than once (engines sharing a GPU): a call then COALESCES that device's utterances onto as few of its
 * engines as 64-utterance shares need -- one batched call beats several single-utterance pipelines racing for the launch
 * path -- and pe_group_assignment reports which engines ran. Not thread-safe: one call at a time per group. */
typedef struct pe_group pe_group;
int pe_group_create(const void* blob, size_t nbytes, const int32_t* devices, int32_t n_devices, pe_group** out);
/* How the last pe_group_create on this thread moved the packed weights between devices: "rccl" (one ncclBroadcast on a
 * communicator of the group's distinct devices -- librccl is dlopen'ed on first use), "peer-copy (<why RCCL was not used>)",
 * "same-device" (all engines share one GPU) or "none" (one engine). PIPER_HIP_GROUP_BCAST=peer forces the copies, =rccl
 * takes the collective even for a single device (self-test on a one-GPU box). */
const char* pe_group_broadcast_path(void);
int32_t pe_group_size(pe_group* g);
/* Member i of the group, e.g. for pe_set_seed / pe_get_info / pe_profile_* per device. Seeds: pe_group_create gives member i the
 * default seed + i (1234 + i), so that no two members draw the same noise for their share of a call; pe_set_seed on a member
 * overrides it (to re-seed a whole group keep the rule: seed + i for member i). */
pe_engine* pe_group_engine(pe_group* g, int32_t i);
int pe_group_synthesize_batch(pe_group* g, const int64_t* ids, const int64_t* offsets, int32_t batch,
                              const float scales[3], const int64_t* sids, pe_result* result);
/* ... with one triple per utterance (scales[batch * 3], as pe_synthesize_batch_scaled): each shard takes its utterances'
 * triples along with their ids */
int pe_group_synthesize_batch_scaled(pe_group* g, const int64_t* ids, const int64_t* offsets, int32_t batch,
                                     const float* scales, const int64_t* sids, pe_result* result);
/* ... and with per-utterance seeds (pe_seeds above; NULL: exactly the _scaled call): each shard takes its utterances' seeds
 * along with their ids, so a seeded utterance's audio does not depend on the member that ran it */
int pe_group_synthesize_batch_seeded(pe_group* g, const int64_t* ids, const int64_t* offsets, int32_t batch,
                                     const float* scales, const int64_t* sids, pe_result* result, const pe_seeds* seeds);
/* ... and with per-utterance speaker blends (pe_blend above; NULL: exactly the _seeded call): each shard takes its
 * utterances' blends along with their ids */
int pe_group_synthesize_batch_blended(pe_group* g, const int64_t* ids, const int64_t* offsets, int32_t batch,
                                      const float* scales, const int64_t* sids, pe_result* result, const pe_seeds* seeds,
                                      const pe_blend* blend);
/* which engine (index into the group) ran utterance i of the last call */
int pe_group_assignment(pe_group* g, int32_t* engine_index, int64_t capacity);
void pe_group_destroy(pe_group* g);

/* Concurrent single-utterance requests as batched engine calls (dynamic batching). The reference serves one phrase at a
 * time on one session (src/cpp/piper.cpp:549-582; its HTTP server, src/python_run/piper/http_server.py, one request at a
 * time); a server on this engine has many caller threads, each with ONE utterance. An engine handle is not thread-safe and a
 * B=1 pipeline leaves most of the chip idle, so: every thread calls pe_coalescer_synthesize (thread-safe, blocking); the
 * thread that finds the engine free leads -- it takes every request queued at that moment with the same scales (up to
 * max_batch; after waiting up to max_wait_us for stragglers, 0 = never wait) and runs them as ONE pe_synthesize_batch-style
 * call while later arrivals queue up for the next leader. Each request gets exactly what its own B=1 call computes: its
 * own noise draws, and int16 PCM peak-normalised over ITS waveform (piper.cpp:410-431) -- the batched kernels treat
 * utterances independently. *pcm is malloc'ed for the caller (pe_free). *batch_size = utterances of the engine call that
 * served the request. pe_coalescer_stats: engine calls / requests so far. The engine must outlive the coalescer and must
 * not be used directly while requests are in flight. */
typedef struct pe_coalescer pe_coalescer;
int pe_coalescer_create(pe_engine* e, int32_t max_batch, int32_t max_wait_us, pe_coalescer** out);
/* The same, but the leader merges queued requests WHATEVER their scales and uploads one triple per request
 * (pe_upload_scaled): a server whose clients set their own speaking rate still runs one batched call. Each request still
 * gets what its own B=1 call with its own scales computes. Requests with a non-finite scale are rejected on entry. */
int pe_coalescer_create_mixed(pe_engine* e, int32_t max_batch, int32_t max_wait_us, pe_coalescer** out);
int pe_coalescer_synthesize(pe_coalescer* c, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                            int16_t** pcm, int64_t* n_samples, int32_t* frames, double* infer_seconds, int32_t* batch_size);
/* ... with the request's noise seed (*seed; pe_seeds above), NULL for an unseeded request: exactly the call above. Both kinds
 * of coalescer merge seeded and unseeded requests into one engine call; a seeded request gets the noise of its own seeded
 * B = 1 call whatever it was merged with. */
int pe_coalescer_synthesize_seeded(pe_coalescer* c, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                                   const uint64_t* seed, int16_t** pcm, int64_t* n_samples, int32_t* frames,
                                   double* infer_seconds, int32_t* batch_size);
/* ... with the request's speaker blend or vector: `blend` is ONE request's count[1], sid, weight, vector[gin] (pe_blend
 * above), NULL for a plain request: exactly the call above. Both kinds of coalescer merge blended and plain requests into
 * one engine call; a blended request gets what its own B = 1 blended call computes. A blend the law refuses fails its own
 * request before it is queued. */
int pe_coalescer_synthesize_blended(pe_coalescer* c, const int64_t* ids, int64_t n_ids, const float scales[3], int64_t sid,
                                    const uint64_t* seed, const pe_blend* blend, int16_t** pcm, int64_t* n_samples,
                                    int32_t* frames, double* infer_seconds, int32_t* batch_size);
int pe_coalescer_stats(pe_coalescer* c, int64_t* engine_calls, int64_t* requests);
void pe_coalescer_destroy(pe_coalescer* c);

const char* pe_last_error(void);
void pe_destroy(pe_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* PIPER_HIP_H_ */
