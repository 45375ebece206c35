// Host engine, life cycle and the synthesis call: construction / destruction, the XCD probe, workspaces, upload, the
// hipGraph cache (capture per shape bucket, LRU), run / finish_run with speculative stage-B sizing, download, streaming, debug
// hooks. Weight packing: engine_pack.cpp; launchers: engine_launch.cpp; the kernel sequences: engine_issue.cpp; which
// kernel form a launch takes: policy.h.
#include "engine_internal.h"

#include <array>
#include <numeric>

namespace pe {

thread_local long g_launches = 0;
std::shared_mutex g_capture_mu;
thread_local int g_entry_depth = 0;

// PIPER_HIP_DEBUG_POISON: a freshly allocated workspace is filled with NaN bit patterns so that a kernel relying on memory
// it never wrote shows up in the result. The fill runs on the null stream and is asynchronous to the host, while the
// engine's stream does not synchronise with the null stream: without the wait below the fill could land AFTER the first
// copies / launches into the new buffer (seen as NaNs in the first injected noise row, profiles/r05_notes.md, call 31-35).
static void poison(void* p, size_t bytes) {
  PE_HIP(hipMemset(p, 0xFF, bytes));
  PE_HIP(hipDeviceSynchronize());
}

Engine::Engine(const WeightSet& ws, int device, ArenaSpec arena) : device_(device) {
  EntryLock entry_lock;       // allocations / synchronising copies must not overlap another engine's graph capture
  // a constructor that throws does not run the destructor: release what was acquired so far
  try {
    PE_HIP(hipSetDevice(device_));
    skeleton_ = arena.skeleton;
    if (arena.base) {
      if (((uintptr_t)arena.base & 255) != 0) throw std::runtime_error("weight arena must be 256-byte aligned");
      arena_ = static_cast<char*>(arena.base);
      arena_bytes_ = arena.bytes;
    } else {
      if (skeleton_) throw std::runtime_error("a skeleton engine needs a caller-provided arena");
      arena_bytes_ = arena_bound(ws);
      PE_HIP(hipMalloc((void**)&arena_, arena_bytes_));
      arena_owned_ = true;
    }
    init(ws);
  } catch (...) {
    free_all();
    throw;
  }
}

Engine::~Engine() { free_all(); }

void Engine::arena_ready() {
  EntryLock entry_lock;
  PE_HIP(hipSetDevice(device_));
  float m = 0.f, lg = 0.f;
  PE_HIP(hipMemcpy(&m, ea_dev_m_, sizeof(float), hipMemcpyDeviceToHost));
  PE_HIP(hipMemcpy(&lg, ea_dev_logs_, sizeof(float), hipMemcpyDeviceToHost));
  ea_m0_ = m;
  ea_es0_ = std::exp(-lg);
  skeleton_ = false;
}

void Engine::free_all() {
  EntryLock entry_lock;
  if (stream_) hipStreamSynchronize(stream_);
  drop_graphs();
  for (void* p : owned_) hipFree(p);
  owned_.clear();
  if (arena_owned_ && arena_) hipFree(arena_);
  arena_ = nullptr;
  if (wsA_) hipFree(wsA_);
  if (wsB_) hipFree(wsB_);
  if (h_audio_) hipHostFree(h_audio_);
  if (h_pcm_) hipHostFree(h_pcm_);
  if (h_pcm_zc_) hipHostFree(h_pcm_zc_);
  if (h_frames_) hipHostFree(h_frames_);
  if (h_in_) hipHostFree(h_in_);
  h_in_ = nullptr; h_in_cap_ = 0;
  if (h_plan_) hipHostFree(h_plan_);
  h_plan_ = nullptr; h_plan_cap_ = 0;
  rows_free(batch_rows_);
  sb_active_ = false;
  stream_pool_free();
  rs_free();
  loud_free();
  if (ev0_) hipEventDestroy(ev0_);
  if (ev1_) hipEventDestroy(ev1_);
  for (auto& k : kev_) { hipEventDestroy(k.a); hipEventDestroy(k.b); }
  kev_.clear();
  for (hipEvent_t e : ev_pool_) hipEventDestroy(e);
  ev_pool_.clear();
  for (float*& p : side_) { if (p) hipFree(p); p = nullptr; }
  if (ffn_parts_) { hipFree(ffn_parts_); ffn_parts_ = nullptr; }
  if (stream_) hipStreamDestroy(stream_);
  wsA_ = wsB_ = nullptr; h_audio_ = nullptr; h_pcm_ = nullptr; h_pcm_zc_ = nullptr; h_frames_ = nullptr;
  ev0_ = ev1_ = nullptr; stream_ = nullptr;
}

// Which XCD runs which workgroup of a small 1-D launch (kernels/glue.h xcc_probe_kernel). The 4-column kernels hand out
// column tiles so that one XCD owns a contiguous run of them (col4.h c4_tile); that needs the dispatch to be a
// round-robin over P XCDs -- workgroup i on XCD pattern[i mod P], the first P all different -- which is what this checks.
// Anything else (PIPER_HIP_XCD=0 forces it): period 0, tiles in workgroup order.
void Engine::probe_xcds() {
  int* d = nullptr;
  PE_HIP(hipMalloc((void**)&d, 64 * sizeof(int)));
  PE_HIP(hipMemsetAsync(d, 0xff, 64 * sizeof(int), stream_));
  launch::xcc_probe(stream_, d);
  PE_HIP(hipMemcpyAsync(xcc_of_, d, 64 * sizeof(int), hipMemcpyDeviceToHost, stream_));
  PE_HIP(hipStreamSynchronize(stream_));
  PE_HIP(hipFree(d));
  int P = 0;
  for (int c = 1; c <= 32 && !P; ++c) {           // smallest period with pairwise different ids inside it
    bool ok = true;
    for (int i = 0; i < c && ok; ++i)
      for (int j = 0; j < i && ok; ++j) ok = xcc_of_[i] != xcc_of_[j];
    for (int i = c; i < 64 && ok; ++i) ok = xcc_of_[i] == xcc_of_[i - c];
    if (ok && c > 1 && xcc_of_[c] == xcc_of_[0]) P = c;
  }
  xcd_period_ = P;
  if (pol_.xcd >= 0) xcd_period_ = (int)pol_.xcd;       // PIPER_HIP_XCD (A/B, tests): 0 = tiles in workgroup order
}

// ------------------------------------------------------------------------------------------------
// workspaces
// ------------------------------------------------------------------------------------------------

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(char* b) : base(b) {}
  template <class T> T* take(size_t n) {
    off = (off + 255) / 256 * 256;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// Workspace policy. Capacities only grow while the grown block fits the budget (a third of the device's memory per
// stage): utterance count and padded length are separate capacities, so a huge batch of short texts followed by one long
// text would otherwise ask for their product. A call whose grown capacities do not fit gets a block sized for exactly
// that call (capacities may shrink); a call that does not fit by itself is an error, raised before anything changes.
size_t Engine::ws_budget() {
  if (!ws_budget_) {
    if (pol_.ws_budget_mb > 0) {
      ws_budget_ = (size_t)pol_.ws_budget_mb << 20;
    } else {
      size_t fr = 0, tot = 0;
      PE_HIP(hipMemGetInfo(&fr, &tot));
      ws_budget_ = std::max<size_t>(tot / 3, (size_t)1 << 30);
    }
  }
  return ws_budget_;
}

void Engine::ensure_stage_a(int B, int Tmax) {
  if (!ffn_parts_ && H_ == 192 && FC_ % 48 == 0 && FC_ / 48 <= 16 && !enc_.empty() && enc_[0].f1p) {
    // partial outputs of the fused small-call FFN (kernels/ffn.h): [utterance][slice][192][columns], once
    PE_HIP(hipStreamSynchronize(stream_));
    const size_t fbytes = (size_t)(FC_ / 48) * H_ * LaunchPolicy::ffn_max_cols * sizeof(float);
    PE_HIP(hipMalloc((void**)&ffn_parts_, fbytes));
    if (pol_.debug_poison) poison(ffn_parts_, fbytes);
  }
  const int Ts = rup(Tmax, 128);    // row strides are multiples of 128 columns (conv epilogue relies on it)
  auto carve = [&](char* base, size_t Bc, size_t T) -> size_t {
    Carver c(base);
    // input block: [rng 4 x u64 | seed keys Bc x u64, use flags Bc (padded to 16 bytes) | lengths Bc | speaker ids Bc |
    // scales Bc x 3 (padded to 4) | ids Bc x T] (contiguous, copied as one piece by upload())
    const size_t ns = in_scale_slots(Bc), head = in_head_bytes(Bc);
    d_in_ = c.take<char>(head + (2 * Bc + ns + Bc * T) * sizeof(int));
    d_rng_ = reinterpret_cast<unsigned long long*>(d_in_);
    d_keys_ = reinterpret_cast<unsigned long long*>(d_in_ + 32);
    d_use_ = reinterpret_cast<int*>(d_in_ + 32 + 8 * Bc);
    d_tlens_ = reinterpret_cast<int*>(d_in_ + head);
    d_sids_ = d_tlens_ + Bc;
    d_scales_ = reinterpret_cast<float*>(d_sids_ + Bc);
    d_ids_ = d_sids_ + Bc + ns;
    in_bytes_ = head + (2 * Bc + ns + Bc * T) * sizeof(int);
    d_dur_ = c.take<int>(Bc * T);
    d_cum_ = c.take<int>(Bc * T);
    d_frames_ = c.take<int>(Bc);
    d_framesc_ = c.take<int>(Bc);
    absmax_ = c.take<unsigned>(Bc);
    x_ = c.take<float>(Bc * H_ * T);
    y_ = c.take<float>(Bc * H_ * T);
    qkv_ = c.take<float>(Bc * 3 * H_ * T);
    att_ = c.take<float>(Bc * H_ * T);
    kT_ = c.take<float>(Bc * H_ * T);            // K as [utterance][channel quad][column][4] and
    vQ_ = c.take<float>(Bc * H_ * T);            // V as [utterance][column quad][H][4]: attn4_kernel's operands (kernels/attn4.h)
    ffh_ = c.take<float>(Bc * FC_ * T);
    stats_ = c.take<float>(Bc * 2 * C_ * T);
    xg_ = c.take<float>(Bc * H_ * T);
    dh_ = c.take<float>(Bc * H_ * T);
    dy_ = c.take<float>(Bc * H_ * T);
    dy2_ = c.take<float>(Bc * H_ * T);
    hproj_ = c.take<float>(Bc * 32 * T);
    z2_ = c.take<float>(Bc * 2 * T);
    logw_ = c.take<float>(Bc * T);
    noise_w_ = c.take<float>(Bc * 2 * T);
    cond_ = c.take<float>(Bc * (size_t)std::max(cond_bs_, 1));
    plan_w_ = c.take<float>(Bc * T);               // timing plan (kernels/timing.h): w per id, and the plan block
    d_plan_ = c.take<int>(plan_words(Bc, T));
    // utterances whose attention score slab does not fit LDS: [utterance][head][query block][32][SP] in global memory
    att_s_ = attn_scores_global((int)T) ? c.take<float>(Bc * nh_ * (size_t)rup((int)T, ATT_QB) * (rup((int)T, 64) + 1)) : nullptr;
    return c.off + 256;
  };
  // (growth re-creates every graph: grow the id capacity by at least half, so that texts of slowly increasing length
  // cost a few re-creations, not one per 128 ids)
  size_t nB = std::max<size_t>(B, capA_B_), nT = capA_T_;
  if ((size_t)Ts > capA_T_) nT = std::max<size_t>(Ts, capA_T_ ? rup((int)(capA_T_ + capA_T_ / 2), 128) : 0);
  if (nB != capA_B_ || nT != capA_T_ || !wsA_) {
    const size_t budget = ws_budget();
    if (carve(nullptr, nB, nT) > budget) { nB = B; nT = Ts; }          // exactly this call
    const size_t exact = carve(nullptr, B, Ts);
    if (exact > budget) {
      carve(wsA_, capA_B_, capA_T_);                                      // (the probes above moved the pointers)
      throw std::runtime_error("call too large: " + std::to_string(B) + " utterances padded to " + std::to_string(Ts) +
                               " ids need " + std::to_string(exact >> 20) + " MiB of text-encoder workspace (budget " +
                               std::to_string(budget >> 20) + " MiB)");
    }
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    if (wsA_) { PE_HIP(hipFree(wsA_)); wsA_ = nullptr; }
    if (wsB_) { PE_HIP(hipFree(wsB_)); wsB_ = nullptr; }                  // stage-B pointers sit in the dropped graphs
    capA_B_ = capA_T_ = 0; capB_B_ = capB_F_ = 0;
    void* blk = nullptr;
    size_t bytes = carve(nullptr, nB, nT);
    if (hipMalloc(&blk, bytes) != hipSuccess) {
      (void)hipGetLastError();
      nB = B; nT = Ts; bytes = exact; blk = nullptr;
      if (hipMalloc(&blk, bytes) != hipSuccess) {
        (void)hipGetLastError();
        carve(nullptr, 0, 0);
        throw std::runtime_error("out of device memory: " + std::to_string(bytes >> 20) + " MiB of text-encoder workspace");
      }
    }
    wsA_ = static_cast<char*>(blk); wsA_bytes_ = bytes; capA_B_ = nB; capA_T_ = nT;
    if (pol_.debug_poison) poison(wsA_, bytes);
    carve(wsA_, capA_B_, capA_T_);
    PE_HIP(hipMemsetAsync(d_in_, 0, 32, stream_));        // generator state: "no upload ingested yet" (embed_kernel)
    if (h_in_cap_ < in_bytes_) {
      if (h_in_) PE_HIP(hipHostFree(h_in_));
      h_in_cap_ = in_bytes_;
      PE_HIP(hipHostMalloc((void**)&h_in_, h_in_cap_));
    }
  }
  Ts_ = (int)capA_T_;
  carve(wsA_, capA_B_, capA_T_);
}

void Engine::ensure_stage_b(int Fmax, int batch) {
  const int Fs = rup(Fmax, 128);
  const size_t Bnow = (size_t)std::max(batch > 0 ? batch : B_, 1);      // (warmup sizes for ITS batch, not the last call's)
  auto hmax_of = [&](size_t F) {        // largest [channels x length] activation of the generator
    size_t hm = (size_t)U_ * F, L = F;
    for (auto& st : ups_) { L *= st.rate; hm = std::max(hm, (size_t)st.ch * L); }
    return hm;
  };
  // per-utterance activations are addressed with 32-bit byte offsets (buffer descriptors)
  if (hmax_of(Fs) * sizeof(float) >= (size_t)1 << 31 || (size_t)3 * H_ * Fs * sizeof(float) >= (size_t)1 << 31)
    throw std::runtime_error("utterance too long: a per-utterance activation would exceed 2 GiB");
  auto carve = [&](char* base, size_t Bc, size_t F) -> size_t {
    Carver c(base);
    const size_t hmax = hmax_of(F), S = F * (size_t)hop_;
    zp_ = c.take<float>(Bc * C_ * F);
    fh_ = c.take<float>(Bc * H_ * F);
    facts_ = c.take<float>(Bc * H_ * F);
    fskip_ = c.take<float>(Bc * H_ * F);
    noise_z_ = c.take<float>(Bc * C_ * F);
    for (int i = 0; i < 5; ++i) hb_[i] = c.take<float>(Bc * hmax);
    zwin_ = c.take<float>((size_t)C_ * F);
    zp_keep_ = pol_.debug_keep ? c.take<float>(Bc * C_ * F) : nullptr;
    d_win_ = c.take<int>(4);
    audio_ = c.take<float>(Bc * S);
    pcm_ = c.take<int16_t>(Bc * S);
    return c.off + 256;
  };
  // the batch capacity of this stage follows stage A's while that fits; under memory pressure it is this call's batch
  size_t nB = std::max(capB_B_, std::max(Bnow, capA_B_)), nF = capB_F_;
  if ((size_t)Fs > capB_F_) nF = std::max<size_t>(Fs, capB_F_ ? rup((int)(capB_F_ + capB_F_ / 2), 128) : 0);
  // (a grown frame capacity past the 2 GiB descriptor range falls back to the exact one)
  if (hmax_of(nF) * sizeof(float) >= (size_t)1 << 31 || (size_t)3 * H_ * nF * sizeof(float) >= (size_t)1 << 31) nF = Fs;
  // (after an exact-size fallback under memory pressure capB_B_ is below stage A's capacity: a block that already holds
  // this call stays -- re-entering here would free and re-allocate it, and drop every graph, on each call)
  const bool fits = capB_exact_ && wsB_ && Bnow <= capB_B_ && (size_t)Fs <= capB_F_;
  if (!fits && (nB != capB_B_ || nF != capB_F_ || !wsB_)) {
    const size_t budget = ws_budget();
    capB_exact_ = false;
    if (carve(nullptr, nB, nF) > budget) { nB = Bnow; nF = Fs; capB_exact_ = true; }
    const size_t exact = carve(nullptr, Bnow, Fs);
    if (exact > budget) {
      carve(wsB_, capB_B_, capB_F_);
      throw std::runtime_error("call too large: " + std::to_string(Bnow) + " utterances of up to " + std::to_string(Fs) +
                               " frames need " + std::to_string(exact >> 20) + " MiB of vocoder workspace (budget " +
                               std::to_string(budget >> 20) + " MiB)");
    }
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    if (wsB_) { PE_HIP(hipFree(wsB_)); wsB_ = nullptr; }
    capB_B_ = capB_F_ = 0;
    void* blk = nullptr;
    size_t bytes = carve(nullptr, nB, nF);
    if (hipMalloc(&blk, bytes) != hipSuccess) {
      (void)hipGetLastError();
      nB = Bnow; nF = Fs; bytes = exact; blk = nullptr; capB_exact_ = true;
      if (hipMalloc(&blk, bytes) != hipSuccess) {
        (void)hipGetLastError();
        carve(nullptr, 0, 0);
        throw std::runtime_error("out of device memory: " + std::to_string(bytes >> 20) + " MiB of vocoder workspace");
      }
    }
    wsB_ = static_cast<char*>(blk); wsB_bytes_ = bytes; capB_B_ = nB; capB_F_ = nF;
    if (pol_.debug_poison) poison(wsB_, bytes);
  }
  Fs_ = (int)capB_F_;
  Ss_ = (long)capB_F_ * hop_;
  carve(wsB_, capB_B_, capB_F_);
  const size_t Bc = capB_B_, hmax = hmax_of(capB_F_);
  // zero-copy PCM: room for every utterance of the batch capacity, up to 256 MiB of pinned memory (beyond: copies)
  So_ = rs_on_ ? (long)rup((int)out_samples(Ss_), 4) : Ss_;
  const size_t zc_want = Bc * (size_t)So_;
  if (pol_.pcm_zc && zc_want * sizeof(int16_t) <= ((size_t)256 << 20) && h_pcm_zc_cap_ < zc_want) {
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();                                     // the pointer is a kernel argument inside the graphs
    if (h_pcm_zc_) PE_HIP(hipHostFree(h_pcm_zc_));
    h_pcm_zc_cap_ = zc_want;
    PE_HIP(hipHostMalloc((void**)&h_pcm_zc_, h_pcm_zc_cap_ * sizeof(int16_t)));
  }
  // per-resblock buffers of the grouped sibling schedule (one-utterance calls, first generator stage): allocated
  // here, outside any graph capture; the schedule only applies below 700 64x64 blocks per stage
  const size_t want = std::min<size_t>(Bc * hmax, (size_t)(pol_.group_tiled ? LaunchPolicy::group_tiled_max_blocks : LaunchPolicy::group_max_blocks64) * 4096);
  if ((pol_.group_mrf || pol_.group_tiled) && side_floats_ < want) {
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    for (float*& sp : side_) { if (sp) PE_HIP(hipFree(sp)); sp = nullptr; }
    side_floats_ = 0;                  // (the capacity is published only once EVERY buffer exists: a failed allocation must not
                                       // leave null pointers behind a capacity that says they are there)
    for (float*& sp : side_) {
      if (hipMalloc((void**)&sp, want * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        for (float*& q : side_) { if (q) hipFree(q); q = nullptr; }
        throw std::runtime_error("out of device memory: " + std::to_string((want * sizeof(float) * 9) >> 20) +
                                 " MiB of per-resblock buffers");
      }
      if (pol_.debug_poison) poison(sp, want * sizeof(float));
    }
    side_floats_ = want;
  }
  if (rs_on_) ensure_resample();
  if (ld_on_) ensure_loudness();
}

// ------------------------------------------------------------------------------------------------
// the synthesis call
// ------------------------------------------------------------------------------------------------

void Engine::upload(const int64_t* ids, const int64_t* offsets, int B, const float* scales,
                    const int64_t* sids, const NoiseIn* noise, bool per_utt, const TimingIn* timing, const SeedsIn* seeds) {
  EntryLock entry_lock;
  if (B <= 0 || B > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!scales) throw std::runtime_error("null scales");
  if (seeds && !seeds->seed) throw std::runtime_error("seeds without a seed array (pe_seeds.seed is null)");
  const bool all_forced = timing ? check_timing(*timing, offsets, B) : false;      // (throws before anything changes)
  PE_HIP(hipSetDevice(device_));
  sb_active_ = false;               // new inputs end a batch stream: its latent and its window state go with them
  lg_dev_peaks_ = nullptr;          // (the next resampling launch clears the peak words a default-mode report would read)
  B_ = B;
  id_off_.assign(offsets, offsets + B + 1);
  tlens_h_.resize(B);
  int Tmax = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t T = offsets[b + 1] - offsets[b];
    if (T <= 0) throw std::runtime_error("empty phoneme id sequence");
    if (T > 8192) throw std::runtime_error("phoneme id sequence longer than 8192");
    tlens_h_[b] = (int)T;
    Tmax = std::max(Tmax, (int)T);
  }
  Tmax_ = Tmax;
  // a speculative run whose results were never fetched may still be reading the pinned input block (zero-copy ids)
  if (spec_pending_) { PE_HIP(hipStreamSynchronize(stream_)); spec_pending_ = false; }
  ensure_stage_a(B, Tmax);
  const int Ts = Ts_;
  // the pinned mirror of the input block; a copy of the previous call that might still read it ended with that call's
  // final synchronisation (an abandoned upload is simply overwritten)
  const size_t Bc = capA_B_;
  unsigned long long* hr = reinterpret_cast<unsigned long long*>(h_in_);
  int* htl = reinterpret_cast<int*>(h_in_ + in_head_bytes(Bc));
  int* hsid = htl + Bc;
  float* hsc = reinterpret_cast<float*>(hsid + Bc);
  int* hid = hsid + Bc + in_scale_slots(Bc);
  for (int b = 0; b < B; ++b) {
    int* row = hid + (size_t)b * Ts;
    const int64_t* src = ids + offsets[b];
    const int T = tlens_h_[b];
    for (int t = 0; t < T; ++t) {
      const int64_t id = src[t];
      if (id < 0 || id >= arch_[A_NVOCAB])
        throw std::runtime_error("phoneme id " + std::to_string(id) + " outside [0, num_symbols)");
      row[t] = (int)id;
    }
    memset(row + T, 0, (size_t)(Ts - T) * sizeof(int));
    htl[b] = T;
    hsid[b] = 0;
  }
  if (nspk_ > 1)
    for (int b = 0; b < B; ++b) {
      const int64_t sp = sids ? sids[b] : 0;
      if (sp < 0 || sp >= nspk_) throw std::runtime_error("speaker id outside [0, num_speakers)");
      hsid[b] = (int)sp;
    }
  float ls_max = 0.f;
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < 3; ++k) hsc[(size_t)b * 3 + k] = scales[(per_utt ? (size_t)b * 3 : 0) + k];
    const float ls = hsc[(size_t)b * 3 + 1];
    if (ls > 0.f && std::isfinite(ls)) ls_max = std::max(ls_max, ls);
  }
  // (below half the slowest rate the ceil of every duration keeps the frames from shrinking in proportion: an over-guess
  // stays a hit, an inflated ratio would oversize later calls)
  spec_rel_.resize(B);
  for (int b = 0; b < B; ++b) {
    const float ls = hsc[(size_t)b * 3 + 1];
    spec_rel_[b] = (ls > 0.f && std::isfinite(ls)) ? std::max(0.5f, ls / ls_max) : 1.f;
  }
  // {seed, runs so far, serial of this upload}: the first kernel of every run() advances the counter on the device
  // (embed_kernel). Short calls enqueue no copy at all: embed_kernel reads the pinned block in place and publishes the
  // lengths / speaker ids / generator state to device memory for the kernels behind it (the serial tells it a replay
  // without a new upload from a fresh one).
  hr[0] = seed_; hr[1] = call_; hr[2] = ++upload_serial_; hr[3] = 0;
  // per-utterance seeds: values in the block (an unseeded call's kernels get no table and read none of it)
  seeded_ = seeds != nullptr;
  if (seeded_) {
    unsigned long long* hk = reinterpret_cast<unsigned long long*>(h_in_ + 32);
    int* hu = reinterpret_cast<int*>(h_in_ + 32 + 8 * Bc);
    for (int b = 0; b < B; ++b) {
      hk[b] = (unsigned long long)seeds->seed[b];
      hu[b] = (!seeds->use || seeds->use[b]) ? 1 : 0;
    }
  }
  ids_zc_ = pol_.ids_from_host((long)B * Ts);
  if (!ids_zc_)
    PE_HIP(hipMemcpyAsync(d_in_, h_in_, in_head_bytes(Bc) + (2 * Bc + in_scale_slots(Bc) + (size_t)B * Ts) * sizeof(int),
                          hipMemcpyHostToDevice, stream_));
  plan_on_ = timing != nullptr;
  plan_skip_ = all_forced;
  if (timing) {
    // the plan block through its own pinned staging block (the previous timed call's copy ended with that call's final
    // synchronisation; an abandoned upload is waited for before its block is overwritten or freed)
    const size_t words = plan_words(Bc, (size_t)Ts);
    PE_HIP(hipStreamSynchronize(stream_));
    if (h_plan_cap_ < words) {
      if (h_plan_) { PE_HIP(hipHostFree(h_plan_)); h_plan_ = nullptr; h_plan_cap_ = 0; }
      PE_HIP(hipHostMalloc((void**)&h_plan_, words * sizeof(int)));
      h_plan_cap_ = words;
    }
    for (int b = 0; b < B; ++b) {
      const int T = tlens_h_[b];
      h_plan_[b] = timing->target ? timing->target[b] : 0;
      float* hr_ = reinterpret_cast<float*>(h_plan_ + Bc + (size_t)b * 2 * Ts);
      int* hf = h_plan_ + Bc + (size_t)b * 2 * Ts + Ts;
      for (int t = 0; t < T; ++t) {
        hr_[t] = timing->rate ? timing->rate[offsets[b] + t] : 1.0f;
        hf[t] = timing->forced ? timing->forced[offsets[b] + t] : -1;
      }
    }
    PE_HIP(hipMemcpyAsync(d_plan_, h_plan_, (Bc + (size_t)B * 2 * Ts) * sizeof(int), hipMemcpyHostToDevice, stream_));
  }
  scales_[0] = scales[0]; scales_[1] = scales[1]; scales_[2] = scales[2];
  have_noise_w_ = noise && noise->noise_w;
  have_noise_z_ = noise && noise->noise_z;
  h_noise_z_ = have_noise_z_ ? noise->noise_z : nullptr;
  h_noise_z_stride_ = have_noise_z_ ? noise->z_stride : 0;
  if (have_noise_w_) {      // injected duration noise (parity tests): pageable staging, so wait for the copy
    if (noise->w_stride < Tmax) throw std::runtime_error("noise_w stride shorter than the longest utterance");
    std::vector<float> nb((size_t)B * 2 * Ts, 0.f);
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < 2; ++c)
        memcpy(&nb[((size_t)b * 2 + c) * Ts], noise->noise_w + ((size_t)b * 2 + c) * noise->w_stride,
               tlens_h_[b] * sizeof(float));
    PE_HIP(hipMemcpyAsync(noise_w_, nb.data(), nb.size() * sizeof(float), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  }
}

// hipGraph cache: the kernel sequence of a stage is captured once per shape bucket and replayed;
// one utterance is ~160 short launches, which would otherwise be bound by host launch rate.
void Engine::run_stage(char which, const std::string& key) {
  const long l0 = g_launches;
#ifndef PE_EMU
  if (use_graphs_ && !prof_on_) {
    auto hit = graph_of_.find(key);
    if (hit == graph_of_.end()) {
      hipGraph_t g = nullptr;
      hipGraphExec_t ex = nullptr;
      // exclusive: no other engine of this process is inside a HIP call while this one captures (see g_capture_mu)
      g_capture_mu.unlock_shared();
      g_capture_mu.lock();
      try {
        PE_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
        try {
          dispatch_stage(which);
        } catch (...) {
          hipStreamEndCapture(stream_, &g);
          if (g) hipGraphDestroy(g);
          throw;
        }
        PE_HIP(hipStreamEndCapture(stream_, &g));
        PE_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
        PE_HIP(hipGraphDestroy(g));
      } catch (...) {
        g_capture_mu.unlock();
        g_capture_mu.lock_shared();
        throw;
      }
      g_capture_mu.unlock();
      g_capture_mu.lock_shared();
      ++graph_captures_;
      if (graphs_.size() >= (size_t)pol_.graphs) {          // evict the least recently used graph only
        // (it may still be executing: destroying the exec object of a launched graph is deferred by the runtime until
        // the launch completes; the stream is in order, so nothing of this engine runs concurrently with it anyway)
        PE_HIP(hipStreamSynchronize(stream_));
        hipGraphExecDestroy((hipGraphExec_t)graphs_.front().exec);
        graph_of_.erase(graphs_.front().key);
        graphs_.pop_front();
      }
      graphs_.push_back(GraphEntry{key, (void*)ex, g_launches - l0});
      hit = graph_of_.emplace(key, std::prev(graphs_.end())).first;
    } else if (std::next(hit->second) != graphs_.end()) {
      graphs_.splice(graphs_.end(), graphs_, hit->second);      // most recently used last; iterators stay valid
    }
    PE_HIP(hipGraphLaunch((hipGraphExec_t)hit->second->exec, stream_));
    run_launches_ += hit->second->launches;
    return;
  }
#endif
  (void)key;
  dispatch_stage(which);
  run_launches_ += g_launches - l0;
}

void Engine::dispatch_stage(char which) {
  switch (which) {
    case 'A': issue_stage_a(); break;
    case 'B': issue_stage_b(); break;
    case 'C': issue_stage_a(); issue_stage_b(); break;
    case 'F': issue_flow(); break;
    case 'V': issue_window_rows(batch_rows_); break;
    case 'P': issue_window_rows(pool_rows_); break;
    default: issue_window(); break;
  }
}

void Engine::drop_graphs() {
#ifndef PE_EMU
  for (auto& e : graphs_) hipGraphExecDestroy((hipGraphExec_t)e.exec);
#endif
  graphs_.clear();
  graph_of_.clear();
  lg_dev_peaks_ = nullptr;          // (whoever drops the graphs is about to move the blocks they point into)
}

// Shape buckets (engine.h). Steps of 32 ids up to 512, then 8 per octave; steps of 64 frames up to 1024, then 16 per octave.
int Engine::id_bucket(int T) {
  int g = rup(std::max(T, 1), 32);
  if (g > 512) {
    int step = 64;
    while (step * 16 <= g) step *= 2;             // step = (largest power of two <= g) / 8
    g = rup(T, step);
  }
  return g;
}
int Engine::frame_bucket(int F) {
  int g = rup(std::max(F, 1), 64);
  if (g > 1024) {
    int step = 64;
    while (step * 32 <= g) step *= 2;             // step = (largest power of two <= g) / 16
    g = rup(F, step);
  }
  return g;
}

void Engine::warmup(int max_batch, int max_ids, float frames_per_id, const float* scales_in, const int64_t* sample, int64_t n_sample) {
  EntryLock entry_lock;
  if (max_batch < 1 || max_batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (max_ids < 1 || max_ids > 8192) throw std::runtime_error("phoneme id sequence longer than 8192");
  PE_HIP(hipSetDevice(device_));
  if (!(frames_per_id > 0.f)) frames_per_id = 8.f;
  const long fmax = std::min<long>(MAX_FRAMES, (long)std::ceil((double)frames_per_id * max_ids) + 1);
  ensure_stage_a(max_batch, max_ids);
  ensure_stage_b(frame_bucket((int)fmax), max_batch);
  if (!sample || n_sample < 1) return;
  // the single-utterance graphs of every id bucket up to max_ids: the sample cut / tiled to the bucket length, twice --
  // the first call of a bucket runs as two graphs around the frame-count read-back, the second as the one speculative
  // graph later calls replay (engine.h)
  const float scales[3] = {scales_in ? scales_in[0] : scales_[0], scales_in ? scales_in[1] : scales_[1], scales_in ? scales_in[2] : scales_[2]};
  std::vector<int64_t> ids;
  int prev = 0;
  for (int T = 32; prev < max_ids; T = id_bucket(T + 1)) {
    const int len = std::min(T, max_ids);
    ids.resize(len);
    for (int t = 0; t < len; ++t) ids[t] = sample[t % n_sample];
    const int64_t off[2] = {0, len};
    for (int rep = 0; rep < 2; ++rep) {
      upload(ids.data(), off, 1, scales, nullptr, nullptr);
      run();
      finish_run();
    }
    // ... and the frame buckets next to the one the sample landed in: other texts of this length differ by a few per cent
    // in frames per id (each call below replays or captures the whole-utterance graph for a forced guess; a guess that
    // is too small for the sample costs one re-run of the second half, like any miss -- not counted)
    const int fg = frame_bucket(Fmax_);
    const long runs0 = spec_runs_, miss0 = spec_misses_;
    const float margin0 = spec_margin_;
    const int streak0 = spec_hit_streak_, rm0 = spec_recent_misses_, rr0 = spec_recent_runs_, cd0 = spec_cooldown_;
    for (int d = -1; d <= 1; ++d) {
      spec_fg_force_ = frame_bucket(std::max(1, fg + d * 64));
      upload(ids.data(), off, 1, scales, nullptr, nullptr);
      run();
      finish_run();
    }
    spec_fg_force_ = 0;
    spec_runs_ = runs0; spec_misses_ = miss0; spec_margin_ = margin0;
    spec_hit_streak_ = streak0; spec_recent_misses_ = rm0; spec_recent_runs_ = rr0; spec_cooldown_ = cd0;
    prev = len;
  }
  PE_HIP(hipStreamSynchronize(stream_));
}

void Engine::run() {
  EntryLock entry_lock;
  PE_HIP(hipSetDevice(device_));
  const int B = B_;
  spec_pending_ = false;
  Tg_ = std::min(id_bucket(Tmax_), Ts_);
  run_launches_ = 0;
  // speculative sizing of stage B from the previous run's frames-per-id ratio (see engine.h)
  bool spec = pol_.speculate(B) && last_ratio_ > 0.f && !have_noise_z_ && use_graphs_ && !prof_on_;
  if (plan_on_) spec = false;                 // a timed call: A, read-back, B -- and nothing of the speculation's state moves
  if (spec && spec_cooldown_ > 0) { --spec_cooldown_; spec = false; }
  int fguess = 0;
  if (spec) {
    // ids counted at each utterance's rate relative to the call's slowest (engine.h: spec_rel_): a batch that mixes speaking
    // rates is sized by its slow utterances, not by the longest text at a fast rate; a uniform call counts plain ids
    float units = 0.f;
    for (int b = 0; b < B; ++b) units = std::max(units, spec_rel(b) * (float)tlens_h_[b]);
    fguess = spec_fg_force_ ? spec_fg_force_ : frame_bucket((int)std::ceil(last_ratio_ * spec_margin_ * units) + 1);
    if (fguess > MAX_FRAMES) spec = false;
  }
  if (spec) {
    // before stage A is enqueued: growing the workspace drops every graph. The guess carries a margin and a bucket
    // rounding: when IT does not fit the workspace budget / the 2 GiB descriptor range the real frame count still may, so
    // the call falls back to the two-graph form and only ensure_stage_b on the real counts can fail it
    try {
      ensure_stage_b(fguess);
    } catch (const std::runtime_error& ex) {
      // only the sizing conditions fall back; a HIP error or an allocation failure is the call's error
      const std::string what = ex.what();
      if (what.compare(0, 14, "call too large") != 0 && what.compare(0, 18, "utterance too long") != 0) throw;
      spec = false;
    }
  }
  char key[200];
  if (spec) {
    // the whole utterance -- text encoder to int16 -- as ONE graph: stage B is issued right behind stage A for the
    // guessed frame bucket (the kernels read the real frame counts from device memory, clamped to the bucket)
    Fg_ = std::min(fguess, Fs_);
    // What the cost models see while the graph is issued (window geometry of the stage kernels, column thresholds): the
    // EXPECTED frame counts -- ratio x ids, without the safety margin and the bucket rounding that size the grids. With
    // the bucket capacity here a 417-frame utterance in the 512-frame bucket got the last stage's two-round geometry
    // (mrf_kernel<32,3,1>: 125.6 us per replay) instead of the one-round one its real length takes (<32,4,1>: 85.7 us;
    // profiles/r04_notes.md). Grids and clamps are sized by Fg_; the real counts arrive in finish_run().
    frames_h_.resize(B);
    for (int b = 0; b < B; ++b)
      frames_h_[b] = pol_.spec_expect ? std::min(Fg_, std::max(1, (int)std::ceil(last_ratio_ * (spec_rel(b) * (float)tlens_h_[b])))) : Fg_;
    lens_b_ = d_framesc_;
    // (the target-loudness setting swaps the launches behind the generator: its graphs live side by side with the others)
    snprintf(key, sizeof(key), "C|%d|%d|%d|%d|%d|%d%s%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, Fg_, loud_key(), seed_key());
    fold_dur_ = Tg_ <= REG_MAXT;              // (part of what graph 'C' is: a fixed function of its key)
    try {
      run_stage('C', key);
    } catch (...) {
      fold_dur_ = false;
      throw;
    }
    fold_dur_ = false;
    ++call_;                                  // mirrors the device-side counter bump of this run
    spec_pending_ = true;
    spec_fg_ = Fg_;
    ++spec_runs_;
    return;
  }
  run_stage('A', stage_a_key(B));
  ++call_;                                    // mirrors the device-side counter bump of this run
  PE_HIP(hipStreamSynchronize(stream_));      // the only data-dependent shape: F
  finish_stage_b_sizes();
  ensure_stage_b(frame_bucket(Fmax_));
  Fg_ = std::min(frame_bucket(Fmax_), Fs_);
  lens_b_ = d_frames_;
  if (have_noise_z_) {
    const long l0 = g_launches;
    issue_stage_b();                           // host-injected noise (tests): not graph-captured
    run_launches_ += g_launches - l0;
  } else {
    snprintf(key, sizeof(key), "B|%d|%d|%d|%d%s%s", B, Fg_, Fs_, Ts_, loud_key(), seed_key());
    run_stage('B', key);
  }
}

// The key of stage A's graph. An untimed call's is what it always was; a timed call's carries the plan's two flags -- a
// plan is present, the duration predictor is left out -- and nothing of the plan's values.
std::string Engine::stage_a_key(int B) const {
  char key[200];
  if (plan_on_) snprintf(key, sizeof(key), "A|%d|%d|%d|%d|%d|p%d%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, (int)plan_skip_, seed_key());
  else snprintf(key, sizeof(key), "A|%d|%d|%d|%d|%d%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, seed_key());
  return key;
}

// Host view of the frame counts stage A produced (the stream is synchronised): frames, sample offsets, the ratio the
// next run's guess is made from.
void Engine::finish_stage_b_sizes() {
  const int B = B_;
#ifdef PE_EMU
  if (const char* pf = getenv("EMU_PLAN_FRAMES"))      // emulator plan-only mode (tests/emu): frames are not computed
    for (int b = 0; b < B; ++b) h_frames_[b] = atoi(pf);
#endif
  frames_h_.assign(h_frames_, h_frames_ + B);
  int Fmax = 1;
  float ratio = 0.f;
  for (int b = 0; b < B; ++b) {
    Fmax = std::max(Fmax, frames_h_[b]);
    ratio = std::max(ratio, (float)frames_h_[b] / (spec_rel(b) * (float)tlens_h_[b]));
  }
  if (Fmax > MAX_FRAMES)
    throw std::runtime_error("utterance too long: more than " + std::to_string(MAX_FRAMES) + " spectrogram frames "
                             "(check length_scale)");
  Fmax_ = Fmax;
  // decaying maximum: one long-winded utterance keeps the estimate up for a while, a lasting change of voice / scales
  // is followed within ~50 calls
  // (a timed call's frames per id say nothing about the voice: it leaves the estimate alone)
  if (!plan_on_) last_ratio_ = std::max(ratio, last_ratio_ * 0.98f + ratio * 0.02f);
  sample_off_.assign(B + 1, 0);
  for (int b = 0; b < B; ++b) sample_off_[b + 1] = sample_off_[b] + out_samples((int64_t)frames_h_[b] * hop_);
}

bool Engine::finish_run() {
  EntryLock entry_lock;
  if (!spec_pending_) return true;
  spec_pending_ = false;
  PE_HIP(hipStreamSynchronize(stream_));
  finish_stage_b_sizes();
  if (++spec_recent_runs_ >= 16) { spec_recent_runs_ = 0; spec_recent_misses_ = 0; }
  if (Fmax_ <= spec_fg_) {                     // the guessed bucket covered every utterance: the results stand
    if (++spec_hit_streak_ >= 32) { spec_hit_streak_ = 0; spec_margin_ = std::max(1.10f, spec_margin_ / 1.05f); }
    return true;
  }
  ++spec_misses_;
  spec_hit_streak_ = 0;
  spec_margin_ = std::min(1.5f, spec_margin_ * 1.15f);
  if (++spec_recent_misses_ >= 4) { spec_recent_misses_ = 0; spec_recent_runs_ = 0; spec_cooldown_ = 64; }
  ensure_stage_b(frame_bucket(Fmax_));
  Fg_ = std::min(frame_bucket(Fmax_), Fs_);
  lens_b_ = d_frames_;
  char key[160];
  snprintf(key, sizeof(key), "B|%d|%d|%d|%d%s%s", B_, Fg_, Fs_, Ts_, loud_key(), seed_key());
  run_stage('B', key);
  return false;
}

// A pinned host buffer of at least n elements: grown with half as much again on top, its content not kept.
template <typename T>
static void grow_pinned(T*& p, size_t& cap, size_t n) {
  if (n <= cap) return;
  if (p) { PE_HIP(hipHostFree(p)); p = nullptr; cap = 0; }
  PE_HIP(hipHostMalloc((void**)&p, (n + n / 2) * sizeof(T)));
  cap = n + n / 2;
}

void Engine::download(bool want_audio, bool want_pcm) {
  EntryLock entry_lock;
  auto grow = [&](size_t total) {
    if (want_audio) grow_pinned(h_audio_, h_audio_cap_, total);
    if (want_pcm) grow_pinned(h_pcm_, h_pcm_cap_, total);
  };
  // pcm16_kernel already wrote the samples into pinned host memory (zero-copy), packed back to back: nothing to enqueue
  const bool zc = pol_.pcm_zc && h_pcm_zc_ != nullptr && h_pcm_zc_cap_ >= (size_t)B_ * (size_t)So_;
  // what is delivered: the generator's waveform, or its resampling (row stride So_; Ss_ at the native rate)
  // (read where a copy is enqueued, not here: a missed guess re-sizes the workspace, and the buffers move with it)
  auto asrc = [&]() -> const float* { return rs_on_ ? raudio_ : audio_; };
  auto psrc = [&]() -> const int16_t* { return rs_on_ ? rpcm_ : pcm_; };
  pcm_zc_live_ = false;
  if (spec_pending_ && B_ == 1 && (want_audio || want_pcm)) {
    // one utterance, speculative run: the copies are enqueued for the guessed length (>= the real one when the guess
    // holds) behind stage B, so that one synchronisation ends the whole call; the host view is trimmed afterwards
    const size_t n = (size_t)out_samples((int64_t)spec_fg_ * hop_);
    grow(n);
    if (want_audio) PE_HIP(hipMemcpyAsync(h_audio_, asrc(), n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (want_pcm && !zc) PE_HIP(hipMemcpyAsync(h_pcm_, psrc(), n * sizeof(int16_t), hipMemcpyDeviceToHost, stream_));
    lim_enqueue_report();
    if (finish_run()) {                        // synchronises; sample_off_ now holds the real length
      pcm_zc_live_ = zc;
      loud_collect();
      return;
    }
    // the guess missed: stage B was re-issued (its pcm16_kernel writes the host buffer again); copies below
  } else {
    finish_run();
  }
  const size_t total = (size_t)sample_off_[B_];
  grow(total);
  if (want_audio)
    for (int b = 0; b < B_; ++b)
      PE_HIP(hipMemcpyAsync(h_audio_ + sample_off_[b], asrc() + (size_t)b * So_,
                            (size_t)(sample_off_[b + 1] - sample_off_[b]) * sizeof(float), hipMemcpyDeviceToHost,
                            stream_));
  if (want_pcm && !zc)
    for (int b = 0; b < B_; ++b)
      PE_HIP(hipMemcpyAsync(h_pcm_ + sample_off_[b], psrc() + (size_t)b * So_,
                            (size_t)(sample_off_[b + 1] - sample_off_[b]) * sizeof(int16_t), hipMemcpyDeviceToHost,
                            stream_));
  lim_enqueue_report();
  PE_HIP(hipStreamSynchronize(stream_));
  pcm_zc_live_ = zc;
  loud_collect();
}

int Engine::stream_begin(const int64_t* ids, int64_t n, const float scales[3], int64_t sid, const NoiseIn* noise,
                         const TimingIn* timing, const SeedsIn* seeds) {
  EntryLock entry_lock;
  const int64_t offs[2] = {0, n};
  const int64_t sids[1] = {sid < 0 ? 0 : sid};
  upload(ids, offs, 1, scales, sids, noise, false, timing, seeds);
  PE_HIP(hipSetDevice(device_));
  spec_pending_ = false;
  stream_front(1, 0);
  s_frames_ = Fmax_;
  s_pos_ = 0;
  s_active_ = true;
  s_gain_r_ = std::max(0.01f, gain_peak_);
  s_gain_first_ = true;
  sample_off_.assign(2, 0);
  return s_frames_;
}

bool Engine::stream_next(int chunk_frames, const float** audio, const int16_t** pcm, int64_t* nsamples) {
  EntryLock entry_lock;
  if (!s_active_ || s_pos_ >= s_frames_) {
    if (s_active_) {                                     // nothing delivered: the stored level when running, else zeros
      const bool run = gain_mode_ == GAIN_RUNNING;
      lg_n_ = 1; lg_dev_peaks_ = nullptr; lg_lazy_ = false;
      lg_gain_.assign(1, run ? 32767.0f / s_gain_r_ : 0.f);
      lg_peak_.assign(1, run ? s_gain_r_ : 0.f);
    }
    s_active_ = false;
    if (nsamples) *nsamples = 0;
    return false;
  }
  if (chunk_frames < 1) throw std::runtime_error("chunk_frames must be >= 1");
  PE_HIP(hipSetDevice(device_));
  const int f0 = s_pos_, f1 = std::min(s_frames_, s_pos_ + chunk_frames);
  const int hf = decoder_halo_frames();
  const int a = std::max(0, f0 - hf), b = std::min(s_frames_, f1 + hf);
  const int win[2] = {a, b - a};
  PE_HIP(hipMemcpyAsync(d_win_, win, sizeof(win), hipMemcpyHostToDevice, stream_));
  // at a converted rate the chunk is outputs [ceil(s0 L / M), ceil(s1 L / M)) of the utterance, resampled out of the window
  const int64_t o0 = out_samples((int64_t)f0 * hop_), o1 = out_samples((int64_t)f1 * hop_);
  if (rs_on_) rs_host_row(0, o0, (int64_t)a * hop_, (int)(o1 - o0), (b - a) * hop_);
  s_wg_ = std::min(rup(chunk_frames + 2 * hf, 32), Fs_);
  if (s_wg_ < b - a) s_wg_ = std::min(rup(b - a, 32), Fs_);
  char key[96];
  snprintf(key, sizeof(key), "W|%d|%d", s_wg_, Fs_);
  run_stage('W', key);
  const size_t n = (size_t)(o1 - o0);
  grow_pinned(h_audio_, h_audio_cap_, n);
  PE_HIP(hipMemcpyAsync(h_audio_, rs_on_ ? raudio_ : audio_ + (size_t)(f0 - a) * hop_, n * sizeof(float), hipMemcpyDeviceToHost,
                        stream_));
  PE_HIP(hipStreamSynchronize(stream_));
  // per-chunk peak normalisation, as the reference's streaming script does (infer_onnx_streaming.py:122) -- or one of the
  // stream-wide levels, in the f32 arithmetic of stream_gain_kernel and chunk_pcm_gain_kernel (kernels/post.h)
  float peak = 0.01f;
  for (size_t i = 0; i < n; ++i) peak = std::max(peak, std::fabs(h_audio_[i]));
  float g0 = 32767.0f / peak, sc = g0, level = peak;
  size_t R = 0;
  if (gain_mode_ == GAIN_FIXED) {
    level = std::max(0.01f, gain_peak_);
    g0 = sc = 32767.0f / level;
  } else if (gain_mode_ == GAIN_RUNNING) {
    const float r = s_gain_first_ ? std::max(0.01f, gain_peak_) : s_gain_r_;
    level = std::max(r, peak);                           // (r >= 0.01, so the floor inside `peak` changes nothing)
    sc = 32767.0f / level;
    g0 = s_gain_first_ ? sc : 32767.0f / r;
    R = std::min<size_t>((size_t)gain_ramp_, n);
    s_gain_r_ = level;
    s_gain_first_ = false;
  }
  const float dg = g0 - sc, Rf = (float)std::max<size_t>(R, 1);
  s_pcm_.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const float g = i < R ? std::fmaf(dg, (float)(int)(R - 1 - i) / Rf, sc) : sc;
    float v = h_audio_[i] * g;
    v = std::min(std::max(v, -32768.0f), 32767.0f);
    s_pcm_[i] = (int16_t)v;
  }
  lg_n_ = 1; lg_dev_peaks_ = nullptr; lg_lazy_ = false;
  lg_gain_.assign(1, sc);
  lg_peak_.assign(1, level);
  s_pos_ = f1;
  if (audio) *audio = h_audio_;
  if (pcm) *pcm = s_pcm_.data();
  if (nsamples) *nsamples = (int64_t)n;
  return true;
}

// ------------------------------------------------------------------------------------------------
// batch streaming
// ------------------------------------------------------------------------------------------------

void Engine::rows_free(ChunkRows& r) {
  if (r.host) hipHostFree(r.host);
  if (r.dev) hipFree(r.dev);
  if (r.pcm) hipHostFree(r.pcm);
  if (r.audio) hipHostFree(r.audio);
  gain_blocks_free(&r.gctl, &r.gdev);
  lg_dev_peaks_ = nullptr;                               // (a default-mode report not yet fetched pointed into r.dev)
  r.host = r.dev = nullptr; r.pcm = nullptr; r.audio = nullptr;
  r.cap = 0; r.pcm_cap = r.audio_cap = 0;
}

// The batch stream's blocks, sized by the stage-A batch capacity so that they grow when that does -- which drops every graph
// anyway -- and not from one batch to the next.
void Engine::ensure_stream_batch(int B) {
  ChunkRows& r = batch_rows_;
  const int want = (int)((std::max<size_t>(capA_B_, (size_t)B) + 1) & ~(size_t)1);
  if (r.host && r.dev && r.cap >= want) return;
  PE_HIP(hipStreamSynchronize(stream_));
  drop_graphs();                                       // the blocks' addresses are kernel arguments inside the 'V' graphs
  rows_free(r);                                        // (the gain blocks too: the next chunk outside the default mode allocates them)
  const size_t bytes = (size_t)sb_words(want) * sizeof(int);
  PE_HIP(hipHostMalloc((void**)&r.host, bytes));
  PE_HIP(hipMalloc((void**)&r.dev, bytes));
  memset(r.host, 0, bytes);
  PE_HIP(hipMemset(r.dev, 0, bytes));
  PE_HIP(hipDeviceSynchronize());
  r.cap = want;
}

// Front half of every stream, on the uploaded batch: text encoder and durations, the frame counts read back, the
// length regulator and the flow. The latent is left in zp_.
void Engine::stream_front(int B, int max_frames) {
  Tg_ = std::min(id_bucket(Tmax_), Ts_);
  char key[160];
  run_stage('A', stage_a_key(B));
  ++call_;
  PE_HIP(hipStreamSynchronize(stream_));
  finish_stage_b_sizes();
  if (max_frames > 0)
    for (int b = 0; b < B; ++b)
      if (frames_h_[b] > max_frames)
        throw std::runtime_error("utterance " + std::to_string(b) + " has " + std::to_string(frames_h_[b]) +
                                 " frames, the stream pool holds at most " + std::to_string(max_frames) + " (max_frames)");
  ensure_stage_b(frame_bucket(Fmax_));
  Fg_ = std::min(frame_bucket(Fmax_), Fs_);
  lens_b_ = d_frames_;
  if (have_noise_z_) {
    issue_flow();
  } else {
    snprintf(key, sizeof(key), "F|%d|%d|%d|%d%s", B, Fg_, Fs_, Ts_, seed_key());
    run_stage('F', key);
  }
}

const std::vector<int32_t>& Engine::stream_begin_batch(const int64_t* ids, const int64_t* offsets, int B, const float* scales,
                                                       const int64_t* sids, const NoiseIn* noise, const TimingIn* timing,
                                                       const SeedsIn* seeds) {
  EntryLock entry_lock;
  upload(ids, offsets, B, scales, sids, noise, true, timing, seeds);
  PE_HIP(hipSetDevice(device_));
  spec_pending_ = false;
  s_active_ = false;                                   // (a one-utterance stream on this handle loses its latent too)
  ensure_stream_batch(B);
  stream_front(B, 0);
  batch_rows_.pos.assign(B, 0);
  batch_rows_.gfirst.assign(B, 1);
  batch_rows_.off.assign(B + 1, 0);
  sample_off_.assign(B + 1, 0);
  sb_active_ = true;
  return frames_h_;
}

void Engine::stream_next_batch(int chunk_frames, bool want_audio, StreamChunk& out) {
  EntryLock entry_lock;
  if (!sb_active_) throw std::runtime_error("no batch stream begun on this handle (pe_stream_begin_batch)");
  if (chunk_frames < 1) throw std::runtime_error("chunk_frames must be >= 1");
  PE_HIP(hipSetDevice(device_));
  ChunkRows& r = batch_rows_;
  r.src = zp_; r.src_bs = (long)C_ * Fs_; r.src_cs = Fs_;      // (where the front half left the latent; conditioning: cond_)
  rows_next(r, frames_h_.data(), nullptr, chunk_frames, nullptr, Fmax_, want_audio, out);
}

// One chunk of a row set. The previous chunk ended with a synchronisation: nothing on the device reads the pinned blocks
// any more. A row with nothing to deliver -- finished, or not live -- gets the one-frame window [0, 1) of its own latent and
// no delivery range.
bool Engine::rows_next(ChunkRows& r, const int32_t* frames, const int32_t* live, int chunk, const int32_t* per_row, int clamp,
                       bool want_audio, StreamChunk& out) {
  const int n = (int)r.pos.size(), cap = r.cap, hf = decoder_halo_frames();
  int* st = r.host;
  long long* off = reinterpret_cast<long long*>(st + sb_o_off(cap));
  int wmax = 1, cmax = 1;
  int64_t total = 0;
  for (int b = 0; b < n; ++b) {
    const int F = frames[b], f0 = r.pos[b];
    const int c = std::min(per_row && per_row[b] > 0 ? per_row[b] : chunk, clamp);
    int a = 0, e = 1, first = 0, count = 0;
    int64_t ocount = 0;
    if ((!live || live[b]) && f0 < F) {
      const int f1 = std::min(F, f0 + c);
      a = std::max(0, f0 - hf);
      e = std::min(F, f1 + hf);
      first = (f0 - a) * hop_;
      count = (f1 - f0) * hop_;
      ocount = out_samples((int64_t)f1 * hop_) - out_samples((int64_t)f0 * hop_);
      cmax = std::max(cmax, c);
    }
    st[b] = a;
    st[sb_o_len(cap) + b] = e - a;
    st[sb_o_first(cap) + b] = first;
    st[sb_o_count(cap) + b] = count;
    // (converted rate: the row of the resampling launch. The row block exists once the workspaces are sized, which the pool
    // sees to before it comes here.)
    if (rs_on_) rs_host_row(b, out_samples((int64_t)f0 * hop_), (int64_t)a * hop_, (int)ocount, (e - a) * hop_);
    off[b] = (long long)total;
    r.off[b] = total;
    total += ocount;
    wmax = std::max(wmax, e - a);
  }
  r.off[n] = total;
  out.batch = n;
  out.sample_offsets = r.off.data();
  out.frames_done = r.pos.data();
  out.pcm = r.pcm;
  out.audio = nullptr;
  if (total == 0) {                                    // no row has frames left
    gain_report_idle(r.gctl, cap, n);
    return false;
  }
  grow_pinned(r.pcm, r.pcm_cap, (size_t)total);
  if (want_audio) grow_pinned(r.audio, r.audio_cap, (size_t)total);
  void* ptrs[2] = {r.pcm, want_audio ? r.audio : nullptr};
  memcpy(st + sb_o_ptrs(cap), ptrs, sizeof(ptrs));
  // the window bucket: by the largest step among the rows that deliver
  r.wg = std::min(rup(cmax + 2 * hf, 32), Fs_);
  if (r.wg < wmax) r.wg = std::min(rup(wmax, 32), Fs_);
  char key[96];
  if (gain_mode_ == GAIN_CHUNK) {
    snprintf(key, sizeof(key), "%c|%d|%d|%d", r.stage, n, r.wg, Fs_);
  } else {
    if (!r.gctl) gain_blocks_alloc(cap, &r.gctl, &r.gdev);      // (the batch stream's: the pool's exist since open)
    if ((int)r.gfirst.size() < n) r.gfirst.assign(n, 1);
    gain_prepare(r.gctl, cap, r.gfirst, n);
    snprintf(key, sizeof(key), "%c|%d|%d|%d|g%d", r.stage, n, r.wg, Fs_, gain_mode_);
  }
  run_stage(r.stage, key);
  PE_HIP(hipStreamSynchronize(stream_));
  gain_collect(r.gctl, cap, n, r.gfirst, r.off.data(),
               rs_on_ ? rs_peaks() : reinterpret_cast<const unsigned*>(r.dev) + sb_o_peak(cap));
  for (int b = 0; b < n; ++b) r.pos[b] += st[sb_o_count(cap) + b] / hop_;
  out.pcm = r.pcm;
  out.audio = want_audio ? r.audio : nullptr;
  return true;
}

// ------------------------------------------------------------------------------------------------
// stream pool
// ------------------------------------------------------------------------------------------------

void Engine::stream_pool_require() const {
  if (!sp_slots_) throw std::runtime_error("no stream pool open on this handle (pe_stream_pool_open)");
}

void Engine::stream_pool_free() {
  if (sp_z_) hipFree(sp_z_);
  if (sp_cond_) hipFree(sp_cond_);
  if (sp_join_) hipHostFree(sp_join_);
  rows_free(pool_rows_);
  sp_z_ = sp_cond_ = nullptr; sp_join_ = nullptr;
  sp_slots_ = sp_fcap_ = sp_maxf_ = 0;
}

int Engine::stream_pool_open(int slots, int max_frames) {
  EntryLock entry_lock;
  if (sp_slots_) throw std::runtime_error("a stream pool is already open on this handle (pe_stream_pool_close)");
  if (slots < 1 || slots > 4096) throw std::runtime_error("stream pool slots must be in [1, 4096]");
  if (max_frames < 1 || max_frames > MAX_FRAMES)
    throw std::runtime_error("stream pool max_frames must be in [1, " + std::to_string(MAX_FRAMES) + "]");
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const int fcap = rup(max_frames, 64), cap = (slots + 1) & ~1;
  // both workspaces for `slots` utterances, stage B for windows up to a whole row: once, here, so that a steady server's
  // joins and chunks never grow them (growth drops every graph)
  ensure_stage_a(slots, 1);
  ensure_stage_b(fcap, slots);
  PE_HIP(hipStreamSynchronize(stream_));
  const size_t zbytes = (size_t)slots * C_ * fcap * sizeof(float);
  const size_t cbytes = (size_t)slots * std::max(cond_dec_.rows, 1) * sizeof(float);
  const size_t sbytes = (size_t)sb_words(cap) * sizeof(int), jbytes = (size_t)sj_words(cap) * sizeof(int);
  ChunkRows& r = pool_rows_;
  try {
    if (hipMalloc((void**)&sp_z_, zbytes) != hipSuccess) {
      (void)hipGetLastError();
      sp_z_ = nullptr;
      throw std::runtime_error("out of device memory: " + std::to_string(zbytes >> 20) + " MiB of stream pool latents");
    }
    PE_HIP(hipMalloc((void**)&sp_cond_, cbytes));
    PE_HIP(hipMalloc((void**)&r.dev, sbytes));
    PE_HIP(hipHostMalloc((void**)&r.host, sbytes));
    PE_HIP(hipHostMalloc((void**)&sp_join_, jbytes));
    PE_HIP(hipMemset(sp_z_, 0, zbytes));
    PE_HIP(hipMemset(sp_cond_, 0, cbytes));
    PE_HIP(hipMemset(r.dev, 0, sbytes));
    memset(r.host, 0, sbytes);
    memset(sp_join_, 0, jbytes);
    gain_blocks_alloc(cap, &r.gctl, &r.gdev);
    PE_HIP(hipDeviceSynchronize());
  } catch (...) {
    stream_pool_free();
    throw;
  }
  sp_slots_ = slots; sp_fcap_ = fcap; sp_maxf_ = max_frames;
  sp_frames_.assign(slots, 0);
  sp_live_.assign(slots, 0);
  r.cap = cap;
  r.pos.assign(slots, 0);
  r.gfirst.assign(slots, 1);
  r.off.assign(slots + 1, 0);
  r.src = sp_z_; r.src_bs = (long)C_ * fcap; r.src_cs = fcap;
  r.cond = sp_cond_; r.cond_bs = cond_dec_.rows;
  return decoder_halo_frames();
}

void Engine::stream_pool_close() {
  EntryLock entry_lock;
  stream_pool_require();
  PE_HIP(hipSetDevice(device_));
  PE_HIP(hipStreamSynchronize(stream_));
#ifndef PE_EMU
  for (auto it = graphs_.begin(); it != graphs_.end();)      // the pool's addresses are kernel arguments inside the 'P' graphs
    if (it->key.compare(0, 2, "P|") == 0) {
      hipGraphExecDestroy((hipGraphExec_t)it->exec);
      graph_of_.erase(it->key);
      it = graphs_.erase(it);
    } else {
      ++it;
    }
#endif
  stream_pool_free();
}

int Engine::stream_pool_state(int32_t* frames, int32_t* frames_done, int32_t* live) const {
  for (int s = 0; s < sp_slots_; ++s) {
    if (frames) frames[s] = sp_frames_[s];
    if (frames_done) frames_done[s] = pool_rows_.pos[s];
    if (live) live[s] = sp_live_[s];
  }
  return sp_slots_;
}

void Engine::stream_pool_leave(int slot) {
  EntryLock entry_lock;
  stream_pool_require();
  if (slot < 0 || slot >= sp_slots_) throw std::runtime_error("stream pool slot outside [0, slots)");
  if (!sp_live_[slot]) throw std::runtime_error("stream pool slot " + std::to_string(slot) + " is free");
  sp_live_[slot] = 0;
}

void Engine::stream_pool_join(const int64_t* ids, const int64_t* offsets, int n, const float* scales, const int64_t* sids,
                              const NoiseIn* noise, int32_t* slot_of, int32_t* total_frames, const TimingIn* timing,
                              const SeedsIn* seeds) {
  EntryLock entry_lock;
  stream_pool_require();
  if (seeds && !seeds->seed) throw std::runtime_error("seeds without a seed array (pe_seeds.seed is null)");
  if (n < 1) throw std::runtime_error("batch size must be in [1, 4096]");
  std::vector<int> take;
  for (int s = 0; s < sp_slots_ && (int)take.size() < n; ++s)
    if (!sp_live_[s]) take.push_back(s);
  if ((int)take.size() < n) {
    int nfree = 0;
    for (int s = 0; s < sp_slots_; ++s) nfree += sp_live_[s] ? 0 : 1;
    throw std::runtime_error("stream pool has " + std::to_string(nfree) + " free slots, " + std::to_string(n) +
                             " utterances want to join");
  }
  // from here to the adopt launch nothing of the pool is touched: whatever fails, the pool is as it was
  if (timing) check_timing(*timing, offsets, n);       // (before the pool's own check below, which reads the targets)
  if (timing && timing->target)
    for (int j = 0; j < n; ++j)
      if (timing->target[j] > sp_maxf_)
        throw std::runtime_error("utterance " + std::to_string(j) + " has a target of " + std::to_string(timing->target[j]) +
                                 " frames, the stream pool holds at most " + std::to_string(sp_maxf_) + " (max_frames)");
  upload(ids, offsets, n, scales, sids, noise, true, timing, seeds);
  PE_HIP(hipSetDevice(device_));
  spec_pending_ = false;
  s_active_ = false;                                   // (a one-utterance stream on this handle loses its latent)
  stream_front(n, sp_maxf_);
  // the previous join ended with a synchronisation: nothing on the device reads the pinned join block any more
  const int cap = pool_rows_.cap;
  sp_join_[0] = n;
  for (int j = 0; j < n; ++j) {
    sp_join_[sj_o_slot(cap) + j] = take[j];
    sp_join_[sj_o_frames(cap) + j] = frames_h_[j];
  }
  const float* cond = nspk_ > 1 ? cond_ + cond_off_dec_ : nullptr;
  PE_LAUNCH_KB("stream_adopt_kernel", 4.0 * n * C_ * ((double)Fg_ + sp_fcap_),
               launch::stream_adopt(dim3((Fg_ + 63) / 64, C_, n), stream_, zp_, (long)C_ * Fs_, Fs_, cond, cond_bs_,
                                    cond ? cond_dec_.rows : 0, sp_join_, cap, sp_z_, (long)C_ * sp_fcap_, sp_fcap_, sp_cond_,
                                    sp_slots_));
  PE_HIP(hipStreamSynchronize(stream_));
  for (int j = 0; j < n; ++j) {
    const int s = take[j];
    sp_frames_[s] = frames_h_[j];
    pool_rows_.pos[s] = 0;
    sp_live_[s] = 1;
    pool_rows_.gfirst[s] = 1;                            // its first chunk resets the slot's level: nothing of the last tenant's stays
    if (slot_of) slot_of[j] = s;
    if (total_frames) total_frames[j] = frames_h_[j];
  }
}

void Engine::stream_pool_next(int chunk_frames, const int32_t* per_slot, bool want_audio, StreamChunk& out) {
  EntryLock entry_lock;
  stream_pool_require();
  if (chunk_frames < 1) throw std::runtime_error("chunk_frames must be >= 1");
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles its sizes first)
  const int S = sp_slots_;
  ChunkRows& r = pool_rows_;
  bool any = false;
  for (int s = 0; s < S; ++s) any = any || (sp_live_[s] && r.pos[s] < sp_frames_[s]);
  if (any) {
    // the workspaces as open sized them, should another call have shrunk them since (an exact-size fallback under memory
    // pressure): a no-op otherwise. Before the rows are written: the resampler's row block exists only then. (A call with
    // nothing to deliver leaves the workspaces alone.)
    if (capA_B_ < (size_t)S) ensure_stage_a(S, 1);
    ensure_stage_b(sp_fcap_, S);
  }
  if (!rows_next(r, sp_frames_.data(), sp_live_.data(), chunk_frames, per_slot, sp_fcap_, want_audio, out)) return;
  for (int s = 0; s < S; ++s)
    if (sp_live_[s] && r.pos[s] >= sp_frames_[s]) sp_live_[s] = 0;      // free from the next call on
}

// ------------------------------------------------------------------------------------------------
// stream-wide gain
// ------------------------------------------------------------------------------------------------

void Engine::set_stream_gain(int mode, float peak, int ramp_samples) {
  EntryLock entry_lock;
  if (mode != GAIN_CHUNK && mode != GAIN_RUNNING && mode != GAIN_FIXED)
    throw std::runtime_error("unknown stream gain mode " + std::to_string(mode) + " (0 chunk, 1 running, 2 fixed)");
  if (!std::isfinite(peak)) throw std::runtime_error("stream gain peak is not finite");
  if (peak < 0.f) throw std::runtime_error("stream gain peak must not be negative");
  if (mode == GAIN_FIXED && !(peak > 0.f)) throw std::runtime_error("a fixed stream gain needs a peak > 0");
  if (ramp_samples < 0 || ramp_samples > GAIN_MAX_RAMP)
    throw std::runtime_error("stream gain ramp_samples outside [0, " + std::to_string(GAIN_MAX_RAMP) + "]");
  bool live = s_active_ && s_pos_ < s_frames_;
  if (sb_active_)
    for (int b = 0; b < B_ && b < (int)batch_rows_.pos.size(); ++b) live = live || batch_rows_.pos[b] < frames_h_[b];
  bool pool = false;
  for (int s = 0; s < sp_slots_; ++s) pool = pool || sp_live_[s] != 0;
  if (live || pool)
    throw std::runtime_error(std::string("the stream gain cannot change while a ") +
                             (pool ? "stream pool slot is occupied" : "stream is live") + " on this handle");
  // peak and ramp are data the kernels read from the control block; the mode picks the launches and is part of the window
  // stages' graph keys, so nothing is dropped here: every mode's graphs stay cached side by side
  gain_mode_ = mode; gain_peak_ = peak; gain_ramp_ = ramp_samples;
}

int Engine::stream_last_gains(float* gain, float* peak, int64_t capacity) {
  EntryLock entry_lock;
  if (lg_n_ < 0) throw std::runtime_error("no stream chunk delivered on this handle yet");
  if ((gain || peak) && capacity < lg_n_) throw std::runtime_error("stream gains buffer too small");
  if (lg_lazy_) {                                        // default mode, batch stream or pool: the peaks stayed on the device
    if (!lg_dev_peaks_)
      throw std::runtime_error("the last chunk's peaks are no longer on the device (another call ran since): ask right after the chunk");
    PE_HIP(hipSetDevice(device_));
    std::vector<unsigned> w((size_t)lg_n_);
    PE_HIP(hipMemcpy(w.data(), lg_dev_peaks_, w.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int b = 0; b < lg_n_; ++b) {
      float c;
      memcpy(&c, &w[b], sizeof(float));
      const float level = std::max(0.01f, c);
      lg_peak_[b] = lg_got_[b] ? level : 0.f;
      lg_gain_[b] = lg_got_[b] ? 32767.0f / level : 0.f;
    }
    lg_dev_peaks_ = nullptr;
    lg_lazy_ = false;
  }
  for (int b = 0; b < lg_n_; ++b) {
    if (gain) gain[b] = lg_gain_[b];
    if (peak) peak[b] = lg_peak_[b];
  }
  return lg_n_;
}

void Engine::gain_blocks_alloc(int cap, int** ctl, int** dev) {
  const size_t cbytes = (size_t)sg_words(cap) * sizeof(int), dbytes = (size_t)sgd_words(cap) * sizeof(int);
  PE_HIP(hipHostMalloc((void**)ctl, cbytes));
  memset(*ctl, 0, cbytes);
  PE_HIP(hipMalloc((void**)dev, dbytes));
  PE_HIP(hipMemset(*dev, 0, dbytes));
  PE_HIP(hipDeviceSynchronize());
}

void Engine::gain_blocks_free(int** ctl, int** dev) {
  if (*ctl) hipHostFree(*ctl);
  if (*dev) hipFree(*dev);
  *ctl = *dev = nullptr;
}

// The previous chunk ended with a synchronisation: nothing on the device reads or writes the control block any more.
void Engine::gain_prepare(int* ctl, int cap, const std::vector<char>& first, int n) {
  memcpy(ctl, &gain_peak_, sizeof(float));
  ctl[1] = gain_ramp_;
  for (int b = 0; b < n && b < cap; ++b) ctl[sg_o_first(cap) + b] = first[b] ? 1 : 0;
}

void Engine::gain_collect(const int* ctl, int cap, int n, std::vector<char>& first, const int64_t* off, const unsigned* peaks) {
  lg_n_ = n;
  lg_got_.resize(n);
  for (int b = 0; b < n; ++b) lg_got_[b] = off[b + 1] > off[b];
  if (gain_mode_ == GAIN_CHUNK) {
    lg_gain_.assign(n, 0.f);
    lg_peak_.assign(n, 0.f);
    lg_dev_peaks_ = peaks;
    lg_lazy_ = true;
    return;
  }
  lg_dev_peaks_ = nullptr;
  lg_lazy_ = false;
  const float* cf = reinterpret_cast<const float*>(ctl);
  lg_gain_.assign(cf + sg_o_rgain(cap), cf + sg_o_rgain(cap) + n);
  lg_peak_.assign(cf + sg_o_rpeak(cap), cf + sg_o_rpeak(cap) + n);
  for (int b = 0; b < n; ++b)
    if (lg_got_[b]) first[b] = 0;
}

void Engine::gain_report_idle(const int* ctl, int cap, int n) {
  lg_n_ = n;
  lg_dev_peaks_ = nullptr;
  lg_lazy_ = false;
  lg_got_.assign(n, 0);
  lg_gain_.assign(n, 0.f);
  lg_peak_.assign(n, 0.f);
  if (gain_mode_ != GAIN_RUNNING || !ctl) return;
  // running: the report words still hold every row's stored state (the chunk that delivered a row's last samples wrote
  // its final level; a row that delivered nothing since wrote its stored one)
  const float* cf = reinterpret_cast<const float*>(ctl);
  for (int b = 0; b < n && b < cap; ++b) { lg_gain_[b] = cf[sg_o_rgain(cap) + b]; lg_peak_[b] = cf[sg_o_rpeak(cap) + b]; }
}

// ------------------------------------------------------------------------------------------------
// output-rate conversion
// ------------------------------------------------------------------------------------------------

void Engine::rs_free() {
  if (rs_coef_) hipFree(rs_coef_);
  if (raudio_) hipFree(raudio_);
  if (rpcm_) hipFree(rpcm_);
  if (rs_dev_) hipFree(rs_dev_);
  if (rs_host_) hipHostFree(rs_host_);
  rs_coef_ = raudio_ = nullptr; rpcm_ = nullptr; rs_dev_ = rs_host_ = nullptr;
  rs_buf_elems_ = 0; rs_cap_ = 0;
}

// modified Bessel function of the first kind, order 0 (power series; x <= 8.6 here: ~30 terms to 1e-17 relative)
static double bessel_i0(double x) {
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// The interpolation filter of the rate pair native -> output, shared by the resampler and the true-peak
// measure: L = output / gcd, M = native / gcd, the half-width K in native samples, Tp = 2 K rounded up to 4 taps per phase.
// table != null: the L x Tp polyphase table in f64, entry [ph][k] the Kaiser-windowed sinc (cutoff 0.46 of the lower rate,
// Z = 16 zero crossings a side, beta = 8.6) at (ph + (K - 1 - k) L) / (L native) seconds; entries past the window's
// support, the padding up to Tp included, are exact zeros. The device tables are these values rounded once to f32.
void Engine::resample_filter(int native, int output, int& L, int& M, int& K, int& Tp, std::vector<double>* table) {
  const int g = std::gcd(native, output);
  L = output / g; M = native / g;
  const double fmin = std::min(native, output), fc = 0.92 * fmin / 2.0, Z = 16.0, beta = 8.6, Th = Z / (2.0 * fc);
  K = (int)std::ceil(Z * (double)native / (0.92 * fmin) - 1e-9);
  Tp = rup(2 * K, 4);
  if (!table) return;
  table->assign((size_t)L * Tp, 0.0);
  const double i0b = bessel_i0(beta), pi = 3.14159265358979323846;
  for (int ph = 0; ph < L; ++ph)
    for (int k = 0; k < 2 * K; ++k) {
      const double t = ((double)ph + (double)(K - 1 - k) * (double)L) / ((double)L * (double)native);
      const double u = t / Th;
      if (std::fabs(u) > 1.0) continue;
      const double x = 2.0 * fc * t;
      const double sinc = std::fabs(x) < 1e-12 ? 1.0 : std::sin(pi * x) / (pi * x);
      (*table)[(size_t)ph * Tp + k] = (2.0 * fc / (double)native) * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
    }
}

void Engine::set_output_rate(int native, int output) {
  EntryLock entry_lock;
  const int header = arch_[A_SR];
  if (native < 0 || output < 0) throw std::runtime_error("sample rates must not be negative");
  if (native == 0) {
    if (header <= 0 && rs_native_ <= 0)
      throw std::runtime_error("native_rate 0 means the voice header's sample rate, and this voice carries none (an .onnx "
                               "does not): pass the sample rate of its .onnx.json");
    native = header > 0 ? header : rs_native_;
  } else if (header > 0 && native != header) {
    throw std::runtime_error("native_rate " + std::to_string(native) + " contradicts the voice header's sample rate " +
                             std::to_string(header));
  }
  bool live = s_active_ && s_pos_ < s_frames_;
  if (sb_active_)
    for (int b = 0; b < B_ && b < (int)batch_rows_.pos.size(); ++b) live = live || batch_rows_.pos[b] < frames_h_[b];
  if (live || sp_slots_)
    throw std::runtime_error(std::string("the output rate cannot change while a ") +
                             (sp_slots_ ? "stream pool is open" : "stream is live") + " on this handle");
  const bool on = output != 0 && output != native;
  if (ld_on_) loud_check_rate(on ? output : native);    // (the target loudness is measured at the delivered rate)
  if (ld_on_ && ld_kind_ == PEAK_TRUE) tp_check_rate(on ? output : native);
  if (ld_on_ && lim_on_ && limiter_window_samples(on ? output : native, (double)lim_ms_) > LIM_MAXW)
    throw std::runtime_error("limiter window " + std::to_string(lim_ms_) + " ms is more than " + std::to_string(LIM_MAXW) +
                             " samples at " + std::to_string(on ? output : native) + " Hz");
  const std::string pair = std::to_string(native) + " -> " + std::to_string(output) + " Hz";
  int L = 1, M = 1, K = 0, Tp = 0, tile = RS_TILE;
  std::vector<float> table;
  if (on) {
    if (output < 8000 || output > 48000)
      throw std::runtime_error("output rate outside [8000, 48000]: " + pair);
    resample_filter(native, output, L, M, K, Tp, nullptr);
    if (L > 640)
      throw std::runtime_error("rate pair " + pair + " needs a table of " + std::to_string(L) + " phases (output / gcd), more than 640");
    if (K > hop_)
      throw std::runtime_error("rate pair " + pair + " needs a filter half-width of " + std::to_string(K) +
                               " native samples, more than the voice's hop size " + std::to_string(hop_));
    // output samples per workgroup: as many as keep the native span (tile * M / L + Tp + alignment slack) inside the LDS array
    const long room = (long)(RS_SPAN - Tp - 6) * L / M;
    tile = (int)std::min<long>(RS_TILE, room / 64 * 64);
    if (tile < 64) throw std::runtime_error("rate pair " + pair + ": the native span of 64 outputs exceeds the staging buffer");
    std::vector<double> exact;
    resample_filter(native, output, L, M, K, Tp, &exact);
    table.resize(exact.size());
    for (size_t i = 0; i < exact.size(); ++i) table[i] = (float)exact[i];
  }
  if (on == rs_on_ && (!on || (native == rs_native_ && output == rs_out_))) {      // nothing changes (the native rate is noted)
    rs_native_ = native;
    if (ld_on_ && output_rate() != ld_fs_) {           // (a voice without a header rate was told another native rate)
      PE_HIP(hipSetDevice(device_));
      finish_run();
      PE_HIP(hipStreamSynchronize(stream_));
      drop_graphs();
      loud_upload_filter(output_rate());
    }
    return;
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  PE_HIP(hipStreamSynchronize(stream_));
  float* coef = nullptr;
  if (on) {
    PE_HIP(hipMalloc((void**)&coef, table.size() * sizeof(float)));
    if (hipMemcpy(coef, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      hipFree(coef);
      throw std::runtime_error("upload of the resampling table failed");
    }
  }
  // from here on nothing throws before the new setting is complete
  drop_graphs();                                       // the stage sequences and their buffer addresses depend on the rate
  if (rs_coef_) hipFree(rs_coef_);
  rs_coef_ = coef;
  rs_on_ = on; rs_native_ = native; rs_out_ = on ? output : 0;
  rs_L_ = L; rs_M_ = M; rs_K_ = K; rs_Tp_ = Tp; rs_tile_ = tile;
  s_active_ = false; sb_active_ = false;               // (finished streams end here: their windows were sized for the old rate)
  pcm_zc_live_ = false;
  if (!on) {                                           // back to the native engine: its buffers and strides
    if (raudio_) hipFree(raudio_);
    if (rpcm_) hipFree(rpcm_);
    raudio_ = nullptr; rpcm_ = nullptr; rs_buf_elems_ = 0;
    So_ = Ss_;
  }
  // (on: the next call's ensure_stage_b derives So_ and sizes the zero-copy PCM buffer and the resampled rows)
  if (ld_on_) loud_upload_filter(output_rate());       // the K-weighting filter of the new delivered rate
}

// The resampled rows [capB_B_][So_] (floats + int16) and the two row blocks, (re)allocated when the workspace capacity or
// the rate changed; called at the end of ensure_stage_b, which has set So_.
void Engine::ensure_resample() {
  const size_t need = capB_B_ * (size_t)So_;
  const int want_cap = (int)((std::max<size_t>(std::max(capA_B_, capB_B_), 64) + 1) & ~(size_t)1);
  if (raudio_ && rpcm_ && rs_buf_elems_ >= need && rs_host_ && rs_dev_ && rs_cap_ >= want_cap) return;
  PE_HIP(hipStreamSynchronize(stream_));
  drop_graphs();
  if (!(raudio_ && rpcm_ && rs_buf_elems_ >= need)) {
    if (raudio_) { PE_HIP(hipFree(raudio_)); raudio_ = nullptr; }
    if (rpcm_) { PE_HIP(hipFree(rpcm_)); rpcm_ = nullptr; }
    rs_buf_elems_ = 0;
    if (hipMalloc((void**)&raudio_, need * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&rpcm_, need * sizeof(int16_t)) != hipSuccess) {
      (void)hipGetLastError();
      if (raudio_) hipFree(raudio_);
      raudio_ = nullptr; rpcm_ = nullptr;
      throw std::runtime_error("out of device memory: " + std::to_string((need * 6) >> 20) + " MiB of resampled output");
    }
    rs_buf_elems_ = need;
    if (pol_.debug_poison) { poison(raudio_, need * sizeof(float)); poison(rpcm_, need * sizeof(int16_t)); }
  }
  if (!(rs_host_ && rs_dev_ && rs_cap_ >= want_cap)) {
    if (rs_host_) { PE_HIP(hipHostFree(rs_host_)); rs_host_ = nullptr; }
    if (rs_dev_) { PE_HIP(hipFree(rs_dev_)); rs_dev_ = nullptr; }
    rs_cap_ = 0;
    const size_t bytes = (size_t)rs_words(want_cap) * sizeof(int);
    PE_HIP(hipHostMalloc((void**)&rs_host_, bytes));
    PE_HIP(hipMalloc((void**)&rs_dev_, bytes));
    memset(rs_host_, 0, bytes);
    PE_HIP(hipMemset(rs_dev_, 0, bytes));
    PE_HIP(hipDeviceSynchronize());
    rs_cap_ = want_cap;
  }
}

void Engine::rs_host_row(int b, int64_t n0, int64_t org, int count, int vlen) {
  if (!rs_host_ || b < 0 || b >= rs_cap_) return;
  reinterpret_cast<long long*>(rs_host_)[b] = n0;
  reinterpret_cast<long long*>(rs_host_ + rs_o_org(rs_cap_))[b] = org;
  rs_host_[rs_o_count(rs_cap_) + b] = count;
  rs_host_[rs_o_vlen(rs_cap_) + b] = vlen;
}

void Engine::debug_resample(const float* x, int batch, int64_t stride, const int32_t* vlen, const int64_t* n0,
                            const int32_t* count, const int64_t* origin, float* out, int64_t out_stride) {
  EntryLock entry_lock;
  if (!rs_on_) throw std::runtime_error("no output rate set (pe_set_output_rate)");
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !vlen || !n0 || !count || !origin || !out) throw std::runtime_error("null argument");
  int maxc = 0;
  for (int b = 0; b < batch; ++b) {
    if (vlen[b] < 0 || vlen[b] > stride) throw std::runtime_error("row " + std::to_string(b) + ": valid length outside [0, stride]");
    if (count[b] < 0 || count[b] > out_stride) throw std::runtime_error("row " + std::to_string(b) + ": output count outside [0, out_stride]");
    if (n0[b] < 0 || n0[b] > ((int64_t)1 << 40)) throw std::runtime_error("row " + std::to_string(b) + ": first output index out of range");
    maxc = std::max(maxc, count[b]);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const int cap = (batch + 1) & ~1;
  const long xs = (long)((stride + 3) & ~(int64_t)3), ys = (long)((std::max<int64_t>(out_stride, 1) + 3) & ~(int64_t)3);
  float *dx = nullptr, *dy = nullptr;
  int *hrows = nullptr, *drows = nullptr;
  auto release = [&]() {
    if (dx) hipFree(dx);
    if (dy) hipFree(dy);
    if (drows) hipFree(drows);
    if (hrows) hipHostFree(hrows);
  };
  try {
    PE_HIP(hipMalloc((void**)&dx, (size_t)batch * std::max<long>(xs, 4) * sizeof(float)));
    PE_HIP(hipMalloc((void**)&dy, (size_t)batch * ys * sizeof(float)));
    PE_HIP(hipMalloc((void**)&drows, (size_t)rs_words(cap) * sizeof(int)));
    PE_HIP(hipHostMalloc((void**)&hrows, (size_t)rs_words(cap) * sizeof(int)));
    memset(hrows, 0, (size_t)rs_words(cap) * sizeof(int));
    for (int b = 0; b < batch; ++b) {
      reinterpret_cast<long long*>(hrows)[b] = n0[b];
      reinterpret_cast<long long*>(hrows + rs_o_org(cap))[b] = origin[b];
      hrows[rs_o_count(cap) + b] = count[b];
      hrows[rs_o_vlen(cap) + b] = vlen[b];
      if (stride > 0)
        PE_HIP(hipMemcpyAsync(dx + (size_t)b * xs, x + (size_t)b * stride, (size_t)stride * sizeof(float), hipMemcpyHostToDevice, stream_));
    }
    PE_HIP(hipMemsetAsync(dy, 0xFF, (size_t)batch * ys * sizeof(float), stream_));
    launch::resample_rows(stream_, hrows, nullptr, 0, drows, cap, batch, (long)stride, (long)out_stride, rs_L_, rs_M_);
    if (maxc > 0) {
      RsP p{};
      p.x = dx; p.x_bs = xs; p.y = dy; p.y_bs = ys;
      p.coef = rs_coef_; p.L = rs_L_; p.M = rs_M_; p.K = rs_K_; p.Tp = rs_Tp_;
      p.rows = drows; p.cap = cap; p.tile = rs_tile_;
      launch::resample(dim3((maxc + rs_tile_ - 1) / rs_tile_, batch), stream_, p);
    }
    for (int b = 0; b < batch; ++b)
      if (count[b] > 0)
        PE_HIP(hipMemcpyAsync(out + (size_t)b * out_stride, dy + (size_t)b * ys, (size_t)count[b] * sizeof(float), hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

// ------------------------------------------------------------------------------------------------
// target loudness
// ------------------------------------------------------------------------------------------------

// The K-weighting biquads from their analog prototypes by the bilinear transform: at 48000 Hz the
// coefficient table of ITU-R BS.1770-4 to 1e-14.
void Engine::loudness_filter(int fs, double coef[10]) {
  if (fs < 4000 || fs > 192000) throw std::runtime_error("loudness filter: rate " + std::to_string(fs) + " Hz outside [4000, 192000]");
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / (double)fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    coef[0] = (Vh + Vb * K / Q + K * K) / a0;
    coef[1] = 2.0 * (K * K - Vh) / a0;
    coef[2] = (Vh - Vb * K / Q + K * K) / a0;
    coef[3] = 2.0 * (K * K - 1.0) / a0;
    coef[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / (double)fs), a0 = 1.0 + K / Q + K * K;
    coef[5] = 1.0; coef[6] = -2.0; coef[7] = 1.0;
    coef[8] = 2.0 * (K * K - 1.0) / a0;
    coef[9] = (1.0 - K / Q + K * K) / a0;
  }
}

void Engine::loud_check_rate(int fs) {
  if (fs <= 0)
    throw std::runtime_error("the target loudness needs the delivered sample rate, and this voice carries none (an .onnx does "
                             "not): call pe_set_output_rate with the sample rate of its .onnx.json first");
  if (fs < 4000 || fs > 192000)
    throw std::runtime_error("the target loudness is not available at " + std::to_string(fs) + " Hz (outside [4000, 192000])");
}

// Everything of the setting that follows the rate: the segment length h = 100 ms, the warm-up W = 50 ms (12 time constants
// of the high-pass's double pole at 38 Hz: (1 + 12) e^-12 = 8e-5 of a state's start is left), the run R of one thread, and
// the filter block -- the coefficients and A^(R 2^k), A = what one sample of silence makes of the four states (the state
// update of loud_step, kernels/loudness.h, with x = 0).
static void loud_plan(int fs, int& h, int& W, int& R, double* blk) {
  Engine::loudness_filter(fs, blk);
  h = (fs + 5) / 10;
  W = (fs + 10) / 20;
  R = (h + W + LOUD_TPB - 1) / LOUD_TPB;
  const double* c = blk;
  long double A[4][4], P[4][4], Tm[4][4];
  for (int col = 0; col < 4; ++col) {
    long double z[4] = {0, 0, 0, 0};
    z[col] = 1;
    const long double ya = z[0];
    const long double n0 = -c[3] * ya + z[1], n1 = -c[4] * ya;
    const long double yb = c[5] * ya + z[2];
    const long double n2 = -c[8] * yb + c[6] * ya + z[3], n3 = -c[9] * yb + c[7] * ya;
    A[0][col] = n0; A[1][col] = n1; A[2][col] = n2; A[3][col] = n3;
  }
  auto mul = [&](long double (&X)[4][4], long double (&Y)[4][4], long double (&Z)[4][4]) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        long double v = 0;
        for (int k = 0; k < 4; ++k) v += X[i][k] * Y[k][j];
        Z[i][j] = v;
      }
  };
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) P[i][j] = i == j ? 1 : 0;
  for (int r = 0; r < R; ++r) { mul(A, P, Tm); memcpy(P, Tm, sizeof(P)); }
  for (int k = 0; k < LOUD_LEVELS; ++k) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) blk[10 + 16 * k + 4 * i + j] = (double)P[i][j];
    mul(P, P, Tm);
    memcpy(P, Tm, sizeof(P));
  }
}

void Engine::loud_upload_filter(int fs) {
  double blk[LOUD_COEF_DOUBLES];
  int h, W, R;
  loud_plan(fs, h, W, R, blk);
  if (!ld_coef_) PE_HIP(hipMalloc((void**)&ld_coef_, sizeof(blk)));
  PE_HIP(hipMemcpy(ld_coef_, blk, sizeof(blk), hipMemcpyHostToDevice));
  ld_fs_ = fs; ld_h_ = h; ld_W_ = W; ld_R_ = R;
}

void Engine::loud_write_ctl() {
  if (!ld_ctl_) return;
  const float C = (float)std::pow(10.0, (double)ld_cdb_ / 20.0);
  memcpy(ld_ctl_, &ld_T_, sizeof(float));
  memcpy(ld_ctl_ + 1, &C, sizeof(float));
}

void Engine::loud_free() {
  if (ld_coef_) hipFree(ld_coef_);
  if (ld_seg_) hipFree(ld_seg_);
  if (ld_dev_) hipFree(ld_dev_);
  if (ld_ctl_) hipHostFree(ld_ctl_);
  if (tp_coef_) hipFree(tp_coef_);
  if (tp_words_) hipFree(tp_words_);
  ld_coef_ = ld_seg_ = nullptr; ld_dev_ = ld_ctl_ = nullptr;
  ld_seg_rows_ = 0; ld_nseg_cap_ = 0; ld_cap_ = 0;
  tp_coef_ = nullptr; tp_words_ = nullptr; tp_fs_ = tp_Q_ = tp_cap_ = 0;
  if (lim_h_) hipFree(lim_h_);
  if (lim_rep_) hipFree(lim_rep_);
  if (lim_host_) hipHostFree(lim_host_);
  if (lim_v_) hipFree(lim_v_);
  if (lim_z_) hipFree(lim_z_);
  lim_v_ = lim_z_ = nullptr; lim_zv_floats_ = 0;
  lim_h_ = nullptr; lim_rep_ = lim_host_ = nullptr; lim_fs_ = lim_W_ = lim_cap_ = 0; lim_h_ms_ = 0.f;
}

void Engine::tp_check_rate(int fs) {
  if (fs < 8000 || fs > 48000)
    throw std::runtime_error("the true-peak ceiling is not available at " + std::to_string(fs) + " Hz (outside [8000, 48000])");
}

void Engine::true_peak_filter(int fs, int& Q, int& K, std::vector<double>& coef) {
  tp_check_rate(fs);
  Q = true_peak_oversample(fs);
  int L, M, Tp;
  resample_filter(fs, Q * fs, L, M, K, Tp, &coef);
  if (L != Q || M != 1 || K != TP_K || Tp != TP_TAPS || Q > TP_MAXQ)
    throw std::runtime_error("true-peak filter at " + std::to_string(fs) + " Hz: unexpected geometry");
}

void Engine::tp_upload_table(int fs) {
  int Q, K;
  std::vector<double> exact;
  true_peak_filter(fs, Q, K, exact);
  float table[TP_MAXQ * TP_TAPS] = {};
  for (size_t i = 0; i < exact.size(); ++i) table[i] = (float)exact[i];
  if (!tp_coef_) PE_HIP(hipMalloc((void**)&tp_coef_, sizeof(table)));
  PE_HIP(hipMemcpy(tp_coef_, table, sizeof(table), hipMemcpyHostToDevice));
  tp_fs_ = fs; tp_Q_ = Q;
}

void Engine::set_loudness_ceiling(int kind) {
  EntryLock entry_lock;
  if (kind != PEAK_SAMPLE && kind != PEAK_TRUE)
    throw std::runtime_error("unknown loudness ceiling kind " + std::to_string(kind) + " (0: sample peak, 1: true peak)");
  if (kind == PEAK_TRUE && ld_on_) tp_check_rate(output_rate());
  lim_check(kind, lim_on_, lim_ms_);
  if (kind == ld_kind_) return;
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  // the kind picks the launches and is part of the graph keys: nothing is dropped, streams are not touched
  ld_kind_ = kind;
}

void Engine::lim_check(int kind, bool on, float window_ms) {
  if (!on) return;
  if (!std::isfinite(window_ms) || window_ms < 1.f || window_ms > 10.f)
    throw std::runtime_error("limiter window " + std::to_string(window_ms) + " ms outside [1, 10]");
  (void)kind;
}

// h_k = H_k / sum H, H_k = (1 + cos(pi k / (W + 1))) / 2, k = -W .. W: a raised cosine that ends above zero, in f64
void Engine::limiter_window(int fs, float window_ms, int& W, std::vector<double>& coef) {
  lim_check(PEAK_SAMPLE, true, window_ms);
  loud_check_rate(fs);
  W = limiter_window_samples(fs, (double)window_ms);
  if (W > LIM_MAXW) throw std::runtime_error("limiter window of " + std::to_string(W) + " samples at " + std::to_string(fs) +
                                             " Hz, more than " + std::to_string(LIM_MAXW));
  coef.assign((size_t)(2 * W + 1), 0.0);
  const double pi = 3.14159265358979323846;
  double sum = 0;
  for (int k = -W; k <= W; ++k) sum += coef[(size_t)(k + W)] = 0.5 * (1.0 + std::cos(pi * (double)k / (double)(W + 1)));
  for (double& c : coef) c /= sum;
}

void Engine::lim_upload_window(int fs) {
  int W;
  std::vector<double> exact;
  limiter_window(fs, lim_ms_, W, exact);
  float table[2 * LIM_MAXW + 1] = {};
  for (size_t i = 0; i < exact.size(); ++i) table[i] = (float)exact[i];
  if (!lim_h_) PE_HIP(hipMalloc((void**)&lim_h_, sizeof(table)));
  PE_HIP(hipMemcpy(lim_h_, table, sizeof(table), hipMemcpyHostToDevice));
  lim_fs_ = fs; lim_W_ = W; lim_h_ms_ = lim_ms_;
}

void Engine::set_loudness_limiter(bool on, float window_ms) {
  EntryLock entry_lock;
  lim_check(ld_kind_, on, window_ms);
  if (on && ld_on_ && limiter_window_samples(output_rate(), (double)window_ms) > LIM_MAXW)
    throw std::runtime_error("limiter window " + std::to_string(window_ms) + " ms is more than " + std::to_string(LIM_MAXW) +
                             " samples at " + std::to_string(output_rate()) + " Hz");
  if (on == lim_on_ && (!on || window_ms == lim_ms_)) return;
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  PE_HIP(hipStreamSynchronize(stream_));
  // on / off picks the launches and is part of the graph keys: nothing is dropped. A new window is a new kernel argument
  // (and a new table behind the same pointer): the graphs go, as with a new rate.
  if (on && lim_h_ && window_ms != lim_h_ms_) drop_graphs();
  lim_on_ = on;
  if (on) lim_ms_ = window_ms;
}

void Engine::set_loudness(bool on, float target_lufs, float ceiling_db) {
  EntryLock entry_lock;
  if (on) {
    if (!std::isfinite(target_lufs) || target_lufs < -40.f || target_lufs > -5.f)
      throw std::runtime_error("target loudness " + std::to_string(target_lufs) + " LUFS outside [-40, -5]");
    if (!std::isfinite(ceiling_db) || ceiling_db < -20.f || ceiling_db > 0.f)
      throw std::runtime_error("peak ceiling " + std::to_string(ceiling_db) + " dB outside [-20, 0]");
    loud_check_rate(output_rate());
    if (ld_kind_ == PEAK_TRUE) tp_check_rate(output_rate());
    if (lim_on_ && limiter_window_samples(output_rate(), (double)lim_ms_) > LIM_MAXW)
      throw std::runtime_error("limiter window " + std::to_string(lim_ms_) + " ms is more than " + std::to_string(LIM_MAXW) +
                               " samples at " + std::to_string(output_rate()) + " Hz");
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  PE_HIP(hipStreamSynchronize(stream_));               // nothing on the device reads the control block any more
  if (on) {
    if (!ld_coef_ || ld_fs_ != output_rate()) {
      if (ld_coef_) drop_graphs();                     // (h / W / R are kernel arguments inside the graphs)
      loud_upload_filter(output_rate());
    }
    ld_T_ = target_lufs; ld_cdb_ = ceiling_db;
    loud_write_ctl();
  }
  // target and ceiling are data; on / off picks the launches and is part of the graph keys, so nothing else is dropped:
  // both sets of graphs stay cached side by side. Streams are not touched.
  ld_on_ = on;
}

// The segment sums [capB_B_][So_ / h + 2] and the control / gain blocks, (re)allocated when the workspace capacity or the
// rate grew; called at the end of ensure_stage_b, which has set So_.
void Engine::ensure_loudness() {
  if (!ld_coef_ || ld_fs_ != output_rate()) loud_upload_filter(output_rate());
  const int nseg = (int)(So_ / ld_h_) + 2;
  const int want_cap = (int)((std::max<size_t>(std::max(capA_B_, capB_B_), 64) + 1) & ~(size_t)1);
  if (ld_kind_ == PEAK_TRUE) {
    // (a first allocation is in no graph yet; a changed table or grown words are inside the PEAK_TRUE graphs)
    if (!tp_coef_ || tp_fs_ != output_rate()) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (tp_coef_) drop_graphs();
      tp_upload_table(output_rate());
    }
    if (!tp_words_ || tp_cap_ < want_cap) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (tp_words_) { drop_graphs(); PE_HIP(hipFree(tp_words_)); tp_words_ = nullptr; }
      tp_cap_ = 0;
      PE_HIP(hipMalloc((void**)&tp_words_, (size_t)want_cap * sizeof(unsigned)));
      if (pol_.debug_poison) poison(tp_words_, (size_t)want_cap * sizeof(unsigned));
      else PE_HIP(hipMemset(tp_words_, 0, (size_t)want_cap * sizeof(unsigned)));
      PE_HIP(hipDeviceSynchronize());
      tp_cap_ = want_cap;
    }
  }
  if (lim_on_) {
    // (as above: a first allocation is in no graph yet; a changed table or grown words are inside the limiter's graphs)
    if (!lim_h_ || lim_fs_ != output_rate() || lim_h_ms_ != lim_ms_) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (lim_h_) drop_graphs();
      lim_upload_window(output_rate());
    }
    if (!lim_rep_ || lim_cap_ < want_cap) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (lim_rep_) { drop_graphs(); PE_HIP(hipFree(lim_rep_)); lim_rep_ = nullptr; }
      if (lim_host_) { PE_HIP(hipHostFree(lim_host_)); lim_host_ = nullptr; }
      lim_cap_ = 0;
      PE_HIP(hipMalloc((void**)&lim_rep_, (size_t)lim_words(want_cap) * sizeof(int)));
      PE_HIP(hipHostMalloc((void**)&lim_host_, (size_t)lim_words(want_cap) * sizeof(int)));
      memset(lim_host_, 0, (size_t)lim_words(want_cap) * sizeof(int));
      if (pol_.debug_poison) poison(lim_rep_, (size_t)lim_words(want_cap) * sizeof(int));
      else PE_HIP(hipMemset(lim_rep_, 0, (size_t)lim_words(want_cap) * sizeof(int)));
      PE_HIP(hipDeviceSynchronize());
      lim_cap_ = want_cap;
    }
    if (ld_kind_ == PEAK_TRUE) {
      const size_t want = std::max<size_t>(capB_B_, 1) * (size_t)std::max<long>(std::max<long>(So_, Ss_), 4);
      if (!lim_z_ || !lim_v_ || lim_zv_floats_ < want) {
        PE_HIP(hipStreamSynchronize(stream_));
        if (lim_z_ || lim_v_) drop_graphs();
        if (lim_z_) { PE_HIP(hipFree(lim_z_)); lim_z_ = nullptr; }
        if (lim_v_) { PE_HIP(hipFree(lim_v_)); lim_v_ = nullptr; }
        lim_zv_floats_ = 0;
        if (hipMalloc((void**)&lim_z_, want * sizeof(float)) != hipSuccess || hipMalloc((void**)&lim_v_, want * sizeof(float)) != hipSuccess) {
          (void)hipGetLastError();
          if (lim_z_) { hipFree(lim_z_); lim_z_ = nullptr; }
          lim_v_ = nullptr;
          throw std::runtime_error("out of device memory: " + std::to_string((2 * want * sizeof(float)) >> 20) + " MiB of limiter rows");
        }
        if (pol_.debug_poison) { poison(lim_z_, want * sizeof(float)); poison(lim_v_, want * sizeof(float)); }
        PE_HIP(hipDeviceSynchronize());
        lim_zv_floats_ = want;
      }
    }
  }
  if (ld_seg_ && ld_seg_rows_ >= capB_B_ && ld_nseg_cap_ >= nseg && ld_ctl_ && ld_dev_ && ld_cap_ >= want_cap) return;
  PE_HIP(hipStreamSynchronize(stream_));
  drop_graphs();
  if (!(ld_seg_ && ld_seg_rows_ >= capB_B_ && ld_nseg_cap_ >= nseg)) {
    if (ld_seg_) { PE_HIP(hipFree(ld_seg_)); ld_seg_ = nullptr; }
    const size_t rows = std::max(ld_seg_rows_, capB_B_);
    const int cols = std::max(ld_nseg_cap_, nseg);
    ld_seg_rows_ = 0; ld_nseg_cap_ = 0;
    if (hipMalloc((void**)&ld_seg_, rows * (size_t)cols * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      ld_seg_ = nullptr;
      throw std::runtime_error("out of device memory: " + std::to_string((rows * (size_t)cols * sizeof(double)) >> 20) + " MiB of loudness segment sums");
    }
    if (pol_.debug_poison) poison(ld_seg_, rows * (size_t)cols * sizeof(double));
    ld_seg_rows_ = rows; ld_nseg_cap_ = cols;
  }
  if (!(ld_ctl_ && ld_dev_ && ld_cap_ >= want_cap)) {
    if (ld_ctl_) { PE_HIP(hipHostFree(ld_ctl_)); ld_ctl_ = nullptr; }
    if (ld_dev_) { PE_HIP(hipFree(ld_dev_)); ld_dev_ = nullptr; }
    ld_cap_ = 0;
    PE_HIP(hipHostMalloc((void**)&ld_ctl_, (size_t)ldc_words(want_cap) * sizeof(int)));
    PE_HIP(hipMalloc((void**)&ld_dev_, (size_t)ld_words(want_cap) * sizeof(int)));
    memset(ld_ctl_, 0, (size_t)ldc_words(want_cap) * sizeof(int));
    PE_HIP(hipMemset(ld_dev_, 0, (size_t)ld_words(want_cap) * sizeof(int)));
    PE_HIP(hipDeviceSynchronize());
    ld_cap_ = want_cap;
    loud_write_ctl();
  }
}

void Engine::lim_enqueue_report() {
  if (!run_lim_ || !lim_rep_ || !lim_host_ || B_ > lim_cap_) return;
  PE_HIP(hipMemcpyAsync(lim_host_, lim_rep_, (size_t)lim_words(lim_cap_) * sizeof(int), hipMemcpyDeviceToHost, stream_));
}

void Engine::loud_collect() {
  ll_tn_ = 0;
  ll_ln_ = 0;
  if (!ld_on_ || !ld_ctl_ || B_ > ld_cap_) { ll_n_ = 0; return; }
  const int n = B_, cap = ld_cap_;
  if (run_lim_ && lim_host_ && n <= lim_cap_) {
    const float* mr = reinterpret_cast<const float*>(lim_host_) + lim_o_maxred(lim_cap_);
    ll_maxred_.assign(mr, mr + n);
    ll_shaped_.assign(lim_host_ + lim_o_count(lim_cap_), lim_host_ + lim_o_count(lim_cap_) + n);
    const float* tr = reinterpret_cast<const float*>(lim_host_) + lim_o_trim(lim_cap_);
    ll_trim_.assign(tr, tr + n);
    ll_ln_ = n;
  }
  if (ld_kind_ == PEAK_TRUE) {
    const float* tf = reinterpret_cast<const float*>(ld_ctl_) + ldc_o_tpeak(cap);
    ll_tpeak_.assign(tf, tf + n);
    ll_tn_ = n;
  }
  const float* rf = reinterpret_cast<const float*>(ld_ctl_ + ldc_o_report(cap));
  ll_lufs_.assign(rf, rf + n);
  ll_scale_.assign(rf + ld_o_scale(cap), rf + ld_o_scale(cap) + n);
  ll_peak_.assign(rf + ld_o_peak(cap), rf + ld_o_peak(cap) + n);
  ll_flags_.assign(ld_ctl_ + ldc_o_report(cap) + ld_o_flags(cap), ld_ctl_ + ldc_o_report(cap) + ld_o_flags(cap) + n);
  ll_n_ = n;
}

int Engine::last_loudness(float* lufs, float* scale, float* peak, int32_t* flags, int64_t capacity) {
  EntryLock entry_lock;
  if (ll_n_ < 0) throw std::runtime_error("no whole-utterance call fetched on this handle yet");
  if ((lufs || scale || peak || flags) && capacity < ll_n_) throw std::runtime_error("loudness report buffer too small");
  for (int b = 0; b < ll_n_; ++b) {
    if (lufs) lufs[b] = ll_lufs_[b];
    if (scale) scale[b] = ll_scale_[b];
    if (peak) peak[b] = ll_peak_[b];
    if (flags) flags[b] = ll_flags_[b];
  }
  return ll_n_;
}

int Engine::last_limiter(float* max_reduction, int32_t* shaped_samples, float* trim, int64_t capacity) {
  EntryLock entry_lock;
  if (ll_n_ < 0) throw std::runtime_error("no whole-utterance call fetched on this handle yet");
  if ((max_reduction || shaped_samples || trim) && capacity < ll_ln_) throw std::runtime_error("limiter report buffer too small");
  for (int b = 0; b < ll_ln_; ++b) {
    if (max_reduction) max_reduction[b] = ll_maxred_[b];
    if (shaped_samples) shaped_samples[b] = ll_shaped_[b];
    if (trim) trim[b] = ll_trim_[b];
  }
  return ll_ln_;
}

void Engine::debug_limiter(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, const float* g, float ceiling_db,
                           int kind, float window_ms, float* env, int16_t* pcm) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !g || !env || !pcm) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  if (!std::isfinite(ceiling_db) || ceiling_db < -20.f || ceiling_db > 0.f)
    throw std::runtime_error("peak ceiling " + std::to_string(ceiling_db) + " dB outside [-20, 0]");
  if (kind != PEAK_SAMPLE && kind != PEAK_TRUE)
    throw std::runtime_error("unknown loudness ceiling kind " + std::to_string(kind) + " (0: sample peak, 1: true peak)");
  lim_check(kind, true, window_ms);
  int W, maxn = 0;
  std::vector<double> exact;
  limiter_window(fs, window_ms, W, exact);
  float table[2 * LIM_MAXW + 1] = {};
  for (size_t i = 0; i < exact.size(); ++i) table[i] = (float)exact[i];
  const int cap = (batch + 1) & ~1;
  const float C = (float)std::pow(10.0, (double)ceiling_db / 20.0);
  std::vector<int> gq((size_t)ld_words(cap), 0);
  std::vector<float> peak((size_t)batch, 0.f);
  for (int b = 0; b < batch; ++b) {
    if (valid[b] < 0 || valid[b] > stride) throw std::runtime_error("row " + std::to_string(b) + ": valid length outside [0, stride]");
    if (!std::isfinite(g[b]) || !(g[b] > 0.f)) throw std::runtime_error("row " + std::to_string(b) + ": gain " + std::to_string(g[b]) + " is not positive and finite");
    maxn = std::max(maxn, valid[b]);
    for (int i = 0; i < valid[b]; ++i) peak[b] = std::max(peak[b], std::fabs(x[(size_t)b * stride + i]));
  }
  // (the rule of loudness_gain_kernel: the ceiling's term is the smaller; P = max(p, t) with the true-peak ceiling)
  auto fill_gq = [&](const float* tpk) {
    for (int b = 0; b < batch; ++b) {
      const float scale = 32767.0f * g[b], P = tpk ? std::max(peak[b], tpk[b]) : peak[b];
      memcpy(&gq[(size_t)ld_o_scale(cap) + b], &scale, sizeof(float));
      memcpy(&gq[(size_t)ld_o_peak(cap) + b], &peak[b], sizeof(float));
      gq[(size_t)ld_o_flags(cap) + b] = (P > 0.f && (double)C / (double)P < (double)g[b]) ? (LOUD_LIMITED | LOUD_SHAPED) : 0;
    }
  };
  const bool tp = kind == PEAK_TRUE;
  int Q = 0, Kh = 0;
  float tptable[TP_MAXQ * TP_TAPS] = {};
  if (tp) {
    std::vector<double> tex;
    true_peak_filter(fs, Q, Kh, tex);
    for (size_t i = 0; i < tex.size(); ++i) tptable[i] = (float)tex[i];
  } else {
    fill_gq(nullptr);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const long xs = (long)((std::max<int64_t>(stride, 1) + 3) & ~(int64_t)3);
  float *dx = nullptr, *dh = nullptr, *denv = nullptr, *dv = nullptr, *dz = nullptr, *dtab = nullptr;
  int *dval = nullptr, *dgq = nullptr, *dctl = nullptr, *drep = nullptr;
  unsigned* dtp = nullptr;
  int16_t* dpcm = nullptr;
  auto release = [&]() {
    if (dv) hipFree(dv);
    if (dz) hipFree(dz);
    if (dtab) hipFree(dtab);
    if (dtp) hipFree(dtp);
    if (dx) hipFree(dx);
    if (dh) hipFree(dh);
    if (denv) hipFree(denv);
    if (dval) hipFree(dval);
    if (dgq) hipFree(dgq);
    if (dctl) hipFree(dctl);
    if (drep) hipFree(drep);
    if (dpcm) hipFree(dpcm);
  };
  try {
    const float ctl[2] = {0.f, C};
    PE_HIP(hipMalloc((void**)&dx, (size_t)batch * xs * sizeof(float)));
    PE_HIP(hipMalloc((void**)&denv, (size_t)batch * xs * sizeof(float)));
    PE_HIP(hipMalloc((void**)&dpcm, (size_t)batch * xs * sizeof(int16_t)));
    PE_HIP(hipMalloc((void**)&dh, sizeof(table)));
    PE_HIP(hipMalloc((void**)&dval, (size_t)batch * sizeof(int)));
    PE_HIP(hipMalloc((void**)&dgq, gq.size() * sizeof(int)));
    PE_HIP(hipMalloc((void**)&dctl, (size_t)ldc_words(cap) * sizeof(int)));      // (pcm16_trim_kernel writes the report's scale)
    PE_HIP(hipMalloc((void**)&drep, (size_t)lim_words(cap) * sizeof(int)));
    for (int b = 0; b < batch; ++b)
      if (stride > 0) {
        PE_HIP(hipMemcpyAsync(dx + (size_t)b * xs, x + (size_t)b * stride, (size_t)stride * sizeof(float), hipMemcpyHostToDevice, stream_));
        // (what lies behind a row's end comes back as the caller left it)
        PE_HIP(hipMemcpyAsync(denv + (size_t)b * xs, env + (size_t)b * stride, (size_t)stride * sizeof(float), hipMemcpyHostToDevice, stream_));
        PE_HIP(hipMemcpyAsync(dpcm + (size_t)b * xs, pcm + (size_t)b * stride, (size_t)stride * sizeof(int16_t), hipMemcpyHostToDevice, stream_));
      }
    PE_HIP(hipMemcpyAsync(dh, table, sizeof(table), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval, valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(drep, 0, (size_t)lim_words(cap) * sizeof(int), stream_));
    TpP tq{};
    if (tp) {
      // the first true-peak pass: t for the rule, v for the envelope
      PE_HIP(hipMalloc((void**)&dv, (size_t)batch * xs * sizeof(float)));
      PE_HIP(hipMalloc((void**)&dz, (size_t)batch * xs * sizeof(float)));
      PE_HIP(hipMalloc((void**)&dtab, sizeof(tptable)));
      PE_HIP(hipMalloc((void**)&dtp, (size_t)batch * sizeof(unsigned)));
      PE_HIP(hipMemcpyAsync(dtab, tptable, sizeof(tptable), hipMemcpyHostToDevice, stream_));
      PE_HIP(hipMemsetAsync(dtp, 0, (size_t)batch * sizeof(unsigned), stream_));
      PE_HIP(hipMemsetAsync(dv, 0xFF, (size_t)batch * xs * sizeof(float), stream_));
      PE_HIP(hipMemsetAsync(dz, 0xFF, (size_t)batch * xs * sizeof(float), stream_));
      PE_HIP(hipStreamSynchronize(stream_));
      tq.x = dx; tq.x_bs = xs; tq.lens = dval; tq.len_mul = 1; tq.x_cap = (long)stride;
      tq.coef = dtab; tq.Q = Q; tq.tpeak = dtp; tq.v = dv;
      launch::true_peak_v(dim3((unsigned)std::max(1, (maxn + TP_TILE - 1) / TP_TILE), batch), stream_, tq);
      std::vector<float> tpk((size_t)batch, 0.f);
      PE_HIP(hipMemcpyAsync(tpk.data(), dtp, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, stream_));
      PE_HIP(hipStreamSynchronize(stream_));
      fill_gq(tpk.data());
    }
    PE_HIP(hipMemcpyAsync(dgq, gq.data(), gq.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging arrays are pageable)
    LimP p{};
    p.x = dx; p.x_bs = xs; p.lens = dval; p.len_mul = 1; p.x_cap = (long)stride;
    p.gq = dgq; p.gcap = cap; p.ctl = dctl; p.h = dh; p.W = W;
    p.pcm = dpcm; p.p_bs = xs; p.host = nullptr; p.rep = drep; p.rcap = cap; p.env = denv; p.e_bs = xs;
    if (tp) {
      p.v = dv; p.z = dz;
      launch::limiter_true(dim3((unsigned)std::max(1, (maxn + LIM_TILE - 1) / LIM_TILE), batch), stream_, p);
      tq.x = dz; tq.v = nullptr; tq.tpeak = reinterpret_cast<unsigned*>(drep) + lim_o_tz(cap);
      launch::true_peak(dim3((unsigned)std::max(1, (maxn + TP_TILE - 1) / TP_TILE), batch), stream_, tq);
      TrimP r{};
      r.z = dz; r.z_bs = xs; r.lens = dval; r.len_mul = 1; r.gq = dgq; r.gcap = cap; r.ctl = dctl;
      r.rep = drep; r.rcap = cap; r.pcm = dpcm; r.p_bs = xs; r.host = nullptr;
      launch::pcm16_trim(dim3((unsigned)std::max(1, (maxn + 255) / 256), batch), stream_, r);
    } else
    launch::limiter(dim3((unsigned)std::max(1, (maxn + LIM_TILE - 1) / LIM_TILE), batch), stream_, p);
    for (int b = 0; b < batch; ++b)
      if (stride > 0) {
        PE_HIP(hipMemcpyAsync(env + (size_t)b * stride, denv + (size_t)b * xs, (size_t)stride * sizeof(float), hipMemcpyDeviceToHost, stream_));
        PE_HIP(hipMemcpyAsync(pcm + (size_t)b * stride, dpcm + (size_t)b * xs, (size_t)stride * sizeof(int16_t), hipMemcpyDeviceToHost, stream_));
      }
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

int Engine::last_true_peak(float* t, int64_t capacity) {
  EntryLock entry_lock;
  if (ll_n_ < 0) throw std::runtime_error("no whole-utterance call fetched on this handle yet");
  if (t && capacity < ll_tn_) throw std::runtime_error("true-peak report buffer too small");
  if (t)
    for (int b = 0; b < ll_tn_; ++b) t[b] = ll_tpeak_[b];
  return ll_tn_;
}

void Engine::debug_true_peak(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float* t) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !t) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  int Q, K, maxn = 0;
  std::vector<double> exact;
  true_peak_filter(fs, Q, K, exact);
  float table[TP_MAXQ * TP_TAPS] = {};
  for (size_t i = 0; i < exact.size(); ++i) table[i] = (float)exact[i];
  for (int b = 0; b < batch; ++b) {
    if (valid[b] < 0 || valid[b] > stride) throw std::runtime_error("row " + std::to_string(b) + ": valid length outside [0, stride]");
    maxn = std::max(maxn, valid[b]);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const long xs = (long)((std::max<int64_t>(stride, 1) + 3) & ~(int64_t)3);
  float *dx = nullptr, *dcoef = nullptr;
  int* dval = nullptr;
  unsigned* dtp = nullptr;
  auto release = [&]() {
    if (dx) hipFree(dx);
    if (dcoef) hipFree(dcoef);
    if (dval) hipFree(dval);
    if (dtp) hipFree(dtp);
  };
  try {
    PE_HIP(hipMalloc((void**)&dx, (size_t)batch * xs * sizeof(float)));
    PE_HIP(hipMalloc((void**)&dcoef, sizeof(table)));
    PE_HIP(hipMalloc((void**)&dval, (size_t)batch * sizeof(int)));
    PE_HIP(hipMalloc((void**)&dtp, (size_t)batch * sizeof(unsigned)));
    for (int b = 0; b < batch; ++b)
      if (stride > 0)
        PE_HIP(hipMemcpyAsync(dx + (size_t)b * xs, x + (size_t)b * stride, (size_t)stride * sizeof(float), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dcoef, table, sizeof(table), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval, valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(dtp, 0, (size_t)batch * sizeof(unsigned), stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging arrays are pageable)
    TpP p{};
    p.x = dx; p.x_bs = xs; p.lens = dval; p.len_mul = 1; p.x_cap = (long)stride;
    p.coef = dcoef; p.Q = Q; p.tpeak = dtp;
    launch::true_peak(dim3((unsigned)std::max(1, (maxn + TP_TILE - 1) / TP_TILE), batch), stream_, p);
    PE_HIP(hipMemcpyAsync(t, dtp, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

void Engine::debug_loudness(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float target, float ceiling_db,
                            float* lufs, float* scale, int32_t* flags) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !lufs || !scale || !flags) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  if (!std::isfinite(target) || target < -40.f || target > -5.f)
    throw std::runtime_error("target loudness " + std::to_string(target) + " LUFS outside [-40, -5]");
  if (!std::isfinite(ceiling_db) || ceiling_db < -20.f || ceiling_db > 0.f)
    throw std::runtime_error("peak ceiling " + std::to_string(ceiling_db) + " dB outside [-20, 0]");
  loud_check_rate(fs);
  int maxn = 0;
  std::vector<unsigned> peaks((size_t)batch, 0u);
  for (int b = 0; b < batch; ++b) {
    if (valid[b] < 0 || valid[b] > stride) throw std::runtime_error("row " + std::to_string(b) + ": valid length outside [0, stride]");
    maxn = std::max(maxn, valid[b]);
    float m = 0.f;
    for (int i = 0; i < valid[b]; ++i) m = std::max(m, std::fabs(x[(size_t)b * stride + i]));
    memcpy(&peaks[b], &m, sizeof(float));
  }
  double blk[LOUD_COEF_DOUBLES];
  int h, W, R;
  loud_plan(fs, h, W, R, blk);
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const int cap = (batch + 1) & ~1, nseg_cap = maxn / h + 2;
  const long xs = (long)((std::max<int64_t>(stride, 1) + 3) & ~(int64_t)3);
  float* dx = nullptr;
  double *dcoef = nullptr, *dseg = nullptr;
  int *dval = nullptr, *ctl = nullptr, *gd = nullptr;
  unsigned* dpk = nullptr;
  auto release = [&]() {
    if (dx) hipFree(dx);
    if (dcoef) hipFree(dcoef);
    if (dseg) hipFree(dseg);
    if (dval) hipFree(dval);
    if (dpk) hipFree(dpk);
    if (gd) hipFree(gd);
    if (ctl) hipHostFree(ctl);
  };
  try {
    PE_HIP(hipMalloc((void**)&dx, (size_t)batch * xs * sizeof(float)));
    PE_HIP(hipMalloc((void**)&dcoef, sizeof(blk)));
    PE_HIP(hipMalloc((void**)&dseg, (size_t)batch * nseg_cap * sizeof(double)));
    PE_HIP(hipMalloc((void**)&dval, (size_t)batch * sizeof(int)));
    PE_HIP(hipMalloc((void**)&dpk, (size_t)batch * sizeof(unsigned)));
    PE_HIP(hipMalloc((void**)&gd, (size_t)ld_words(cap) * sizeof(int)));
    PE_HIP(hipHostMalloc((void**)&ctl, (size_t)ldc_words(cap) * sizeof(int)));
    memset(ctl, 0, (size_t)ldc_words(cap) * sizeof(int));
    const float C = (float)std::pow(10.0, (double)ceiling_db / 20.0);
    memcpy(ctl, &target, sizeof(float));
    memcpy(ctl + 1, &C, sizeof(float));
    for (int b = 0; b < batch; ++b)
      if (stride > 0)
        PE_HIP(hipMemcpyAsync(dx + (size_t)b * xs, x + (size_t)b * stride, (size_t)stride * sizeof(float), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dcoef, blk, sizeof(blk), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval, valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dpk, peaks.data(), (size_t)batch * sizeof(unsigned), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(dseg, 0xFF, (size_t)batch * nseg_cap * sizeof(double), stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging vectors are pageable)
    LoudP p{};
    p.x = dx; p.x_bs = xs; p.lens = dval; p.len_mul = 1; p.x_cap = (long)stride;
    p.coef = dcoef; p.h = h; p.W = W; p.R = R; p.seg = dseg; p.nseg_cap = nseg_cap;
    launch::loudness_seg(dim3((unsigned)std::max(1, (maxn + h - 1) / h), batch), stream_, p);
    launch::loudness_gain(stream_, batch, dseg, nseg_cap, dval, 1, (long)stride, h, dpk, nullptr, ctl, gd, cap, 0);
    PE_HIP(hipStreamSynchronize(stream_));
    const float* rf = reinterpret_cast<const float*>(ctl + ldc_o_report(cap));
    for (int b = 0; b < batch; ++b) {
      lufs[b] = rf[b];
      scale[b] = rf[ld_o_scale(cap) + b];
      flags[b] = ctl[ldc_o_report(cap) + ld_o_flags(cap) + b];
    }
  } catch (...) {
    hipStreamSynchronize(stream_);
    release();
    throw;
  }
  release();
}

// ------------------------------------------------------------------------------------------------
// timing plan
// ------------------------------------------------------------------------------------------------

// The rules of include/piper_hip.h (pe_timing). Nothing of an engine is read: a refusal changes nothing.
bool Engine::check_timing(const TimingIn& t, const int64_t* offsets, int B) {
  bool all_forced = true;
  for (int b = 0; b < B; ++b) {
    const int64_t T = offsets[b + 1] - offsets[b];
    if (T <= 0) throw std::runtime_error("empty phoneme id sequence");
    if (T > 8192) throw std::runtime_error("phoneme id sequence longer than 8192");
    const std::string utt = "utterance " + std::to_string(b);
    long long sum = 0, nfree = 0;
    for (int64_t i = 0; i < T; ++i) {
      if (t.rate) {
        const float r = t.rate[offsets[b] + i];
        if (!std::isfinite(r) || !(r > 0.f))
          throw std::runtime_error(utt + ", id " + std::to_string(i) + ": rate must be finite and > 0");
      }
      const int32_t f = t.forced ? t.forced[offsets[b] + i] : -1;
      if (f < -1 || f > MAX_FRAMES)
        throw std::runtime_error(utt + ", id " + std::to_string(i) + ": forced duration " + std::to_string(f) + " outside [-1, " +
                                 std::to_string(MAX_FRAMES) + "]");
      if (f >= 0) sum += f; else ++nfree;
    }
    const int32_t N = t.target ? t.target[b] : 0;
    if (N < 0 || N > MAX_FRAMES)
      throw std::runtime_error(utt + ": target_frames " + std::to_string(N) + " outside [0, " + std::to_string(MAX_FRAMES) + "]");
    if (N > 0 && nfree > 0 && (long long)N < sum + nfree)
      throw std::runtime_error(utt + ": target_frames " + std::to_string(N) + " is below the forced durations' sum " +
                               std::to_string(sum) + " plus one frame for each of the " + std::to_string(nfree) + " free ids");
    if (N > 0 && nfree == 0 && (long long)N != sum)
      throw std::runtime_error(utt + ": every id is forced and the durations' sum " + std::to_string(sum) +
                               " differs from target_frames " + std::to_string(N));
    if (N == 0 && nfree == 0 && (sum < 1 || sum > MAX_FRAMES))
      throw std::runtime_error(utt + ": every id is forced and the durations' sum " + std::to_string(sum) + " is outside [1, " +
                               std::to_string(MAX_FRAMES) + "]");
    all_forced = all_forced && nfree == 0;
  }
  return all_forced;
}

// duration_plan_kernel's parameters for the uploaded call on top of duration_kernel's
void Engine::plan_params(PlanP& pp, const DurP& dp) const {
  const size_t Bc = capA_B_;
  pp.d = dp;
  pp.target = d_plan_;
  pp.rate = reinterpret_cast<const float*>(d_plan_ + Bc);
  pp.forced = d_plan_ + Bc + Ts_;
  pp.pl_bs = (long)2 * Ts_;
  pp.w_out = plan_skip_ ? nullptr : plan_w_;
}

void Engine::debug_timing(const float* logw, const int64_t* offsets, int batch, const float* scales, const TimingIn* timing,
                          int32_t* dur_out, int32_t* frames_out, float* w_out) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!logw || !offsets || !scales || !dur_out || !frames_out) throw std::runtime_error("null argument");
  const TimingIn none;
  const TimingIn& t = timing ? *timing : none;
  check_timing(t, offsets, batch);
  int Tmax = 1;
  for (int b = 0; b < batch; ++b) Tmax = std::max(Tmax, (int)(offsets[b + 1] - offsets[b]));
  PE_HIP(hipSetDevice(device_));
  finish_run();
  // one host image, one device block: [lens B | frames B | clamped B | scales 3B | target B | per utterance: logw, rate,
  // forced, dur, cum, w of Ts words each]
  const size_t Ts = (size_t)rup(Tmax, 4), B = (size_t)batch, head = 7 * B, row = 6 * Ts, words = head + B * row;
  std::vector<int> h(words, 0);
  float* hf = reinterpret_cast<float*>(h.data());
  for (size_t b = 0; b < B; ++b) {
    const int T = (int)(offsets[b + 1] - offsets[b]);
    h[b] = T;
    for (int k = 0; k < 3; ++k) hf[3 * B + 3 * b + k] = scales[3 * b + k];
    h[6 * B + b] = t.target ? t.target[b] : 0;
    const size_t r0 = head + b * row;
    for (int i = 0; i < T; ++i) {
      hf[r0 + i] = logw[offsets[b] + i];
      hf[r0 + Ts + i] = t.rate ? t.rate[offsets[b] + i] : 1.0f;
      h[r0 + 2 * Ts + i] = t.forced ? t.forced[offsets[b] + i] : -1;
    }
  }
  int* dv = nullptr;
  PE_HIP(hipMalloc((void**)&dv, words * sizeof(int)));
  try {
    PE_HIP(hipMemcpyAsync(dv, h.data(), words * sizeof(int), hipMemcpyHostToDevice, stream_));
    float* df = reinterpret_cast<float*>(dv);
    PlanP pp{};
    pp.d.z0 = df + head; pp.d.z_bs = (long)row; pp.d.m0 = 0.f; pp.d.es0 = 1.f; pp.d.scales = df + 3 * B;
    pp.d.lens = dv; pp.d.dur = dv + head + 3 * Ts; pp.d.cum = dv + head + 4 * Ts; pp.d.d_bs = (int)row;
    pp.d.frames = dv + B; pp.d.logw_out = nullptr; pp.d.frames_host = nullptr; pp.d.frames_clamped = dv + 2 * B;
    pp.d.frame_cap = MAX_FRAMES + 1;
    pp.target = dv + 6 * B;
    pp.rate = df + head + Ts; pp.forced = dv + head + 2 * Ts; pp.pl_bs = (long)row;
    pp.w_out = df + head + 5 * Ts;
    launch::duration_plan(dim3(batch), stream_, pp);
    PE_HIP(hipMemcpyAsync(h.data(), dv, words * sizeof(int), hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);
    hipFree(dv);
    throw;
  }
  hipFree(dv);
  for (size_t b = 0; b < B; ++b) {
    const int T = (int)(offsets[b + 1] - offsets[b]);
    const size_t r0 = head + b * row;
    frames_out[b] = h[B + b];
    for (int i = 0; i < T; ++i) {
      dur_out[offsets[b] + i] = h[r0 + 3 * Ts + i];
      if (w_out) w_out[offsets[b] + i] = hf[r0 + 5 * Ts + i];
    }
  }
}

const std::vector<int32_t>& Engine::durations_host() {
  EntryLock entry_lock;
  finish_run();
  std::vector<int> tmp((size_t)B_ * Ts_);
  PE_HIP(hipMemcpy(tmp.data(), d_dur_, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
  dur_h_.clear();
  for (int b = 0; b < B_; ++b)
    for (int t = 0; t < tlens_h_[b]; ++t) dur_h_.push_back(tmp[(size_t)b * Ts_ + t]);
  return dur_h_;
}

// Test hook: what randn_kernel draws for (seed_, call, site) -- the generator of the product path when the caller
// injects no noise: draws [row * RNG_PITCH, row * RNG_PITCH + n) of the site's stream (kernels.h: the pipeline's noise
// for column f of logical row r = utterance * channels + channel is draw r * RNG_PITCH + f).
void Engine::debug_randn(int site, uint64_t call, int64_t row, int64_t n, float* out) {
  if (n <= 0 || row < 0 || !out || site < 0 || site > 1) throw std::runtime_error("debug_randn: bad arguments");
  EntryLock entry_lock;
  PE_HIP(hipSetDevice(device_));
  float* d = nullptr;
  unsigned long long* st = nullptr;
  const long rows = (long)((n + RNG_PITCH - 1) / RNG_PITCH);
  const int cols = rows > 1 ? RNG_PITCH : (int)n;
  PE_HIP(hipMalloc((void**)&d, (size_t)rows * cols * sizeof(float)));
  if (hipMalloc((void**)&st, 16) != hipSuccess) { hipFree(d); throw std::runtime_error("debug_randn: out of memory"); }
  const unsigned long long hst[2] = {seed_, call};
  hipMemcpy(st, hst, sizeof(hst), hipMemcpyHostToDevice);
  launch::randn(stream_, d, rows, cols, (long)cols, (long)row, st, site);
  hipStreamSynchronize(stream_);
  hipMemcpy(out, d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(d);
  hipFree(st);
}

// Per-stage tensors for parity debugging (tests only): name in {x_enc, stats (m_p | logs_p), xg, logw, plan_w, z_p, z, noise_w,
// noise_z, audio, pool_z, pool_cond}.
void Engine::debug_tensor(const std::string& name, int b, std::vector<float>& out, int* rows, int* cols) {
  EntryLock entry_lock;
  finish_run();
  PE_HIP(hipStreamSynchronize(stream_));
  const float* src = nullptr;
  int R = 0, Cn = 0;
  long stride = 0;
  if (name == "x_enc") { src = stage_a_enc_out() + (size_t)b * H_ * Ts_; R = H_; Cn = tlens_h_[b]; stride = Ts_; }
  else if (name == "stats") { src = stats_ + (size_t)b * 2 * C_ * Ts_; R = 2 * C_; Cn = tlens_h_[b]; stride = Ts_; }
  else if (name == "xg") { src = xg_ + (size_t)b * H_ * Ts_; R = H_; Cn = tlens_h_[b]; stride = Ts_; }
  else if (name == "logw" && plan_skip_)
    throw std::runtime_error("logw is not available: every id of the call was forced, the duration predictor did not run");
  else if (name == "plan_w") {
    if (!plan_on_) throw std::runtime_error("plan_w is only available after a timed call");
    if (plan_skip_)
      throw std::runtime_error("plan_w is not available: every id of the call was forced, the duration predictor did not run");
    src = plan_w_ + (size_t)b * Ts_; R = 1; Cn = tlens_h_[b]; stride = Ts_;
  }
  else if (name == "logw") { src = logw_ + (size_t)b * Ts_; R = 1; Cn = tlens_h_[b]; stride = Ts_; }
  else if (name == "z") { src = zp_ + (size_t)b * C_ * Fs_; R = C_; Cn = frames_h_[b]; stride = Fs_; }
  else if (name == "z_p") {
    if (!zp_keep_) throw std::runtime_error("z_p is only kept with PIPER_HIP_DEBUG_KEEP=1");
    src = zp_keep_ + (size_t)b * C_ * Fs_; R = C_; Cn = frames_h_[b]; stride = Fs_;
  }
  else if (name == "noise_w") { src = noise_w_ + (size_t)b * 2 * Ts_; R = 2; Cn = tlens_h_[b]; stride = Ts_; }
  else if (name == "noise_z") {
    if (sb_active_) throw std::runtime_error("noise_z is not available during a batch stream (its buffer holds the windows)");
    src = noise_z_ + (size_t)b * C_ * Fs_; R = C_; Cn = frames_h_[b]; stride = Fs_;
  }
  else if (name == "audio") { src = audio_ + (size_t)b * Ss_; R = 1; Cn = frames_h_[b] * hop_; stride = Ss_; }
  else if (name == "pool_z" || name == "pool_cond") {
    // stream pool: the WHOLE resident row of slot b (all Fcap frames, whatever its tenant's length), its conditioning row
    stream_pool_require();
    if (b < 0 || b >= sp_slots_) throw std::runtime_error("stream pool slot outside [0, slots)");
    if (name == "pool_z") { src = sp_z_ + (size_t)b * C_ * sp_fcap_; R = C_; Cn = sp_fcap_; stride = sp_fcap_; }
    else { src = sp_cond_ + (size_t)b * cond_dec_.rows; R = 1; Cn = cond_dec_.rows; stride = cond_dec_.rows; }
  }
  else throw std::runtime_error("unknown debug tensor " + name);
  out.resize((size_t)R * Cn);
  for (int r = 0; r < R; ++r)
    PE_HIP(hipMemcpy(out.data() + (size_t)r * Cn, src + (size_t)r * stride, Cn * sizeof(float), hipMemcpyDeviceToHost));
  *rows = R;
  *cols = Cn;
}

}  // namespace pe

#ifdef PE_STAMPS
// tuning build only (`make stamps`): the kernels live in four launch translation units, each with its own copy of the
// stamp / trace arrays (pe_rt.h PE_TRACE_FETCHER); these two entry points merge them.
extern "C" int pe_trace_fetch_conv(long long*, long long*, unsigned*);
extern "C" int pe_trace_fetch_bf3(long long*, long long*, unsigned*);
extern "C" int pe_trace_fetch_front(long long*, long long*, unsigned*);
extern "C" int pe_trace_fetch_tail(long long*, long long*, unsigned*);
static int pe_trace_merge(long long* stamps, long long* trace, unsigned* count) {
  int (*const fetch[4])(long long*, long long*, unsigned*) = {pe_trace_fetch_conv, pe_trace_fetch_bf3, pe_trace_fetch_front,
                                                               pe_trace_fetch_tail};
  std::vector<long long> st(PE_NSTAMP_K * PE_NSTAMP_I), tr((size_t)PE_NTRACE * 5);
  unsigned total = 0;
  for (auto f : fetch) {
    unsigned n = 0;
    const int rc = f(st.data(), tr.data(), &n);
    if (rc) return rc;
    if (stamps)
      for (size_t i = 0; i < st.size(); ++i)
        if (st[i]) stamps[i] = st[i];
    if (trace)
      for (unsigned r = 0; r < (n < PE_NTRACE ? n : PE_NTRACE) && total < PE_NTRACE; ++r, ++total)
        memcpy(trace + (size_t)total * 5, tr.data() + (size_t)r * 5, 5 * sizeof(long long));
  }
  if (count) *count = total;
  return 0;
}
// phase timestamps of pe_rt.h's PE_STAMP, [PE_NSTAMP_K][PE_NSTAMP_I] 100 MHz ticks
extern "C" int pe_debug_stamps(long long* out) {
  memset(out, 0, sizeof(long long) * PE_NSTAMP_K * PE_NSTAMP_I);
  return pe_trace_merge(out, nullptr, nullptr);
}
// per-launch trace: up to PE_NTRACE records (id, wall in, wall out, clock in, clock out) and their count; resets the counters
extern "C" int pe_debug_trace(long long* out, unsigned* count) { return pe_trace_merge(nullptr, out, count); }
#endif
