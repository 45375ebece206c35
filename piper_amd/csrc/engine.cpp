// Host engine, life cycle and the synthesis call: construction / destruction, the XCD probe, workspaces, upload, the
// hipGraph cache (capture per shape bucket, LRU), run / finish_run with speculative stage-B sizing, download, the timing
// plan, debug_tensor / debug_randn. Streams: engine_stream.cpp; output rate, loudness, true peak, limiter:
// engine_deliver.cpp; weight packing: engine_pack.cpp; launchers: engine_launch.cpp; the kernel sequences:
// engine_issue.cpp; which kernel form a launch takes: policy.h.
#include "engine_internal.h"

#include <array>
#include <numeric>

namespace pe {

thread_local long g_launches = 0;
std::shared_mutex g_capture_mu;
thread_local int g_entry_depth = 0;

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
  // (every side buffer by hand, in this order, while the stream still exists: member destruction is only the net under
  // error paths)
  wsA_.reset(); wsB_.reset();
  h_audio_.reset(); h_pcm_.reset(); h_pcm_zc_.reset(); h_frames_.reset(); h_in_.reset(); h_plan_.reset();
  rows_free(batch_rows_);
  sb_active_ = false;
  stream_pool_free();
  rs_coef_.reset(); raudio_.reset(); rpcm_.reset(); rs_dev_.reset(); rs_host_.reset();
  ld_coef_.reset(); ld_seg_.reset(); ld_dev_.reset(); ld_ctl_.reset(); tp_coef_.reset(); tp_words_.reset();
  lim_h_.reset(); lim_rep_.reset(); lim_host_.reset(); lim_v_.reset(); lim_z_.reset();
  codes_.reset(); h_codes_.reset();
  rs_cap_ = ld_cap_ = lim_cap_ = 0;                    // (the row blocks the capacities spoke of are gone)
  if (ev0_) hipEventDestroy(ev0_);
  if (ev1_) hipEventDestroy(ev1_);
  for (auto& k : kev_) { hipEventDestroy(k.a); hipEventDestroy(k.b); }
  kev_.clear();
  for (hipEvent_t e : ev_pool_) hipEventDestroy(e);
  ev_pool_.clear();
  for (auto& p : side_) p.reset();
  ffn_parts_.reset();
  if (stream_) hipStreamDestroy(stream_);
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
    side_alloc(ffn_parts_, (size_t)(FC_ / 48) * H_ * LaunchPolicy::ffn_max_cols, true, FILL_POISON);
  }
  const int Ts = rup(Tmax, 128);    // row strides are multiples of 128 columns (conv epilogue relies on it)
  auto carve = [&](char* base, size_t Bc, size_t T) -> size_t {
    Carver c(base);
    // input block: [rng 4 x u64 | seed keys Bc x u64, use flags Bc (padded to 16 bytes) | lengths Bc | speaker ids Bc |
    // scales Bc x 3 (padded to 4) | ids Bc x T] (contiguous, copied as one piece by upload())
    // In front of it, in the same allocation, the blend area of a multi-speaker voice (engine.h: in_blend_bytes).
    const size_t ns = in_scale_slots(Bc), head = in_head_bytes(Bc), bl = in_blend_bytes(Bc);
    d_blend_ = c.take<char>(bl + head + (2 * Bc + ns + Bc * T) * sizeof(int));
    d_in_ = base ? d_blend_ + bl : nullptr;
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
    // speaker vectors of a blended call and cond_kernel's row index into them (speaker_blend_kernel)
    g_tab_ = nspk_ > 1 ? c.take<float>(Bc * (size_t)gin_) : nullptr;
    g_rows_ = nspk_ > 1 ? c.take<int>(Bc) : nullptr;
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
      carve(wsA_.get(), capA_B_, capA_T_);                                // (the probes above moved the pointers)
      throw std::runtime_error("call too large: " + std::to_string(B) + " utterances padded to " + std::to_string(Ts) +
                               " ids need " + std::to_string(exact >> 20) + " MiB of text-encoder workspace (budget " +
                               std::to_string(budget >> 20) + " MiB)");
    }
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    wsA_.reset();
    wsB_.reset();                                                         // stage-B pointers sit in the dropped graphs
    capA_B_ = capA_T_ = 0; capB_B_ = capB_F_ = 0;
    try {
      wsA_.grow(carve(nullptr, nB, nT), "text-encoder workspace");
    } catch (const std::runtime_error&) {                                 // (the grown block does not fit: exactly this call)
      nB = B; nT = Ts;
      carve(nullptr, 0, 0);
      wsA_.grow(exact, "text-encoder workspace");
    }
    capA_B_ = nB; capA_T_ = nT;
    if (pol_.debug_poison) poison(wsA_.get(), wsA_.bytes());
    carve(wsA_.get(), capA_B_, capA_T_);
    PE_HIP(hipMemsetAsync(d_in_, 0, 32, stream_));        // generator state: "no upload ingested yet" (embed_kernel)
    h_in_.grow(in_blend_bytes(capA_B_) + in_bytes_);
  }
  Ts_ = (int)capA_T_;
  carve(wsA_.get(), capA_B_, capA_T_);
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
      carve(wsB_.get(), capB_B_, capB_F_);
      throw std::runtime_error("call too large: " + std::to_string(Bnow) + " utterances of up to " + std::to_string(Fs) +
                               " frames need " + std::to_string(exact >> 20) + " MiB of vocoder workspace (budget " +
                               std::to_string(budget >> 20) + " MiB)");
    }
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    wsB_.reset();
    capB_B_ = capB_F_ = 0;
    try {
      wsB_.grow(carve(nullptr, nB, nF), "vocoder workspace");
    } catch (const std::runtime_error&) {                                 // (the grown block does not fit: exactly this call)
      nB = Bnow; nF = Fs; capB_exact_ = true;
      carve(nullptr, 0, 0);
      wsB_.grow(exact, "vocoder workspace");
    }
    capB_B_ = nB; capB_F_ = nF;
    if (pol_.debug_poison) poison(wsB_.get(), wsB_.bytes());
  }
  Fs_ = (int)capB_F_;
  Ss_ = (long)capB_F_ * hop_;
  carve(wsB_.get(), capB_B_, capB_F_);
  const size_t Bc = capB_B_, hmax = hmax_of(capB_F_);
  // zero-copy PCM: room for every utterance of the batch capacity, up to 256 MiB of pinned memory (beyond: copies)
  So_ = rs_on_ ? (long)rup((int)out_samples(Ss_), 4) : Ss_;
  const size_t zc_want = Bc * (size_t)So_;
  if (pol_.pcm_zc && zc_want * sizeof(int16_t) <= ((size_t)256 << 20) && h_pcm_zc_.size() < zc_want) {
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();                                     // the pointer is a kernel argument inside the graphs
    h_pcm_zc_.grow(zc_want);
  }
  // per-resblock buffers of the grouped sibling schedule (one-utterance calls, first generator stage): allocated
  // here, outside any graph capture; the schedule only applies below 700 64x64 blocks per stage
  const size_t want = std::min<size_t>(Bc * hmax, (size_t)(pol_.group_tiled ? LaunchPolicy::group_tiled_max_blocks : LaunchPolicy::group_max_blocks64) * 4096);
  if ((pol_.group_mrf || pol_.group_tiled) && side_floats_ < want) {
    PE_HIP(hipStreamSynchronize(stream_));
    drop_graphs();
    for (auto& sp : side_) sp.reset();
    side_floats_ = 0;                  // (the capacity is published only once EVERY buffer exists: a failed allocation must not
                                       // leave null pointers behind a capacity that says they are there)
    DevBuf<float> fresh[9];
    for (auto& sp : fresh) side_alloc(sp, want, false, FILL_POISON, "per-resblock buffers", want * sizeof(float) * 9);
    for (int i = 0; i < 9; ++i) side_[i] = std::move(fresh[i]);
    side_floats_ = want;
  }
  if (rs_on_) ensure_resample();
  if (ld_on_) ensure_loudness();
  if (fmt_ != G711_S16) ensure_g711();
}

// ------------------------------------------------------------------------------------------------
// the synthesis call
// ------------------------------------------------------------------------------------------------

void Engine::upload(const int64_t* ids, const int64_t* offsets, int B, const float* scales,
                    const int64_t* sids, const NoiseIn* noise, bool per_utt, const TimingIn* timing, const SeedsIn* seeds,
                    const BlendIn* blend) {
  EntryLock entry_lock;
  if (B <= 0 || B > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!scales) throw std::runtime_error("null scales");
  if (seeds && !seeds->seed) throw std::runtime_error("seeds without a seed array (pe_seeds.seed is null)");
  if (blend) check_blend(*blend, B);                                               // (throws before anything changes)
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
  char* const h_in = this->h_in();
  unsigned long long* hr = reinterpret_cast<unsigned long long*>(h_in);
  int* htl = reinterpret_cast<int*>(h_in + in_head_bytes(Bc));
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
      // (an utterance with components or a vector of its own has no speaker id: whatever stands there is not read)
      const int64_t sp = (sids && !(blend && blend->count[b] != 0)) ? sids[b] : 0;
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
    unsigned long long* hk = reinterpret_cast<unsigned long long*>(h_in + 32);
    int* hu = reinterpret_cast<int*>(h_in + 32 + 8 * Bc);
    for (int b = 0; b < B; ++b) {
      hk[b] = (unsigned long long)seeds->seed[b];
      hu[b] = (!seeds->use || seeds->use[b]) ? 1 : 0;
    }
  }
  // speaker blends: counts, components in fixed rows of BLEND_MAX, vectors, in the area in front of the block
  blended_ = blend != nullptr;
  const size_t bl = in_blend_bytes(Bc);
  if (blended_) {
    char* const area = h_in - bl;
    int* hc = reinterpret_cast<int*>(area);
    int* hs = hc + Bc;
    float* hw = reinterpret_cast<float*>(hs + Bc * BLEND_MAX);
    float* hv = hw + Bc * BLEND_MAX;
    size_t at = 0;
    for (int b = 0; b < B; ++b) {
      const int n = blend->count[b];
      hc[b] = n;
      for (int k = 0; k < BLEND_MAX; ++k) {
        hs[(size_t)b * BLEND_MAX + k] = k < n ? (int)blend->sid[at + k] : 0;
        hw[(size_t)b * BLEND_MAX + k] = k < n ? blend->weight[at + k] : 0.f;
      }
      if (n > 0) at += (size_t)n;
      if (n < 0) memcpy(hv + (size_t)b * gin_, blend->vector + (size_t)b * gin_, (size_t)gin_ * sizeof(float));
    }
  }
  ids_zc_ = pol_.ids_from_host((long)B * Ts);
  if (!ids_zc_) {
    const size_t bytes = in_head_bytes(Bc) + (2 * Bc + in_scale_slots(Bc) + (size_t)B * Ts) * sizeof(int);
    if (blended_) PE_HIP(hipMemcpyAsync(d_blend_, h_in - bl, bl + bytes, hipMemcpyHostToDevice, stream_));
    else PE_HIP(hipMemcpyAsync(d_in_, h_in, bytes, hipMemcpyHostToDevice, stream_));
  }
  plan_on_ = timing != nullptr;
  plan_skip_ = all_forced;
  if (timing) {
    // the plan block through its own pinned staging block (the previous timed call's copy ended with that call's final
    // synchronisation; an abandoned upload is waited for before its block is overwritten or freed)
    const size_t words = plan_words(Bc, (size_t)Ts);
    PE_HIP(hipStreamSynchronize(stream_));
    h_plan_.grow(words);
    int* const hp = h_plan_.get();
    for (int b = 0; b < B; ++b) {
      const int T = tlens_h_[b];
      hp[b] = timing->target ? timing->target[b] : 0;
      float* hr_ = reinterpret_cast<float*>(hp + Bc + (size_t)b * 2 * Ts);
      int* hf = hp + Bc + (size_t)b * 2 * Ts + Ts;
      for (int t = 0; t < T; ++t) {
        hr_[t] = timing->rate ? timing->rate[offsets[b] + t] : 1.0f;
        hf[t] = timing->forced ? timing->forced[offsets[b] + t] : -1;
      }
    }
    PE_HIP(hipMemcpyAsync(d_plan_, hp, (Bc + (size_t)B * 2 * Ts) * sizeof(int), hipMemcpyHostToDevice, stream_));
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
    snprintf(key, sizeof(key), "C|%d|%d|%d|%d|%d|%d%s%s%s%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, Fg_, loud_key(), fmt_key(), seed_key(), blend_key());
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
    (void)fmt_key();                           // (no key here: the run's format is noted all the same)
    issue_stage_b();                           // host-injected noise (tests): not graph-captured
    run_launches_ += g_launches - l0;
  } else {
    snprintf(key, sizeof(key), "B|%d|%d|%d|%d%s%s%s", B, Fg_, Fs_, Ts_, loud_key(), fmt_key(), seed_key());
    run_stage('B', key);
  }
}

// The key of stage A's graph. An untimed call's is what it always was; a timed call's carries the plan's two flags -- a
// plan is present, the duration predictor is left out -- and nothing of the plan's values.
std::string Engine::stage_a_key(int B) const {
  char key[200];
  if (plan_on_) snprintf(key, sizeof(key), "A|%d|%d|%d|%d|%d|p%d%s%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, (int)plan_skip_, seed_key(), blend_key());
  else snprintf(key, sizeof(key), "A|%d|%d|%d|%d|%d%s%s", B, Tg_, Ts_, (int)have_noise_w_, Fs_, seed_key(), blend_key());
  return key;
}

// Host view of the frame counts stage A produced (the stream is synchronised): frames, sample offsets, the ratio the
// next run's guess is made from.
void Engine::finish_stage_b_sizes() {
  const int B = B_;
#ifdef PE_EMU
  if (const char* pf = getenv("EMU_PLAN_FRAMES"))      // emulator plan-only mode (tests/emu): frames are not computed
    for (int b = 0; b < B; ++b) h_frames_.get()[b] = atoi(pf);
#endif
  frames_h_.assign(h_frames_.get(), h_frames_.get() + B);
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
  snprintf(key, sizeof(key), "B|%d|%d|%d|%d%s%s%s", B_, Fg_, Fs_, Ts_, loud_key(), fmt_key(), seed_key());
  run_stage('B', key);
  return false;
}

void Engine::download(bool want_audio, bool want_pcm) {
  EntryLock entry_lock;
  auto grow = [&](size_t total) {
    if (want_audio) grow_pinned(h_audio_, total);
    if (want_pcm) grow_pinned(h_pcm_, total);
  };
  // pcm16_kernel already wrote the samples into pinned host memory (zero-copy), packed back to back: nothing to enqueue
  const bool zc = pol_.pcm_zc && h_pcm_zc_ && h_pcm_zc_.size() >= (size_t)B_ * (size_t)So_;
  // what is delivered: the generator's waveform, or its resampling (row stride So_; Ss_ at the native rate)
  // (read where a copy is enqueued, not here: a missed guess re-sizes the workspace, and the buffers move with it)
  auto asrc = [&]() -> const float* { return rs_on_ ? raudio_.get() : audio_; };
  auto psrc = [&]() -> const int16_t* { return rs_on_ ? rpcm_.get() : pcm_; };
  // the G.711 codes of a run with a format: packed on the device by g711_kernel, one copy of the call's total
  const int fmt = run_fmt_;
  auto codes = [&](size_t n) {
    if (fmt == G711_S16 || !codes_) return;
    grow_pinned(h_codes_, std::max<size_t>(n, 1));
    n = std::min(n, codes_.size());
    if (n > 0) PE_HIP(hipMemcpyAsync(h_codes_.get(), codes_.get(), n, hipMemcpyDeviceToHost, stream_));
  };
  lc_rows_ = 0;
  pcm_zc_live_ = false;
  if (spec_pending_ && B_ == 1 && (want_audio || want_pcm || fmt != G711_S16)) {
    // one utterance, speculative run: the copies are enqueued for the guessed length (>= the real one when the guess
    // holds) behind stage B, so that one synchronisation ends the whole call; the host view is trimmed afterwards
    const size_t n = (size_t)out_samples((int64_t)spec_fg_ * hop_);
    grow(n);
    if (want_audio) PE_HIP(hipMemcpyAsync(h_audio_.get(), asrc(), n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (want_pcm && !zc) PE_HIP(hipMemcpyAsync(h_pcm_.get(), psrc(), n * sizeof(int16_t), hipMemcpyDeviceToHost, stream_));
    codes(n);
    lim_enqueue_report();
    if (finish_run()) {                        // synchronises; sample_off_ now holds the real length
      pcm_zc_live_ = zc;
      lc_rows_ = fmt != G711_S16 ? B_ : 0;
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
      PE_HIP(hipMemcpyAsync(h_audio_.get() + sample_off_[b], asrc() + (size_t)b * So_,
                            (size_t)(sample_off_[b + 1] - sample_off_[b]) * sizeof(float), hipMemcpyDeviceToHost,
                            stream_));
  if (want_pcm && !zc)
    for (int b = 0; b < B_; ++b)
      PE_HIP(hipMemcpyAsync(h_pcm_.get() + sample_off_[b], psrc() + (size_t)b * So_,
                            (size_t)(sample_off_[b + 1] - sample_off_[b]) * sizeof(int16_t), hipMemcpyDeviceToHost,
                            stream_));
  codes(total);
  lim_enqueue_report();
  PE_HIP(hipStreamSynchronize(stream_));
  pcm_zc_live_ = zc;
  lc_rows_ = fmt != G711_S16 ? B_ : 0;
  loud_collect();
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
  DevBuf<int> dbuf;
  dbuf.grow(words);
  int* const dv = dbuf.get();
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
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
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

// ---- speaker blends

void Engine::check_blend(const BlendIn& blend, int B) const {
  if (nspk_ <= 1) throw std::runtime_error("speaker blend on a single-speaker voice");
  if (!blend.count) throw std::runtime_error("blend without a count array (pe_blend.count is null)");
  size_t at = 0;
  for (int b = 0; b < B; ++b) {
    const int n = blend.count[b];
    const std::string utt = "utterance " + std::to_string(b);
    if (n < -1 || n > BLEND_MAX)
      throw std::runtime_error(utt + ": blend count " + std::to_string(n) + " outside [-1, " + std::to_string(BLEND_MAX) + "]");
    if (n < 0) {
      if (!blend.vector) throw std::runtime_error(utt + ": count -1 without speaker vectors (pe_blend.vector is null)");
      for (int i = 0; i < gin_; ++i)
        if (!std::isfinite(blend.vector[(size_t)b * gin_ + i]))
          throw std::runtime_error(utt + ": speaker vector element " + std::to_string(i) + " is not finite");
    }
    if (n > 0) {
      if (!blend.sid || !blend.weight)
        throw std::runtime_error(utt + ": " + std::to_string(n) + " blend components without " +
                                 (blend.sid ? "weights (pe_blend.weight is null)" : "ids (pe_blend.sid is null)"));
      for (int k = 0; k < n; ++k) {
        const int64_t s = blend.sid[at + k];
        if (s < 0 || s >= nspk_)
          throw std::runtime_error(utt + ", blend component " + std::to_string(k) + ": speaker id " + std::to_string(s) +
                                   " outside [0, num_speakers)");
        if (!std::isfinite(blend.weight[at + k]))
          throw std::runtime_error(utt + ", blend component " + std::to_string(k) + ": weight is not finite");
      }
      at += (size_t)n;
    }
  }
}

// speaker_blend_kernel's arguments for a blend area at `area` (host or device) laid out for capacity Bc
BlendP Engine::blend_params(const char* area, size_t Bc) const {
  BlendP p{};
  p.emb_g = emb_g_; p.gin = gin_; p.sids = d_sids_;
  p.count = reinterpret_cast<const int*>(area);
  p.csid = p.count + Bc;
  p.cw = reinterpret_cast<const float*>(p.csid + Bc * BLEND_MAX);
  p.vec = p.cw + Bc * BLEND_MAX;
  p.g = g_tab_; p.rows = g_rows_;
  return p;
}

void Engine::speaker_embedding(int64_t sid, float* out, int64_t capacity) {
  EntryLock entry_lock;
  if (nspk_ <= 1) throw std::runtime_error("speaker embedding of a single-speaker voice");
  if (sid < 0 || sid >= nspk_) throw std::runtime_error("speaker id outside [0, num_speakers)");
  if (!out || capacity < gin_) throw std::runtime_error("speaker embedding: output holds fewer than gin values");
  PE_HIP(hipSetDevice(device_));
  PE_HIP(hipMemcpy(out, emb_g_ + (size_t)sid * gin_, (size_t)gin_ * sizeof(float), hipMemcpyDeviceToHost));
}

void Engine::debug_blend(const BlendIn& blend, int batch, const int64_t* sids, float* out) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!out) throw std::runtime_error("null argument");
  check_blend(blend, batch);
  for (int b = 0; b < batch; ++b)
    if (blend.count[b] == 0 && sids && (sids[b] < 0 || sids[b] >= nspk_))
      throw std::runtime_error("utterance " + std::to_string(b) + ": speaker id outside [0, num_speakers)");
  PE_HIP(hipSetDevice(device_));
  finish_run();
  // one host image, one device block: [sids B | count B | component ids 8 B | weights 8 B | vectors B x gin | g B x gin]
  const size_t B = (size_t)batch, G = (size_t)gin_, words = B * (18 + 2 * G);
  std::vector<int> h(words, 0);
  float* hf = reinterpret_cast<float*>(h.data());
  size_t at = 0;
  for (size_t b = 0; b < B; ++b) {
    const int n = blend.count[b];
    h[b] = (n == 0 && sids) ? (int)sids[b] : 0;
    h[B + b] = n;
    for (int k = 0; k < n; ++k) {
      h[2 * B + b * BLEND_MAX + k] = (int)blend.sid[at + k];
      hf[10 * B + b * BLEND_MAX + k] = blend.weight[at + k];
    }
    if (n > 0) at += (size_t)n;
    if (n < 0) memcpy(hf + 18 * B + b * G, blend.vector + b * G, G * sizeof(float));
  }
  DevBuf<int> dbuf;
  dbuf.grow(words);
  int* const dv = dbuf.get();
  try {
    PE_HIP(hipMemcpyAsync(dv, h.data(), words * sizeof(int), hipMemcpyHostToDevice, stream_));
    BlendP p = blend_params(reinterpret_cast<const char*>(dv + B), B);
    p.sids = dv;
    p.g = reinterpret_cast<float*>(dv) + B * (18 + G);
    p.rows = nullptr;
    launch::speaker_blend(stream_, batch, p);
    PE_HIP(hipMemcpyAsync(out, p.g, B * G * sizeof(float), hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
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
  DevBuf<float> d;
  DevBuf<unsigned long long> st;
  const long rows = (long)((n + RNG_PITCH - 1) / RNG_PITCH);
  const int cols = rows > 1 ? RNG_PITCH : (int)n;
  d.grow((size_t)rows * cols);
  st.grow(2);
  const unsigned long long hst[2] = {seed_, call};
  hipMemcpy(st.get(), hst, sizeof(hst), hipMemcpyHostToDevice);
  launch::randn(stream_, d.get(), rows, cols, (long)cols, (long)row, st.get(), site);
  hipStreamSynchronize(stream_);
  hipMemcpy(out, d.get(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
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
  else if (name == "g") {
    // the speaker vector utterance b used: its row of the blended call's table, else the table row of its id
    if (nspk_ <= 1) throw std::runtime_error("g is only available for a multi-speaker voice");
    if (b < 0 || b >= B_) throw std::runtime_error("utterance outside [0, batch)");
    if (blended_) src = g_tab_ + (size_t)b * gin_;
    else {
      int sid = 0;
      PE_HIP(hipMemcpy(&sid, d_sids_ + b, sizeof(int), hipMemcpyDeviceToHost));
      src = emb_g_ + (size_t)sid * gin_;
    }
    R = 1; Cn = gin_; stride = gin_;
  }
  else if (name == "audio") { src = audio_ + (size_t)b * Ss_; R = 1; Cn = frames_h_[b] * hop_; stride = Ss_; }
  else if (name == "pool_z" || name == "pool_cond") {
    // stream pool: the WHOLE resident row of slot b (all Fcap frames, whatever its tenant's length), its conditioning row
    stream_pool_require();
    if (b < 0 || b >= sp_slots_) throw std::runtime_error("stream pool slot outside [0, slots)");
    if (name == "pool_z") { src = sp_z_.get() + (size_t)b * C_ * sp_fcap_; R = C_; Cn = sp_fcap_; stride = sp_fcap_; }
    else { src = sp_cond_.get() + (size_t)b * cond_dec_.rows; R = 1; Cn = cond_dec_.rows; stride = cond_dec_.rows; }
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
