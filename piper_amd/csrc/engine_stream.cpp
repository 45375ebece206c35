// Host engine, streaming: the one-utterance stream, the batch stream in lock step, the stream pool and the stream-wide
// gain. The window stages' kernel sequences: engine_issue.cpp; life cycle, workspaces and whole-utterance calls: engine.cpp.
#include "engine_internal.h"
#include "kernels/stream_loudness_rule.h"
#include "kernels/stream_limiter_rule.h"
#include "kernels/g711_law.h"

namespace pe {

// One sample through the K-weighting cascade in f64, as loud_step (kernels/loudness.h): the one-utterance stream's filter.
static inline double host_loud_step(const double (&c)[10], double x, double (&z)[4]) {
  const double ya = std::fma(c[0], x, z[0]);
  z[0] = std::fma(-c[3], ya, std::fma(c[1], x, z[1]));
  z[1] = std::fma(-c[4], ya, c[2] * x);
  const double yb = std::fma(c[5], ya, z[2]);
  z[2] = std::fma(-c[8], yb, std::fma(c[6], ya, z[3]));
  z[3] = std::fma(-c[9], yb, c[7] * ya);
  return yb;
}

// The gated loudness of a prefix of N samples from its segment sums, serial in f64.
static bool host_gated_loudness(const std::vector<double>& s, int64_t N, int h, bool& is_short, double& L) {
  is_short = N < 4 * (int64_t)h;
  L = 0.0;
  if (N <= 0) return false;
  if (is_short) {
    double sum = 0.0;
    for (double v : s) sum += v;
    L = -0.691 + 10.0 * std::log10(sum / (double)N);
    return L > -70.0;
  }
  const int nb = (int)(N / h) - 3;
  const double inv = 1.0 / (4.0 * (double)h);
  double gate = -70.0;
  bool ok = false;
  for (int pass = 0; pass < 2; ++pass) {
    double tot = 0.0;
    int ct = 0;
    for (int j = 0; j < nb; ++j) {
      const double zj = (((s[j] + s[j + 1]) + s[j + 2]) + s[j + 3]) * inv;
      const double lj = -0.691 + 10.0 * std::log10(zj);
      if (lj > -70.0 && lj > gate) { tot += zj; ++ct; }
    }
    ok = ct > 0;
    if (!ok) return false;
    L = -0.691 + 10.0 * std::log10(tot / (double)ct);
    gate = L - 10.0;
  }
  return ok;
}

int Engine::stream_begin(const int64_t* ids, int64_t n, const float scales[3], int64_t sid, const NoiseIn* noise,
                         const TimingIn* timing, const SeedsIn* seeds, const BlendIn* blend) {
  EntryLock entry_lock;
  const int64_t offs[2] = {0, n};
  const int64_t sids[1] = {sid < 0 ? 0 : sid};
  upload(ids, offs, 1, scales, sids, noise, false, timing, seeds, blend);
  PE_HIP(hipSetDevice(device_));
  spec_pending_ = false;
  stream_front(1, 0);
  s_frames_ = Fmax_;
  s_pos_ = 0;
  s_active_ = true;
  s_gain_r_ = std::max(0.01f, gain_peak_);
  s_gain_first_ = true;
  if (gain_mode_ == GAIN_LOUDNESS) {                   // the stream's loudness state starts from nothing
    HostLoud fresh;
    loudness_filter(output_rate(), fresh.coef);
    fresh.h = (output_rate() + 5) / 10;
    fresh.z[0] = fresh.z[1] = fresh.z[2] = fresh.z[3] = 0.0;
    fresh.lu = std::numeric_limits<float>::quiet_NaN();
    fresh.L = -std::numeric_limits<float>::infinity();
    fresh.flags = LOUD_SHORT | LOUD_UNMEASURABLE;
    if (slim_on_) {                                      // the limiter's window at the delivered rate, rounded as the device table
      std::vector<double> exact;
      limiter_window(output_rate(), slim_ms_, fresh.W, exact);
      fresh.hw.assign(exact.size(), 0.f);
      to_f32(exact, fresh.hw.data());
    }
    s_sl_ = std::move(fresh);
  }
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
      if (gain_mode_ == GAIN_LOUDNESS) {                 // the stream's end state
        lg_gain_[0] = s_sl_.first ? 0.f : s_sl_.G; lg_peak_[0] = s_sl_.r;
        lsl_n_ = 1; lsl_lufs_.assign(1, s_sl_.L); lsl_flags_.assign(1, s_sl_.flags);
      }
    }
    s_active_ = false;
    lc_s_rows_ = 0; lc_s_codes_ = nullptr; lc_s_off_ = nullptr;
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
  grow_pinned(h_audio_, n);
  float* const ha = h_audio_.get();
  PE_HIP(hipMemcpyAsync(ha, rs_on_ ? raudio_.get() : audio_ + (size_t)(f0 - a) * hop_, n * sizeof(float), hipMemcpyDeviceToHost,
                        stream_));
  PE_HIP(hipStreamSynchronize(stream_));
  // per-chunk peak normalisation, as the reference's streaming script does (infer_onnx_streaming.py:122) -- or one of the
  // stream-wide levels, in the f32 arithmetic of stream_gain_kernel and chunk_pcm_gain_kernel (kernels/post.h)
  float peak = 0.01f;
  for (size_t i = 0; i < n; ++i) peak = std::max(peak, std::fabs(ha[i]));
  float g0 = 32767.0f / peak, sc = g0, level = peak;
  size_t R = 0;
  const bool lim = slim_active() && s_sl_.W > 0;
  lsm_n_ = 0;
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
  } else if (gain_mode_ == GAIN_LOUDNESS && n > 0) {
    // the rule of stream_loudness_gain_kernel on an f64 serial filter that runs through the chunks
    HostLoud& q = s_sl_;
    float c = 0.f;
    for (size_t i = 0; i < n; ++i) {
      c = std::max(c, std::fabs(ha[i]));
      const double y = host_loud_step(q.coef, (double)ha[i], q.z);
      const size_t j = (size_t)((q.N + (int64_t)i) / q.h);
      if (j >= q.seg.size()) q.seg.resize(j + 1, 0.0);
      q.seg[j] = std::fma(y, y, q.seg[j]);
    }
    q.N += (int64_t)n;
    bool is_short;
    double L;
    const bool ok = host_gated_loudness(q.seg, q.N, q.h, is_short, L);
    const float rp = std::max(q.r, c);
    const SlRule o = sl_rule(ok, is_short, L, sl_T_, (float)std::pow(10.0, (double)sl_cdb_ / 20.0), sl_prior_, rp, q.G, q.first, q.lu, lim);
    g0 = o.g0; sc = o.g1; level = rp;
    R = std::min<size_t>((size_t)gain_ramp_, n);
    q.r = rp; q.G = o.g1; q.first = false;
    q.L = ok ? (float)L : -std::numeric_limits<float>::infinity();
    q.flags = o.flags;
    lsl_n_ = 1; lsl_lufs_.assign(1, q.L); lsl_flags_.assign(1, q.flags);
  }
  const float dg = g0 - sc, Rf = (float)std::max<size_t>(R, 1);
  const float* fout = ha;
  size_t nout = n;
  if (lim) {
    // the look-ahead limiter (the arithmetic of kernels/stream_limiter_rule.h): the chunk joins the held-back
    // samples, and the stream is handed out up to D = 2 W short of its end -- to its end with the last frame
    HostLoud& q = s_sl_;
    const int W = q.W, D = 2 * W;
    const float C = (float)std::pow(10.0, (double)sl_cdb_ / 20.0), cq = (float)std::floor(32767.0 * (double)C);
    for (size_t i = 0; i < n; ++i) {
      q.hx.push_back(ha[i]);
      q.hs.push_back(slm_scale_at(sc, dg, (int)R, Rf, (int)i));
    }
    const int64_t base = q.N - (int64_t)q.hx.size(), b0 = q.B, b1 = slm_delivered(q.N, D, f1 >= s_frames_);
    nout = (size_t)(b1 - b0);
    std::vector<float> rr(nout + 4 * (size_t)W, 1.0f), d(nout + 2 * (size_t)W), e(nout);
    for (size_t k = 0; k < rr.size(); ++k) {
      const int64_t i = b0 - 2 * W + (int64_t)k;
      if (i >= 0 && i >= base && i < q.N) rr[k] = slm_r(q.hx[(size_t)(i - base)], q.hs[(size_t)(i - base)], C);
    }
    slm_host_env(rr.data(), (int)nout, W, q.hw.data(), d.data(), e.data());
    s_pcm_.resize(nout);
    s_pcm_f_.resize(nout);
    float red = 0.f;
    int shaped = 0;
    for (size_t k = 0; k < nout; ++k) {
      const size_t j = (size_t)(b0 + (int64_t)k - base);
      s_pcm_f_[k] = q.hx[j];
      s_pcm_[k] = slm_pcm(q.hx[j], e[k], q.hs[j], cq);
      red = std::max(red, 1.0f - e[k]);
      shaped += e[k] < 1.0f ? 1 : 0;
    }
    q.B = b1;
    const size_t keep = std::min(q.hx.size(), (size_t)4 * W);
    q.hx.erase(q.hx.begin(), q.hx.end() - (long)keep);
    q.hs.erase(q.hs.begin(), q.hs.end() - (long)keep);
    fout = s_pcm_f_.data();
    lsm_n_ = 1; lsm_maxred_.assign(1, red); lsm_shaped_.assign(1, shaped);
  } else {
    s_pcm_.resize(n);
    for (size_t i = 0; i < n; ++i) {
      const float g = i < R ? std::fmaf(dg, (float)(int)(R - 1 - i) / Rf, sc) : sc;
      float v = ha[i] * g;
      v = std::min(std::max(v, -32768.0f), 32767.0f);
      s_pcm_[i] = (int16_t)v;
    }
  }
  // sample format: the host twin of the encoder on what this call hands out
  lc_s_rows_ = 0; lc_s_codes_ = nullptr; lc_s_off_ = nullptr;
  if (fmt_ != G711_S16) {
    s_codes_.resize(std::max<size_t>(nout, 1));
    for (size_t i = 0; i < nout; ++i) s_codes_[i] = (uint8_t)g711_code(fmt_, s_pcm_[i]);
    s_codes_off_[0] = 0; s_codes_off_[1] = (int64_t)nout;
    lc_s_rows_ = 1; lc_s_codes_ = s_codes_.data(); lc_s_off_ = s_codes_off_;
  }
  lg_n_ = 1; lg_dev_peaks_ = nullptr; lg_lazy_ = false;
  lg_gain_.assign(1, sc);
  lg_peak_.assign(1, level);
  s_pos_ = f1;
  if (audio) *audio = fout;
  if (pcm) *pcm = s_pcm_.data();
  if (nsamples) *nsamples = (int64_t)nout;
  return true;
}

// ------------------------------------------------------------------------------------------------
// batch streaming
// ------------------------------------------------------------------------------------------------

void Engine::rows_free(ChunkRows& r) {
  r.host.reset(); r.dev.reset(); r.pcm.reset(); r.audio.reset(); r.gctl.reset(); r.gdev.reset();
  r.pcm_dev.reset(); r.codes_dev.reset(); r.codes.reset();
  lc_s_rows_ = 0; lc_s_codes_ = nullptr; lc_s_off_ = nullptr;      // (a chunk's codes not yet read pointed into r.codes)
  r.lctl.reset(); r.ldev.reset(); r.lseg.reset(); r.ltail.reset();
  r.lnseg = r.lW = 0;
  r.mctl.reset(); r.mreph.reset(); r.mrep.reset(); r.mstail.reset();
  lg_dev_peaks_ = nullptr;                               // (a default-mode report not yet fetched pointed into r.dev)
  r.cap = 0;
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
  side_alloc(r.host, (size_t)sb_words(want), false, FILL_ZERO);
  side_alloc(r.dev, (size_t)sb_words(want), false, FILL_ZERO);
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
                                                       const SeedsIn* seeds, const BlendIn* blend) {
  EntryLock entry_lock;
  upload(ids, offsets, B, scales, sids, noise, true, timing, seeds, blend);
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
  int* st = r.host.get();
  long long* off = reinterpret_cast<long long*>(st + sb_o_off(cap));
  int wmax = 1, cmax = 1;
  int64_t total = 0;
  // the look-ahead limiter: a row hands out its stream up to D = 2 W short of what exists, everything with
  // the chunk that consumes its last frame; the chunk counts go to `coff`, the delivered ones to the offsets
  const bool lim = slim_active();
  const int D = lim ? 2 * limiter_window_samples(output_rate(), slim_ms_) : 0;
  bool any = false;
  std::vector<int64_t> coff((size_t)n + 1, 0), Nk, Bk;
  if (lim) {
    if (!r.gctl) gain_blocks_alloc(r, cap);
    if ((int)r.gfirst.size() < n) r.gfirst.assign(n, 1);
    sl_ensure(r, cap, out_samples((int64_t)clamp * hop_));
    slim_ensure(r, cap);
    if ((int)r.mN.size() < n) { r.mN.assign(n, 0); r.mB.assign(n, 0); }
    Nk.assign(r.mN.begin(), r.mN.begin() + n);
    Bk.assign(r.mB.begin(), r.mB.begin() + n);
  }
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
      any = true;
    }
    coff[b + 1] = coff[b] + ocount;
    int64_t dcount = ocount;
    if (lim) {
      int* m = r.mctl.get();
      const int64_t N0 = r.gfirst[b] ? 0 : r.mN[b], B0 = r.gfirst[b] ? 0 : r.mB[b];
      dcount = 0;
      if (ocount > 0) {
        Nk[b] = N0 + ocount;
        Bk[b] = slm_delivered(Nk[b], D, f0 + c >= F);
        dcount = Bk[b] - B0;
      }
      m[b] = (int)std::min<int64_t>(N0, 0x7fffffff);
      m[slm_o_b0(cap) + b] = (int)std::min<int64_t>(B0, 0x7fffffff);
      m[slm_o_cnt(cap) + b] = (int)dcount;
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
    total += dcount;
    wmax = std::max(wmax, e - a);
  }
  r.off[n] = total;
  out.batch = n;
  out.sample_offsets = r.off.data();
  out.frames_done = r.pos.data();
  out.pcm = r.pcm.get();
  out.audio = nullptr;
  lsm_n_ = 0;
  // sample format: the chunk's codes follow what is delivered, under the same offsets (a call that runs nothing: none)
  const bool law = fmt_ != G711_S16;
  lc_s_rows_ = law ? n : 0;
  lc_s_off_ = law ? r.off.data() : nullptr;
  lc_s_codes_ = nullptr;
  if (!any) {                                          // no row has frames left (a call may deliver nothing while rows go on)
    gain_report_idle(r.gctl.get(), cap, n);
    if (gain_mode_ == GAIN_LOUDNESS) sl_collect(r, n, false);
    if (lim) { lsm_n_ = n; lsm_maxred_.assign(n, 0.f); lsm_shaped_.assign(n, 0); }
    return false;
  }
  grow_pinned(r.pcm, (size_t)std::max<int64_t>(total, 1));
  if (want_audio) grow_pinned(r.audio, (size_t)std::max<int64_t>(total, 1));
  if (law) {
    // the stage's int16 go to a device staging buffer of the packed layout, which the encoder reads behind the stage; the
    // buffers' addresses are data of the pinned block, not part of a graph, and the previous chunk has been waited for
    const size_t want = ((size_t)std::max<int64_t>(total, 1) + 15) & ~(size_t)15;
    if (!r.pcm_dev || !r.codes_dev || r.pcm_dev.size() < want || r.codes_dev.size() < want) {
      r.pcm_dev.reset(); r.codes_dev.reset();
      side_alloc(r.pcm_dev, want + want / 2, false, FILL_POISON, "stream chunk staging");
      side_alloc(r.codes_dev, want + want / 2, false, FILL_POISON, "stream chunk codes");
    }
    grow_pinned(r.codes, want);
    lc_s_codes_ = r.codes.get();
  }
  void* ptrs[2] = {law ? (void*)r.pcm_dev.get() : (void*)r.pcm.get(), want_audio ? r.audio.get() : nullptr};
  memcpy(st + sb_o_ptrs(cap), ptrs, sizeof(ptrs));
  // the window bucket: by the largest step among the rows that deliver
  r.wg = std::min(rup(cmax + 2 * hf, 32), Fs_);
  if (r.wg < wmax) r.wg = std::min(rup(wmax, 32), Fs_);
  char key[96];
  if (gain_mode_ == GAIN_CHUNK) {
    snprintf(key, sizeof(key), "%c|%d|%d|%d", r.stage, n, r.wg, Fs_);
  } else {
    if (!r.gctl) gain_blocks_alloc(r, cap);            // (the batch stream's: the pool's exist since open)
    if ((int)r.gfirst.size() < n) r.gfirst.assign(n, 1);
    if (gain_mode_ == GAIN_LOUDNESS) {
      sl_ensure(r, cap, out_samples((int64_t)clamp * hop_));
      sl_prepare(r, n);
    } else {
      gain_prepare(r.gctl.get(), cap, r.gfirst, n);
    }
    if (lim) snprintf(key, sizeof(key), "%c|%d|%d|%d|g3l%d", r.stage, n, r.wg, Fs_, slim_W_);
    else snprintf(key, sizeof(key), "%c|%d|%d|%d|g%d", r.stage, n, r.wg, Fs_, gain_mode_);
  }
  run_stage(r.stage, key);
  if (law) {
    // the same int16 bytes as without a format, through the staging buffer; then the flat encoder on the `total` delivered
    const long l0 = g_launches;
    if (total > 0) PE_HIP(hipMemcpyAsync(r.pcm.get(), r.pcm_dev.get(), (size_t)total * sizeof(int16_t), hipMemcpyDeviceToHost, stream_));
    PE_LAUNCH_KB("g711_kernel", 3.0 * (double)total, launch::g711_flat(stream_, r.pcm_dev.get(), (long)total, r.codes_dev.get(), fmt_));
    run_launches_ += g_launches - l0;
    if (total > 0) PE_HIP(hipMemcpyAsync(r.codes.get(), r.codes_dev.get(), (size_t)total, hipMemcpyDeviceToHost, stream_));
  }
  if (lim) PE_HIP(hipMemcpyAsync(r.mreph.get(), r.mrep.get(), (size_t)slm_rep_words(cap) * sizeof(int), hipMemcpyDeviceToHost, stream_));
  PE_HIP(hipStreamSynchronize(stream_));
  // (which rows moved their state is decided by the chunks, not by what was handed out)
  gain_collect(r.gctl.get(), cap, n, r.gfirst, coff.data(),
               rs_on_ ? rs_peaks() : reinterpret_cast<const unsigned*>(r.dev.get()) + sb_o_peak(cap));
  if (gain_mode_ == GAIN_LOUDNESS) sl_collect(r, n, true);
  if (lim) {
    lsm_n_ = n;
    lsm_maxred_.assign(n, 0.f);
    lsm_shaped_.assign(n, 0);
    const int* w = r.mreph.get();
    for (int b = 0; b < n; ++b) {
      if (r.off[b + 1] > r.off[b]) {
        memcpy(&lsm_maxred_[b], w + lim_o_maxred(cap) + b, sizeof(float));
        lsm_shaped_[b] = w[lim_o_count(cap) + b];
      }
      r.mN[b] = Nk[b];
      r.mB[b] = Bk[b];
    }
  }
  for (int b = 0; b < n; ++b) r.pos[b] += st[sb_o_count(cap) + b] / hop_;
  out.pcm = r.pcm.get();
  out.audio = want_audio ? r.audio.get() : nullptr;
  return true;
}

// ------------------------------------------------------------------------------------------------
// stream pool
// ------------------------------------------------------------------------------------------------

void Engine::stream_pool_require() const {
  if (!sp_slots_) throw std::runtime_error("no stream pool open on this handle (pe_stream_pool_open)");
}

void Engine::stream_pool_free() {
  sp_z_.reset(); sp_cond_.reset(); sp_join_.reset();
  rows_free(pool_rows_);
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
  // everything is built beside the pool and moved in once it is complete: a failure leaves the pool exactly as it was
  DevBuf<float> z, cond;
  PinBuf<int> join;
  ChunkRows r{'P'};
  side_alloc(z, (size_t)slots * C_ * fcap, false, FILL_ZERO, "stream pool latents");
  side_alloc(cond, (size_t)slots * std::max(cond_dec_.rows, 1), false, FILL_ZERO);
  side_alloc(r.dev, (size_t)sb_words(cap), false, FILL_ZERO);
  side_alloc(r.host, (size_t)sb_words(cap), false, FILL_ZERO);
  side_alloc(join, (size_t)sj_words(cap), false, FILL_ZERO);
  gain_blocks_alloc(r, cap);
  PE_HIP(hipDeviceSynchronize());
  sp_z_ = std::move(z); sp_cond_ = std::move(cond); sp_join_ = std::move(join);
  sp_slots_ = slots; sp_fcap_ = fcap; sp_maxf_ = max_frames;
  sp_frames_.assign(slots, 0);
  sp_live_.assign(slots, 0);
  r.cap = cap;
  r.pos.assign(slots, 0);
  r.gfirst.assign(slots, 1);
  r.off.assign(slots + 1, 0);
  r.src = sp_z_.get(); r.src_bs = (long)C_ * fcap; r.src_cs = fcap;
  r.cond = sp_cond_.get(); r.cond_bs = cond_dec_.rows;
  pool_rows_ = std::move(r);
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
                              const SeedsIn* seeds, const BlendIn* blend) {
  EntryLock entry_lock;
  stream_pool_require();
  if (seeds && !seeds->seed) throw std::runtime_error("seeds without a seed array (pe_seeds.seed is null)");
  if (blend) check_blend(*blend, n);
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
  upload(ids, offsets, n, scales, sids, noise, true, timing, seeds, blend);
  PE_HIP(hipSetDevice(device_));
  spec_pending_ = false;
  s_active_ = false;                                   // (a one-utterance stream on this handle loses its latent)
  stream_front(n, sp_maxf_);
  // the previous join ended with a synchronisation: nothing on the device reads the pinned join block any more
  const int cap = pool_rows_.cap;
  int* const join = sp_join_.get();
  join[0] = n;
  for (int j = 0; j < n; ++j) {
    join[sj_o_slot(cap) + j] = take[j];
    join[sj_o_frames(cap) + j] = frames_h_[j];
  }
  const float* cond = nspk_ > 1 ? cond_ + cond_off_dec_ : nullptr;
  PE_LAUNCH_KB("stream_adopt_kernel", 4.0 * n * C_ * ((double)Fg_ + sp_fcap_),
               launch::stream_adopt(dim3((Fg_ + 63) / 64, C_, n), stream_, zp_, (long)C_ * Fs_, Fs_, cond, cond_bs_,
                                    cond ? cond_dec_.rows : 0, join, cap, sp_z_.get(), (long)C_ * sp_fcap_, sp_fcap_, sp_cond_.get(),
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

void Engine::gain_blocks_alloc(ChunkRows& r, int cap) {
  side_alloc(r.gctl, (size_t)sg_words(cap), false, FILL_ZERO);
  side_alloc(r.gdev, (size_t)sgd_words(cap), false, FILL_ZERO);
  PE_HIP(hipDeviceSynchronize());
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
  if (gain_mode_ == GAIN_LOUDNESS) return;             // (sl_collect: the report lies in the rows' own control block)
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
// streams at a target loudness (kernels/stream_loudness.h)
// ------------------------------------------------------------------------------------------------

void Engine::set_stream_loudness(float target_lufs, float ceiling_db, float prior_lufs, int ramp_samples) {
  EntryLock entry_lock;
  check_target(target_lufs);
  check_ceiling(ceiling_db);
  if (std::isinf(prior_lufs) || (prior_lufs == prior_lufs && (prior_lufs < -70.f || prior_lufs > 0.f)))
    throw std::runtime_error("prior loudness " + std::to_string(prior_lufs) + " LUFS outside [-70, 0] (NaN: none)");
  if (ramp_samples < 0 || ramp_samples > GAIN_MAX_RAMP)
    throw std::runtime_error("stream loudness ramp_samples " + std::to_string(ramp_samples) + " outside [0, " +
                             std::to_string(GAIN_MAX_RAMP) + "]");
  loud_check_rate(output_rate());
  bool live = s_active_ && s_pos_ < s_frames_;
  if (sb_active_)
    for (int b = 0; b < B_ && b < (int)batch_rows_.pos.size(); ++b) live = live || batch_rows_.pos[b] < frames_h_[b];
  bool pool = false;
  for (int s = 0; s < sp_slots_; ++s) pool = pool || sp_live_[s] != 0;
  if (live || pool)
    throw std::runtime_error(std::string("the stream loudness cannot change while a ") +
                             (pool ? "stream pool slot is occupied" : "stream is live") + " on this handle");
  // all four numbers are data the gain kernel reads from the control block; the mode is part of the window stages' graph
  // keys, so nothing is dropped here
  sl_T_ = target_lufs; sl_cdb_ = ceiling_db; sl_prior_ = prior_lufs;
  gain_mode_ = GAIN_LOUDNESS; gain_ramp_ = ramp_samples;
}

int Engine::stream_last_loudness(float* lufs, float* gain, float* peak, int32_t* flags, int64_t capacity) {
  EntryLock entry_lock;
  if (lsl_n_ < 0 || lg_n_ < 0) throw std::runtime_error("no stream chunk delivered at a target loudness on this handle yet");
  if (gain_mode_ != GAIN_LOUDNESS) throw std::runtime_error("the stream loudness is not set (pe_set_stream_loudness)");
  if ((lufs || gain || peak || flags) && capacity < lsl_n_) throw std::runtime_error("stream loudness report buffer too small");
  for (int b = 0; b < lsl_n_; ++b) {
    if (lufs) lufs[b] = lsl_lufs_[b];
    if (gain) gain[b] = lg_gain_[b];
    if (peak) peak[b] = lg_peak_[b];
    if (flags) flags[b] = lsl_flags_[b];
  }
  return lsl_n_;
}

// ------------------------------------------------------------------------------------------------
// look-ahead limiter on streams (kernels/stream_limiter.h)
// ------------------------------------------------------------------------------------------------

void Engine::set_stream_limiter(bool on, float window_ms) {
  EntryLock entry_lock;
  lim_check(on, window_ms);
  loud_check_rate(output_rate());
  if (on) check_limiter_window_at(window_ms, output_rate());
  bool live = s_active_ && s_pos_ < s_frames_;
  if (sb_active_)
    for (int b = 0; b < B_ && b < (int)batch_rows_.pos.size(); ++b) live = live || batch_rows_.pos[b] < frames_h_[b];
  bool pool = false;
  for (int s = 0; s < sp_slots_; ++s) pool = pool || sp_live_[s] != 0;
  if (live || pool)
    throw std::runtime_error(std::string("the stream limiter cannot change while a ") +
                             (pool ? "stream pool slot is occupied" : "stream is live") + " on this handle");
  // on / off and W are part of the window stages' graph keys, the weights a table behind a fixed address: nothing is dropped
  slim_on_ = on;
  if (on) slim_ms_ = window_ms;
}

int Engine::stream_last_limiter(float* max_reduction, int32_t* shaped_samples, int64_t capacity) {
  EntryLock entry_lock;
  if ((max_reduction || shaped_samples) && capacity < lsm_n_) throw std::runtime_error("stream limiter report buffer too small");
  for (int b = 0; b < lsm_n_; ++b) {
    if (max_reduction) max_reduction[b] = lsm_maxred_[b];
    if (shaped_samples) shaped_samples[b] = lsm_shaped_[b];
  }
  return lsm_n_;
}

// The weights of the window at the delivered rate (they depend on W alone, and W is in the graph keys: a graph captured for
// one W is replayed only after the table holds that W's weights again) and the rows' limiter blocks.
void Engine::slim_ensure(ChunkRows& r, int cap) {
  const int fs = output_rate();
  if (!slim_h_ || slim_fs_ != fs || slim_hms_ != slim_ms_) {
    int W;
    std::vector<double> exact;
    limiter_window(fs, slim_ms_, W, exact);
    float table[2 * LIM_MAXW + 1] = {};
    to_f32(exact, table);
    PE_HIP(hipStreamSynchronize(stream_));
    if (!slim_h_) slim_h_.grow(2 * LIM_MAXW + 1);
    PE_HIP(hipMemcpy(slim_h_.get(), table, sizeof(table), hipMemcpyHostToDevice));
    slim_fs_ = fs; slim_W_ = W; slim_hms_ = slim_ms_;
  }
  if (r.mctl && r.mreph && r.mrep && r.mstail) return;
  PE_HIP(hipStreamSynchronize(stream_));
  side_alloc(r.mctl, (size_t)slm_words(cap), false, FILL_ZERO);
  side_alloc(r.mreph, (size_t)slm_rep_words(cap), false, FILL_ZERO);
  side_alloc(r.mrep, (size_t)slm_rep_words(cap), false, FILL_POISON_OR_ZERO);
  side_alloc(r.mstail, (size_t)cap * 2 * SLM_TAIL, false, FILL_POISON, "stream limiter scale tails");
  PE_HIP(hipDeviceSynchronize());
  r.mN.assign(r.mN.size(), 0);
  r.mB.assign(r.mB.size(), 0);
}

SlmP Engine::slim_params(const ChunkRows& r) const {
  SlmP p{};
  p.mctl = r.mctl.get(); p.lctl = r.lctl.get(); p.ldev = r.ldev.get(); p.gq = r.gdev.get(); p.cap = r.cap;
  p.tail = r.ltail.get(); p.TW = sl_W_; p.stail = r.mstail.get();
  p.h = slim_h_.get(); p.W = slim_W_;
  p.st = r.dev.get(); p.rep = r.mrep.get();
  return p;
}

void Engine::sl_ensure(ChunkRows& r, int cap, int64_t max_samples) {
  const int fs = output_rate();
  loud_check_rate(fs);
  if (!sl_coef_ || sl_fs_ != fs) {
    PE_HIP(hipStreamSynchronize(stream_));
    if (sl_coef_) drop_graphs();                       // (h / W / R are kernel arguments inside the graphs)
    sl_upload_filter(fs);
  }
  const int nseg = (int)((max_samples + sl_h_ - 1) / sl_h_) + 2;
  if (r.lctl && r.ldev && r.lseg && r.ltail && r.lnseg >= nseg && r.lW == sl_W_) return;
  PE_HIP(hipStreamSynchronize(stream_));
  if (r.lctl) drop_graphs();                           // the blocks' addresses are kernel arguments inside the stage's graphs
  r.lnseg = r.lW = 0;
  side_alloc(r.lctl, (size_t)slc_words(cap), false, FILL_ZERO);
  side_alloc(r.ldev, (size_t)sld_words(cap), false, FILL_POISON_OR_ZERO);
  side_alloc(r.lseg, (size_t)cap * nseg, false, FILL_POISON, "stream loudness segment sums");
  side_alloc(r.ltail, (size_t)cap * 2 * sl_W_, false, FILL_POISON);
  PE_HIP(hipDeviceSynchronize());
  r.lnseg = nseg; r.lW = sl_W_;
  // (nothing of a stream survives this: every row starts afresh, as after a begin or a join)
  r.gfirst.assign(r.gfirst.size(), 1);
}

// The previous chunk ended with a synchronisation: nothing on the device reads or writes the control block any more.
void Engine::sl_prepare(ChunkRows& r, int n) {
  int* ctl = r.lctl.get();
  const float C = (float)std::pow(10.0, (double)sl_cdb_ / 20.0);
  memcpy(ctl, &sl_T_, sizeof(float));
  memcpy(ctl + 1, &C, sizeof(float));
  memcpy(ctl + 2, &sl_prior_, sizeof(float));
  ctl[3] = gain_ramp_;
  for (int b = 0; b < n && b < r.cap; ++b) ctl[slc_o_first(r.cap) + b] = r.gfirst[b] ? 1 : 0;
}

SlP Engine::sl_params(const ChunkRows& r) const {
  SlP p{};
  p.ctl = r.lctl.get(); p.dev = r.ldev.get(); p.cap = r.cap;
  p.coef = sl_coef_.get(); p.h = sl_h_; p.W = sl_W_; p.R = sl_R_;
  p.seg = r.lseg.get(); p.nseg_cap = r.lnseg; p.tail = r.ltail.get();
  return p;
}

// The report of a chunk call over n rows (ran: its kernels ran; else nothing was delivered): a row whose stream has
// delivered nothing yet reports {-inf, 0, 0, SHORT | UNMEASURABLE}, every other row what its last chunk wrote.
void Engine::sl_collect(ChunkRows& r, int n, bool ran) {
  lsl_n_ = n;
  lsl_lufs_.assign(n, -std::numeric_limits<float>::infinity());
  lsl_flags_.assign(n, LOUD_SHORT | LOUD_UNMEASURABLE);
  lg_gain_.assign(n, 0.f);
  lg_peak_.assign(n, 0.f);
  const int cap = r.cap;
  const int* ctl = r.lctl.get();
  if (!ctl) return;
  const float* cf = reinterpret_cast<const float*>(ctl);
  for (int b = 0; b < n && b < cap; ++b) {
    const bool got = ran && lg_got_[b];
    if (b < (int)r.gfirst.size() && r.gfirst[b] && !got) continue;
    lsl_lufs_[b] = cf[slc_o_lufs(cap) + b];
    lsl_flags_[b] = ctl[slc_o_flags(cap) + b];
    lg_gain_[b] = cf[slc_o_gain(cap) + b];
    lg_peak_[b] = cf[slc_o_peak(cap) + b];
    if (got) r.gfirst[b] = 0;
  }
}

}  // namespace pe
