// Host engine, the delivery chain behind the generator: output-rate conversion, target loudness, the true-peak ceiling and
// the look-ahead limiter -- the host-side filter design, the setters and their refusals, the side buffers (ensure_*), the
// kernel sequences (issue_resample, issue_loudness), the reports and the four debug hooks. Life cycle, workspaces and the
// synthesis call: engine.cpp; streams: engine_stream.cpp.
#include "engine_internal.h"
#include "kernels/stream_limiter_rule.h"

#include <numeric>

namespace pe {

// ------------------------------------------------------------------------------------------------
// refusals and small formulas, each written once
// ------------------------------------------------------------------------------------------------

void Engine::check_target(float target_lufs) {
  if (!std::isfinite(target_lufs) || target_lufs < -40.f || target_lufs > -5.f)
    throw std::runtime_error("target loudness " + std::to_string(target_lufs) + " LUFS outside [-40, -5]");
}

void Engine::check_ceiling(float ceiling_db) {
  if (!std::isfinite(ceiling_db) || ceiling_db < -20.f || ceiling_db > 0.f)
    throw std::runtime_error("peak ceiling " + std::to_string(ceiling_db) + " dB outside [-20, 0]");
}

void Engine::check_ceiling_kind(int kind) {
  if (kind != PEAK_SAMPLE && kind != PEAK_TRUE)
    throw std::runtime_error("unknown loudness ceiling kind " + std::to_string(kind) + " (0: sample peak, 1: true peak)");
}

void Engine::check_limiter_window_at(float window_ms, int fs) {
  if (limiter_window_samples(fs, (double)window_ms) > LIM_MAXW)
    throw std::runtime_error("limiter window " + std::to_string(window_ms) + " ms is more than " + std::to_string(LIM_MAXW) +
                             " samples at " + std::to_string(fs) + " Hz");
}

int Engine::check_row_lengths(const int32_t* valid, int batch, int64_t stride) {
  int maxn = 0;
  for (int b = 0; b < batch; ++b) {
    if (valid[b] < 0 || valid[b] > stride) throw std::runtime_error("row " + std::to_string(b) + ": valid length outside [0, stride]");
    maxn = std::max(maxn, valid[b]);
  }
  return maxn;
}

void Engine::to_f32(const std::vector<double>& exact, float* out) {
  for (size_t i = 0; i < exact.size(); ++i) out[i] = (float)exact[i];
}

int Engine::row_block_cap() const {
  return (int)((std::max<size_t>(std::max(capA_B_, capB_B_), 64) + 1) & ~(size_t)1);
}

static float ceiling_ratio(float ceiling_db) { return (float)std::pow(10.0, (double)ceiling_db / 20.0); }

// ------------------------------------------------------------------------------------------------
// output-rate conversion
// ------------------------------------------------------------------------------------------------

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
  if (ld_on_ && lim_on_) check_limiter_window_at(lim_ms_, on ? output : native);
  if (gain_mode_ == GAIN_LOUDNESS) loud_check_rate(on ? output : native);      // (so is a stream's running loudness)
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
    to_f32(exact, table.data());
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
  DevBuf<float> coef;
  if (on) {
    coef.grow(table.size());
    if (hipMemcpy(coef.get(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("upload of the resampling table failed");
    }
  }
  // from here on nothing throws before the new setting is complete
  drop_graphs();                                       // the stage sequences and their buffer addresses depend on the rate
  rs_coef_ = std::move(coef);
  rs_on_ = on; rs_native_ = native; rs_out_ = on ? output : 0;
  rs_L_ = L; rs_M_ = M; rs_K_ = K; rs_Tp_ = Tp; rs_tile_ = tile;
  s_active_ = false; sb_active_ = false;               // (finished streams end here: their windows were sized for the old rate)
  pcm_zc_live_ = false;
  if (!on) {                                           // back to the native engine: its buffers and strides
    raudio_.reset();
    rpcm_.reset();
    So_ = Ss_;
  }
  // (on: the next call's ensure_stage_b derives So_ and sizes the zero-copy PCM buffer and the resampled rows)
  if (ld_on_) loud_upload_filter(output_rate());       // the K-weighting filter of the new delivered rate
}

// The resampled rows [capB_B_][So_] (floats + int16) and the two row blocks, (re)allocated when the workspace capacity or
// the rate changed; called at the end of ensure_stage_b, which has set So_.
void Engine::ensure_resample() {
  const size_t need = capB_B_ * (size_t)So_;
  const int want_cap = row_block_cap();
  const bool bufs = raudio_ && rpcm_ && raudio_.size() >= need, rows = rs_host_ && rs_dev_ && rs_cap_ >= want_cap;
  if (bufs && rows) return;
  PE_HIP(hipStreamSynchronize(stream_));
  drop_graphs();
  if (!bufs) {                                         // (one error speaks for both: after a failure neither is there)
    DevBuf<float> a;
    DevBuf<int16_t> p;
    raudio_.reset(); rpcm_.reset();
    side_alloc(a, need, false, FILL_POISON, "resampled output", need * 6);
    side_alloc(p, need, false, FILL_POISON, "resampled output", need * 6);
    raudio_ = std::move(a); rpcm_ = std::move(p);
  }
  if (!rows) {
    rs_cap_ = 0;
    side_alloc(rs_host_, (size_t)rs_words(want_cap), false, FILL_ZERO);
    side_alloc(rs_dev_, (size_t)rs_words(want_cap), false, FILL_ZERO);
    PE_HIP(hipDeviceSynchronize());
    rs_cap_ = want_cap;
  }
}

void Engine::rs_host_row(int b, int64_t n0, int64_t org, int count, int vlen) {
  if (!rs_host_ || b < 0 || b >= rs_cap_) return;
  int* h = rs_host_.get();
  reinterpret_cast<long long*>(h)[b] = n0;
  reinterpret_cast<long long*>(h + rs_o_org(rs_cap_))[b] = org;
  h[rs_o_count(rs_cap_) + b] = count;
  h[rs_o_vlen(rs_cap_) + b] = vlen;
}

// Output-rate conversion of B rows of x into raudio_: the row block (from the pinned block `hst`, or whole utterances of
// lens[b] * hop native samples), then resample_kernel on tiles of rs_tile_ outputs; max_out bounds every row's count.
void Engine::issue_resample(int B, const float* x, long x_bs, const int* hst, const int* lens, long max_out, double native_samples) {
  if (B > rs_cap_ || !raudio_ || !rs_coef_) throw std::runtime_error("resampling buffers are not sized for this call");
  max_out = std::max<long>(1, std::min<long>(max_out, So_));
  PE_LAUNCH_K("resample_rows_kernel",
              launch::resample_rows(stream_, hst, lens, hop_, rs_dev_.get(), rs_cap_, B, std::min<long>(x_bs, Ss_), So_, rs_L_, rs_M_));
  RsP p{};
  p.x = x; p.x_bs = x_bs; p.y = raudio_.get(); p.y_bs = So_;
  p.coef = rs_coef_.get(); p.L = rs_L_; p.M = rs_M_; p.K = rs_K_; p.Tp = rs_Tp_;
  p.rows = rs_dev_.get(); p.cap = rs_cap_; p.tile = rs_tile_;
  // algorithmic bytes: every native sample in once, every output out once (the table stays in cache)
  PE_LAUNCH_KB("resample_kernel", 4.0 * native_samples * (1.0 + (double)rs_L_ / rs_M_),
               launch::resample(dim3((unsigned)((max_out + rs_tile_ - 1) / rs_tile_), B), stream_, p));
}

void Engine::debug_resample(const float* x, int batch, int64_t stride, const int32_t* vlen, const int64_t* n0,
                            const int32_t* count, const int64_t* origin, float* out, int64_t out_stride) {
  EntryLock entry_lock;
  if (!rs_on_) throw std::runtime_error("no output rate set (pe_set_output_rate)");
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !vlen || !n0 || !count || !origin || !out) throw std::runtime_error("null argument");
  check_row_lengths(vlen, batch, stride);
  int maxc = 0;
  for (int b = 0; b < batch; ++b) {
    if (count[b] < 0 || count[b] > out_stride) throw std::runtime_error("row " + std::to_string(b) + ": output count outside [0, out_stride]");
    if (n0[b] < 0 || n0[b] > ((int64_t)1 << 40)) throw std::runtime_error("row " + std::to_string(b) + ": first output index out of range");
    maxc = std::max(maxc, count[b]);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const int cap = (batch + 1) & ~1;
  const long xs = (long)((stride + 3) & ~(int64_t)3), ys = (long)((std::max<int64_t>(out_stride, 1) + 3) & ~(int64_t)3);
  DevBuf<float> dx, dy;
  DevBuf<int> drows;
  PinBuf<int> hrows;
  try {
    dx.grow((size_t)batch * std::max<long>(xs, 4));
    dy.grow((size_t)batch * ys);
    drows.grow((size_t)rs_words(cap));
    hrows.grow((size_t)rs_words(cap));
    hrows.zero();
    int* h = hrows.get();
    for (int b = 0; b < batch; ++b) {
      reinterpret_cast<long long*>(h)[b] = n0[b];
      reinterpret_cast<long long*>(h + rs_o_org(cap))[b] = origin[b];
      h[rs_o_count(cap) + b] = count[b];
      h[rs_o_vlen(cap) + b] = vlen[b];
    }
    rows_to_device(dx.get(), xs, x, batch, stride);
    PE_HIP(hipMemsetAsync(dy.get(), 0xFF, dy.bytes(), stream_));
    launch::resample_rows(stream_, h, nullptr, 0, drows.get(), cap, batch, (long)stride, (long)out_stride, rs_L_, rs_M_);
    if (maxc > 0) {
      RsP p{};
      p.x = dx.get(); p.x_bs = xs; p.y = dy.get(); p.y_bs = ys;
      p.coef = rs_coef_.get(); p.L = rs_L_; p.M = rs_M_; p.K = rs_K_; p.Tp = rs_Tp_;
      p.rows = drows.get(); p.cap = cap; p.tile = rs_tile_;
      launch::resample(dim3((maxc + rs_tile_ - 1) / rs_tile_, batch), stream_, p);
    }
    rows_to_host(out, out_stride, dy.get(), ys, batch, count);
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
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
  ld_coef_.grow(LOUD_COEF_DOUBLES);
  PE_HIP(hipMemcpy(ld_coef_.get(), blk, sizeof(blk), hipMemcpyHostToDevice));
  ld_fs_ = fs; ld_h_ = h; ld_W_ = W; ld_R_ = R;
}

void Engine::sl_upload_filter(int fs) {
  double blk[LOUD_COEF_DOUBLES];
  int h, W, R;
  loud_plan(fs, h, W, R, blk);
  sl_coef_.grow(LOUD_COEF_DOUBLES);
  PE_HIP(hipMemcpy(sl_coef_.get(), blk, sizeof(blk), hipMemcpyHostToDevice));
  sl_fs_ = fs; sl_h_ = h; sl_W_ = W; sl_R_ = R;
}

void Engine::loud_write_ctl() {
  if (!ld_ctl_) return;
  const float C = ceiling_ratio(ld_cdb_);
  memcpy(ld_ctl_.get(), &ld_T_, sizeof(float));
  memcpy(ld_ctl_.get() + 1, &C, sizeof(float));
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
  to_f32(exact, table);
  tp_coef_.grow(TP_MAXQ * TP_TAPS);
  PE_HIP(hipMemcpy(tp_coef_.get(), table, sizeof(table), hipMemcpyHostToDevice));
  tp_fs_ = fs; tp_Q_ = Q;
}

void Engine::set_loudness_ceiling(int kind) {
  EntryLock entry_lock;
  check_ceiling_kind(kind);
  if (kind == PEAK_TRUE && ld_on_) tp_check_rate(output_rate());
  lim_check(lim_on_, lim_ms_);
  if (kind == ld_kind_) return;
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  // the kind picks the launches and is part of the graph keys: nothing is dropped, streams are not touched
  ld_kind_ = kind;
}

void Engine::lim_check(bool on, float window_ms) {
  if (!on) return;
  if (!std::isfinite(window_ms) || window_ms < 1.f || window_ms > 10.f)
    throw std::runtime_error("limiter window " + std::to_string(window_ms) + " ms outside [1, 10]");
}

// h_k = H_k / sum H, H_k = (1 + cos(pi k / (W + 1))) / 2, k = -W .. W: a raised cosine that ends above zero, in f64
void Engine::limiter_window(int fs, float window_ms, int& W, std::vector<double>& coef) {
  lim_check(true, window_ms);
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
  to_f32(exact, table);
  lim_h_.grow(2 * LIM_MAXW + 1);
  PE_HIP(hipMemcpy(lim_h_.get(), table, sizeof(table), hipMemcpyHostToDevice));
  lim_fs_ = fs; lim_W_ = W; lim_h_ms_ = lim_ms_;
}

void Engine::set_loudness_limiter(bool on, float window_ms) {
  EntryLock entry_lock;
  lim_check(on, window_ms);
  if (on && ld_on_) check_limiter_window_at(window_ms, output_rate());
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
    check_target(target_lufs);
    check_ceiling(ceiling_db);
    loud_check_rate(output_rate());
    if (ld_kind_ == PEAK_TRUE) tp_check_rate(output_rate());
    if (lim_on_) check_limiter_window_at(lim_ms_, output_rate());
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
// rate grew; called at the end of ensure_stage_b, which has set So_. The true-peak and limiter blocks: a first allocation
// is in no graph yet; a changed table or a grown block is inside the graphs of its setting (side_alloc's `idle`).
void Engine::ensure_loudness() {
  if (!ld_coef_ || ld_fs_ != output_rate()) loud_upload_filter(output_rate());
  const int nseg = (int)(So_ / ld_h_) + 2;
  const int want_cap = row_block_cap();
  if (ld_kind_ == PEAK_TRUE) {
    if (!tp_coef_ || tp_fs_ != output_rate()) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (tp_coef_) drop_graphs();
      tp_upload_table(output_rate());
    }
    if (tp_words_.size() < (size_t)want_cap) {
      side_alloc(tp_words_, (size_t)want_cap, true, FILL_POISON_OR_ZERO);
      PE_HIP(hipDeviceSynchronize());
    }
  }
  if (lim_on_) {
    if (!lim_h_ || lim_fs_ != output_rate() || lim_h_ms_ != lim_ms_) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (lim_h_) drop_graphs();
      lim_upload_window(output_rate());
    }
    if (!lim_rep_ || lim_cap_ < want_cap) {
      lim_cap_ = 0;
      side_alloc(lim_rep_, (size_t)lim_words(want_cap), true, FILL_POISON_OR_ZERO);
      side_alloc(lim_host_, (size_t)lim_words(want_cap), false, FILL_ZERO);
      PE_HIP(hipDeviceSynchronize());
      lim_cap_ = want_cap;
    }
    // true-peak ceiling: the per-position maxima v and the shaped floats z
    const size_t want = std::max<size_t>(capB_B_, 1) * (size_t)std::max<long>(std::max<long>(So_, Ss_), 4);
    if (ld_kind_ == PEAK_TRUE && (!lim_z_ || !lim_v_ || lim_z_.size() < want)) {
      PE_HIP(hipStreamSynchronize(stream_));
      if (lim_z_ || lim_v_) drop_graphs();
      DevBuf<float> z, v;                              // (one error speaks for both: after a failure neither is there)
      lim_z_.reset(); lim_v_.reset();
      side_alloc(z, want, false, FILL_POISON, "limiter rows", 2 * want * sizeof(float));
      side_alloc(v, want, false, FILL_POISON, "limiter rows", 2 * want * sizeof(float));
      lim_z_ = std::move(z); lim_v_ = std::move(v);
      PE_HIP(hipDeviceSynchronize());
    }
  }
  const bool seg = ld_seg_ && ld_seg_rows_ >= capB_B_ && ld_nseg_cap_ >= nseg, blocks = ld_ctl_ && ld_dev_ && ld_cap_ >= want_cap;
  if (seg && blocks) return;
  PE_HIP(hipStreamSynchronize(stream_));
  drop_graphs();
  if (!seg) {
    const size_t rows = std::max(ld_seg_rows_, capB_B_);
    const int cols = std::max(ld_nseg_cap_, nseg);
    ld_seg_rows_ = 0; ld_nseg_cap_ = 0;
    side_alloc(ld_seg_, rows * (size_t)cols, false, FILL_POISON, "loudness segment sums");
    ld_seg_rows_ = rows; ld_nseg_cap_ = cols;
  }
  if (!blocks) {
    ld_cap_ = 0;
    side_alloc(ld_ctl_, (size_t)ldc_words(want_cap), false, FILL_ZERO);
    side_alloc(ld_dev_, (size_t)ld_words(want_cap), false, FILL_ZERO);
    PE_HIP(hipDeviceSynchronize());
    ld_cap_ = want_cap;
    loud_write_ctl();
  }
}

void Engine::lim_enqueue_report() {
  if (!run_lim_ || !lim_rep_ || !lim_host_ || B_ > lim_cap_) return;
  PE_HIP(hipMemcpyAsync(lim_host_.get(), lim_rep_.get(), (size_t)lim_words(lim_cap_) * sizeof(int), hipMemcpyDeviceToHost, stream_));
}

void Engine::loud_collect() {
  ll_tn_ = 0;
  ll_ln_ = 0;
  if (!ld_on_ || !ld_ctl_ || B_ > ld_cap_) { ll_n_ = 0; return; }
  const int n = B_, cap = ld_cap_;
  const int* ctl = ld_ctl_.get();
  if (run_lim_ && lim_host_ && n <= lim_cap_) {
    const int* lh = lim_host_.get();
    const float* mr = reinterpret_cast<const float*>(lh) + lim_o_maxred(lim_cap_);
    ll_maxred_.assign(mr, mr + n);
    ll_shaped_.assign(lh + lim_o_count(lim_cap_), lh + lim_o_count(lim_cap_) + n);
    const float* tr = reinterpret_cast<const float*>(lh) + lim_o_trim(lim_cap_);
    ll_trim_.assign(tr, tr + n);
    ll_ln_ = n;
  }
  if (ld_kind_ == PEAK_TRUE) {
    const float* tf = reinterpret_cast<const float*>(ctl) + ldc_o_tpeak(cap);
    ll_tpeak_.assign(tf, tf + n);
    ll_tn_ = n;
  }
  const float* rf = reinterpret_cast<const float*>(ctl + ldc_o_report(cap));
  ll_lufs_.assign(rf, rf + n);
  ll_scale_.assign(rf + ld_o_scale(cap), rf + ld_o_scale(cap) + n);
  ll_peak_.assign(rf + ld_o_peak(cap), rf + ld_o_peak(cap) + n);
  ll_flags_.assign(ctl + ldc_o_report(cap) + ld_o_flags(cap), ctl + ldc_o_report(cap) + ld_o_flags(cap) + n);
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

int Engine::last_true_peak(float* t, int64_t capacity) {
  EntryLock entry_lock;
  if (ll_n_ < 0) throw std::runtime_error("no whole-utterance call fetched on this handle yet");
  if (t && capacity < ll_tn_) throw std::runtime_error("true-peak report buffer too small");
  if (t)
    for (int b = 0; b < ll_tn_; ++b) t[b] = ll_tpeak_[b];
  return ll_tn_;
}

// Target loudness of B delivered rows (whole utterances): the segment sums of the K-weighted rows, the gated loudness and
// the scale per row, and the int16 conversion with that scale in pcm16_kernel's place (kernels/loudness.h).
// The floats are only read, so it does not matter which kernel wrote them (conv_post, the fused stage tail, the resampler).
void Engine::issue_loudness(int B, const float* x, long x_bs, const int* lens, int len_mul, const unsigned* peaks, long max_n,
                            int16_t* pcm, int16_t* zc, double samples) {
  if (!ld_coef_ || !ld_seg_ || !ld_ctl_ || !ld_dev_ || B > ld_cap_ || (size_t)B > ld_seg_rows_ || ld_h_ < 1)
    throw std::runtime_error("loudness buffers are not sized for this call");
  max_n = std::max<long>(1, std::min<long>(max_n, x_bs));
  LoudP p{};
  p.x = x; p.x_bs = x_bs; p.lens = lens; p.len_mul = len_mul; p.x_cap = x_bs;
  p.coef = ld_coef_.get(); p.h = ld_h_; p.W = ld_W_; p.R = ld_R_;
  p.seg = ld_seg_.get(); p.nseg_cap = ld_nseg_cap_;
  const bool tp = ld_kind_ == PEAK_TRUE;
  if (tp && (!tp_coef_ || (size_t)B > tp_words_.size() || tp_fs_ != output_rate()))
    throw std::runtime_error("true-peak buffers are not sized for this call");
  p.tpeak = tp ? tp_words_.get() : nullptr;
  const bool lim = lim_on_;
  run_lim_ = lim;
  if (lim && tp && (!lim_z_ || !lim_v_ || (size_t)B * (size_t)x_bs > lim_z_.size()))
    throw std::runtime_error("limiter buffers are not sized for this call");
  if (lim && (!lim_h_ || !lim_rep_ || B > lim_cap_ || lim_fs_ != output_rate() || lim_h_ms_ != lim_ms_))
    throw std::runtime_error("limiter buffers are not sized for this call");
  p.limrep = lim ? lim_rep_.get() : nullptr; p.limcap = lim ? lim_cap_ : 0;
  const int nseg = (int)std::min<long>((max_n + ld_h_ - 1) / ld_h_, ld_nseg_cap_);
  // algorithmic bytes: every delivered sample in once (the warm-up is read again out of the caches)
  PE_LAUNCH_KB("loudness_seg_kernel", 4.0 * samples, launch::loudness_seg(dim3((unsigned)nseg, B), stream_, p));
  if (tp) {
    // true-peak ceiling: max |x interpolated tp_Q_ times| per row, into the words loudness_seg_kernel cleared
    TpP q{};
    q.x = x; q.x_bs = x_bs; q.lens = lens; q.len_mul = len_mul; q.x_cap = x_bs;
    q.coef = tp_coef_.get(); q.Q = tp_Q_; q.tpeak = tp_words_.get();
    if (lim) {      // (the limiter's envelope wants the per-position maxima as well)
      q.v = lim_v_.get();
      PE_LAUNCH_KB("true_peak_v_kernel", 8.0 * samples, launch::true_peak_v(dim3((unsigned)((max_n + TP_TILE - 1) / TP_TILE), B), stream_, q));
    } else
    PE_LAUNCH_KB("true_peak_kernel", 4.0 * samples, launch::true_peak(dim3((unsigned)((max_n + TP_TILE - 1) / TP_TILE), B), stream_, q));
  }
  PE_LAUNCH_K("loudness_gain_kernel",
              launch::loudness_gain(stream_, B, ld_seg_.get(), ld_nseg_cap_, lens, len_mul, x_bs, ld_h_, peaks, tp ? tp_words_.get() : nullptr,
                                    ld_ctl_.get(), ld_dev_.get(), ld_cap_, lim ? 1 : 0));
  if (lim) {
    // look-ahead limiter: the conversion, with the rows loudness_gain_kernel marked SHAPED turned down around their peaks
    LimTail t{};
    t.x = x; t.x_bs = x_bs; t.lens = lens; t.len_mul = len_mul; t.x_cap = x_bs;
    t.gq = ld_dev_.get(); t.gcap = ld_cap_; t.ctl = ld_ctl_.get(); t.rep = lim_rep_.get(); t.rcap = lim_cap_;
    t.h = lim_h_.get(); t.W = lim_W_;
    if (tp) { t.v = lim_v_.get(); t.z = lim_z_.get(); t.tp_coef = tp_coef_.get(); t.Q = tp_Q_; }
    t.pcm = pcm; t.zc = zc;
    issue_limiter_tail(t, B, max_n, samples, true);
    return;
  }
  PE_LAUNCH_KB("pcm16_gain_kernel", samples * (4.0 + 2.0 + (zc ? 2.0 : 0.0)),
               launch::pcm16_gain(dim3((unsigned)((max_n + 255) / 256), B), stream_, x, x_bs, ld_dev_.get(), ld_cap_, lens, len_mul, pcm,
                                  x_bs, zc));
}

// A launch of the tail: with its level-2 profile row (the run path), or bare (the hook, which leaves no rows)
#define PE_TAIL_LAUNCH(kname, bytes, call)         \
  do {                                             \
    if (profile_rows) PE_LAUNCH_KB(kname, bytes, call); \
    else { call; }                                 \
  } while (0)

void Engine::issue_limiter_tail(const LimTail& t, int B, long max_n, double samples, bool profile_rows) {
  LimP q{};
  q.x = t.x; q.x_bs = t.x_bs; q.lens = t.lens; q.len_mul = t.len_mul; q.x_cap = t.x_cap;
  q.gq = t.gq; q.gcap = t.gcap; q.ctl = t.ctl; q.h = t.h; q.W = t.W;
  q.pcm = t.pcm; q.p_bs = t.x_bs; q.host = t.zc; q.rep = t.rep; q.rcap = t.rcap;
  q.env = t.env; q.e_bs = t.env ? t.x_bs : 0;
  const double conv_bytes = samples * (4.0 + 2.0 + (t.zc ? 2.0 : 0.0));
  if (!t.v) {
    PE_TAIL_LAUNCH("limiter_kernel", conv_bytes, launch::limiter(dim3((unsigned)((max_n + LIM_TILE - 1) / LIM_TILE), B), stream_, q));
    return;
  }
  // true-peak ceiling: z = x e and max |z|, the true peak of z into its word, then the conversion with the trimmed scale
  q.v = t.v; q.z = t.z;
  PE_TAIL_LAUNCH("limiter_true_kernel", 12.0 * samples,
                 launch::limiter_true(dim3((unsigned)((max_n + LIM_TILE - 1) / LIM_TILE), B), stream_, q));
  TpP tz{};
  tz.x = t.z; tz.x_bs = t.x_bs; tz.lens = t.lens; tz.len_mul = t.len_mul; tz.x_cap = t.x_cap;
  tz.coef = t.tp_coef; tz.Q = t.Q; tz.tpeak = reinterpret_cast<unsigned*>(t.rep) + lim_o_tz(t.rcap);
  PE_TAIL_LAUNCH("true_peak_kernel", 4.0 * samples, launch::true_peak(dim3((unsigned)((max_n + TP_TILE - 1) / TP_TILE), B), stream_, tz));
  TrimP r{};
  r.z = t.z; r.z_bs = t.x_bs; r.lens = t.lens; r.len_mul = t.len_mul; r.gq = t.gq; r.gcap = t.gcap; r.ctl = t.ctl;
  r.rep = t.rep; r.rcap = t.rcap; r.pcm = t.pcm; r.p_bs = t.x_bs; r.host = t.zc;
  PE_TAIL_LAUNCH("pcm16_trim_kernel", conv_bytes, launch::pcm16_trim(dim3((unsigned)((max_n + 255) / 256), B), stream_, r));
}
#undef PE_TAIL_LAUNCH

// ------------------------------------------------------------------------------------------------
// sample format: G.711 codes of the delivered int16
// ------------------------------------------------------------------------------------------------

void Engine::set_sample_format(int format) {
  EntryLock entry_lock;
  if (format != G711_S16 && format != G711_ULAW && format != G711_ALAW)
    throw std::runtime_error("unknown sample format " + std::to_string(format) + " (0: s16, 1: ulaw, 2: alaw)");
  bool live = s_active_ && s_pos_ < s_frames_;
  if (sb_active_)
    for (int b = 0; b < B_ && b < (int)batch_rows_.pos.size(); ++b) live = live || batch_rows_.pos[b] < frames_h_[b];
  if (live || sp_slots_)
    throw std::runtime_error(std::string("the sample format cannot change while a ") +
                             (sp_slots_ ? "stream pool is open" : "stream is live") + " on this handle");
  if (format == fmt_) return;
  PE_HIP(hipSetDevice(device_));
  finish_run();                                        // (a speculative run still in flight settles first)
  // the format picks one launch and is part of the graph keys: nothing is dropped, streams that ended are not touched
  fmt_ = format;
}

// The packed codes of a whole-utterance call: one byte per delivered sample of the batch capacity. Called at the end of
// ensure_stage_b, which has set So_; a buffer that grows is inside the graphs of its format.
void Engine::ensure_g711() {
  const size_t need = std::max<size_t>(capB_B_ * (size_t)So_, 16);
  if (codes_ && codes_.size() >= need) return;
  side_alloc(codes_, need, true, FILL_POISON, "G.711 codes");
}

void Engine::issue_g711(int B, const int16_t* pcm, long p_bs, const int* lens, int len_mul, long max_n, double samples) {
  if (!codes_ || codes_.size() < (size_t)B * (size_t)p_bs) throw std::runtime_error("G.711 code buffer is not sized for this call");
  max_n = std::max<long>(1, std::min<long>(max_n, p_bs));
  PE_LAUNCH_KB("g711_kernel", 3.0 * samples,
               launch::g711_rows(stream_, B, max_n, lens, len_mul, pcm, p_bs, codes_.get(), (long)codes_.size(), fmt_));
}

int Engine::last_codes(int which, const uint8_t** codes, const int64_t** offsets) {
  EntryLock entry_lock;
  if (which != 0 && which != 1) throw std::runtime_error("pe_last_codes: which must be 0 (whole utterances) or 1 (stream chunk)");
  const int rows = which == 0 ? lc_rows_ : lc_s_rows_;
  static const uint8_t nothing[1] = {0};                 // (a chunk call that delivered nothing: rows of no bytes, not NULL)
  const uint8_t* view = which == 0 ? h_codes_.get() : lc_s_codes_;
  if (codes) *codes = rows ? (view ? view : nothing) : nullptr;
  if (offsets) *offsets = rows ? (which == 0 ? sample_off_.data() : lc_s_off_) : nullptr;
  return rows;
}

// ------------------------------------------------------------------------------------------------
// test hooks: one kernel family alone on caller-given rows
// ------------------------------------------------------------------------------------------------

void Engine::debug_limiter(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, const float* g, float ceiling_db,
                           int kind, float window_ms, float* env, int16_t* pcm) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !g || !env || !pcm) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  check_ceiling(ceiling_db);
  check_ceiling_kind(kind);
  lim_check(true, window_ms);
  int W;
  std::vector<double> exact;
  limiter_window(fs, window_ms, W, exact);
  float table[2 * LIM_MAXW + 1] = {};
  to_f32(exact, table);
  const int cap = (batch + 1) & ~1;
  const float C = ceiling_ratio(ceiling_db);
  std::vector<int> gq((size_t)ld_words(cap), 0);
  std::vector<float> peak((size_t)batch, 0.f);
  const int maxn = check_row_lengths(valid, batch, stride);
  for (int b = 0; b < batch; ++b) {
    if (!std::isfinite(g[b]) || !(g[b] > 0.f)) throw std::runtime_error("row " + std::to_string(b) + ": gain " + std::to_string(g[b]) + " is not positive and finite");
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
    to_f32(tex, tptable);
  } else {
    fill_gq(nullptr);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const long xs = (long)((std::max<int64_t>(stride, 1) + 3) & ~(int64_t)3);
  const size_t rows = (size_t)batch * xs;
  const unsigned tp_grid = (unsigned)std::max(1, (maxn + TP_TILE - 1) / TP_TILE);
  DevBuf<float> dx, dh, denv, dv, dz, dtab;
  DevBuf<int> dval, dgq, dctl, drep;
  DevBuf<unsigned> dtp;
  DevBuf<int16_t> dpcm;
  try {
    const float ctl[2] = {0.f, C};
    dx.grow(rows);
    denv.grow(rows);
    dpcm.grow(rows);
    dh.grow(2 * LIM_MAXW + 1);
    dval.grow((size_t)batch);
    dgq.grow(gq.size());
    dctl.grow((size_t)ldc_words(cap));                 // (pcm16_trim_kernel writes the report's scale)
    drep.grow((size_t)lim_words(cap));
    rows_to_device(dx.get(), xs, x, batch, stride);
    rows_to_device(denv.get(), xs, env, batch, stride);      // (what lies behind a row's end comes back as the caller left it)
    rows_to_device(dpcm.get(), xs, pcm, batch, stride);
    PE_HIP(hipMemcpyAsync(dh.get(), table, sizeof(table), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval.get(), valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dctl.get(), ctl, sizeof(ctl), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(drep.get(), 0, drep.bytes(), stream_));
    if (tp) {
      // the first true-peak pass: t for the rule, v for the envelope
      dv.grow(rows);
      dz.grow(rows);
      dtab.grow(TP_MAXQ * TP_TAPS);
      dtp.grow((size_t)batch);
      PE_HIP(hipMemcpyAsync(dtab.get(), tptable, sizeof(tptable), hipMemcpyHostToDevice, stream_));
      PE_HIP(hipMemsetAsync(dtp.get(), 0, dtp.bytes(), stream_));
      PE_HIP(hipMemsetAsync(dv.get(), 0xFF, dv.bytes(), stream_));
      PE_HIP(hipMemsetAsync(dz.get(), 0xFF, dz.bytes(), stream_));
      PE_HIP(hipStreamSynchronize(stream_));
      TpP tq{};
      tq.x = dx.get(); tq.x_bs = xs; tq.lens = dval.get(); tq.len_mul = 1; tq.x_cap = (long)stride;
      tq.coef = dtab.get(); tq.Q = Q; tq.tpeak = dtp.get(); tq.v = dv.get();
      launch::true_peak_v(dim3(tp_grid, batch), stream_, tq);
      std::vector<float> tpk((size_t)batch, 0.f);
      PE_HIP(hipMemcpyAsync(tpk.data(), dtp.get(), (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, stream_));
      PE_HIP(hipStreamSynchronize(stream_));
      fill_gq(tpk.data());
    }
    PE_HIP(hipMemcpyAsync(dgq.get(), gq.data(), gq.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging arrays are pageable)
    LimTail t{};
    t.x = dx.get(); t.x_bs = xs; t.lens = dval.get(); t.len_mul = 1; t.x_cap = (long)stride;
    t.gq = dgq.get(); t.gcap = cap; t.ctl = dctl.get(); t.rep = drep.get(); t.rcap = cap;
    t.h = dh.get(); t.W = W;
    t.v = dv.get(); t.z = dz.get(); t.tp_coef = dtab.get(); t.Q = Q;      // (all null with the sample-peak ceiling)
    t.pcm = dpcm.get(); t.zc = nullptr; t.env = denv.get();
    issue_limiter_tail(t, batch, std::max(maxn, 1), 0.0, false);
    rows_to_host(env, stride, denv.get(), xs, batch);
    rows_to_host(pcm, stride, dpcm.get(), xs, batch);
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
}

void Engine::debug_g711(int format, bool flat, const int16_t* x, int batch, int64_t stride, const int32_t* valid, uint8_t* out,
                        int64_t out_capacity) {
  EntryLock entry_lock;
  if (format != G711_ULAW && format != G711_ALAW) throw std::runtime_error("G.711 hook: format must be 1 (ulaw) or 2 (alaw)");
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (flat && batch != 1) throw std::runtime_error("G.711 hook: the flat form takes one row");
  if (!x || !valid || !out) throw std::runtime_error("null argument");
  if (stride < 1 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [1, 2^28]");
  if (out_capacity < 1 || out_capacity > ((int64_t)1 << 32)) throw std::runtime_error("out_capacity outside [1, 2^32]");
  const int maxn = check_row_lengths(valid, batch, stride);
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const long xs = (long)((stride + 3) & ~(int64_t)3);
  DevBuf<int16_t> dx;
  DevBuf<int> dval;
  DevBuf<uint8_t> dout;
  try {
    dx.grow((size_t)batch * std::max<long>(xs, 8));
    dval.grow((size_t)batch);
    dout.grow((size_t)out_capacity);
    rows_to_device(dx.get(), xs, x, batch, stride);
    PE_HIP(hipMemcpyAsync(dval.get(), valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dout.get(), out, (size_t)out_capacity, hipMemcpyHostToDevice, stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging arrays are pageable)
    if (flat) launch::g711_flat(stream_, dx.get(), std::min<long>(valid[0], (long)out_capacity), dout.get(), format);
    else launch::g711_rows(stream_, batch, std::max(maxn, 1), dval.get(), 1, dx.get(), xs, dout.get(), (long)out_capacity, format);
    PE_HIP(hipMemcpyAsync(out, dout.get(), (size_t)out_capacity, hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
}

void Engine::debug_true_peak(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float* t) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !t) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  int Q, K;
  std::vector<double> exact;
  true_peak_filter(fs, Q, K, exact);
  float table[TP_MAXQ * TP_TAPS] = {};
  to_f32(exact, table);
  const int maxn = check_row_lengths(valid, batch, stride);
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const long xs = (long)((std::max<int64_t>(stride, 1) + 3) & ~(int64_t)3);
  DevBuf<float> dx, dcoef;
  DevBuf<int> dval;
  DevBuf<unsigned> dtp;
  try {
    dx.grow((size_t)batch * xs);
    dcoef.grow(TP_MAXQ * TP_TAPS);
    dval.grow((size_t)batch);
    dtp.grow((size_t)batch);
    rows_to_device(dx.get(), xs, x, batch, stride);
    PE_HIP(hipMemcpyAsync(dcoef.get(), table, sizeof(table), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval.get(), valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(dtp.get(), 0, dtp.bytes(), stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging arrays are pageable)
    TpP p{};
    p.x = dx.get(); p.x_bs = xs; p.lens = dval.get(); p.len_mul = 1; p.x_cap = (long)stride;
    p.coef = dcoef.get(); p.Q = Q; p.tpeak = dtp.get();
    launch::true_peak(dim3((unsigned)std::max(1, (maxn + TP_TILE - 1) / TP_TILE), batch), stream_, p);
    PE_HIP(hipMemcpyAsync(t, dtp.get(), (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, stream_));
    PE_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
}

void Engine::debug_loudness(const float* x, int batch, int64_t stride, const int32_t* valid, int fs, float target, float ceiling_db,
                            float* lufs, float* scale, int32_t* flags) {
  EntryLock entry_lock;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !valid || !lufs || !scale || !flags) throw std::runtime_error("null argument");
  if (stride < 0 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [0, 2^28]");
  check_target(target);
  check_ceiling(ceiling_db);
  loud_check_rate(fs);
  const int maxn = check_row_lengths(valid, batch, stride);
  std::vector<unsigned> peaks((size_t)batch, 0u);
  for (int b = 0; b < batch; ++b) {
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
  DevBuf<float> dx;
  DevBuf<double> dcoef, dseg;
  DevBuf<int> dval, gd;
  DevBuf<unsigned> dpk;
  PinBuf<int> ctl;
  try {
    dx.grow((size_t)batch * xs);
    dcoef.grow(LOUD_COEF_DOUBLES);
    dseg.grow((size_t)batch * nseg_cap);
    dval.grow((size_t)batch);
    dpk.grow((size_t)batch);
    gd.grow((size_t)ld_words(cap));
    ctl.grow((size_t)ldc_words(cap));
    ctl.zero();
    const float C = ceiling_ratio(ceiling_db);
    memcpy(ctl.get(), &target, sizeof(float));
    memcpy(ctl.get() + 1, &C, sizeof(float));
    rows_to_device(dx.get(), xs, x, batch, stride);
    PE_HIP(hipMemcpyAsync(dcoef.get(), blk, sizeof(blk), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dval.get(), valid, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemcpyAsync(dpk.get(), peaks.data(), (size_t)batch * sizeof(unsigned), hipMemcpyHostToDevice, stream_));
    PE_HIP(hipMemsetAsync(dseg.get(), 0xFF, dseg.bytes(), stream_));
    PE_HIP(hipStreamSynchronize(stream_));             // (the staging vectors are pageable)
    LoudP p{};
    p.x = dx.get(); p.x_bs = xs; p.lens = dval.get(); p.len_mul = 1; p.x_cap = (long)stride;
    p.coef = dcoef.get(); p.h = h; p.W = W; p.R = R; p.seg = dseg.get(); p.nseg_cap = nseg_cap;
    launch::loudness_seg(dim3((unsigned)std::max(1, (maxn + h - 1) / h), batch), stream_, p);
    launch::loudness_gain(stream_, batch, dseg.get(), nseg_cap, dval.get(), 1, (long)stride, h, dpk.get(), nullptr, ctl.get(), gd.get(), cap, 0);
    PE_HIP(hipStreamSynchronize(stream_));
    const float* rf = reinterpret_cast<const float*>(ctl.get() + ldc_o_report(cap));
    for (int b = 0; b < batch; ++b) {
      lufs[b] = rf[b];
      scale[b] = rf[ld_o_scale(cap) + b];
      flags[b] = ctl.get()[ldc_o_report(cap) + ld_o_flags(cap) + b];
    }
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
}

// The production kernels of a stream at a target loudness, chunk after chunk: the rows are windows of hop 1 that hold the
// whole row, the chunk of row b its next chunks[k][b] samples; the peak word is the host's max |x| over the chunk.
void Engine::debug_stream_loudness(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                                   float ceiling_db, float prior_lufs, int ramp_samples, float* lufs, float* g0, float* g1,
                                   int32_t* flags, int16_t* pcm) {
  debug_stream_rows(x, batch, stride, fs, chunks, n_chunks, target, ceiling_db, prior_lufs, ramp_samples, 0.f, lufs, g0, g1, flags,
                    nullptr, nullptr, pcm);
}

void Engine::debug_stream_limiter(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                                  float ceiling_db, float prior_lufs, int ramp_samples, float window_ms, float* lufs, float* g0,
                                  float* g1, int32_t* flags, int32_t* delivered, float* env, int16_t* pcm) {
  if (!delivered || !env) throw std::runtime_error("null argument");
  lim_check(true, window_ms);
  debug_stream_rows(x, batch, stride, fs, chunks, n_chunks, target, ceiling_db, prior_lufs, ramp_samples, window_ms, lufs, g0, g1,
                    flags, delivered, env, pcm);
}

// window_ms > 0: with the look-ahead limiter (stream_limiter_kernel in the conversion's place; a row ends with its last chunk
// of length > 0; pcm in delivery order, delivered[n_chunks][batch], env[batch][stride]).
void Engine::debug_stream_rows(const float* x, int batch, int64_t stride, int fs, const int32_t* chunks, int n_chunks, float target,
                               float ceiling_db, float prior_lufs, int ramp_samples, float window_ms, float* lufs, float* g0, float* g1,
                               int32_t* flags, int32_t* delivered, float* env, int16_t* pcm) {
  EntryLock entry_lock;
  const bool lim = window_ms > 0.f;
  if (batch < 1 || batch > 4096) throw std::runtime_error("batch size must be in [1, 4096]");
  if (!x || !chunks || !lufs || !g0 || !g1 || !flags || !pcm) throw std::runtime_error("null argument");
  if (stride < 1 || stride > ((int64_t)1 << 28)) throw std::runtime_error("row stride outside [1, 2^28]");
  if (n_chunks < 1 || n_chunks > 65536) throw std::runtime_error("n_chunks outside [1, 65536]");
  if (fs < 8000 || fs > 48000) throw std::runtime_error("stream loudness hook: rate " + std::to_string(fs) + " Hz outside [8000, 48000]");
  check_target(target);
  check_ceiling(ceiling_db);
  if (std::isinf(prior_lufs) || (prior_lufs == prior_lufs && (prior_lufs < -70.f || prior_lufs > 0.f)))
    throw std::runtime_error("prior loudness " + std::to_string(prior_lufs) + " LUFS outside [-70, 0] (NaN: none)");
  if (ramp_samples < 0 || ramp_samples > GAIN_MAX_RAMP) throw std::runtime_error("ramp_samples outside [0, " + std::to_string(GAIN_MAX_RAMP) + "]");
  int maxc = 1;
  std::vector<int> lastk((size_t)batch, -1);             // the call that consumes the row's last samples
  for (int b = 0; b < batch; ++b) {
    int64_t sum = 0;
    for (int k = 0; k < n_chunks; ++k) {
      const int c = chunks[(size_t)k * batch + b];
      if (c < 0) throw std::runtime_error("row " + std::to_string(b) + ": negative chunk length");
      sum += c;
      maxc = std::max(maxc, c);
      if (c > 0) lastk[b] = k;
    }
    if (sum > stride) throw std::runtime_error("row " + std::to_string(b) + ": the chunks hold more than stride samples");
  }
  double blk[LOUD_COEF_DOUBLES];
  int h, W, R;
  loud_plan(fs, h, W, R, blk);
  int LW = 0;
  float table[2 * LIM_MAXW + 1] = {};
  if (lim) {
    std::vector<double> exact;
    limiter_window(fs, window_ms, LW, exact);
    to_f32(exact, table);
  }
  PE_HIP(hipSetDevice(device_));
  finish_run();
  const int cap = (batch + 1) & ~1, nseg_cap = (int)((stride + h - 1) / h) + 2;
  const long xs = (long)((stride + 3) & ~(int64_t)3);
  DevBuf<float> dx, dtail, dstail, dh, denv;
  DevBuf<double> dcoef, dseg;
  DevBuf<int> ddev, dgq, drep;
  PinBuf<int> ctl, st, mctl;
  PinBuf<int16_t> hp;
  try {
    if (lim) {
      dstail.grow((size_t)cap * 2 * SLM_TAIL);
      dh.grow(2 * LIM_MAXW + 1);
      denv.grow((size_t)batch * xs);
      drep.grow((size_t)slm_rep_words(cap));
      mctl.grow((size_t)slm_words(cap));
      mctl.zero();
      PE_HIP(hipMemcpyAsync(dh.get(), table, sizeof(table), hipMemcpyHostToDevice, stream_));
      PE_HIP(hipMemsetAsync(dstail.get(), 0xFF, dstail.bytes(), stream_));
      PE_HIP(hipMemsetAsync(drep.get(), 0xFF, drep.bytes(), stream_));
      rows_to_device(denv.get(), xs, env, batch, stride);    // (what no call delivers comes back as the caller left it)
    }
    dx.grow((size_t)batch * xs);
    dcoef.grow(LOUD_COEF_DOUBLES);
    dseg.grow((size_t)cap * nseg_cap);
    dtail.grow((size_t)cap * 2 * W);
    ddev.grow((size_t)sld_words(cap));
    dgq.grow((size_t)sgd_words(cap));
    ctl.grow((size_t)slc_words(cap));
    st.grow((size_t)sb_words(cap));
    hp.grow((size_t)batch * stride);
    ctl.zero();
    st.zero();
    memcpy(hp.get(), pcm, (size_t)batch * stride * sizeof(int16_t));      // (what no chunk covers comes back as the caller left it)
    const float C = ceiling_ratio(ceiling_db);
    memcpy(ctl.get(), &target, sizeof(float));
    memcpy(ctl.get() + 1, &C, sizeof(float));
    memcpy(ctl.get() + 2, &prior_lufs, sizeof(float));
    ctl.get()[3] = ramp_samples;
    rows_to_device(dx.get(), xs, x, batch, stride);
    PE_HIP(hipMemcpyAsync(dcoef.get(), blk, sizeof(blk), hipMemcpyHostToDevice, stream_));
    // (every word of the state a stream carries is poisoned: a row's first chunk must not read any of it)
    PE_HIP(hipMemsetAsync(dseg.get(), 0xFF, dseg.bytes(), stream_));
    PE_HIP(hipMemsetAsync(dtail.get(), 0xFF, dtail.bytes(), stream_));
    PE_HIP(hipMemsetAsync(ddev.get(), 0xFF, ddev.bytes(), stream_));
    PE_HIP(hipMemsetAsync(dgq.get(), 0, dgq.bytes(), stream_));
    PE_HIP(hipStreamSynchronize(stream_));
    SlP p{};
    p.ctl = ctl.get(); p.dev = ddev.get(); p.cap = cap; p.coef = dcoef.get(); p.h = h; p.W = W; p.R = R;
    p.seg = dseg.get(); p.nseg_cap = nseg_cap; p.tail = dtail.get();
    SlChunkP q{};
    q.x = dx.get(); q.x_bs = xs; q.st = st.get(); q.cap = cap; q.hop = 1;
    int* s = st.get();
    void* ptrs[2] = {hp.get(), nullptr};
    memcpy(s + sb_o_ptrs(cap), ptrs, sizeof(ptrs));
    std::vector<int64_t> done((size_t)batch, 0), given((size_t)batch, 0);
    std::vector<char> first((size_t)batch, 1);
    const int nseg = (maxc + h - 1) / h + 1, steps = std::max(1, (maxc + CHUNK_SPB - 1) / CHUNK_SPB);
    SlmP m{};
    m.mctl = mctl.get(); m.lctl = ctl.get(); m.ldev = ddev.get(); m.gq = dgq.get(); m.cap = cap;
    m.tail = dtail.get(); m.TW = W; m.stail = dstail.get(); m.h = dh.get(); m.W = LW;
    m.st = s; m.rep = drep.get(); m.env = denv.get(); m.e_bs = xs;
    for (int k = 0; k < n_chunks; ++k) {
      for (int b = 0; b < batch; ++b) {
        const int c = chunks[(size_t)k * batch + b];
        float pk = 0.f;
        for (int i = 0; i < c; ++i) pk = std::max(pk, std::fabs(x[(size_t)b * stride + done[b] + i]));
        s[b] = 0;
        s[sb_o_len(cap) + b] = (int)stride;
        s[sb_o_first(cap) + b] = (int)done[b];
        s[sb_o_count(cap) + b] = c;
        reinterpret_cast<long long*>(s + sb_o_off(cap))[b] = (long long)b * stride + (lim ? given[b] : done[b]);
        memcpy(s + sb_o_peak(cap) + b, &pk, sizeof(float));
        ctl.get()[slc_o_first(cap) + b] = first[b];
        if (lim) {
          const int64_t to = c > 0 ? slm_delivered(done[b] + c, 2 * LW, k == lastk[b]) : given[b];
          mctl.get()[b] = (int)done[b];
          mctl.get()[slm_o_b0(cap) + b] = (int)given[b];
          mctl.get()[slm_o_cnt(cap) + b] = (int)(to - given[b]);
          delivered[(size_t)k * batch + b] = (int32_t)(to - given[b]);
          given[b] = to;
        }
      }
      launch::stream_loudness_seg(stream_, nseg, batch, p, q);
      launch::stream_loudness_gain(stream_, batch, p, q, dgq.get(), lim ? drep.get() : nullptr);
      if (lim) launch::stream_limiter(stream_, (maxc + 2 * LW + LIM_TILE - 1) / LIM_TILE, batch, m, q);
      else launch::chunk_pcm_gain(dim3(steps, batch), stream_, dx.get(), xs, s, cap, 1, dgq.get());
      PE_HIP(hipStreamSynchronize(stream_));
      const float* cf = reinterpret_cast<const float*>(ctl.get());
      for (int b = 0; b < batch; ++b) {
        const size_t o = (size_t)k * batch + b;
        const int c = chunks[o];
        const bool none = first[b] && c == 0;            // (nothing delivered yet: the kernel wrote the empty report)
        lufs[o] = cf[slc_o_lufs(cap) + b];
        g0[o] = none ? 0.f : cf[slc_o_g0(cap) + b];
        g1[o] = cf[slc_o_gain(cap) + b];
        flags[o] = ctl.get()[slc_o_flags(cap) + b];
        done[b] += c;
        if (c > 0) first[b] = 0;
      }
    }
    memcpy(pcm, hp.get(), (size_t)batch * stride * sizeof(int16_t));
    if (lim) {
      rows_to_host(env, stride, denv.get(), xs, batch);
      PE_HIP(hipStreamSynchronize(stream_));
    }
  } catch (...) {
    hipStreamSynchronize(stream_);                     // (nothing is freed under a running kernel)
    throw;
  }
}

}  // namespace pe
