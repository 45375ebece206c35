// SynthesisConfig::limiter through the piper:: API: textToAudio on a sentence of two phrases with targetLufs set, without and
// with the limiter; the setting read back from the engine (pe_get_loudness_limiter) and every phrase's report
// (pe_last_limiter, pe_last_loudness); then the limiter cleared, and set again without targetLufs (the engine remembers it).
//   usage: test_limiter <voice.onnx>
// Prints one `phrase i red=... shaped=... trim=... scale=... flags=... max=...` line per phrase and `OK ...`; the pytest
// wrapper checks them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "piper.hpp"
#include "piper_hip.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_limiter voice.onnx\n";
    return 2;
  }
  try {
    piper::PiperConfig config;
    piper::Voice voice;
    std::optional<piper::SpeakerId> speaker;
    piper::loadVoice(config, argv[1], std::string(argv[1]) + ".json", voice, speaker, false);
    piper::initialize(config);
    piper::SynthesisConfig& sc = voice.synthesisConfig;
    sc.noiseScale = 0.0f;
    sc.noiseW = 0.0f;
    sc.lengthScale = 3.0f;
    sc.phonemeSilenceSeconds.emplace();
    (*sc.phonemeSilenceSeconds)[U','] = 0.01f;
    const char* text = "abcdefgh abcdefgh, hgfedcba hgfedcba abc";
    if (sc.limiter || sc.limiterMs != 5.0f) {
      std::cerr << "ERROR: the limiter is not off with 5 ms by default\n";
      return 1;
    }

    std::vector<int16_t> off, on, again;
    piper::SynthesisResult r;
    int32_t lim = -1, W = -1, n = -1;
    float ms = 0.f;
    sc.targetLufs = -8.0f;
    sc.peakCeilingDb = -2.0f;
    piper::textToAudio(config, voice, text, off, r, nullptr);
    float red[8], trim[8], L[8], scale[8], peak[8];
    int32_t cnt[8], flags[8];
    if (pe_get_loudness_limiter(voice.session.engine, &lim, &ms, &W) || lim != 0 ||
        pe_last_limiter(voice.session.engine, red, cnt, trim, 8, &n) || n != 0) {
      std::cerr << "ERROR: the limiter is on without SynthesisConfig::limiter\n";
      return 1;
    }

    sc.limiter = true;
    sc.limiterMs = 4.0f;
    piper::textToAudio(config, voice, text, on, r, nullptr);
    if (pe_get_loudness_limiter(voice.session.engine, &lim, &ms, &W) || lim != 1 || ms != 4.0f) {
      std::cerr << "ERROR: limiter / limiterMs did not reach the engine\n";
      return 1;
    }
    if (pe_last_limiter(voice.session.engine, red, cnt, trim, 8, &n) || n != 2 ||
        pe_last_loudness(voice.session.engine, L, scale, peak, flags, 8, &n) || n != 2) {
      std::cerr << "ERROR: expected the report of two phrases, got " << n << ": " << pe_last_error() << "\n";
      return 1;
    }
    if (on.size() != off.size()) {
      std::cerr << "ERROR: the limiter changed the length\n";
      return 1;
    }
    int top = 0;
    for (int16_t v : on) top = std::max(top, std::abs((int)v));
    for (int i = 0; i < n; ++i)
      std::printf("phrase %d red=%.6f shaped=%d trim=%.6f scale=%.4f flags=%d\n", i, red[i], cnt[i], trim[i], scale[i], flags[i]);

    sc.limiter = false;
    piper::textToAudio(config, voice, text, again, r, nullptr);
    int32_t m = -1;
    if (pe_get_loudness_limiter(voice.session.engine, &lim, nullptr, nullptr) || lim != 0 || again != off ||
        pe_last_limiter(voice.session.engine, nullptr, nullptr, nullptr, 0, &m) || m != 0) {
      std::cerr << "ERROR: clearing the limiter does not give the limiter-off delivery back\n";
      return 1;
    }
    sc.targetLufs.reset();
    sc.limiter = true;
    piper::textToAudio(config, voice, text, again, r, nullptr);
    int32_t lon = 1;
    if (pe_get_loudness(voice.session.engine, &lon, nullptr, nullptr) || lon ||
        pe_get_loudness_limiter(voice.session.engine, &lim, &ms, nullptr) || lim != 1 || ms != 4.0f) {
      std::cerr << "ERROR: the limiter without targetLufs is not remembered by the engine\n";
      return 1;
    }
    std::printf("OK phrases=%d window=%d max=%d differs=%d ceiling=%.9f\n", n, W, top, (int)(on != off), std::pow(10.0, -2.0 / 20.0));
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
