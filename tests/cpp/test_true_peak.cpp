// SynthesisConfig::truePeak through the piper:: API: textToAudio on a sentence of two phrases with targetLufs and truePeak
// set, the kind read back from the engine (pe_get_loudness_ceiling) and every phrase's true peak (pe_last_true_peak); then
// truePeak cleared, and set again without targetLufs (the engine remembers the kind).
//   usage: test_true_peak <voice.onnx>
// Prints one `phrase i t=... p=... scale=... flags=...` line per phrase and `OK ...`; the pytest wrapper checks them.
#include <cmath>
#include <cstdio>
#include <iostream>

#include "piper.hpp"
#include "piper_hip.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_true_peak voice.onnx\n";
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
    if (sc.truePeak) {
      std::cerr << "ERROR: truePeak is not false by default\n";
      return 1;
    }

    std::vector<int16_t> sample, tp, again;
    piper::SynthesisResult r;
    int32_t kind = -1, q = -1, k = -1, n = -1;
    sc.targetLufs = -5.0f;
    sc.peakCeilingDb = -2.0f;
    piper::textToAudio(config, voice, text, sample, r, nullptr);
    float t[8], L[8], scale[8], peak[8];
    int32_t flags[8];
    if (pe_get_loudness_ceiling(voice.session.engine, &kind, &q, &k) || kind != PE_PEAK_SAMPLE ||
        pe_last_true_peak(voice.session.engine, t, 8, &n) || n != 0) {
      std::cerr << "ERROR: the true-peak kind is on without truePeak\n";
      return 1;
    }

    sc.truePeak = true;
    piper::textToAudio(config, voice, text, tp, r, nullptr);
    if (pe_get_loudness_ceiling(voice.session.engine, &kind, &q, &k) || kind != PE_PEAK_TRUE) {
      std::cerr << "ERROR: truePeak did not reach the engine\n";
      return 1;
    }
    if (pe_last_true_peak(voice.session.engine, t, 8, &n) || n != 2 ||
        pe_last_loudness(voice.session.engine, L, scale, peak, flags, 8, &n) || n != 2) {
      std::cerr << "ERROR: expected the report of two phrases, got " << n << ": " << pe_last_error() << "\n";
      return 1;
    }
    for (int i = 0; i < n; ++i) std::printf("phrase %d t=%.6f p=%.6f scale=%.4f flags=%d\n", i, t[i], peak[i], scale[i], flags[i]);
    if (tp.size() != sample.size()) {
      std::cerr << "ERROR: the kind changed the length\n";
      return 1;
    }

    sc.truePeak = false;
    piper::textToAudio(config, voice, text, again, r, nullptr);
    int32_t m = -1;
    if (pe_get_loudness_ceiling(voice.session.engine, &kind, nullptr, nullptr) || kind != PE_PEAK_SAMPLE || again != sample ||
        pe_last_true_peak(voice.session.engine, nullptr, 0, &m) || m != 0) {
      std::cerr << "ERROR: clearing truePeak does not give the sample-peak ceiling back\n";
      return 1;
    }
    sc.targetLufs.reset();
    sc.truePeak = true;
    piper::textToAudio(config, voice, text, again, r, nullptr);
    int32_t on = 1;
    if (pe_get_loudness(voice.session.engine, &on, nullptr, nullptr) || on ||
        pe_get_loudness_ceiling(voice.session.engine, &kind, nullptr, nullptr) || kind != PE_PEAK_TRUE) {
      std::cerr << "ERROR: truePeak without targetLufs is not remembered by the engine\n";
      return 1;
    }
    std::printf("OK phrases=%d oversample=%d half_width=%d ceiling=%.9f\n", n, q, k, std::pow(10.0, -2.0 / 20.0));
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
