// SynthesisConfig::targetLufs / peakCeilingDb through the piper:: API: textToAudio on a sentence of two phrases with the
// target set, every phrase's report read back from the engine (pe_last_loudness), then the same with the field cleared.
//   usage: test_loudness <voice.onnx>
// Prints one `phrase i L=... scale=... peak=... flags=...` line per phrase and `OK ...`; the pytest wrapper checks them.
#include <cmath>
#include <cstdio>
#include <iostream>

#include "piper.hpp"
#include "piper_hip.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_loudness voice.onnx\n";
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

    std::vector<int16_t> plain, loud, again;
    piper::SynthesisResult r;
    piper::textToAudio(config, voice, text, plain, r, nullptr);
    int32_t on = 1, n = -1;
    float t = 0.f, c = 0.f;
    if (pe_get_loudness(voice.session.engine, &on, &t, &c) || on) {
      std::cerr << "ERROR: the setting is on without targetLufs\n";
      return 1;
    }

    const float T = -24.0f;
    sc.targetLufs = T;
    sc.peakCeilingDb = -1.5f;
    piper::textToAudio(config, voice, text, loud, r, nullptr);
    if (pe_get_loudness(voice.session.engine, &on, &t, &c) || !on || t != T || c != -1.5f) {
      std::cerr << "ERROR: targetLufs did not reach the engine\n";
      return 1;
    }
    float L[8], scale[8], peak[8];
    int32_t flags[8];
    if (pe_last_loudness(voice.session.engine, L, scale, peak, flags, 8, &n) || n != 2) {
      std::cerr << "ERROR: expected the report of two phrases, got " << n << ": " << pe_last_error() << "\n";
      return 1;
    }
    int at_target = 0;
    for (int i = 0; i < n; ++i) {
      std::printf("phrase %d L=%.6f scale=%.4f peak=%.6f flags=%d\n", i, L[i], scale[i], peak[i], flags[i]);
      // what the phrase is delivered at: its loudness plus the gain relative to full scale
      const double delivered = (double)L[i] + 20.0 * std::log10((double)scale[i] / 32767.0);
      if (flags[i] & (PE_LOUD_LIMITED | PE_LOUD_SHORT | PE_LOUD_UNMEASURABLE)) continue;
      if (std::fabs(delivered - (double)T) > 1e-3) {
        std::cerr << "ERROR: phrase " << i << " is delivered at " << delivered << " LUFS, not " << T << "\n";
        return 1;
      }
      ++at_target;
    }
    if (loud.size() != plain.size() || loud == plain) {
      std::cerr << "ERROR: the target changed the length, or nothing at all\n";
      return 1;
    }

    sc.targetLufs.reset();
    piper::textToAudio(config, voice, text, again, r, nullptr);
    if (pe_get_loudness(voice.session.engine, &on, &t, &c) || on || again != plain) {
      std::cerr << "ERROR: clearing targetLufs does not give the default back\n";
      return 1;
    }
    std::printf("OK phrases=%d at_target=%d samples=%zu\n", n, at_target, loud.size());
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
