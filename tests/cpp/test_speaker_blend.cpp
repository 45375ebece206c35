// SynthesisConfig::speakerBlend and ::speakerVector through the piper:: API, at noise scales 0 so that every call is a
// function of its inputs alone: the unit blend {(s, 1)} and the table row of s as a vector give the PCM of speakerId = s in
// synthesize; a real blend gives another PCM; synthesizeBatch gives every utterance its own blended synthesize; textToAudio
// speaks its phrases with the vector; both fields together, or either one beside speakerId, throw.
//   usage: test_speaker_blend <multi-speaker voice.onnx>
// Prints `OK ...`; the pytest wrapper checks it.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "piper.hpp"
#include "piper_hip.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_speaker_blend voice.onnx\n";
    return 2;
  }
  try {
    piper::PiperConfig config;
    piper::Voice voice;
    std::optional<piper::SpeakerId> speaker;
    piper::loadVoice(config, argv[1], std::string(argv[1]) + ".json", voice, speaker, false);
    piper::initialize(config);
    piper::SynthesisConfig& sc = voice.synthesisConfig;
    if (!sc.speakerBlend.empty() || !sc.speakerVector.empty()) {
      std::cerr << "ERROR: a blend is set by default\n";
      return 1;
    }
    sc.noiseScale = 0.f;
    sc.noiseW = 0.f;
    sc.lengthScale = 0.4f;          // (short utterances: the emulator runs the vocoder slowly)
    pe_engine* e = voice.session.engine;
    piper::SynthesisResult r;
    int32_t gin = 0;
    if (pe_get_speaker_dim(e, &gin) || gin < 1) {
      std::cerr << "ERROR: not a multi-speaker voice\n";
      return 1;
    }
    std::vector<float> row((size_t)gin);
    if (pe_get_speaker_embedding(e, 2, row.data(), gin)) {
      std::cerr << "ERROR: " << pe_last_error() << "\n";
      return 1;
    }
    const std::vector<std::pair<piper::SpeakerId, float>> mix = {{1, 0.7f}, {3, 0.3f}};

    std::vector<piper::PhonemeId> ids = {1, 10, 2};
    std::vector<int16_t> plain, unit, vec, blended;
    sc.speakerId = 2;
    piper::synthesize(ids, sc, voice.session, plain, r);
    sc.speakerId.reset();
    sc.speakerBlend = {{2, 1.0f}};
    piper::synthesize(ids, sc, voice.session, unit, r);
    sc.speakerBlend.clear();
    sc.speakerVector = row;
    piper::synthesize(ids, sc, voice.session, vec, r);
    sc.speakerVector.clear();
    sc.speakerBlend = mix;
    piper::synthesize(ids, sc, voice.session, blended, r);

    // synthesizeBatch: every utterance is its own blended synthesize
    std::vector<std::vector<piper::PhonemeId>> lists = {{1, 2}, ids};
    std::vector<std::vector<int16_t>> pcm2;
    piper::synthesizeBatch(lists, sc, voice.session, pcm2, r);
    const bool batch = pcm2.size() == 2 && !pcm2[0].empty() && pcm2[0] != blended && pcm2[1] == blended;

    // textToAudio: the vector speaks the phrase as speakerId does (an ignored vector would leave speaker 0)
    std::vector<int16_t> text_vec, text_plain;
    sc.speakerBlend.clear();
    sc.speakerVector = row;
    piper::textToAudio(config, voice, "a", text_vec, r, nullptr);
    sc.speakerVector.clear();
    sc.speakerId = 2;
    piper::textToAudio(config, voice, "a", text_plain, r, nullptr);
    const bool text = !text_vec.empty() && text_vec == text_plain;

    // the refused combinations
    int refused = 0;
    std::vector<int16_t> none;
    for (int k = 0; k < 3; ++k) {
      sc.speakerId.reset();
      sc.speakerBlend.clear();
      sc.speakerVector.clear();
      if (k != 2) sc.speakerId = 1;
      if (k != 1) sc.speakerBlend = mix;
      if (k != 0) sc.speakerVector = row;
      try {
        piper::synthesize(ids, sc, voice.session, none, r);
      } catch (const std::exception&) {
        refused += none.empty() ? 1 : 0;
      }
    }
    std::printf("OK unit=%d row=%d blend_differs=%d batch=%d text=%d refused=%d samples=%zu\n", (int)(unit == plain), (int)(vec == plain),
                (int)(blended != plain), (int)batch, (int)text, refused, plain.size());
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
