// SynthesisConfig::sampleFormat through the piper:: API: synthesizeEncoded and textToEncodedAudio against synthesize and
// textToAudio passed through the host twin pe_g711_encode (bit for bit, silences included), the silence bytes themselves
// (0xFF mu-law, 0xD5 A-law), the G.711 header textToWavFile writes, the refusal under S16, and S16 given back afterwards.
//   usage: test_g711 <voice.onnx>
// Prints one `law ... ` line per law and `OK`; the pytest wrapper checks them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

#include "piper.hpp"
#include "piper_hip.h"

static uint32_t le(const std::string& s, size_t at, int bytes) {
  uint32_t v = 0;
  for (int i = 0; i < bytes; ++i) v |= (uint32_t)(unsigned char)s[at + i] << (8 * i);
  return v;
}

static int fail(const std::string& what) {
  std::cerr << "ERROR: " << what << "\n";
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_g711 voice.onnx\n";
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
    sc.lengthScale = 1.0f;
    sc.sentenceSilenceSeconds = 0.01f;
    sc.phonemeSilenceSeconds.emplace();
    (*sc.phonemeSilenceSeconds)[U','] = 0.005f;
    const char* text = "abcdefgh abc, hgfedcba";
    const size_t sentenceSilence = (size_t)(0.01f * sc.sampleRate), phraseSilence = (size_t)(0.005f * sc.sampleRate);
    if (sc.sampleFormat != piper::S16 || sc.sampleWidth != 2) return fail("the sample format is not S16 / 2 bytes by default");

    std::vector<std::vector<piper::Phoneme>> sentences;
    piper::phonemize_codepoints("abcdefgh", sentences);
    std::vector<piper::PhonemeId> ids;
    std::map<piper::Phoneme, std::size_t> missing;
    piper::phonemes_to_ids(sentences[0], voice.phonemizeConfig, ids, missing);

    piper::SynthesisResult r;
    std::vector<int16_t> one, all;
    piper::synthesize(ids, sc, voice.session, one, r);
    piper::textToAudio(config, voice, text, all, r, nullptr);
    if (one.empty() || all.size() <= one.size()) return fail("nothing synthesized");
    std::vector<uint8_t> none;
    bool threw = false;
    try {
      piper::textToEncodedAudio(config, voice, text, none, r, nullptr);
    } catch (const std::exception&) {
      threw = true;
    }
    if (!threw || !none.empty()) return fail("textToEncodedAudio under S16 did not throw");
    std::ostringstream pcmWav;
    piper::textToWavFile(config, voice, text, pcmWav, r);
    if (pcmWav.str().size() != 44 + 2 * all.size() || le(pcmWav.str(), 20, 2) != 1 || le(pcmWav.str(), 34, 2) != 16)
      return fail("the S16 WAV is not the 44-byte PCM header and the int16");

    const struct { piper::SampleFormat fmt; int32_t pe; uint8_t zero; uint32_t tag; const char* name; } laws[2] = {
        {piper::MuLaw, PE_FORMAT_ULAW, 0xFF, 7, "ulaw"}, {piper::ALaw, PE_FORMAT_ALAW, 0xD5, 6, "alaw"}};
    for (const auto& law : laws) {
      sc.sampleFormat = law.fmt;
      std::vector<uint8_t> want1(one.size()), wantAll(all.size()), got1, gotAll;
      if (pe_g711_encode(law.pe, one.data(), want1.data(), (int64_t)one.size()) ||
          pe_g711_encode(law.pe, all.data(), wantAll.data(), (int64_t)all.size()))
        return fail(pe_last_error());
      piper::synthesizeEncoded(ids, sc, voice.session, got1, r);
      int32_t fmt = -1;
      if (pe_get_sample_format(voice.session.engine, &fmt) || fmt != law.pe) return fail("sampleFormat did not reach the engine");
      if (got1 != want1) return fail(std::string("synthesizeEncoded differs from g711(synthesize), ") + law.name);
      int calls = 0;
      std::vector<uint8_t> streamed;
      piper::textToEncodedAudio(config, voice, text, gotAll, r, [&]() {
        ++calls;
        streamed.insert(streamed.end(), gotAll.begin(), gotAll.end());
      });
      if (calls != 1 || streamed != wantAll) return fail(std::string("textToEncodedAudio with a callback differs, ") + law.name);
      gotAll.clear();
      piper::textToEncodedAudio(config, voice, text, gotAll, r, nullptr);
      if (gotAll != wantAll) return fail(std::string("textToEncodedAudio differs from g711(textToAudio), ") + law.name);
      // the silences are the law's zero code: the sentence's at the end, the phrase's behind the comma
      size_t zeros = 0;
      for (size_t i = gotAll.size() - sentenceSilence; i < gotAll.size(); ++i) zeros += gotAll[i] == law.zero;
      if (sentenceSilence == 0 || zeros != sentenceSilence) return fail(std::string("sentence silence is not the zero code, ") + law.name);
      size_t run = 0, longest = 0;
      for (size_t i = 0; i + sentenceSilence < gotAll.size(); ++i) {
        run = gotAll[i] == law.zero ? run + 1 : 0;
        longest = std::max(longest, run);
      }
      if (phraseSilence == 0 || longest < phraseSilence) return fail(std::string("phoneme silence is not the zero code, ") + law.name);
      // the header written by hand
      std::ostringstream wav;
      piper::textToWavFile(config, voice, text, wav, r);
      const std::string w = wav.str();
      const size_t n = wantAll.size(), pad = n & 1;
      if (w.size() != 58 + n + pad || w.compare(0, 4, "RIFF") || le(w, 4, 4) != w.size() - 8 || w.compare(8, 8, "WAVEfmt ") ||
          le(w, 16, 4) != 18 || le(w, 20, 2) != law.tag || le(w, 22, 2) != 1 || le(w, 24, 4) != (uint32_t)sc.sampleRate ||
          le(w, 28, 4) != (uint32_t)sc.sampleRate || le(w, 32, 2) != 1 || le(w, 34, 2) != 8 || le(w, 36, 2) != 0 ||
          w.compare(38, 4, "fact") || le(w, 42, 4) != 4 || le(w, 46, 4) != n || w.compare(50, 4, "data") || le(w, 54, 4) != n ||
          memcmp(w.data() + 58, wantAll.data(), n) != 0)
        return fail(std::string("the G.711 WAV header or data is wrong, ") + law.name);
      if (sc.sampleWidth != 2) return fail("sampleWidth moved");
      std::printf("law %s tag=%u samples=%zu one=%zu zero=0x%02X silence=%zu\n", law.name, law.tag, n, got1.size(), law.zero, zeros);
    }
    // back to S16: the int16 as before, and the engine's format cleared
    sc.sampleFormat = piper::S16;
    std::vector<int16_t> again;
    piper::textToAudio(config, voice, text, again, r, nullptr);
    int32_t fmt = -1;
    if (again != all || pe_get_sample_format(voice.session.engine, &fmt) || fmt != PE_FORMAT_S16)
      return fail("S16 afterwards is not what it was");
    std::printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
