// SynthesisConfig::seed through the piper:: API: phrase k of a textToAudio call, counted over the whole text, draws from
// seed + k (wrapping at 2^64); utterance k of synthesizeBatch likewise; synthesize takes the seed as it is, gives the same
// PCM again whatever the engine served in between, and another PCM without the seed.
//   usage: test_seeds <voice.onnx>          (with PIPER_HIP_DEBUG_KEEP=1: the noise tensors are read back)
// What a phrase drew is its duration noise (pe_debug_tensor "noise_w") against pe_debug_randn(site 0, counter 0, row = channel)
// under pe_set_seed(that phrase's seed) -- the law of include/piper_hip.h (pe_seeds). Prints one `phrase ...` / `utterance ...`
// line each and `OK ...`; the pytest wrapper checks them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "piper.hpp"
#include "piper_hip.h"

// whether utterance b of the engine's last call drew its duration noise from `seed`; *ids receives its id count
static bool drew_from(pe_engine* e, int b, uint64_t seed, int* ids) {
  std::vector<float> nw(2 * 8192), ref(8192);
  int32_t rows = 0, cols = 0;
  if (pe_debug_tensor(e, "noise_w", b, nw.data(), (int64_t)nw.size(), &rows, &cols) || rows != 2 || cols < 1) {
    std::cerr << "ERROR: noise_w of utterance " << b << ": " << pe_last_error() << "\n";
    std::exit(1);
  }
  *ids = cols;
  pe_set_seed(e, seed);
  bool same = true;
  for (int c = 0; c < 2; ++c) {
    if (pe_debug_randn(e, 0, 0, c, cols, ref.data())) {
      std::cerr << "ERROR: pe_debug_randn: " << pe_last_error() << "\n";
      std::exit(1);
    }
    same = same && !std::memcmp(ref.data(), nw.data() + (size_t)c * cols, (size_t)cols * sizeof(float));
  }
  return same;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: test_seeds voice.onnx\n";
    return 2;
  }
  try {
    piper::PiperConfig config;
    piper::Voice voice;
    std::optional<piper::SpeakerId> speaker;
    piper::loadVoice(config, argv[1], std::string(argv[1]) + ".json", voice, speaker, false);
    piper::initialize(config);
    piper::SynthesisConfig& sc = voice.synthesisConfig;
    if (sc.seed) {
      std::cerr << "ERROR: a seed is set by default\n";
      return 1;
    }
    sc.phonemeSilenceSeconds.emplace();
    (*sc.phonemeSilenceSeconds)[U','] = 0.01f;
    pe_engine* e = voice.session.engine;
    piper::SynthesisResult r;

    // three phrases from the last seed there is: seed, then 0, then 1
    const uint64_t top = ~(uint64_t)0;
    sc.seed = top;
    std::vector<int16_t> text_pcm;
    piper::textToAudio(config, voice, "abcdefgh, hgfedc, abc", text_pcm, r, nullptr);
    int ok = 1;
    for (int k = 0; k < 3; ++k) {
      int n = 0;
      const uint64_t want = top + (uint64_t)k;
      const bool m = drew_from(e, k, want, &n), other = drew_from(e, k, want + 1, &n);
      std::printf("phrase %d ids=%d seed=%llu match=%d next=%d\n", k, n, (unsigned long long)want, (int)m, (int)other);
      ok = ok && m && !other;
    }

    // synthesizeBatch: utterance k gets seed + k
    sc.seed = 100;
    std::vector<std::vector<piper::PhonemeId>> lists = {{1, 0, 10, 0, 11, 0, 2}, {1, 0, 12, 0, 13, 0, 14, 0, 2}};
    std::vector<std::vector<int16_t>> pcm2;
    piper::synthesizeBatch(lists, sc, voice.session, pcm2, r);
    for (int k = 0; k < 2; ++k) {
      int n = 0;
      const bool m = drew_from(e, k, 100 + (uint64_t)k, &n);
      std::printf("utterance %d ids=%d seed=%d match=%d\n", k, n, 100 + k, (int)m);
      ok = ok && m && n == (int)lists[k].size();
    }

    // synthesize: the seed as it is; the same PCM again behind other calls; another PCM without it
    std::vector<piper::PhonemeId> ids = {1, 0, 10, 0, 11, 0, 12, 0, 2};
    std::vector<int16_t> a, b, plain, c;
    sc.seed = 7;
    piper::synthesize(ids, sc, voice.session, a, r);
    int n = 0;
    const bool m7 = drew_from(e, 0, 7, &n);
    sc.seed.reset();
    piper::synthesize(ids, sc, voice.session, plain, r);
    sc.seed = 7;
    piper::synthesize(ids, sc, voice.session, b, r);
    sc.seed = 8;
    piper::synthesize(ids, sc, voice.session, c, r);
    std::printf("OK phrases=%d law=%d one=%d repeat=%d plain_differs=%d other_seed_differs=%d samples=%zu\n", 3, ok, (int)m7, (int)(a == b),
                (int)(a != plain), (int)(a != c), a.size());
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "EXCEPTION: " << e.what() << "\n";
    return 1;
  }
}
