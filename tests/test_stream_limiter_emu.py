"""Look-ahead limiter on streams at a target loudness (pe_set_stream_limiter: every stream holds back 2 W samples and delivers
the envelope a whole-stream computation would give) on the test-only emulator build of the engine, the activation workspaces
and the stream state poisoned. The contract is restated in f64 in tests/stream_limiter_case.py. Kernel cases go through the
debug entry on rows of a few thousand samples; engine cases run on the tiny voices with the inputs of
tests/emu/stream_batch_case.py. The GPU twin is tests/test_gpu_stream_limiter.py (-m gpu)."""
import os
import subprocess
import sys

import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import stream_batch_case as K                            # noqa: E402
import stream_limiter_case as M                          # noqa: E402
import stream_pool_case as P                             # noqa: E402

# the target at which the tiny voices' streams are shaped (their loudness lies near -16 LUFS with peaks near 0.5; the
# multi-speaker voice of the pool is softer), and one at which nothing is LIMITED
T, T_POOL, T_FREE, CEIL, RAMP, MS = -12.0, -8.0, -40.0, -1.0, 64, 5.0


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(emu_lib, preset="tiny"):
    """An engine whose workspaces and stream state are poisoned with NaN patterns before use (read at creation)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PIPER_HIP_DEBUG_POISON", "1")
        cfg = W.preset(preset)
        return cfg, Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), lib=emu_lib)


@pytest.fixture(scope="module")
def tiny(emu_lib):
    cfg, eng = _engine(emu_lib)
    yield cfg, eng, K.inputs(cfg)
    eng.close()


# ---- 1. composition at a constant gain
@pytest.mark.parametrize("ramp", (0, 96))
@pytest.mark.parametrize("fs,window_ms", M.CASES)
def test_cuts_compose_at_a_constant_gain(tiny, fs, window_ms, ramp):
    M.check_const(tiny[1], fs, window_ms, ramp)


# ---- 2. varying gain
@pytest.mark.parametrize("fs", (8000, 22050))
def test_varying_gain(tiny, fs):
    M.check_varying(tiny[1], fs)


# ---- 3. what it is for
@pytest.mark.parametrize("fs", (8000, 16000, 48000))
def test_one_click_no_longer_sets_the_level(tiny, fs):
    M.check_feature(tiny[1], fs)


# ---- 4. engine streams
def _rated(emu_lib, rate, preset="tiny"):
    cfg, eng = _engine(emu_lib, preset)
    if rate:
        eng.set_output_rate(rate)
    return cfg, eng


# (a chunk of one frame costs the emulator a second per call: that case runs at the native rate on the two shorter
# utterances here, at every rate and on all three in the GPU twin)
@pytest.mark.parametrize("rate,chunk,window_ms", [(None, 4, MS), (None, 1, 10.0), (8000, 4, MS), (48000, 4, MS)])
def test_batch_stream(emu_lib, rate, chunk, window_ms):
    cfg, eng = _rated(emu_lib, rate)
    ids, nw, nz = K.inputs(cfg)
    n = 2 if chunk == 1 else 3
    inputs = (ids[:n], nw[:n], nz[:n])
    shaped, out, _ = M.check_batch(eng, inputs, chunk, K.SCALES[:n], T, CEIL, RAMP, window_ms, ("batch", rate, chunk))
    print(f"\nbatch stream at {eng.output_rate} Hz, chunks of {chunk}, T {T}: shaped samples {shaped}, "
          f"delivered per call {[st.dl for st, _ in out]}")
    assert shaped > 0, "vacuous: nothing was shaped"
    if chunk == 1:
        # D exceeds the chunk: the first call delivers nothing and the stream goes on
        assert all(st.D > st.n[0] and st.dl[0] == 0 and sum(st.dl) == sum(st.n) for st, _ in out)
    eng.close()


def test_batch_stream_that_is_never_limited_is_mode_3(emu_lib):
    cfg, eng = _rated(emu_lib, None)
    _, out, base = M.check_batch(eng, K.inputs(cfg), K.CHUNK, K.SCALES, T_FREE, CEIL, RAMP, MS, ("batch", "free"))
    M.check_unlimited(out, base, "batch")
    eng.close()


@pytest.mark.parametrize("rate", (None, 8000, 48000))
def test_one_utterance_stream(emu_lib, rate):
    cfg, eng = _rated(emu_lib, rate)
    shaped, _, _ = M.check_one(eng, K.inputs(cfg), 2, K.CHUNK, K.SCALES, T, CEIL, RAMP, MS, ("one", rate))
    print(f"\none-utterance stream at {eng.output_rate} Hz, T {T}: shaped samples {shaped}")
    assert shaped > 0, "vacuous: nothing was shaped"
    if rate is None:
        _, (st, (X, Pc, s)), base = M.check_one(eng, K.inputs(cfg), 1, K.CHUNK, K.SCALES, T_FREE, CEIL, RAMP, MS, ("one", "free"))
        M.check_unlimited([(st, (X, Pc, s))], [base], "one")
    eng.close()


@pytest.mark.parametrize("rate", (None, 8000, 48000))
def test_pool(emu_lib, rate):
    """A join in mid-stream with a first chunk of its own, a whole-utterance call and a batch that grows both workspaces (and
    poisons them again) between two chunks, a listener that hangs up in mid-stream and another speaker in its slot."""
    cfg, eng = _rated(emu_lib, rate, "tiny-ms")
    big = [W.synthetic_phoneme_ids(n, 90 + i, id_max=cfg.n_vocab - 1) for i, n in enumerate((136, 3, 4, 5))]
    t3 = P.emu_texts(cfg, True)[3]

    def between(k):
        if k == 0:
            eng.synthesize(t3.ids, t3.scales, sid=t3.sid)
        else:
            eng.synthesize_batch(big, (0.667, 0.3, 0.8))

    shaped = M.check_pool(eng, lambda: P.emu_texts(cfg, True), P.join, K.CHUNK, T_POOL, CEIL, RAMP, MS, between, ("pool", rate))
    print(f"\npool at {eng.output_rate} Hz, T {T_POOL}: shaped samples {shaped}")
    assert shaped > 0, "vacuous: nothing was shaped"
    eng.close()


# ---- 5. refusals and idempotence
def test_refusals(emu_lib):
    M.check_refusals(lambda preset="tiny": _engine(emu_lib, preset), emu_lib, K, P,
                     lambda: Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), lib=emu_lib))


def test_on_and_off_again_leaves_mode_3_as_it_was(emu_lib):
    cfg, eng = _engine(emu_lib)
    M.check_idempotence(eng, K.inputs(cfg), K.CHUNK, K.SCALES, T, CEIL, RAMP, MS)
    eng.close()
