"""One gain across a stream's chunks on the MI355X (run with -m gpu): pe_set_stream_gain through
piper_amd.engine.Engine.set_stream_gain on the small shapes of tests/test_gpu_stream_batch.py -- tiny (9, 17, 26, 38, 50 ids,
chunks of 7 frames) and medium (32, 48, 64 ids, chunks of 45). The rule is the float32 restatement of
tests/emu/stream_gain_case.py applied to the floats the engine delivers: int16 equal outside ramps, within one inside them.
The emulator counterpart, with poisoned workspaces, the error cases and the untouched default, is
tests/test_stream_gain_emu.py."""
import os
import sys

import numpy as np
import pytest

from piper_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import stream_gain_case as G                             # noqa: E402
import stream_pool_case as P                             # noqa: E402
import test_gpu_stream_batch as S                        # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"tiny": ((9, 17, 26, 38, 50), 7), "medium": ((32, 48, 64), 45)}
F32 = np.float32
_engines = {}


def engine_for(preset):
    """Engines of this module's own: the gain setting is the handle's, and the other GPU tests share theirs."""
    from piper_amd.engine import Engine
    if preset not in _engines:
        cfg = W.preset(preset)
        _engines[preset] = (cfg, Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0))
    return _engines[preset]


def drain(eng, ids, nw, nz, chunk):
    return G.drain(eng, ids, nw, nz, chunk, S.SCALES)


@pytest.mark.parametrize("preset", list(CASES))
def test_running_level_ragged_batch_and_one_utterance_stream(preset):
    """The running mode without prior and ramp: every chunk is the restatement, the reported peaks are the running maxima
    and end at the maximum of everything delivered, the gains never rise, behind the peak chunk the int16 is the whole
    call's (1e-3 RMS), finished utterances keep reporting their state, and chunk k of utterance b is the one-utterance
    stream's chunk k in the same mode."""
    lens, chunk = CASES[preset]
    cfg, eng = engine_for(preset)
    ids, nw, nz = S.inputs_for(cfg, lens)
    eng.set_stream_gain("running", 0.0, 0.0)
    try:
        per, rep, calls = drain(eng, ids, nw, nz, chunk)
        full = eng.synthesize_batch(ids, S.SCALES, noise_w=nw, noise_z=nz)
        nchunks = [len(c) for c in per]
        assert nchunks == [-(-int(f) // chunk) for f in full.frames] and len(set(nchunks)) > 1, nchunks
        G.check_running_behaviour(per, rep, full.pcm, S.RMS_TOL, preset)
        G.check_finished_rows_keep_their_state(rep, calls)
        behind = sum(len(G.after_peak(c)) for c in per)
        print(f"\n[{preset}] chunks {nchunks}, {behind} behind their utterance's peak chunk, final peaks "
              f"{[round(float(r[-1][1]), 3) for r in rep]}")
        assert behind >= 1
        for b in range(len(lens)):
            one, rep1 = [], []
            for a, p in eng.stream(ids[b], S.SCALES, chunk_frames=chunk, noise_w=nw[b], noise_z=nz[b]):
                one.append((a, p))
                g1, p1 = eng.stream_last_gains()
                rep1.append((g1[0], p1[0]))
            assert len(one) == len(per[b]), b
            G.check_stream(one, "running", 0.0, 0, reports=rep1, where=(preset, "one", b))
            for k, ((a, p), (a1, p1)) in enumerate(zip(per[b], one)):
                assert a.shape == a1.shape and np.max(np.abs(a - a1)) < S.CHUNK_TOL, (b, k)
                assert G.pcm_rms(p, p1) <= S.RMS_TOL, (b, k)
    finally:
        eng.set_stream_gain("chunk")


@pytest.mark.parametrize("preset", list(CASES))
def test_ramp_of_64_samples(preset):
    lens, chunk = CASES[preset]
    cfg, eng = engine_for(preset)
    ids, nw, nz = S.inputs_for(cfg, lens)
    eng.set_stream_gain("running", 0.0, 64 * 1000.0 / eng.output_rate)
    try:
        assert eng.stream_gain == ("running", 0.0, 64)
        per, rep, _ = drain(eng, ids, nw, nz, chunk)
        G.check_ramps(per, rep, 64, preset)
    finally:
        eng.set_stream_gain("chunk")


@pytest.mark.parametrize("preset", list(CASES))
def test_at_8000_hz(preset):
    """Both of the above through the resampled conversion: peaks and ramps count in output samples."""
    lens, chunk = CASES[preset]
    cfg, eng = engine_for(preset)
    ids, nw, nz = S.inputs_for(cfg, lens)
    eng.set_output_rate(8000)
    try:
        eng.set_stream_gain("running", 0.0, 0.0)
        per, rep, calls = drain(eng, ids, nw, nz, chunk)
        full = eng.synthesize_batch(ids, S.SCALES, noise_w=nw, noise_z=nz)
        assert per[-1][0][0].size == -(-chunk * eng.hop * 8000 // cfg.sample_rate)
        G.check_running_behaviour(per, rep, full.pcm, S.RMS_TOL, (preset, 8000))
        G.check_finished_rows_keep_their_state(rep, calls)
        eng.set_stream_gain("running", 0.0, 64 * 1000.0 / 8000)
        assert eng.stream_gain == ("running", 0.0, 64)
        per, rep, _ = drain(eng, ids, nw, nz, chunk)
        G.check_ramps(per, rep, 64, (preset, 8000))
    finally:
        eng.set_stream_gain("chunk")
        eng.set_output_rate(0)


def test_pool_levels_are_per_slot_and_resident():
    """Four slots on the multi-speaker tiny voice, four speakers (tests/emu/stream_gain_case.py: pool_scenario): joins in
    mid-stream, a whole-utterance call and a larger batch between two chunks, a join without room, a finished tenant's and a
    departed listener's slot reused -- every chunk held to its own slot's level."""
    from piper_amd.engine import Engine
    cfg = W.preset("tiny-ms")
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    lens, chunk = (9, 17, 38, 17), 7
    scales = (0.667, 0.3, 0.8)
    ids, nw, nz = S.inputs_for(cfg, lens)
    sids = (1, 3, 0, 2)
    frames = eng.synthesize_batch(ids, scales, sids=list(sids), noise_w=nw, noise_z=nz).frames
    assert frames[0] < frames[1] < frames[2] and frames[0] > 2 * chunk, frames

    def make_texts():
        return [P.Listener("ids%d/%d" % (lens[i], i), ids[i], scales, sids[i], nw[i][:, :lens[i]], nz[i]) for i in range(4)]

    big = [W.synthetic_phoneme_ids(T, 90 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate((136, 3, 4, 5, 6, 7))]

    def between(k):
        if k == 0:
            eng.synthesize(ids[3], scales, sid=2)
        else:
            eng.synthesize_batch(big, scales)

    G.pool_scenario(eng, make_texts, P.join, 4, int(frames.max()), chunk, 0.05, 64, between, S.CHUNK_TOL, S.RMS_TOL)
    eng.close()


def test_a_steady_server_stops_capturing_in_every_mode():
    """pe_graph_stats: a second identical stream captures nothing in any mode, and neither does a change of peak or ramp
    alone -- they are data in the control block, not kernel arguments."""
    lens, chunk = CASES["tiny"]
    cfg, eng = engine_for("tiny")
    ids, nw, _ = S.inputs_for(cfg, lens)

    def stream():
        # injected duration noise fixes the frame counts (and with them the buckets), the prior noise is the engine's:
        # every stage of the stream is a captured graph
        for _ in eng.stream_batch(ids, S.SCALES, chunk_frames=chunk, noise_w=nw):
            pass
        return eng.graph_stats[1]

    try:
        seen = []
        for mode, peak in (("chunk", 0.0), ("running", 0.0), ("fixed", 0.5)):
            eng.set_stream_gain(mode, peak, 0.0)
            c1 = stream()
            c2 = stream()
            eng.set_stream_gain(mode, 0.25, 3.0)
            c3 = stream()
            eng.set_stream_gain(mode, 0.7, 0.0)
            c4 = stream()
            seen.append((mode, c1, c2, c3, c4))
            assert c1 > 0 and c2 == c1 and c3 == c1 and c4 == c1, seen
        # ... and back in a mode that has been seen: its graphs are still there
        eng.set_stream_gain("running", 0.0, 0.0)
        assert stream() == seen[-1][1], seen
        print(f"\ncaptures per mode (first stream, second, other peak and ramp, again): {seen}")
    finally:
        eng.set_stream_gain("chunk")
