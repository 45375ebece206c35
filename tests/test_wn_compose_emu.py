"""PIPER_HIP_WN_COMPOSE on the kernel emulator: a coupling layer's pre composed into its first gate conv (gate4pre_kernel,
kernels/gate4.h) and the hidden state written whole by the first res/skip launch (colchain4_kernel mode 2 with w2). No GPU.

The 192-hidden, 96-half tiny voice and a multi-speaker override of it (gin 16: the speaker bias must reach the composed gate
conv), PIPER_HIP_DEBUG_POISON=1 throughout. Frame counts are forced through the timing plan, so the shapes are
certain: 1 .. 5 frames (every way the two edge corrections of pre's bias overlap: padl = 2 of 5 taps), 12 and 13 (one past a
12-column gate tile), 37, and a ragged call of 3 and 13 frames. Duration noise and prior noise are injected, so every knob
value sees the same z_p. For each case and each knob value 1, 2, 3: z and audio meet the f64 truth gates of
tests/one_utterance_truth_case.py (stages F and G from the engine's own z_p and z, K = 8); durations, noise_z and z_p equal
knob 0's bit for bit. The launch maps: knob 0 runs flow_n * wn_layers gate4_kernel launches and no gate4pre_kernel; knob 1 and
2 run one colchain4_kernel<false> launch fewer (the first coupling layer's pre), flow_n gate4pre_kernel launches in place of as
many gate4_kernel launches, and still gate4_kernel and colchain4_kernel<true>; knob 3 (post into the skip convs: not built)
runs knob 0's launches and gives its bits.

Mutation check (by hand, profiles/wn_compose.md): with the edge branch of gate4_body's epilogue disabled (every workgroup adds
the full bias sum) the cases of 1 .. 5 and 13 frames fail their z gates; 12 and 37 fail too, their last columns lie in a
workgroup whose taps reach past L."""
import os
import subprocess

import numpy as np
import pytest

import one_utterance_truth_case as U
from piper_amd import _lib as L
from piper_amd.engine import Timing

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
TARGET = "emu"
U.WIDE.setdefault("tiny192-ms", dict(U.WIDE["tiny192"], n_speakers=4, gin=16))
KNOBS = (0, 1, 2, 3)
FLOW = ("gate4_kernel", "gate4pre_kernel", "colchain4_kernel<true>", "colchain4_kernel<false>")


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()
    U.print_table(TARGET)


def _durations(F):
    """ids and forced durations of an utterance of exactly F frames: two ids (one frame, the rest), one id for one frame."""
    return [1, F - 1] if F > 1 else [1]


def _run(lib, vname, frames, knob, wseed, sids):
    cfg, _ = U.voice(vname, wseed)
    durs = [_durations(F) for F in frames]
    ids, nw, nz = U.batch_inputs(cfg, [len(d) for d in durs], 11)
    nz = np.ascontiguousarray(nz[:, :, :max(frames)])
    eng = U.engine_for(vname, {"PIPER_HIP_WN_COMPOSE": knob, "PIPER_HIP_DEBUG_POISON": 1}, lib=lib, wseed=wseed)
    eng.profile_enable(2)
    eng.profile_reset()
    try:
        r = eng.synthesize_batch(ids, U.SCALES, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(durations=durs))
        names = {row["name"]: int(row["launches"]) for row in eng.profile()[5:] if row["launches"]}
    finally:
        eng.profile_enable(0)
    durations = eng.durations()
    off = np.concatenate([[0], np.cumsum([len(s) for s in ids])])
    # (every id is forced, so the duration predictor does not run: no logw, no duration noise to read back)
    got = [{"x_enc": eng.debug_tensor("x_enc", b), "stats": eng.debug_tensor("stats", b), "logw": None,
            "durations": durations[off[b]:off[b + 1]].astype(np.int64), "z_p": eng.debug_tensor("z_p", b),
            "z": eng.debug_tensor("z", b), "noise_z": eng.debug_tensor("noise_z", b), "audio": r.audio[b].copy(),
            "frames": int(r.frames[b])} for b in range(len(ids))]
    for b, g in enumerate(got):
        assert g["frames"] == frames[b] and np.array_equal(g["durations"], durs[b]), (b, g["frames"], g["durations"])
        assert np.array_equal(g["noise_z"], nz[b][:, :frames[b]]), b
    return ids, nw, got, names


def _case(lib, vname, frames, wseed=1234, sids=None):
    cfg, w = U.voice(vname, wseed)
    base = None
    for knob in KNOBS:
        ids, nw, got, names = _run(lib, vname, frames, knob, wseed, sids)
        flow = {k: names.get(k, 0) for k in FLOW}
        print(f"[{TARGET} {vname} frames {frames} WN_COMPOSE={knob}] flow launches {flow}")
        ngate = cfg.flow_n * cfg.wn_layers
        if knob == 0:
            base = (got, names)
            # the parent's route: pre + flow_n * (wn_layers gate convs + wn_layers - 1 res/skip launches + one chain launch)
            assert flow["gate4_kernel"] == ngate and flow["gate4pre_kernel"] == 0 and flow["colchain4_kernel<true>"] == cfg.flow_n, flow
            continue
        got0, names0 = base
        for b, g in enumerate(got):
            for k in ("durations", "noise_z", "z_p", "x_enc", "stats"):
                assert np.array_equal(g[k], got0[b][k]), (knob, b, k)
        if knob == 3:          # not built: knob 0's launches and bits
            assert names == names0, (names, names0)
            for b, g in enumerate(got):
                assert np.array_equal(g["z"], got0[b]["z"]) and np.array_equal(g["audio"], got0[b]["audio"]), b
        else:
            want = dict(names0)
            want["colchain4_kernel<false>"] -= 1
            want["gate4_kernel"] -= cfg.flow_n
            want["gate4pre_kernel"] = cfg.flow_n
            assert names == want, (knob, names, want)
            assert names["gate4_kernel"] > 0 and names["colchain4_kernel<true>"] == cfg.flow_n
            assert sum(names.values()) == sum(names0.values()) - 1
            for b, g in enumerate(got):
                assert not np.array_equal(g["z"], got0[b]["z"]), (knob, b, "the composed route gave knob 0's bits")
        for b, g in enumerate(got):
            what = f"[{TARGET} {vname} frames {frames} WN_COMPOSE={knob} utt {b}]"
            sid = None if sids is None else sids[b]
            assert np.all(np.isfinite(g["z"])) and np.all(np.isfinite(g["audio"])), what
            fig, _ = U.measure(w, cfg, ids[b], U.SCALES, nw[b], g, sid, "FG")
            for s in ("z", "audio"):
                f = fig[s]
                U.ROWS.append((TARGET, vname, frames, f"WN_COMPOSE={knob}", "f32", b, s, f["e_hip"], f["e_ref"], f["r_hip"], f["r_ref"]))
            U.check_gates(fig, {s: (U.GATES[TARGET][s] if s in ("z", "audio") else None) for s in U.STAGES}, what)


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 12, 13, 37])
def test_one_utterance_of_forced_frames(emu_lib, F):
    _case(emu_lib, "tiny192", [F])


def test_ragged_call_of_two_utterances(emu_lib):
    _case(emu_lib, "tiny192", [3, 13])


@pytest.mark.parametrize("frames,sids", [([3], [2]), ([13], [1]), ([3, 13], [3, 1])])
def test_speaker_bias_reaches_the_composed_gate_conv(emu_lib, frames, sids):
    _case(emu_lib, "tiny192-ms", frames, wseed=5, sids=sids)
