"""PIPER_HIP_WN_COMPOSE values 1 and 4 on the kernel emulator: a coupling layer's post composed into the skip rows of its WN
res/skip convs when the weights are packed (engine_pack.cpp pack_post4). Every WN layer adds
M_j . acts_j + c_j, 96 rows, into the skip sum (colchain4_kernel mode 2 with rows1 = 288, or 96 for the last layer), and the
chain launch subtracts the completed sum from x1 without a post GEMM (colchain4_kernel mode 1 with w1 == null). No GPU.

The 192-hidden, 96-half tiny voice and a multi-speaker override of it, PIPER_HIP_DEBUG_POISON=1 throughout (rows 96 .. 191 of
the skip sum are never written on the composed route: a read of them would give NaN). Frame counts are forced through the
timing plan: 1 .. 5 frames (every way a 4-column tile meets an utterance's end), 13, 37, and the ragged call of
3 and 13 frames; speakers [2], [1] and [3, 1] on the multi-speaker voice. Both Flip parities: the voice has two or more
coupling layers. Duration noise and prior noise are injected, so every knob value sees the same z_p.

For each case, knob 1 against knob 2 and knob 4 against knob 0 (the same build without post composed):
  - z and audio meet the f64 truth gates of tests/one_utterance_truth_case.py (stages F and G, K = 8);
  - durations, noise_z, z_p, x_enc and stats equal knob 0's bit for bit;
  - the launch map per kernel name equals the uncomposed route's;
  - z differs from the uncomposed route's z (the composed route really ran), knob 2's z and audio differ from knob 1's;
  - PIPER_HIP_CHAIN_RS=0 with knob 1 gives the bits of knob 1 (the last layer's conv as a launch of its own, the chain launch
    without any GEMM in front: the same additions in the same order).

Mutation check (by hand, profiles/post_compose.md): M_j packed without the Flip parity order, or bpost dropped from c_0 --
every case fails its z gate."""
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
PAIRS = ((1, 2), (4, 0))          # (post composed, the same route without it)


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


def _run(lib, vname, frames, env, wseed, sids):
    cfg, _ = U.voice(vname, wseed)
    durs = [_durations(F) for F in frames]
    ids, nw, nz = U.batch_inputs(cfg, [len(d) for d in durs], 11)
    nz = np.ascontiguousarray(nz[:, :, :max(frames)])
    eng = U.engine_for(vname, dict(env, PIPER_HIP_DEBUG_POISON=1), lib=lib, wseed=wseed)
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
    assert cfg.flow_n >= 2          # both Flip parities
    runs = {k: _run(lib, vname, frames, {"PIPER_HIP_WN_COMPOSE": k}, wseed, sids) for k in (0, 1, 2, 4)}
    got0 = runs[0][2]
    for knob, plain in PAIRS:
        ids, nw, got, names = runs[knob]
        gotp, namesp = runs[plain][2], runs[plain][3]
        print(f"[{TARGET} {vname} frames {frames} WN_COMPOSE={knob}] launches {sorted(names.items())}")
        assert names == namesp, (knob, names, namesp)
        assert names["colchain4_kernel<true>"] == cfg.flow_n, names
        for b, g in enumerate(got):
            what = f"[{TARGET} {vname} frames {frames} WN_COMPOSE={knob} utt {b}]"
            for k in ("durations", "noise_z", "z_p", "x_enc", "stats"):
                assert np.array_equal(g[k], got0[b][k]), (what, k)
            assert not np.array_equal(g["z"], gotp[b]["z"]), (what, f"the composed route gave the bits of knob {plain}")
            assert np.all(np.isfinite(g["z"])) and np.all(np.isfinite(g["audio"])), what
            sid = None if sids is None else sids[b]
            fig, _ = U.measure(w, cfg, ids[b], U.SCALES, nw[b], g, sid, "FG")
            for s in ("z", "audio"):
                f = fig[s]
                U.ROWS.append((TARGET, vname, frames, f"WN_COMPOSE={knob}", "f32", b, s, f["e_hip"], f["e_ref"], f["r_hip"], f["r_ref"]))
            U.check_gates(fig, {s: (U.GATES[TARGET][s] if s in ("z", "audio") else None) for s in U.STAGES}, what)
    for b, g in enumerate(runs[1][2]):          # (pair (1, 2) above: z differs; the audio must as well)
        assert not np.array_equal(g["audio"], runs[2][2][b]["audio"]), (b, "knob 2 gave knob 1's audio")
    # the last res/skip conv on its own: one launch more per coupling layer, none of them colchain4_kernel<true>, the same bits
    _, _, gotr, namesr = _run(lib, vname, frames, {"PIPER_HIP_WN_COMPOSE": 1, "PIPER_HIP_CHAIN_RS": 0}, wseed, sids)
    names1 = runs[1][3]
    assert "colchain4_kernel<true>" not in namesr and sum(namesr.values()) == sum(names1.values()) + cfg.flow_n, (namesr, names1)
    assert namesr["colchain4_kernel<false>"] == names1["colchain4_kernel<false>"] + 2 * cfg.flow_n, (namesr, names1)
    for b, g in enumerate(gotr):
        for k in ("z", "audio"):
            assert np.array_equal(g[k], runs[1][2][b][k]), (b, k, "PIPER_HIP_CHAIN_RS=0 changed the bits of the composed route")


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 13, 37])
def test_one_utterance_of_forced_frames(emu_lib, F):
    _case(emu_lib, "tiny192", [F])


def test_ragged_call_of_two_utterances(emu_lib):
    _case(emu_lib, "tiny192", [3, 13])


@pytest.mark.parametrize("frames,sids", [([3], [2]), ([13], [1]), ([3, 13], [3, 1])])
def test_speaker_bias_does_not_disturb_the_composed_skip_convs(emu_lib, frames, sids):
    _case(emu_lib, "tiny192-ms", frames, wseed=5, sids=sids)
