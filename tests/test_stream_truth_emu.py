"""CPU (emulator) twin of tests/test_gpu_stream_truth.py: the three streaming paths against f64 truths of the engine's own latent,
halo check included (tests/stream_truth_case.py has the plays, the checks and the gates; profiles/stream_truth.md the measured
figures). The voices are tiny, tiny-ms (another speaker per row: the resident conditioning row) and the 192-channel tiny192, all
ResBlock2 with a halo of 11 frames; forced frame counts are no multiples of 4. The emulator has no graphs: every case is one
profiled play. The last test is the CPU statement about the ResBlock1 bound, which no f32 run can check."""
import os
import subprocess

import numpy as np
import pytest
import torch

import one_utterance_truth_case as U
import stream_truth_case as S
from piper_amd import _lib as L

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
VOICES = ("tiny", "tiny-ms", "tiny192")
SIDS = {"tiny-ms": (1, 3, 0, 2)}
# the generator forms of a window stage on the emulator, read off the first profiled run (profiles/stream_truth.md)
GEN = {"conv_splitk_kernel<", "conv_mfma_kernel<", "mrf_kernel<"}


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()
    S.print_tables("emu")          # (with -s: the figures of profiles/stream_truth.md)


def _sid(vname, i):
    return SIDS[vname][i] if vname in SIDS else None


def _halo(eng):
    pool = eng.stream_pool(1, 8)          # (opening a pool returns the halo without running a kernel)
    try:
        return pool.halo
    finally:
        pool.close()


@pytest.mark.parametrize("vname", VOICES)
def test_one_utterance_stream(emu_lib, vname):
    """Stage W. 3 ids, fewer frames than the halo: chunks of 1 (every window is the whole utterance, clipped on both sides) and
    one chunk of at least F (the unchunked call). 12 ids at 2h + 13 frames: chunks of 3, 4 and 5 (a partial 4-column tile, one
    tile, one tile and a frame; the one-frame chunk with a full halo on both sides is in the last stream) with the halo check over
    the three chunkings -- the first and last windows clipped on one side, the inner ones full; chunks
    of 13 with a partial last one in the bucket of the one before; and 13, 1, 7, 100000 in one stream: the bucket shrinks and grows."""
    cfg, _ = U.voice(vname)
    eng = U.engine_for(vname, S.ENV, lib=emu_lib)
    h = _halo(eng)
    short = S.pick_scale(vname, S.utt(cfg, "ids3", 3, 5, 41, sid=_sid(vname, 0), cols=256), h - 4)
    for asks in ([1], [h]):
        got, _, _ = S.case_one("emu", vname, eng, True, f"F<h ask {asks}", short, asks, wanted=GEN)
        assert got[0].F == h - 4 and len(got[0].chunks) == (h - 4 if asks == [1] else 1)
    F = 2 * h + 13
    mid = S.pick_scale(vname, S.utt(cfg, "ids12", 12, 7, 43, sid=_sid(vname, 1), cols=512), F)
    recs = []
    for c in (3, 4, 5):
        got, _, (_, r) = S.case_one("emu", vname, eng, True, f"2h+13 ask [{c}]", mid, [c], wanted=GEN)
        assert got[0].F == F and len(got[0].chunks) == -(-F // c)
        recs += r
    S.check_halo("emu", vname, "W", "2h+13 ask [3], [4], [5]", recs, h, eng.hop)
    got, _, _ = S.case_one("emu", vname, eng, True, "2h+13 ask [13]", mid, [13], wanted=GEN)
    assert [a.size // eng.hop for a, _ in got[0].chunks] == [13, 13, 9]
    got, _, _ = S.case_one("emu", vname, eng, True, "2h+13 ask [13, 1, 7, 100000]", mid, [13, 1, 7, 100000], wanted=GEN)
    assert [a.size // eng.hop for a, _ in got[0].chunks] == [13, 1, 7, 14]


@pytest.mark.parametrize("vname", VOICES)
def test_batch_stream(emu_lib, vname):
    """Stage V. Four rows of forced 1, h, h + 2 and 2h + 13 frames with a scale triple each, chunks of 4: they finish at four
    different calls, a finished row delivers nothing (its idle window [0, 1) with count 0 runs next to the others, which still meet
    their gates), and the halo check on the chunks of all rows, in chunks of 4 and of 3. Then the 2h + 13 utterance of
    test_one_utterance_stream as a batch of one: it meets the gates there and here (the kernel forms differ, so no equal bits
    are asked for; its six chunks with a full halo are too few for a halo check of their own)."""
    cfg, _ = U.voice(vname)
    eng = U.engine_for(vname, S.ENV, lib=emu_lib)
    h = _halo(eng)
    frames = (1, h, h + 2, 2 * h + 13)
    utts = [S.utt(cfg, f"row{i}", 3 + 2 * i, 11 + i, 60 + i, F=F, sid=_sid(vname, i), scales=U.MIXED_SCALES[i]) for i, F in enumerate(frames)]
    got, _, (_, recs) = S.case_batch("emu", vname, eng, True, f"forced {frames} ask 4", utts, 4, wanted=GEN)
    assert tuple(u.F for u in got) == frames
    last = [u.calls[-1] for u in got]
    assert len(set(last)) == 4 and last == [-(-F // 4) - 1 for F in frames], last
    # (six chunks of 4 with a full halo are too few for the reference's own condition: the same rows in chunks of 3 as well)
    _, _, (_, more) = S.case_batch("emu", vname, eng, True, f"forced {frames} ask 3", utts, 3, wanted=GEN)
    S.check_halo("emu", vname, "V", f"forced {frames} ask 4 and 3", recs + more, h, eng.hop)
    mid = S.pick_scale(vname, S.utt(cfg, "ids12", 12, 7, 43, sid=_sid(vname, 1), cols=512), 2 * h + 13)
    S.case_batch("emu", vname, eng, True, "batch of one, 2h+13 ask 4", [mid], 4, wanted=GEN)


@pytest.mark.parametrize("vname", VOICES)
def test_stream_pool(emu_lib, vname):
    """Stage P, 3 slots. Three listeners of forced 2h + 13, 2h + 17 and 2h + 8 frames join with a first chunk of 1 frame
    (per_slot), then 4; after three calls the third hangs up in mid-stream and a newcomer of h - 2 frames takes its slot: the
    resident row is then the newcomer's latent bit for bit and exactly zero where the longer tenant's frames were. The truth of
    every chunk comes from the resident row."""
    cfg, _ = U.voice(vname)
    eng = U.engine_for(vname, S.ENV, lib=emu_lib)
    h = _halo(eng)
    frames = (2 * h + 13, 2 * h + 17, 2 * h + 8)
    three = [S.utt(cfg, f"slot{i}", 5 + 3 * i, 21 + i, 70 + i, F=F, sid=_sid(vname, i), scales=U.MIXED_SCALES[i]) for i, F in enumerate(frames)]
    new = S.utt(cfg, "newcomer", 4, 29, 79, F=h - 2, sid=_sid(vname, 3), scales=U.MIXED_SCALES[3])
    got, _, _ = S.case_pool("emu", vname, eng, True, f"forced {frames} + {h - 2}, first 1 then 4", three, new, 2, 1, 4, 48, wanted=GEN)
    assert tuple(u.F for u in got) == frames + (h - 2,) and got[3].slot == got[2].slot == 2


def test_resblock1_halo_bound_is_one_frame_generous(emu_lib):
    """The ResBlock1 voices (tiny-high here, high in profiles/stream_truth.md) carry a halo of 14 frames; in f64 a window with
    13 on each side gives the same chunk within 1e-10, so the influence of the 14th frame is nothing an f32 run could see: the
    f32 halo check does not exist for them, and this is the statement in its place. Gaussian z, F = 2h + 13, every one-frame
    chunk that has a full halo on both sides."""
    for vname, wseed in (("tiny-high", 7), ("high", 1234)):
        cfg, _ = U.voice(vname, wseed)
        eng = U.engine_for(vname, S.ENV, lib=emu_lib, wseed=wseed, fresh=True)
        try:
            h = _halo(eng)
            hop = eng.hop
        finally:
            eng.close()
        assert cfg.resblock == 1 and h == 14
        F = 2 * h + 13
        z = np.random.default_rng(5).standard_normal((cfg.inter, F)).astype(np.float32)
        worst = 0.0
        for f0 in range(h, F - h, 6 if vname == "high" else 1):
            cut = {}
            for hh in (h, h - 1):
                a = S.generate(vname, wseed, torch.float64, z[:, f0 - hh:f0 + 1 + hh], None)
                cut[hh] = a[hh * hop:(hh + 1) * hop]
            worst = max(worst, float(np.max(np.abs(cut[h] - cut[h - 1]))))
        print(f"[{vname}] halo {h}: max |chunk with {h - 1} halo frames - chunk with {h}| in f64 {worst:.2e}")
        assert worst <= 1e-10, (vname, worst)
