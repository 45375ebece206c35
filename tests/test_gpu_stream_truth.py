"""The chunked decode against f64 truths on an MI355X (run with -m gpu; -s prints the per-chunk tables): the one-utterance
stream (stage W), the batch stream (stage V) and the stream pool (stage P), each chunk from the engine's own latent against the
f64 generator, with the window edges -- an utterance shorter than the halo, a one-frame chunk, a chunk longer than the
utterance, changing chunk sizes, finished rows, a reused pool row -- and the halo check that tells a window one frame short from
an exact one (tests/stream_truth_case.py has the plays, the checks and the gates; profiles/stream_truth.md the measured figures).

The compared play is the replay of a warm engine: a first play with other ids and noise of the same lengths, the figures from a
second during which nothing is captured, the kernel names from a third under the level-2 profile that must give the second's
chunks bit for bit. Every engine runs with PIPER_HIP_DEBUG_POISON=1.

Out of scope, tested elsewhere: converted output rates, the running and fixed stream gains, loudness, the limiter and the seeds.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import functools

import numpy as np
import pytest

import one_utterance_truth_case as U
import stream_truth_case as S

pytestmark = pytest.mark.gpu

# The generator forms a window stage selects, read off the first profiled run (profiles/stream_truth.md). A one-row window takes
# the same forms at 32 frames (chunks of up to 10 frames at a halo of 11), at 96 (a chunk of 45) and at 64 (a chunk of 100000 cut
# to the row), in stage W and as a batch of one in stage V; rows of 32-frame windows take the tiled up-conv, four rows another MRF form than three.
GEN_W = {"conv_splitk_kernel<1,false,4,4>", "conv_splitk_kernel<1,false,8,4>", "conv_splitk_group_kernel<4,2,64>",
         "conv_splitk_sum_kernel<4,2>", "mrf_kernel<32,1,1>", "mrf_kernel<64,1,2>"}
GEN_ROWS3 = {"conv_splitk_kernel<1,false,4,4>", "conv_splitk_kernel<1,false,8,4>", "conv_mfma_kernel<2,2,1,1,16,false,128>",
             "mrf_kernel<32,1,1>", "mrf_kernel<64,1,2>"}
GEN_ROWS4 = (GEN_ROWS3 - {"mrf_kernel<32,1,1>"}) | {"mrf_kernel<32,2,1>"}
GEN_OTHER = {"high": {"conv_splitk_kernel<1,false,8,4>", "conv_mfma_kernel<2,2,1,1,16,false,64>", "conv_mfma_group_kernel<2,2,1,1,16,64>",
                      "mrf_kernel<32,2,1>", "mrf_sum_kernel"},
             "x-low": GEN_ROWS3 | {"conv_mfma_kernel<1,4,1,1,16,false,64>"},
             "tiny-ms": {"cond_kernel", "conv_splitk_kernel<1,false,4,4>", "conv_mfma_kernel<1,4,1,1,16,false,64>", "mrf_kernel<32,1,1>"}}
_PICKS = {}
_FIG45 = {}


def _ends_on_engine_error(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        from piper_amd.engine import EngineError
        try:
            return fn(*a, **kw)
        except EngineError as ex:
            pytest.exit(f"HIP / engine error in {fn.__name__}: {ex}", returncode=3)
    return run


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    S.print_tables("gpu")          # (with -s: the figures kept in profiles/stream_truth.md)


def _halo(eng):
    pool = eng.stream_pool(1, 8)          # (opening a pool returns the halo without running a kernel)
    try:
        return pool.halo
    finally:
        pool.close()


def _medium(kind):
    """The medium voice's one-utterance inputs, picked once on the CPU oracle: "short" 3 ids at h - 4 frames, "mid" 12 ids at
    2h + 13, "long" 37 ids at 2 * 45 + 11 frames (a partial last chunk of 45)."""
    if kind not in _PICKS:
        cfg, _ = U.voice("medium")
        h = _halo(U.engine_for("medium", S.ENV))
        T, index, seed, F = {"short": (3, 5, 41, h - 4), "mid": (12, 7, 43, 2 * h + 13), "long": (37, 3, 137, 101)}[kind]
        _PICKS[kind] = (S.pick_scale("medium", S.utt(cfg, f"ids{T}", T, index, seed, cols=4 * F + 64), F), F)
    return _PICKS[kind]


@pytest.mark.parametrize("asks", [[1], [11]])
@_ends_on_engine_error
def test_one_utterance_stream_shorter_than_the_halo(asks):
    """Medium, 3 ids, h - 4 frames. Chunks of 1: every window is the whole utterance, clipped on both sides. One chunk of at
    least F: the unchunked call."""
    eng = U.engine_for("medium", S.ENV)
    u, F = _medium("short")
    got, _, _ = S.case_one("gpu", "medium", eng, False, f"F<h ask {asks}", u, asks, wanted=GEN_W)
    assert got[0].F == F and len(got[0].chunks) == (F if asks == [1] else 1)


@_ends_on_engine_error
def test_one_utterance_stream_halo():
    """Medium, 12 ids, 2h + 13 frames, chunks of 1, 4 and 5 frames (a single frame, one full 4-column tile, one tile and a
    frame): the first and last windows are clipped on one side, the inner ones full. The halo check over the three chunkings."""
    eng = U.engine_for("medium", S.ENV)
    u, F = _medium("mid")
    h = _halo(eng)
    recs = []
    for c in (1, 4, 5):
        got, _, (_, r) = S.case_one("gpu", "medium", eng, False, f"2h+13 ask [{c}]", u, [c], wanted=GEN_W)
        assert got[0].F == F and len(got[0].chunks) == -(-F // c)
        recs += r
    S.check_halo("gpu", "medium", "W", "2h+13 ask [1], [4], [5]", recs, h, eng.hop)


@_ends_on_engine_error
def test_one_utterance_stream_reference_chunk_with_partial_last():
    """Medium, 37 ids, 101 frames, the reference's chunk of 45: the last chunk has 11 frames, its window is shorter than the one
    before it in the same bucket, over whatever that one left in the window buffer."""
    eng = U.engine_for("medium", S.ENV)
    u, F = _medium("long")
    got, names, (figs, _) = S.case_one("gpu", "medium", eng, False, "101 frames ask [45]", u, [45], wanted=GEN_W)
    assert [a.size // eng.hop for a, _ in got[0].chunks] == [45, 45, 11]
    _FIG45["f32"], _FIG45["names"] = figs[0], names


@_ends_on_engine_error
def test_one_utterance_stream_bucket_shrinks_and_grows():
    """One stream asking for 45, then 1, then 7, then 100000 frames (pe_stream_next called directly)."""
    eng = U.engine_for("medium", S.ENV)
    u, F = _medium("long")
    got, _, _ = S.case_one("gpu", "medium", eng, False, "101 frames ask [45, 1, 7, 100000]", u, [45, 1, 7, 100000], wanted=GEN_W)
    assert [a.size // eng.hop for a, _ in got[0].chunks] == [45, 1, 7, 48]


@_ends_on_engine_error
def test_batch_stream_ragged_rows_and_finished_rows():
    """Medium, four rows of forced 1, h, h + 1 and 2h + 13 frames with a scale triple each, chunks of 4. A finished row delivers
    nothing, and every other row still meets its gates in the calls after (the idle window [0, 1) with count 0 runs next to
    them). The rows finish at calls 0, 2, 2 and 8: h and h + 1 frames are both three chunks of 4 (the emulator twin, with h + 2,
    has four different calls). The halo check over all rows' chunks of this play and of one in chunks of 1."""
    cfg, _ = U.voice("medium")
    eng = U.engine_for("medium", S.ENV)
    h = _halo(eng)
    frames = (1, h, h + 1, 2 * h + 13)
    utts = [S.utt(cfg, f"row{i}", 3 + 2 * i, 11 + i, 60 + i, F=F, scales=U.MIXED_SCALES[i]) for i, F in enumerate(frames)]
    got, _, (_, recs) = S.case_batch("gpu", "medium", eng, False, f"forced {frames} ask 4", utts, 4, wanted=GEN_ROWS4)
    assert tuple(u.F for u in got) == frames
    assert [u.calls[-1] for u in got] == [-(-F // 4) - 1 for F in frames]
    assert all(u.calls == list(range(len(u.chunks))) for u in got)
    # (six chunks of 4 with a full halo are too few for the reference's own condition: the same rows in chunks of 1 as well)
    _, _, (_, more) = S.case_batch("gpu", "medium", eng, False, f"forced {frames} ask 1", utts, 1, wanted=GEN_ROWS4)
    S.check_halo("gpu", "medium", "V", f"forced {frames} ask 4 and 1", recs + more, h, eng.hop)


@_ends_on_engine_error
def test_batch_of_one_next_to_the_one_utterance_stream():
    """The same utterance (2h + 13 frames, chunks of 4) as a batch of one and as a one-utterance stream: both meet the gates, and
    the batch of one the halo check over its chunks of 4 and of 1 (the one-utterance stream's is test_one_utterance_stream_halo).
    The kernel forms differ, so no equal bits are asked for."""
    eng = U.engine_for("medium", S.ENV)
    u, F = _medium("mid")
    h = _halo(eng)
    a, _, (_, recs) = S.case_batch("gpu", "medium", eng, False, "batch of one, 2h+13 ask 4", [u], 4, wanted=GEN_W)
    _, _, (_, more) = S.case_batch("gpu", "medium", eng, False, "batch of one, 2h+13 ask 1", [u], 1, wanted=GEN_W)
    S.check_halo("gpu", "medium", "V", "batch of one, 2h+13 ask 4 and 1", recs + more, h, eng.hop)
    b, _, _ = S.case_one("gpu", "medium", eng, False, "2h+13 ask [4] (next to the batch of one)", u, [4], wanted=GEN_W)
    assert a[0].F == b[0].F == F and np.array_equal(a[0].z, b[0].z)


@_ends_on_engine_error
def test_stream_pool_short_first_chunk_leave_and_reuse():
    """Medium, 3 slots. Three listeners of forced 2h + 13, 2h + 17 and 2h + 8 frames join with a first chunk of 1 frame
    (per_slot), then 4; after three calls the third hangs up in mid-stream and a newcomer of h - 2 frames takes the slot the
    longer tenant left: its resident row is the newcomer's latent bit for bit on [0, F) and exactly zero behind. The truth of
    every chunk comes from the resident row."""
    cfg, _ = U.voice("medium")
    eng = U.engine_for("medium", S.ENV)
    h = _halo(eng)
    frames = (2 * h + 13, 2 * h + 17, 2 * h + 8)
    three = [S.utt(cfg, f"slot{i}", 5 + 3 * i, 21 + i, 70 + i, F=F, scales=U.MIXED_SCALES[i]) for i, F in enumerate(frames)]
    new = S.utt(cfg, "newcomer", 4, 29, 79, F=h - 2, scales=U.MIXED_SCALES[3])
    got, _, (_, recs) = S.case_pool("gpu", "medium", eng, False, f"forced {frames} + {h - 2}, first 1 then 4", three, new, 2, 1, 4, 48,
                                    halo=False, wanted=GEN_ROWS3)
    assert tuple(u.F for u in got) == frames + (h - 2,) and got[3].slot == got[2].slot == 2
    # (13 and 16 chunks with a full halo leave the reference's own s at 2 sigma of its 1/16: the same scenario in chunks of 1 as well)
    _, _, (_, more) = S.case_pool("gpu", "medium", eng, False, f"forced {frames} + {h - 2}, first 1 then 1", three, new, 2, 1, 1, 48,
                                  halo=False, wanted=GEN_ROWS3)
    S.check_halo("gpu", "medium", "P", f"forced {frames} + {h - 2}, first 1 then 4 and then 1", recs + more, h, eng.hop)


@pytest.mark.parametrize("vname", ["high", "x-low", "tiny-ms"])
@_ends_on_engine_error
def test_other_voices_through_the_batch_stream(vname):
    """high (ResBlock1, halo 14): 64 and 20 ids at forced 2 * 45 + 13 and 45 + h frames, chunks of 45, gates only (its halo
    statement is the f64 one of tests/test_stream_truth_emu.py). x-low (96 channels) and tiny-ms with three different speakers in
    one batch (the resident conditioning row): rows of h, h + 1 and 2h + 13 frames, chunks of 4 and of 1, with the halo check over both plays."""
    cfg, _ = U.voice(vname)
    eng = U.engine_for(vname, S.ENV)
    h = _halo(eng)
    if vname == "high":
        assert h == 14
        frames, lens, chunk = (2 * 45 + 13, 45 + h), (64, 20), 45
    else:
        assert h == 11
        frames, lens, chunk = (h, h + 1, 2 * h + 13), (4, 6, 12), 4
    sids = (2, 0, 3) if cfg.n_speakers > 1 else (None,) * 3
    utts = [S.utt(cfg, f"row{i}", T, 31 + i, 80 + i, F=F, sid=sids[i], scales=U.MIXED_SCALES[i]) for i, (T, F) in enumerate(zip(lens, frames))]
    got, names, (_, recs) = S.case_batch("gpu", vname, eng, False, f"forced {frames} ask {chunk}", utts, chunk, wanted=GEN_OTHER[vname])
    assert tuple(u.F for u in got) == frames
    if vname != "high":
        _, _, (_, more) = S.case_batch("gpu", vname, eng, False, f"forced {frames} ask 1", utts, 1, wanted=GEN_OTHER[vname])
        S.check_halo("gpu", vname, "V", f"forced {frames} ask {chunk} and 1", recs + more, h, eng.hop)
    assert ("cond_kernel" in names) == (cfg.n_speakers > 1), sorted(names)


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3", "bf16x3"])
@_ends_on_engine_error
def test_matrix_modes_on_the_reference_chunk(mode):
    """Medium, the 45-frame case under the split matrix modes on fresh engines: the utterance's pooled error against the truth
    of its own latent meets truth_gates relative to the f32 run's error."""
    if "f32" not in _FIG45:
        test_one_utterance_stream_reference_chunk_with_partial_last()
    u, F = _medium("long")
    eng = U.engine_for("medium", dict(S.ENV, PIPER_HIP_MATRIX=mode), fresh=True)
    try:
        got, names, (figs, _) = S.case_one("gpu", "medium", eng, False, "101 frames ask [45]", u, [45], mode=mode, K=None)
    finally:
        eng.close()
    assert got[0].F == F
    if mode == "bf16x6":          # a one-row window stays on the split-K f32 forms under bf16x6 (exact operands either way)
        assert names == _FIG45["names"], (mode, sorted(set(names) ^ set(_FIG45["names"])))
    else:
        assert any(f"split_kernel<{U.SM[mode]}," in n for n in names), (mode, sorted(names))
    f32, fig = _FIG45["f32"], figs[0]
    err = {"torch": fig["e_ref"], "fl": fig["fl"], "f32": f32["e_hip"], mode: fig["e_hip"]}
    print(f"[gpu medium W 101 frames ask [45] {mode}]: {err}")
    assert U.truth_gates(err, mode, "gauss"), (mode, err)
