"""The noise generator against the reference of tests/rng_case.py, on the CPU: the reference itself against Random123's
known answers, then the kernel emulator's build of piper_amd/csrc/kernels/rng.h -- every draw of 2^20 per site and call,
the stream law over windows whose counter, stream and seed words all cross 2^32, the three places of the product path that
draw (embed_kernel, a randn_kernel launch, regulate_kernel), and the seeds of a group's members.

The emulator's log2 / sin / cos are glibc's f32 functions, the reference's are numpy's: gate E <= 1e-6 (rng_case.EMU_GATE),
the reference's own 4.3e-7 against the f64 truth plus a few f32 ulps between the two libraries; measured here 4.2e-7.
What the emulator cannot show is the accuracy of the hardware's transcendental units: tests/test_gpu_rng.py.

The emulator runs a whole call in 15 to 40 s, most of it the vocoder, so the product-path cases are the smallest that reach
each draw site: the batches of the seam keep one utterance of 128 / 129 ids and three short ones (the id bucket, and with it
the count of Philox blocks, is the longest utterance's), and the utterance of more than 1024 frames is a one-utterance stream
of which only the first chunk is decoded. The full-size voices at 33 and 37 ids run on the device only."""
import os
import subprocess

import numpy as np
import pytest

import one_utterance_truth_case as U
import rng_case as R
from piper_amd import _lib as L, weights as W

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
SEED = 2026


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()


def _ids(cfg, lens, first=70):
    return [W.synthetic_phoneme_ids(T, first + i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(lens)]


def test_reference_reproduces_the_known_answer_vectors():
    for c, k, want in R.KAT:
        got = tuple(int(x[0]) for x in R.philox4x32_10(c, k))
        assert got == want, ([hex(x) for x in got], [hex(x) for x in want])
    # vectorised: the three at once
    got = R.philox4x32_10([[v[0][i] for v in R.KAT] for i in range(4)], [[v[1][i] for v in R.KAT] for i in range(2)])
    assert [tuple(int(x[j]) for x in got) for j in range(3)] == [v[2] for v in R.KAT]


def test_reference_uniforms_and_edges():
    """The uniforms at the ends of the integer range, and what the finder returns."""
    ra = np.array([0, 1, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1], np.uint64)
    u1, u2 = R.uniforms(ra, ra)
    assert u1[0] == np.float32(2.0 ** -32) and u1[2] < 1.0 and u1[3] == 1.0 and u1[4] == 1.0 and u2[0] == 0.0 and u2[4] == 1.0
    t, rad, g = R.transform(ra, ra, np.array([0, 1, 0, 1, 0]))
    assert rad[3] == 0.0 and rad[4] == 0.0 and t[3] == 0.0 and abs(float(g[4])) <= R.ZERO_RAD
    assert abs(rad[0] - np.sqrt(2 * 32 * np.log(2.0))) < 1e-12
    edges = R.edge_draws(SEED, 1, 0, n=1 << 16)
    rs, rb, _ = R.stream(SEED, 1, 0, 0, 0, 1 << 16)
    assert set(edges) == set(R.EDGE_CLASSES) and all(v.size == 2 * R.EDGE_K for v in edges.values())
    assert rs[edges["u1 smallest"]].max() <= np.sort(np.unique(rs))[R.EDGE_K - 1]
    assert np.abs(rb[edges["u2 nearest 0.5"]].astype(np.int64) - 2 ** 31).max() < 2 ** 32 * 1e-3


@pytest.mark.parametrize("site", [0, 1])
@pytest.mark.parametrize("call", [1, 2])
def test_every_draw_of_a_site(emu_lib, site, call):
    eng = U.engine_for("tiny", {}, lib=emu_lib)
    eng.set_seed(SEED)
    n = 1 << 20
    t, rad, g32 = R.truth(SEED, call, site, 0, 0, n)
    print(f"reference: E {R.errors(g32, t, rad)[0]:.3e}")
    R.check(eng.debug_randn(site, call, n), t, rad, R.EMU_GATE, f"[emu site {site} call {call}]")


def test_stream_law(emu_lib):
    eng = U.engine_for("tiny", {}, lib=emu_lib)
    worst = R.check_windows(eng, R.EMU_GATE, "emu")
    print(f"stream law: {len(R.windows())} windows, worst E {worst:.3e}")


@pytest.mark.parametrize("lens, drawn_by", [([128, 3, 1, 2], "embed_kernel"), ([129, 3, 1, 2], "randn_kernel")])
def test_product_path_on_both_sides_of_the_embed_seam(emu_lib, lens, drawn_by):
    """Four utterances in the id bucket of 128: 4 * 2 * 32 = 256 Philox blocks, the most embed_kernel draws itself; of 129
    ids (bucket 160): a randn_kernel launch. The same law on both sides."""
    cfg, _ = U.voice("tiny")
    eng = U.engine_for("tiny", {}, lib=emu_lib, fresh=True)
    try:
        names, _ = R.product_calls(eng, cfg, 77, _ids(cfg, lens), R.EMU_GATE, f"emu tiny {lens}", runs=0)
    finally:
        eng.close()
    assert ("randn_kernel" in names) == (drawn_by == "randn_kernel") and "embed_kernel" in names and "regulate_kernel" in names, names


def test_product_path_ragged_batch_two_calls(emu_lib):
    """3, 5, 40 and 129 ids: rows 2 b + c and inter b + c of utterances of unequal lengths, at run counters 1 and 2."""
    cfg, _ = U.voice("tiny")
    eng = U.engine_for("tiny", {}, lib=emu_lib, fresh=True)
    try:
        names, frames = R.product_calls(eng, cfg, 2 ** 32 + 1, _ids(cfg, [3, 5, 40, 129]), R.EMU_GATE, "emu tiny ragged", runs=1)
    finally:
        eng.close()
    assert "randn_kernel" in names and len(set(frames)) == 4, (names, frames)


def test_one_utterance_stream_past_1024_frames(emu_lib):
    """A one-utterance stream with the engine's own noise: after the first chunk noise_w / noise_z are the reference's at the
    stream's run counter. 200 ids at length_scale 6 pass 1024 frames (more than four workgroups of regulate_kernel along the frames)."""
    cfg, _ = U.voice("tiny")
    ids = _ids(cfg, [200])[0]
    eng = U.engine_for("tiny", {}, lib=emu_lib, fresh=True)
    try:
        eng.set_seed(31)
        for call in (1, 2):
            chunks = eng.stream(ids, (0.667, 6.0, 0.8), chunk_frames=16)
            next(chunks)
            frames = R.check_engine_noise(eng, cfg, 31, call, [len(ids)], R.EMU_GATE, "emu tiny stream")
            chunks.close()
            assert frames[0] == eng.stream_frames > 1024, (frames, eng.stream_frames)
    finally:
        eng.close()


def test_group_members_draw_distinct_streams(emu_lib, monkeypatch):
    """A group nobody seeded: member i draws from the default seed + i, in every group created that way."""
    R.check_group(emu_lib, monkeypatch, "tiny", R.EMU_GATE, "emu")
