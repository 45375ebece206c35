"""CPU (emulator) twin of tests/test_gpu_arch_envelope.py: every architecture that Engine::init accepts and no shipped quality
has, stage by stage against f64 truths (tests/arch_envelope_case.py has the table, the seeds and their margins;
tests/one_utterance_truth_case.py the checks and the gates; profiles/arch_envelope.md the measured ratios) -- and, on this twin
only, one architecture just outside every rule of Engine::init: refused by name, never a crash.

The emulator has no graphs, so every case is one profiled call with injected noise: the 9-id utterance and the ragged call of
5, 1, 12, 2 and 3 ids of every architecture (none had to drop to three utterances: the f64 truths of the widest ragged call take
under a second here; the cost is the emulator's, 12 s for a ragged call of a 192-channel voice, 1 to 4 s for the tiny ones)."""
import os
import subprocess

import numpy as np
import pytest

import arch_envelope_case as A
import one_utterance_truth_case as U
from piper_amd import _lib as L, weights as W
from piper_amd.engine import Engine, EngineError

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
TARGET = A.EMU
CALLS = [pytest.param(A.ONE, id="one9"), pytest.param(A.RAGGED, id="ragged5")]


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()
    U.print_table(TARGET)          # (with -s: the figures kept in profiles/arch_envelope.md)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("name", sorted(A.ARCH))
def test_accepted_architectures_stage_by_stage(emu_lib, name, lens):
    """Every case of A.ARCH on the default policy: all gates, and the kernels the case is there for."""
    _, names, _ = A.run_case(TARGET, name, lens, lib=emu_lib)
    A.check_names(name, names)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("name", ["A10-ksize1", "A10-ksize1-192"])
def test_one_tap_ddsconv_on_the_unfused_duration_flows(emu_lib, name, lens):
    """kernel_size 1 under PIPER_HIP_FUSE_DP=0: cf_pre_kernel, scale_kernel and spline_inverse_kernel around the same DDS layers."""
    _, names, _ = A.run_case(TARGET, name, lens, env={"PIPER_HIP_FUSE_DP": 0}, route="PIPER_HIP_FUSE_DP=0", lib=emu_lib)
    A.check_names(name, names)
    U.require(names, {"cf_pre_kernel", "scale_kernel", "spline_inverse_kernel"}, name)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("knob", sorted(A.FORCED))
@pytest.mark.parametrize("name", A.FORCED_ON)
def test_forced_forms_on_the_uneven_192_channel_voices(emu_lib, name, knob, lens):
    """A1, A2 and A7 under PIPER_HIP_COL4=0 (the 16-column chain kernels) and PIPER_HIP_COLCHAIN=0 (plain convs plus ln_kernel):
    the same gates, and the kernel set really changed against the default policy's run of the same call."""
    _, ref, _ = A.run_case(TARGET, name, lens, lib=emu_lib)
    _, names, _ = A.run_case(TARGET, name, lens, env=dict([knob.split("=")]), route=knob, lib=emu_lib)
    A.check_forced(name, knob, names, ref)


@pytest.mark.parametrize("name", A.SPLIT_ON)
def test_split_matrix_modes_on_odd_channel_counts(emu_lib, name):
    """A11 (17-channel halves) and D1 (24 and 12 generator channels), the ragged call, f32 / f16x3 / bf16x3 on fresh engines: on
    every utterance all in front of the flow is the f32 run's bit for bit; z and audio meet truth_gates relative to the f32 run's
    error."""
    runs = {}
    for m in ("f32", "f16x3", "bf16x3"):
        eng = U.engine_for(name, {"PIPER_HIP_MATRIX": m}, lib=emu_lib, fresh=True)
        try:
            runs[m] = A.run_case(TARGET, name, A.RAGGED, route="default", mode=m, eng=eng,
                                 gated=U.STAGES if m == "f32" else ("x_enc", "m_p", "logs_p", "logw"))
        finally:
            eng.close()
        if m != "f32":
            assert any(f"split_kernel<{U.SM[m]}," in n for n in runs[m][1]), (m, sorted(runs[m][1]))
    f32, _, ffig = runs["f32"]
    for m, (got, _, fig) in runs.items():
        for u in range(len(A.RAGGED)):
            for k in ("noise_z", "x_enc", "stats", "logw", "durations", "z_p"):
                assert np.array_equal(got[u][k], f32[u][k]), (m, u, k)
            for s in ("z", "audio"):
                err = {"torch": fig[u][s]["e_ref"], "fl": fig[u][s]["fl"], "f32": ffig[u][s]["e_hip"], m: fig[u][s]["e_hip"]}
                print(f"[{TARGET} {name} {A.RAGGED} default {m} utt {u}] {s}: {err}")
                assert U.truth_gates(err, m, "gauss"), (m, u, s, err)


# ---- the refusal edge: one architecture just outside every rule of Engine::init (csrc/engine_pack.cpp). tests/test_loader_hardening.py
# holds the .onnx reader to named errors; it builds no engine, so none of these rules is covered there and none is skipped here.
REFUSED = [
    (dict(hidden=288, n_heads=4), "hidden_channels must be a multiple of 32 and <= 256"),          # (head dimension 72)
    (dict(hidden=48), "hidden_channels must be a multiple of 32 and <= 256"),
    (dict(hidden=256, n_heads=1), "head dimension must be even and <= 128"),
    (dict(hidden=160, n_heads=32), "head dimension must be even and <= 128"),          # head dimension 5
    (dict(window=5), "relative-attention window too wide"),
    (dict(kernel_size=2), "kernel_size must be 1 or 3"),
    (dict(kernel_size=5), "kernel_size must be 1 or 3"),
    (dict(inter=33), "bad architecture header"),
    (dict(flow_n=3), "odd number of flow layers is not supported"),
    (dict(num_bins=8), "spline with num_bins != 10 is not supported"),
    (dict(n_speakers=2, gin=0), "multi-speaker voice without gin_channels"),
    (dict(up_rates=(8, 8, 4), up_kernel_sizes=(16, 16, 4)), "dec.ups.2: ConvTranspose1d with kernel != 2*stride is not supported"),
    (dict(up_rates=(3, 5), up_kernel_sizes=(6, 10)), "dec.ups.0: ConvTranspose1d with an odd stride is not supported"),
]


@pytest.mark.parametrize("over,text", REFUSED, ids=[",".join(f"{k}={v}" for k, v in o.items()).replace(" ", "") for o, _ in REFUSED])
def test_architectures_outside_the_envelope_are_refused_by_name(emu_lib, over, text):
    """Creating the engine raises EngineError whose text names the rule; the process lives on, and a valid engine made right after
    gives the audio of the gated 9-id run of A9-window0 bit for bit (the emulator with injected noise is deterministic)."""
    cfg = W.preset("tiny", **over)
    try:
        blob = W.pack_blob(cfg, W.synthetic_weights(cfg, 1234))
    except Exception as ex:          # the Python side cannot even lay this architecture out: nothing reaches Engine::init
        pytest.fail(f"the weight writer refused {over} before the engine could: {ex!r}")
    with pytest.raises(EngineError) as ei:
        Engine(blob=blob, lib=emu_lib).close()
    assert text in str(ei.value), (over, str(ei.value))
    assert "kernel != 2*stride" not in str(ei.value) or over["up_kernel_sizes"][-1] != 2 * over["up_rates"][-1], str(ei.value)
    want, _, _ = A.run_case(TARGET, "A9-window0", A.ONE, lib=emu_lib)
    ids, nw, nz, sids = A.inputs("A9-window0", A.ONE)
    eng = U.engine_for("A9-window0", lib=emu_lib, fresh=True)
    try:
        r = eng.synthesize_batch(ids, U.SCALES, sids=sids, noise_w=nw, noise_z=nz)
        assert np.array_equal(r.audio[0], want[0]["audio"]) and int(r.frames[0]) == want[0]["frames"]
    finally:
        eng.close()
