"""The architecture envelope stage by stage against f64 truths on an MI355X (run with -m gpu): every architecture that
Engine::init accepts and no shipped quality has -- uneven hidden / inter / filter widths, 1 to 7 heads, window 0 and 1,
kernel_size 1, shallow and deep flows with 1, 3 and 7 WN taps, speaker conditioning of 7 to 512 channels, five generator shapes
(tests/arch_envelope_case.py has the table, the seeds and their margins; tests/one_utterance_truth_case.py the checks and the
gates; profiles/arch_envelope.md the measured ratios and the reason for every K that is not 8). The LDS sizes at hidden 256 and
head dimension 128, the guarded generic-width kernels and the MFMA paths at 24, 12 and 17 channels run for real only here.

Each architecture gets two calls: one utterance of 9 ids -- the repeated call of a warm engine, the whole utterance as one
graph with the engine's own prior noise -- and a ragged call of 5, 1, 12, 2 and 3 ids, which is two graphs and never
speculative; the kernel names are those of a profiled repeat that must reproduce durations and z_p bit for bit
(one_utterance_truth_case.run). A test takes under a second, nearly all of it the f64 truths on the CPU.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import arch_envelope_case as A
import one_utterance_truth_case as U

pytestmark = pytest.mark.gpu

TARGET = A.GPU
CALLS = [pytest.param(A.ONE, id="one9"), pytest.param(A.RAGGED, id="ragged5")]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    U.print_table(TARGET)          # (with -s: the figures kept in profiles/arch_envelope.md)


def _case(name, lens, **kw):
    from piper_amd.engine import EngineError
    try:
        return A.run_case(TARGET, name, lens, **kw)
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {name} {lens} {kw.get('route', 'default')}: {ex}", returncode=3)


def _fresh(name, env):
    from piper_amd.engine import EngineError
    try:
        return U.engine_for(name, env, fresh=True)
    except EngineError as ex:
        pytest.exit(f"HIP / engine error creating {name} {env}: {ex}", returncode=3)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("name", sorted(A.ARCH))
def test_accepted_architectures_stage_by_stage(name, lens):
    """Every case of A.ARCH on the default policy: all gates, and the kernels the case is there for."""
    _, names, _ = _case(name, lens)
    A.check_names(name, names)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("name", ["A10-ksize1", "A10-ksize1-192"])
def test_one_tap_ddsconv_on_the_unfused_duration_flows(name, lens):
    """kernel_size 1 under PIPER_HIP_FUSE_DP=0: cf_pre_kernel, scale_kernel and spline_inverse_kernel around the same DDS layers."""
    _, names, _ = _case(name, lens, env={"PIPER_HIP_FUSE_DP": 0}, route="PIPER_HIP_FUSE_DP=0")
    A.check_names(name, names)
    U.require(names, {"cf_pre_kernel", "scale_kernel", "spline_inverse_kernel"}, name)


@pytest.mark.parametrize("lens", CALLS)
@pytest.mark.parametrize("knob", sorted(A.FORCED))
@pytest.mark.parametrize("name", A.FORCED_ON)
def test_forced_forms_on_the_uneven_192_channel_voices(name, knob, lens):
    """A1, A2 and A7 under PIPER_HIP_COL4=0 (the 16-column chain kernels) and PIPER_HIP_COLCHAIN=0 (plain convs plus ln_kernel):
    the same gates, and the kernel set really changed against the default policy's run of the same call."""
    _, ref, _ = _case(name, lens)
    _, names, _ = _case(name, lens, env=dict([knob.split("=")]), route=knob)
    A.check_forced(name, knob, names, ref)


@pytest.mark.parametrize("name", A.SPLIT_ON)
def test_split_matrix_modes_on_odd_channel_counts(name):
    """A11 (17-channel halves) and D1 (24 and 12 generator channels), the ragged call, f32 / f16x3 / bf16x3 on fresh engines (the
    same run counter, so the same prior noise): on every utterance all in front of the flow is the f32 run's bit for bit; z and
    audio meet truth_gates relative to the f32 run's error."""
    runs = {}
    for m in ("f32", "f16x3", "bf16x3"):
        eng = _fresh(name, {"PIPER_HIP_MATRIX": m})
        try:
            runs[m] = _case(name, A.RAGGED, route="default", mode=m, eng=eng,
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
