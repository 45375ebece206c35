"""The architecture envelope against f64 truths: what tests/test_gpu_arch_envelope.py (an MI355X) and
tests/test_arch_envelope_emu.py (the kernel emulator) share -- the table of architectures, the inputs and one run routine.

Engine::init (csrc/engine_pack.cpp) accepts far more than the four shipped qualities: any hidden that is a multiple of 32 up
to 256, any even inter, any head count with an even head dimension up to 128, window 0 .. 4, kernel_size 1 or 3, any filter
width, any even number of coupling layers, any WN depth and tap count, any up-sampling ladder with kernel = 2 * stride, up to
four resblock kernels with any dilations, any gin. Every architecture of ARCH is preset("tiny", **overrides), registered in
one_utterance_truth_case.WIDE under its case name, and held to every check of that module (six stage tensors under the K gates
from the engine's own input to each stage, every duration the ceil of the f64 value, the z_p 8-ulp bound, the frame counts)
on two calls: one utterance of 9 ids, and a ragged call of five utterances of 5, 1, 12, 2 and 3 ids (the 1-, 2- and 3-id rows
between longer ones). Multi-speaker voices give every utterance of a call another speaker, as far as the voice has them.

Each entry: (overrides, what it is there for, kernels it must launch, kernels it must not launch). The kernel names hold on
the emulator and on the device alike (both follow the default policy at these sizes); a name, or a prefix ending in '<' / ','.

Duration-noise seeds (SEEDS: {case: (seed of the 9-id call, seed of the ragged call)}) were picked on the CPU as the first
seed from 1 that keeps the oracle's own f64 durations at least 1e-3 (relative) from an integer, ten times ORACLE_MARGIN:
seed 1 everywhere but the ragged calls of A5 and A11 (seed 2). MARGINS holds what each achieves, 1.3e-3 (A4, ragged) at the
least; check_durations asserts the 1e-4 on every utterance."""
import numpy as np

import one_utterance_truth_case as U

ONE, RAGGED = [9], [5, 1, 12, 2, 3]
EMU, GPU = "emu-arch", "gpu-arch"
for _t in (EMU, GPU):          # K = 8, the project's gate for two f32 summation orders; K_CASE below where a measured ratio asks for more
    U.GATES.setdefault(_t, {s: 8 for s in U.STAGES})
W192 = dict(hidden=192, inter=192, filter=96, n_layers=2)          # U.WIDE["tiny192"]

FRONT4 = ("colchain4_kernel<false>", "lngemm4_kernel", "dds_layer4_kernel")
FRONT4_GONE = ("attn4_kernel<", "colchain4_kernel<", "lngemm4_kernel", "dds_layer4_kernel", "ffn_kernel")

ARCH = {
    # ---- A. text encoder and duration predictor
    "A1-proj192-half48": (dict(hidden=192, inter=96, filter=96, n_layers=2),
                          "the 4-column front with a 192-row projection (stacked proj + pre, split 192), a flow on 48-channel halves",
                          FRONT4 + ("attn4_kernel<96,false>", "ffn_kernel"), ()),
    "A2-proj128-heads4": (dict(hidden=192, inter=64, filter=96, n_layers=2, n_heads=4),
                          "a 128-row projection, no multiple of 192: unstacked; head dimension 48 on 192 channels",
                          ("attn_kernel<48>", "colchain4_kernel<false>", "dds_layer4_kernel"), ("attn4_kernel<",)),
    "A3-inter-wider": (dict(hidden=96, inter=192, filter=96, n_layers=2), "inter wider than hidden",
                       ("attn_kernel<48>", "ln_kernel", "dds_layer16_kernel<3>", "conv_splitk16_kernel<false,"), FRONT4_GONE),
    "A4-hidden256-dk128": (dict(hidden=256, inter=32, filter=64, n_layers=1),
                           "the upper edge of hidden and of the head dimension: the window takes 1152 of 1280 floats",
                           ("attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "conv_splitk16_kernel<true,12,2,4>"), FRONT4_GONE),
    "A5-heads7": (dict(hidden=224, inter=32, filter=40, n_layers=1, n_heads=7), "seven heads of 32",
                  ("attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "conv_splitk16_kernel<true,12,2,4>"), FRONT4_GONE),
    "A6-h128-inter160": (dict(hidden=128, inter=160, filter=80, n_layers=1), "80-channel halves on 128 hidden channels",
                         ("attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "conv_splitk16_kernel<false,"), FRONT4_GONE),
    "A7-filter100-heads6": (dict(hidden=192, inter=192, filter=100, n_layers=2, n_heads=6),
                            "a filter that is no multiple of 48: the FFN unfused among 4-column launches; head dimension 32",
                            ("attn_kernel<0>", "colchain4_kernel<false>", "colchain4_kernel<true>", "lngemm4_kernel", "dds_layer4_kernel",
                             "gate4pre_kernel"), ("ffn_kernel", "attn4_kernel<")),
    "A8-filter768-window1": (dict(hidden=192, inter=192, filter=768, n_layers=1, window=1),
                             "ffn_kernel with all 16 slices; a clipped relative-position window",
                             FRONT4 + ("attn4_kernel<96,false>", "ffn_kernel", "colchain4_kernel<true>", "gate4pre_kernel"), ()),
    "A9-window0": (dict(window=0), "no relative-position window", ("attn_kernel<0>", "ln_kernel"), FRONT4_GONE),
    "A9-window1-head1": (dict(window=1, n_heads=1), "one head, window 1", ("attn_kernel<0>", "ln_kernel"), FRONT4_GONE),
    "A10-ksize1": (dict(kernel_size=1), "one-tap FFN and DDSConv: the residual is tap 0 (dds_layer16_kernel)",
                   ("attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>"), FRONT4_GONE),
    "A10-ksize1-192": (dict(W192, kernel_size=1), "one-tap FFN and DDSConv on 192 channels (dds_layer4_kernel)",
                       FRONT4 + ("attn4_kernel<96,false>",), ("ffn_kernel",)),
    "A11-half17-filter33": (dict(inter=34, filter=33), "17-channel coupling halves and an odd filter",
                            ("attn_kernel<0>", "ln_kernel", "conv_splitk_kernel<2,true,", "conv_mfma_kernel<2,2,1,1,16,false,64>"), FRONT4_GONE),
    # ---- B. flow and duration flows
    "B1-shallow": (dict(flow_n=2, wn_layers=1, wn_kernel=3, dp_flows=2, dds_layers=1), "the smallest of every depth",
                   ("dds_layer16_kernel<8>", "conv_splitk_kernel<2,true,"), ("gate4_kernel",)),
    "B2-flow6-wnk7": (dict(flow_n=6, wn_layers=2, wn_kernel=7), "six coupling layers, seven WN taps",
                      ("conv_splitk_kernel<2,true,",), ("gate4_kernel",)),
    "B3-wnk1-dds4": (dict(wn_kernel=1, dds_layers=4, dp_flows=3), "one-tap WN, four DDS layers, three duration flows",
                     ("dds_layer16_kernel<8>", "conv_splitk_kernel<2,true,"), ("gate4_kernel",)),
    "B4-192-wnk7-wn6": (dict(hidden=192, inter=192, filter=96, n_layers=1, wn_kernel=7, wn_layers=6),
                        "seven taps on the 192-channel flow: gate4_kernel (at most 5 taps) must not run",
                        FRONT4 + ("ffn_kernel", "conv_splitk16_kernel<true,12,2,4>", "colchain4_kernel<true>"), ("gate4_kernel", "gate4pre_kernel")),
    # ---- C. speakers
    "C1-192-gin24": (dict(W192, n_speakers=3, gin=24), "speaker conditioning on the 4-column kernels, gin 24",
                     FRONT4 + ("cond_kernel", "gate4_kernel", "gate4pre_kernel", "colchain4_kernel<true>"), ()),
    "C2-192-gin512": (dict(hidden=192, inter=192, filter=48, n_layers=1, n_speakers=5, gin=512), "gin 512, five speakers",
                      FRONT4 + ("cond_kernel", "gate4_kernel", "gate4pre_kernel", "colchain4_kernel<true>"), ()),
    "C3-gin7-up40": (dict(up_initial=40, n_speakers=2, gin=7), "an odd gin, a 40-channel generator entry",
                     ("cond_kernel", "conv_mfma_group_kernel<", "mrf_sum_kernel", "conv_post_kernel", "mrf_kernel<32,1,1>"), ()),
    # ---- D. generator
    "D1-up4x4-ch24-12": (dict(up_rates=(4, 4), up_kernel_sizes=(8, 8), up_initial=48, rb_kernel_sizes=(3,), rb_dilations=((1,),)),
                         "24 and 12 generator channels, one resblock of one dilation",
                         ("conv_mfma_kernel<2,2,1,1,16,false,64>", "mrf_kernel<32,1,1>", "pcm16_kernel"), ("conv_post_kernel",)),
    "D2-up2x5": (dict(up_rates=(2, 2, 2, 2, 2), up_kernel_sizes=(4,) * 5, up_initial=128), "five up-sampling stages of 2",
                 ("mrf_kernel<64,1,2>", "mrf_kernel<32,1,1>", "pcm16_kernel"), ("conv_post_kernel",)),
    "D3-rb1-four-kernels": (dict(resblock=1, rb_kernel_sizes=(3, 5, 7, 9), rb_dilations=((1,), (2,), (3,), (1,))),
                            "ResBlock1 with four kernels of one dilation each",
                            ("mrf_kernel<32,1,1>", "pcm16_kernel"), ("conv_post_kernel",)),
    "D4-dil-1-4-7": (dict(rb_kernel_sizes=(5, 9), rb_dilations=((1, 4, 7), (2, 3, 5))), "two resblock kernels, three uneven dilations: no fused MRF stage",
                     ("conv_mfma_group_kernel<", "mrf_sum_kernel", "conv_post_kernel", "pcm16_kernel"), ("mrf_kernel<",)),
    "D5-k11-dil27": (dict(rb_kernel_sizes=(3, 11), rb_dilations=((1, 9, 27), (1, 2, 4))), "an 11-tap kernel and a dilation of 27: no fused MRF stage",
                     ("conv_mfma_group_kernel<", "mrf_sum_kernel", "conv_post_kernel", "pcm16_kernel"), ("mrf_kernel<",)),
}
for _name, (_over, _, _, _) in ARCH.items():
    U.WIDE.setdefault(_name, _over)

SEEDS = {name: (1, 2 if name in ("A5-heads7", "A11-half17-filter33") else 1) for name in ARCH}
# the oracle's own f64 w: the least relative distance from an integer over every id of the (9-id call, ragged call)
MARGINS = {"A1-proj192-half48": (1.3e-02, 1.5e-02), "A2-proj128-heads4": (4.0e-02, 4.3e-03), "A3-inter-wider": (9.9e-02, 2.2e-03),
           "A4-hidden256-dk128": (5.0e-02, 1.3e-03), "A5-heads7": (1.4e-03, 1.7e-02), "A6-h128-inter160": (3.3e-02, 5.9e-03),
           "A7-filter100-heads6": (3.0e-02, 9.4e-03), "A8-filter768-window1": (2.6e-02, 9.3e-03), "A9-window0": (6.8e-02, 2.4e-02),
           "A9-window1-head1": (5.5e-02, 7.9e-03), "A10-ksize1": (4.8e-02, 2.3e-02), "A10-ksize1-192": (2.4e-02, 3.0e-02),
           "A11-half17-filter33": (4.2e-02, 7.5e-03), "B1-shallow": (1.1e-02, 1.1e-02), "B2-flow6-wnk7": (4.2e-02, 1.7e-02),
           "B3-wnk1-dds4": (1.2e-01, 2.6e-03), "B4-192-wnk7-wn6": (9.4e-03, 5.3e-03), "C1-192-gin24": (4.5e-02, 2.1e-02),
           "C2-192-gin512": (9.1e-02, 2.9e-02), "C3-gin7-up40": (3.1e-02, 3.2e-02), "D1-up4x4-ch24-12": (4.2e-02, 1.7e-02),
           "D2-up2x5": (4.2e-02, 1.7e-02), "D3-rb1-four-kernels": (4.2e-02, 1.7e-02), "D4-dil-1-4-7": (4.2e-02, 1.7e-02),
           "D5-k11-dil27": (4.2e-02, 1.7e-02)}          # (the D cases share tiny's front half, and with it B2's figures)

# E: the forced forms on the uneven 192-channel voices: knob -> (kernels that must appear, kernels that must be gone) against the
# default policy's run of the same voice, on all three; FORCED_ALSO: what one voice adds to those sets (only A1 runs attn4_kernel
# and only A1 and A2 ffn_kernel by default; only A7, whose halves are 96 channels wide, the chained res/skip launches and the
# composed gate conv). PIPER_HIP_COLCHAIN=0 leaves the duration predictor's and the flow's colchain4_kernel<false> launches alone.
FORCED_ON = ("A1-proj192-half48", "A2-proj128-heads4", "A7-filter100-heads6")
FORCED = {
    "PIPER_HIP_COL4=0": ({"colchain_kernel<6>", "lngemm_kernel<6>", "dds_layer16_kernel<6>"},
                         {"colchain4_kernel<", "lngemm4_kernel", "dds_layer4_kernel"}),
    "PIPER_HIP_COLCHAIN=0": ({"ln_kernel"}, {"lngemm4_kernel"}),
}
FORCED_ALSO = {"A1-proj192-half48": ({"attn_kernel<96>"}, {"attn4_kernel<", "ffn_kernel"}), "A2-proj128-heads4": (set(), {"ffn_kernel"}),
               "A7-filter100-heads6": (set(), {"colchain4_kernel<true>", "gate4pre_kernel"})}


def check_forced(name, knob, names, ref):
    """The kernel set really changed: everything of FORCED / FORCED_ALSO appeared that the default run did not launch, and
    everything it replaces was launched by the default run and is gone."""
    appear, absent = (a | b for a, b in zip(FORCED[knob], FORCED_ALSO[name]))
    U.require(names, appear, (name, knob))
    assert set(names) != set(ref) and not [n for n in appear if n in ref], (name, knob, sorted(ref))
    for n in absent:
        U.require(ref, {n}, (name, knob, "flipped from a policy that does not launch it"))
    gone(names, absent, (name, knob))

# F: split matrix modes on odd channel counts
SPLIT_ON = ("A11-half17-filter33", "D1-up4x4-ch24-12")

# {(target, case, utterances, route): {(utterance, stage): K}} for every measured ratio above 4: the smallest power of two at least
# twice the ratio. All but one are logw of an utterance of one to nine ids -- a handful of values against an oracle f32 error that
# falls anywhere between zero and a few ulp by chance, 1-id utterances most of all (profiles/arch_envelope.md has every figure and
# the reason); every other utterance and stage of the same call keeps K = 8, and the durations are exact checks.
K_CASE = {
    (EMU, 'A10-ksize1-192', 5, 'default'): {(1, 'logw'): 16},
    (EMU, 'A3-inter-wider', 5, 'default'): {(1, 'logw'): 32},
    (EMU, 'A4-hidden256-dk128', 5, 'default'): {(1, 'logw'): 256},
    (EMU, 'A5-heads7', 5, 'default'): {(0, 'logw'): 16},
    (EMU, 'B1-shallow', 5, 'default'): {(1, 'logw'): 32},
    (EMU, 'A10-ksize1-192', 5, 'PIPER_HIP_FUSE_DP=0'): {(1, 'logw'): 64},
    (EMU, 'A1-proj192-half48', 5, 'PIPER_HIP_COL4=0'): {(1, 'logs_p'): 16},
    (EMU, 'A2-proj128-heads4', 5, 'PIPER_HIP_COLCHAIN=0'): {(0, 'logw'): 16},
    (EMU, 'A7-filter100-heads6', 5, 'PIPER_HIP_COLCHAIN=0'): {(1, 'logw'): 32, (3, 'logw'): 16},
    (GPU, 'A1-proj192-half48', 5, 'default'): {(1, 'logw'): 128},
    (GPU, 'A11-half17-filter33', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'A3-inter-wider', 1, 'default'): {(0, 'logw'): 16},
    (GPU, 'A4-hidden256-dk128', 5, 'default'): {(1, 'logw'): 256},
    (GPU, 'A5-heads7', 5, 'default'): {(1, 'logw'): 16},
    (GPU, 'B2-flow6-wnk7', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'C1-192-gin24', 5, 'default'): {(3, 'logw'): 16},
    (GPU, 'D1-up4x4-ch24-12', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'D2-up2x5', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'D3-rb1-four-kernels', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'D4-dil-1-4-7', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'D5-k11-dil27', 5, 'default'): {(4, 'logw'): 16},
    (GPU, 'A10-ksize1-192', 5, 'PIPER_HIP_FUSE_DP=0'): {(1, 'logw'): 32},
    (GPU, 'A1-proj192-half48', 5, 'PIPER_HIP_COL4=0'): {(1, 'logw'): 32},
    (GPU, 'A2-proj128-heads4', 5, 'PIPER_HIP_COL4=0'): {(1, 'logw'): 16},
    (GPU, 'A2-proj128-heads4', 5, 'PIPER_HIP_COLCHAIN=0'): {(1, 'logw'): 512},
    (GPU, 'A7-filter100-heads6', 5, 'PIPER_HIP_COLCHAIN=0'): {(1, 'logw'): 64},
}
_RUNS = {}


def sids_for(cfg, B):
    """Every utterance its own speaker, as far as the voice has them; None for a single-speaker voice."""
    if cfg.n_speakers <= 1:
        return None
    return [cfg.n_speakers - 1] if B == 1 else [(b + 1) % cfg.n_speakers for b in range(B)]


def inputs(name, lens):
    """(ids, duration noise [B][2][max T], prior noise [B][C][32 max T + 64], speaker ids) of one call of a case."""
    cfg, _ = U.voice(name)
    ids, nw, nz = U.batch_inputs(cfg, lens, SEEDS[name][0 if len(lens) == 1 else 1])
    return ids, nw, nz, sids_for(cfg, len(lens))


def gone(names, absent, what):
    left = [x for x in names for n in absent if x == n or (n[-1] in "<," and x.startswith(n))]
    assert not left, (what, left, sorted(names))


def run_case(target, name, lens, env=None, route="default", mode="f32", lib=None, eng=None, gated=U.STAGES, graph=None):
    """One compared call of a case on `target` (EMU: one profiled call with injected noise on `lib`; GPU: U.run's graph
    protocol, "spec" for one utterance and "two" for five) with every check of U.check_call; returns (tensors, names, figures)."""
    key = (target, name, tuple(lens), route, mode)
    if eng is None and key in _RUNS:          # a default run that a forced form is compared with: once per module
        return _RUNS[key]
    ids, nw, nz, sids = inputs(name, lens)
    e = eng or U.engine_for(name, env, lib=lib)
    if target == EMU:
        got, names = U.run(e, ids, U.SCALES, sids, nw, nz)
        for b, g in enumerate(got):
            assert np.array_equal(g["noise_z"], nz[b][:, :g["frames"]]), b
    else:
        got, names = U.run(e, ids, U.SCALES, sids, nw, graph=graph or ("spec" if len(lens) == 1 else "two"))
    print(f"[{target} {name} {lens} {route} {mode}] frames {[g['frames'] for g in got]} kernels: {sorted(names)}")
    figs = U.check_call(target, name, ids, U.SCALES, sids, nw, got, route, mode, gated=gated,
                        k_case=K_CASE.get((target, name, len(lens), route)))
    if eng is None:
        _RUNS[key] = (got, names, figs)
    return got, names, figs


def check_names(name, names):
    _, _, want, absent = ARCH[name]
    U.require(names, set(want), name)
    gone(names, absent, name)
