"""Per-utterance noise seeds (include/piper_hip.h: pe_seeds): what tests/test_seeds_emu.py (the kernel
emulator) and tests/test_gpu_seeds.py (an MI355X) share. numpy only, no device of its own.

The law. An utterance that carries a seed S draws, at both sampling sites, element (row = channel, column = id or frame) of
the documented stream with key S and run counter 0: rng_case.truth(S, 0, site, channel, 0, n), and what
debug_randn(site, 0, n, row=channel) returns under set_seed(S). An utterance without a seed draws what it always drew:
(engine seed, run counter, row = b * channels + c).

"Exact" is np.array_equal against debug_randn of an ORACLE engine -- a second handle, so that the engine under test keeps
its own seed and run counter -- plus rng_case.check against the f64 truth under the caller's gate.

PCM_LSB. Two runs that were fed identical noise are held to 7 LSB of int16 against each other: the project holds each
path's float waveform to 2e-4 of full scale against the oracle (TIGHT_AUDIO_TOL), 6.6 LSB."""
import numpy as np

import rng_case as R
from piper_amd import weights as W

SEEDS = (0, 2 ** 64 - 1, 2 ** 32, 2 ** 32 + 1, 0xDEADBEEF12345678)        # the key's second word is in use
PCM_LSB = 7
SCALES = R.SCALES


def ids_of(cfg, lens, first=70):
    return [W.synthetic_phoneme_ids(T, first + i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(lens)]


def seeds_for(n, first=0):
    return [SEEDS[(first + i) % len(SEEDS)] for i in range(n)]


def expected(oracle, seed, call, site, row0, rows, n):
    """debug_randn rows row0 .. row0 + rows - 1 of (seed, call, site), n columns each, from the oracle engine."""
    oracle.set_seed(int(seed) % 2 ** 64)
    return np.stack([oracle.debug_randn(site, call, n, row=row0 + c) for c in range(rows)])


def check_rows(x, oracle, seed, call, site, row0, gate, what):
    """x [rows][n]: bit-equal to the oracle's rows row0 .. of (seed, call, site) and under the gates against the f64 truth."""
    rows, n = x.shape
    want = expected(oracle, seed, call, site, row0, rows, n)
    assert np.array_equal(x, want), (what, "not the documented draws", site, int(np.argmax(x != want)))
    t = np.empty(x.shape, np.float64)
    rad = np.empty(x.shape, np.float64)
    for c in range(rows):
        t[c], rad[c], _ = R.truth(int(seed) % 2 ** 64, call, site, row0 + c, 0, n)
    R.check(np.ascontiguousarray(x).reshape(-1), t.reshape(-1), rad.reshape(-1), gate, f"[{what} site {site}]")


def check_noise(eng, oracle, cfg, seeds, lens, gate, what, sites=(0, 1), engine_seed=None, call=None):
    """noise_w / noise_z of every utterance of the engine's last call. Utterance b with seeds[b] = S: rows 0 .. channels - 1
    of (S, counter 0). With seeds[b] None: rows channels * b .. of (engine_seed, call), the engine's own stream. Returns the
    frame counts (with site 1 among `sites`)."""
    frames = []
    for b, T in enumerate(lens):
        got = []
        if 0 in sites:
            nw = eng.debug_tensor("noise_w", b)
            assert nw.shape == (2, T), (what, b, nw.shape)
            got.append((0, nw, 2))
        if 1 in sites:
            nz = eng.debug_tensor("noise_z", b)
            assert nz.shape[0] == cfg.inter and nz.shape[1] >= 1, (what, b, nz.shape)
            frames.append(nz.shape[1])
            got.append((1, nz, cfg.inter))
        for site, x, ch in got:
            if seeds[b] is None:
                assert engine_seed is not None and call is not None, what
                check_rows(x, oracle, engine_seed, call, site, ch * b, gate, f"{what} utt {b} unseeded")
            else:
                check_rows(x, oracle, seeds[b], 0, site, 0, gate, f"{what} utt {b} seed {int(seeds[b]) % 2 ** 64:#x}")
    return frames


def pcm_close(a, b, what):
    """Two int16 waveforms of runs fed identical noise: same length, within PCM_LSB. Returns whether they were bit-equal."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = int(np.max(np.abs(a.astype(np.int32) - b.astype(np.int32)))) if a.size else 0
    print(f"[{what}] pcm: max |d| {d} LSB over {a.size} samples, bit-equal {d == 0}")
    assert d <= PCM_LSB, (what, d)
    return d == 0


def profiled_names(eng, call):
    """{kernel name: launches} of `call()` under the level-2 profile (a profiled call is never a graph)."""
    eng.profile_enable(2)
    eng.profile_reset()
    try:
        call()
        return {row["name"]: int(row["launches"]) for row in eng.profile()[5:] if row["launches"]}
    finally:
        eng.profile_enable(0)
