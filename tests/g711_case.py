"""G.711 delivery (pe_set_sample_format, kernels/g711.h): the law restated in numpy and the cases the emulator tests
(tests/test_g711_emu.py) and the GPU tests (tests/test_gpu_g711.py) share. G.711 is integer arithmetic on the delivered
int16, so every comparison here is array_equal: there is no tolerance anywhere.

The law is that of the ITU-T G.191 software tools (include/piper_hip.h states it). With `lin` an int16, >> arithmetic and
~ one's complement:
    mu-law:  a = (lin < 0 ? (~lin) >> 2 : lin >> 2) + 33;  if (a > 0x1FFF) a = 0x1FFF;
             seg = 1; for (i = a >> 6; i; i >>= 1) seg++;
             code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF));  if (lin >= 0) code |= 0x80;
    A-law:   ix = lin < 0 ? (~lin) >> 4 : lin >> 4;
             if (ix > 15) { e = 1; while (ix > 31) { ix >>= 1; e++; }  ix = ix - 16 + (e << 4); }
             if (lin >= 0) ix |= 0x80;   code = ix ^ 0x55;
Python's audioop.lin2ulaw is NOT this mu-law (it negates after the shift and differs on 508 negative inputs); its
lin2alaw and both of its expanders agree, and are compared where the module imports."""
import numpy as np

FORMATS = ("ulaw", "alaw")
ZERO = {"ulaw": 0xFF, "alaw": 0xD5}                     # code(0): what silence is padded with
CANARY = 0xA5
SPAN = 2048                                              # samples per workgroup of the kernel (params.h: G711_SPAN)
ALL = np.arange(-32768, 32768, dtype=np.int32)


# ---- the restatement
def ulaw(lin):
    lin = np.asarray(lin).astype(np.int32)
    a = np.where(lin < 0, (~lin) >> 2, lin >> 2) + 33
    a = np.minimum(a, 0x1FFF)
    seg = np.ones_like(a)
    i = a >> 6
    while np.any(i):
        seg += (i != 0)
        i = i >> 1
    code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF))
    code = np.where(lin >= 0, code | 0x80, code)
    return code.astype(np.uint8)


def alaw(lin):
    lin = np.asarray(lin).astype(np.int32)
    ix = np.where(lin < 0, (~lin) >> 4, lin >> 4)
    big = ix > 15
    e = np.ones_like(ix)
    t = ix.copy()
    m = big & (t > 31)
    while np.any(m):
        t = np.where(m, t >> 1, t)
        e = e + m
        m = big & (t > 31)
    ix = np.where(big, t - 16 + (e << 4), ix)
    ix = np.where(lin >= 0, ix | 0x80, ix)
    return (ix ^ 0x55).astype(np.uint8)


def ulaw_expand(code):
    c = np.asarray(code).astype(np.int32)
    mant = ~c
    exponent = (mant >> 4) & 7
    step = 4 << (exponent + 1)
    v = (0x80 << exponent) + step * (mant & 0xF) + step // 2 - 4 * 33
    return np.where(c < 0x80, -v, v).astype(np.int16)


def alaw_expand(code):
    c = np.asarray(code).astype(np.int32)
    ix = (c ^ 0x55) & 0x7F
    iexp = ix >> 4
    mant = (ix & 0xF) + np.where(iexp > 0, 16, 0)
    mant = (mant << 4) + 8
    mant = np.where(iexp > 1, mant << np.maximum(iexp - 1, 0), mant)
    return np.where(c > 127, mant, -mant).astype(np.int16)


def g711(fmt, lin):
    return {"ulaw": ulaw, "alaw": alaw}[fmt](lin)


def expand(fmt, code):
    return {"ulaw": ulaw_expand, "alaw": alaw_expand}[fmt](code)


# ---- 1. the law, on the host
def check_law(lib):
    """pe_g711_encode over all 65536 int16 and pe_g711_decode over all 256 codes against the restatement (and audioop where
    it imports), and the properties the issue lists: every code occurs, decode(code(x)) is monotone, the largest error is
    644 / 512, code(decode(c)) == c but for mu-law's negative zero 0x7F, the anchors."""
    from piper_amd.engine import EngineError, g711_decode, g711_encode
    try:
        import audioop
    except ImportError:                                  # (gone from Python 3.13 on)
        audioop = None
    codes256 = np.arange(256, dtype=np.uint8)
    x16 = ALL.astype(np.int16)
    anchors = {"ulaw": {0: 0xFF, -1: 0x7F, 32767: 0x80, -32768: 0x00}, "alaw": {0: 0xD5, -1: 0x55, 32767: 0xAA, -32768: 0x2A}}
    for fmt, err in (("ulaw", 644), ("alaw", 512)):
        want = g711(fmt, ALL)
        got = g711_encode(fmt, x16, lib)
        assert got.dtype == np.uint8 and np.array_equal(got, want), fmt
        dec = g711_decode(fmt, codes256, lib)
        assert dec.dtype == np.int16 and np.array_equal(dec, expand(fmt, codes256)), fmt
        if audioop is not None:
            exp = np.frombuffer(getattr(audioop, fmt + "2lin")(codes256.tobytes(), 2), np.int16)
            assert np.array_equal(dec, exp), fmt
            if fmt == "alaw":
                assert np.array_equal(got, np.frombuffer(audioop.lin2alaw(x16.tobytes(), 2), np.uint8))
        assert np.unique(got).size == 256
        back = dec[got].astype(np.int32)                 # decode(code(x))
        assert np.all(np.diff(back) >= 0)
        assert int(np.max(np.abs(back - ALL))) == err, int(np.max(np.abs(back - ALL)))
        again = g711_encode(fmt, dec, lib)               # code(decode(c))
        differ = np.nonzero(again != codes256)[0].tolist()
        assert differ == ([0x7F] if fmt == "ulaw" else []), differ
        if fmt == "ulaw":
            assert dec[0x7F] == 0 and again[0x7F] == 0xFF
        for lin, code in anchors[fmt].items():
            assert int(got[lin + 32768]) == code == int(g711(fmt, [lin])[0]), (fmt, lin)
        assert ZERO[fmt] == anchors[fmt][0]
    for bad in ("s16", "g722"):
        try:
            g711_encode(bad, x16[:4], lib)
        except EngineError:
            continue
        raise AssertionError(bad)


# ---- 2. the kernel alone
# Lengths of the ragged batch, in an order in which every pair (packed offset mod 4, length mod 4) occurs: the packed start of
# a row has any residue, so the last dword of one row and the first of the next may be one dword owned by two workgroups.
RAGGED = (0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 3 * SPAN + 1, 6, 1, 11, 2, 4, 3, 10, 1, 5, 3, 8, 2, 6, 7, 9, 3, 12, 19, 15, 16)
PAD = 0                                                  # behind every row's end: codes 0xFF / 0xD5, not the canary


def ragged_pairs(lengths):
    off, pairs = 0, set()
    for n in lengths:
        pairs.add((off % 4, n % 4))
        off += n
    return pairs


def check_kernel_rows(eng, fmt):
    """The rows form: one row of all 65536 values (it crosses every span seam), then the ragged batch. The codes equal the
    restatement, every byte past the total is still the canary, two runs are bit-equal."""
    assert g711(fmt, [PAD])[0] != CANARY
    codes, tail = eng.debug_g711(fmt, [ALL.astype(np.int16)], pad=PAD, canary=CANARY)
    assert tail.size == 64 and np.all(tail == CANARY)
    assert np.array_equal(codes, g711(fmt, ALL))
    need = {0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 3 * SPAN + 1}
    assert need <= set(RAGGED) and len(ragged_pairs(RAGGED)) == 16, sorted(ragged_pairs(RAGGED))
    rng = np.random.default_rng(711)
    rows = [rng.integers(-32768, 32768, n).astype(np.int16) for n in RAGGED]
    want = g711(fmt, np.concatenate(rows))
    runs = [eng.debug_g711(fmt, rows, pad=PAD, canary=CANARY) for _ in range(2)]
    for codes, tail in runs:
        assert codes.size == sum(RAGGED) and tail.size == 64 and np.all(tail == CANARY)
        bad = np.nonzero(codes != want)[0]
        assert bad.size == 0, (fmt, bad[:8].tolist())
    assert np.array_equal(runs[0][0], runs[1][0])


FLAT = tuple(range(18)) + (SPAN - 1, SPAN, SPAN + 1, 4095, 4096, 4097)


def check_kernel_flat(eng, fmt):
    """The flat form: n in 0 .. 17 and around one and two workgroup spans; the same canary check."""
    rng = np.random.default_rng(712)
    for n in FLAT:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        codes, tail = eng.debug_g711(fmt, [x], flat=True, pad=PAD, canary=CANARY)
        assert codes.size == n and tail.size == 64 and np.all(tail == CANARY), n
        assert np.array_equal(codes, g711(fmt, x)), (fmt, n)


# ---- 3. whole utterances
# (name, set_loudness arguments or None): the routes of the delivery stage -- pcm16_kernel, pcm16_gain_kernel, limiter_kernel,
# pcm16_trim_kernel
SETTINGS = (("peak", None), ("loudness", dict(target_lufs=-8.0, ceiling_db=-1.0)),
            ("limiter", dict(target_lufs=-8.0, ceiling_db=-1.0, limiter=True, limiter_ms=5.0)),
            ("true-peak limiter", dict(target_lufs=-8.0, ceiling_db=-1.0, true_peak=True, limiter=True, limiter_ms=5.0)))


def check_result(r, base, fmt, where):
    """audio and pcm are the s16 call's bits, codes[b] == g711(pcm[b]) under the same offsets."""
    assert base.codes is None and r.codes is not None and len(r.codes) == len(r.pcm) == len(base.pcm), where
    for b in range(len(r.pcm)):
        assert r.pcm[b].size and np.array_equal(r.audio[b], base.audio[b]) and np.array_equal(r.pcm[b], base.pcm[b]), (where, b)
        assert r.codes[b].dtype == np.uint8 and r.codes[b].size == r.pcm[b].size, (where, b)
        bad = np.nonzero(r.codes[b] != g711(fmt, r.pcm[b]))[0]
        assert bad.size == 0, (where, b, bad[:8].tolist())


def whole_utterances(eng, cfg, rate, K, stretch, settings=None):
    """The ragged three-text batch of the loudness tests (the third stretched by a timing plan) on every route of the delivery
    stage at one rate: with ulaw, then alaw, the floats and the int16 are the s16 call's bits and the codes are g711 of the
    int16. One case fetches with want_pcm = 0: its codes are those of the call that also took the int16."""
    from piper_amd.engine import Timing
    ids, nw, nz = K.inputs(cfg)
    nz = np.ascontiguousarray(np.pad(nz, ((0, 0), (0, 0), (0, max(0, stretch + 8 - nz.shape[2])))))
    plan = Timing(target_frames=[0, 0, stretch])
    eng.set_output_rate(rate or 0)
    for name, loud in SETTINGS:
        if settings is not None and name not in settings:
            continue
        eng.set_loudness(**loud) if loud else eng.set_loudness(None)
        eng.set_sample_format("s16")
        base = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        assert eng.sample_format == "s16" and int(base.frames[2]) == stretch
        for fmt in FORMATS:
            eng.set_sample_format(fmt)
            assert eng.sample_format == fmt
            r = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
            check_result(r, base, fmt, (rate, name, fmt))
        if name == "limiter":
            eng.upload(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
            eng.run()
            only = eng.fetch(want_audio=False, want_pcm=False)
            assert only.pcm == [] and len(only.codes) == len(r.codes)
            for x, y in zip(only.codes, r.codes):
                assert x.size and np.array_equal(x, y)
    eng.set_loudness(None)
    eng.set_sample_format(None)
    assert eng.sample_format == "s16"


# ---- 4. the speculative one-utterance form
def speculative(make_engine, graphs):
    """Two engines with equal seeds make the same calls, one with a law and one without: every call is the one-graph form with
    a constant launch count, the law's one more than s16's; the floats and int16 are equal, the codes are g711 of the int16;
    once each format has been seen, alternating s16 / ulaw / alaw captures nothing more."""
    from piper_amd import weights as W
    cfg, _, a = make_engine()
    _, _, b = make_engine()
    one, sc = W.synthetic_phoneme_ids(20, 3, id_max=cfg.n_vocab - 1), (0.667, 1.0, 0.8)
    a.set_sample_format("ulaw")
    for e in (a, b):
        if graphs:
            e.warmup(1, 32, sample_ids=one)
        else:                                            # (the emulator captures nothing: one call gives the estimate)
            e.synthesize(one, sc)
    runs0 = a.speculation_stats[0]
    launches = []
    for k in range(3):
        r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
        launches.append(a.run_launches)
        assert a.run_launches == b.run_launches + 1, (k, a.run_launches, b.run_launches)
        check_result(r, rb, "ulaw", ("speculative", k))
    assert a.speculation_stats[0] == runs0 + 3 and len(set(launches)) == 1, (a.speculation_stats, launches)
    for fmt in ("s16", "alaw", "ulaw"):                  # each seen once ...
        a.set_sample_format(fmt)
        a.synthesize(one, sc), b.synthesize(one, sc)
    c0 = a.graph_stats[1]
    assert not graphs or c0 > 0
    for k in range(2):                                   # ... then they alternate on cached graphs
        for fmt in ("s16", "ulaw", "alaw"):
            a.set_sample_format(fmt)
            r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
            assert a.run_launches == b.run_launches + (fmt != "s16"), (fmt, a.run_launches, b.run_launches)
            if fmt == "s16":
                assert r.codes is None and np.array_equal(r.pcm[0], rb.pcm[0]) and np.array_equal(r.audio[0], rb.audio[0])
            else:
                check_result(r, rb, fmt, ("alternating", k, fmt))
    assert a.graph_stats[1] == c0, (c0, a.graph_stats)
    assert a.speculation_stats[0] == runs0 + 12, (runs0, a.speculation_stats)
    a.close()
    b.close()


# ---- 5. off is the parent
def off_is_parent(make_engine, K):
    """An engine that never had a format set and one that had it set and cleared make the same calls: equal bits, equal
    launch counts; g711_kernel is among the profile's rows only while a law is set."""
    cfg, _, fresh = make_engine()
    _, _, eng = make_engine()
    ids, nw, nz = K.inputs(cfg)
    one, sc = ids[0], (0.667, 0.5, 0.8)

    def calls(e):
        x = e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        lx = e.run_launches
        y = e.synthesize(one, sc)
        return x, lx, y, e.run_launches

    eng.set_sample_format("alaw")
    on, f1 = calls(eng), calls(fresh)
    assert (on[1], on[3]) == (f1[1] + 1, f1[3] + 1), (on[1], on[3], f1[1], f1[3])
    check_result(on[0], f1[0], "alaw", "batch")
    check_result(on[2], f1[2], "alaw", "one")
    eng.set_sample_format("s16")
    for _ in range(2):
        got, want = calls(eng), calls(fresh)
        assert (got[1], got[3]) == (want[1], want[3]), (got[1], got[3], want[1], want[3])
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            assert g.codes is None and w.codes is None
            for x, y in zip(g.audio + g.pcm, w.audio + w.pcm):
                assert x.size and np.array_equal(x, y)
    for e, fmt in ((fresh, None), (eng, "s16"), (eng, "ulaw"), (eng, "s16")):
        if fmt:
            e.set_sample_format(fmt)
        e.profile_enable(2)
        e.profile_reset()
        e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        rows = {r["name"]: r["launches"] for r in e.profile() if r["launches"] > 0}
        e.profile_enable(0)
        assert ("g711_kernel" in rows) == (fmt == "ulaw"), (fmt, sorted(rows))
        assert rows.get("pcm16_kernel") == 1 and rows.get("g711_kernel", 1) == 1, rows
    fresh.close()
    eng.close()


# ---- 6. streams
# stream settings: (name, how to set it) -- gain modes chunk, running, loudness, and the stream limiter, under which some call
# hands out nothing and the last call hands out the rest
def stream_setting(eng, name):
    if name == "chunk":
        eng.set_stream_gain("chunk")
    elif name == "running":
        eng.set_stream_gain("running", peak=0.05, ramp_ms=2.0)
    elif name == "loudness":
        eng.set_stream_loudness(-16.0, -1.0, ramp_ms=2.0)
    else:
        assert name == "limiter"
        eng.set_stream_loudness(-12.0, -1.0, ramp_ms=2.0, limiter=True, limiter_ms=10.0)


STREAM_SETTINGS = ("chunk", "running", "loudness", "limiter")


def drain_batch(eng, K, cfg, first):
    """Every chunk of the ragged batch stream, a short first chunk: [call][row] -> Chunk."""
    ids, nw, nz = K.inputs(cfg)
    return [list(item) for item in eng.stream_batch(ids, K.SCALES, chunk_frames=lambda k: first if k == 0 else K.CHUNK,
                                                    noise_w=nw, noise_z=nz)]


def drain_pool(eng, P, cfg, chunk, first, multi_speaker):
    """One listener streams, two newcomers join in mid-stream, each with a short first chunk of its own; the calls go on until
    every slot is free: [call] -> {slot: Chunk}."""
    texts = P.emu_texts(cfg, multi_speaker)
    out = []
    with eng.stream_pool(3, 64) as pool:
        pending = {s: first for s in P.join(pool, [texts[2]])}
        for k in range(200):
            out.append(pool.next(chunk, per_slot=pending))
            pending = None
            if k == 1:
                slots = P.join(pool, [texts[0], texts[1]])
                pending = {s: first for s in slots}
            if k > 1 and pool.free_slots == [0, 1, 2]:
                break
        else:
            raise AssertionError("the pool never drained")
    return out


def check_chunks(got, base, fmt, where):
    """Chunk for chunk and row for row: pcm (and the floats) equal the s16 stream's, codes == g711(pcm)."""
    assert len(got) == len(base), (where, len(got), len(base))
    delivered = empty_calls = 0
    for k, (g, w) in enumerate(zip(got, base)):
        rows = sorted(g) if isinstance(g, dict) else range(len(g))
        assert not isinstance(g, dict) or sorted(g) == sorted(w), (where, k)
        n = 0
        for b in rows:
            assert w[b].codes is None and g[b].codes is not None, (where, k, b)
            assert np.array_equal(g[b].pcm, w[b].pcm) and np.array_equal(g[b].audio, w[b].audio), (where, k, b)
            assert g[b].codes.dtype == np.uint8 and np.array_equal(g[b].codes, g711(fmt, g[b].pcm)), (where, k, b)
            n += g[b].pcm.size
        delivered += n
        empty_calls += n == 0
    assert delivered > 0, where
    return empty_calls


# (setting, kind): the full cross product; the emulator tests run a covering subset of it
STREAM_CASES = tuple((name, kind) for name in STREAM_SETTINGS for kind in ("batch", "pool"))


def check_streams(eng, cfg, K, P, rate, cases=STREAM_CASES, fmts=FORMATS, multi_speaker=False):
    """Batch stream and pool (a newcomer joins in mid-stream, short first chunks) under the given stream settings at one rate,
    each law against the s16 stream. With the stream limiter the first chunk is one frame, shorter than what the limiter
    holds back: that call hands out nothing, and the last one hands out the rest."""
    eng.set_output_rate(rate or 0)
    for name, kind in cases:
        stream_setting(eng, name)
        first = 1 if name == "limiter" else 2
        if kind == "batch":
            drain = lambda: drain_batch(eng, K, cfg, first)                                      # noqa: E731
        else:
            drain = lambda: drain_pool(eng, P, cfg, K.CHUNK, first, multi_speaker)               # noqa: E731
        eng.set_sample_format("s16")
        base = drain()
        for fmt in fmts:
            eng.set_sample_format(fmt)
            empty = check_chunks(drain(), base, fmt, (rate, name, kind, fmt))
            if name == "limiter":
                assert empty > 0, "vacuous: the limiter held nothing back"
    eng.set_sample_format("s16")
    eng.set_stream_gain("chunk")


def check_one_stream(eng, cfg, K, rate, settings=("chunk", "limiter")):
    """Engine.stream(..., codes=True): triples, the pairs of the s16 stream and the host twin's codes; without codes=True the
    pairs stay pairs, and under s16 the third entry is None."""
    ids, nw, nz = K.inputs(cfg)
    eng.set_output_rate(rate or 0)
    kw = dict(chunk_frames=K.CHUNK, noise_w=nw[1], noise_z=nz[1])
    for i, name in enumerate(settings):
        stream_setting(eng, name)
        eng.set_sample_format("s16")
        base = list(eng.stream(ids[1], K.SCALES[1], **kw))
        assert all(len(t) == 2 for t in base)
        if i == 0:
            assert all(len(t) == 3 and t[2] is None for t in eng.stream(ids[1], K.SCALES[1], codes=True, **kw))
        for fmt in FORMATS:
            eng.set_sample_format(fmt)
            got = list(eng.stream(ids[1], K.SCALES[1], codes=True, **kw))
            assert len(got) == len(base) > 2
            for (a, p, c), (a0, p0) in zip(got, base):
                assert np.array_equal(a, a0) and np.array_equal(p, p0)
                assert c is not None and c.dtype == np.uint8 and np.array_equal(c, g711(fmt, p))
            assert sum(p.size for _, p, _ in got) > 0
        if i == 0:
            assert all(len(t) == 2 for t in eng.stream(ids[1], K.SCALES[1], **kw))
    eng.set_sample_format("s16")
    eng.set_stream_gain("chunk")


def check_refusals(eng, cfg, K, P):
    """An unknown format is refused by name; so is a change while a stream is live or a pool is open, with set_output_rate's
    wording; nothing changes then."""
    import pytest
    from piper_amd.engine import EngineError
    ids, nw, nz = K.inputs(cfg)
    with pytest.raises(EngineError, match="7"):
        eng._check(eng._lib.pe_set_sample_format(eng._h, 7))
    with pytest.raises(EngineError, match="g722"):
        eng.set_sample_format("g722")
    eng.set_sample_format("ulaw")
    for k, _ in enumerate(eng.stream(ids[1], K.SCALES[1], chunk_frames=K.CHUNK, noise_w=nw[1], noise_z=nz[1])):
        if k == 0:
            with pytest.raises(EngineError, match="sample format cannot change while a stream is live"):
                eng.set_sample_format("alaw")
            assert eng.sample_format == "ulaw"
    eng.set_sample_format("alaw")                        # the stream has ended
    for k, _ in enumerate(eng.stream_batch(ids, K.SCALES, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)):
        if k == 0:
            with pytest.raises(EngineError, match="sample format cannot change while a stream is live"):
                eng.set_sample_format("s16")
            assert eng.sample_format == "alaw"
    with eng.stream_pool(2, 48):
        with pytest.raises(EngineError, match="sample format cannot change while a stream pool is open"):
            eng.set_sample_format("s16")
        assert eng.sample_format == "alaw"
    eng.set_sample_format("s16")
    with pytest.raises(EngineError, match="format"):
        eng.debug_g711("s16", [np.zeros(4, np.int16)])


# ---- 7. fronts
def parse_wav(blob):
    """The chunks of a RIFF/WAVE file, {id: payload}, the RIFF size checked against the file's."""
    import struct
    assert blob[:4] == b"RIFF" and blob[8:12] == b"WAVE" and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8
    pos, chunks = 12, {}
    while pos < len(blob):
        cid, n = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        chunks[cid] = blob[pos + 8:pos + 8 + n]
        pos += 8 + n + (n & 1)
    return chunks


def check_g711_wav(blob, fmt, rate, codes):
    """The header written by hand: an 18-byte fmt chunk (tag 7 mu-law / 6 A-law, mono, byte rate = rate, block align 1, 8
    bits, cbSize 0), a fact chunk with the sample count, the data."""
    import struct
    ch = parse_wav(blob)
    assert list(ch) == [b"fmt ", b"fact", b"data"], list(ch)
    assert struct.unpack("<HHIIHHH", ch[b"fmt "]) == ({"ulaw": 7, "alaw": 6}[fmt], 1, rate, rate, 1, 8, 0)
    assert struct.unpack("<I", ch[b"fact"])[0] == len(codes) == len(ch[b"data"])
    assert ch[b"data"] == codes


def check_voice(voice, tmp_path):
    """PiperVoice on the text voice, two sentences with sentence silence: under a law the *_raw methods return code bytes --
    g711 of the s16 bytes --, the silence is the law's zero code (0xFF / 0xD5, never 0x00), decoding the whole stream gives
    the s16 stream with zeros in the gaps passed through encode -> decode, and synthesize writes a G.711 WAV."""
    from piper_amd.engine import g711_decode
    lib = voice.session._lib
    voice.phonemize = lambda text: [list(s) for s in text.split("|")]        # (two sentences of the text voice)
    kw = dict(noise_scale=0.0, noise_w=0.0, length_scale=1.5)
    text, gap = "this is a test|and one more", 0.01
    rate = voice.sample_rate
    nsil = int(gap * rate)
    ids = voice.phonemes_to_ids(list("a test"))

    def setfmt(fmt):
        voice.session.set_sample_format(fmt)
        voice.sample_format = voice.session.sample_format

    setfmt("s16")
    base = list(voice.synthesize_stream_raw(text, sentence_silence=gap, **kw))
    one = voice.synthesize_ids_to_raw(ids, **kw)
    two = voice.synthesize_ids_batch_to_raw([ids, ids[:5] + ids[-1:]], **kw)
    assert len(base) == 2 and all(b.endswith(bytes(2 * nsil)) and len(b) > 2 * nsil for b in base) and nsil > 0
    for fmt in FORMATS:
        setfmt(fmt)
        assert voice.sample_format == fmt
        got = list(voice.synthesize_stream_raw(text, sentence_silence=gap, **kw))
        assert len(got) == 2
        for g, b in zip(got, base):
            assert 2 * len(g) == len(b)
            assert g[-nsil:] == bytes([ZERO[fmt]]) * nsil and bytes([0]) * nsil != g[-nsil:]
            assert np.array_equal(np.frombuffer(g, np.uint8), g711(fmt, np.frombuffer(b, np.int16)))
        whole, whole16 = np.frombuffer(b"".join(got), np.uint8), np.frombuffer(b"".join(base), np.int16)
        assert np.array_equal(g711_decode(fmt, whole, lib), expand(fmt, g711(fmt, whole16)))
        assert np.array_equal(np.frombuffer(voice.synthesize_ids_to_raw(ids, **kw), np.uint8), g711(fmt, np.frombuffer(one, np.int16)))
        batch = voice.synthesize_ids_batch_to_raw([ids, ids[:5] + ids[-1:]], **kw)
        for g, b in zip(batch, two):
            assert len(g) and np.array_equal(np.frombuffer(g, np.uint8), g711(fmt, np.frombuffer(b, np.int16)))
        path = tmp_path / f"voice_{fmt}.wav"
        with open(path, "wb") as f:
            voice.synthesize(text, f, sentence_silence=gap, **kw)
        check_g711_wav(path.read_bytes(), fmt, rate, b"".join(got))
    setfmt("s16")


def check_infer(lib, tmp_path, model):
    """python -m piper_amd.infer --sample-format ulaw on two lines: G.711 WAVs whose data is g711 of the s16 run's data."""
    import io
    import json
    import wave
    from piper_amd import infer, weights as W
    lines = "".join(json.dumps({"phoneme_ids": [int(v) for v in W.synthetic_phoneme_ids(n, s, id_max=39)]}) + "\n"
                    for n, s in ((12, 3), (17, 4)))
    data = {}
    for fmt in ("s16", "ulaw"):
        d = tmp_path / fmt
        args = ["--model", model, "--output-dir", str(d), "--sample-rate", "16000", "--seed", "5", "--batch", "2",
                "--sample-format", fmt]
        assert infer.main(args, stdin=io.StringIO(lines), lib=lib) == 0
        data[fmt] = [(d / f"{k}.wav").read_bytes() for k in range(2)]
    for k in range(2):
        with wave.open(io.BytesIO(data["s16"][k]), "rb") as w:
            assert (w.getframerate(), w.getsampwidth()) == (16000, 2)
            pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16)
        assert pcm.size > 0
        check_g711_wav(data["ulaw"][k], "ulaw", 16000, g711("ulaw", pcm).tobytes())
