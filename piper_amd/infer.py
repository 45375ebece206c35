"""JSONL -> WAV driver for a voice .onnx, the counterpart of the reference's
``python -m piper_train.infer_onnx`` (reference src/python/piper_train/infer_onnx.py:19-102): one JSON object
per stdin line with ``phoneme_ids`` (and optionally ``speaker_id``), one ``<line index>.wav`` per utterance in
``--output-dir``, same scale options and defaults. The ONNX Runtime session is replaced by the HIP engine;
``--batch N`` (new) groups N consecutive lines into one batched GPU call. A line may carry its own ``length_scale``,
``noise_scale`` and / or ``noise_w`` (new): they override the command-line values for that utterance alone, and the group
it belongs to still runs as one call (one scale triple per utterance). ``--output-rate R`` (new) delivers the audio at R Hz,
resampled on the GPU from ``--sample-rate`` (the voice's own rate); the WAV headers then say R. A line may also carry
``durations`` (one int per id: >= 0 that id's frames, -1 predicted), ``rate`` (one multiplier per id) and / or
``target_seconds`` (the utterance's exact length, converted to frames with ``--sample-rate`` and the voice's hop) (new): a
group with such a line runs as one timed call; a group without is the call it always was. ``--seed N`` gives the utterance
of line k (the index that names its WAV) the noise seed ``N + k``, and a line's own ``seed`` overrides it (new): a seeded
line's audio depends on the voice, the line and its seed alone -- not on ``--batch``, the lines around it or the run -- and
lines without a seed draw from the engine's own stream in the same call. ``--speaker-blend 1:0.7,3:0.3`` (ids, or names from
the ``speaker_id_map`` of the ``.json`` beside the model) speaks every line with that weighted mix of speaker embeddings, the
weights used as given; a line's ``"speaker_blend": {"1": 0.7, "3": 0.3}`` or ``"speaker_vector": [...]`` (the embedding
itself) or its ``speaker_id`` wins over the option, and ``speaker_id`` beside either key on one line is an error that names
the line (new). ``--sample-format ulaw|alaw`` (new) writes G.711 WAVs -- 8-bit mu-law or A-law, format tag 7 / 6, with a
``fact`` chunk --, the codes companded on the GPU from the int16 the default format would have written.

    python -m piper_amd.infer --model voice.onnx --output-dir out/ < utterances.jsonl
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
import time
import wave
from pathlib import Path
from typing import Iterable, List, Optional, Tuple

from .engine import Engine, Timing

_LOGGER = logging.getLogger("piper_amd.infer")


def read_utterances(lines: Iterable[str]) -> List[Tuple[int, List[int], Optional[int]]]:
    """(line index, phoneme ids, speaker id) for every non-empty line; the index names the WAV file, as in
    the reference (blank lines keep their number)."""
    utts = []
    for i, line in enumerate(lines):
        line = line.strip()
        if not line:
            continue
        obj = json.loads(line)
        utts.append((i, [int(p) for p in obj["phoneme_ids"]], obj.get("speaker_id")))
    return utts


SCALE_KEYS = ("noise_scale", "length_scale", "noise_w")      # the order of an engine scale triple


def read_scales(lines: Iterable[str], default: Tuple[float, float, float]) -> List[Optional[Tuple[float, float, float]]]:
    """Per non-empty line (the order of read_utterances): its (noise_scale, length_scale, noise_w) with the line's own
    keys over ``default``, or None when the line sets none of them."""
    out: List[Optional[Tuple[float, float, float]]] = []
    for line in lines:
        line = line.strip()
        if not line:
            continue
        obj = json.loads(line)
        if not any(k in obj for k in SCALE_KEYS):
            out.append(None)
            continue
        out.append(tuple(float(obj[k]) if k in obj else float(d) for k, d in zip(SCALE_KEYS, default)))
    return out


TIMING_KEYS = ("durations", "rate", "target_seconds")


def read_timing(lines: Iterable[str]) -> List[Optional[dict]]:
    """Per non-empty line (the order of read_utterances): its timing keys as a dict, or None when it has none of them."""
    out: List[Optional[dict]] = []
    for line in lines:
        line = line.strip()
        if not line:
            continue
        obj = json.loads(line)
        out.append({k: obj[k] for k in TIMING_KEYS if k in obj} or None)
    return out


def read_seeds(lines: Iterable[str], base: Optional[int]) -> List[Optional[int]]:
    """Per non-empty line (the order of read_utterances): its noise seed modulo 2^64 -- the line's own ``seed``, else
    ``base`` + the line's index -- or None where there is neither."""
    out: List[Optional[int]] = []
    for i, line in enumerate(lines):
        line = line.strip()
        if not line:
            continue
        obj = json.loads(line)
        if obj.get("seed") is not None:
            out.append(int(obj["seed"]) % (1 << 64))
        else:
            out.append(None if base is None else (int(base) + i) % (1 << 64))
    return out


def parse_blend(text: str, names: Optional[dict] = None) -> List[Tuple[int, float]]:
    """``1:0.7,3:0.3`` -> [(1, 0.7), (3, 0.3)], the order kept; a speaker is an id or a name from ``names``."""
    return blend_pairs([tuple(part.rsplit(":", 1)) for part in text.split(",") if part.strip()], names, "--speaker-blend")


def blend_pairs(items, names: Optional[dict], where: str) -> List[Tuple[int, float]]:
    out = []
    for item in items:
        if len(item) != 2:
            raise ValueError(f"{where}: a blend component is speaker:weight, got {item!r}")
        who, weight = item
        who = who.strip() if isinstance(who, str) else who
        if isinstance(who, str) and names and who in names:
            who = names[who]
        try:
            out.append((int(who), float(weight)))
        except ValueError:
            raise ValueError(f"{where}: no speaker {who!r}") from None
    if not out:
        raise ValueError(f"{where}: an empty blend")
    return out


def read_speakers(lines: Iterable[str], default: Optional[List[Tuple[int, float]]], names: Optional[dict] = None) -> list:
    """Per non-empty line (the order of read_utterances): its entry of Engine's ``speakers`` -- the line's own
    ``speaker_blend`` ({speaker: weight}, the order kept) or ``speaker_vector`` (a list of floats), else its ``speaker_id``,
    else ``default`` (the --speaker-blend option), else None. ``speaker_id`` beside either key on one line, or both keys, is an
    error that names the line (counted from 1)."""
    out = []
    for i, line in enumerate(lines):
        line = line.strip()
        if not line:
            continue
        obj = json.loads(line)
        blend, vector, sid = obj.get("speaker_blend"), obj.get("speaker_vector"), obj.get("speaker_id")
        if (blend is not None) + (vector is not None) + (sid is not None) > 1:
            raise ValueError(f"line {i + 1}: give one of speaker_id, speaker_blend and speaker_vector, not several")
        if blend is not None:
            out.append(blend_pairs(list(blend.items()), names, f"line {i + 1}"))
        elif vector is not None:
            out.append([float(x) for x in vector])
        elif sid is not None:
            out.append(int(sid))
        else:
            out.append(default)
    return out


def group_timing(own: List[Optional[dict]], native_rate: int, hop: int) -> Optional[Timing]:
    """The plan of a group of lines, or None when no line of it carries a timing key."""
    if all(t is None for t in own):
        return None
    get = lambda t, k: None if t is None else t.get(k)      # noqa: E731
    secs = [get(t, "target_seconds") for t in own]
    return Timing(rate=[get(t, "rate") for t in own], durations=[get(t, "durations") for t in own],
                  target_frames=[0 if s is None else int(round(float(s) * native_rate / hop)) for s in secs])


def write_wav(path: Path, sample_rate: int, pcm) -> None:
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


def main(argv=None, *, stdin=None, lib=None) -> int:
    parser = argparse.ArgumentParser(prog="piper_amd.infer")
    parser.add_argument("--model", required=True, help="Path to model (.onnx)")
    parser.add_argument("--output-dir", required=True, help="Path to write WAV files")
    parser.add_argument("--sample-rate", type=int, default=22050)
    parser.add_argument("--output-rate", type=int, default=0,
                        help="deliver the audio at this rate, resampled on the GPU from --sample-rate (0: off)")
    parser.add_argument("--target-lufs", type=float, default=None,
                        help="deliver every utterance at this integrated loudness (ITU-R BS.1770-4, LUFS; default: peak-normalised)")
    parser.add_argument("--peak-ceiling-db", type=float, default=-1.0, help="peak ceiling in dB with --target-lufs (sample peak; with --true-peak: dBTP)")
    parser.add_argument("--true-peak", action="store_true",
                        help="hold the ceiling as a true peak (ITU-R BS.1770-4 Annex 2), measured on the GPU; with --target-lufs")
    parser.add_argument("--limiter", action="store_true",
                        help="where the ceiling and --target-lufs conflict, turn down only the peaks (look-ahead limiter on the GPU)")
    parser.add_argument("--limiter-ms", type=float, default=5.0, help="window of --limiter in ms, 1 to 10")
    parser.add_argument("--sample-format", choices=("s16", "ulaw", "alaw"), default="s16",
                        help="ulaw / alaw: write G.711 WAVs (8-bit mu-law / A-law), companded on the GPU")
    parser.add_argument("--noise-scale", type=float, default=0.667)
    parser.add_argument("--noise-scale-w", type=float, default=0.8)
    parser.add_argument("--length-scale", type=float, default=1.0)
    parser.add_argument("--batch", type=int, default=1, help="utterances per GPU call")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--seed", type=int, default=None,
                        help="noise seed: line k gets seed + k, whatever --batch; a line's own \"seed\" overrides it")
    parser.add_argument("--speaker-blend", default=None,
                        help="blend of speakers for every line, e.g. 1:0.7,3:0.3 (ids, or names from the model's .json); "
                             "a line's own speaker_id, \"speaker_blend\" or \"speaker_vector\" overrides it")
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG)

    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    engine = Engine(onnx_path=str(args.model), device=args.device, lib=lib)
    _LOGGER.info("Loaded model from %s", args.model)
    wav_rate = args.sample_rate
    if args.output_rate:
        engine.set_output_rate(args.output_rate, native=args.sample_rate)
        wav_rate = args.output_rate
    if args.target_lufs is not None:
        if not args.output_rate:
            engine.set_output_rate(None, native=args.sample_rate)      # (an .onnx carries no rate of its own)
        engine.set_loudness(args.target_lufs, args.peak_ceiling_db, true_peak=args.true_peak, limiter=args.limiter,
                            limiter_ms=args.limiter_ms)
    engine.set_sample_format(args.sample_format)
    scales = (args.noise_scale, args.length_scale, args.noise_scale_w)
    lines = list(stdin if stdin is not None else sys.stdin)
    utts = read_utterances(lines)
    line_scales = read_scales(lines, scales)
    line_timing = read_timing(lines)
    line_seeds = read_seeds(lines, args.seed)
    names = None
    conf = Path(str(args.model) + ".json")
    if conf.is_file():
        names = json.loads(conf.read_text(encoding="utf-8")).get("speaker_id_map") or None
    line_speakers = read_speakers(lines, None if args.speaker_blend is None else parse_blend(args.speaker_blend, names), names)
    step = max(1, args.batch)
    for k in range(0, len(utts), step):
        group = utts[k:k + step]
        sids = [u[2] for u in group]
        own = line_scales[k:k + step]
        # lines without scale keys: the command-line triple; any line with its own: one triple per utterance
        call_scales = scales if all(s is None for s in own) else [scales if s is None else s for s in own]
        t0 = time.perf_counter()
        timing = group_timing(line_timing[k:k + step], args.sample_rate, engine.hop)
        extra = {} if timing is None else {"timing": timing}
        seeds = line_seeds[k:k + step]
        if any(s is not None for s in seeds):
            extra["seeds"] = seeds
        speakers = line_speakers[k:k + step]
        if any(isinstance(s, list) for s in speakers):        # a blend or a vector in the group: every speaker goes this way
            extra["speakers"] = speakers
            sids = [None] * len(group)
        res = engine.synthesize_batch([u[1] for u in group], call_scales,
                                      sids=None if all(s is None for s in sids) else [s or 0 for s in sids], **extra)
        infer_sec = time.perf_counter() - t0
        audio_sec = sum(p.shape[-1] for p in res.pcm) / wav_rate
        _LOGGER.debug("Real-time factor for %s..%s: %0.4f (infer=%0.4f sec, audio=%0.2f sec)", group[0][0] + 1,
                      group[-1][0] + 1, infer_sec / audio_sec if audio_sec > 0 else 0.0, infer_sec, audio_sec)
        for b, ((idx, _, _), pcm) in enumerate(zip(group, res.pcm)):
            if args.sample_format != "s16":
                from .voice import write_g711_wav
                with open(out_dir / f"{idx}.wav", "wb") as f:
                    write_g711_wav(f, args.sample_format, wav_rate, res.codes[b].tobytes())
                continue
            write_wav(out_dir / f"{idx}.wav", wav_rate, pcm)
    engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
