"""``PiperVoice`` -- host-side mirror of the reference's Python runtime class
(reference src/python_run/piper/voice.py:20-185): same constructor surface (``load``), same
``phonemes_to_ids`` / ``synthesize_ids_to_raw`` / ``synthesize_stream_raw`` / ``synthesize``
signatures, argument meaning and defaults. The one difference is what sits behind it: the
``onnxruntime.InferenceSession`` is replaced by the MI355X HIP engine (libpiper_hip.so), which reads
the same ``.onnx`` file; the float->int16 conversion (util.py:5-12) runs on the GPU as well.

Phonemisation stays on the host and is out of scope (BASELINE.json north_star): ``phonemize`` handles
``phoneme_type: text`` voices natively (unicode code points after NFD normalisation, as
piper-phonemize's ``phonemize_codepoints`` does) and defers to the optional ``piper_phonemize``
package for espeak voices."""
from __future__ import annotations

import json
import logging
import struct
import unicodedata
import wave
from dataclasses import dataclass
from pathlib import Path
from typing import Iterable, List, Optional, Union

import numpy as np

from .config import PhonemeType, PiperConfig
from .engine import Engine, Timing

PAD = "_"  # padding (0)        -- reference const.py
BOS = "^"  # beginning of sentence
EOS = "$"  # end of sentence


def phonemes_to_ids_cpp(phonemes, id_map, intersperse_pad: bool = True) -> List[int]:
    """The C++ front end's rule (piper-phonemize ``phonemes_to_ids`` as called at reference
    src/cpp/piper.cpp:555 with the defaults of piper.hpp:44-47): BOS, PAD, then id(s)+PAD per phoneme,
    EOS -- i.e. one more PAD after BOS than the Python runtime emits. This is the sequence the shipped
    voices were trained on; the reference's etc/test_sentences fixtures pin it."""
    ids: List[int] = list(id_map[BOS])
    if intersperse_pad:
        ids.extend(id_map[PAD])
    for phoneme in phonemes:
        if phoneme not in id_map:
            continue
        ids.extend(id_map[phoneme])
        if intersperse_pad:
            ids.extend(id_map[PAD])
    ids.extend(id_map[EOS])
    return ids


_LOGGER = logging.getLogger(__name__)

# G.711 sample formats (Engine.set_sample_format): the WAVE format tag and the code of a zero sample, which is what silence
# is padded with -- 0x00 is full-scale negative in mu-law
G711_WAV_TAG = {"ulaw": 7, "alaw": 6}
G711_ZERO = {"ulaw": b"\xff", "alaw": b"\xd5"}


def write_g711_wav(f, sample_format: str, sample_rate: int, codes: bytes):
    """A mono G.711 WAV into the binary file ``f``. The ``wave`` module writes PCM only, so the header is written by hand:
    an 18-byte ``fmt `` chunk (tag 7 mu-law / 6 A-law, 1 channel, rate, byte rate = rate, block align 1, 8 bits, cbSize
    0), a ``fact`` chunk with the sample count, then ``data`` (padded to an even length, as RIFF asks)."""
    n = len(codes)
    pad = n & 1
    f.write(b"RIFF" + struct.pack("<I", 4 + (8 + 18) + (8 + 4) + (8 + n + pad)) + b"WAVE")
    f.write(b"fmt " + struct.pack("<IHHIIHHH", 18, G711_WAV_TAG[sample_format], 1, int(sample_rate), int(sample_rate), 1, 8, 0))
    f.write(b"fact" + struct.pack("<II", 4, n))
    f.write(b"data" + struct.pack("<I", n))
    f.write(codes)
    if pad:
        f.write(b"\0")


@dataclass
class PiperVoice:
    session: Engine
    config: PiperConfig
    output_sample_rate: Optional[int] = None      # None: the voice's own rate (config.sample_rate)
    sample_format: str = "s16"                    # "ulaw" / "alaw": the *_raw methods return G.711 code bytes

    @staticmethod
    def load(model_path: Union[str, Path], config_path: Optional[Union[str, Path]] = None,
             use_cuda: bool = True, device: int = 0, output_sample_rate: Optional[int] = None,
             target_lufs: Optional[float] = None, peak_ceiling_db: float = -1.0, true_peak: bool = False,
             limiter: bool = False, limiter_ms: float = 5.0, sample_format: Optional[str] = None) -> "PiperVoice":
        """Load an ONNX voice and its config. ``use_cuda`` is accepted for signature compatibility;
        the engine always runs on the GPU (``device``). ``output_sample_rate`` (new): deliver the audio at this rate,
        resampled on the GPU before the int16 conversion (Engine.set_output_rate; the config's rate is the native one).
        ``target_lufs`` (new): deliver every whole utterance at this integrated loudness (ITU-R BS.1770-4, mono) under a
        ceiling of ``peak_ceiling_db`` dB on the sample peak, or with ``true_peak`` on the true peak (dBTP, BS.1770-4
        Annex 2) as well (Engine.set_loudness); ``limiter``: where ceiling and target conflict, only the peaks are turned
        down, by a zero-phase window of ``limiter_ms`` (1 to 10; either kind of ceiling). Streams keep their chunk rule.
        ``sample_format`` (new): ``"ulaw"`` or ``"alaw"`` -- the ``*_raw`` methods then return G.711 code bytes, one per
        sample, companded on the GPU (Engine.set_sample_format), sentence silence is the law's zero code, and
        ``synthesize`` writes a G.711 WAV; None or ``"s16"``: 16-bit PCM as ever."""
        if config_path is None:
            config_path = f"{model_path}.json"
        with open(config_path, "r", encoding="utf-8") as config_file:
            config_dict = json.load(config_file)
        config = PiperConfig.from_dict(config_dict)
        session = Engine(onnx_path=str(model_path), device=device)
        if output_sample_rate:
            session.set_output_rate(int(output_sample_rate), native=int(config.sample_rate))
        if target_lufs is not None:
            if not output_sample_rate:
                session.set_output_rate(None, native=int(config.sample_rate))      # (an .onnx carries no rate of its own)
            session.set_loudness(float(target_lufs), float(peak_ceiling_db), true_peak=bool(true_peak), limiter=bool(limiter),
                                 limiter_ms=float(limiter_ms))
        elif true_peak or limiter:                           # (remembered for a later set_loudness)
            session.set_loudness(None, true_peak=bool(true_peak), limiter=bool(limiter), limiter_ms=float(limiter_ms))
        session.set_sample_format(sample_format)
        return PiperVoice(config=config, session=session, output_sample_rate=output_sample_rate or None,
                          sample_format=session.sample_format)

    @property
    def sample_rate(self) -> int:
        """The rate of the audio this voice delivers: ``output_sample_rate`` when set, else the config's."""
        return int(self.output_sample_rate or self.config.sample_rate)

    def phonemize(self, text: str) -> List[List[str]]:
        """Text to phonemes grouped by sentence."""
        if self.config.phoneme_type == PhonemeType.TEXT:
            # piper_phonemize.phonemize_codepoints with its default casing: full case folding, then NFD; one sentence
            return [list(unicodedata.normalize("NFD", text.casefold()))]
        if self.config.phoneme_type == PhonemeType.ESPEAK:
            try:
                from piper_phonemize import phonemize_espeak, tashkeel_run  # type: ignore
            except ImportError as e:
                raise RuntimeError(
                    "espeak phonemisation needs the piper_phonemize package on the host "
                    "(out of scope for the GPU engine); pass phoneme ids to synthesize_ids_to_raw") from e
            if self.config.espeak_voice == "ar":
                text = tashkeel_run(text)
            return phonemize_espeak(text, self.config.espeak_voice)
        raise ValueError(f"Unexpected phoneme type: {self.config.phoneme_type}")

    def phonemes_to_ids(self, phonemes: List[str]) -> List[int]:
        """Phonemes to ids (voice.py:72-87: BOS, then id(s)+PAD per phoneme, then EOS)."""
        id_map = self.config.phoneme_id_map
        ids: List[int] = list(id_map[BOS])
        for phoneme in phonemes:
            if phoneme not in id_map:
                _LOGGER.warning("Missing phoneme from id map: %s", phoneme)
                continue
            ids.extend(id_map[phoneme])
            ids.extend(id_map[PAD])
        ids.extend(id_map[EOS])
        return ids

    def synthesize(self, text: str, wav_file: wave.Wave_write, speaker_id: Optional[int] = None,
                   length_scale: Optional[float] = None, noise_scale: Optional[float] = None,
                   noise_w: Optional[float] = None, sentence_silence: float = 0.0, seed: Optional[int] = None,
                   speaker_blend=None, speaker_vector=None):
        """Synthesize WAV audio from text. ``seed``, ``speaker_blend`` and ``speaker_vector``: as in synthesize_stream_raw.
        With a G.711 ``sample_format`` the ``wave`` module cannot write the file: ``wav_file`` is then a binary file
        object, and gets a mu-law / A-law WAV (write_g711_wav)."""
        if self.sample_format != "s16":
            codes = b"".join(self.synthesize_stream_raw(text, speaker_id=speaker_id, length_scale=length_scale,
                                                        noise_scale=noise_scale, noise_w=noise_w,
                                                        sentence_silence=sentence_silence, seed=seed,
                                                        speaker_blend=speaker_blend, speaker_vector=speaker_vector))
            write_g711_wav(wav_file, self.sample_format, self.sample_rate, codes)
            return
        wav_file.setframerate(self.sample_rate)
        wav_file.setsampwidth(2)
        wav_file.setnchannels(1)
        for audio_bytes in self.synthesize_stream_raw(text, speaker_id=speaker_id, length_scale=length_scale,
                                                      noise_scale=noise_scale, noise_w=noise_w,
                                                      sentence_silence=sentence_silence, seed=seed,
                                                      speaker_blend=speaker_blend, speaker_vector=speaker_vector):
            wav_file.writeframes(audio_bytes)

    def synthesize_stream_raw(self, text: str, speaker_id: Optional[int] = None,
                              length_scale: Optional[float] = None, noise_scale: Optional[float] = None,
                              noise_w: Optional[float] = None, sentence_silence: float = 0.0,
                              seed: Optional[int] = None, speaker_blend=None, speaker_vector=None) -> Iterable[bytes]:
        """Synthesize raw audio per sentence from text. ``seed``: sentence k of the text gets the noise seed ``seed + k``
        (wrapping at 2^64), so that the same text with the same settings gives the same audio on any handle.
        ``speaker_blend`` / ``speaker_vector``: every sentence's speaker, as in synthesize_ids_to_raw."""
        sentence_phonemes = self.phonemize(text)
        num_silence_samples = int(sentence_silence * self.sample_rate)
        if self.sample_format != "s16":                      # one byte per sample, the law's zero code
            silence_bytes = G711_ZERO[self.sample_format] * num_silence_samples
        else:
            silence_bytes = bytes(num_silence_samples * 2)
        for k, phonemes in enumerate(sentence_phonemes):
            phoneme_ids = self.phonemes_to_ids(phonemes)
            yield self.synthesize_ids_to_raw(phoneme_ids, speaker_id=speaker_id, length_scale=length_scale,
                                             noise_scale=noise_scale, noise_w=noise_w,
                                             seed=None if seed is None else (int(seed) + k) % (1 << 64),
                                             speaker_blend=speaker_blend, speaker_vector=speaker_vector) + silence_bytes

    def _scales(self, length_scale, noise_scale, noise_w):
        if length_scale is None:
            length_scale = self.config.length_scale
        if noise_scale is None:
            noise_scale = self.config.noise_scale
        if noise_w is None:
            noise_w = self.config.noise_w
        return (noise_scale, length_scale, noise_w)

    def _speaker(self, speaker_id):
        if self.config.num_speakers <= 1:
            return None
        return 0 if speaker_id is None else speaker_id

    def _speaker_entry(self, speaker_id, speaker_blend, speaker_vector):
        """One utterance's entry of Engine's ``speakers`` from at most one of an id, a blend and a vector, or None when the
        utterance has a plain id. A blend is a mapping ``{speaker: weight}`` or a sequence of ``(speaker, weight)`` pairs,
        its order kept; a speaker is an id or a name from the config's ``speaker_id_map``."""
        if (speaker_id is not None) + (speaker_blend is not None) + (speaker_vector is not None) > 1:
            raise ValueError("give at most one of speaker_id, speaker_blend and speaker_vector")
        if speaker_vector is not None:
            return np.asarray(speaker_vector, np.float32).reshape(-1)
        if speaker_blend is None:
            return None
        names = getattr(self.config, "speaker_id_map", None) or {}
        out = []
        for who, weight in (speaker_blend.items() if isinstance(speaker_blend, dict) else speaker_blend):
            if isinstance(who, str) and who in names:
                who = names[who]
            elif isinstance(who, str) and who.lstrip("-").isdigit():
                who = int(who)
            elif isinstance(who, str):
                raise ValueError(f"speaker_blend: no speaker named {who!r} in speaker_id_map")
            out.append((int(who), float(weight)))
        return out

    def target_frames(self, seconds: Optional[float]) -> int:
        """A length in seconds as spectrogram frames of this voice: round(seconds * native rate / hop) with the
        config's sample rate as the native one; None: 0, no target."""
        if seconds is None:
            return 0
        return int(round(float(seconds) * int(self.config.sample_rate) / self.session.hop))

    def _timing(self, durations, rate, target_seconds) -> Optional[Timing]:
        """The plan of a call from per-utterance lists (None: nothing of that kind), or None for an untimed call."""
        if durations is None and rate is None and target_seconds is None:
            return None
        return Timing(rate=rate, durations=durations,
                      target_frames=None if target_seconds is None else [self.target_frames(s) for s in target_seconds])

    def synthesize_ids_to_raw(self, phoneme_ids: List[int], speaker_id: Optional[int] = None,
                              length_scale: Optional[float] = None, noise_scale: Optional[float] = None,
                              noise_w: Optional[float] = None, durations=None, rate=None,
                              target_seconds: Optional[float] = None, seed: Optional[int] = None,
                              speaker_blend=None, speaker_vector=None) -> bytes:
        """Synthesize raw 16-bit mono audio from phoneme ids (voice.py:140-185). New, all optional (Engine's ``Timing``):
        ``durations`` -- one int per id, >= 0 = that id lasts exactly so many frames, -1 = predicted; ``rate`` -- one
        multiplier of the predicted duration per id; ``target_seconds`` -- the utterance lasts
        round(seconds * native rate / hop) frames exactly (the byte count follows from the output rate); ``seed`` -- the
        utterance's noise seed (Engine's ``seeds``): its audio then depends on the voice, the ids, the settings and the seed
        alone, not on what the handle served before; ``speaker_blend`` -- ``{speaker: weight}`` or ``(speaker, weight)``
        pairs, ids or names from ``speaker_id_map``: a weighted mix of speaker embeddings, weights used as given;
        ``speaker_vector`` -- ``Engine.speaker_dim`` floats used as the speaker embedding itself (Engine's ``speakers``).
        At most one of ``speaker_id``, ``speaker_blend`` and ``speaker_vector``."""
        timing = self._timing(None if durations is None else [durations], None if rate is None else [rate],
                              None if target_seconds is None else [target_seconds])
        entry = self._speaker_entry(speaker_id, speaker_blend, speaker_vector)
        if entry is not None:
            r = self.session.synthesize_batch([phoneme_ids], self._scales(length_scale, noise_scale, noise_w), timing=timing,
                                              seeds=None if seed is None else [seed], speakers=[entry])
        elif timing is None and seed is None:
            r = self.session.synthesize(phoneme_ids, self._scales(length_scale, noise_scale, noise_w),
                                        sid=self._speaker(speaker_id))
        else:
            sid = self._speaker(speaker_id)
            r = self.session.synthesize_batch([phoneme_ids], self._scales(length_scale, noise_scale, noise_w),
                                              sids=None if sid is None else [sid], timing=timing,
                                              seeds=None if seed is None else [seed])
        return self._raw(r)[0]

    def _raw(self, r) -> List[bytes]:
        """What the *_raw methods return per utterance: the int16 bytes, or the G.711 codes under a sample format."""
        if self.sample_format != "s16":
            if r.codes is None:
                raise RuntimeError(f"the engine delivered no codes: its sample format is not {self.sample_format!r}")
            return [c.tobytes() for c in r.codes]
        return [p.tobytes() for p in r.pcm]

    def synthesize_ids_batch_to_raw(self, phoneme_id_lists: List[List[int]], speaker_ids=None,
                                    length_scale: Optional[float] = None, noise_scale: Optional[float] = None,
                                    noise_w: Optional[float] = None, durations=None, rate=None,
                                    target_seconds=None, seeds=None, speaker_blend=None, speaker_vector=None) -> List[bytes]:
        """Batched extension: several utterances in one GPU call, each identical to its own
        synthesize_ids_to_raw() (same noise stream aside). ``length_scale`` / ``noise_scale`` / ``noise_w`` may each be
        one value for every utterance or a list with one value per utterance (None entries: the voice's default).
        ``durations`` / ``rate`` / ``target_seconds``: lists with one entry per utterance as in synthesize_ids_to_raw
        (None entries: nothing of that kind for that utterance). ``seeds``: one noise seed or None per utterance; a seeded
        utterance is then identical to its own seeded synthesize_ids_to_raw(), noise included. ``speaker_blend`` /
        ``speaker_vector``: lists with one entry per utterance as in synthesize_ids_to_raw (None entries: a plain id)."""
        sids = None
        n = len(phoneme_id_lists)
        if self.config.num_speakers > 1:
            sids = [0 if s is None else s for s in (speaker_ids or [None] * n)]
        speakers = None
        if speaker_blend is not None or speaker_vector is not None:
            for what, v in (("speaker_blend", speaker_blend), ("speaker_vector", speaker_vector), ("speaker_ids", speaker_ids)):
                if v is not None and len(v) != n:
                    raise ValueError(f"{what}: {len(v)} entries for {n} utterances")
            speakers = [self._speaker_entry(None if speaker_ids is None else speaker_ids[i],
                                            None if speaker_blend is None else speaker_blend[i],
                                            None if speaker_vector is None else speaker_vector[i]) for i in range(n)]
            speakers = [(sids[i] if sids is not None else None) if e is None else e for i, e in enumerate(speakers)]
            sids = None
        knobs = (length_scale, noise_scale, noise_w)
        if any(isinstance(v, (list, tuple)) for v in knobs):
            def at(v, i):
                if not isinstance(v, (list, tuple)):
                    return v
                if len(v) != n:
                    raise ValueError(f"{len(v)} per-utterance scale values for {n} utterances")
                return v[i]
            scales = [self._scales(*(at(v, i) for v in knobs)) for i in range(n)]
        else:
            scales = self._scales(length_scale, noise_scale, noise_w)
        timing = self._timing(durations, rate, target_seconds)
        if speakers is not None:
            r = self.session.synthesize_batch(phoneme_id_lists, scales, timing=timing, seeds=seeds, speakers=speakers)
        elif timing is None and seeds is None:
            r = self.session.synthesize_batch(phoneme_id_lists, scales, sids=sids)
        else:
            r = self.session.synthesize_batch(phoneme_id_lists, scales, sids=sids, timing=timing, seeds=seeds)
        return self._raw(r)
