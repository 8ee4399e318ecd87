"""``csm-generate`` on MI355X: flag names and defaults of reference ``src/csm/cli/generate.py:28-105``.  The two things the
reference downloads from the hub are passed as local files (``--mimi-weights``, ``--text-tokenizer``); WAV I/O goes through
``csm.data.load_audio`` / ``Generator.save_wav`` because torchaudio is not installed."""
import argparse
import os
import time
import wave

import torch

from ..data import load_audio, resample
from ..generator import Segment, load_csm_1b
from ..sampling import FULL_LEVEL, LEVELS, NAMES, PARAMS, own_params

# reference cli/generate.py:16-25
VOICE_PRESETS = {"neutral": 0, "warm": 1, "deep": 2, "bright": 3, "soft": 4, "energetic": 5, "calm": 6, "clear": 7,
                 "resonant": 8, "authoritative": 9}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate speech with CSM (MI355X)")
    p.add_argument("--model-path", type=str, required=True, help="Path to the model checkpoint (the hub download is not available offline)")
    p.add_argument("--text", type=str, default=None, help="Text to generate speech for (required unless --serve-file is given)")
    voice = p.add_mutually_exclusive_group()
    voice.add_argument("--speaker", type=int, default=0, help="Speaker ID (default: 0)")
    voice.add_argument("--voice", type=str, choices=VOICE_PRESETS.keys(), help="Voice preset to use")
    p.add_argument("--output", type=str, default="audio.wav", help="Output file path (default: audio.wav)")
    p.add_argument("--context-audio", type=str, nargs="*", help="Path(s) to audio file(s) to use as context")
    p.add_argument("--context-text", type=str, nargs="*", help="Text(s) corresponding to the context audio files")
    p.add_argument("--context-speaker", type=int, nargs="*", help="Speaker ID(s) for the context segments")
    p.add_argument("--max-audio-length-ms", type=int, default=10000)
    p.add_argument("--temperature", type=float, default=0.9)
    p.add_argument("--topk", type=int, default=50)
    p.add_argument("--top-p", type=float, default=1.0,
                   help="nucleus cut in (0, 1], applied inside the sampler to what --topk kept: the largest values whose probability "
                        "reaches it stay (1.0: off)")
    p.add_argument("--min-p", type=float, default=0.0,
                   help="min-p cut in [0, 1], applied before --top-p: tokens below min-p times the largest probability go (0.0: off)")
    p.add_argument("--repetition-penalty", type=float, default=1.0, metavar="R",
                   help="repetition penalty in (0, 100], applied inside the sampler before the temperature: the logit x of every code "
                        "the utterance drew for the same codebook in its last --repetition-window frames becomes x / R (x > 0) or "
                        "x * R (1.0: off)")
    p.add_argument("--repetition-window", type=int, default=64, metavar="W",
                   help="frames the repetition penalty looks back, 0..64 (default 64; a turn's window covers that turn only)")
    p.add_argument("--typical-p", type=float, default=1.0, metavar="P",
                   help="locally typical sampling, in (0, 1] (default 1.0: off): after the other filters, keep the codes whose "
                        "surprise is closest to the entropy until their probability reaches P - it can drop the most likely code "
                        "(all modes)")
    p.add_argument("--stats-file", type=str, default=None, metavar="PATH",
                   help="write what the model thought of the codes it drew (return_stats / serve(stats=True)) as JSON lines: one "
                        "object per utterance or turn - with --serve-file one per line, under its \"line\" id - holding "
                        "\"codebook0\" (per frame: logprob, entropy and pmax of the semantic codebook), \"frame_logprob\" (per frame, "
                        "the sum of all K log-probabilities) and \"mean_logprob\" (all modes)")
    p.add_argument("--acoustic-temperature", type=float, default=None, metavar="T",
                   help="temperature of codebooks 1..K-1 (the acoustic ones; codebook 0 keeps --temperature)")
    p.add_argument("--acoustic-topk", type=int, default=None, metavar="K",
                   help="top-k of codebooks 1..K-1 (codebook 0 keeps --topk)")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--mimi-weights", type=str, required=True, help="local Mimi weights (transformers.MimiModel state dict)")
    p.add_argument("--text-tokenizer", type=str, required=True, help="local directory of the Llama-3.2 tokenizer files")
    p.add_argument("--stream", action="store_true", help="write the WAV chunk by chunk while the frames are generated")
    p.add_argument("--chunk-frames", type=int, default=4, help="80-ms frames per streamed chunk (default: 4)")
    p.add_argument("--lora-adapter", type=str, default=None,
                   help="LoRA adapter file written by csm-finetune-lora (.safetensors with its _metadata.json), applied without merging")
    p.add_argument("--decode-weights", type=str, choices=["bf16", "fp8"], default="bf16",
                   help="weights streamed by the decode steps: bf16 (default) or fp8 (weight-only e4m3, one scale per output row; "
                        "not with --lora-adapter or --serve-file lines that name an adapter, unless --fp8-adapters)")
    p.add_argument("--fp8-adapters", action="store_true",
                   help="with --decode-weights fp8: run --lora-adapter and the adapters of --serve-file lines un-merged on the FP8 "
                        "base (Model.fp8_adapters; the adapters were trained against the bf16 base - check the voices)")
    p.add_argument("--next-text", type=str, action="append", default=None,
                   help="a further line, spoken after --text in the same conversation with the KV cache kept (repeatable)")
    p.add_argument("--next-speaker", type=int, action="append", default=None,
                   help="speaker ID of the corresponding --next-text (repeatable; default: the speaker of --text)")
    p.add_argument("--on-overflow", type=str, choices=["error", "drop_oldest", "shift"], default="error",
                   help="--next-text / --serve-file conversations, when history + line + max audio reach the model's length: error "
                        "(default), drop_oldest (drop the oldest turns, prefill the rest again) or shift (drop them and slide the "
                        "KV cache: nothing is prefilled again)")
    p.add_argument("--keep-turns", type=int, default=0,
                   help="with --on-overflow drop_oldest / shift: leading turns (the voice prompt of --context-*) that are never "
                        "dropped (default 0)")
    p.add_argument("--serve-file", type=str, default=None,
                   help="JSON-lines file of utterances {\"text\", \"speaker\", \"adapter\"?: LoRA adapter file, \"seed\"?: int, "
                        "\"temperature\"?: float, \"topk\"?: int, \"top_p\"?: float, \"min_p\"?: float, \"repetition_penalty\"?: float, "
                        "\"repetition_window\"?: int, \"typical_p\"?: float, \"conversation\"?: id}: all are served as one running batch (Generator.serve) with the context of "
                        "--context-*; lines with the same conversation id are successive turns of one served conversation, in file "
                        "order (KV cache kept between them; adapter and seed of its first line); a line's temperature / topk hold for "
                        "that utterance or turn (default: --temperature / --topk; a file that names one is served with "
                        "row_sampling=True); likewise a line's top_p / min_p (default: --top-p / --min-p; a file that names one, or "
                        "a --top-p / --min-p that is not 1.0 / 0.0, is served with row_filters=True); a line's repetition_penalty / "
                        "repetition_window, and a list of one number per codebook for any of the four keys before them (a file or a "
                        "command line that uses any of these, --acoustic-* included, is served with row_processors=True); a line's "
                        "typical_p, a number or a list per codebook (a file that names one, or a --typical-p that is not 1.0, is "
                        "served with row_typical=True); one WAV "
                        "per utterance, <output stem>_<i>.wav with i = 0, 1, ... counting the file's non-empty lines")
    p.add_argument("--cache-context", action="store_true",
                   help="--serve-file: prefill the --context-* segments once as a voice (Generator.voice; one per distinct adapter "
                        "among --lora-adapter and the lines) and submit every line with its voice instead of the context - no "
                        "Mimi encode and no prefill of the context per line; conversations start from the voice")
    p.add_argument("--slots", type=int, default=16, help="--serve-file: utterances decoded at once (1..16, default 16)")
    p.add_argument("--streams", type=int, default=None, metavar="N",
                   help="--serve-file: keep up to N (--slots..256) utterances in flight over the --slots rows "
                        "(Generator.serve(streams=N)): each step gives the rows to the utterances with the least audio so far and "
                        "parks the others mid-utterance.  No pacing: the audio goes to files")
    p.add_argument("--hear-slots", type=int, default=0,
                   help="--serve-file: encoder slots of the server's batched hearing (Generator.serve(hear_slots=N), 0..16; "
                        "default 0: every conversation that hears has its own encode stream)")
    p.add_argument("--output-sample-rate", type=int, default=None, metavar="HZ",
                   help="sample rate of the WAV(s) written (default: the codec's 24000); another rate is resampled on the device, "
                        "chunk by chunk with --stream and on the server (all modes)")
    args = p.parse_args(argv)
    if args.output_sample_rate is not None and args.output_sample_rate < 1:
        p.error("--output-sample-rate must be >= 1")
    if args.text is None and args.serve_file is None:
        p.error("one of --text and --serve-file is required")
    if args.serve_file is not None and (args.text is not None or args.next_text or args.stream):
        p.error("--serve-file takes its lines from the file: not with --text, --next-text or --stream")
    if not 1 <= args.slots <= 16:
        p.error("--slots must be 1..16")
    if not 0 <= args.hear_slots <= 16:
        p.error("--hear-slots must be 0..16")
    if args.streams is not None and args.serve_file is None:
        p.error("--streams goes with --serve-file")
    if args.streams is not None and not args.slots <= args.streams <= 256:
        p.error("--streams must be --slots..256")
    if args.hear_slots and args.serve_file is None:
        p.error("--hear-slots goes with --serve-file")
    if args.cache_context and (args.serve_file is None or not args.context_audio):
        p.error("--cache-context goes with --serve-file and --context-audio / --context-text / --context-speaker")
    if args.keep_turns < 0:
        p.error("--keep-turns must be >= 0")
    if args.fp8_adapters and args.decode_weights != "fp8":
        p.error("--fp8-adapters goes with --decode-weights fp8")
    if args.next_speaker and len(args.next_speaker) != len(args.next_text or []):
        p.error("--next-speaker must be given once per --next-text (or not at all)")
    return args


def sampling_kw(args, codebooks):
    """The sampling keywords of the generate calls from the command line: --temperature / --topk / --top-p / --min-p, with
    --acoustic-temperature / --acoustic-topk expanded to one value per codebook (codebook 0 keeps the plain flag's), and
    --repetition-penalty / --repetition-window only where they are not 1.0 / 64 and --typical-p only where it is not 1.0 - without
    the new flags, the call it was.
    ``codebooks``: the model's K, or a callable that gives it (called only if an --acoustic-* flag needs it)."""
    kw = dict(temperature=args.temperature, topk=args.topk, top_p=args.top_p, min_p=args.min_p)
    if callable(codebooks) and (args.acoustic_temperature is not None or args.acoustic_topk is not None):
        codebooks = codebooks()
    if args.acoustic_temperature is not None:
        kw["temperature"] = [args.temperature] + [args.acoustic_temperature] * (codebooks - 1)
    if args.acoustic_topk is not None:
        kw["topk"] = [args.topk] + [args.acoustic_topk] * (codebooks - 1)
    if (args.repetition_penalty, args.repetition_window) != (1.0, 64):
        kw.update(repetition_penalty=args.repetition_penalty, repetition_window=args.repetition_window)
    if getattr(args, "typical_p", 1.0) != 1.0:
        kw["typical_p"] = args.typical_p
    return kw


def uses_processors(args):
    """Whether the command line names what only the processed sampler has."""
    return (args.acoustic_temperature is not None or args.acoustic_topk is not None
            or (args.repetition_penalty, args.repetition_window) != (1.0, 64))


def out_rate_kw(args):
    """The ``output_sample_rate`` keyword of the generate / serve calls: nothing without --output-sample-rate."""
    return {} if args.output_sample_rate is None else {"output_sample_rate": args.output_sample_rate}


def out_rate(generator, args) -> int:
    """The rate of what is written: --output-sample-rate, or the generator's."""
    return int(generator.sample_rate if args.output_sample_rate is None else args.output_sample_rate)


def stats_kw(args):
    """The ``return_stats`` keyword of the generate calls: nothing without --stats-file."""
    return {"return_stats": True} if getattr(args, "stats_file", None) else {}


def write_stats(args, objects):
    """--stats-file: one JSON object per line - ``SampleStats.summary()`` of each utterance, with the extra keys given."""
    import json
    os.makedirs(os.path.dirname(os.path.abspath(args.stats_file)), exist_ok=True)
    with open(args.stats_file, "w") as f:
        for extra, stats in objects:
            f.write(json.dumps({**extra, **stats.summary()}) + "\n")


def build_context(args, sample_rate):
    """Reference generate.py:129-156: (audio, text, speaker) triples -> Segments at the generator's sample rate."""
    context = []
    if args.context_audio:
        if not (args.context_text and args.context_speaker):
            raise ValueError("If context audio is provided, context text and speaker must also be provided")
        if not (len(args.context_audio) == len(args.context_text) == len(args.context_speaker)):
            raise ValueError("The number of context audio, text, and speaker entries must be the same")
        for path, text, speaker in zip(args.context_audio, args.context_text, args.context_speaker):
            wav, sr = load_audio(path)
            wav = resample(wav.mean(0) if wav.size(0) > 1 else wav.squeeze(0), sr, sample_rate)
            context.append(Segment(text=text, speaker=speaker, audio=wav))
    return context


def main(argv=None):
    args = parse_args(argv)
    speaker_id = VOICE_PRESETS[args.voice] if args.voice else args.speaker
    extra = {} if args.decode_weights == "bf16" else {"decode_weights": args.decode_weights}     # (the default needs no word)
    if args.fp8_adapters:
        extra["fp8_adapters"] = True
    generator = load_csm_1b(args.model_path, args.device, mimi_weights=args.mimi_weights, tokenizer_path=args.text_tokenizer, **extra)
    context = build_context(args, generator.sample_rate)
    adapter = None
    if args.lora_adapter:
        adapter = "cli"
        generator.load_adapter(adapter, args.lora_adapter)
    if args.serve_file:
        return serve_to_wavs(generator, args, context, adapter)
    if args.next_text:
        return converse_to_wav(generator, args, speaker_id, context, adapter)
    if args.stream:
        return stream_to_wav(generator, args, speaker_id, context, adapter)
    audio = generator.generate(text=args.text, speaker=speaker_id, context=context, max_audio_length_ms=args.max_audio_length_ms,
                               adapter=adapter, **sampling_kw(args, lambda: generator._model.args.audio_num_codebooks), **out_rate_kw(args),
                               **stats_kw(args))
    if args.stats_file:
        audio, stats = audio
        write_stats(args, [({}, stats)])
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    generator.save_wav(args.output, audio, **({} if args.output_sample_rate is None else {"sample_rate": args.output_sample_rate}))
    print(f"Audio saved to {args.output} ({audio.numel() / out_rate(generator, args):.2f} s at {out_rate(generator, args)} Hz)")
    return 0


def stream_to_wav(generator, args, speaker_id, context, adapter=None):
    """--stream: each chunk of ``generate_stream`` is appended to the WAV as it arrives (``wave`` patches the header's
    length on close); the samples are converted exactly as ``Generator.save_wav`` converts them, so the file is the same."""
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    t0 = time.perf_counter()
    n = 0
    stats = None
    with wave.open(args.output, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(out_rate(generator, args))
        for chunk in generator.generate_stream(text=args.text, speaker=speaker_id, context=context,
                                               max_audio_length_ms=args.max_audio_length_ms, chunk_frames=args.chunk_frames,
                                               adapter=adapter, **sampling_kw(args, lambda: generator._model.args.audio_num_codebooks),
                                               **out_rate_kw(args), **stats_kw(args)):
            if args.stats_file:
                chunk, part = chunk
                stats = part if stats is None else stats.extend(part)
            pcm = (chunk.detach().float().cpu().clamp(-1, 1) * 32767.0).to(torch.int16).numpy().tobytes()
            if n == 0:
                print(f"first chunk after {time.perf_counter() - t0:.3f} s")
            w.writeframes(pcm)
            n += chunk.numel()
    if args.stats_file:
        from ..sampling import SampleStats
        write_stats(args, [({}, stats if stats is not None else SampleStats(generator._model.args.audio_num_codebooks))])
    print(f"Audio saved to {args.output} ({n / out_rate(generator, args):.2f} s at {out_rate(generator, args)} Hz, streamed in "
          f"{time.perf_counter() - t0:.2f} s)")
    return 0


def read_serve_file(path, codebooks=None):
    """--serve-file: one JSON object per non-empty line -> [{"text", "speaker", "adapter", "seed"}], plus "conversation" (a
    string), "temperature" (a float), "topk" (an int), "top_p" and "min_p" (floats), "repetition_penalty" (a float) and
    "repetition_window" (an int) and "typical_p" (a float, or a list of K) on the lines that carry those keys.  With ``codebooks`` (the model's K, or a callable that gives
    it: called at the first list) the first four may also be a list of K numbers, one per codebook; a list of another length is
    refused here."""
    import json
    lines = []

    def per_codebook(i, key, value, integer):
        nonlocal codebooks
        kind = "integers" if integer else "numbers"
        if callable(codebooks):
            codebooks = codebooks()
        if codebooks is None or len(value) != codebooks or not all(
                not isinstance(v, bool) and isinstance(v, int if integer else (int, float)) for v in value):
            raise ValueError(f"{path}:{i}: \"{key}\" is a list of one value per codebook ({codebooks} {kind}), got {value!r}")
        return [v if integer else float(v) for v in value]
    with open(path) as f:
        for i, raw in enumerate(f, 1):
            if not raw.strip():
                continue
            d = json.loads(raw)
            if not isinstance(d, dict) or not isinstance(d.get("text"), str):
                raise ValueError(f"{path}:{i}: every line is a JSON object with a \"text\" string")
            unknown = set(d) - {"text", "speaker", "adapter", "seed", "conversation", "temperature", "topk", "top_p", "min_p",
                                "repetition_penalty", "repetition_window", "typical_p"}
            if unknown:
                raise ValueError(f"{path}:{i}: unknown keys {sorted(unknown)}")
            lines.append({"text": d["text"], "speaker": int(d.get("speaker", 0)), "adapter": d.get("adapter"),
                          "seed": None if d.get("seed") is None else int(d["seed"])})
            if d.get("conversation") is not None:
                lines[-1]["conversation"] = str(d["conversation"])
            for k in ("temperature", "topk", "top_p", "min_p", "typical_p"):
                if isinstance(d.get(k), list):
                    lines[-1][k] = per_codebook(i, k, d.pop(k), k == "topk")
            if d.get("repetition_penalty") is not None:
                if isinstance(d["repetition_penalty"], bool) or not isinstance(d["repetition_penalty"], (int, float)):
                    raise ValueError(f"{path}:{i}: \"repetition_penalty\" is a number, got {d['repetition_penalty']!r}")
                lines[-1]["repetition_penalty"] = float(d["repetition_penalty"])
            if d.get("repetition_window") is not None:
                if isinstance(d["repetition_window"], bool) or not isinstance(d["repetition_window"], int):
                    raise ValueError(f"{path}:{i}: \"repetition_window\" is an integer, got {d['repetition_window']!r}")
                lines[-1]["repetition_window"] = d["repetition_window"]
            if d.get("temperature") is not None:
                if isinstance(d["temperature"], bool) or not isinstance(d["temperature"], (int, float)):
                    raise ValueError(f"{path}:{i}: \"temperature\" is a number, got {d['temperature']!r}")
                lines[-1]["temperature"] = float(d["temperature"])
            if d.get("topk") is not None:
                if isinstance(d["topk"], bool) or not isinstance(d["topk"], int):
                    raise ValueError(f"{path}:{i}: \"topk\" is an integer, got {d['topk']!r}")
                lines[-1]["topk"] = d["topk"]
            for k in ("top_p", "min_p", "typical_p"):
                if d.get(k) is not None:
                    if isinstance(d[k], bool) or not isinstance(d[k], (int, float)):
                        raise ValueError(f"{path}:{i}: \"{k}\" is a number, got {d[k]!r}")
                    lines[-1][k] = float(d[k])
    if not lines:
        raise ValueError(f"{path}: no utterances")
    return lines


def _line(level, line):
    """The keywords of one --serve-file line for ``submit`` / ``say`` that belong to ``level`` (``sampling.LEVELS``: the
    parameters it is the first to read): only what the line carries."""
    return {NAMES[j]: line[NAMES[j]] for j in own_params(level) if NAMES[j] in line}


def _serve(level, lines, asked=False, defaults=None):
    """``Generator.serve`` keywords for these lines and the command line: the flag of ``level`` (with ``row_sampling=True``, which
    it needs, and what ``defaults()`` gives - the command line's values - as the server's) as soon as a line names one of the
    level's keys - or, whole rows, a list per codebook under a lower key - or the command line does (``asked``); else nothing."""
    lower = NAMES[:own_params(level).start] if level == FULL_LEVEL else ()
    if not asked and not any(_line(level, ln) or any(isinstance(ln.get(k), list) for k in lower) for ln in lines):
        return {}
    return {"row_sampling": True, LEVELS[level].flag: True, **(defaults() if defaults else {})}


def _serve_args(level, lines, args, codebooks):
    """``_serve`` with the command line ``args`` (None: the lines alone): it asks for ``level`` with one of the level's own flags
    off its identity or - whole rows - what ``uses_processors`` looks for, and ``sampling_kw`` gives the server's defaults.  (The
    level of the pair takes nothing from the command line: --temperature / --topk are the server's at any level.)"""
    if args is None or level == 1:
        return _serve(level, lines)
    asked = (any(getattr(args, NAMES[j], PARAMS[j].identity) != PARAMS[j].identity for j in own_params(level))
             or level == FULL_LEVEL and uses_processors(args))
    return _serve(level, lines, asked, lambda: sampling_kw(args, codebooks))


def line_sampling(line):
    """The sampling keywords of one --serve-file line for ``submit`` / ``say``: only what the line carries."""
    return _line(1, line)


def serve_sampling(lines):
    """``Generator.serve`` keywords for these lines: ``row_sampling=True`` as soon as one of them carries a parameter."""
    return _serve(1, lines)


def line_filters(line):
    """The filter keywords of one --serve-file line for ``submit`` / ``say``: only what the line carries."""
    return _line(2, line)


def serve_filters(lines, top_p=1.0, min_p=0.0):
    """``Generator.serve`` keywords for these lines and the command line's --top-p / --min-p: ``row_filters=True`` (with
    ``row_sampling=True``, which it needs, and the two as the server's defaults) as soon as a line names a filter or the
    command line's are not 1.0 / 0.0; nothing otherwise - the server is then the one it is without filters."""
    return _serve(2, lines, (top_p, min_p) != (1.0, 0.0), lambda: {"top_p": top_p, "min_p": min_p})


def line_processors(line):
    """The repetition keywords of one --serve-file line for ``submit`` / ``say``: only what the line carries."""
    return _line(3, line)


def serve_processors(lines, args=None, codebooks=None):
    """``Generator.serve`` keywords for these lines and the command line: ``row_processors=True`` (with ``row_sampling=True``, which it
    needs, and the command line's values - --acoustic-* expanded - as the server's defaults) as soon as a line names a repetition
    penalty, a window or a list per codebook, or the command line uses --repetition-* / --acoustic-*; nothing otherwise."""
    return _serve_args(3, lines, args, codebooks)


def line_typical(line):
    """The typical-sampling keyword of one --serve-file line for ``submit`` / ``say``: only if the line carries it."""
    return _line(4, line)


def serve_typical(lines, args=None, codebooks=None):
    """``Generator.serve`` keywords for these lines and the command line: ``row_typical=True`` (with ``row_sampling=True``, which it
    needs, and the command line's values as the server's defaults) as soon as a line names "typical_p" or --typical-p is not
    1.0; nothing otherwise."""
    return _serve_args(4, lines, args, codebooks)


def line_kw(line):
    """Every sampling keyword of one --serve-file line for ``submit`` / ``say``, whatever its level."""
    return {k: v for n in range(1, len(LEVELS)) for k, v in _line(n, line).items()}


def serve_lines(lines, args, codebooks):
    """The sampling keywords of ``Generator.serve`` for these lines and the command line: --temperature / --topk, and what
    every level adds (``_serve_args``), lowest level first."""
    kw = {"temperature": args.temperature, "topk": args.topk}
    for n in range(1, len(LEVELS)):
        kw.update(_serve_args(n, lines, args, codebooks))
    return kw


def serve_voices(generator, lines, context, adapter=None):
    """--cache-context: the --context-* segments as one ``Generator.voice`` per distinct adapter among the lines (--lora-adapter
    for lines without one): {adapter name or None: Voice}.  Call it after the lines' adapters are loaded and before ``serve``."""
    return {name: generator.voice(context, adapter=name)
            for name in sorted({ln["adapter"] or adapter for ln in lines}, key=lambda n: (n is not None, n or ""))}


def line_prompt(line, context, voices, adapter=None):
    """The prompt keywords of one --serve-file line for ``submit`` / ``conversation``: the context - or, with --cache-context
    (``voices``: ``serve_voices``), no context and the voice of the line's adapter."""
    if voices is None:
        return {"context": context}
    return {"context": [], "voice": voices[line["adapter"] or adapter]}


def serve_to_wavs(generator, args, context, adapter=None):
    """--serve-file: every line is a request of one ``Generator.serve`` batch; adapter files are loaded once each, under their
    path as name (--lora-adapter is the default for lines without one).  Lines with a "conversation" id are the turns of one
    served conversation (``BatchServer.conversation``): its first line is queued with the rest, each later one when the turn
    before it is done.  A line's "temperature" / "topk" are that utterance's or that turn's; if any line has one, the server is
    made with ``row_sampling=True`` (--temperature / --topk are then the other lines' values); "top_p" / "min_p" likewise, with
    ``row_filters=True`` (``serve_filters``); "repetition_penalty" / "repetition_window", a list per codebook or the command
    line's --repetition-* / --acoustic-* make it ``row_processors=True`` (``serve_processors``); "typical_p" or --typical-p make it
    ``row_typical=True`` (``serve_typical``).  Utterance i (the i-th non-empty line, from 0) goes to <output stem>_<i>.wav.
    With --cache-context the context becomes one voice per adapter (``serve_voices``) and every line and every conversation
    starts from its voice instead of the context (``line_prompt``)."""
    def K():
        return generator._model.args.audio_num_codebooks
    lines = read_serve_file(args.serve_file, K)
    for path in sorted({ln["adapter"] for ln in lines if ln["adapter"]}):
        generator.load_adapter(path, path)
    stem, ext = os.path.splitext(os.path.abspath(args.output))
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    t0 = time.perf_counter()
    voices = serve_voices(generator, lines, context, adapter) if args.cache_context else None     # (the adapters are loaded)
    server = generator.serve(slots=args.slots, chunk_frames=args.chunk_frames, hear_slots=args.hear_slots,
                             **serve_lines(lines, args, K), **out_rate_kw(args), **({"streams": args.streams} if args.streams else {}),
                             **({"stats": True} if args.stats_file else {}))
    line_stats = {}
    convs, line_of = {}, {}                           # conversation id -> [conversation, its lines still to say]; request -> line

    def say(cid):
        conv, todo = convs[cid]
        i = todo.pop(0)
        line_of[conv.say(lines[i]["text"], lines[i]["speaker"], max_audio_length_ms=args.max_audio_length_ms,
                         **line_kw(lines[i]))] = (i, cid)

    for i, ln in enumerate(lines):
        cid = ln.get("conversation")
        if cid is None:
            line_of[server.submit(ln["text"], ln["speaker"], adapter=ln["adapter"] or adapter, seed=ln["seed"],
                                  max_audio_length_ms=args.max_audio_length_ms, **line_prompt(ln, context, voices, adapter),
                                  **line_kw(ln))] = (i, None)
        elif cid in convs:
            convs[cid][1].append(i)
        else:
            convs[cid] = [server.conversation(adapter=ln["adapter"] or adapter, seed=ln["seed"], on_overflow=args.on_overflow,
                                              keep_turns=args.keep_turns, **line_prompt(ln, context, voices, adapter)), [i]]
            say(cid)
    while server.queued or server.active or (args.streams and server.in_flight):     # (--streams: parked requests hold no slot)
        for req, _, done in server.step():
            if done:
                i, cid = line_of[req]
                out = f"{stem}_{i}{ext or '.wav'}"
                generator.save_wav(out, req.audio(), **({} if args.output_sample_rate is None else {"sample_rate": req.sample_rate}))
                print(f"line {i}: {req.audio().numel() / out_rate(generator, args):.2f} s -> {out} (after {time.perf_counter() - t0:.2f} s)")
                line_stats[i] = req.stats
                if cid is not None and convs[cid][1]:
                    say(cid)
    if args.stats_file:
        write_stats(args, [({"line": i}, line_stats[i]) for i in sorted(line_stats)])
    print(f"{len(lines)} utterances served in {time.perf_counter() - t0:.2f} s")
    return 0


def _pcm(audio):
    return (audio.detach().float().cpu().clamp(-1, 1) * 32767.0).to(torch.int16).numpy().tobytes()


def converse_to_wav(generator, args, speaker_id, context, adapter=None):
    """--next-text: --text and every further line are the turns of one ``Generator.conversation`` (the KV cache is kept between
    them); all turns go to --output in order, chunk by chunk with --stream.  Samples are converted as ``Generator.save_wav``
    converts them."""
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    lines = [(args.text, speaker_id)] + list(zip(args.next_text, args.next_speaker or [speaker_id] * len(args.next_text)))
    conv = generator.conversation(context=context, adapter=adapter, on_overflow=args.on_overflow, keep_turns=args.keep_turns)
    kw = dict(max_audio_length_ms=args.max_audio_length_ms, **sampling_kw(args, lambda: generator._model.args.audio_num_codebooks),
              **out_rate_kw(args), **stats_kw(args))
    t0 = time.perf_counter()
    n = 0
    turn_stats = []
    with wave.open(args.output, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(out_rate(generator, args))
        for i, (text, spk) in enumerate(lines):
            t1 = time.perf_counter()
            if args.stream:
                first = None
                for chunk in conv.generate_stream(text, spk, chunk_frames=args.chunk_frames, **kw):
                    if args.stats_file:
                        chunk, part = chunk
                        if len(turn_stats) <= i:
                            turn_stats.append(part)
                        else:
                            turn_stats[i].extend(part)
                    pcm = _pcm(chunk)
                    first = first if first is not None else time.perf_counter() - t1
                    w.writeframes(pcm)
                    n += chunk.numel()
                print(f"turn {i + 1}: first chunk after {first if first is not None else float('nan'):.3f} s")
            else:
                audio = conv.generate(text, spk, **kw)
                if args.stats_file:
                    audio, part = audio
                    turn_stats.append(part)
                w.writeframes(_pcm(audio))
                n += audio.numel()
                print(f"turn {i + 1}: {audio.numel() / out_rate(generator, args):.2f} s of audio in {time.perf_counter() - t1:.2f} s")
    if args.stats_file:
        write_stats(args, [({"turn": i}, st) for i, st in enumerate(turn_stats)])
    print(f"Audio saved to {args.output} ({n / out_rate(generator, args):.2f} s at {out_rate(generator, args)} Hz, {len(lines)} turns in "
          f"{time.perf_counter() - t0:.2f} s)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
