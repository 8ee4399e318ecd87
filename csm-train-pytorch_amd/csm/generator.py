"""Generation API of reference ``src/csm/generator.py`` (``Segment``, ``Generator``, ``load_csm_1b``) on MI355X.

The autoregressive core (``Model.generate_frame`` driven by ``Generator.generate``, generator.py:147-218) and the frame
tokenisation (generator.py:77-145) are implemented here.  Two inputs of the reference cannot exist in this build
environment (no network): the Llama-3 text tokenizer (``AutoTokenizer.from_pretrained``, generator.py:35-36) and the
Mimi codec weights (``hf_hub_download``, generator.py:67).  Both are therefore *injected*: ``Generator(model,
text_tokenizer=..., audio_tokenizer=...)``; when omitted the reference's own loading calls are attempted and their
failure is reported as-is.  The audio tokenizer protocol is Mimi's: ``encode([1,1,N]) -> [1,K,T]`` int64,
``decode([1,K,T]) -> [1,1,N]``, ``sample_rate``.  Watermarking (silentcipher) is post-processing outside the hot path
and is not applied here (out of scope).
"""
from dataclasses import dataclass
from typing import Iterator, List, Optional, Tuple

import torch

from .models.model import Model, ModelArgs
from .sampling import (FULL_LEVEL, LEVELS, NAMES, PARAMS, SampleStats, _as_list, _is_number, check_filters, names_processors,
                       normalise, per_codebook)


@dataclass
class Segment:
    """A segment of speech (reference generator.py:18-25)."""

    speaker: int
    text: str
    audio: torch.Tensor  # (num_samples,), sample_rate = 24_000


def load_llama3_tokenizer(path: str = "meta-llama/Llama-3.2-1B"):
    """Reference generator.py:28-45 (needs the Hugging Face hub, a local cache of meta-llama/Llama-3.2-1B, or ``path`` =
    a local directory holding that tokenizer's files)."""
    import os
    from tokenizers.processors import TemplateProcessing
    from transformers import AutoTokenizer

    tokenizer = AutoTokenizer.from_pretrained(path, local_files_only=os.path.isdir(path))
    bos, eos = tokenizer.bos_token, tokenizer.eos_token
    tokenizer._tokenizer.post_processor = TemplateProcessing(
        single=f"{bos}:0 $A:0 {eos}:0", pair=f"{bos}:0 $A:0 {eos}:0 {bos}:1 $B:1 {eos}:1",
        special_tokens=[(f"{bos}", tokenizer.bos_token_id), (f"{eos}", tokenizer.eos_token_id)])
    return tokenizer


def _untouched(v):
    """A value as the frame calls take it: a number as it is, a sequence as a list."""
    return v if _is_number(v) else _as_list(v)


def filter_kwargs(top_p, min_p, B=None):
    """The ``top_p`` / ``min_p`` keywords of a frame call: {} at the defaults (1.0 / 0.0 - the call is then today's, untouched),
    else both, held to ``check_filters`` here (before any cache is taken over).  ``B``: either one may be a sequence of B values."""
    if _is_number(top_p) and _is_number(min_p):
        top_p, min_p = check_filters(top_p, min_p)
        return {} if (top_p, min_p) == (1.0, 0.0) else {"top_p": top_p, "min_p": min_p}
    if B is None:
        raise ValueError(f"top_p and min_p are numbers, got top_p={top_p!r}, min_p={min_p!r}")
    normalise(B, 1, 1, None, None, top_p, min_p, unit="utterance")
    return {"top_p": _untouched(top_p), "min_p": _untouched(min_p)}


def sampling_kwargs(gen, temperature, topk, top_p, min_p, repetition_penalty=1.0, repetition_window=64, B=None, typical_p=1.0):
    """(temperature, topk, keywords) of the frame calls of a generation on the Generator ``gen``.  Nothing new named -
    ``repetition_penalty`` 1.0, ``repetition_window`` 64 and no per-codebook sequence: what the call has always made of them (``filter_kwargs``;
    ``Generator._batch_sampling`` with ``B``), untouched.  Otherwise every one of the six goes to the rows' processors
    (``DecodeState.sampling_args``): one entry per row, each a number or K numbers (one per codebook), checked here
    (``sampling.normalise``, the check the state makes), before any cache is taken over.  Without ``B`` (one utterance) a value is
    a number or K numbers - the one entry of a batch of one; with ``B`` a number or a sequence of B entries, each a number or K
    numbers - a flat sequence of B numbers keeps its meaning, one value per utterance.  ``typical_p`` other than the number 1.0
    (a number, K numbers, or with ``B`` an entry per utterance) sends all seven to the rows (the typical rows sampler)."""
    given = [temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p]
    if B is None:
        given = [v if _is_number(v) else [per_codebook(name, v, gen._model.args.audio_num_codebooks)]
                 for name, v in zip(NAMES, given)]
    named = [not (_is_number(v) and v == p.identity) for p, v in zip(PARAMS, given)]      # (off its identity)
    below = LEVELS[FULL_LEVEL - 1].reads                 # the pair and the filters: what the levels below whole rows read
    if not names_processors(*given[:below]) and not any(named[below:]):
        if B is not None:
            temperature, topk = gen._batch_sampling(temperature, topk, B)
        return temperature, topk, filter_kwargs(top_p, min_p, B)
    # to the rows: all that the first level of whole rows reads, and of the levels above it up to the last parameter named
    a, n = gen._model.args, 1 if B is None else B
    sent = max(j + 1 for j in range(len(PARAMS)) if j < LEVELS[FULL_LEVEL].reads or named[j])
    normalise(n, a.audio_num_codebooks, a.audio_vocab_size, unit="utterance", **dict(zip(NAMES[:sent], given[:sent])))
    rows = [[v] * n if _is_number(v) else _as_list(v) for v in given[:sent]]
    return rows[0], rows[1], dict(zip(NAMES[2:sent], rows[2:]))


class Generator:
    """Speech generator using the CSM model (reference generator.py:48)."""

    def __init__(self, model: Model, text_tokenizer=None, audio_tokenizer=None):
        self._model = model
        self._model.setup_caches(1)
        self._text_tokenizer = text_tokenizer if text_tokenizer is not None else load_llama3_tokenizer()
        if audio_tokenizer is None:
            raise RuntimeError("Generator needs an audio tokenizer with Mimi's encode/decode protocol: the reference fetches "
                               "Mimi weights from the hub (generator.py:67), which this environment cannot do")
        self._audio_tokenizer = audio_tokenizer
        self.sample_rate = audio_tokenizer.sample_rate
        self.device = model.device
        self._run = 0                  # bumped by every generate*: an open generate_stream stops when it changes
        self._bank = None              # LoRA adapters chosen per utterance (add_adapter / load_adapter)

    # ---- per-utterance LoRA adapters (csm/lora_bank.py) -----------------------------------------------------------------
    def _lora_bank(self):
        if self._bank is None:
            from .lora_bank import LoRABank
            self._bank = LoRABank(self._model)
        return self._bank

    def add_adapter(self, name: str, state):
        """Register a ``LoRAState`` of this model (e.g. ``CSMLoRATrainer``'s live ``model.lora``) under ``name``; generation
        reads it in place.  Every adapter of the bank must share target modules, target layers, bias use and padded rank."""
        return self._lora_bank().add(name, state)

    def load_adapter(self, name: str, path: str):
        """Load an adapter file written by ``csm-finetune-lora`` / ``CSMLoRATrainer.save_model(save_mode="lora")`` under
        ``name`` (no merge: the base weights are shared by every adapter)."""
        return self._lora_bank().load(name, path)

    @property
    def adapters(self) -> List[str]:
        """Names of the loaded adapters."""
        return [] if self._bank is None else self._bank.names

    def _resolve_adapters(self, names):
        if all(n is None for n in names):
            return None
        if self._bank is None:
            raise ValueError(f"unknown LoRA adapter {next(n for n in names if n is not None)!r} (none loaded)")
        return self._bank.resolve(names)

    def _out_resampler(self, output_sample_rate):
        """``output_sample_rate=`` of the generate / serve calls: None for None or the codec's own rate (the call is then today's,
        untouched), else the device ``Resampler`` from the codec's rate to it.  A bad rate raises here, before anything runs."""
        from .codec.resample import rate_resampler
        return rate_resampler("output_sample_rate", output_sample_rate, self.sample_rate, self.device, to_native=False)

    def _tokenize_text_segment(self, text: str, speaker: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference generator.py:77-100: ``f"[{speaker}]{text}"`` ids into the last column."""
        K1 = self._model.args.audio_num_codebooks + 1
        ids = self._text_tokenizer.encode(f"[{speaker}]{text}")
        frame = torch.zeros(len(ids), K1).long()
        mask = torch.zeros(len(ids), K1).bool()
        frame[:, -1] = torch.tensor(ids)
        mask[:, -1] = True
        return frame.to(self.device), mask.to(self.device)

    def _tokenize_audio(self, audio: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference generator.py:102-130: Mimi codes [K,T] + one all-zero EOS frame into the first K columns."""
        audio = audio.to(self.device)
        return self._audio_frames(self._audio_tokenizer.encode(audio.unsqueeze(0).unsqueeze(0))[0])

    def _audio_frames(self, codes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Mimi codes [K,T] -> their T frames + one all-zero EOS frame (``_tokenize_audio``; ``HeardTurn.end`` for streamed codes)."""
        K1 = self._model.args.audio_num_codebooks + 1
        eos = torch.zeros(codes.size(0), 1, dtype=codes.dtype, device=codes.device)
        codes = torch.cat([codes, eos], dim=1)
        frame = torch.zeros(codes.size(1), K1).long().to(self.device)
        mask = torch.zeros(codes.size(1), K1).bool().to(self.device)
        frame[:, :-1] = codes.transpose(0, 1)
        mask[:, :-1] = True
        return frame, mask

    def _tokenize_segment(self, segment: Segment) -> Tuple[torch.Tensor, torch.Tensor]:
        tt, tm = self._tokenize_text_segment(segment.text, segment.speaker)
        at, am = self._tokenize_audio(segment.audio)
        return torch.cat([tt, at], dim=0), torch.cat([tm, am], dim=0)

    @torch.inference_mode()
    def generate(self, text: str, speaker: int, context: List[Segment], max_audio_length_ms: float = 90_000,
                 temperature: float = 0.9, topk: int = 50, eos_check_every: int = 8, adapter: Optional[str] = None,
                 top_p: float = 1.0, min_p: float = 0.0, output_sample_rate: Optional[int] = None,
                 repetition_penalty=1.0, repetition_window=64, voice=None, typical_p=1.0, return_stats: bool = False):
        """Reference generator.py:147-218.  ``adapter``: the name of a bank adapter (``add_adapter`` / ``load_adapter``) to
        speak with, or None.  The reference tests every frame for EOS on the host (one device sync per
        frame, generator.py:196-199); here the all-zero test runs on the device and the host looks at it once per
        ``eos_check_every`` frames, so the frame graphs are enqueued back to back.  The audio returned is the same: frames
        sampled past the EOS frame are dropped.
        ``top_p`` (in (0, 1]) / ``min_p`` (in [0, 1]): a nucleus and a min-p cut applied inside the sampler to what top-k kept -
        first p_i >= min_p * p_max, then the smallest set of the largest values whose probability reaches top_p.  At 1.0 / 0.0
        (the defaults) the call is what it is without them; otherwise it samples through the filtered rows sampler.
        ``output_sample_rate``: the rate of the audio returned (None: the codec's 24 kHz); another rate is resampled on the
        device (``csm.codec.resample``) - the codes are the same.
        ``repetition_penalty`` r (0 < r <= 100) / ``repetition_window`` (0..64 frames): inside the sampler, the logit x of every
        code the utterance drew for this codebook in its last ``repetition_window`` frames becomes x / r (x > 0) or x * r before
        the temperature.  ``temperature`` / ``topk`` / ``top_p`` / ``min_p`` and these two may each be a sequence of K numbers, one
        per codebook (codebook 0 is the semantic one).  At 1.0 / 64 with plain numbers the call is what it is without them;
        otherwise it samples through the processed rows sampler (``DecodeState.set_row_processors``).
        ``typical_p`` (in (0, 1], a number or K numbers): locally typical sampling (Meister et al. 2022) as the last filter - of
        what the others left, the tokens whose surprise -ln p is closest to the entropy stay, most typical first, until their
        probability reaches ``typical_p``; unlike top-p and min-p it can drop the most likely code.  At 1.0 the call is what it is
        without it; otherwise it samples through the typical rows sampler (``DecodeState.set_row_typical``).
        ``voice``: a ``Voice`` (``Generator.voice``) that comes before ``context`` - the call is then
        ``conversation(voice=voice, context=context, adapter=adapter).generate(text, speaker, ...)`` with every other argument
        passed through: the voice's K / V are copied in, only ``context`` and the text are fed.
        ``return_stats``: return (audio, ``SampleStats``) - per frame and codebook, the model's own log-probability of the
        code drawn, and the entropy and largest probability of the distribution it was drawn from (temperature 1, before
        any filter or penalty), cut where the codes are cut.  The codes and the audio are the same; the frames cost one more
        launch each.  Refused on the recompute path (``model.use_kv_cache = False``)."""
        from .conversation import _Turn, drive, prepare_call, spoken
        call = prepare_call(self, max_audio_length_ms, temperature, topk, top_p, min_p, repetition_penalty, repetition_window,
                            typical_p, output_sample_rate, return_stats, eos_check_every=eos_check_every, stateless=voice is None)
        if voice is not None:
            return self.conversation(context, adapter, voice=voice)._speak(text, speaker, call)
        ads = self._resolve_adapters([adapter])
        self._run += 1
        self._model.reset_caches()
        turn = _Turn()
        for _ in drive(turn, self._step(call, ads, *self._prompt_frames(text, speaker, context, call.max_audio_frames)), call):
            pass
        return spoken(self, turn, call)

    def _stats_check(self, return_stats):
        """``return_stats`` is refused where the frames cannot give it, before any cache is taken over."""
        if return_stats and not getattr(self._model, "use_kv_cache", True):
            raise ValueError("the recompute path (use_kv_cache = False) has no return_stats: the statistics need the KV-cache path")

    def _prompt_frames(self, text: str, speaker: int, context: List[Segment], max_audio_frames: int, held: int = 0):
        """Prompt frames of an utterance - the context segments, then the text: (tokens [S,K+1], mask [S,K+1]), held to the
        reference's length rule.  ``held``: positions that come before them (a voice's) and count towards it."""
        parts = [self._tokenize_segment(seg) for seg in context] + [self._tokenize_text_segment(text, speaker)]
        tokens = torch.cat([t for t, _ in parts], dim=0).long().to(self.device)
        mask = torch.cat([m for _, m in parts], dim=0).bool().to(self.device)
        max_seq_len = self._model.bb.max_seq_len - max_audio_frames
        if held + tokens.size(0) >= max_seq_len:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_audio_frames: {max_seq_len}")
        return tokens, mask

    def _step(self, call, ads, tokens, mask):
        """``step`` of ``conversation.drive`` for a stateless call: the prompt frames first, then each sampled frame fed back."""
        K = self._model.args.audio_num_codebooks
        audio_mask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], dim=1).unsqueeze(1).to(self.device)
        pad = torch.zeros(1, 1, dtype=torch.long, device=self.device)
        pos = torch.arange(0, tokens.size(0)).unsqueeze(0).long().to(self.device)
        tokens, mask = tokens.unsqueeze(0), mask.unsqueeze(0)

        def step(turn):
            nonlocal tokens, mask, pos
            if turn.samples:
                tokens, mask, pos = torch.cat([turn.samples[-1].long(), pad], dim=1).unsqueeze(1), audio_mask, pos[:, -1:] + 1
            turn.samples.append(self._model.generate_frame(tokens, mask, pos, call.temperature, call.topk, adapters=ads,
                                                           **call.filters))
            if call.return_stats:
                turn.stats.append(self._model._decode_state.frame_stats())        # (a device copy: the host reads it at a look)
        return step

    def generate_stream(self, text: str, speaker: int, context: List[Segment], max_audio_length_ms: float = 90_000,
                        temperature: float = 0.9, topk: int = 50, chunk_frames: int = 4,
                        adapter: Optional[str] = None, top_p: float = 1.0, min_p: float = 0.0,
                        output_sample_rate: Optional[int] = None, repetition_penalty=1.0,
                        repetition_window=64, voice=None, typical_p=1.0, return_stats: bool = False) -> Iterator[torch.Tensor]:
        """``generate`` that hands the audio out while it is being made: an iterator of 1-D device tensors of
        ``chunk_frames * 1920`` samples (the last one may be shorter), decoded by the audio tokenizer's stateful
        ``decode_stream()``.  The frames are sampled by the same ``generate_frame`` calls in the same order as ``generate``,
        so under the same torch seed the concatenated chunks equal ``generate``'s audio.  The host looks for EOS once per
        chunk; frames from EOS on are never decoded.  A later ``generate`` / ``generate_batch`` / ``generate_stream`` on this
        Generator invalidates the stream (its next ``next()`` raises ``RuntimeError``); abandoning it is harmless.
        ``adapter``, ``top_p``, ``min_p``, ``repetition_penalty``, ``repetition_window``, ``typical_p`` and per-codebook sequences: as
        for ``generate``.  ``output_sample_rate``: the chunks go through a stateful
        ``ResampleStream`` - they concatenate to ``generate(..., output_sample_rate=)``'s audio bit for bit; the stream lags by
        the filter's half-width, and what it still owes comes as one last short chunk.
        ``voice``: as for ``generate`` - the call is ``conversation(voice=voice, context=context,
        adapter=adapter).generate_stream(text, speaker, ...)``.
        ``return_stats``: the iterator yields (chunk, ``SampleStats`` of the chunk's frames) - read with the chunk's one host
        look; the resampler's last short chunk comes with no frames."""
        from .conversation import prepare_call
        call = prepare_call(self, max_audio_length_ms, temperature, topk, top_p, min_p, repetition_penalty, repetition_window,
                            typical_p, output_sample_rate, return_stats, chunk_frames=chunk_frames, stateless=voice is None)
        if voice is not None:
            return self.conversation(context, adapter, voice=voice)._speak_stream(text, speaker, call)
        ads = self._resolve_adapters([adapter])
        self._run += 1
        return self._stream(self._run, text, speaker, context, call, ads)

    @torch.inference_mode()
    def _stream(self, run, text, speaker, context, call, ads):
        from .conversation import _Turn, stream_spoken

        def check():
            if self._run != run:
                raise RuntimeError("this stream was invalidated: a later generate / generate_batch / generate_stream call on "
                                   "the same Generator took over the model's caches")

        check()
        self._model.reset_caches()
        step = self._step(call, ads, *self._prompt_frames(text, speaker, context, call.max_audio_frames))
        yield from stream_spoken(self, _Turn(), step, call, check)

    @torch.inference_mode()
    def generate_batch(self, texts: List[str], speakers: List[int], contexts: List[List[Segment]],
                       max_audio_length_ms: float = 90_000, temperature: float = 0.9, topk: int = 50,
                       eos_check_every: int = 8, adapters: Optional[List[Optional[str]]] = None, top_p=1.0,
                       min_p=0.0, output_sample_rate: Optional[int] = None, repetition_penalty=1.0,
                       repetition_window=64, typical_p=1.0, return_stats: bool = False) -> List[torch.Tensor]:
        """``generate`` for up to 16 utterances at once (not in the reference, whose loop is single-utterance): the prompts
        (different lengths) are prefilled one by one into their rows of the KV caches, then every decode frame advances all
        rows together - the decode kernels share each weight load between the batch rows, so B utterances cost about as
        much as one.  A row stops contributing at its own EOS frame; the loop ends when every row has one.  Up to 4 rows
        each row's codes are those of a one-utterance run; 5..16 rows go through the MFMA decode products, whose rows are
        the same bits for any batch size in 5..16 (not those of 1..4).  Live (un-merged) LoRA adapters: at most 4.
        ``adapters``: one bank adapter name or None per utterance (``add_adapter`` / ``load_adapter``), 1..16 rows; with it, a
        live ``model.lora`` must be absent or merged.
        ``temperature`` / ``topk``: a number for all utterances, or a sequence of one value per utterance for either one -
        each row then samples with its own pair (the rows sampler, ``DecodeState.set_row_sampling``) and has the codes it
        has in a batch of the same size run with its pair for everybody; two numbers are the one-pair path.
        ``top_p`` / ``min_p``: a number or one value per utterance for either one (``generate``); at 1.0 / 0.0 the call is what it
        is without them, otherwise every row samples through the filtered rows sampler with its own four parameters.
        ``repetition_penalty`` / ``repetition_window`` (``generate``): a number or one value per utterance; with them, or with an
        entry per utterance that is a sequence of K numbers (one per codebook) in any of the six, every row samples through the
        processed rows sampler with its own parameters.  A flat sequence of B numbers is one value per utterance, as before.
        ``output_sample_rate``: as for ``generate``, for every utterance.
        ``return_stats``: return (the audio list, one ``SampleStats`` per utterance), as for ``generate``."""
        out_rs = self._out_resampler(output_sample_rate)
        self._stats_check(return_stats)
        B = len(texts)
        if not (1 <= B <= 16 and len(speakers) == B and len(contexts) == B):
            raise ValueError("generate_batch takes 1..16 utterances with one speaker id and one context list each")
        temperature, topk, filters = sampling_kwargs(self, temperature, topk, top_p, min_p, repetition_penalty,
                                                     repetition_window, B, typical_p=typical_p)
        if adapters is not None and len(adapters) != B:
            raise ValueError(f"generate_batch: {len(adapters)} adapter names for {B} utterances (one name or None each)")
        ads = self._resolve_adapters(list(adapters)) if adapters is not None else None
        self._run += 1
        self._model.reset_caches()
        max_audio_frames = int(max_audio_length_ms / 80)
        K = self._model.args.audio_num_codebooks
        prompts = [self._prompt_frames(text, spk, ctx, max_audio_frames) for text, spk, ctx in zip(texts, speakers, contexts)]
        toks, msks = [t for t, _ in prompts], [m for _, m in prompts]
        if return_stats:
            filters = dict(filters, stats=True)
        frames = [self._model.engine.generate_first_frames(toks, msks, temperature, topk, adapters=ads, **filters)]          # [B, K] each
        fstats = [self._model._decode_state.frame_stats()] if return_stats else []
        mask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1).to(self.device)
        pad = torch.zeros(B, 1, dtype=torch.long, device=self.device)
        pos = torch.ones(B, 1, dtype=torch.long, device=self.device)       # only "not the prompt" matters: positions live on the device
        eos_at = [None] * B
        step = max(1, int(eos_check_every))
        for i in range(1, max_audio_frames + 1):
            if i % step == 0 or i == max_audio_frames:
                allz = (torch.stack(frames, 1) == 0).all(dim=2).cpu()                               # [B, frames so far]
                for b in range(B):
                    hit = allz[b].nonzero()
                    eos_at[b] = int(hit[0]) if hit.numel() else None
                if all(e is not None for e in eos_at) or i == max_audio_frames:
                    break
            tokens = torch.cat([frames[-1].long(), pad], dim=1).unsqueeze(1)
            frames.append(self._model.generate_frame(tokens, mask, pos, temperature, topk, **filters))
            if return_stats:
                fstats.append(self._model._decode_state.frame_stats())
        out, stats = [], []
        codes_all = torch.stack(frames, 2).long()                                                    # [B, K, T]
        for b in range(B):
            n = eos_at[b] if eos_at[b] is not None else min(len(frames), max_audio_frames)
            if return_stats:
                stats.append(SampleStats.of_frames(K, fstats[:n], b))
            if n == 0:
                out.append(torch.zeros(0, device=self.device))
            else:
                audio = self._audio_tokenizer.decode(codes_all[b:b + 1, :, :n]).squeeze(0).squeeze(0)
                out.append(audio if out_rs is None else out_rs(audio))
        return (out, stats) if return_stats else out

    def _batch_sampling(self, temperature, topk, B):
        """``generate_batch``'s temperature / topk: numbers pass through; a sequence must have one valid value per utterance
        (checked here, before the caches are taken over) and comes back as a list."""
        if not (_is_number(temperature) and _is_number(topk)):
            normalise(B, 1, self._model.args.audio_vocab_size, temperature, topk, unit="utterance")
        return _untouched(temperature), _untouched(topk)

    def serve(self, slots: int = 16, chunk_frames: int = 4, temperature: float = 0.9, topk: int = 50, hear_slots: int = 0,
              row_sampling: bool = False, row_filters: bool = False, top_p: float = 1.0, min_p: float = 0.0,
              output_sample_rate: Optional[int] = None, row_processors: bool = False, repetition_penalty=1.0,
              repetition_window=64, row_typical: bool = False, typical_p=1.0, streams: Optional[int] = None,
              max_lead_ms: Optional[float] = None, clock=None, sleep=None, stats: bool = False):
        """A running batch (csm/serving.py): ``server.submit(text, speaker, context, adapter=None, seed=None,
        max_audio_length_ms=90_000)`` queues an utterance, ``server.step()`` makes the next ``chunk_frames`` frames of audio for
        every utterance that holds one of the ``slots`` (<= 16) rows - utterances join at chunk boundaries, stream their audio
        chunk by chunk and leave at their own EOS - and ``server.run()`` iterates until all are done.  Temperature and top-k
        belong to the server - unless ``row_sampling=True``: then they are the requests' defaults, ``submit`` / ``conversation``
        / ``say`` take ``temperature=`` and ``topk=`` of their own (say > conversation > server), each slot samples with its
        request's pair through the rows sampler, and one captured frame serves every mix (a change never recaptures).  With
        ``row_filters=True`` as well (it needs ``row_sampling``), ``top_p`` / ``min_p`` are the requests' default nucleus and min-p
        cuts and ``submit`` / ``conversation`` / ``say`` take their own (``top_p=``, ``min_p=``); every draw then goes through the
        filtered rows sampler, and a request at 1.0 / 0.0 has the codes it has without ``row_filters``.  With
        ``row_processors=True`` (it needs ``row_sampling`` and includes ``row_filters``), ``repetition_penalty`` / ``repetition_window``
        are the requests' default windowed repetition penalty (``generate``), ``submit`` / ``conversation`` / ``say`` take their own,
        and each of the six parameters may be a sequence of K numbers, one per codebook; every draw then goes through the
        processed rows sampler, which remembers each slot's last 64 frames, and a request at penalty 1 has the codes it has with
        ``row_filters``.  With ``row_typical=True`` (it needs ``row_sampling`` and includes ``row_processors``), ``typical_p`` is the
        requests' default for locally typical sampling (``generate``), ``submit`` / ``conversation`` / ``say`` take their own - a
        number or K numbers - every draw goes through the typical rows sampler, and a request at 1.0 has the codes it has with
        ``row_processors``.  ``server.conversation(context, adapter, seed)`` opens a multi-turn dialogue on it: ``conv.say(text,
        speaker)`` queues its next turn as a request, ``conv.add(Segment)`` (or ``conv.hear(speaker)`` -> ``feed`` / ``end``, encoded
        while it is spoken) is the other party's turn; its KV history is parked
        between turns and resumed into any free slot, so more conversations than slots can be open.  It takes over the model's caches like any ``generate*`` call (open streams and older servers are
        invalidated) and binds the adapters loaded so far: load adapters first.
        ``hear_slots`` (0..16): 0, the default, gives every conversation that hears its own encode stream, one encoder step per
        ``feed``; N >= 1 gives the server one rows encoder of N slots - ``feed`` only buffers, ``server.hear_step()`` (called by
        ``step()``) encodes all open heard turns in one batched step, ``server.end_heard([(turn, text), ...])`` ends several.
        ``output_sample_rate``: the rate of every chunk and of ``Request.audio()`` (None: the codec's 24 kHz); the server then keeps
        one rows resampler over its slots - one more launch per ``step()``.  ``conv.hear(speaker, sample_rate=)`` is the input side.
        ``streams=N`` (slots <= N <= 256; None: today's server): up to N requests are in flight over the ``slots`` rows - every
        ``step()`` gives the rows to the requests whose listeners have the least audio ahead of them and parks the others in
        the middle of their utterances (one launch out, one in; the module docstring's "More listeners than slots"), with the
        same codes and audio per seeded request.  ``max_lead_ms``: a request that far ahead of its listener's clock is not
        scheduled (``clock`` / ``sleep``: ``time.monotonic`` / ``time.sleep`` unless given; all three need ``streams``).  It
        adds ``req.pause()`` / ``req.resume()``; ``server.cancel(req, heard_frames=None)`` works on every server.
        ``stats=True``: every request carries ``req.stats``, a ``SampleStats`` (``generate(return_stats=)``) that grows chunk by
        chunk with its codes, across park / resume, and is cut by ``cancel(heard_frames=)``; one more launch per frame."""
        from .serving import BatchServer
        return BatchServer(self, slots, chunk_frames, temperature, topk, hear_slots, row_sampling, row_filters, top_p, min_p,
                           output_sample_rate, row_processors, repetition_penalty, repetition_window, row_typical, typical_p,
                           streams, max_lead_ms, clock, sleep, stats)

    def voice(self, context: List[Segment], adapter: Optional[str] = None):
        """A voice prompt prefilled ONCE (csm/conversation.py: ``Voice``): the segments are tokenised and Mimi-encoded as every
        ``generate`` call does, prefilled on a one-row state with the bank adapter ``adapter`` and the K / V of their L positions
        are kept.  ``generate`` / ``generate_stream`` / ``conversation`` / ``server.submit`` / ``server.conversation`` take it as
        ``voice=``: the K / V are copied into the cache row (one launch for all voice requests a server admits together) and
        only what follows the voice - further context, the text - is fed, so a request pays neither the Mimi encode nor the
        prefill of its voice.  Refused (ValueError): an empty context, one that alone breaks the reference's length rule, an
        unknown adapter name, ``model.use_kv_cache`` off, live un-merged ``model.lora`` adapters.  The prefill does not depend on
        ``model.decode_weights``: one voice serves bf16 and FP8 decode alike.  It belongs to this Generator and model."""
        from .conversation import make_voice
        return make_voice(self, context, adapter)

    def conversation(self, context: Optional[List[Segment]] = None, adapter: Optional[str] = None, on_overflow: str = "error",
                     keep_turns: int = 0, voice=None):
        """A multi-turn dialogue that keeps its KV cache between turns (csm/conversation.py): ``conv.generate(text, speaker)`` /
        ``conv.generate_stream(...)`` speak the next line with every earlier turn as context, ``conv.add(Segment)`` adds the
        other party's turn - or ``turn = conv.hear(speaker)``, ``turn.feed(audio)`` as the audio arrives and ``turn.end(text)``,
        which Mimi-encodes the turn while it is spoken (``HeardTurn``).  ``adapter``: a bank adapter name for the whole conversation.  ``on_overflow``: ``"error"`` raises
        the reference's "Inputs too long" error when history + line + max_audio_frames reach max_seq_len, ``"drop_oldest"``
        drops whole turns - the oldest first, after the ``keep_turns`` leading ones (the voice prompt), which always stay - and
        prefills what is left; ``"shift"`` drops the same turns but keeps the cache: the kept keys are rotated back to their new
        positions (``DecodeState.shift_row``), nothing is prefilled again and the turn is appended as any other.
        ``voice``: a ``Voice`` (``Generator.voice``) the history starts with, already cached (``cached == voice.positions``):
        the first turn copies its K / V into the conversation's state and appends ``context`` - which comes after the voice -
        and the text.  ``adapter`` must be None or the voice's; the conversation speaks with the voice's.  After ``reset()`` or a
        ``drop_oldest`` the history is prefilled again from its tokens, like any other."""
        from .conversation import Conversation
        return Conversation(self, context or [], adapter, on_overflow, keep_turns, voice)

    def save_wav(self, path: str, audio: torch.Tensor, sample_rate: Optional[int] = None):
        """16-bit PCM writer (torchaudio is not available in this image).  ``sample_rate``: the rate ``audio`` is at (None: the
        codec's) - what a call with ``output_sample_rate=`` returned is written with that rate in the header."""
        import wave
        pcm = (audio.detach().float().cpu().clamp(-1, 1) * 32767.0).to(torch.int16).numpy().tobytes()
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(int(self.sample_rate if sample_rate is None else sample_rate))
            w.writeframes(pcm)


def load_csm_1b(ckpt_path: str = "ckpt.pt", device: str = "cuda", text_tokenizer=None, audio_tokenizer=None,
                mimi_weights: str = None, tokenizer_path: str = None, decode_weights: str = "bf16",
                fp8_adapters: bool = False) -> Generator:
    """Reference generator.py:221-244.  ``mimi_weights`` / ``tokenizer_path`` name local files for the two tokenizers the
    reference pulls from the hub.  ``decode_weights``: "bf16" or "fp8" (``Model.decode_weights``: weight-only e4m3 decode).
    ``fp8_adapters``: with "fp8", let per-utterance adapters and the bank run un-merged on the quantised base
    (``Model.fp8_adapters``: an opt-in - the adapters were trained against the bf16 base)."""
    if audio_tokenizer is None and mimi_weights:
        from .codec import load_mimi
        audio_tokenizer = load_mimi(mimi_weights, device=device)
    if text_tokenizer is None and tokenizer_path:
        text_tokenizer = load_llama3_tokenizer(tokenizer_path)
    args = ModelArgs(backbone_flavor="llama-1B", decoder_flavor="llama-100M", text_vocab_size=128256,
                     audio_vocab_size=2051, audio_num_codebooks=32)
    model = Model(args, device=device)
    model.load_state_dict(torch.load(ckpt_path, map_location="cpu", weights_only=False))
    model.decode_weights = decode_weights
    model.fp8_adapters = fp8_adapters
    return Generator(model, text_tokenizer=text_tokenizer, audio_tokenizer=audio_tokenizer)
