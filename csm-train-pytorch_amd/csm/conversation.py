"""Multi-turn generation that keeps the backbone's KV cache between turns (not in the reference, whose ``generate`` starts from
nothing every call: it Mimi-encodes every context segment again and prefills the whole history from position 0).

A ``Conversation`` owns the token history the model has been conditioned on and one ``DecodeState`` (KV caches, captured frame
graph).  A turn feeds only what the cache does not hold yet - ``history[cached:]`` plus the new line's text frames - through
``DecodeState.append`` (``csm_attn_append``: the new positions attend to the cached ones), so the time to the first frame
depends on the new line, not on the length of the conversation.  The frames the model speaks stay in the cache as they were
sampled; the other party's audio is Mimi-encoded once, when it is ``add``ed - or, with ``hear``, frame by frame while it is
still being spoken (``HeardTurn``), which takes the encode off the path between its last sample and our first chunk.
"""
from contextlib import contextmanager
from typing import Iterator, List, NamedTuple, Optional

import torch

from .engine import DecodeState
from .generator import sampling_kwargs
from .sampling import SampleStats

OVERFLOW = ("error", "drop_oldest", "shift")


class _Call(NamedTuple):
    """One ``generate`` / ``generate_stream`` call of a ``Generator`` or a ``Conversation``, checked (``prepare_call``)."""
    temperature: object
    topk: object
    filters: dict              # the other keywords of the frame calls (``sampling_kwargs``), ``stats=True`` among them when asked
    out_rs: object             # the ``Resampler`` to ``output_sample_rate``, or None
    return_stats: bool
    max_audio_frames: int
    every: int                 # frames between two host looks for EOS: ``eos_check_every``, a stream's ``chunk_frames``


def prepare_call(gen, max_audio_length_ms, temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p,
                 output_sample_rate, return_stats, eos_check_every=None, chunk_frames=None, stateless=False) -> _Call:
    """What every ``generate`` / ``generate_stream`` does first: the sampling values (``sampling_kwargs``), the output rate,
    ``return_stats`` of a ``stateless`` call (a ``Generator``'s own: it may be on the recompute path) and - for a stream, which
    names ``chunk_frames`` - the chunk size and the codec's ``decode_stream`` are checked, so a bad one raises at the call, before
    any cache or run counter is touched."""
    temperature, topk, filters = sampling_kwargs(gen, temperature, topk, top_p, min_p, repetition_penalty, repetition_window,
                                                 typical_p=typical_p)
    out_rs = gen._out_resampler(output_sample_rate)
    if stateless:
        gen._stats_check(return_stats)
    if chunk_frames is None:
        every = max(1, int(eos_check_every))
    else:
        if int(chunk_frames) != chunk_frames or chunk_frames < 1:
            raise ValueError(f"chunk_frames must be an integer >= 1, got {chunk_frames!r}")
        codec, every = gen._audio_tokenizer, int(chunk_frames)
        if not callable(getattr(codec, "decode_stream", None)):
            raise TypeError(f"{type(codec).__name__} has no decode_stream(): streaming needs a stateful decoder "
                            "(decoding chunks independently would be wrong at the chunk edges)")
    if return_stats:
        filters = dict(filters, stats=True)
    return _Call(temperature, topk, filters, out_rs, return_stats, int(max_audio_length_ms / 80), every)


class _Turn:
    """A spoken utterance in flight: the sampled frames, how many of them were handed out and - a conversation's turn - how many
    were fed back into its cache."""

    def __init__(self):
        self.samples: List[torch.Tensor] = []
        self.stats: List[torch.Tensor] = []        # per sample, its frame's statistics on the device (return_stats)
        self.kept = 0                              # frames handed to the caller so far (stream) / kept (generate)
        self.base = 0                              # history length (= cached positions) after the text frames
        self.fed = 0                               # samples[:fed] have been fed to the backbone (one position each)
        self.done = False


def drive(turn: _Turn, step, call: _Call):
    """THE utterance loop.  ``step(turn)`` samples the next frame into ``turn.samples`` (the first one from the prompt, every
    later one from the frame before it; with ``return_stats`` its statistics into ``turn.stats``), so the frame calls are enqueued
    back to back; the all-zero EOS test runs on the device and the host looks at it once per ``call.every`` frames and at the
    last one.  Every look sets ``turn.kept`` and yields the slice of ``turn.samples`` it adds to the kept frames - the frames
    before the EOS frame; the look that finds it is the last.  Frames sampled past EOS are never kept."""
    looked = 0                                     # samples[:looked] are known not to be EOS
    for i in range(call.max_audio_frames):
        step(turn)
        n = len(turn.samples)
        if n - looked >= call.every or i == call.max_audio_frames - 1:
            hit = (torch.cat(turn.samples[looked:], 0) == 0).all(dim=1).nonzero()                  # one host look per chunk
            turn.kept = looked + int(hit[0]) if hit.numel() else n
            yield slice(looked, turn.kept)
            if hit.numel():
                return
            looked = n


def spoken(gen, turn: _Turn, call: _Call):
    """What ``generate`` returns for a driven turn: ONE decode of its kept frames (and their statistics)."""
    samples = turn.samples[:turn.kept]
    audio = torch.zeros(0, device=gen.device)
    if samples:
        audio = gen._audio_tokenizer.decode(torch.stack(samples).permute(1, 2, 0).long()).squeeze(0).squeeze(0)
        audio = audio if call.out_rs is None else call.out_rs(audio)
    if not call.return_stats:
        return audio
    return audio, SampleStats.of_frames(gen._model.args.audio_num_codebooks, turn.stats[:turn.kept])


def stream_spoken(gen, turn: _Turn, step, call: _Call, check):
    """What ``generate_stream`` yields: ``drive`` with every look's frames pushed through the codec's stateful decoder (and the
    resampler stream).  ``check()`` raises once the stream was invalidated - asked after every chunk handed out."""
    K = gen._model.args.audio_num_codebooks
    decoder = gen._audio_tokenizer.decode_stream()
    out = call.out_rs.stream() if call.out_rs is not None else None
    for new in drive(turn, step, call):
        if new.stop > new.start:
            chunk = decoder.step(torch.stack(turn.samples[new]).permute(1, 2, 0).long()).reshape(-1)       # codes [1, K, n]
            chunk = chunk if out is None else out.feed(chunk)
            yield (chunk, SampleStats.of_frames(K, turn.stats[new])) if call.return_stats else chunk
            check()
    if out is not None and out.pos:                                # the samples the resampler still owes (its lag)
        yield (out.flush(), SampleStats(K)) if call.return_stats else out.flush()


class Voice:
    """``Generator.voice(context, adapter)``: a voice prompt that was tokenised, Mimi-encoded and prefilled ONCE and is forked
    into any number of requests, conversations and server slots (``generate(voice=)``, ``conversation(voice=)``,
    ``BatchServer.submit(voice=)`` / ``.conversation(voice=)``).

    ``tokens`` / ``mask`` ([L, K+1]) are the segments' frames in the layout of a conversation's history, ``turns`` their lengths,
    ``kv`` ([layers, 2, KV, L, hd] bf16) the backbone's K / V of those L positions as ``DecodeState.park_row`` returns them,
    ``adapter`` the bank adapter it was prefilled with (a name or None), ``positions`` = L and ``nbytes`` the size of ``kv``.
    ``kv`` is never written after creation: every user copies it into a cache row of its own (``resume_row`` / ``fork_rows``) or
    shifts it out of place (``shift_parked``), so one tensor is shared by reference by all of them.

    A voice belongs to the model (and Generator) it was made on and is valid for the weights of that moment: after training
    steps or a merge make a new one.  The prefill is the training forward and does not read ``model.decode_weights``, so one
    voice serves bf16 and FP8 decode alike.  A plain tensor, not captured into any frame graph: voices can be made and dropped
    while a server runs."""

    def __init__(self, gen, tokens, mask, turns, kv, adapter):
        self._gen, self._model = gen, gen._model
        self.tokens, self.mask, self.turns, self.kv, self.adapter = tokens, mask, tuple(turns), kv, adapter

    @property
    def positions(self) -> int:
        return self.tokens.shape[0]

    @property
    def nbytes(self) -> int:
        return self.kv.numel() * self.kv.element_size()

    def check(self, gen, adapter, what: str):
        """The rules of every ``voice=`` argument: the voice is this Generator's (and its model's), and ``adapter`` is not named
        or names the voice's own.  Returns the adapter the caller speaks with: the voice's."""
        if self._gen is not gen or self._model is not gen._model:
            raise ValueError(f"{what}: this voice was made on another Generator / model (its cache holds that model's K / V)")
        if adapter is not None and adapter != self.adapter:
            raise ValueError(f"{what}: adapter {adapter!r} with a voice that was prefilled with adapter {self.adapter!r} - the "
                             "cache is only valid for the adapter it was computed with")
        return self.adapter


@torch.inference_mode()
def make_voice(gen, context, adapter=None) -> Voice:
    """``Generator.voice``: the segments are tokenised as ``_tokenize_segment`` does, prefilled on a one-row ``DecodeState`` made
    with the bank adapter ``adapter``, and the row is parked."""
    m, e = gen._model, gen._model.engine
    context = list(context)
    if not context:
        raise ValueError("voice: an empty context (a voice is at least one segment)")
    if not getattr(m, "use_kv_cache", True):
        raise ValueError("voice: a voice is a KV cache: model.use_kv_cache must be on")
    lora = getattr(m, "lora", None)
    if lora is not None and not lora.merged:
        raise ValueError("voice: live (un-merged) LoRA adapters are attached as model.lora - their weights move, so the cache "
                         "would go stale: merge them (merge_lora_weights), detach them, or add them to the bank and name one")
    ads = gen._resolve_adapters([adapter])                          # (an unknown name raises ValueError here)
    toks, msks = zip(*(gen._tokenize_segment(seg) for seg in context))
    tokens, mask = torch.cat(toks, 0).long().to(gen.device), torch.cat(msks, 0).bool().to(gen.device)
    limit = m.bb.max_seq_len - 1                                    # the reference's rule with one frame of audio
    if tokens.shape[0] >= limit:
        raise ValueError(f"voice: Inputs too long, must be below max_seq_len - max_audio_frames: {limit}")
    e._need()
    st = DecodeState(e, 1, ads)
    st.prefill(tokens.unsqueeze(0), mask.unsqueeze(0))
    return Voice(gen, tokens, mask, [t.shape[0] for t in toks], st.park_row(0, tokens.shape[0]), adapter)


class HeardTurn:
    """``conv.hear(speaker)`` on a ``Conversation`` or a ``ServedConversation``: the other party's turn, Mimi-encoded while it is
    still being spoken (``MimiCodec.encode_stream``) so that nothing but the last partial frame is left to encode when it ends.
    ``feed(audio)`` encodes the whole frames now available and touches neither the history nor the caches - it may be called
    while the conversation's own turn streams, while the server steps and while other conversations speak; ``end(text)`` flushes
    the last partial frame (zero-padded) and enters the turn exactly as ``add(Segment(speaker, text, audio))`` does - for audio
    of a whole number of frames ``tokens`` and ``mask`` are equal to that path's; ``cancel()`` drops the turn."""

    def __init__(self, conv, speaker: int, stream, resampler=None):
        self._conv, self.speaker, self._stream = conv, speaker, stream
        self._rs = resampler                       # ``hear(sample_rate=)``: a ResampleStream in front of the encode stream
        self._codes: List[torch.Tensor] = []
        self._frames = 0
        self.closed = False

    def _check(self, what):
        if self.closed:
            raise RuntimeError(f"{what}: this heard turn was ended or cancelled")

    def _take(self, codes):
        if codes.shape[2]:
            self._codes.append(codes[0])
            self._frames += codes.shape[2]

    @property
    def frames(self) -> int:
        """Frames encoded so far."""
        return self._frames

    @property
    def pending(self) -> int:
        """Whole frames fed but not encoded yet: always 0 here - ``feed`` encodes them at once.  (On a server with
        ``hear_slots`` they wait for ``hear_step``: ``SlotHeardTurn`` in csm/serving.py.)"""
        return 0

    @torch.inference_mode()
    def feed(self, audio: torch.Tensor) -> int:
        """The next samples of the turn, any number of them ((n,), at the ``sample_rate`` given to ``hear`` - the codec's 24 kHz
        by default); returns ``frames``."""
        self._check("feed")
        if self._rs is not None:
            audio = self._rs.feed(audio)
        self._take(self._stream.feed(audio.reshape(1, 1, -1)))
        return self._frames

    @torch.inference_mode()
    def end(self, text: str) -> None:
        """The turn is over and ``text`` is what was said: the history gets the text frames, the streamed codes and the all-zero
        EOS frame; they enter the cache with the next spoken turn."""
        self._check("end")
        conv, gen = self._conv, self._conv._gen
        conv._before_history("end")                                 # (raises with the turn still open: end() can be retried)
        if self._rs is not None:                                    # the samples the resampler still owes, then the encoder's flush
            self._take(self._stream.feed(self._rs.flush().reshape(1, 1, -1)))
        self._take(self._stream.flush())
        self._enter(*gen._tokenize_text_segment(text, self.speaker))

    def _enter(self, tt, tm) -> None:
        """The turn enters the history: the text frames ``tt`` / ``tm``, the codes taken so far, the EOS frame."""
        conv, gen = self._conv, self._conv._gen
        K = gen._model.args.audio_num_codebooks
        codes = torch.cat(self._codes, 1) if self._codes else torch.zeros(K, 0, dtype=torch.long, device=gen.device)
        at, am = gen._audio_frames(codes.to(gen.device))
        self.closed, conv._heard = True, None
        conv._push(torch.cat([tt, at], dim=0).long(), torch.cat([tm, am], dim=0).bool())

    def cancel(self) -> None:
        """Drop the turn: nothing of it enters the history."""
        if not self.closed:
            self.closed, self._conv._heard = True, None


def hear_resampler(gen, sample_rate):
    """``hear(sample_rate=)``: None for None or the codec's own rate, else the ``Resampler`` from that rate to the codec's."""
    from .codec.resample import rate_resampler
    return rate_resampler("sample_rate", sample_rate, gen.sample_rate, gen.device, to_native=True)


class _History:
    """The dialogue history of ``Conversation`` and ``ServedConversation`` (csm/serving.py): the frames the model has been
    conditioned on (``_tokens`` / ``_mask``), the lengths of the turns that make them up (``_turns``), how many leading positions
    have their K / V cached (``_cached``), the length rule and the other party's turns (``add`` / ``hear``).  Where the cached
    K / V live - a state of its own, a parked tensor between two slots - is the subclass's, and so is ``_before_history(what)``:
    what ``add`` and ``HeardTurn.end`` do before they extend the history."""

    def __init__(self, gen, on_overflow: str, keep_turns: int, voice):
        if on_overflow not in OVERFLOW:
            raise ValueError(f"on_overflow must be one of {OVERFLOW}, got {on_overflow!r}")
        if isinstance(keep_turns, bool) or not isinstance(keep_turns, int) or keep_turns < 0:       # (a bool is not a count)
            raise ValueError(f"keep_turns must be an integer >= 0, got {keep_turns!r}")
        self._gen, self._on_overflow, self._keep_turns = gen, on_overflow, keep_turns
        K1 = gen._model.args.audio_num_codebooks + 1
        self._tokens = torch.zeros(0, K1, dtype=torch.long, device=gen.device)
        self._mask = torch.zeros(0, K1, dtype=torch.bool, device=gen.device)
        self._turns: List[int] = []                # lengths of the turns that make up the history
        self._cached = 0
        self._heard: Optional[HeardTurn] = None    # the other party's turn being heard (hear), at most one
        self._enc = None                           # its encode stream: made at the first hear, reused
        self._hear_rs = {}                         # hear(sample_rate=): input rate -> its ResampleStream, made once, reused
        if voice is not None:                      # the history starts as the voice's frames, already cached (``voice.kv``)
            self._tokens, self._mask, self._turns, self._cached = voice.tokens, voice.mask, list(voice.turns), voice.positions

    # ---- read-only views ---------------------------------------------------------------------------------------------------
    @property
    def tokens(self) -> torch.Tensor:
        return self._tokens

    @property
    def mask(self) -> torch.Tensor:
        return self._mask

    @property
    def cached(self) -> int:
        return self._cached

    # ---- history -----------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def add(self, segment) -> None:
        """The other party's turn (or any context segment): only THIS segment is tokenised and Mimi-encoded, here, once.  It
        enters the cache with the next spoken turn."""
        if self._heard is not None:
            raise RuntimeError("add: a heard turn is open on this conversation - end() or cancel() it first")
        self._before_history("add")
        t, m = self._gen._tokenize_segment(segment)
        self._push(t.long(), m.bool())

    def hear(self, speaker: int, sample_rate: Optional[int] = None) -> HeardTurn:
        """The other party starts to speak: ``turn.feed(audio)`` Mimi-encodes the turn as it arrives, ``turn.end(text)`` enters it
        as ``add`` would - with nothing left to encode but its last partial frame.  ``sample_rate``: the rate of the samples
        ``feed`` will get (None: the codec's 24 kHz); another rate is resampled on the device as it arrives, and the turn enters
        as ``add`` of ``ops.resample(whole, sample_rate, 24000)`` would.
        At most one heard turn is open per conversation; its encode stream is made at the first ``hear`` and started anew
        (``reset()``) for every later one, and so is the ``ResampleStream`` of each rate."""
        rs = hear_resampler(self._gen, sample_rate)
        if self._heard is not None:
            raise RuntimeError("hear: this conversation already has a heard turn open - end() or cancel() it first")
        if self._enc is None:
            codec = self._gen._audio_tokenizer
            if not callable(getattr(codec, "encode_stream", None)):
                raise TypeError(f"{type(codec).__name__} has no encode_stream(): hearing a turn as it arrives needs a stateful encoder")
            self._enc = codec.encode_stream()
        else:
            self._enc.reset()
        stream = None
        if rs is not None:
            stream = self._hear_rs.get(rs.orig_sr)
            if stream is None:
                stream = self._hear_rs[rs.orig_sr] = rs.stream()
            else:
                stream.reset()
        self._heard = HeardTurn(self, speaker, self._enc, stream)
        return self._heard

    def _push(self, t, m):
        self._tokens = torch.cat([self._tokens, t.to(self._tokens.device)], 0)
        self._mask = torch.cat([self._mask, m.to(self._mask.device)], 0)
        self._turns.append(t.shape[0])

    def _close_turn(self, frames):
        """The spoken turn the text frames opened is over: its kept frames ([k, K] codes) and one all-zero EOS frame enter the
        history (the layout of ``Generator._tokenize_segment``)."""
        k, K = frames.shape
        t = torch.zeros(k + 1, K + 1, dtype=torch.long, device=self._tokens.device)
        t[:k, :K] = frames
        m = torch.zeros(k + 1, K + 1, dtype=torch.bool, device=self._mask.device)
        m[:, :K] = True
        self._tokens = torch.cat([self._tokens, t], 0)
        self._mask = torch.cat([self._mask, m], 0)
        self._turns[-1] += k + 1

    def fit_history(self, n_new: int, limit: int):
        """The reference's length rule (generator.py:168-170) on history + new text: ``drop_oldest`` and ``shift`` drop whole
        turns, the oldest first AFTER the ``keep_turns`` leading ones (the voice prompt), until it holds.  Raises the
        reference's error - with nothing changed - when it cannot.  Returns None when nothing had to go; else (head, out): the
        cut starts at position ``head`` of the OLD history and is gone from ``_tokens`` / ``_mask`` / ``_turns``; ``out`` of its
        positions were cached (<= 0: none) - what becomes of the cache is the caller's."""
        L = self._tokens.shape[0]
        if L + n_new < limit:
            return None
        first = min(self._keep_turns, len(self._turns))
        drop, left = first, L
        if self._on_overflow != "error":
            while drop < len(self._turns) and left + n_new >= limit:
                left -= self._turns[drop]
                drop += 1
        if left + n_new >= limit:
            raise ValueError(f"Inputs too long, must be below max_seq_len - max_audio_frames: {limit}")
        head, gone = sum(self._turns[:first]), L - left
        self._tokens = torch.cat([self._tokens[:head], self._tokens[head + gone:]], 0) if head else self._tokens[gone:]
        self._mask = torch.cat([self._mask[:head], self._mask[head + gone:]], 0) if head else self._mask[gone:]
        self._turns = self._turns[:first] + self._turns[drop:]
        return head, min(self._cached, head + gone) - head


open_heard_turn = _History.hear        # (the name it had as a free function: ``open_heard_turn(conv, speaker, sample_rate)``)


class Conversation(_History):
    """``Generator.conversation(...)``.  One dialogue, B = 1.

    ``tokens`` / ``mask`` ([L, K+1]) are the frame history the model has been conditioned on, laid out as the reference lays out
    its context: per turn the text frames, the audio frames, one all-zero EOS frame - for a spoken turn the codes are the ones
    the model sampled, not a re-encoding of its audio.  ``cached`` leading positions of it have their K / V in the cache; the
    rest goes in with the next turn.  Under the same torch seed the first ``generate`` equals ``Generator.generate`` with the
    same context bit for bit; later turns differ from a stateless call by design (own codes instead of re-encoded ones).

    The conversation owns its ``DecodeState`` and installs it as the model's only while one of its calls samples a frame, so
    ``Generator.generate*`` calls between turns and other conversations do not disturb it; only its own open
    ``generate_stream`` is invalidated by its own next call (the frames already handed out are kept, the rest rolled back -
    the same happens when a stream is abandoned).  The caches of a conversation take 67 MB at CSM-1B (16 layers x K and V x
    8 kv heads x 2048 positions x 64 x bf16) plus the depth decoder's 0.5 MB.

    The cache is only valid for the weights it was computed with: after training steps, an adapter swap or a merge call
    ``reset()`` - the history is kept and prefilled again by the next turn.
    """

    def __init__(self, gen, context=(), adapter: Optional[str] = None, on_overflow: str = "error", keep_turns: int = 0,
                 voice: Optional[Voice] = None):
        super().__init__(gen, on_overflow, keep_turns, voice)
        self._m = gen._model
        if voice is not None:
            adapter = voice.check(gen, adapter, "conversation")
        self._ads = gen._resolve_adapters([adapter])
        self._state: Optional[DecodeState] = None
        self._run = 0
        self._open: Optional[_Turn] = None
        # a voice's K / V, parked, while they wait for the state the first turn makes (never written)
        self._fork = voice.kv if voice is not None else None
        for seg in context:
            self.add(seg)

    def _before_history(self, what):
        """What ``add`` and ``HeardTurn.end`` do before they extend the history: an open stream of this conversation is
        invalidated and its turn settled."""
        self._run += 1
        self._settle()

    def reset(self) -> None:
        """Drop the cache (and the captured frame graph), keep the history: the next turn prefills it from position 0 with the
        weights and adapters of that moment."""
        self._run += 1
        self._settle()
        self._state, self._cached, self._fork = None, 0, None

    def _fit(self, n_new: int, max_audio_frames: int):
        """The reference's length rule on history + new text (``fit_history``).  Under ``drop_oldest`` what is kept is prefilled
        again.  Under ``shift`` the cache slides instead: ONE ``DecodeState.shift_row`` takes the cut's cached positions out and
        rotates the keys behind them back (cut positions that were only pending just leave the pending tokens), so the turn is
        fed by ``append`` like any other - unless nothing cached is left, which is ``drop_oldest``."""
        cut = self.fit_history(n_new, self._m.bb.max_seq_len - max_audio_frames)
        if cut is None:
            return
        head, out = cut
        if self._on_overflow != "shift" or self._cached - max(out, 0) < 1:
            self._cached = 0
        elif out > 0:
            self._state.shift_row(0, head, out)
            self._cached -= out

    # ---- a spoken turn -----------------------------------------------------------------------------------------------------
    @contextmanager
    def _installed(self):
        m = self._m
        prev = getattr(m, "_decode_state", None)
        m._decode_state = self._state
        try:
            yield
        finally:
            m._decode_state = prev

    def _step(self, text, speaker, call: _Call):
        """``step`` of ``drive`` for this conversation's next turn."""
        return lambda turn: self._next_frame(turn, call) if turn.samples else self._begin(turn, text, speaker, call)

    def _begin(self, turn: _Turn, text, speaker, call: _Call):
        """Feed what the cache lacks plus the new line's text frames, sample the first frame: ``turn`` is now the open one."""
        m, e = self._m, self._m.engine
        temperature, topk, filters = call.temperature, call.topk, dict(call.filters)
        stats = filters.pop("stats", False)
        if not getattr(m, "use_kv_cache", True):
            raise RuntimeError("a Conversation keeps the KV cache between turns: model.use_kv_cache must be on")
        tt, tm = self._gen._tokenize_text_segment(text, speaker)
        if self._fork is not None:                                   # a voice's first turn: its K / V into a state of our own
            e._need()
            self._state = DecodeState(e, 1, self._ads)
            self._state.resume_row(0, self._fork)
            self._fork = None
        self._fit(tt.shape[0], call.max_audio_frames)
        new_t = torch.cat([self._tokens[self._cached:], tt.long()], 0)
        new_m = torch.cat([self._mask[self._cached:], tm.bool()], 0)
        e._need()
        if self._state is None:
            self._state = DecodeState(e, 1, self._ads)
        st = self._state
        if stats:
            st.enable_stats()                                        # (it stays on: the state's later turns keep the one frame body)
        if self._cached == 0:
            last_h = st.prefill(new_t.unsqueeze(0), new_m.unsqueeze(0))
        else:
            last_h = st.append(new_t, new_m)
        self._push(tt.long(), tm.bool())
        self._cached = turn.base = self._tokens.shape[0]
        self._open = turn
        if filters:                                                  # (the rows path of this conversation's state)
            temperature, topk = st.sampling_args(temperature, topk, **filters)
            if st.sampler.keeps_history:
                # (a turn's repetition window covers its own frames)
                st.reset_row_history(0)
                st.set_live([0])
        turn.samples.append(e._frame_tail(st, last_h, temperature, topk, None))
        if stats:
            turn.stats.append(st.frame_stats())

    def _next_frame(self, turn: _Turn, call: _Call):
        """Feed the last sampled frame, sample the next one (``Model.generate_frame`` on this conversation's state)."""
        K = self._m.args.audio_num_codebooks
        dev = self._gen.device
        tokens = torch.cat([turn.samples[-1].long(), torch.zeros(1, 1, dtype=torch.long, device=dev)], dim=1).unsqueeze(1)
        mask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], dim=1).unsqueeze(1).to(dev)
        with self._installed():
            s = self._m.generate_frame(tokens, mask, torch.ones(1, 1, dtype=torch.long), call.temperature, call.topk,
                                       **call.filters)
        turn.fed += 1
        turn.samples.append(s)
        if call.return_stats:
            turn.stats.append(self._state.frame_stats())

    def _settle(self):
        """Close the turn in flight, if any: the history gets its kept frames and one all-zero EOS frame (the layout of
        ``Generator._tokenize_segment``), the cache is rolled back to the last position that is part of the history."""
        turn, self._open = self._open, None
        if turn is None or turn.done:
            return
        turn.done = True
        k = turn.kept
        self._close_turn(torch.cat(turn.samples[:k], 0) if k else self._tokens[:0, :-1])
        # positions base .. base+fed-1 hold samples[:fed]; of those the kept frames stay.  The EOS frame always enters with the
        # next turn's append, also where eos_check_every > 1 had fed it already (a decode step and an append round differently):
        # what the cache holds after a turn does not depend on how often the host looked for EOS
        keep = min(turn.fed, k)
        if turn.fed > keep:
            self._state.truncate(turn.base + keep)
        self._cached = turn.base + keep

    @torch.inference_mode()
    def generate(self, text: str, speaker: int, max_audio_length_ms: float = 90_000, temperature: float = 0.9, topk: int = 50,
                 eos_check_every: int = 8, top_p: float = 1.0, min_p: float = 0.0,
                 output_sample_rate: Optional[int] = None, repetition_penalty=1.0, repetition_window=64,
                 typical_p=1.0, return_stats: bool = False):
        """Speak ``text`` as ``speaker`` with the whole history as context; arguments (``top_p`` / ``min_p``, ``repetition_penalty``
        / ``repetition_window`` / ``typical_p``, per-codebook sequences, ``output_sample_rate`` and ``return_stats`` included: this
        turn's) and EOS handling as ``Generator.generate``.  The repetition window looks at this turn's frames only.  The first
        turn with ``return_stats`` puts the conversation's state into statistics mode, where it stays."""
        return self._speak(text, speaker, prepare_call(self._gen, max_audio_length_ms, temperature, topk, top_p, min_p,
                                                        repetition_penalty, repetition_window, typical_p, output_sample_rate,
                                                        return_stats, eos_check_every=eos_check_every))

    @torch.inference_mode()
    def _speak(self, text, speaker, call: _Call):
        """``generate`` for a prepared call (``Generator.generate(voice=)`` makes its own): the turn driven to its end."""
        self._run += 1
        self._settle()
        turn = _Turn()
        try:
            for _ in drive(turn, self._step(text, speaker, call), call):
                pass
        finally:
            self._settle()
        return spoken(self._gen, turn, call)

    def generate_stream(self, text: str, speaker: int, max_audio_length_ms: float = 90_000, temperature: float = 0.9,
                        topk: int = 50, chunk_frames: int = 4, top_p: float = 1.0, min_p: float = 0.0,
                        output_sample_rate: Optional[int] = None, repetition_penalty=1.0,
                        repetition_window=64, typical_p=1.0, return_stats: bool = False) -> Iterator[torch.Tensor]:
        """``generate`` handing the audio out chunk by chunk, as ``Generator.generate_stream`` does (``return_stats``: (chunk,
        ``SampleStats``) pairs, likewise); under the same seed the chunks concatenate to ``generate``'s audio.  A later call on
        THIS conversation invalidates the stream."""
        return self._speak_stream(text, speaker, prepare_call(self._gen, max_audio_length_ms, temperature, topk, top_p, min_p,
                                                               repetition_penalty, repetition_window, typical_p,
                                                               output_sample_rate, return_stats, chunk_frames=chunk_frames))

    def _speak_stream(self, text, speaker, call: _Call):
        """``generate_stream`` for a prepared call: this conversation's open stream, if any, ends here; the new one is returned."""
        self._run += 1
        self._settle()
        return self._stream(self._run, text, speaker, call)

    @torch.inference_mode()
    def _stream(self, run, text, speaker, call: _Call):
        def check():
            if self._run != run:
                raise RuntimeError("this stream was invalidated: a later call on the same Conversation took its turn")

        check()
        turn = _Turn()
        try:
            yield from stream_spoken(self._gen, turn, self._step(text, speaker, call), call, check)
        finally:
            if self._open is turn:
                self._settle()
