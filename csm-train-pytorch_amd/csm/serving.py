"""A running batch: utterances join, stream their audio and leave slot by slot (``Generator.serve``).

``generate_batch`` is closed - all prompts arrive together, nothing is heard before the last row ends - and ``generate_stream``
speaks for one user.  ``BatchServer`` puts batch decode, per-row LoRA adapters and streaming together: up to 16 slots over one
``DecodeState`` (csm/engine.py: ``prefill_row``, ``set_row_adapter``, ``set_active``, ``serve_first`` / ``serve_frame``) and one
batched stateful Mimi decoder (``MimiCodec.decode_stream_rows``).

One ``step()`` makes one chunk of ``chunk_frames`` frames for every request in a slot:
  1. the rows already running sample their first frame of the chunk (one decode frame; free slots idle);
  2. queued requests are admitted into free slots - lowest slot first, one prefill each, then ONE frame tail over the batch
     gives their first frame.  Admission happens here only, at a chunk boundary, so every row of the chunk has the same n;
  3. ``chunk_frames - 1`` decode frames advance all of them (a row that has reached its ``max_audio_length`` idles);
  4. the host looks at the chunk once for EOS frames; one rows-codec step decodes every row at the full n (frames past a
     row's end zeroed) and each row's audio is cut to its frames before EOS / its length limit (the decoder is causal, so
     those samples are exact); rows that ended release their slot.
A request with a ``seed`` draws its sampler noise from its own generator (``DecodeState.fill_noise``), so its codes and audio do
not depend on its slot, its neighbours or when it joined.

Sampling parameters.  By default temperature and top-k belong to the server: they reach the sampler as launch scalars and are the
key of the captured frame graph.  With ``serve(row_sampling=True)`` they belong to the request: ``submit`` / ``conversation`` /
``say`` take ``temperature`` and ``topk`` (say > conversation > server's), the slot gets them at admission
(``DecodeState.set_row_sampling``: two small device writes outside the graph) and every draw of every frame goes through the rows
sampler (``csm_sample_topk_rows``), which reads ``topk[b]`` / ``temperature[b]`` from device memory.  One captured frame
then serves every mix of parameters - a greedy row (``topk=1``) next to a 0.9 / 50 one - and a change never recaptures.  A row's
codes are those of a default server made with that row's pair (the same bits).  A free row keeps the pair of its last request.

Filters.  ``serve(row_sampling=True, row_filters=True, top_p=1.0, min_p=0.0)`` adds a nucleus (top-p) and a min-p cut per request,
resolved and checked like the pair (``submit`` / ``conversation`` / ``say`` take ``top_p`` and ``min_p``; say > conversation >
server's) and written at admission (``DecodeState.set_row_filters``).  The server raises its state to that level before its first
capture, so every draw goes through the filtered rows sampler (``csm_sample_filtered_rows``): min-p, then the nucleus, inside the
sampler's one launch, on what top-k kept.  A row at (1.0, 0.0) skips both and has the codes of a ``row_sampling`` server; a change
of any row's four parameters replays the same captured frame.  Without ``row_filters`` nothing here is touched.

Processors.  ``serve(row_sampling=True, row_processors=True, repetition_penalty=1.0, repetition_window=64)`` includes the filters and
adds a windowed repetition penalty per request (``repetition_penalty`` / ``repetition_window``, resolved and checked like the others)
and parameters per codebook: each of the six is a number or a sequence of K numbers.  They are written at admission
(``DecodeState.set_row_processors``: six [K, B] buffers, column b) and every draw goes through the processed rows sampler
(``csm_sample_processed_rows``), which keeps each slot's last 64 codes per codebook in a ring on the device and penalises the
logits of the codes of the last ``repetition_window`` frames before the draw.  Every joining row starts at frame 0
(``reset_row_history``), resumed conversation turns included - a turn's window covers that turn's frames only, nothing is parked
with the conversation - and only the rows a frame is for count it: the joined rows in the first-frame tail, the active rows in a
decode frame.  So a request has the same codes in any slot, whoever joins beside it; at penalty 1 they are the codes of a
``row_filters`` server; a change of any of a row's parameters replays the same captured frame.

Typical sampling.  ``serve(row_sampling=True, row_typical=True, typical_p=1.0)`` includes the processors and adds locally typical
sampling per request (``typical_p`` in (0, 1], a number or K numbers; resolved and checked like the others), written at admission
(``DecodeState.set_row_typical``: the seventh of the state's [K, B] buffers, at 1.0 until then); every draw goes through the
typical rows sampler (``csm_sample_typical_rows``), which keeps, of what the other filters left, the tokens whose surprise is
closest to the entropy - it can drop the most likely code, which no other filter can.  At 1.0 a request has the codes of a ``row_processors`` server; a
change of ``typical_p`` replays the same captured frame.

Multi-turn conversations (``BatchServer.conversation`` -> ``ServedConversation``) outlive their slot.  A conversation holds a
slot only while it speaks: at the end of the chunk in which its turn ended the K / V of its history positions are parked
(``DecodeState.park_row``: one copy, base + kept frames - what the row sampled after EOS or after its length limit is not
history) and the slot is free again; its next turn is admitted like any request into ANY free slot, where the parked history is
copied back (``resume_row``) and only what the cache lacks - the last frame(s) of its own turn, the EOS frame, the other party's
``add``ed turns, the new line's text - is fed.  All turns resumed at one chunk boundary are fed by ONE ``DecodeState.append_rows``
(one walk over the backbone's weights; ``csm_attn_append_rows``), after the prefills of plain requests and first turns and before
the one frame tail that gives every joiner its first frame.  So more conversations than slots can be open at once, and a turn's
time to its first chunk depends on the new line, not on the length of the dialogue.
An idle row's position is pinned to 0 and the frame writes a zero token's K / V at position 1 of that row: harmless for a row
that is free, fatal for a history.  A row held by a conversation is therefore never idled: where a plain request at its length
limit idles for the rest of the chunk, a conversation's row keeps sampling to the chunk's end and the extra frames are cut from
the audio and from the parked length, as frames after EOS are - which is why ``say`` asks for ``chunk_frames - 1`` positions of
headroom beyond ``max_audio_frames``.  A conversation's ``seed`` gives it one generator for its whole life, which moves only
when the conversation samples a frame and travels with it from slot to slot.

Voices (``Generator.voice`` -> ``Voice``, csm/conversation.py): a voice prompt tokenised, Mimi-encoded and prefilled once.
``submit(text, speaker, context, voice=v)`` tokenises only ``context`` and the text; the request carries that feed and the voice.
All voice requests admitted at one chunk boundary get the voice's K / V by ONE ``DecodeState.fork_rows`` (``csm_kv_fork_rows``:
the same source for any number of rows) and are fed, together with the resumed conversation turns, by the ONE ``append_rows`` -
no Mimi encode and no prefill per request.  ``conversation(voice=v)`` starts with the voice as its history and ``v.kv`` as its
parked cache (shared, never written: ``resume_row`` copies, ``shift_parked`` is out of place), so its first ``say`` is a resumed
turn.  The length rule counts the voice's positions; ``adapter`` must be None or the voice's.

Hearing (``conv.hear`` -> ``turn.feed`` / ``turn.end``) Mimi-encodes the other party's turn while it is spoken.  By default
every conversation owns a ``MimiEncodeStream`` and every ``feed`` is one encoder step for that conversation.  With
``serve(hear_slots=N)`` (1..16) the server owns ONE ``MimiEncodeStreamRows`` of N slots instead: ``hear`` takes a free encoder
slot, ``feed`` only buffers, and ``hear_step()`` - which ``step()`` calls first - encodes what waits in every open heard turn
with one batched ``drain``: N listeners cost one encoder step per chunk (plus one per distinct backlog, ``peel_schedule``).
``turn.end`` drains and flushes its own slot; ``end_heard`` does it for turns that end together with one drain for all.

Other sample rates (csm/codec/resample.py).  ``conv.hear(speaker, sample_rate=16000)`` takes the turn's samples at that rate:
without ``hear_slots`` the turn owns a ``ResampleStream`` in front of its encode stream; with them ``feed`` buffers the raw
samples and ``hear_step`` first resamples every row that has new ones - ONE rows launch per distinct input rate among them
(``ResampleStreamRows`` over the encoder slots) - and hands the 24 kHz samples to the encoder's ``feed``; ``end_heard`` ends the
resampler streams (their ``final`` step) before the encoder's flush.  ``serve(output_sample_rate=48000)`` makes every chunk and
``Request.audio()`` 48 kHz: one table, one rows stream over the decode slots, one rows launch per ``step()`` on the rows that
produced audio - a row that ends in that step ends its stream there (``final``), so its last chunk carries the resampler's lag.
Histories are codes and do not change.

More listeners than slots (``serve(streams=N)``, slots <= N <= 256).  A step makes a stream's audio several times faster than it
is heard, so a request need not hold its row all the time.  Up to N requests are *in flight*: admitted, not done.  An in-flight
request owns one codec state (and one resampler carry) from admission to its end - the rows codec objects are made with
``state_slots=N``, their kernels take the arena's slot count apart from the rows of a launch, so that state is never copied -
and holds a decode slot only in the steps it is scheduled.  What a row is, in the middle of an utterance: the K / V of the
``row_pos + 1`` positions it holds, its last sampled frame (``_tok``: sampled, not yet fed), at the ring levels its ring of
sampled codes and its frame counter, its noise generator, and on the host its adapter, its sampling parameters and its
counters.  ``DecodeState.park_rows`` takes the device part of up to 16 rows out in ONE launch per kind (``csm_kv_park_rows``,
``csm_sample_hist_move_rows``) and ``resume_rows`` puts it into any rows (``csm_kv_fork_rows`` and the ring move back); no
buffer a captured frame reads changes address and the level stays, so a rotation never recaptures.
The schedule runs at the start of every ``step()``, before the running rows' first frame.  Candidates: the in-flight requests
that are neither paused nor - under ``max_lead_ms`` - too far ahead, each with its *lead*; and, while fewer than ``streams`` are
in flight (paused ones count), the queued requests in FIFO order with lead minus infinity.  Lead = the milliseconds of audio
emitted - fair share, the clock is never read - or, with ``max_lead_ms=L``, that minus the time since ``t0``, the clock at the
return of the step that delivered the request's first chunk (before it: the emitted milliseconds); only leads below L are
candidates.  The ``slots`` candidates with the least (lead, id) get the slots: rows that were not chosen leave by ONE
``park_rows``, chosen parked requests return by ONE ``resume_rows`` - lowest free slot first, in (lead, id) order, with their
``_tok`` row, adapter and parameters; the ring counters are restored, not reset - chosen new ones go through the admission
above, and a chosen request that holds a slot stays there.  Resumed rows are running rows of that step.  A row that
is not scheduled in a step that runs always leaves its slot (an idle frame would overwrite position 1 of its cache): in fair
share that only happens with more candidates than slots, under ``max_lead_ms`` also to a request that is at or over the bound
while others run, free slots or not.  With no candidate ``step()`` returns ``[]`` and touches nothing.
``next_due()``: the seconds until somebody is a candidate (0.0: now; None: nothing in flight or queued, or all paused; never
less than a millisecond otherwise - at the instant a lead reaches the bound it is not yet below it); ``run()`` sleeps it
(``sleep`` / ``clock``: ``time.sleep`` / ``time.monotonic`` unless given).  ``req.pause()`` takes a request out of the
candidates - the next step that runs parks it if it holds a slot - and ``req.resume()`` puts it back.  A seeded request has
the codes and audio it has without ``streams``, however often and wherever it is parked.  ``Request.state`` / ``preemptions`` /
``slots_held`` and ``server.stats`` (steps, parks, resumes, launches of each) tell what happened.
``cancel(req, heard_frames=None)`` - every server, with or without ``streams`` - ends a request wherever it is.  A plain
request is dropped; a conversation's turn ends as at a length limit with ``min(heard_frames, emitted)`` frames kept (barge-in:
history and parked cache hold the text and what was heard), taken out of its slot or out of its parked row.  Its codec and
resampler slots are free at once; the resampler's lag is not flushed.

Limitations: a join stalls the other rows for one whole prefill or append (no chunked prefill); the context audio of a request
and a conversation's ``add``ed turns are Mimi-encoded at ``submit`` / ``add``, one segment at a time (only ``conv.hear`` encodes
while the turn is being spoken - and only with ``hear_slots`` batched over the conversations); adapters added to the
Generator after ``serve()`` are unknown to the server (the state binds the bank at creation).
"""
from collections import deque
from typing import Iterator, List, Optional, Tuple

import torch

from .conversation import HeardTurn, _History, hear_resampler
from .engine import DecodeState
from .sampling import FULL_LEVEL, HIST_FRAMES, LEVELS, NAMES, PARAMS, SampleStats, _as_list, _is_number, check_row, own_params


MAX_STREAMS = 256           # the most requests in flight on a ``streams`` server (each keeps a codec state for its whole life)
FRAME_MS = 80.0             # one frame of audio
MIN_SLEEP = 1e-3            # ``next_due`` never asks for less: at the exact instant a lead reaches the bound it is not yet below it


def _collapsed(vals):
    """``check_row``'s tuples of K values, each as one number where every codebook has the same."""
    return tuple(v[0] if all(x == v[0] for x in v) else v for v in vals)


class Request:
    """One utterance of a ``BatchServer``: its audio arrives in ``chunks`` while it holds a slot; ``done`` once it has ended."""

    def __init__(self, rid, text, speaker, adapter, seed, max_audio_frames, tokens, mask, device, temperature=None, topk=None,
                 top_p=1.0, min_p=0.0, repetition_penalty=1.0, repetition_window=HIST_FRAMES, typical_p=1.0):
        self.id, self.text, self.speaker, self.adapter, self.seed = rid, text, speaker, adapter, seed
        self.temperature, self.topk = temperature, topk      # resolved: what it is sampled with
        self.top_p, self.min_p = top_p, min_p                # (likewise; 1.0 / 0.0 on a server without row_filters)
        # (likewise; 1.0 / 64 without row_processors.  With them each of the six is a number, or a tuple of K: one per codebook)
        self.repetition_penalty, self.repetition_window = repetition_penalty, repetition_window
        self.typical_p = typical_p                           # (likewise; 1.0 without row_typical)
        self.max_audio_frames = max_audio_frames
        self.slot: Optional[int] = None          # the slot it holds (None while queued and after it ended)
        self.done = False
        self.chunks: List[torch.Tensor] = []
        self._codes: List[torch.Tensor] = []
        self.stats = None                        # serve(stats=True): a SampleStats that grows chunk by chunk with ``_codes``
        self._tokens, self._mask, self._device = tokens, mask, device
        self._sampled = 0                        # frames sampled / handed out so far
        self._emitted = 0
        self._conv: Optional["ServedConversation"] = None     # the conversation this is a turn of (tokens / mask: what it feeds)
        self.sample_rate: Optional[int] = None   # the rate of ``chunks`` / ``audio()`` (the server's; set when it queues)
        self._base = 0                           # a turn: positions the cache holds once the feed is in
        self._voice = None                       # submit(voice=): the Voice whose K / V the slot gets; tokens / mask: what follows it
        self.cancelled = False                   # ended by BatchServer.cancel
        self.preemptions = 0                     # times it was parked in the middle of the utterance (``streams`` servers)
        self.slots_held: List[int] = []          # every decode slot it has held, in order
        self._srv = None
        self._paused = False
        self._row = None                         # engine.ParkedRow while it is in flight without a slot; _tokrow: its last frame
        self._tokrow = None
        self._cslot: Optional[int] = None        # its codec / resampler slot (the decode slot, unless the server has ``streams``)
        self._t0 = None                          # pacing: the clock when its first chunk was delivered

    @property
    def state(self) -> str:
        """``queued`` / ``running`` (it holds a slot) / ``parked`` (in flight, out of its slot) / ``paused`` / ``done``."""
        if self.done:
            return "done"
        if self._paused:
            return "paused"
        return "running" if self.slot is not None else "parked" if self._row is not None else "queued"

    def pause(self) -> None:
        """Take the request out of the schedule (a ``streams`` server): if it holds a slot, the next ``step()`` parks it; a
        queued one is passed over.  Nothing is lost - ``resume()`` continues with the same codes.  No-op on a done request."""
        self._srv._pause(self, True)

    def resume(self) -> None:
        """Put a paused request back into the schedule."""
        self._srv._pause(self, False)

    def audio(self) -> torch.Tensor:
        """The audio so far (all of it once ``done``): the chunks concatenated."""
        return torch.cat(self.chunks) if self.chunks else torch.zeros(0, device=self._device)

    def codes(self) -> torch.Tensor:
        """The frames behind ``audio()``, [K, T] int64."""
        if not self._codes:
            return torch.zeros(self._tokens.shape[-1] - 1, 0, dtype=torch.long, device=self._device)
        return torch.cat(self._codes, 1)


class SlotHeardTurn(HeardTurn):
    """``conv.hear(speaker)`` on a server with ``hear_slots``: the turn holds one slot of the server's ``MimiEncodeStreamRows``
    from ``hear`` to ``end`` / ``cancel`` / ``conv.close()``.  ``feed`` only buffers (nothing is launched; the piece is held as
    given until the next ``hear_step``, so do not overwrite it before); ``frames`` counts the frames encoded so far,
    ``pending`` the whole frames that wait for the next ``hear_step``."""

    def __init__(self, conv, speaker: int, server, slot: int, rows=None):
        super().__init__(conv, speaker, server._hear)
        self._srv, self.slot = server, slot
        self._rows = rows                        # ``hear(sample_rate=)``: the server's ResampleStreamRows of that rate (or None)
        self._raw: List[torch.Tensor] = []       # samples at that rate fed since the last hear_step, as given
        self._raw_n = 0

    @property
    def pending(self) -> int:
        if self.closed:
            return 0
        if self._rows is None:
            return self._stream.pending(self.slot)
        from .codec.resample import step_outputs
        rs = self._rows.rs                       # what the waiting raw samples will give the encoder, in whole frames
        more = step_outputs(self._rows.pos[self.slot], self._raw_n, False, rs.o, rs.n, rs.width)
        return (self._stream._count[self.slot] + more) // self._stream.frame

    def feed(self, audio: torch.Tensor) -> int:
        self._check("feed")
        self._srv._check()
        if self._rows is None:
            self._stream.feed(self.slot, audio.reshape(-1))
        elif audio.numel():
            self._raw.append(audio.detach().reshape(-1))
            self._raw_n += audio.numel()
        return self._frames

    def _take_raw(self, limit: int):
        """Up to ``limit`` of the waiting raw samples as one tensor (None when nothing waits)."""
        if not self._raw_n:
            return None
        dev = self._rows.rs.device
        buf = self._raw[0].to(dev, torch.float32) if len(self._raw) == 1 else torch.cat([p.to(dev, torch.float32) for p in self._raw])
        head, rest = buf[:limit], buf[limit:]
        self._raw, self._raw_n = ([rest], rest.numel()) if rest.numel() else ([], 0)
        return head

    def end(self, text: str) -> None:
        self._srv.end_heard([(self, text)])

    def cancel(self) -> None:
        if not self.closed:
            self._srv._free_heard(self)
            super().cancel()


class ServedConversation(_History):
    """``BatchServer.conversation(...)``: one dialogue served turn by turn (see the module docstring).  ``tokens`` / ``mask`` /
    ``cached`` mean what they mean on ``Conversation`` and the history has its layout: per turn the text frames, the audio frames,
    one all-zero EOS frame; a spoken turn's frames are the sampled codes; the EOS frame always enters with the next feed."""

    def __init__(self, server, context, adapter, seed, on_overflow, temperature=None, topk=None, top_p=None, min_p=None,
                 keep_turns: int = 0, repetition_penalty=None, repetition_window=None, voice=None, typical_p=None):
        super().__init__(server._gen, on_overflow, keep_turns, voice)
        self._srv, self.adapter, self.seed = server, adapter, seed
        # its turns' defaults, resolved
        for name, v in zip(NAMES, server._resolve("conversation", (temperature, topk, top_p, min_p, repetition_penalty,
                                                                   repetition_window, typical_p))):
            setattr(self, name, v)
        # DecodeState.park_row of the ``cached`` leading positions, while it holds no slot.  A voice's K / V are the parked cache -
        # shared, never written (resume_row copies it into the slot, shift_parked is out of place) - so the first ``say`` is a
        # resumed turn like any other
        self._parked = voice.kv if voice is not None else None
        self._noise = None                       # its generator (made at the first admission: lives on the state's device)
        self._open: Optional[Request] = None
        self.closed = False
        for seg in context:
            self.add(seg)

    def _idle(self, what):
        self._srv._check()
        if self.closed:
            raise RuntimeError(f"{what}: this conversation was closed")
        if self._open is not None and not self._open.done:
            raise RuntimeError(f"{what}: this conversation's turn (request {self._open.id}) is still open - one turn at a time")

    def hear(self, speaker: int, sample_rate: Optional[int] = None) -> HeardTurn:
        """The other party starts to speak: ``turn.feed(audio)`` Mimi-encodes the turn as it arrives - between the server's steps,
        whoever holds the slots - and ``turn.end(text)`` enters it as ``add`` would, under ``add``'s rules (no turn of this
        conversation still open), with nothing left to encode but its last partial frame.  On a server with ``hear_slots`` the
        turn takes one of its encoder slots (``SlotHeardTurn``; RuntimeError when none is free).  ``sample_rate``: the rate of
        the samples ``feed`` will get (None: the codec's 24 kHz), resampled on the device - module docstring."""
        self._srv._check()
        if self.closed:
            raise RuntimeError("hear: this conversation was closed")
        if self._srv.hear_slots:
            return self._srv._open_heard(self, speaker, sample_rate)
        return super().hear(speaker, sample_rate)

    _before_history = _idle                      # (``add`` and ``HeardTurn.end``: under ``say``'s rules)

    def _fit(self, n_new: int, max_audio_frames: int):
        """``Conversation._fit``: the reference's length rule on history + new text (``fit_history``).  Under ``drop_oldest`` the
        parked cache is dropped and what is kept is prefilled again; under ``shift`` ONE ``DecodeState.shift_parked`` takes the
        cut's cached positions out of the parked cache, so the turn is resumed and fed by the stacked ``append_rows`` like any
        other - unless nothing cached is left, which is ``drop_oldest``."""
        cut = self.fit_history(n_new, self._srv._model.bb.max_seq_len - max_audio_frames)
        if cut is None:
            return
        head, out = cut                                            # (cached = parked positions)
        if self._on_overflow != "shift" or self._parked is None or self._cached - max(out, 0) < 1:
            self._cached, self._parked = 0, None
        elif out > 0:
            self._parked = self._srv._state.shift_parked(self._parked, head, out)
            self._cached -= out

    @torch.inference_mode()
    def say(self, text: str, speaker: int, max_audio_length_ms: float = 90_000, temperature: Optional[float] = None,
            topk: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None,
            repetition_penalty=None, repetition_window=None, typical_p=None) -> Request:
        """Queue the next spoken turn; its audio streams through ``step()`` / ``run()`` like any request's.  The length rule
        counts ``chunk_frames - 1`` frames beyond ``max_audio_length_ms``: a conversation's row samples to the end of its last
        chunk (module docstring), and that must fit the cache - it raises here, not in ``step``.  ``temperature`` / ``topk``
        (``row_sampling`` servers), ``top_p`` / ``min_p`` (``row_filters`` servers) and ``repetition_penalty`` / ``repetition_window`` /
        a sequence of K values for any of the six (``row_processors`` servers), ``typical_p`` (``row_typical`` servers): this
        turn's, over the conversation's.  The window looks at this turn's frames only."""
        self._idle("say")
        srv = self._srv
        params = srv._resolve("say", (temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p),
                              [getattr(self, name) for name in NAMES])
        max_audio_frames = int(max_audio_length_ms / 80)
        if max_audio_frames < 1:
            raise ValueError(f"max_audio_length_ms = {max_audio_length_ms!r} is less than one 80 ms frame")
        tt, tm = self._gen._tokenize_text_segment(text, speaker)
        self._fit(tt.shape[0], max_audio_frames + srv.chunk_frames - 1)
        feed_t = torch.cat([self._tokens[self._cached:], tt.long().to(self._tokens.device)], 0)
        feed_m = torch.cat([self._mask[self._cached:], tm.bool().to(self._mask.device)], 0)
        self._push(tt.long(), tm.bool())
        req = Request(srv._next_id, text, speaker, self.adapter, self.seed, max_audio_frames, feed_t, feed_m, self._gen.device, *params)
        req._conv, req._base, req.sample_rate, req._srv = self, self._tokens.shape[0], srv.sample_rate, srv
        req.stats = SampleStats(srv._K) if srv.sample_stats else None
        srv._next_id += 1
        srv._queue.append(req)
        self._open = req
        return req

    def _end_turn(self, req: Request, state, b, kept: Optional[int] = None):
        """The turn has ended in slot ``b`` (``BatchServer.step``): the history gets the kept frames and one EOS frame, the cache
        its history positions only - base + the kept frames that were fed back - which are parked.  ``kept``
        (``BatchServer.cancel``): the frames that count, at most those emitted; ``b`` is then the slot, or None for a turn that
        holds none - a preempted one's positions come out of its parked row, a queued one's parked cache stays as it is."""
        k = req._emitted if kept is None else min(int(kept), req._emitted)
        self._close_turn(req.codes().t()[:k])
        # positions base .. base + sampled - 2 hold the frames that were fed back (the last one sampled never was)
        if b is None and req._row is None:       # (cancelled while queued: nothing of the turn ever reached a cache)
            return
        self._cached = req._base + min(req._sampled - 1, k)
        self._parked = state.park_row(b, self._cached) if b is not None else req._row.kv[:, :, :, :self._cached].contiguous()

    def close(self) -> None:
        """Drop the parked cache (the history stays readable); a heard turn that holds an encoder slot is cancelled."""
        self._idle("close")
        if isinstance(self._heard, SlotHeardTurn):
            self._heard.cancel()
        self._parked, self._cached, self.closed = None, 0, True


class BatchServer:
    """``Generator.serve``: see the module docstring.  Without ``row_sampling`` temperature and top-k belong to the server - they
    are launch scalars of the sampler and the key of the captured frame graph.  With it they are the defaults of the requests,
    which may bring their own: the rows sampler reads each slot's pair from device memory and the graph's key is (None, None).
    ``row_filters`` (needs ``row_sampling``): ``top_p`` / ``min_p`` are the requests' default filters and requests may bring their
    own; every draw goes through the filtered rows sampler.  ``row_processors`` (needs ``row_sampling``; includes what
    ``row_filters`` gives): ``repetition_penalty`` / ``repetition_window`` join the requests' defaults, each of the six may be a
    sequence of K values (one per codebook), and every draw goes through the processed rows sampler, which remembers each slot's
    last 64 frames (``DecodeState.set_row_processors``).  ``row_typical`` (needs ``row_sampling``; includes what ``row_processors``
    gives): ``typical_p`` joins the requests' defaults, a number or K numbers, and every draw goes through the typical rows
    sampler (``DecodeState.set_row_typical``); a request at 1.0 has the codes it has with ``row_processors``.
    ``stats`` (``sample_stats`` on the server; ``server.stats`` is its counters): the state runs in statistics mode
    (``DecodeState.enable_stats``: one more launch per frame) and every request carries ``req.stats``, a ``SampleStats`` that
    grows chunk by chunk with its codes - read with the chunk's one host look.  The numbers are per frame, not state: nothing
    moves with a parked row, and ``cancel(req, heard_frames=k)`` cuts them to k frames."""

    def __init__(self, gen, slots: int = 16, chunk_frames: int = 4, temperature: float = 0.9, topk: int = 50, hear_slots: int = 0,
                 row_sampling: bool = False, row_filters: bool = False, top_p: float = 1.0, min_p: float = 0.0,
                 output_sample_rate: Optional[int] = None, row_processors: bool = False, repetition_penalty=1.0,
                 repetition_window=HIST_FRAMES, row_typical: bool = False, typical_p=1.0, streams: Optional[int] = None,
                 max_lead_ms: Optional[float] = None, clock=None, sleep=None, stats: bool = False):
        out_rs = gen._out_resampler(output_sample_rate)      # (a bad rate raises here, before anything is taken over)
        gen._stats_check(stats)
        if streams is None:
            for name, v in (("max_lead_ms", max_lead_ms), ("clock", clock), ("sleep", sleep)):
                if v is not None:
                    raise ValueError(f"{name} belongs to the schedule of a server with more streams than slots: it needs streams=")
        else:
            if isinstance(streams, bool) or not isinstance(streams, int):
                raise ValueError(f"streams must be an integer in slots..{MAX_STREAMS}, got {streams!r}")
            if max_lead_ms is not None and (not _is_number(max_lead_ms) or not 0 < float(max_lead_ms) < float("inf")):
                raise ValueError(f"max_lead_ms must be a finite number > 0 (milliseconds of audio ahead of the listener), got {max_lead_ms!r}")
            for name, v in (("clock", clock), ("sleep", sleep)):
                if v is not None and not callable(v):
                    raise ValueError(f"{name} must be callable, got {v!r}")
        # the level: the highest one asked for (it includes those below); a flag needs row_sampling, a value off its identity its flag
        flags = dict(row_sampling=row_sampling, row_filters=row_filters, row_processors=row_processors, row_typical=row_typical)
        given = (temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p)
        level = max((n for n, lv in enumerate(LEVELS) if lv.flag and flags[lv.flag]), default=0)
        for n in range(len(LEVELS) - 1, 1, -1):
            if flags[LEVELS[n].flag] and not row_sampling:
                raise ValueError(LEVELS[n].needs)
            if level < n and self._names(n, given, lambda j: not (_is_number(given[j]) and given[j] == PARAMS[j].identity)):
                raise ValueError(LEVELS[n].value.format(**dict(zip(NAMES, given))))
        if int(slots) != slots or not 1 <= slots <= 16:
            raise ValueError(f"slots must be an integer in 1..16, got {slots!r}")
        if streams is not None and not slots <= streams <= MAX_STREAMS:
            raise ValueError(f"streams must be an integer in slots..{MAX_STREAMS} (slots = {int(slots)}), got {streams!r}")
        if int(hear_slots) != hear_slots or not 0 <= hear_slots <= 16:
            raise ValueError(f"hear_slots must be an integer in 0..16 (0: one encode stream per conversation), got {hear_slots!r}")
        if int(chunk_frames) != chunk_frames or chunk_frames < 1:
            raise ValueError(f"chunk_frames must be an integer >= 1, got {chunk_frames!r}")
        codec = gen._audio_tokenizer
        if not callable(getattr(codec, "decode_stream_rows", None)):
            raise TypeError(f"{type(codec).__name__} has no decode_stream_rows(): serving needs a batched stateful decoder")
        if hear_slots and not callable(getattr(codec, "encode_stream_rows", None)):
            raise TypeError(f"{type(codec).__name__} has no encode_stream_rows(): hear_slots needs a batched stateful encoder")
        self._gen, self._model = gen, gen._model
        self.slots, self.chunk_frames, self.hear_slots = int(slots), int(chunk_frames), int(hear_slots)
        self.level = level
        for n in range(1, len(LEVELS)):                  # (row_sampling, row_filters, row_processors, row_typical)
            setattr(self, LEVELS[n].flag, level >= n)
        self._K = gen._model.args.audio_num_codebooks
        # the requests' defaults: what the level reads held to the requests' rule (before anything is taken over), the rest at its
        # identity - but the pair of a server without row_sampling: the scalar path's two launch numbers, as they are
        reads = LEVELS[level].reads
        defaults = self._held(None, given[:reads] + tuple(p.identity for p in PARAMS[reads:]))
        for name, v in zip(NAMES, defaults if level else (float(temperature), int(topk)) + defaults[LEVELS[1].reads:]):
            setattr(self, name, v)
        gen._run += 1                                    # takes over the model's caches, as generate_batch does
        self._run = gen._run
        self._model.reset_caches()
        self._model.engine._need()                       # (sharded / offloaded parameters: gathered before anything reads them)
        self._bank = dict(gen._bank.entries) if gen._bank is not None else {}
        # more streams than slots: a request keeps one codec (and resampler) state from admission to its end, whichever decode
        # slot it is scheduled into - the arenas are sized to ``streams`` and nothing of them is ever copied
        self.streams = None if streams is None else int(streams)
        more = {} if self.streams is None else {"state_slots": self.streams}
        with torch.inference_mode():
            self._state = DecodeState(self._model.engine, self.slots, bank=list(self._bank.values()))
            self.sample_stats = bool(stats)
            if self.sample_stats:
                self._state.enable_stats()               # (before the first capture)
            self._codec = codec.decode_stream_rows(slots=self.slots, max_chunk_frames=self.chunk_frames, **more)
        # heard turns: one rows encoder for all conversations (None: each conversation makes its own MimiEncodeStream).  Made
        # outside inference mode: ``conv.hear`` opens its slot (an in-place zero fill of the state) from ordinary caller code
        self._hear = codec.encode_stream_rows(slots=self.hear_slots) if self.hear_slots else None
        self._hearing: List[Optional[SlotHeardTurn]] = [None] * self.hear_slots     # encoder slot -> the turn that holds it
        self._hear_rs = {}                               # input rate -> ResampleStreamRows over the encoder slots (hear(sample_rate=))
        # speaking at another rate: one rows resampler over the decode slots, a step takes at most one chunk per row
        self.sample_rate = int(gen.sample_rate) if out_rs is None else out_rs.new_sr
        self._out = None
        if out_rs is not None:
            self._out = out_rs.stream_rows(self.slots, self.chunk_frames * (int(gen.sample_rate) * 80 // 1000), **more)     # (80 ms frames)
        self._model._decode_state = self._state
        # every row starts with valid parameters (the sampler runs on all rows), the state at its level before the first capture
        self._set_rows(range(self.slots), self._defaults())
        K = self._K
        dev = gen.device
        self._tok = torch.zeros(self.slots, 1, K + 1, dtype=torch.long, device=dev)      # each row's last sampled frame
        self._mask = torch.cat([torch.ones(self.slots, 1, K, dtype=torch.bool), torch.zeros(self.slots, 1, 1, dtype=torch.bool)],
                               2).to(dev)
        self._last_h = None
        self._rows: List[Optional[Request]] = [None] * self.slots
        self._queue = deque()
        self._next_id = 0
        self.last_join_rows = 0                          # requests admitted by the latest step (for timing a join)
        # the schedule of a ``streams`` server: the requests in flight (admitted, not done - running, parked or paused), the codec
        # slots nobody holds, the pacing bound and its clock
        self._flight: List[Request] = []
        self._cfree = list(range(self.streams or 0))
        self.max_lead_ms = None if max_lead_ms is None else float(max_lead_ms)
        if self.streams is not None:
            import time
            self._clock, self._sleep = clock or time.monotonic, sleep or time.sleep
        self.stats = {"steps": 0, "parks": 0, "resumes": 0, "park_launches": 0, "resume_launches": 0}

    # ------------------------------------------------------------------------------------------------------------ requests
    def _check(self):
        if self._gen._run != self._run:
            raise RuntimeError("this server was invalidated: a later generate / generate_batch / generate_stream / serve call on "
                               "the same Generator took over the model's caches")

    @staticmethod
    def _names(n, values, named):
        """Whether ``values`` name what only level ``n`` and above take: one of its own parameters (``named(j)``), or - the first
        level of whole rows - a sequence (one value per codebook) in a parameter below it."""
        mine = own_params(n)
        return any(named(j) for j in mine) or (n == FULL_LEVEL and any(_as_list(v) is not None for v in values[:mine.start]))

    def _defaults(self):
        return tuple(getattr(self, name) for name in NAMES)

    def _held(self, what, params):
        """One value per parameter as this server's rows take them: those its level reads held to their rules - a number each, or
        (whole rows) K numbers, one per codebook, which come back as a tuple of K where they differ - and the rest as they are.  A
        rule's refusal names the call (``what``) where the rows are whole, as it always did."""
        lv = LEVELS[self.level]
        reads = lv.reads
        if not reads:                                    # (the scalar path: nothing of a request's reaches the sampler)
            return tuple(params)
        try:
            head = _collapsed(check_row(self._K, self._model.args.audio_vocab_size, range(reads), params[:reads], each=lv.rings))
        except ValueError as e:
            raise ValueError(f"{what}: {e}" if what and lv.rings else str(e)) from None
        return head + tuple(params[reads:])

    def _resolve(self, what, named, default=None):
        """A request's sampling parameters (one per ``PARAMS`` record; None: not named), resolved against ``default`` (the server's
        if None) and held to the rows' rules (``_held``) - at the call, so a bad request raises before it queues.  What only a level
        above the server's takes is refused when named, highest level first; what its level does not read comes back as the default."""
        d = self._defaults() if default is None else default
        for n in range(len(LEVELS) - 1, self.level, -1):
            if self._names(n, named, lambda j: named[j] is not None and not (
                    PARAMS[j].identity_ok and _is_number(named[j]) and named[j] == PARAMS[j].identity)):
                raise ValueError(LEVELS[n].refusal.format(what=what, **dict(zip(NAMES, self._defaults()))))
        return self._held(what, [dv if j >= LEVELS[self.level].reads or v is None else v for j, (v, dv) in enumerate(zip(named, d))])

    def _sample_args(self):
        """What ``serve_first`` / ``serve_frame`` get: the server's two numbers, or None, None (each row's own pair)."""
        return (None, None) if self.row_sampling else (self.temperature, self.topk)

    def submit(self, text: str, speaker: int, context, adapter: Optional[str] = None, seed: Optional[int] = None,
               max_audio_length_ms: float = 90_000, temperature: Optional[float] = None, topk: Optional[int] = None,
               top_p: Optional[float] = None, min_p: Optional[float] = None, repetition_penalty=None,
               repetition_window=None, voice=None, typical_p=None) -> Request:
        """Queue one utterance; it takes a slot at the next chunk boundary that has a free one.  The prompt is tokenised here, so
        the reference's length rule ("Inputs too long ...") and an unknown adapter name raise here.  ``temperature`` / ``topk``
        (``row_sampling`` servers), ``top_p`` / ``min_p`` (``row_filters`` servers) and ``repetition_penalty`` / ``repetition_window`` /
        a sequence of K values, one per codebook, for any of the six (``row_processors`` servers), ``typical_p`` (``row_typical``
        servers): this request's, over the server's.
        ``voice``: a ``Voice`` of this Generator - the prompt is the voice, then ``context`` (which may be empty), then
        the text; only context and text are tokenised here and fed at admission, and the length rule counts the voice's positions.
        ``adapter`` must be None or the voice's: the request speaks with the voice's."""
        self._check()
        params = self._resolve("submit", (temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p))
        if voice is not None:
            adapter = voice.check(self._gen, adapter, "submit")
        if adapter is not None and adapter not in self._bank:
            known = self._gen._bank is not None and adapter in self._gen._bank.entries
            raise ValueError(f"unknown LoRA adapter {adapter!r} (bound by this server: {list(self._bank)})" +
                             (": it was added after serve(); the state binds the bank at creation - start a new server" if known else ""))
        max_audio_frames = int(max_audio_length_ms / 80)
        if max_audio_frames < 1:
            raise ValueError(f"max_audio_length_ms = {max_audio_length_ms!r} is less than one 80 ms frame")
        with torch.inference_mode():
            tokens, mask = self._gen._prompt_frames(text, speaker, context, max_audio_frames,
                                                    held=voice.positions if voice is not None else 0)
        req = Request(self._next_id, text, speaker, adapter, seed, max_audio_frames, tokens, mask, self._gen.device, *params)
        req.sample_rate, req._voice, req._srv = self.sample_rate, voice, self
        req.stats = SampleStats(self._K) if self.sample_stats else None
        self._next_id += 1
        self._queue.append(req)
        return req

    def conversation(self, context=(), adapter: Optional[str] = None, seed: Optional[int] = None,
                     on_overflow: str = "error", temperature: Optional[float] = None,
                     topk: Optional[int] = None, top_p: Optional[float] = None,
                     min_p: Optional[float] = None, keep_turns: int = 0, repetition_penalty=None,
                     repetition_window=None, voice=None, typical_p=None) -> ServedConversation:
        """A multi-turn dialogue on this server: ``conv.say(text, speaker, max_audio_length_ms)`` queues its next spoken turn (a
        ``Request``), ``conv.add(Segment)`` is the other party's turn, ``conv.close()`` drops its parked cache.  ``adapter`` and
        ``seed`` hold for the whole conversation; ``on_overflow`` / ``keep_turns`` as for ``Generator.conversation`` (``"shift"``
        slides the parked cache at ``say``).  ``temperature`` / ``topk``
        (``row_sampling`` servers), ``top_p`` / ``min_p`` (``row_filters`` servers) and ``repetition_penalty`` /
        ``repetition_window`` / per-codebook sequences (``row_processors`` servers), ``typical_p`` (``row_typical`` servers): the
        defaults of its turns, over the server's; ``say`` may name a turn's own.
        ``voice``: a ``Voice`` of this Generator the history starts with, already
        cached - its K / V are the conversation's parked cache (shared, never written), so the first ``say`` is resumed and
        fed like a later turn; ``context`` comes after the voice; ``adapter`` must be None or the voice's."""
        self._check()
        if voice is not None:
            adapter = voice.check(self._gen, adapter, "conversation")
        if adapter is not None and adapter not in self._bank:
            raise ValueError(f"unknown LoRA adapter {adapter!r} (bound by this server: {list(self._bank)})")
        return ServedConversation(self, list(context), adapter, seed, on_overflow, temperature, topk, top_p, min_p, keep_turns,
                                  repetition_penalty, repetition_window, voice, typical_p)

    @property
    def queued(self) -> int:
        return len(self._queue)

    @property
    def active(self) -> List[Request]:
        """The requests that hold a slot, in slot order."""
        return [r for r in self._rows if r is not None]

    # ------------------------------------------------------------------------------------------------------------- hearing
    def _open_heard(self, conv, speaker: int, sample_rate=None) -> SlotHeardTurn:
        rs = hear_resampler(self._gen, sample_rate)
        if conv._heard is not None:
            raise RuntimeError("hear: this conversation already has a heard turn open - end() or cancel() it first")
        free = [s for s, t in enumerate(self._hearing) if t is None]
        if not free:
            raise RuntimeError(f"hear: all hear_slots = {self.hear_slots} encoder slots are taken - end() or cancel() a heard turn, "
                               "or serve with more")
        rows = None
        if rs is not None:                               # one rows stream per input rate, over the encoder slots; a step takes <= 1 s
            rows = self._hear_rs.get(rs.orig_sr)
            if rows is None:
                rows = self._hear_rs[rs.orig_sr] = rs.stream_rows(self.hear_slots)
            rows.open(free[0])
        self._hear.open(free[0])
        conv._heard = self._hearing[free[0]] = SlotHeardTurn(conv, speaker, self, free[0], rows)
        return conv._heard

    def _free_heard(self, turn: SlotHeardTurn):
        self._hear.close(turn.slot)
        if turn._rows is not None:
            turn._rows.close(turn.slot)
        self._hearing[turn.slot] = None

    def _resample_heard(self, turns, final=False):
        """The raw samples waiting in ``turns`` go through their rates' rows resamplers - one launch per distinct rate (more only
        for a backlog beyond a launch's ``max_in``) - and on to the encoder's ``feed``.  ``final``: the turns end - every one of
        them with a rate ends its resampler stream, with or without new samples."""
        by_rate = {}
        for t in turns:
            if t._rows is not None and (t._raw_n or final):
                by_rate.setdefault(t._rows.rs.orig_sr, []).append(t)
        for group in by_rate.values():
            rows = group[0]._rows
            while group:
                xs = [t._take_raw(rows.max_in) for t in group]
                last = [t for t in group if not t._raw_n]                # (nothing left behind: the turn's part is done)
                ys = rows.step([t.slot for t in group], xs, final=[t.slot for t in last] if final else ())
                for t, y in zip(group, ys):
                    self._hear.feed(t.slot, y)
                group = [t for t in group if t._raw_n]

    @torch.inference_mode()
    def hear_step(self) -> int:
        """Encode what waits in every open heard turn: ONE ``drain`` over all of them (nothing is launched when nothing waits).
        ``step()`` calls it first.  Returns the number of frames encoded."""
        self._check()
        self._resample_heard([t for t in self._hearing if t is not None])
        turns = [t for t in self._hearing if t is not None and self._hear.pending(t.slot)]
        if not turns:
            return 0
        codes = self._hear.drain([t.slot for t in turns])
        for t in turns:
            t._take(codes[t.slot].unsqueeze(0))
        return sum(codes[t.slot].shape[1] for t in turns)

    @torch.inference_mode()
    def end_heard(self, ended) -> None:
        """``ended`` = [(turn, text), ...]: heard turns of this server that end together.  Each enters its conversation as
        ``turn.end(text)`` would - under ``add``'s rules - but what is left to encode, the zero-padded last partial frames
        included, goes through ONE batched drain.  All turns are checked (and their texts tokenised) before anything is
        encoded or entered: when one is refused the call raises and none has changed."""
        self._check()
        ended = list(ended)
        texts = []
        for i, (turn, text) in enumerate(ended):
            if not isinstance(turn, SlotHeardTurn) or turn._srv is not self:
                raise ValueError("end_heard: not a heard turn of this server (turns of hear_slots = 0 servers and of Generator."
                                 "conversation() end through turn.end())")
            if any(turn is t for t, _ in ended[:i]):
                raise ValueError("end_heard: a turn is named twice")
            turn._check("end")
            turn._conv._before_history("end")                       # (a ServedConversation's only checks: nothing to undo)
            texts.append(self._gen._tokenize_text_segment(text, turn.speaker))
        if not ended:
            return
        slots = [turn.slot for turn, _ in ended]
        self._resample_heard([turn for turn, _ in ended], final=True)
        codes = self._hear.drain(slots, flush=slots)
        for (turn, _), (tt, tm) in zip(ended, texts):
            turn._take(codes[turn.slot].unsqueeze(0))
            self._free_heard(turn)
            turn._enter(tt, tm)

    # ---------------------------------------------------------------------------------------------------------------- step
    def _frame(self, rows):
        """One decode frame for ``rows`` (slot indices); the others idle on zero tokens.  Returns [slots, K]."""
        st = self._state
        st.set_active(rows)
        live = st.active.view(self.slots, 1, 1)
        out = st.serve_frame(self._tok * live, self._mask, *self._sample_args())
        self._tok[:, 0, :self._K] = torch.where(live[:, 0].bool(), out.long(), self._tok[:, 0, :self._K])
        for b in rows:
            self._rows[b]._sampled += 1
        if self.sample_stats:
            self._fstats.append(st.frame_stats())        # (a device copy: the chunk's look reads it)
        return out

    def _set_rows(self, rows, params, joined=False):
        """``params`` (one value per ``PARAMS`` record) to the slots ``rows`` through the state's writer of the server's level -
        after the writers below it for what it does not bring itself (the filters come after the pair); ``joined``: the rows start
        an utterance - where the level keeps rings, their frame counters return to 0."""
        own = LEVELS[self.level].writes
        for n in [n for n in range(1, self.level) if not set(LEVELS[n].writes) <= set(own)] + [self.level] * bool(own):
            for b in rows:
                getattr(self._state, "set_" + LEVELS[n].flag)(b, *[params[j] for j in LEVELS[n].writes])
        if joined and LEVELS[self.level].rings:
            for b in rows:
                self._state.reset_row_history(b)

    def _admit(self, queue=None):
        """Queued requests into free slots: plain requests and first turns are prefilled one by one, the turns of conversations
        with a parked cache are resumed, the requests with a voice are forked by ONE ``fork_rows``, and those two kinds are fed
        by ONE ``append_rows``, then one frame tail for all of them.  Returns (their slots, [slots, K]).  ``queue``: the requests
        to admit, when the schedule of a ``streams`` server has chosen them (it leaves them a free slot each)."""
        st, joined, resumed, forked, hs = self._state, [], [], [], {}
        queue = self._queue if queue is None else queue
        for b in range(self.slots):
            if not queue:
                break
            if self._rows[b] is not None:
                continue
            req = queue.popleft()
            conv = req._conv
            st.set_row_adapter(b, self._bank[req.adapter] if req.adapter is not None else None)
            # (every joining row, resumed turns included: with rings, a turn's window covers its own frames)
            self._set_rows((b,), [getattr(req, name) for name in NAMES], joined=True)
            if conv is not None and conv.seed is not None:
                if conv._noise is None:
                    conv._noise = st.new_row_generator(conv.seed)
                st.set_row_seed(b, None, generator=conv._noise)
            else:
                st.set_row_seed(b, req.seed)
            if conv is not None and conv._parked is not None:
                st.resume_row(b, conv._parked)
                conv._parked = None
                resumed.append(b)
            elif req._voice is not None:
                forked.append(b)
                resumed.append(b)
            else:
                hs[b] = st.prefill_row(b, req._tokens, req._mask)
            if conv is not None:
                conv._cached = req._base
            # its codec / resampler slot: the decode slot - or, with ``streams``, the lowest one nobody holds, kept to its end
            c = req._cslot = b if self.streams is None else self._cfree.pop(0)
            self._codec.open(c)
            if self._out is not None:
                self._out.open(c)
            req.slot, self._rows[b] = b, req
            req.slots_held.append(b)
            if self.streams is not None:
                self._flight.append(req)
            joined.append(b)
        if not joined:
            return joined, None
        if forked:
            st.fork_rows(forked, [self._rows[b]._voice.kv for b in forked])
        if resumed:
            h = st.append_rows(resumed, [self._rows[b]._tokens for b in resumed], [self._rows[b]._mask for b in resumed])
            hs.update({b: h[j] for j, b in enumerate(resumed)})
        for b, h in hs.items():
            if self._last_h is None:
                self._last_h = torch.zeros(self.slots, h.shape[-1], dtype=h.dtype, device=h.device)
            self._last_h[b] = h
        first = st.serve_first(self._last_h, joined, *self._sample_args())
        if self.sample_stats:
            # the chunk's first frame: the joined rows' columns over what the running rows' frame left (or alone)
            fs = st.frame_stats()
            if self._fstats:
                fs[:, :, [b for b in range(self.slots) if b not in joined]] = self._fstats[0][:, :, [b for b in range(self.slots) if b not in joined]]
                self._fstats[0] = fs
            else:
                self._fstats.append(fs)
        for b in joined:
            self._tok[b, 0, :self._K] = first[b]
            self._rows[b]._sampled = 1
        return joined, first

    @torch.inference_mode()
    def step(self) -> List[Tuple[Request, torch.Tensor, bool]]:
        """One chunk: ``(request, audio_chunk, done)`` for every request that held a slot in it (a request's last chunk may be
        shorter than ``chunk_frames * 1920`` samples, or empty when its first frame of the chunk was EOS)."""
        self._check()
        if self.hear_slots:
            self.hear_step()
        n, K = self.chunk_frames, self._K
        self.stats["steps"] += 1
        fresh = None
        if self.streams is not None:
            fresh = self._schedule()
            if fresh is None:                            # nobody is a candidate: nothing runs, nothing is moved
                self.last_join_rows = 0
                return []
        running = [b for b in range(self.slots) if self._rows[b] is not None]
        self._fstats = []                                # statistics mode: one [3, K, slots] device tensor per frame of the chunk
        first = self._frame(running) if running else None
        joined, first_j = self._admit(fresh)
        self.last_join_rows = len(joined)
        if first is None and first_j is None:
            return []
        if first is None:
            first = first_j
        elif first_j is not None:
            jm = torch.zeros(self.slots, 1, dtype=torch.bool)
            jm[joined] = True
            first = torch.where(jm.to(first.device), first_j, first)
        frames = [first]
        held = running + joined
        for _ in range(n - 1):
            # (a conversation's row is never idled: an idle frame would overwrite position 1 of its history - module docstring)
            rows = [b for b in held if self._rows[b]._conv is not None or self._rows[b]._sampled < self._rows[b].max_audio_frames]
            frames.append(self._frame(rows) if rows else frames[-1])
            if self.sample_stats and not rows:
                self._fstats.append(self._fstats[-1])
        chunk = torch.stack(frames, 2).long()                                        # [slots, K, n]
        allz = (chunk == 0).all(dim=1).cpu()                                         # the chunk's one host look
        fstats = torch.stack(self._fstats, 1).cpu() if self.sample_stats else None   # [3, n, K, slots], with the same look
        keep, done = {}, {}
        for b in held:
            req = self._rows[b]
            valid = min(n, req.max_audio_frames - req._emitted)
            hit = allz[b, :valid].nonzero()
            keep[b] = int(hit[0]) if hit.numel() else valid
            done[b] = bool(hit.numel()) or req._emitted + keep[b] >= req.max_audio_frames
        heard = sorted(b for b in held if keep[b] > 0)
        cs = {b: self._rows[b]._cslot for b in held}                                 # decode slot -> codec / resampler slot
        audio = None
        if heard:
            # what a row sampled after its EOS frame, or idled out after its length limit, is junk: the decoder gets zeros there
            # (its output for those frames is cut below; the frames before them do not depend on it - the decoder is causal)
            live = torch.tensor([[j < keep[b] for j in range(n)] for b in heard], device=chunk.device)
            audio = self._codec.step([cs[b] for b in heard], chunk[heard] * live[:, None, :])
        spoken = {}
        if self._out is not None:
            # ONE rows launch: the rows that produced audio, plus a row that ended on an empty chunk and is still owed its lag;
            # a row that ends in this step ends its resampler stream with it
            rows = [b for b in sorted(held) if keep[b] > 0 or (done[b] and self._out.pos[cs[b]] > 0)]
            if rows:
                xs = [audio[heard.index(b), :keep[b] * (audio.shape[1] // n)] if keep[b] > 0 else None for b in rows]
                spoken = dict(zip(rows, self._out.step([cs[b] for b in rows], xs, final=[cs[b] for b in rows if done[b]])))
        out = []
        for b in sorted(held):
            req = self._rows[b]
            if b in spoken and keep[b] == 0:                         # (only the lag: no frames, no codes)
                part = spoken[b].clone()
                if part.numel():
                    req.chunks.append(part)
            elif keep[b] > 0:
                part = (spoken[b] if b in spoken else audio[heard.index(b), :keep[b] * (audio.shape[1] // n)]).clone()
                req.chunks.append(part)
                req._codes.append(chunk[b, :, :keep[b]].clone())
                if fstats is not None:
                    req.stats.extend(SampleStats(K, fstats[:, :keep[b], :, b].clone()))
                req._emitted += keep[b]
            else:
                part = torch.zeros(0, device=self._gen.device)
            if done[b]:
                if req._conv is not None:
                    req._conv._end_turn(req, self._state, b)
                req.done, req.slot, self._rows[b] = True, None, None
                self._state.set_row_seed(b, None)
                if self.streams is not None:
                    self._leave(req)
            out.append((req, part, done[b]))
        if self.max_lead_ms is not None:
            # a listener's clock starts when this step hands over its first chunk
            now = self._clock()
            for req, _, _ in out:
                if req._t0 is None and req._emitted:
                    req._t0 = now
        return out

    def run(self) -> Iterator[Tuple[Request, torch.Tensor, bool]]:
        """``step()`` until the queue is drained and every slot is free, yielding each ``(request, audio_chunk, done)``.  A
        ``streams`` server sleeps ``next_due()`` (through ``sleep``) while everybody is far enough ahead of their listener, and
        returns when nothing is queued or runnable - paused requests are left as they are."""
        if self.streams is not None:
            while True:
                due = self.next_due()
                if due is None:
                    return
                if due > 0:
                    self._sleep(due)
                    continue
                for item in self.step():
                    yield item
        while self._queue or any(r is not None for r in self._rows):
            for item in self.step():
                yield item

    # ------------------------------------------------------------------------------------- more streams than slots: the schedule
    @property
    def in_flight(self) -> List[Request]:
        """The requests admitted and not done (running, parked or paused), in admission order - a ``streams`` server's."""
        return list(self._flight)

    def _lead(self, req, now):
        """Milliseconds of audio the request's listener has ahead: what was emitted, less - under pacing, once the first chunk
        was delivered - the time the listener has been listening."""
        ms = req._emitted * FRAME_MS
        return ms if now is None or req._t0 is None else ms - (now - req._t0) * 1000.0

    def _candidates(self, now):
        """(the in-flight requests that may run now, each as (lead, id, request); the queued requests that may join, in FIFO
        order): neither paused ones nor - under pacing - those at or over ``max_lead_ms``; joiners only while fewer than
        ``streams`` are in flight, paused ones included."""
        flying = [(self._lead(r, now), r.id, r) for r in self._flight if not r._paused]
        if self.max_lead_ms is not None:
            flying = [c for c in flying if c[0] < self.max_lead_ms]
        room = self.streams - len(self._flight)
        return flying, [r for r in self._queue if not r._paused][:max(room, 0)]

    def _schedule(self):
        """The start of a ``streams`` server's step: the ``slots`` candidates with the least (lead, id) get the slots.  Rows
        that were not chosen leave by ONE ``park_rows``; chosen requests without a slot return by ONE ``resume_rows``, lowest
        free slot first; a chosen request that holds a slot stays there.  Returns the chosen queued requests (for ``_admit``),
        taken off the queue - or None when nobody is a candidate (nothing was touched)."""
        flying, new = self._candidates(self._clock() if self.max_lead_ms is not None else None)
        cands = sorted([(float("-inf"), r.id, r) for r in new] + flying, key=lambda c: c[:2])[:self.slots]
        if not cands:
            return None
        chosen = [c[2] for c in cands]
        out = [b for b in range(self.slots) if self._rows[b] is not None and all(self._rows[b] is not r for r in chosen)]
        if out:
            self._park(out)
        back = [r for r in chosen if r.slot is None and r._row is not None]
        if back:
            self._resume(back)
        fresh = deque(r for r in chosen if r.slot is None)
        for r in fresh:
            self._queue.remove(r)
        return fresh

    def _park(self, slots):
        """The requests in ``slots`` leave their rows in the middle of their utterances: ONE ``DecodeState.park_rows`` (K / V,
        rings, generators) and one gather of their last sampled frames.  Their codec state stays where it is."""
        parked = self._state.park_rows(slots)
        toks = self._tok[slots]                          # (a gather: a copy of its own)
        for j, b in enumerate(slots):
            req = self._rows[b]
            req._row, req._tokrow, req.slot, self._rows[b] = parked[j], toks[j], None, None
            req.preemptions += 1
        self.stats["parks"] += len(slots)
        self.stats["park_launches"] += 1

    def _resume(self, reqs):
        """Parked requests into the free slots, lowest first: ONE ``DecodeState.resume_rows``, one scatter of their last sampled
        frames, and each row's adapter and sampling parameters (the ring counters are restored, not reset)."""
        free = [b for b in range(self.slots) if self._rows[b] is None][:len(reqs)]
        self._state.resume_rows(free, [r._row for r in reqs])
        self._tok[free] = torch.stack([r._tokrow for r in reqs])
        for b, req in zip(free, reqs):
            self._state.set_row_adapter(b, self._bank[req.adapter] if req.adapter is not None else None)
            self._set_rows((b,), [getattr(req, name) for name in NAMES])
            req._row, req._tokrow, req.slot, self._rows[b] = None, None, b, req
            req.slots_held.append(b)
        self.stats["resumes"] += len(reqs)
        self.stats["resume_launches"] += 1

    def _leave(self, req):
        """A request of a ``streams`` server has ended: it is no longer in flight and its codec slot is free."""
        import bisect
        self._flight.remove(req)
        bisect.insort(self._cfree, req._cslot)

    def next_due(self) -> Optional[float]:
        """Seconds until ``step()`` has somebody to run: 0.0 if it has now; None if nothing is in flight or queued, or all are
        paused; else - under ``max_lead_ms`` - until the first listener's lead is back under the bound, never less than a
        millisecond (at the exact instant a lead reaches the bound it is not yet below it)."""
        self._check()
        if self.streams is None:
            return 0.0 if self._queue or any(r is not None for r in self._rows) else None
        now = self._clock() if self.max_lead_ms is not None else None
        flying, new = self._candidates(now)
        if flying or new:
            return 0.0
        waits = [self._lead(r, now) - self.max_lead_ms for r in self._flight if not r._paused] if now is not None else []
        return max(min(waits) / 1000.0, MIN_SLEEP) if waits else None

    def _pause(self, req, paused):
        self._check()
        if self.streams is None:
            raise RuntimeError("pause() / resume() need a server made with serve(streams=): this server's requests hold their slot "
                               "from admission to their end")
        if not req.done:
            req._paused = bool(paused)

    @torch.inference_mode()
    def cancel(self, req: Request, heard_frames: Optional[int] = None) -> None:
        """End ``req`` now, wherever it is - queued, running, parked or paused (nothing happens to a done one).  A plain request
        is dropped.  A conversation's turn ends the way a length limit ends it, with ``min(heard_frames, emitted)`` frames kept
        (None: all emitted) - barge-in: the history and the parked cache hold the text and exactly the frames the listener
        heard, and the next ``say`` works.  Only the history and the cache are those of the heard frames: a seeded conversation's
        noise generator is not rewound - it stands after every frame the turn sampled - so the next turn has the codes of a turn
        that was given ``heard_frames`` frames only where that turn sampled as many frames.  The request is ``done`` with ``cancelled = True``; its slot, codec slot and resampler
        slot are free (the resampler's lag is not flushed)."""
        self._check()
        if req._srv is not self:
            raise ValueError("cancel: not a request of this server")
        if heard_frames is not None and (isinstance(heard_frames, bool) or int(heard_frames) != heard_frames or heard_frames < 0):
            raise ValueError(f"heard_frames must be an integer >= 0 (None: every frame emitted), got {heard_frames!r}")
        if req.done:
            return
        if req.stats is not None and heard_frames is not None:
            req.stats.cut(heard_frames)
        b = req.slot
        if b is None and req._row is None:
            self._queue.remove(req)
        if req._conv is not None:
            req._conv._end_turn(req, self._state, b, req._emitted if heard_frames is None else heard_frames)
        if b is not None:
            self._rows[b], req.slot = None, None
            self._state.set_row_seed(b, None)
        if req._cslot is not None:
            if self._out is not None:
                self._out.close(req._cslot)
            if self.streams is not None:
                self._leave(req)
        req._row, req._tokrow, req._paused = None, None, False
        req.done = req.cancelled = True
