"""Voices, host side: a voice prompt prefilled once and forked into requests, conversations and slots - the bookkeeping of
csm/conversation.py, csm/generator.py and csm/serving.py against the stub state, codec and tokenizer of
tests/test_serve_conversation_cpu.py (a row's cache is the list of frames fed to it, so a voice's ``kv`` is its frames), the
--serve-file --cache-context line handling, and the new library export."""
import os
import re
import types

import pytest
import torch

from test_serve_conversation_cpu import K, LONG, MAX_SEQ, SPF, ConvState, RowsCodec, State, StubModel, Tok, _run, _seg


class ForkState(State):
    """The served stub with a logging ``fork_rows``: every row gets a copy of its parked frames."""

    def fork_rows(self, rows, parkeds):
        assert len(rows) == len(set(rows)) == len(parkeds)
        for b, parked in zip(rows, parkeds):
            self.cache[b] = parked.clone()
        self.log.append(("fork_rows", tuple(rows), tuple(p.shape[0] for p in parkeds)))


class VoiceConvState(ConvState):
    """The one-row stub with ``park_row`` / ``resume_row``: what ``Generator.voice`` and a voice's conversation use."""
    made = []

    def __init__(self, engine, B, adapters=None):
        super().__init__(engine, B, adapters)
        self.adapters, self.log = adapters, []
        VoiceConvState.made.append(self)

    def prefill(self, tokens, masks):
        self.log.append(("prefill", tokens.shape[1]))
        return super().prefill(tokens, masks)

    def append(self, tokens, masks):
        self.log.append(("append", tokens.shape[0]))
        return super().append(tokens, masks)

    def park_row(self, b, length):
        assert b == 0 and 1 <= length <= self.cur + 1
        return torch.cat(self.fed, 0)[:length].clone()

    def resume_row(self, b, parked):
        self.log.append(("resume", parked.shape[0]))
        self.cur, self.fed = parked.shape[0] - 1, [parked.clone()]


@pytest.fixture
def world(monkeypatch):
    import csm.conversation as C
    import csm.serving as S
    from csm.generator import Generator
    monkeypatch.setattr(S, "DecodeState", ForkState)
    monkeypatch.setattr(C, "DecodeState", VoiceConvState)
    State.made, State.scripts, VoiceConvState.made = [], {}, []

    def _gen(conv_script=(), bank=()):
        gen = Generator(StubModel(conv_script), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
        if bank:
            entries = {name: object() for name in bank}

            def resolve(names):
                for n in names:
                    if n is not None and n not in entries:
                        raise ValueError(f"unknown LoRA adapter {n!r} (loaded: {list(entries)})")
                return [None if n is None else entries[n] for n in names]
            gen._bank = types.SimpleNamespace(entries=entries, names=list(entries), resolve=resolve)
        return gen

    def _serve(gen, scripts, **kw):
        State.scripts = scripts
        srv = gen.serve(**kw)
        st = State.made[-1]
        st.holders = lambda: {b for b, r in enumerate(srv._rows) if r is not None and r._conv is not None}
        return srv, st
    return _gen, _serve


VOICE = [(3, "yo", 1), (2, "hey", 0)]


def _voice_ctx():
    return [_seg(*s) for s in VOICE]


# ----------------------------------------------------------------------------------------------------------------- exports
def test_library_exports_kv_fork_rows():
    from csm import hip
    from csm.engine import DecodeState
    from csm.hip import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "csm_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+csm_kv_fork_rows\s*\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 12 == len(hip._SIGS["csm_kv_fork_rows"][0])
    assert "csm_kv_fork_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_kv_fork_rows") and callable(ops.kv_fork_rows)
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    assert callable(DecodeState.fork_rows)


# ------------------------------------------------------------------------------------------------------------------- voice
def test_voice_holds_the_context_prefilled_once(world):
    _gen, _ = world
    gen = _gen()
    v = gen.voice(_voice_ctx())
    parts = [gen._tokenize_segment(s) for s in _voice_ctx()]
    assert torch.equal(v.tokens, torch.cat([t for t, _ in parts], 0)) and torch.equal(v.mask, torch.cat([m for _, m in parts], 0))
    assert v.tokens.shape[1] == K + 1 and v.turns == tuple(t.shape[0] for t, _ in parts)
    assert v.positions == v.tokens.shape[0] == v.kv.shape[0] and v.adapter is None
    assert v.nbytes == v.kv.numel() * v.kv.element_size()
    assert len(VoiceConvState.made) == 1 and VoiceConvState.made[0].log == [("prefill", v.positions)]


def test_voice_refusals(world):
    _gen, _serve = world
    gen, other = _gen(bank=("a1",)), _gen(bank=("a1",))
    with pytest.raises(ValueError, match="empty context"):
        gen.voice([])
    with pytest.raises(ValueError, match="Inputs too long"):
        gen.voice([_seg(MAX_SEQ)])
    with pytest.raises(ValueError, match="unknown LoRA adapter 'nope'"):
        gen.voice(_voice_ctx(), adapter="nope")
    gen._model.use_kv_cache = False
    with pytest.raises(ValueError, match="use_kv_cache"):
        gen.voice(_voice_ctx())
    gen._model.use_kv_cache = True
    gen._model.lora = types.SimpleNamespace(merged=False)
    with pytest.raises(ValueError, match="un-merged"):
        gen.voice(_voice_ctx())
    gen._model.lora = types.SimpleNamespace(merged=True)
    v, v1 = gen.voice(_voice_ctx()), gen.voice(_voice_ctx(), adapter="a1")
    assert v1.adapter == "a1" and VoiceConvState.made[-1].adapters is not None
    # a voice of another generator; an adapter that is not the voice's - on every entry point, at the call
    srv, st = _serve(gen, {0: [LONG]}, slots=2)
    foreign = other.voice(_voice_ctx())
    for call in (lambda vv, **kw: gen.conversation(voice=vv, **kw), lambda vv, **kw: gen.generate("hi", 0, [], voice=vv, **kw),
                 lambda vv, **kw: gen.generate_stream("hi", 0, [], voice=vv, **kw),
                 lambda vv, **kw: srv.submit("hi", 0, [], voice=vv, **kw), lambda vv, **kw: srv.conversation(voice=vv, **kw)):
        with pytest.raises(ValueError, match="another Generator"):
            call(foreign)
        with pytest.raises(ValueError, match="adapter 'a1' with a voice that was prefilled with adapter None"):
            call(v, adapter="a1")
        with pytest.raises(ValueError, match="adapter 'a2' with a voice"):
            call(v1, adapter="a2")
    assert srv.queued == 0
    assert srv.submit("hi", 0, [], voice=v1, max_audio_length_ms=8 * 80).adapter == "a1" and srv.conversation(voice=v1, adapter="a1").adapter == "a1"
    # the adapter must be bound by this server: a1x joined the bank after serve()
    gen._bank.entries["a1x"] = object()
    vx = gen.voice(_voice_ctx(), adapter="a1x")
    with pytest.raises(ValueError, match="unknown LoRA adapter 'a1x'"):
        srv.submit("hi", 0, [], voice=vx)
    with pytest.raises(ValueError, match="unknown LoRA adapter 'a1x'"):
        srv.conversation(voice=vx)


# --------------------------------------------------------------------------------------------------------------- admission
def test_admission_forks_all_voice_requests_in_one_launch(world):
    """3 voice requests, 1 resumed turn and 1 plain request at one boundary: one prefill_row, one resume_row, one fork_rows with
    3 rows, one append_rows with 4 rows, one serve_first."""
    _gen, _serve = world
    gen = _gen()
    v = gen.voice(_voice_ctx())
    kv0 = v.kv.clone()
    srv, st = _serve(gen, {0: [[1, 2, 3, 0], LONG], 1: [LONG], 2: [LONG], 3: [LONG], 4: [LONG]}, slots=6, chunk_frames=4)
    conv = srv.conversation()
    conv.say("a", 0, max_audio_length_ms=30 * 80)
    srv.step()
    assert conv._parked is not None and srv.active == []
    del st.log[:]
    reqs = [srv.submit("x", 1, [], voice=v, max_audio_length_ms=30 * 80)]
    turn = conv.say("b", 0, max_audio_length_ms=30 * 80)
    reqs.append(srv.submit("y", 2, [_seg(1, "mid", 2)], voice=v, max_audio_length_ms=30 * 80))
    plain = srv.submit("p", 3, [_seg(1)], max_audio_length_ms=30 * 80)
    reqs.append(srv.submit("z", 4, [], voice=v, max_audio_length_ms=30 * 80))
    # only context + text were tokenised at the call: the request carries that feed and the voice
    assert torch.equal(reqs[0]._tokens, gen._tokenize_text_segment("x", 1)[0]) and reqs[0]._voice is v
    assert torch.equal(reqs[1]._tokens, torch.cat([gen._tokenize_segment(_seg(1, "mid", 2))[0], gen._tokenize_text_segment("y", 2)[0]]))
    cached = conv.cached
    srv.step()
    n_first = [e[0] for e in st.log].index("first")
    L = v.positions
    assert st.log[:n_first + 1] == [
        ("resume", 1, cached), ("prefill", 3, plain._tokens.shape[0]), ("fork_rows", (0, 2, 4), (L, L, L)),
        ("append_rows", (0, 1, 2, 4), (reqs[0]._tokens.shape[0], turn._tokens.shape[0], reqs[1]._tokens.shape[0],
                                       reqs[2]._tokens.shape[0])),
        ("first", (0, 1, 2, 3, 4))]
    assert [r.slot for r in reqs] == [0, 2, 4] and (turn.slot, plain.slot) == (1, 3)
    # each forked row holds the voice, then its own feed, then what it sampled
    for r in reqs:
        assert torch.equal(st.cache[r.slot][:L + r._tokens.shape[0]], torch.cat([v.tokens, r._tokens]))
    _run(srv)
    assert all(r.done for r in reqs) and torch.equal(v.kv, kv0)


def test_voice_none_never_forks(world):
    _gen, _serve = world
    gen = _gen(conv_script=[5, 6, 0, 9])
    srv, st = _serve(gen, {0: [[1, 2, 3, 0], [4, 5, 0, 9]], 1: [LONG]}, slots=3, chunk_frames=4)
    conv = srv.conversation(context=[_seg(2)])
    conv.say("a", 0, max_audio_length_ms=30 * 80)
    srv.submit("x", 1, [_seg(1)], max_audio_length_ms=8 * 80)
    _run(srv)
    conv.say("b", 0, max_audio_length_ms=30 * 80)
    _run(srv)
    assert {"prefill", "resume", "append_rows"} <= {e[0] for e in st.log} and not any(e[0] == "fork_rows" for e in st.log)
    gen.conversation(context=[_seg(2)]).generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    assert [e[0] for e in VoiceConvState.made[-1].log] == ["prefill"]


# ------------------------------------------------------------------------------------------------------------ length rule
def test_length_rule_counts_the_voice_at_the_call(world):
    _gen, _serve = world
    gen = _gen()
    v = gen.voice(_voice_ctx())
    srv, st = _serve(gen, {0: [LONG]}, slots=2, chunk_frames=4)
    L, T = v.positions, gen._tokenize_text_segment("hello", 0)[0].shape[0]
    # a request fits with L + T < MAX_SEQ - max_audio_frames
    with pytest.raises(ValueError, match=rf"Inputs too long, must be below max_seq_len - max_audio_frames: {L + T}$"):
        srv.submit("hello", 0, [], voice=v, max_audio_length_ms=(MAX_SEQ - L - T) * 80)
    assert srv.queued == 0
    srv.submit("hello", 0, [], max_audio_length_ms=(MAX_SEQ - L - T) * 80)         # (the same call without the voice fits)
    srv.submit("hello", 0, [], voice=v, max_audio_length_ms=(MAX_SEQ - L - T - 1) * 80)
    S = gen._tokenize_segment(_seg(1))[0].shape[0]
    with pytest.raises(ValueError, match="Inputs too long"):
        srv.submit("hello", 0, [_seg(1)], voice=v, max_audio_length_ms=(MAX_SEQ - L - T - S) * 80)
    srv.submit("hello", 0, [_seg(1)], voice=v, max_audio_length_ms=(MAX_SEQ - L - T - S - 1) * 80)
    assert srv.queued == 3
    # a conversation's turn: the voice is history, and the row samples to its chunk's end (chunk_frames - 1 more positions)
    conv = srv.conversation(voice=v)
    with pytest.raises(ValueError, match="Inputs too long"):
        conv.say("hello", 0, max_audio_length_ms=(MAX_SEQ - L - T - 3) * 80)
    assert conv.tokens.shape[0] == L and conv._open is None and srv.queued == 3
    conv.say("hello", 0, max_audio_length_ms=(MAX_SEQ - L - T - 4) * 80)
    one = gen.conversation(voice=v)
    with pytest.raises(ValueError, match="Inputs too long"):
        one.generate("hello", 0, max_audio_length_ms=(MAX_SEQ - L - T) * 80)


# ---------------------------------------------------------------------------------------------------------------- history
def test_served_conversation_starts_as_the_voice(world):
    _gen, _serve = world
    gen = _gen()
    v = gen.voice(_voice_ctx())
    kv0 = v.kv.clone()
    srv, st = _serve(gen, {0: [[1, 2, 3, 0] + [9] * 8]}, slots=2, chunk_frames=4)
    L = v.positions
    conv = srv.conversation(voice=v, context=[_seg(1, "then", 1)], keep_turns=2, on_overflow="drop_oldest")
    extra = gen._tokenize_segment(_seg(1, "then", 1))
    assert torch.equal(conv.tokens, torch.cat([v.tokens, extra[0]])) and torch.equal(conv.mask, torch.cat([v.mask, extra[1]]))
    assert conv._turns == list(v.turns) + [extra[0].shape[0]] and conv.cached == L and conv._parked is v.kv
    r = conv.say("one", 0, max_audio_length_ms=8 * 80)
    # its first say is a resumed turn: what follows the voice and the text are the feed
    assert torch.equal(r._tokens, torch.cat([extra[0], gen._tokenize_text_segment("one", 0)[0]]))
    srv.step()
    assert st.log[:3] == [("resume", 0, L), ("append_rows", (0,), (r._tokens.shape[0],)), ("first", (0,))]
    assert not any(e[0] in ("prefill", "fork_rows") for e in st.log)
    assert r.done and conv._parked is not v.kv and torch.equal(conv._parked, conv.tokens[:conv.cached])
    # keep_turns over the voice's turns: an overflow drops what came after them, the voice stays and is prefilled again
    before = conv.tokens.clone()
    conv.say("two", 0, max_audio_length_ms=(MAX_SEQ - before.shape[0]) * 80)
    assert torch.equal(conv.tokens, torch.cat([before[:L], gen._tokenize_text_segment("two", 0)[0]]))
    assert conv._turns[:2] == list(v.turns) and conv.cached == 0 and conv._parked is None
    del st.log[:]
    srv.step()
    assert st.log[0] == ("prefill", 0, conv._open._tokens.shape[0]) and st.log[0][2] == L + gen._tokenize_text_segment("two", 0)[0].shape[0]
    assert torch.equal(v.kv, kv0)


def test_one_row_conversation_starts_as_the_voice(world):
    _gen, _ = world
    turn1, turn2 = [5, 6, 7, 0, 9, 9, 9, 9], [11, 12, 0, 9]
    gen = _gen(conv_script=turn1[:4] + turn2)
    v = gen.voice(_voice_ctx())
    kv0 = v.kv.clone()
    L = v.positions
    conv = gen.conversation(voice=v, context=[_seg(1, "then", 1)], keep_turns=2)
    extra = gen._tokenize_segment(_seg(1, "then", 1))[0]
    assert torch.equal(conv.tokens, torch.cat([v.tokens, extra])) and conv.mask.shape == conv.tokens.shape
    assert conv._turns == list(v.turns) + [extra.shape[0]] and conv.cached == L and conv._state is None
    conv.generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    st = VoiceConvState.made[-1]
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert st.log == [("resume", L), ("append", extra.shape[0] + T)]                 # the voice is copied in, never prefilled
    assert torch.equal(torch.cat(st.fed, 0)[:L], v.tokens) and conv.cached == L + extra.shape[0] + T + 3
    # reset(): the history - the voice's frames included - is prefilled again from its tokens
    hist = conv.tokens.shape[0]
    conv.reset()
    assert conv.cached == 0 and conv._state is None
    conv.generate("more", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    assert VoiceConvState.made[-1] is not st
    assert VoiceConvState.made[-1].log == [("prefill", hist + gen._tokenize_text_segment("more", 0)[0].shape[0])]
    assert torch.equal(v.kv, kv0)


def test_generate_with_a_voice_is_the_conversation_call(world):
    _gen, _ = world
    script = [5, 6, 7, 0]
    gen = _gen(conv_script=script * 3)
    v = gen.voice(_voice_ctx())
    ref = gen.conversation(voice=v, context=[_seg(1)]).generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    ref_log = VoiceConvState.made[-1].log
    out = gen.generate("hi", 0, [_seg(1)], max_audio_length_ms=20 * 80, eos_check_every=4, voice=v)
    assert torch.equal(out, ref) and out.numel() == 3 * SPF and VoiceConvState.made[-1].log == ref_log
    assert ref_log[0] == ("resume", v.positions) and ref_log[1][0] == "append"
    chunks = list(gen.generate_stream("hi", 0, [_seg(1)], max_audio_length_ms=20 * 80, chunk_frames=4, voice=v))
    assert torch.equal(torch.cat(chunks), ref) and VoiceConvState.made[-1].log == ref_log


# -------------------------------------------------------------------------------------------------------------------- CLI
def test_serve_file_cache_context(tmp_path):
    """``--serve-file --cache-context`` against a recording generator: one voice per distinct adapter, made before ``serve``;
    every line and every conversation gets its voice and no context."""
    from csm.cli import generate as G
    calls = []

    class Srv:
        queued, active = 0, []

        def submit(self, text, speaker, context, **kw):
            calls.append(("submit", text, context, kw.get("voice"), kw["adapter"]))
            return object()

        def conversation(self, **kw):
            calls.append(("conversation", kw["context"], kw.get("voice"), kw["adapter"]))
            return types.SimpleNamespace(say=lambda text, speaker, **kw: calls.append(("say", text)) or object())

    gen = types.SimpleNamespace(sample_rate=24000, load_adapter=lambda name, path: calls.append(("load", name)),
                                voice=lambda context, adapter=None: calls.append(("voice", context, adapter)) or ("V", adapter),
                                serve=lambda **kw: calls.append(("serve",)) or Srv())
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav")]
    ctx = ["--context-audio", "a.wav", "--context-text", "hello", "--context-speaker", "1"]
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one"}\n{"text": "two", "adapter": "b.st"}\n{"text": "three", "conversation": "c"}\n'
                 '{"text": "four", "adapter": "b.st", "conversation": "d"}\n{"text": "five"}\n')
    context = ["SEGMENT"]
    G.serve_to_wavs(gen, G.parse_args(base + ctx + ["--serve-file", str(p), "--cache-context"]), context, adapter="cli")
    assert calls == [("load", "b.st"), ("voice", context, "b.st"), ("voice", context, "cli"), ("serve",),
                     ("submit", "one", [], ("V", "cli"), "cli"), ("submit", "two", [], ("V", "b.st"), "b.st"),
                     ("conversation", [], ("V", "cli"), "cli"), ("say", "three"),
                     ("conversation", [], ("V", "b.st"), "b.st"), ("say", "four"), ("submit", "five", [], ("V", "cli"), "cli")]
    del calls[:]
    G.serve_to_wavs(gen, G.parse_args(base + ctx + ["--serve-file", str(p)]), context)
    assert not any(c[0] == "voice" for c in calls)
    assert ("submit", "one", context, None, None) in calls and ("conversation", context, None, None) in calls
    assert G.line_prompt({"adapter": None}, context, None) == {"context": context}
    assert G.serve_voices(gen, [{"adapter": None}], context) == {None: ("V", None)}
    for bad in (base + ["--text", "x", "--cache-context"], base + ["--serve-file", str(p), "--cache-context"]):
        with pytest.raises(SystemExit):
            G.parse_args(bad)
