"""Served conversations, host side: the history / park / resume bookkeeping of csm/serving.py against a stub decode state that
models each row's cache as the list of frames fed to it - an idled row loses position 1, as on the device - and the new library
exports."""
import os
import re
import types

import pytest
import torch

K = 4                       # codebooks of the stub model
MAX_SEQ = 96
SPF = 4                     # samples per frame of the stub codec
LONG = list(range(1, 90))


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


class RowsCodec:
    sample_rate = 24000

    def __init__(self):
        self.log = []

    def encode(self, audio):
        T = audio.shape[-1] // SPF
        return (torch.arange(K * T).reshape(1, K, T) % 7) + 1

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(SPF, -1)

    def decode_stream(self):
        return types.SimpleNamespace(step=self.decode)

    def decode_stream_rows(self, slots=16, max_chunk_frames=32):
        codec = self

        class Rows:
            def open(self, slot):
                codec.log.append(("open", slot))

            def step(self, rows, codes):
                codec.log.append(("step", tuple(rows), codes.shape[2]))
                return codes.float().sum(1).repeat_interleave(SPF, -1)
        return Rows()


def _speaker(tk):
    """The speaker of the LAST text segment of a feed ("[<speaker>]text" through Tok: BOS, '[', the digit)."""
    start = int((tk[:, K] == 1).nonzero()[-1])
    return int(tk[start + 2, K]) - 3 - ord("0")


class State:
    """What BatchServer uses of DecodeState.  ``cache[b]``: the frames row b's cache holds, position by position.  A row samples
    the script of the speaker of its latest feed; ``scripts[speaker]`` is a list of scripts, one per turn of that speaker."""
    scripts = {}
    made = []

    def __init__(self, engine, B, adapters=None, bank=None):
        self.B, self.bank, self.log = B, bank, []
        self.active_rows = list(range(B))
        self.active = torch.ones(B, dtype=torch.int32)
        self.script, self.at, self.adapter, self.gen = [None] * B, [0] * B, [None] * B, [None] * B
        self.cache = [torch.zeros(0, K + 1, dtype=torch.long) for _ in range(B)]
        self.turn = {}
        self.idled_while_held = []
        self.holders = lambda: set()
        State.made.append(self)

    def _start(self, b, tk):
        sp = _speaker(tk)
        t = self.turn.get(sp, 0)
        self.turn[sp] = t + 1
        scr = State.scripts[sp]
        self.script[b], self.at[b] = scr[t % len(scr)], 0

    def _next(self, rows):
        out = torch.full((self.B, K), 99, dtype=torch.int32)
        for b in rows:
            out[b] = self.script[b][self.at[b]]
            self.at[b] += 1
        return out

    def prefill_row(self, b, tk, mk):
        self.cache[b] = tk.clone().long()
        self._start(b, tk)
        self.log.append(("prefill", b, tk.shape[0]))
        return torch.zeros(8)

    def append_rows(self, rows, tokens_list, masks_list):
        assert len(rows) == len(set(rows)) == len(tokens_list) == len(masks_list)
        for b, tk in zip(rows, tokens_list):
            assert self.cache[b].shape[0] > 0
            self.cache[b] = torch.cat([self.cache[b], tk.long()], 0)
            self._start(b, tk)
        self.log.append(("append_rows", tuple(rows), tuple(t.shape[0] for t in tokens_list)))
        return torch.zeros(len(rows), 8)

    def park_row(self, b, length):
        assert 1 <= length <= self.cache[b].shape[0]
        self.log.append(("park", b, length))
        return self.cache[b][:length].clone()

    def resume_row(self, b, parked):
        self.cache[b] = parked.clone()
        self.log.append(("resume", b, parked.shape[0]))

    def set_row_adapter(self, b, state):
        self.adapter[b] = state

    def new_row_generator(self, seed):
        return ["generator", seed]

    def set_row_seed(self, b, seed, generator=None):
        self.gen[b] = generator if generator is not None else seed

    def set_active(self, rows):
        self.active_rows = sorted(rows)
        missing = self.holders() - set(rows)
        if missing:
            self.idled_while_held.append(sorted(missing))

    def serve_first(self, last_h, rows, temperature, topk):
        self.log.append(("first", tuple(rows)))
        return self._next(rows)

    def serve_frame(self, tokens, masks, temperature, topk):
        rows = self.active_rows
        for b in range(self.B):
            if b in rows:
                self.cache[b] = torch.cat([self.cache[b], tokens[b].long()], 0)
            else:                                   # the device pins an idle row to position 0 and writes a zero token at 1
                c = self.cache[b]
                self.cache[b] = torch.cat([c[:1], torch.zeros(1, K + 1, dtype=torch.long)], 0) if c.shape[0] else c
        self.log.append(("frame", tuple(rows)))
        return self._next(rows)


class ConvState:
    """The stub of tests/test_conversation_cpu.py: what Conversation uses of DecodeState."""

    def __init__(self, engine, B, adapters=None):
        self.cur, self.fed = -1, []

    def prefill(self, tokens, masks):
        self.cur = tokens.shape[1] - 1
        self.fed = [tokens[0].clone()]
        return torch.zeros(1, 8)

    def append(self, tokens, masks):
        self.fed.append(tokens.clone())
        self.cur += tokens.shape[0]
        return torch.zeros(1, 8)

    def truncate(self, length):
        self.cur = length - 1


class StubModel:
    device = torch.device("cpu")
    use_kv_cache = True

    def __init__(self, conv_script=()):
        self.args = types.SimpleNamespace(audio_num_codebooks=K)
        self.bb = types.SimpleNamespace(max_seq_len=MAX_SEQ)
        self.script, self.i = list(conv_script), 0
        self.engine = types.SimpleNamespace(_need=lambda: None, _frame_tail=lambda *a: self._sample())
        self._decode_state = None

    def _sample(self):
        v = self.script[self.i]
        self.i += 1
        return torch.full((1, K), v, dtype=torch.int32)

    def generate_frame(self, tokens, mask, pos, temperature, topk, **kw):
        self._decode_state.cur += 1
        return self._sample()

    def setup_caches(self, n):
        pass

    def reset_caches(self):
        self._decode_state = None


@pytest.fixture
def make(monkeypatch):
    import csm.conversation as C
    import csm.serving as S
    from csm.generator import Generator
    monkeypatch.setattr(S, "DecodeState", State)
    monkeypatch.setattr(C, "DecodeState", ConvState)
    State.made, State.scripts = [], {}

    def _make(scripts, conv_script=(), **kw):
        State.scripts = scripts
        codec = RowsCodec()
        gen = Generator(StubModel(conv_script), text_tokenizer=Tok(), audio_tokenizer=codec)
        srv = gen.serve(**kw)
        st = State.made[-1]
        st.holders = lambda: {b for b, r in enumerate(srv._rows) if r is not None and r._conv is not None}
        return gen, srv, st, codec
    return _make


def _seg(frames=3, text="yo", speaker=1):
    from csm.generator import Segment
    return Segment(speaker, text, torch.zeros(SPF * frames))


def _run(srv):
    for _ in srv.run():
        pass


def _audio(values):
    return torch.tensor([float(K * v) for v in values]).repeat_interleave(SPF)


# --------------------------------------------------------------------------------------------------------------- exports
def test_library_exports_rows_append_and_pinned_gemm():
    from csm import hip
    from csm.engine import DecodeState
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csm_hip.h")).read()
    for name in ("csm_attn_append_rows", "csm_gemm_bf16_pinned"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in hip.EXPORTS and hasattr(hip.lib, name), name
    assert callable(hip.ops.attn_append_rows)
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    for m in ("append_rows", "park_row", "resume_row", "new_row_generator"):
        assert callable(getattr(DecodeState, m)), m
    from csm.serving import BatchServer, ServedConversation
    assert callable(BatchServer.conversation) and callable(ServedConversation.say) and callable(ServedConversation.add)


# --------------------------------------------------------------------------------------------------------------- history
def test_history_layout_equals_conversation(make):
    """Spoken turn (EOS inside the chunk), added turn, spoken turn (length limit inside a chunk): tokens, mask and cached are
    what ``Conversation`` keeps for the same inputs and the same sampled frames (its host looks once per chunk of 4, too)."""
    turn1, turn2 = [5, 6, 7, 0, 9, 9, 9, 9], [11, 12, 13, 14, 15, 16, 17, 18]
    gen, srv, st, codec = make({0: [turn1, turn2]}, conv_script=turn1[:4] + turn2, slots=2, chunk_frames=4)
    ref = gen.conversation(context=[_seg(3)])
    ref.generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    ref.add(_seg(2, "and?", 1))
    ref.generate("more", 0, max_audio_length_ms=6 * 80, eos_check_every=4)
    ref.add(_seg(1, "ok", 1))                                            # (settles the second turn)

    conv = srv.conversation(context=[_seg(3)])
    assert conv.cached == 0 and torch.equal(conv.tokens, gen._tokenize_segment(_seg(3))[0])
    r1 = conv.say("hi", 0, max_audio_length_ms=20 * 80)
    _run(srv)
    assert r1.done and torch.equal(r1.audio(), _audio([5, 6, 7]))
    conv.add(_seg(2, "and?", 1))
    r2 = conv.say("more", 0, max_audio_length_ms=6 * 80)
    _run(srv)
    assert r2.done and torch.equal(r2.audio(), _audio(turn2[:6]))        # cut at the length limit
    conv.add(_seg(1, "ok", 1))
    assert torch.equal(conv.tokens, ref.tokens) and torch.equal(conv.mask, ref.mask)
    # ``cached`` means the same - leading history positions whose K / V are kept - but the served row sampled to its chunk's end
    # and so fed its sixth frame back, which Conversation (it stops at the length limit) leaves to the next turn
    assert conv.cached == ref.cached + 1 == conv.tokens.shape[0] - gen._tokenize_segment(_seg(1, "ok", 1))[0].shape[0] - 1
    assert conv._turns == ref._turns
    # the parked cache is exactly the first ``cached`` positions of the history: the frames sampled after EOS / after the
    # length limit (the row sampled 8 to the chunk's end) are not in it, and no idle frame has touched position 1
    assert torch.equal(conv._parked, conv.tokens[:conv.cached])
    assert st.idled_while_held == []


def test_second_say_while_open_raises_and_close(make):
    gen, srv, st, codec = make({0: [LONG]}, slots=2, chunk_frames=2)
    conv = srv.conversation()
    r = conv.say("a", 0, max_audio_length_ms=5 * 80)
    for call in (lambda: conv.say("b", 0), lambda: conv.add(_seg()), conv.close):
        with pytest.raises(RuntimeError, match="still open"):
            call()
    srv.step()
    with pytest.raises(RuntimeError, match="still open"):
        conv.say("b", 0)
    _run(srv)
    assert r.done and conv._parked is not None
    conv.close()
    assert conv._parked is None and conv.closed
    with pytest.raises(RuntimeError, match="closed"):
        conv.say("b", 0)
    with pytest.raises(ValueError, match="on_overflow"):
        srv.conversation(on_overflow="nope")
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        srv.conversation(adapter="nope")


def test_length_rule_counts_the_chunk_headroom(make):
    gen, srv, st, codec = make({0: [LONG]}, slots=2, chunk_frames=4)
    T = gen._tokenize_text_segment("hello", 0)[0].shape[0]
    conv = srv.conversation()
    # a plain request fits with max_audio_frames = MAX_SEQ - T - 1; a turn needs chunk_frames - 1 = 3 more positions
    srv.submit("hello", 0, [], max_audio_length_ms=(MAX_SEQ - T - 1) * 80)
    for frames in (MAX_SEQ - T - 1, MAX_SEQ - T - 3):
        with pytest.raises(ValueError, match=rf"Inputs too long, must be below max_seq_len - max_audio_frames: {MAX_SEQ - frames - 3}$"):
            conv.say("hello", 0, max_audio_length_ms=frames * 80)
    assert conv.tokens.shape[0] == 0 and conv._open is None and srv.queued == 1      # raised at say: nothing was queued
    conv.say("hello", 0, max_audio_length_ms=(MAX_SEQ - T - 4) * 80)
    with pytest.raises(ValueError):
        srv.conversation().say("hello", 0, max_audio_length_ms=10)


def test_drop_oldest_resets_cached_and_prefills(make):
    gen, srv, st, codec = make({0: [[1, 2, 3, 0] + [9] * 8]}, slots=2, chunk_frames=4)
    conv = srv.conversation(context=[_seg(20, "first", 1)], on_overflow="drop_oldest")
    strict = srv.conversation(context=[_seg(20, "first", 1)])
    conv.say("one", 0, max_audio_length_ms=8 * 80)
    _run(srv)
    assert conv.cached > 0 and conv._parked is not None
    before = conv.tokens.clone()
    first = conv._turns[0]
    big = (MAX_SEQ - before.shape[0]) * 80
    strict.say("one", 0, max_audio_length_ms=8 * 80)
    _run(srv)
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_audio_frames"):
        strict.say("two", 0, max_audio_length_ms=big)
    del st.log[:]
    r = conv.say("two", 0, max_audio_length_ms=big)
    assert conv.cached == 0 and conv._parked is None                      # the dropped prefix takes the cache with it
    T = gen._tokenize_text_segment("two", 0)[0].shape[0]
    assert torch.equal(conv.tokens, torch.cat([before[first:], gen._tokenize_text_segment("two", 0)[0]], 0))
    srv.step()
    assert st.log[0] == ("prefill", 0, before.shape[0] - first + T)       # from position 0, through prefill_row
    assert not any(e[0] in ("append_rows", "resume") for e in st.log)
    assert r.done and conv.cached == r._base + 3                           # (the turn ended inside its first chunk: 3 frames kept)


# ----------------------------------------------------------------------------------------------------------------- slots
def test_slot_released_at_turn_end_and_resumed_elsewhere(make):
    scripts = {0: [[1, 2, 0, 9], [4, 5, 6, 0]], 1: [LONG], 2: [LONG]}
    gen, srv, st, codec = make(scripts, slots=2, chunk_frames=4)
    conv = srv.conversation(seed=77)
    r1 = conv.say("a", 0, max_audio_length_ms=30 * 80)
    srv.step()
    assert r1.done and r1.slot is None and srv.active == []               # parked at the end of the chunk its turn ended in
    assert st.gen == [None, None] and conv._noise == ["generator", 77]
    assert ("park", 0, conv.cached) in st.log
    # more conversations than slots can be open: slot 0 goes to a plain request, the conversation resumes in slot 1
    p = srv.submit("x", 1, [], max_audio_length_ms=30 * 80)
    srv.step()
    assert p.slot == 0
    conv.add(_seg(2))
    r2 = conv.say("b", 0, max_audio_length_ms=30 * 80)
    cached = conv.cached
    del st.log[:]
    srv.step()
    assert st.log[:4] == [("frame", (0,)), ("resume", 1, cached), ("append_rows", (1,), (r2._tokens.shape[0],)), ("first", (1,))]
    assert r2.done and torch.equal(r2.audio(), _audio([4, 5, 6]))
    assert conv._noise == ["generator", 77]                               # one generator for its whole life, whatever the slot
    assert torch.equal(conv._parked, conv.tokens[:conv.cached])
    assert st.idled_while_held == []
    others = [srv.conversation() for _ in range(5)]                       # five open conversations on two slots
    reqs = [c.say("z", 2, max_audio_length_ms=2 * 80) for c in others]
    _run(srv)
    assert all(r.done for r in reqs) and all(c._parked is not None for c in others)


def test_admission_order_prefills_one_append_rows_one_first(make):
    scripts = {s: [[1, 2, 3, 0], LONG] for s in range(3)}
    scripts[3] = [LONG]
    gen, srv, st, codec = make(scripts, slots=6, chunk_frames=4)
    convs = [srv.conversation(seed=s) for s in range(3)]
    for s, c in enumerate(convs):
        c.say("a", s, max_audio_length_ms=30 * 80)
    srv.step()
    assert all(c._parked is not None for c in convs) and srv.active == []
    del st.log[:]
    # one boundary: a plain request, a first turn, and the three resumed turns
    second = [convs[0].say("b", 0, max_audio_length_ms=30 * 80)]
    plain = srv.submit("x", 3, [], max_audio_length_ms=30 * 80)
    second.append(convs[1].say("b", 1, max_audio_length_ms=30 * 80))
    fresh = srv.conversation()
    first_turn = fresh.say("n", 3, max_audio_length_ms=30 * 80)
    second.append(convs[2].say("b", 2, max_audio_length_ms=30 * 80))
    srv.step()
    kinds = [e[0] for e in st.log]
    n_first = kinds.index("first")
    assert kinds[:n_first].count("append_rows") == 1 and kinds.count("first") == 1
    ar = kinds.index("append_rows")
    assert all(k in ("prefill", "resume") for k in kinds[:ar]) and kinds[:ar].count("prefill") == 2 and ar == n_first - 1
    assert st.log[ar] == ("append_rows", (0, 2, 4), tuple(r._tokens.shape[0] for r in second))
    assert st.log[n_first] == ("first", (0, 1, 2, 3, 4))
    assert (plain.slot, first_turn.slot) == (1, 3)
    assert st.gen[:5] == [["generator", 0], None, ["generator", 1], None, ["generator", 2]]


def test_set_active_never_excludes_a_conversation_row(make):
    """A conversation's row at its length limit keeps sampling to the chunk's end where a plain request idles; the extra frames
    are cut from the audio and from the parked length."""
    gen, srv, st, codec = make({0: [LONG], 1: [LONG], 2: [LONG]}, slots=3, chunk_frames=4)
    conv = srv.conversation()
    rc = conv.say("c", 0, max_audio_length_ms=6 * 80)
    rp = srv.submit("p", 1, [], max_audio_length_ms=6 * 80)
    rl = srv.submit("l", 2, [], max_audio_length_ms=12 * 80)
    srv.step()
    base = rc._base
    srv.step()
    assert rc.done and rp.done and not rl.done
    # after the sixth frame the plain row idles, the conversation's row does not
    assert [e for e in st.log if e[0] == "frame"][-2:] == [("frame", (0, 2)), ("frame", (0, 2))]
    assert st.idled_while_held == []
    assert torch.equal(rc.audio(), _audio(LONG[:6])) and rc.codes().shape == (K, 6)
    assert conv.cached == base + 6 and conv._parked.shape[0] == base + 6
    assert torch.equal(conv._parked, conv.tokens[:conv.cached])
    assert conv.tokens.shape[0] == base + 7 and not conv.tokens[-1].any()
    _run(srv)
    assert rl.done and torch.equal(rl.audio(), _audio(LONG[:12]))


def test_generate_cli_conversation_key(tmp_path):
    from csm.cli.generate import read_serve_file
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "conversation": "u1"}\n{"text": "two", "speaker": 1}\n{"text": "three", "conversation": "u1", "seed": 3}\n')
    assert read_serve_file(str(p)) == [{"text": "one", "speaker": 0, "adapter": None, "seed": None, "conversation": "u1"},
                                       {"text": "two", "speaker": 1, "adapter": None, "seed": None},
                                       {"text": "three", "speaker": 0, "adapter": None, "seed": 3, "conversation": "u1"}]
