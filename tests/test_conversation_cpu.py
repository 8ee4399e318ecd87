"""Conversations, host side: the history / cache bookkeeping of csm/conversation.py against a stub model and codec, the
csm-generate flags, and the library export."""
import types

import pytest
import torch

K = 4                       # codebooks of the stub model
MAX_SEQ = 64


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


class Codec:
    """Mimi's protocol: 1 frame per 4 samples, codes derived from the sample count; counts its encode calls."""
    sample_rate = 24000

    def __init__(self):
        self.encoded = []

    def encode(self, audio):
        T = audio.shape[-1] // 4
        self.encoded.append(T)
        return (torch.arange(K * T).reshape(1, K, T) % 7) + 1

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(4, -1)

    def decode_stream(self):
        return types.SimpleNamespace(step=self.decode)


class State:
    """What Conversation uses of DecodeState: prefill / append / truncate and the position."""
    made = []

    def __init__(self, engine, B, adapters=None):
        self.cur, self.log, self.fed = -1, [], []
        State.made.append(self)

    def prefill(self, tokens, masks):
        assert tokens.dim() == 3 and tokens.shape[0] == 1
        self.cur = tokens.shape[1] - 1
        self.fed = [tokens[0].clone()]
        self.log.append(("prefill", tokens.shape[1]))
        return torch.zeros(1, 8)

    def append(self, tokens, masks):
        assert self.cur >= 0 and tokens.dim() == 2
        self.fed.append(tokens.clone())
        self.cur += tokens.shape[0]
        self.log.append(("append", tokens.shape[0]))
        return torch.zeros(1, 8)

    def truncate(self, length):
        assert 1 <= length <= self.cur + 1
        self.cur = length - 1
        self.log.append(("truncate", length))

    def content(self):
        """The frames the cache holds, positions 0 .. cur."""
        return torch.cat(self.fed, 0)[:self.cur + 1]


class StubModel:
    device = torch.device("cpu")
    use_kv_cache = True

    def __init__(self, script):
        self.args = types.SimpleNamespace(audio_num_codebooks=K)
        self.bb = types.SimpleNamespace(max_seq_len=MAX_SEQ)
        self.script, self.i = script, 0
        self._decode_state = None
        self.engine = types.SimpleNamespace(_need=lambda: None, _frame_tail=self._tail)

    def setup_caches(self, n):
        pass

    def reset_caches(self):
        self._decode_state = None

    def _sample(self):
        s = self.script[self.i % len(self.script)]
        self.i += 1
        return s.clone()

    def _tail(self, st, last_h, temperature, topk, noise):
        return self._sample()

    def generate_frame(self, tokens, mask, pos, temperature, topk, **kw):
        st = self._decode_state
        assert st is not None and int(pos[0, 0]) != 0 and tokens.shape == (1, 1, K + 1)
        st.fed.append(tokens[0].clone())
        # positions after a truncate are overwritten: keep `fed` consistent with `cur`
        flat = torch.cat(st.fed, 0)
        st.fed = [torch.cat([flat[:st.cur + 1], tokens[0]], 0)]
        st.cur += 1
        return self._sample()


def _frames(n, start=1):
    return [torch.full((1, K), start + i, dtype=torch.int32) for i in range(n)]


ZERO = torch.zeros(1, K, dtype=torch.int32)


@pytest.fixture
def make(monkeypatch):
    import csm.conversation as C
    from csm.generator import Generator
    monkeypatch.setattr(C, "DecodeState", State)
    State.made = []

    def _make(script, **kw):
        codec = Codec()
        m = StubModel(script)
        gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)
        return gen, gen.conversation(**kw), m, codec
    return _make


def _seg(frames=3, text="yo", speaker=1):
    from csm.generator import Segment
    return Segment(speaker, text, torch.zeros(4 * frames))


def _check_cache(conv):
    """The cache holds exactly the first ``cached`` positions of the history."""
    st = conv._state
    assert st.cur == conv.cached - 1
    assert torch.equal(st.content(), conv.tokens[:conv.cached])


def test_history_layout_after_generate_and_add(make):
    gen, conv, m, codec = make(_frames(3) + [ZERO], context=[_seg(3)])
    assert conv.cached == 0 and codec.encoded == [3]
    t_ctx, m_ctx = gen._tokenize_segment(_seg(3))
    assert torch.equal(conv.tokens, t_ctx) and torch.equal(conv.mask, m_ctx)
    codec.encoded.clear()
    audio = conv.generate("hi", 0, max_audio_length_ms=10 * 80, eos_check_every=1)
    assert audio.numel() == 3 * 4
    tt, tm = gen._tokenize_text_segment("hi", 0)
    spoken = torch.zeros(4, K + 1, dtype=torch.long)
    spoken[:3, :K] = torch.cat(_frames(3), 0)
    smask = torch.zeros(4, K + 1, dtype=torch.bool)
    smask[:, :K] = True
    assert torch.equal(conv.tokens, torch.cat([t_ctx, tt, spoken], 0))          # text, kept codes, ONE zero EOS frame
    assert torch.equal(conv.mask, torch.cat([m_ctx, tm, smask], 0))
    L = conv.tokens.shape[0]
    conv.add(_seg(2, "and you"))
    assert codec.encoded == [2]                                                  # only the new segment was encoded
    t2, _ = gen._tokenize_segment(_seg(2, "and you"))
    assert torch.equal(conv.tokens[L:], t2)
    codec.encoded.clear()
    assert conv.cached <= L                                                      # an added turn enters with the next spoken one
    conv.generate("ok", 0, max_audio_length_ms=10 * 80, eos_check_every=1)
    assert codec.encoded == [] and len(State.made) == 1
    assert [op for op, _ in conv._state.log if op != "truncate"] == ["prefill", "append"]
    _check_cache(conv)
    with pytest.raises(AttributeError):
        conv.tokens = None


def test_cached_eos_found_with_later_frames_fed(make):
    gen, conv, m, _ = make(_frames(2) + [ZERO] + _frames(5, 10))
    conv.generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=8)       # 8 frames sampled, 7 fed; EOS is sample 2
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert conv.tokens.shape[0] == T + 2 + 1 and not conv.tokens[-1].any() and conv.tokens[-2].any()
    assert conv.cached == T + 2                                                  # cut back to the EOS frame's position
    assert ("truncate", T + 2) in conv._state.log
    _check_cache(conv)


def test_cached_eos_found_and_not_fed(make):
    gen, conv, m, _ = make(_frames(2) + [ZERO])
    conv.generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=1)       # the EOS frame is seen before it is fed
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert conv.tokens.shape[0] == T + 3 and conv.cached == T + 2
    assert not any(op == "truncate" for op, _ in conv._state.log)
    _check_cache(conv)
    conv.generate("more", 0, max_audio_length_ms=20 * 80, eos_check_every=1)     # ... and goes in with the next append
    T2 = gen._tokenize_text_segment("more", 0)[0].shape[0]
    assert conv._state.log[1] == ("append", 1 + T2)
    _check_cache(conv)


def test_cached_frame_limit_hit(make):
    gen, conv, m, _ = make(_frames(9))
    audio = conv.generate("hi", 0, max_audio_length_ms=5 * 80, eos_check_every=2)
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert audio.numel() == 5 * 4
    assert conv.tokens.shape[0] == T + 5 + 1 and not conv.tokens[-1].any()
    assert conv.cached == T + 4                                                  # the last frame and the EOS frame were never fed
    _check_cache(conv)
    conv.generate("x", 0, max_audio_length_ms=2 * 80)
    assert conv._state.log[1][0] == "append" and conv._state.log[1][1] == 2 + gen._tokenize_text_segment("x", 0)[0].shape[0]
    _check_cache(conv)


def test_stream_equals_generate_history_and_abandon(make):
    gen, a, _, _ = make(_frames(6) + [ZERO] + _frames(3, 20))
    _, b, _, _ = make(_frames(6) + [ZERO] + _frames(3, 20))
    wav = a.generate("hi", 0, max_audio_length_ms=20 * 80, eos_check_every=4)
    parts = list(b.generate_stream("hi", 0, max_audio_length_ms=20 * 80, chunk_frames=4))
    assert torch.equal(torch.cat(parts), wav) and torch.equal(a.tokens, b.tokens) and a.cached == b.cached
    # abandoned after the first chunk: the 2 frames handed out are the turn, the rest is rolled back
    gen, c, _, _ = make(_frames(9))
    s = c.generate_stream("hi", 0, max_audio_length_ms=9 * 80, chunk_frames=2)
    next(s)
    s.close()
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert c.tokens.shape[0] == T + 2 + 1 and c.cached == T + 1 and not c.tokens[-1].any()
    _check_cache(c)
    # its own next call invalidates an open stream and keeps what was handed out
    s = c.generate_stream("yo", 0, max_audio_length_ms=9 * 80, chunk_frames=3)
    next(s)
    L = c.tokens.shape[0]
    c.add(_seg(1))
    assert c.tokens.shape[0] > L + 3
    with pytest.raises(RuntimeError):
        next(s)
    c.generate("z", 0, max_audio_length_ms=2 * 80)
    _check_cache(c)


def test_overflow_error_and_drop_oldest(make):
    gen, conv, m, _ = make(_frames(40), context=[_seg(5, "a"), _seg(6, "b")])
    with pytest.raises(ValueError, match=r"Inputs too long, must be below max_seq_len - max_audio_frames: 14"):
        conv.generate("hi", 0, max_audio_length_ms=50 * 80)
    assert conv.tokens.shape[0] == sum(gen._tokenize_segment(s)[0].shape[0] for s in (_seg(5, "a"), _seg(6, "b")))
    gen, conv, m, _ = make(_frames(40), context=[_seg(5, "a"), _seg(6, "b")], on_overflow="drop_oldest")
    conv.generate("hi", 0, max_audio_length_ms=3 * 80)                           # fits: nothing dropped
    first = gen._tokenize_segment(_seg(5, "a"))[0].shape[0]
    second = gen._tokenize_segment(_seg(6, "b"))[0].shape[0]
    before = conv.tokens.clone()
    L = before.shape[0]
    T = gen._tokenize_text_segment("next", 0)[0].shape[0]
    frames = MAX_SEQ - (L - first) - T - 1                                       # fits only without the first turn
    assert L + T + frames >= MAX_SEQ > (L - first) + T + frames and frames > 0
    conv.generate("next", 0, max_audio_length_ms=frames * 80)
    assert torch.equal(conv.tokens[:L - first], before[first:])                  # whole turns only: the second one starts the history
    assert ("prefill", L - first + T) in conv._state.log and len(State.made) == 1
    _check_cache(conv)
    with pytest.raises(ValueError, match="Inputs too long"):                     # a line that cannot fit even alone
        conv.generate("x" * 80, 0, max_audio_length_ms=80)
    with pytest.raises(ValueError):
        gen.conversation(on_overflow="slide")
    assert second > 0


def test_generate_cli_conversation_flags():
    from csm.cli.generate import parse_args
    base = ["--model-path", "c.pt", "--text", "hi", "--mimi-weights", "m", "--text-tokenizer", "t"]
    a = parse_args(base)
    assert a.next_text is None and a.next_speaker is None and a.stream is False and a.chunk_frames == 4 and a.speaker == 0
    a = parse_args(base + ["--next-text", "and then", "--next-text", "bye", "--next-speaker", "1", "--next-speaker", "0"])
    assert a.next_text == ["and then", "bye"] and a.next_speaker == [1, 0]
    a = parse_args(base + ["--speaker", "3", "--next-text", "x", "--stream"])
    assert a.next_text == ["x"] and a.next_speaker is None and a.speaker == 3 and a.stream is True
    with pytest.raises(SystemExit):
        parse_args(base + ["--next-text", "x", "--next-text", "y", "--next-speaker", "1"])


def test_library_exports_attn_append():
    from csm import hip
    assert "csm_attn_append" in hip.EXPORTS and hasattr(hip.lib, "csm_attn_append")
    assert callable(hip.ops.attn_append) if hasattr(hip, "ops") else True
    from csm.engine import DecodeState
    assert callable(DecodeState.append) and callable(DecodeState.truncate)
