"""The streaming Mimi encoder, host side: the encoder's layer list and history lengths, a pure-torch model of the chunked
strided convolution (the rule csm_conv1d_stream_strided_f32 implements), the new export, and ``HeardTurn``'s bookkeeping on
``Conversation`` / ``ServedConversation`` against a stub model and a Python fake of ``encode_stream``."""
import math
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from test_conversation_cpu import K, State, StubModel, Tok, ZERO, _frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPF = 4                     # samples per frame of the stub codec


# ------------------------------------------------------------------------------------------------------------- layer list
def test_encoder_conv_layers_and_history():
    from csm.codec.mimi import encoder_conv_layers, history_len
    layers = encoder_conv_layers()
    names = [n for n, *_ in layers]
    assert names == ["encoder.layers.0",
                     "encoder.layers.1.block.1", "encoder.layers.1.block.3", "encoder.layers.3",
                     "encoder.layers.4.block.1", "encoder.layers.4.block.3", "encoder.layers.6",
                     "encoder.layers.7.block.1", "encoder.layers.7.block.3", "encoder.layers.9",
                     "encoder.layers.10.block.1", "encoder.layers.10.block.3", "encoder.layers.12",
                     "encoder.layers.14", "downsample"]
    assert [(k, s) for _, k, s, _, _ in layers] == [(7, 1), (3, 1), (1, 1), (8, 4), (3, 1), (1, 1), (10, 5), (3, 1), (1, 1), (12, 6),
                                                    (3, 1), (1, 1), (16, 8), (3, 1), (4, 2)]
    assert [elu for _, _, _, elu, _ in layers] == [False] + [True] * 13 + [False]
    assert [rep for *_, rep in layers] == [False] * 14 + [True]                # only downsample replicates its left edge
    assert math.prod(s for _, _, s, _, _ in layers[:-1]) * 2 == 1920 == math.prod(s for _, _, s, _, _ in layers)
    # k_eff - stride: the left padding of MimiCodec._conv
    assert [history_len("conv", k, s) for _, k, s, _, _ in layers] == [6, 2, 0, 4, 2, 0, 5, 2, 0, 6, 2, 0, 8, 2, 2]
    assert history_len("conv", 3, 2, dilation=2) == 3 and history_len("conv", 7, 1) == 6 and history_len("conv", 2, 2) == 0
    assert encoder_conv_layers((3, 2))[3][:3] == ("encoder.layers.3", 4, 2) and encoder_conv_layers((3, 2))[6][:3] == ("encoder.layers.6", 6, 3)


# ------------------------------------------------------------------------------------------------------------- the rule
def _stream_conv_model(x, w, stride, dil, groups, sched, replicate):
    """The chunked conv as the kernel does it: per chunk the input is [hist | x_chunk], hist = the last H = k_eff - stride
    columns of the previous [hist | x_chunk] (zeros at first, or - replicate - column 0 of the first chunk), outputs start at
    columns 0, stride, 2*stride, ... of it.  Returns (outputs, final history)."""
    C_in, k = x.shape[0], w.shape[2]
    H = (k - 1) * dil + 1 - stride
    hist = torch.zeros(C_in, H, dtype=x.dtype)
    ys, c0 = [], 0
    for i, n_out in enumerate(sched):
        xc = x[:, c0:c0 + n_out * stride]
        c0 += n_out * stride
        if i == 0 and replicate:
            hist = xc[:, :1].expand(C_in, H)
        cat = torch.cat([hist, xc], 1)
        ys.append(F.conv1d(cat[None], w, stride=stride, dilation=dil, groups=groups)[0])
        assert ys[-1].shape[1] == n_out
        hist = cat[:, cat.shape[1] - H:]
    return torch.cat(ys, 1), hist


@pytest.mark.parametrize("case", [(4, 8, 8, 4, 1, 1), (8, 8, 4, 2, 1, 1), (6, 4, 3, 2, 2, 1), (8, 8, 16, 8, 1, 8), (1, 4, 7, 1, 1, 1)])
@pytest.mark.parametrize("replicate", [False, True])
def test_chunked_strided_conv_rule(case, replicate):
    C_in, C_out, k, stride, dil, groups = case
    g = torch.Generator().manual_seed(sum(case))
    T_out = 23
    # small integers in float64: every product and partial sum is exact, so torch.equal holds whatever order F.conv1d sums in
    x = torch.randint(-8, 9, (C_in, T_out * stride), generator=g).double()
    w = torch.randint(-8, 9, (C_out, C_in // groups, k), generator=g).double()
    H = (k - 1) * dil + 1 - stride
    padded = F.pad(x[None], (H, 0), mode="replicate" if replicate else "constant")[0] if H else x
    full = F.conv1d(padded[None], w, stride=stride, dilation=dil, groups=groups)[0]
    assert full.shape == (C_out, T_out)
    for seed in range(4):
        sched, gs = [], torch.Generator().manual_seed(seed)
        while sum(sched) < T_out:
            sched.append(min(int(torch.randint(1, 6, (1,), generator=gs)), T_out - sum(sched)))
        got, hist = _stream_conv_model(x, w, stride, dil, groups, sched, replicate)
        assert torch.equal(got, full), (case, sched)
        assert torch.equal(hist, padded[:, padded.shape[1] - H:]), (case, sched)
    got, _ = _stream_conv_model(x, w, stride, dil, groups, [1] * T_out, replicate)    # H > n_in: old and new columns mix
    assert torch.equal(got, full)


# ------------------------------------------------------------------------------------------------------------- the export
def test_strided_stream_symbol_declared_and_exported():
    import ctypes
    from csm import hip
    name = "csm_conv1d_stream_strided_f32"
    header = open(os.path.join(ROOT, "include", "csm_hip.h")).read()
    assert re.search(rf"\bint {name}\(", header)
    assert name in hip.EXPORTS and hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    assert len(getattr(hip.lib, name).argtypes) == 17
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    from csm.codec.mimi import MimiCodec, MimiEncodeStream
    assert callable(hip.ops.conv1d_stream_strided_f32) and callable(MimiCodec.encode_stream)
    for m in ("step", "feed", "flush", "reset"):
        assert callable(getattr(MimiEncodeStream, m)), m


# ------------------------------------------------------------------------------------------------------------- HeardTurn
class FakeEncodeStream:
    """encode_stream protocol in Python: SPF samples per frame; frame f of an utterance has the codes f % 7 + 1 + codebook."""

    def __init__(self, log):
        self.log, self.pos, self.rem = log, 0, 0
        log.append("new")

    def reset(self):
        self.pos, self.rem = 0, 0
        self.log.append("reset")

    def _codes(self, n):
        f = torch.arange(self.pos, self.pos + n)
        self.pos += n
        return ((f[None, :] % 7) + 1 + torch.arange(K)[:, None]).unsqueeze(0)

    def feed(self, wav):
        assert wav.dim() == 3 and wav.shape[:2] == (1, 1)
        total = self.rem + wav.shape[-1]
        self.rem = total % SPF
        self.log.append(("feed", wav.shape[-1]))
        return self._codes(total // SPF)

    def flush(self):
        n, self.rem = int(self.rem > 0), 0
        self.log.append(("flush", n))
        return self._codes(n)


class Codec:
    """The stub codec: ``encode`` gives what the fake stream gives for the same audio (partial frame zero-padded)."""
    sample_rate = 24000

    def __init__(self):
        self.log = []

    def encode(self, audio):
        s = FakeEncodeStream([])
        return torch.cat([s.feed(audio.reshape(1, 1, -1)), s.flush()], 2)

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(SPF, -1)

    def decode_stream(self):
        return types.SimpleNamespace(step=self.decode)

    def encode_stream(self, max_chunk_frames=32):
        return FakeEncodeStream(self.log)


@pytest.fixture
def make(monkeypatch):
    import csm.conversation as C
    from csm.generator import Generator
    monkeypatch.setattr(C, "DecodeState", State)
    State.made = []

    def _make(script, **kw):
        codec = Codec()
        gen = Generator(StubModel(script), text_tokenizer=Tok(), audio_tokenizer=codec)
        return gen, gen.conversation(**kw), codec
    return _make


def _segment(n_samples, text="yo", speaker=1):
    from csm.generator import Segment
    return Segment(speaker, text, torch.zeros(n_samples))


def _hear(conv, n_samples, pieces, text="yo", speaker=1):
    turn = conv.hear(speaker)
    audio, at = torch.zeros(n_samples), 0
    for p in pieces:
        turn.feed(audio[at:at + p])
        at += p
    assert at == n_samples
    return turn


def test_heard_turn_equals_add(make):
    gen, a, _ = make(_frames(3) + [ZERO])
    _, b, codec = make(_frames(3) + [ZERO])
    a.add(_segment(5 * SPF))
    turn = _hear(b, 5 * SPF, [3, 0, 9, 1, 7])
    assert turn.frames == 5 and b.tokens.shape[0] == 0 and b.cached == 0         # feed touches neither history nor cache
    turn.end("yo")
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.mask, b.mask) and a._turns == b._turns
    assert codec.log == ["new", ("feed", 3), ("feed", 0), ("feed", 9), ("feed", 1), ("feed", 7), ("flush", 0)]
    # text frames, the streamed codes, one all-zero EOS frame
    tt, tm = gen._tokenize_text_segment("yo", 1)
    T = tt.shape[0]
    assert torch.equal(b.tokens[:T], tt) and torch.equal(b.mask[:T], tm)
    want = (torch.arange(5)[:, None] % 7) + 1 + torch.arange(K)[None, :]
    assert torch.equal(b.tokens[T:T + 5, :K], want) and not b.tokens[T:T + 5, K].any()
    assert b.tokens.shape[0] == T + 6 and not b.tokens[-1].any()
    assert bool(b.mask[T:, :K].all()) and not b.mask[T:, K].any()
    # a partial last frame is flushed (zero-padded) into one more frame, as the stub's encode does
    a.add(_segment(2 * SPF + 1, "hm"))
    t2 = _hear(b, 2 * SPF + 1, [2 * SPF + 1])
    assert t2.frames == 2
    t2.end("hm")
    assert t2.frames == 3 and torch.equal(a.tokens, b.tokens) and torch.equal(a.mask, b.mask)
    assert codec.log[-3:] == ["reset", ("feed", 2 * SPF + 1), ("flush", 1)]      # one stream per conversation, reused
    # both conversations speak the same next turn from it
    wa = a.generate("ok", 0, max_audio_length_ms=10 * 80, eos_check_every=1)
    wb = b.generate("ok", 0, max_audio_length_ms=10 * 80, eos_check_every=1)
    assert torch.equal(wa, wb) and torch.equal(a.tokens, b.tokens) and a.cached == b.cached


def test_heard_turn_rules(make):
    gen, conv, codec = make(_frames(9))
    turn = conv.hear(1)
    with pytest.raises(RuntimeError, match="heard turn open"):
        conv.hear(1)
    with pytest.raises(RuntimeError, match="heard turn is open"):
        conv.add(_segment(SPF))
    turn.feed(torch.zeros(2 * SPF))
    turn.cancel()
    assert conv.tokens.shape[0] == 0 and turn.closed
    for call in (lambda: turn.feed(torch.zeros(SPF)), lambda: turn.end("x")):
        with pytest.raises(RuntimeError, match="ended or cancelled"):
            call()
    turn.cancel()                                                                 # idempotent
    conv.add(_segment(SPF))                                                       # and add works again
    L = conv.tokens.shape[0]
    t2 = conv.hear(0)
    assert codec.log.count("new") == 1 and codec.log[-1] == "reset" and t2.frames == 0
    # end() while this conversation's own stream is open: as add, it invalidates the stream and keeps what was handed out
    s = conv.generate_stream("hi", 0, max_audio_length_ms=9 * 80, chunk_frames=2)
    next(s)
    t2.feed(torch.zeros(SPF))                                                     # hearing while speaking is fine
    next(s)
    t2.end("no")
    with pytest.raises(RuntimeError, match="invalidated"):
        next(s)
    T = gen._tokenize_text_segment("hi", 0)[0].shape[0]
    assert conv.tokens.shape[0] == L + T + 4 + 1 + gen._tokenize_text_segment("no", 0)[0].shape[0] + 1 + 1
    with pytest.raises(RuntimeError, match="ended or cancelled"):
        t2.end("no")
    # an end() with no audio at all: text and the EOS frame
    t3 = conv.hear(1)
    L = conv.tokens.shape[0]
    t3.end("")
    assert conv.tokens.shape[0] == L + gen._tokenize_text_segment("", 1)[0].shape[0] + 1
    # a codec without a stateful encoder
    bare = types.SimpleNamespace(sample_rate=24000, encode=None, decode=None)
    from csm.generator import Generator
    with pytest.raises(TypeError, match="encode_stream"):
        Generator(StubModel(_frames(2)), text_tokenizer=Tok(), audio_tokenizer=bare).conversation().hear(0)


def test_heard_turn_on_served_conversation(monkeypatch):
    import test_serve_conversation_cpu as S
    import csm.conversation as conv_mod
    import csm.serving as srv_mod
    from csm.generator import Generator
    monkeypatch.setattr(srv_mod, "DecodeState", S.State)
    monkeypatch.setattr(conv_mod, "DecodeState", S.ConvState)
    S.State.made, S.State.scripts = [], {0: [[5, 6, 7, 0] + [9] * 8] * 3, 2: [S.LONG]}

    class ServeCodec(S.RowsCodec):
        def encode(self, audio):
            s = FakeEncodeStream([])
            return torch.cat([s.feed(audio.reshape(1, 1, -1)), s.flush()], 2)

        def encode_stream(self, max_chunk_frames=32):
            return FakeEncodeStream(self.log)

    gen = Generator(S.StubModel(), text_tokenizer=Tok(), audio_tokenizer=ServeCodec())
    server = gen.serve(slots=2, chunk_frames=2)
    a, b = server.conversation(), server.conversation()
    other = server.conversation()
    other.say("elsewhere", 2, max_audio_length_ms=12 * 80)
    a.add(_segment(3 * SPF))
    turn = b.hear(1)
    turn.feed(torch.zeros(SPF + 1))
    server.step()                                                                 # another conversation speaks meanwhile
    turn.feed(torch.zeros(2 * SPF - 1))
    assert turn.frames == 3 and b.tokens.shape[0] == 0
    with pytest.raises(RuntimeError, match="heard turn open"):
        b.hear(1)
    with pytest.raises(RuntimeError, match="heard turn is open"):
        b.add(_segment(SPF))
    turn.end("yo")
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.mask, b.mask) and a._turns == b._turns
    # end() obeys add's rule: not while this conversation's own turn is open - and can be retried once it is done
    r = b.say("hi", 0, max_audio_length_ms=20 * 80)
    t2 = b.hear(1)
    t2.feed(torch.zeros(SPF))
    with pytest.raises(RuntimeError, match="still open"):
        t2.end("and")
    assert not t2.closed
    while not r.done:
        server.step()
    L = b.tokens.shape[0]
    t2.end("and")
    assert b.tokens.shape[0] == L + gen._tokenize_text_segment("and", 1)[0].shape[0] + 2 and b.cached < L
    r = b.say("more", 0, max_audio_length_ms=20 * 80)                             # the heard turn enters with the next feed
    while not r.done:
        server.step()
    assert torch.equal(b._parked, b.tokens[:b.cached]) and b.cached > L
    t3 = b.hear(1)
    t3.cancel()
    b.close()
    with pytest.raises(RuntimeError, match="closed"):
        b.hear(1)
