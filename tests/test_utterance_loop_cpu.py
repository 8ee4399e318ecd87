"""The utterance loop of ``Generator.generate`` / ``generate_stream`` and ``Conversation.generate`` / ``generate_stream``, host
side, through the public calls only: how many frame calls a generation makes and how many frames it keeps for every EOS
position, look distance and frame limit (frames sampled past EOS consume the global torch generator, so the count decides the
bits of the next call), what a conversation's history and cache hold afterwards, and that every error of a call's preamble is
raised by the call itself with nothing touched."""
import itertools

import pytest
import torch

from test_conversation_cpu import K, State, StubModel, Tok, Codec, ZERO, _frames

TEXT, SPEAKER = "hi", 0
N_TEXT = len(Tok().encode(f"[{SPEAKER}]{TEXT}"))
LONGEST = 9                                      # the largest frame limit of the cases


class CountingModel(StubModel):
    """The stateless paths' model: ``generate_frame`` only hands out the next scripted frame; ``i`` counts the calls."""

    def generate_frame(self, tokens, mask, pos, temperature, topk, **kw):
        return self._sample()


def _script(e):
    """LONGEST + 1 frames, none of them zero but the one at index ``e`` (None: no EOS frame at all)."""
    frames = _frames(LONGEST + 1)
    if e is not None:
        frames[e] = ZERO
    return frames


def _expected(e, every, N):
    """(frame calls, frames kept): the host looks after every multiple of ``every`` frames and after the last one."""
    looks = sorted(set(range(every, N + 1, every)) | {N})
    if N == 0:
        return 0, 0
    if e is None or e >= N:
        return N, N
    return next(p for p in looks if p > e), e


@pytest.fixture
def world(monkeypatch):
    import csm.conversation as C
    from csm.generator import Generator
    monkeypatch.setattr(C, "DecodeState", State)
    State.made = []

    def make(script, model=StubModel, codec=Codec):
        m = model(script)
        return Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec()), m
    return make


def _frames_of(audio):
    return audio.numel() // 4                    # (the stub codec: 4 samples per frame)


def _check_conversation(conv, m, sampled, kept, N):
    assert m.i == sampled
    if N == 0:                                   # no turn was begun: nothing fed, no state made, the history untouched
        assert conv.tokens.shape[0] == 0 and conv._turns == [] and conv.cached == 0 and conv._state is None
        return
    assert conv.tokens.shape[0] == N_TEXT + kept + 1 and conv._turns == [N_TEXT + kept + 1]
    assert not conv.tokens[-1].any() and conv._open is None
    assert conv.cached == N_TEXT + min(sampled - 1, kept)
    st = conv._state
    assert st.cur == conv.cached - 1 and torch.equal(st.content(), conv.tokens[:conv.cached])


@pytest.mark.parametrize("e,every,N", list(itertools.product([None, 0, 1, 2, 3, 4, 7, 8], [1, 3, 4, 8], [0, 1, 4, 7, 9])))
def test_frame_calls_and_kept_frames_on_all_four_paths(world, e, every, N):
    sampled, kept = _expected(e, every, N)
    ms = N * 80
    gen, m = world(_script(e), CountingModel)
    assert _frames_of(gen.generate(TEXT, SPEAKER, [], max_audio_length_ms=ms, eos_check_every=every)) == kept
    assert m.i == sampled
    gen, m = world(_script(e), CountingModel)
    chunks = list(gen.generate_stream(TEXT, SPEAKER, [], max_audio_length_ms=ms, chunk_frames=every))
    assert sum(_frames_of(c) for c in chunks) == kept and m.i == sampled
    assert all(0 < _frames_of(c) <= every for c in chunks)
    gen, m = world(_script(e))
    conv = gen.conversation()
    assert _frames_of(conv.generate(TEXT, SPEAKER, max_audio_length_ms=ms, eos_check_every=every)) == kept
    _check_conversation(conv, m, sampled, kept, N)
    gen, m = world(_script(e))
    conv = gen.conversation()
    chunks = list(conv.generate_stream(TEXT, SPEAKER, max_audio_length_ms=ms, chunk_frames=every))
    assert sum(_frames_of(c) for c in chunks) == kept
    _check_conversation(conv, m, sampled, kept, N)


class NoStreamCodec(Codec):
    decode_stream = None


def _bad_calls(recompute_error):
    """The preamble errors of a ``generate_stream`` call, as (keywords, error type, match)."""
    return [(dict(top_p=2.0), ValueError, "top_p"),
            (dict(output_sample_rate=0), ValueError, "output_sample_rate"),
            (dict(chunk_frames=0), ValueError, "chunk_frames"),
            (dict(chunk_frames=2.5), ValueError, "chunk_frames")] + recompute_error


def test_generator_stream_errors_are_raised_by_the_call(world):
    gen, m = world(_script(None), CountingModel)
    stream = gen.generate_stream(TEXT, SPEAKER, [], max_audio_length_ms=8 * 80, chunk_frames=2)
    first = next(stream)
    run, calls = gen._run, m.i
    for kw, err, match in _bad_calls([(dict(adapter="nobody"), ValueError, "unknown LoRA adapter")]):
        with pytest.raises(err, match=match):
            gen.generate_stream(TEXT, SPEAKER, [], **kw)
    m.use_kv_cache = False
    with pytest.raises(ValueError, match="return_stats"):
        gen.generate_stream(TEXT, SPEAKER, [], return_stats=True)
    m.use_kv_cache = True
    gen._audio_tokenizer = NoStreamCodec()
    with pytest.raises(TypeError, match="decode_stream"):
        gen.generate_stream(TEXT, SPEAKER, [])
    assert gen._run == run and m.i == calls      # nothing was taken over: the open stream goes on where it was
    assert _frames_of(first) == 2 and sum(_frames_of(c) for c in stream) == 6


def test_conversation_stream_errors_are_raised_by_the_call(world):
    gen, m = world(_script(None))
    with pytest.raises(ValueError, match="unknown LoRA adapter"):        # (a conversation's adapter is named when it is made)
        gen.conversation(adapter="nobody")
    conv = gen.conversation()
    stream = conv.generate_stream(TEXT, SPEAKER, max_audio_length_ms=8 * 80, chunk_frames=2)
    first = next(stream)
    run, calls, length = conv._run, m.i, conv.tokens.shape[0]
    for kw, err, match in _bad_calls([]):
        with pytest.raises(err, match=match):
            conv.generate_stream(TEXT, SPEAKER, **kw)
    codec, gen._audio_tokenizer = gen._audio_tokenizer, NoStreamCodec()
    with pytest.raises(TypeError, match="decode_stream"):
        conv.generate_stream(TEXT, SPEAKER)
    gen._audio_tokenizer = codec
    assert conv._run == run and m.i == calls and conv.tokens.shape[0] == length and conv._open is not None
    assert _frames_of(first) == 2 and sum(_frames_of(c) for c in stream) == 6
    assert len(State.made) == 1 and conv.tokens.shape[0] == N_TEXT + 8 + 1
    # return_stats on the recompute path: a conversation refuses that path as a whole, when the turn begins
    gen, m = world(_script(None))
    conv = gen.conversation()
    m.use_kv_cache = False
    stream = conv.generate_stream(TEXT, SPEAKER, return_stats=True)
    with pytest.raises(RuntimeError, match="use_kv_cache must be on"):
        next(stream)
    assert conv.tokens.shape[0] == 0 and conv._state is None and len(State.made) == 1
