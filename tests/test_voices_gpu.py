"""Voices on the GPU, on the tiny model and HF-initialised Mimi of tests/test_serve_conversation_gpu.py: a voice prompt prefilled
once (``Generator.voice``) and forked into one-row conversations, server requests and served conversations.

Everything that compares our own paths with each other is torch.equal on bits ("Voices": contracts 1 to 6).  A voice
request is not bit-equal to the stateless ``submit(context=...)`` - its text goes through the append kernels - so closeness is
bounded as tests/test_serve_conversation_gpu.py bounds it: against the fp32 oracle, at most 2x what one from-scratch prefill errs."""
import pytest
import torch

from test_serve_conversation_gpu import K, MS, SumRowsCodec, _bits, _finish, _seg, _serve, _tiny
from test_serving_gpu import TEMP, TOPK, Tok, _adapter, _hf_mimi

pytestmark = pytest.mark.gpu
PROBE = dict(text="the line we follow", speaker=1, seed=1234)


def _voice_ctx():
    return [_seg(1, 5, 0, "hi")]                                       # 5 frames + text: 13 positions


@pytest.fixture(scope="module")
def world(dev):
    """The world of tests/test_serve_conversation_gpu.py with a bank of two adapters, a voice without adapter, one made with
    ``a1`` and a two-turn voice; ``bits``: each voice's ``kv`` as it was made (contract 6: it never changes)."""
    from csm.codec import MimiCodec
    from csm.generator import Generator
    codec = MimiCodec(_hf_mimi().state_dict(), device="cuda")
    m = _tiny()
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)
    for name, seed in (("a1", 1), ("a2", 2)):
        gen.add_adapter(name, _adapter(m, seed))
    v, v1 = gen.voice(_voice_ctx()), gen.voice(_voice_ctx(), adapter="a1")
    v2 = gen.voice(_voice_ctx() + [_seg(2, 20, 1, "hi")])
    w = dict(m=m, gen=gen, v=v, v1=v1, v2=v2, bits={id(x): x.kv.clone() for x in (v, v1, v2)})
    yield w
    for x in (v, v1, v2):
        assert torch.equal(_bits(x.kv), _bits(w["bits"][id(x)]))


def _untouched(world):
    for x in (world["v"], world["v1"], world["v2"]):
        assert torch.equal(_bits(x.kv), _bits(world["bits"][id(x)]))


# ---------------------------------------------------------------------------------------------------------------- engine
def test_voice_fields(world):
    m, v, v1, v2 = world["m"], world["v"], world["v1"], world["v2"]
    L = v.positions
    assert L == 13 and v.tokens.shape == v.mask.shape == (L, K + 1) and v.turns == (L,) and v2.turns == (13, 28)
    assert v.kv.shape == (m.bb.num_layers, 2, m.bb.num_kv_heads, L, 64) and v.kv.dtype == torch.bfloat16 and v.kv.is_contiguous()
    assert v.nbytes == v.kv.numel() * 2 and (v.adapter, v1.adapter) == (None, "a1")
    assert torch.equal(v.tokens, v1.tokens) and not torch.equal(_bits(v.kv), _bits(v1.kv))       # the adapter is in the cache


def test_fork_rows_equals_resume_rows(world):
    """Contract 1: the caches, ``bb.pos`` and ``row_pos`` after one ``fork_rows`` are those after the R ``resume_row`` calls."""
    from csm.engine import DecodeState
    m, v, v1, v2 = world["m"], world["v"], world["v1"], world["v2"]
    for rows, parkeds in (([3], [v2.kv]), ([9, 0, 15], [v.kv, v2.kv, v.kv]),
                          ([(7 * r + 5) % 16 for r in range(16)], [(v.kv, v1.kv, v2.kv)[r % 3] for r in range(16)])):
        a, b = DecodeState(m.engine, 16), DecodeState(m.engine, 16)
        for st in (a, b):                                              # something to overwrite, and something to leave alone
            st.bb.kv.fill_(0.25)
            st.resume_row(1, v2.kv[:, :, :, :30].contiguous())
        for r, p in zip(rows, parkeds):
            a.resume_row(r, p)
        b.fork_rows(rows, parkeds)
        assert torch.equal(_bits(a.bb.kv), _bits(b.bb.kv)) and torch.equal(a.bb.pos, b.bb.pos) and a.row_pos == b.row_pos
        assert [b.row_pos[r] for r in rows] == [p.shape[3] - 1 for p in parkeds]
    st = DecodeState(m.engine, 4)
    with pytest.raises(ValueError, match="distinct"):
        st.fork_rows([1, 1], [v.kv, v.kv])
    with pytest.raises(ValueError, match="distinct"):
        st.fork_rows([4], [v.kv])
    with pytest.raises(ValueError, match="1..16 rows"):
        st.fork_rows([0, 1], [v.kv])
    with pytest.raises(ValueError, match="not a parked history"):
        st.fork_rows([0], [v.kv[:, :1]])
    with pytest.raises(ValueError, match="not a parked history"):
        st.fork_rows([0], [v.kv.float()])
    assert st.row_pos == [-1] * 4
    _untouched(world)


@pytest.mark.parametrize("name", [None, "a1"])
def test_voice_kv_equals_a_served_rows_prefill(world, name):
    """Contract 2: ``v.kv`` is ``park_row(b, L)`` after ``prefill_row(b, v.tokens, v.mask)`` on a 16-row state whose row has the
    voice's adapter."""
    from csm.engine import DecodeState
    gen, m = world["gen"], world["m"]
    v = world["v1"] if name else world["v"]
    bank = gen._bank.entries
    st = DecodeState(m.engine, 16, bank=list(bank.values()))
    st.set_row_adapter(6, bank[name] if name else None)
    st.prefill_row(6, v.tokens, v.mask)
    assert torch.equal(_bits(st.park_row(6, v.positions)), _bits(v.kv))


# ------------------------------------------------------------------------------------------------------------- one row
def _hand_built(world, v, text, speaker, frames):
    """The first turn from existing primitives: prefill the voice's tokens, append the text frames, the frame tail, then
    ``generate_frame`` - (codes [frames, K], audio)."""
    from csm.engine import DecodeState
    gen, m = world["gen"], world["m"]
    e = m.engine
    with torch.inference_mode():
        st = DecodeState(e, 1, gen._resolve_adapters([v.adapter]))
        st.prefill(v.tokens.unsqueeze(0), v.mask.unsqueeze(0))
        last_h = st.append(*gen._tokenize_text_segment(text, speaker))
        samples = [e._frame_tail(st, last_h, TEMP, TOPK, None)]
        msk = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1).cuda()
        prev, m._decode_state = getattr(m, "_decode_state", None), st
        try:
            while len(samples) < frames:
                tok = torch.cat([samples[-1].long(), torch.zeros(1, 1, dtype=torch.long, device="cuda")], 1).unsqueeze(1)
                samples.append(m.generate_frame(tok, msk, torch.ones(1, 1, dtype=torch.long), TEMP, TOPK))
        finally:
            m._decode_state = prev
        codes = torch.cat(samples, 0).long()
        assert not bool((codes == 0).all(dim=1).any())                 # (no EOS among them: the turn ends at its length limit)
        return codes, gen._audio_tokenizer.decode(codes.t().unsqueeze(0)).reshape(-1)


@pytest.mark.parametrize("name", [None, "a1"])
def test_conversation_first_turn_equals_hand_built(world, name):
    """Contract 3, and ``generate(voice=)`` / ``generate_stream(voice=)`` are that conversation's calls."""
    gen = world["gen"]
    v = world["v1"] if name else world["v"]
    torch.manual_seed(41)
    codes, audio = _hand_built(world, v, "hello there", 1, 6)
    torch.manual_seed(41)
    conv = gen.conversation(voice=v)
    assert conv.cached == v.positions and torch.equal(conv.tokens, v.tokens)
    got = conv.generate("hello there", 1, max_audio_length_ms=MS, temperature=TEMP, topk=TOPK)
    T = gen._tokenize_text_segment("hello there", 1)[0].shape[0]
    base = v.positions + T
    assert torch.equal(conv.tokens[base:base + 6, :K], codes) and torch.equal(got, audio)
    assert conv.tokens.shape[0] == base + 7 and conv.cached == base + 5
    torch.manual_seed(41)
    assert torch.equal(gen.generate("hello there", 1, [], max_audio_length_ms=MS, temperature=TEMP, topk=TOPK, voice=v), audio)
    torch.manual_seed(41)
    chunks = list(gen.generate_stream("hello there", 1, [], max_audio_length_ms=MS, temperature=TEMP, topk=TOPK, chunk_frames=4,
                                      voice=v))
    assert [c.numel() for c in chunks] == [4 * 1920, 2 * 1920] and torch.equal(torch.cat(chunks), audio)
    _untouched(world)


# -------------------------------------------------------------------------------------------------------------- serving
def _probe(srv, v, **kw):
    return srv.submit(PROBE["text"], PROBE["speaker"], [_seg(3)], voice=v, seed=PROBE["seed"], max_audio_length_ms=MS, **kw)


@pytest.fixture(scope="module")
def alone(world):
    out = {}
    for key in ("v", "v1"):
        srv = _serve(world["gen"])
        r = _probe(srv, world[key])
        srv.step()
        assert r.slot == 0
        _finish(srv)
        assert r.done and r.codes().shape == (K, 6) and r.audio().numel() == 6 * 1920
        out[key] = (r.codes(), r.audio())
    assert not torch.equal(out["v"][0], out["v1"][0])                  # the adapter changes what is said
    return out


def _log_calls(st):
    log = []
    for name in ("fork_rows", "append_rows", "resume_row", "prefill_row", "serve_first"):
        def wrapped(*a, _f=getattr(st, name), _n=name, **k):
            out = _f(*a, **k)
            log.append((_n, a, out))
            return out
        setattr(st, name, wrapped)
    return log


@pytest.mark.parametrize("key", ["v", "v1"])
def test_voice_request_among_fifteen_neighbours(world, alone, key):
    """Contract 4 (another slot, 15 neighbours admitted at the same boundary: requests with the same voice, with another voice
    and adapter, resumed conversation turns, plain submits with context) and contract 5 (the admitted rows' caches)."""
    from csm.engine import DecodeState
    gen, m = world["gen"], world["m"]
    v, other = world[key], world["v1" if key == "v" else "v"]
    srv = _serve(gen)
    convs = [srv.conversation(context=[_seg(30 + i, 2 + i, 0, "c" * (1 + i))] if i % 2 else [], adapter=[None, "a2", "a1"][i % 3],
                              seed=500 + i) for i in range(4)]
    for i, c in enumerate(convs):
        c.say(f"first {i}", 0, max_audio_length_ms=(3 + i) * 80)
    _finish(srv)
    log = _log_calls(srv._state)
    same = [srv.submit(f"same voice {i}", 2, [_seg(40 + i, 2)] if i else [], voice=v, seed=i or None, max_audio_length_ms=(5 + i) * 80)
            for i in range(2)]
    convs[0].say("second 0", 0, max_audio_length_ms=5 * 80)
    others = [srv.submit("other voice", 0, [], voice=other, seed=9, max_audio_length_ms=7 * 80)]
    plain = [srv.submit("plain", 2, [_seg(3)], adapter="a2", seed=3, max_audio_length_ms=6 * 80)]
    convs[1].say("second 1", 1, max_audio_length_ms=6 * 80)
    r = _probe(srv, v)
    same += [srv.submit(f"same voice late {i}", 1, [], voice=v, seed=20 + i, max_audio_length_ms=(5 + i) * 80) for i in range(2)]
    others += [srv.submit(f"other voice late {i}", 0, [_seg(50 + i, 1)], voice=other, max_audio_length_ms=7 * 80) for i in range(2)]
    for i in (2, 3):
        convs[i].say(f"second {i}", 0, max_audio_length_ms=(4 + i) * 80)
    plain += [srv.submit("late plain " * (1 + i), 1, [_seg(60 + i, 2)] if i else [], seed=70 + i, max_audio_length_ms=7 * 80) for i in range(3)]
    assert srv.queued == 16
    srv.step()
    slot = r.slot
    assert slot == 6 and srv.last_join_rows == 16
    # ONE fork_rows for the eight voice requests, ONE append_rows for them and the four resumed turns, ONE frame tail
    kinds = [e[0] for e in log]
    assert kinds.count("fork_rows") == 1 and kinds.count("append_rows") == 1 and kinds.count("serve_first") == 1
    assert kinds.count("resume_row") == 4 and kinds.count("prefill_row") == 4
    forks = next(e for e in log if e[0] == "fork_rows")[1]
    voiced = same + others + [r]
    assert sorted(forks[0]) == sorted(q.slot for q in voiced) and all(any(p is x.kv for x in (v, other)) for p in forks[1])
    assert len(next(e for e in log if e[0] == "append_rows")[1][0]) == 12
    # contract 5: the rows' caches [0, L + n_feed) are those of a fresh state given prefill_row(voice) then append_rows(feed)
    fresh = DecodeState(m.engine, 16, bank=list(gen._bank.entries.values()))
    for q in (r, others[0], others[2], same[1]):
        b, vq, n = q.slot, q._voice, q._voice.positions + q._tokens.shape[0]
        fresh.set_row_adapter(b, gen._bank.entries[vq.adapter] if vq.adapter else None)
        fresh.prefill_row(b, vq.tokens, vq.mask)
        fresh.append_rows([b], [q._tokens], [q._mask])
        assert fresh.row_pos[b] == n - 1
        assert torch.equal(_bits(srv._state.bb.kv[:, :, b, :, :n]), _bits(fresh.bb.kv[:, :, b, :, :n])), b
    m._decode_state = srv._state
    _finish(srv)
    assert r.done and torch.equal(r.codes(), alone[key][0]) and torch.equal(r.audio(), alone[key][1])
    assert all(q.done for q in voiced + plain)
    _untouched(world)


@pytest.mark.parametrize("key", ["v", "v1"])
def test_served_conversation_first_turn_equals_the_request(world, alone, key):
    """Contract 4, third case: the first turn of ``srv.conversation(voice=v, seed=s)`` - a resumed turn, no new code in the
    admission - has the request's codes and audio; the voice's K / V are the parked cache, shared."""
    v = world[key]
    srv = _serve(world["gen"])
    for i in range(3):
        srv.submit("filler", 2, [], seed=i, max_audio_length_ms=(4 + i) * 80)
    conv = srv.conversation(voice=v, context=[_seg(3)], seed=PROBE["seed"])
    assert conv._parked is v.kv and conv.cached == v.positions and conv.adapter == v.adapter
    log = _log_calls(srv._state)
    r = conv.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=MS)
    srv.step()
    assert r.slot == 3 and [e[0] for e in log if e[0] in ("fork_rows", "resume_row")] == ["resume_row"]
    _finish(srv)
    assert r.done and torch.equal(r.codes(), alone[key][0]) and torch.equal(r.audio(), alone[key][1])
    assert conv._parked is not v.kv and conv._parked.data_ptr() != v.kv.data_ptr()
    _untouched(world)


def test_shifted_conversations_leave_the_voice_alone(world):
    """Contract 6: ``on_overflow="shift"`` cuts the second turn of the VOICE out of the cache at the first ``say`` /
    ``generate`` - out of place on the server (``shift_parked``), in the conversation's own row on one row - and ``v.kv`` keeps
    its bits."""
    gen, m, v2 = world["gen"], world["m"], world["v2"]
    L = v2.positions
    big = (m.bb.max_seq_len - L) * 80                                  # history + text + frames >= max_seq_len
    srv = _serve(gen)
    conv = srv.conversation(voice=v2, on_overflow="shift", keep_turns=1, seed=5)
    r = conv.say("one", 0, max_audio_length_ms=big)
    assert conv.cached == 13 and conv._parked is not v2.kv and conv._parked.shape[3] == 13 and conv._turns[0] == 13
    _untouched(world)
    srv.step()
    srv.step()
    assert r._emitted == 8
    _untouched(world)
    one = gen.conversation(voice=v2, on_overflow="shift", keep_turns=1)
    chunks = one.generate_stream("one", 0, max_audio_length_ms=big, temperature=TEMP, topk=TOPK, chunk_frames=4)
    assert next(chunks).numel() == 4 * 1920 and one._state.row_pos[0] >= 13 and one._turns[0] == 13 and len(one._turns) == 2
    chunks.close()
    _untouched(world)


# ------------------------------------------------------------------------------------------- closeness to a from-scratch prefill
def test_voice_request_vs_one_prefill_against_oracle(dev):
    """The bound of tests/test_serve_conversation_gpu.py::test_served_cache_vs_one_prefill_against_oracle: the codebook-0 logits
    at the last prompt position of a voice request (voice 13 positions, then a 4-frame context segment and the text through the
    stacked append) may err against the fp32 oracle at most 2x what ONE from-scratch prefill of the same tokens errs.
    Measured on one MI355X (50 positions, 13 of them the voice's, max |logit| 0.86): voice request 6.6e-3, one prefill 8.4e-3."""
    from csm.engine import DecodeState
    from csm.generator import Generator
    from test_conversation_gpu import _c0_logits, _oracle, _tiny_oracle_model
    O, T = _oracle()
    m, p32 = _tiny_oracle_model()
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=SumRowsCodec(T.n_codebooks, T.audio_vocab))
    v = gen.voice(_voice_ctx())
    srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)
    srv.submit("neighbour", 2, [], seed=1, max_audio_length_ms=60 * 80)
    srv.submit("another", 2, [], voice=v, seed=2, max_audio_length_ms=6 * 80)
    log = _log_calls(srv._state)
    r = srv.submit("the line we follow", 1, [_seg(11, 4)], voice=v, seed=3, max_audio_length_ms=MS)
    srv.step()
    rows, h = next((e[1][0], e[2]) for e in log if e[0] == "append_rows")
    tokens, mask = torch.cat([v.tokens, r._tokens]), torch.cat([v.mask, r._mask])
    with torch.inference_mode():                                       # (the server's state was made under it)
        got = _c0_logits(m, h[list(rows).index(r.slot)].unsqueeze(0))
    one = _c0_logits(m, DecodeState(m.engine, 1).prefill(tokens.unsqueeze(0), mask.unsqueeze(0)))
    with torch.no_grad():
        hid = O.backbone_hidden(p32, T, tokens.cpu().unsqueeze(0), mask.cpu().unsqueeze(0))
        ref = hid[0, -1].float() @ p32["codebook0_head.weight"].t().float()
    e_voice, e_one = float((got.cpu() - ref).abs().max()), float((one.cpu() - ref).abs().max())
    print(f"voice request vs oracle ({tokens.shape[0]} positions, {v.positions} from the voice): voice {e_voice:.3e}, one prefill "
          f"{e_one:.3e}, max |logit| {float(ref.abs().max()):.3e}")
    m._decode_state = None
    assert e_voice <= 2 * e_one, (e_voice, e_one)
