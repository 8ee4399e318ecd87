"""More listeners than slots on the GPU (``Generator.serve(streams=)``, csm/serving.py): a seeded request that is parked in the
middle of its utterance, resumed into another slot, paused and resumed has the codes and the audio it has alone on a server
without ``streams`` - at every sampler level, with an adapter, at another output rate, with FP8 decode weights, and as a
conversation's turn together with the turn after it.  And the rows codec objects with more state slots than rows of a launch.
Everything is compared with torch.equal; the load and its submission order are tests/serve_streams_order.py's, which
tests/test_serve_streams_cpu.py proves to park the probe twice and to move it."""
import pytest
import torch

import serve_streams_order as ORDER
from test_serving_gpu import PROBE, TEMP, TOPK, K, world  # noqa: F401  (the tiny model, Mimi and the adapters of the serving tests)

pytestmark = pytest.mark.gpu
assert PROBE["frames"] == ORDER.PROBE_FRAMES


def _submit_probe(srv, ctx, adapter=None, **kw):
    return srv.submit(PROBE["text"], PROBE["speaker"], ctx, adapter=adapter, seed=PROBE["seed"],
                      max_audio_length_ms=PROBE["frames"] * 80, **kw)


def _alone(gen, ctx, adapter=None, **serve_kw):
    """The probe alone on today's server."""
    srv = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK, **serve_kw)
    r = _submit_probe(srv, ctx, adapter)
    for _ in srv.run():
        pass
    assert r.done and r.codes().shape == (K, PROBE["frames"]) and r.preemptions == 0
    return r


def _among(gen, ctx, adapter=None, names=(None,), probe=None, **serve_kw):
    """The probe among 23 seeded others on 16 slots and 24 streams, in the order of the contract.  Returns (probe, server)."""
    srv = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK, streams=ORDER.STREAMS, **serve_kw)

    def other(i):
        return srv.submit("n" * (3 + i % 5), i % 3, ctx if i % 8 == 3 else [], adapter=names[i % len(names)], seed=100 + i,
                          max_audio_length_ms=ORDER.OTHER_FRAMES * 80)
    b, others = ORDER.submit_all(probe or (lambda: _submit_probe(srv, ctx, adapter)), other)
    assert b.id == ORDER.PROBE_AT
    return b, others, srv


def _same(b, a, srv):
    assert b.done and b.preemptions >= 2 and len(set(b.slots_held)) >= 2, (b.preemptions, b.slots_held)
    assert srv.stats["park_launches"] <= srv.stats["steps"] and srv.stats["resume_launches"] <= srv.stats["steps"]
    assert torch.equal(b.codes(), a.codes()), f"codes differ after {b.preemptions} parks through slots {b.slots_held}"
    assert b.audio().shape == a.audio().shape and torch.equal(b.audio(), a.audio())


def _run(srv):
    for _ in srv.run():
        pass


def test_parked_and_resumed_request_has_the_bits_it_has_alone(world):
    gen, ctx, codec = world["plain"], world["ctx"], world["codec"]
    a = _alone(gen, ctx)
    b, others, srv = _among(gen, ctx)
    _run(srv)
    _same(b, a, srv)
    assert torch.equal(b.audio(), codec.decode(b.codes().unsqueeze(0)).reshape(-1))      # the codec slot never moved: decode()'s audio
    assert all(o.done and o.codes().shape[1] > 0 for o in others) and srv.in_flight == [] and srv.stats["parks"] >= 16
    st = srv._state
    assert st.graph is not None and st.row_gen == {}                                     # one captured frame; every generator left


@pytest.mark.parametrize("level", ["processed", "typical"])
def test_parked_request_at_the_ring_levels(world, level):
    """The ring of sampled codes and the frame counter travel with the request: a window of 16 frames over 14 looks back
    across every park."""
    kw = dict(row_sampling=True, row_processors=True, repetition_penalty=1.3, repetition_window=16) if level == "processed" else \
        dict(row_sampling=True, row_typical=True, typical_p=0.9)
    gen, ctx = world["plain"], world["ctx"]
    a = _alone(gen, ctx, **kw)
    b, _, srv = _among(gen, ctx, **kw)
    _run(srv)
    _same(b, a, srv)
    plain = _alone(gen, ctx)
    assert not torch.equal(plain.codes(), a.codes())                                      # (the level changes what is said)


def test_parked_request_with_a_bank_adapter(world):
    gen, ctx = world["banked"], world["ctx"]
    a = _alone(gen, ctx, adapter="a1")
    b, _, srv = _among(gen, ctx, adapter="a1", names=(None, "a2", "a1"))
    _run(srv)
    _same(b, a, srv)
    assert not torch.equal(a.codes(), _alone(gen, ctx).codes())


def test_parked_request_at_another_output_rate(world):
    gen, ctx = world["plain"], world["ctx"]
    a = _alone(gen, ctx, output_sample_rate=48000)
    b, _, srv = _among(gen, ctx, output_sample_rate=48000)
    _run(srv)
    _same(b, a, srv)
    assert b.sample_rate == 48000 and b.audio().numel() == 2 * PROBE["frames"] * 1920


def test_parked_request_with_fp8_decode_weights(world):
    m, gen, ctx = world["m"], world["plain"], world["ctx"]
    m.decode_weights = "fp8"
    try:
        a = _alone(gen, ctx)
        b, _, srv = _among(gen, ctx)
        _run(srv)
        _same(b, a, srv)
    finally:
        m.decode_weights = "bf16"
    assert not torch.equal(a.codes(), _alone(gen, ctx).codes())


def test_conversation_turn_preempted_mid_turn_and_its_next_turn(world):
    gen, ctx = world["plain"], world["ctx"]

    def dialogue(srv, conv):
        t1 = conv.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=PROBE["frames"] * 80)
        return conv, t1

    plain = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK)
    conv_a, a1 = dialogue(plain, plain.conversation(context=ctx, seed=77))
    _run(plain)
    a2 = conv_a.say("and then the answer", 0, max_audio_length_ms=9 * 80)
    _run(plain)
    assert a1.done and a2.done and a2.codes().shape == (K, 9)
    hold = {}

    def probe():
        hold["conv"], t1 = dialogue(hold["srv"], hold["srv"].conversation(context=ctx, seed=77))
        return t1
    srv = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK, streams=ORDER.STREAMS)
    hold["srv"] = srv

    def other(i):
        return srv.submit("n" * (3 + i % 5), i % 3, [], seed=100 + i, max_audio_length_ms=ORDER.OTHER_FRAMES * 80)
    b1, others = ORDER.submit_all(probe, other)
    while not b1.done:
        srv.step()
    assert b1.preemptions >= 2 and len(set(b1.slots_held)) >= 2
    b2 = hold["conv"].say("and then the answer", 0, max_audio_length_ms=9 * 80)          # the others are still speaking
    assert any(not o.done for o in others)
    _run(srv)
    for a, b in ((a1, b1), (a2, b2)):
        assert torch.equal(b.codes(), a.codes()) and torch.equal(b.audio(), a.audio())
    assert torch.equal(hold["conv"].tokens, conv_a.tokens) and hold["conv"].cached == conv_a.cached


def test_pause_two_steps_then_resume_and_cancel_with_heard_frames(world):
    gen, ctx = world["plain"], world["ctx"]
    a = _alone(gen, ctx)
    srv = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK, streams=ORDER.STREAMS)
    first = srv.submit("somebody before", 0, [], seed=3, max_audio_length_ms=30 * 80)   # (slot 0 is taken: the probe sits in 1)
    b = _submit_probe(srv, ctx)
    srv.step()
    b.pause()
    late = srv.submit("somebody after", 2, [], seed=4, max_audio_length_ms=30 * 80)
    srv.step()
    srv.step()                                                                            # parked; ``late`` has its slot
    assert b.state == "paused" and b.slot is None and b._emitted == 4 and late.slot == 1 and first._emitted == 12
    b.resume()
    _run(srv)
    assert b.preemptions == 1 and b.slots_held == [1, 2]
    assert torch.equal(b.codes(), a.codes()) and torch.equal(b.audio(), a.audio())
    # barge-in: a turn cancelled after 8 frames of which 5 were heard = a turn that was given exactly 5 frames.  History and
    # cache are those of the heard frames; the conversation's noise generator is NOT rewound, so the next turns agree because
    # both sides sampled the same two whole chunks (a conversation's row samples to the end of the chunk its limit falls in:
    # 8 frames here as there) - a cancel after another number of steps leaves the generator elsewhere and other codes follow
    ref = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK)
    conv_a = ref.conversation(context=ctx, seed=77)
    a1 = conv_a.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=5 * 80)
    _run(ref)
    a2 = conv_a.say("and then the answer", 0, max_audio_length_ms=9 * 80)
    _run(ref)
    for streams in (None, ORDER.STREAMS):                                                 # cancel works on every server
        srv = gen.serve(slots=ORDER.SLOTS, chunk_frames=ORDER.CHUNK, temperature=TEMP, topk=TOPK, streams=streams)
        conv_b = srv.conversation(context=ctx, seed=77)
        b1 = conv_b.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=PROBE["frames"] * 80)
        srv.step()
        srv.step()
        assert b1._emitted == 8 and not b1.done
        srv.cancel(b1, heard_frames=5)
        assert b1.done and b1.cancelled and srv.active == []
        assert torch.equal(conv_b.tokens, conv_a.tokens[:conv_b.tokens.shape[0]]) and conv_b.cached == a1._base + 5
        b2 = conv_b.say("and then the answer", 0, max_audio_length_ms=9 * 80)
        _run(srv)
        assert torch.equal(b2.codes(), a2.codes()) and torch.equal(b2.audio(), a2.audio()), streams
        assert torch.equal(conv_b.tokens, conv_a.tokens)


# ---- the rows objects with more state slots than rows of a launch ------------------------------------------------------------
def test_mimi_rows_decoder_with_40_state_slots(world):
    from csm.codec.mimi import MimiDecodeStreamRows
    codec = world["codec"]
    rows = MimiDecodeStreamRows(codec, slots=16, max_chunk_frames=4, state_slots=40)
    assert rows.slots == 16 and rows.state_slots == 40 and rows.kv[0][0].shape[0] == 40
    g = torch.Generator().manual_seed(5)
    T = 11
    codes = {s: torch.randint(0, 2048, (K, T), generator=g).cuda() for s in (37, 0, 39, 16, 5)}
    for s in codes:
        rows.open(s)
    got, at = [], 0
    for n, mates in ((4, [0, 39]), (4, [16]), (3, [5, 0, 39, 16])):                       # slot 37 among changing neighbours
        order = mates[:1] + [37] + mates[1:]
        out = rows.step(order, torch.stack([codes[s][:, rows.pos[s]:rows.pos[s] + n] for s in order]))
        got.append(out[1].clone())
        at += n
    assert at == T and torch.equal(torch.cat(got), codec.decode(codes[37].unsqueeze(0)).reshape(-1))
    with pytest.raises(ValueError, match=r"slot 40 out of range \(0\.\.39\)"):
        rows.open(40)
    with pytest.raises(ValueError, match=r"step takes 1\.\.16 distinct slots in 0\.\.39"):
        rows.step(list(range(17)), torch.zeros(17, K, 1, dtype=torch.long))
    plain = MimiDecodeStreamRows(codec, slots=3, max_chunk_frames=4)                       # None: today's object
    assert plain.state_slots == 3 and plain.kv[0][0].shape[0] == 3
    with pytest.raises(ValueError, match=r"slot 3 out of range \(0\.\.2\)"):
        plain.open(3)


def test_resample_rows_with_40_state_slots(dev):
    from csm.codec.resample import get_resampler
    rs = get_resampler(24000, 48000, "cuda")
    rows = rs.stream_rows(16, 2000, state_slots=40)
    assert rows.slots == 16 and rows.state_slots == 40 and rows._arena.shape[0] == 40
    g = torch.Generator().manual_seed(6)
    xs = {s: torch.randn(4500, generator=g).cuda() for s in (37, 0, 39, 16)}
    for s in xs:
        rows.open(s)
    got = []
    for lo, hi, mates, last in ((0, 1920, [0, 39], False), (1920, 3000, [16], False), (3000, 4500, [39, 16, 0], True)):
        order = mates[:1] + [37] + mates[1:]
        ys = rows.step(order, [xs[s][rows.pos[s]:rows.pos[s] + (hi - lo)] for s in order], final=[37] if last else ())
        got.append(ys[1].clone())
    assert torch.equal(torch.cat(got), rs(xs[37]))
    assert rows.open_slots == [0, 16, 39]
    with pytest.raises(ValueError, match=r"slot 40 out of range \(0\.\.39\)"):
        rows.open(40)
