"""The running batch on the GPU (Generator.serve, csm/serving.py): a seeded request's codes and audio do not depend on its slot,
its neighbours or when it joined, and they are the codes of the existing paths - the engine's batched frames (B in 5..16), a
one-utterance run (slots <= 4), the per-row adapter batch and the FP8 batch - driven with the noise its seed stands for.
Everything is compared with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K, V = 32, 2051
TEMP, TOPK = 0.8, 12
ALL7 = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]
PROBE = dict(text="the line we follow", speaker=1, seed=1234, frames=14)        # 14 frames: ends inside a chunk of 4


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


def _hf_mimi(seed=0):
    from transformers import MimiConfig, MimiModel
    torch.manual_seed(seed)
    m = MimiModel(MimiConfig()).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith("embed_sum"):
                buf.copy_(torch.randn(buf.shape, generator=g))
        for mod in m.modules():
            if hasattr(mod, "_embed"):
                mod._embed = None
        for name, p in m.named_parameters():
            if name.endswith("layer_scale.scale"):
                p.copy_(0.5 + 0.1 * torch.randn(p.shape, generator=g))
    return m


def _adapter(m, seed, r=8, alpha=16.0, b_scale=0.05):
    """A generation-only adapter set of ``m`` with non-zero B."""
    from csm.training.lora import LoRAState
    st = LoRAState(m, r, alpha, 0.0, list(ALL7), None, False, seed=seed, grad=False)
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    with torch.no_grad():
        for ad in st.adapters.values():
            ad.B[:, :r].copy_((torch.randn(ad.B.shape[0], r, generator=g, device="cuda") * b_scale).to(BF))
    return st


@pytest.fixture(scope="module")
def world(dev):
    from csm.codec import MimiCodec
    from csm.generator import Generator, Segment
    from csm.models.model import Model, ModelArgs
    codec = MimiCodec(_hf_mimi().state_dict(), device="cuda")
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=2)
    plain = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)                 # no adapter bank
    banked = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)
    states = {"a1": _adapter(m, 1), "a2": _adapter(m, 2)}
    for name, st in states.items():
        banked.add_adapter(name, st)
    ctx = [Segment(0, "hi", torch.randn(24000, generator=torch.Generator().manual_seed(1)) * 0.2)]
    return dict(m=m, codec=codec, plain=plain, banked=banked, states=states, ctx=ctx)


def _probe(srv, ctx, adapter=None):
    return srv.submit(PROBE["text"], PROBE["speaker"], ctx, adapter=adapter, seed=PROBE["seed"],
                      max_audio_length_ms=PROBE["frames"] * 80)


def _alone(gen, ctx, slots=16, adapter=None):
    srv = gen.serve(slots=slots, chunk_frames=4, temperature=TEMP, topk=TOPK)
    r = _probe(srv, ctx, adapter)
    chunks = [(a.numel(), d) for _, a, d in srv.run()]
    assert r.done and r.codes().shape == (K, PROBE["frames"])
    assert chunks == [(4 * 1920, False)] * 3 + [(2 * 1920, True)]
    return r


def _seed_noise(seed, frames):
    """The noise a request's seed stands for (DecodeState.fill_noise): per frame ONE [K, V] Exp(1) draw from its own generator."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.empty(K, V, dtype=torch.float32, device="cuda").exponential_(1, generator=g) for _ in range(frames)]


def _drive(m, req, B, adapters=None):
    """The existing path: ``Engine.generate_first_frames`` / ``generate_frame(noise=...)`` on B copies of the request's prompt,
    row 0 with the request's noise and the other rows with noise of their own.  Returns row 0's codes [K, frames]."""
    q = _seed_noise(req.seed, req.max_audio_frames)
    tk, mk = req._tokens, req._mask

    def noise(f):
        g = torch.Generator(device="cuda").manual_seed(9000 + f)
        full = torch.empty(K, B, V, dtype=torch.float32, device="cuda").exponential_(1, generator=g)
        full[:, 0] = q[f]
        return list(full)

    m.setup_caches(B)
    m.reset_caches()
    amask = torch.cat([torch.ones(B, 1, K, dtype=torch.bool), torch.zeros(B, 1, 1, dtype=torch.bool)], 2).cuda()
    out = [m.engine.generate_first_frames([tk] * B, [mk] * B, TEMP, TOPK, noise=noise(0), adapters=adapters)]
    for f in range(1, req.max_audio_frames):
        cur = torch.cat([out[-1].long(), torch.zeros(B, 1, dtype=torch.long, device="cuda")], 1).unsqueeze(1)
        out.append(m.generate_frame(cur, amask, torch.ones(B, 1, dtype=torch.long), TEMP, TOPK, noise=noise(f)))
    m.reset_caches()
    return torch.stack([o[0] for o in out], 1).long()


def test_request_does_not_depend_on_slot_neighbours_or_join_time(world):
    gen, ctx, codec = world["banked"], world["ctx"], world["codec"]
    a = _alone(gen, ctx)                                                              # run A: alone, slot 0
    assert torch.equal(a.audio(), codec.decode(a.codes().unsqueeze(0)).reshape(-1))   # the chunks are decode()'s audio
    # run B: 15 others first - different prompt lengths, lengths (rows leave at different times) and adapters - then the probe
    # and more others, which wait for slots
    srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)
    names = [None, "a1", "a2", None]

    def other(i):
        frames = 20 if i == 0 else 3 + (i * 5) % 17                                   # (slot 0 stays taken: the probe sits elsewhere)
        return srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], adapter=names[i % 4], seed=i if i % 2 else None,
                          max_audio_length_ms=frames * 80)
    others = [other(i) for i in range(15)]
    srv.step()
    srv.step()
    assert any(o.done for o in others) and not all(o.done for o in others)
    b = _probe(srv, ctx)
    others += [other(i) for i in range(15, 22)]
    srv.step()
    slot, neighbours = b.slot, len(srv.active)
    assert slot not in (None, 0) and neighbours >= 12
    for _ in srv.run():
        pass
    assert b.done and all(o.done for o in others) and srv.queued == 0
    assert all(o.codes().shape[1] == o.max_audio_frames for o in others)
    wide = sum(int((o.codes() >= 2048).sum()) for o in others + [b])
    print(f"ids >= 2048 (outside Mimi's codebooks) among {sum(o.codes().numel() for o in others + [b])} served codes: {wide}")
    assert torch.equal(b.codes(), a.codes()), f"codes differ between slot 0 alone and slot {slot} among {neighbours}"
    assert torch.equal(b.audio(), a.audio())
    # an adapter changes what is said (otherwise the adapter rows above test nothing)
    c = _alone(gen, ctx, adapter="a1")
    assert not torch.equal(c.codes(), a.codes())


def test_server_row_equals_engine_batch_frames(world):
    """Anchor to the existing path at a batch size in 5..16 (the MFMA products give a row the same bits for any of them)."""
    a = _alone(world["banked"], world["ctx"])
    assert torch.equal(a.codes(), _drive(world["m"], a, 6))
    a = _alone(world["plain"], world["ctx"], slots=9)
    assert torch.equal(a.codes(), _drive(world["m"], a, 16))


def test_small_server_equals_one_utterance_run(world):
    """slots <= 4 and no adapters: the rows are those of a one-row launch."""
    gen, ctx = world["plain"], world["ctx"]
    srv = gen.serve(slots=3, chunk_frames=4, temperature=TEMP, topk=TOPK)
    srv.submit("somebody else", 0, [], seed=5, max_audio_length_ms=9 * 80)
    srv.submit("and a third voice here", 2, ctx, max_audio_length_ms=30 * 80)
    srv.step()
    b = _probe(srv, ctx)
    for _ in srv.run():
        pass
    assert b.done and b.codes().shape == (K, PROBE["frames"])
    assert torch.equal(b.codes(), _drive(world["m"], b, 1))


def test_adapter_row_equals_adapter_batch(world):
    """A request with an adapter: the per-row adapter batch (what generate_batch(adapters=[...]) runs) with the same noise."""
    st = world["states"]
    c = _alone(world["banked"], world["ctx"], adapter="a2")
    ref = _drive(world["m"], c, 6, adapters=[st["a2"], None, st["a1"], st["a2"], None, None])
    assert torch.equal(c.codes(), ref)


def test_fp8_server_row_equals_fp8_batch(world):
    m, gen = world["m"], world["plain"]
    m.decode_weights = "fp8"
    try:
        a = _alone(gen, world["ctx"])
        assert torch.equal(a.codes(), _drive(m, a, 6))
        with pytest.raises(ValueError, match="fp8"):
            world["banked"].serve()                                                  # adapters in play: bf16 only, as today
    finally:
        m.decode_weights = "bf16"
    b = _alone(gen, world["ctx"])
    assert not torch.equal(a.codes(), b.codes())                                      # (FP8 weights change what is said)


def test_row_pos_is_the_one_host_mirror_of_the_device_positions(world):
    """``DecodeState.row_pos`` follows the device position vector through every way a state is filled and advanced - also a
    multi-row state filled by ``prefill`` - and ``cur`` is its maximum; a row at the length limit refuses its frame and moves
    nothing, while the other rows still decode."""
    from csm.engine import DecodeState
    m = world["m"]
    e = m.engine
    amask = torch.cat([torch.ones(2, 1, K, dtype=torch.bool), torch.zeros(2, 1, 1, dtype=torch.bool)], 2).cuda()

    def text_prompt(*shape, seed):
        tk = torch.zeros(*shape, K + 1, dtype=torch.long)
        tk[..., -1] = torch.randint(3, 200, shape, generator=torch.Generator().manual_seed(seed))
        mk = torch.zeros(*shape, K + 1, dtype=torch.bool)
        mk[..., -1] = True
        return tk.cuda(), mk.cuda()

    def frame_input(codes):
        return torch.cat([codes.long(), torch.zeros(2, 1, dtype=torch.long, device="cuda")], 1).unsqueeze(1)

    def mirrored(st):
        assert st.row_pos == st.bb.pos.tolist() and st.cur == max(st.row_pos)

    # frames after prefill, with the graph (eager, capture, replay) and without
    st = DecodeState(e, 2)
    assert st.cur == -1
    last_h = st.prefill(*text_prompt(2, 5, seed=3))
    mirrored(st)
    assert st.row_pos == [4, 4]
    out = e._frame_tail(st, last_h, TEMP, TOPK, None)
    m._decode_state = st
    try:
        for graph in (True, False):
            m.use_hip_graph = graph
            for _ in range(3):
                out = e.generate_frame(frame_input(out), amask, torch.ones(2, 1, dtype=torch.long), TEMP, TOPK)
                mirrored(st)
        assert st.row_pos == [10, 10] and st.graph is not None
    finally:
        m.use_hip_graph = True
        m.reset_caches()
    # park_row on the prefill-filled state
    n = st.row_pos[1] + 1
    assert st.park_row(1, n).shape[3] == n
    with pytest.raises(ValueError, match="park_row"):
        st.park_row(1, n + 1)
    # rows at the length limit
    limit = m.bb.max_seq_len
    st = DecodeState(e, 2)
    st.prefill_row(0, *text_prompt(limit, seed=4))
    last = st.prefill_row(1, *text_prompt(5, seed=5))
    mirrored(st)
    assert st.row_pos == [limit - 1, 4]
    out = st.serve_first(torch.stack([last, last]), [0, 1], TEMP, TOPK)
    try:
        for graph in (True, False):
            m.use_hip_graph = graph
            with pytest.raises(ValueError, match="exceeds max_seq_len"):
                st.serve_frame(frame_input(out), amask, TEMP, TOPK)
            assert st.row_pos == [limit - 1, 4]
        st.set_active([1])
        st.serve_frame(frame_input(out), amask, TEMP, TOPK)
        assert st.row_pos == [limit - 1, 5] and int(st.bb.pos[1]) == 5
    finally:
        m.use_hip_graph = True
