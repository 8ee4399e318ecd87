"""Per-request sampling parameters on the GPU (``Generator.serve(row_sampling=True)``, ``DecodeState.set_row_sampling``, the rows
sampler): a request sampled with its own (temperature, topk) among fifteen others with theirs has the codes and audio it has
alone on a default server made with that pair; a server whose requests name nothing is the default server bit for bit; a change
of parameters replays the same captured graph; the engine's frames and ``generate_batch`` take one value per row.  Everything is
compared with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K, V = 32, 2051
TEMP, TOPK = 0.8, 12
ALL7 = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]
PROBE = dict(text="the line we follow", speaker=1, seed=1234, frames=10)        # 10 frames: ends inside a chunk of 4


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
    banked.add_adapter("a1", _adapter(m, 1))
    ctx = [Segment(0, "hi", torch.randn(24000, generator=torch.Generator().manual_seed(1)) * 0.2)]
    return dict(m=m, codec=codec, plain=plain, banked=banked, ctx=ctx)


def _finish(srv):
    for _ in srv.run():
        pass


def _same(a, b):
    assert torch.equal(a.codes(), b.codes()), (a.id, a.codes()[:4, :6], b.codes()[:4, :6])
    assert torch.equal(a.audio(), b.audio())


@pytest.mark.parametrize("slots", [16, 2])
def test_nothing_named_is_the_default_server(world, slots):
    gen, ctx = world["plain"], world["ctx"]

    def run(**kw):
        srv = gen.serve(slots=slots, chunk_frames=4, temperature=TEMP, topk=TOPK, **kw)
        reqs = [srv.submit("n" * (3 + 2 * i), i % 3, ctx if i == 1 else [], seed=40 + i, max_audio_length_ms=(5 + 3 * i) * 80)
                for i in range(3)]
        srv.step()
        reqs.append(srv.submit("a late one", 1, [], seed=50, max_audio_length_ms=6 * 80))
        _finish(srv)
        assert all(r.done and r.codes().shape == (K, r.max_audio_frames) for r in reqs)
        return srv, reqs
    srv_d, want = run()
    srv_r, got = run(row_sampling=True)
    assert srv_d._state.row_sampling is None and srv_d._state.graph_key == (TEMP, TOPK)
    assert srv_r._state.row_sampling == [(TEMP, TOPK)] * slots and srv_r._state.graph_key == (None, None)
    for a, b in zip(got, want):
        _same(a, b)


OTHERS = [(0.5, 1), (0.9, 50), (1.3, 65), (0.7, 200), (1.0, 12), (0.8, 64), (1.1, 2051), (0.6, 1)]


@pytest.mark.parametrize("pair", [(0.6, 5), (1.2, 200)])                   # the one-wave and the block-wide finish
def test_parameters_follow_the_request(world, pair):
    gen, ctx = world["banked"], world["ctx"]

    def probe(srv, **kw):
        return srv.submit(PROBE["text"], PROBE["speaker"], ctx, seed=PROBE["seed"], max_audio_length_ms=PROBE["frames"] * 80, **kw)
    srv = gen.serve(slots=16, chunk_frames=4, temperature=pair[0], topk=pair[1])        # alone on a default server made with the pair
    a = probe(srv)
    _finish(srv)
    assert a.done and a.codes().shape == (K, PROBE["frames"])
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True)                        # (the server's own pair: 0.9 / 50)

    def other(i):
        t, k = OTHERS[i % len(OTHERS)]
        kw = {} if i % len(OTHERS) == 1 else dict(temperature=t, topk=k)                # (one in eight names nothing)
        frames = 14 if i == 0 else 3 + (i * 5) % 9                                      # (slot 0 stays taken: the probe sits elsewhere)
        return srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], adapter="a1" if i % 5 == 2 else None,
                          seed=i if i % 2 else None, max_audio_length_ms=frames * 80, **kw)
    others = [other(i) for i in range(15)]
    srv.step()
    b = probe(srv, temperature=pair[0], topk=pair[1])
    others += [other(i) for i in range(15, 21)]                                         # these wait for slots
    srv.step()
    assert b.slot not in (None, 0) and srv.last_join_rows == 4 and len(srv.active) >= 8 and srv.queued > 0     # (it joined 12 others)
    assert srv._state.row_sampling[b.slot] == pair and len(set(srv._state.row_sampling)) >= 6
    row_t, row_k = srv._state.sampler.params[:2]                                        # [K, B]: every codebook's row of the buffers
    assert row_k.tolist() == [[k for _, k in srv._state.row_sampling]] * K
    assert torch.equal(row_t.cpu(), torch.tensor([t for t, _ in srv._state.row_sampling]).expand(K, -1))
    _finish(srv)
    assert b.done and all(o.done for o in others) and (b.temperature, b.topk) == pair
    _same(b, a)
    greedy = [o for o in others if o.topk == 1]
    assert greedy and all(o.codes().shape[1] == o.max_audio_frames for o in others)


def test_a_change_of_parameters_replays_the_same_graph(world):
    gen, m, ctx = world["plain"], world["m"], world["ctx"]

    def run():
        srv = gen.serve(slots=6, chunk_frames=4, row_sampling=True)
        st = srv._state
        reqs = [srv.submit("the first", 0, ctx, seed=1, max_audio_length_ms=20 * 80, temperature=0.7, topk=8)]
        srv.step()                                 # the tail, one eager frame (warm-up), the captured frame, its first replay
        graph = st.graph
        assert (graph is not None) == getattr(m, "use_hip_graph", True)
        for i, (t, k) in enumerate([(1.2, 200), (0.5, 1), (0.95, 65)]):
            reqs.append(srv.submit(f"joiner {i}", i % 3, [], seed=10 + i, max_audio_length_ms=(10 + 2 * i) * 80, temperature=t, topk=k))
            srv.step()
            assert st.graph is graph and reqs[-1].slot == i + 1 and st.row_sampling[i + 1] == (t, k)
            if graph is not None:
                assert st.graph_key == (None, None)
        _finish(srv)
        assert st.graph is graph and all(r.done for r in reqs)
        return reqs
    with_graph = run()
    m.use_hip_graph = False
    try:
        eager = run()
    finally:
        m.use_hip_graph = True
    for a, b in zip(with_graph, eager):
        _same(a, b)


def test_engine_frames_take_one_pair_per_row(world):
    m = world["m"]
    e = m.engine
    B, frames = 5, 4
    pairs = [(0.9, 50), (0.6, 1), (1.2, 200), (0.9, 50), (0.7, 65)]
    g = torch.Generator().manual_seed(7)
    toks, msks = [], []
    for b in range(B):
        tk = torch.zeros(4 + b, K + 1, dtype=torch.long)
        tk[:, -1] = torch.randint(3, 200, (4 + b,), generator=g)
        mk = torch.zeros(4 + b, K + 1, dtype=torch.bool)
        mk[:, -1] = True
        toks.append(tk.cuda())
        msks.append(mk.cuda())
    gq = torch.Generator(device="cuda").manual_seed(8)
    noise = [list(torch.empty(K, B, V, dtype=torch.float32, device="cuda").exponential_(1, generator=gq)) for _ in range(frames)]
    amask = torch.cat([torch.ones(B, 1, K, dtype=torch.bool), torch.zeros(B, 1, 1, dtype=torch.bool)], 2).cuda()

    def run(temperature, topk):
        m.setup_caches(B)
        m.reset_caches()
        out = [e.generate_first_frames(toks, msks, temperature, topk, noise=noise[0])]
        for f in range(1, frames):                                          # eager (warm-up), captured, replayed
            cur = torch.cat([out[-1].long(), torch.zeros(B, 1, dtype=torch.long, device="cuda")], 1).unsqueeze(1)
            out.append(m.generate_frame(cur, amask, torch.ones(B, 1, dtype=torch.long), temperature, topk, noise=noise[f]))
        st = m._decode_state
        m.reset_caches()
        return torch.stack(out, 2), st                                      # [B, K, frames]
    got, st = run([t for t, _ in pairs], torch.tensor([k for _, k in pairs]))
    assert st.row_sampling == pairs and st.graph_key == (None, None) and st.graph is not None
    ref = {p: run(*p)[0] for p in set(pairs)}
    for b, p in enumerate(pairs):
        assert torch.equal(got[b], ref[p][b]), (b, p)
    assert not torch.equal(ref[(0.9, 50)][1], ref[(0.6, 1)][1])           # (the pair changes what a row says)
    # a number for one of the two holds for every row; the rule of set_row_sampling; the recompute path refuses
    from csm.engine import DecodeState
    st = DecodeState(e, 3)
    assert st.sampling_args(0.8, [5, 6, 7]) == (None, None) and st.row_sampling == [(0.8, 5), (0.8, 6), (0.8, 7)]
    st.set_row_sampling(1, 1.25, 2051)
    row_t, row_k = st.sampler.params[:2]                                    # [K, B]: every codebook's row of the buffers
    assert row_k.tolist() == [[5, 2051, 7]] * K and row_t.tolist() == [[pytest.approx(0.8), 1.25, pytest.approx(0.8)]] * K
    assert st.sampling_args(0.9, 50) == (0.9, 50) and st.sampling_args(None, None) == (None, None)
    for t, k in ((0.0, 5), (float("nan"), 5), (float("inf"), 5), (-1.0, 5), (0.9, 0), (0.9, 2052), (0.9, 2.5)):
        with pytest.raises(ValueError, match="temperature must be|topk must be"):
            st.set_row_sampling(0, t, k)
    with pytest.raises(ValueError, match="one value per row"):
        st.sampling_args([0.9, 0.8], 5)
    assert st.row_sampling == [(0.8, 5), (1.25, 2051), (0.8, 7)]
    with pytest.raises(RuntimeError, match="set_row_sampling first"):
        DecodeState(e, 2).sampler.draw(None, 0, None)                      # (what a frame body called with None, None does)
    m.use_kv_cache = False
    try:
        with pytest.raises(ValueError, match="per-row sampling parameters need the KV-cache path"):
            m.generate_frame(toks[0].unsqueeze(0), msks[0].unsqueeze(0), torch.arange(4).unsqueeze(0), [0.9], [50])
    finally:
        m.use_kv_cache = True
        m.reset_caches()


def test_generate_batch_with_one_pair_per_utterance(world):
    gen = world["plain"]
    texts, speakers = ["one voice", "another voice here", "a third"], [0, 1, 2]
    pairs = [(0.9, 50), (0.6, 1), (0.9, 50)]

    def run(temperature, topk):
        torch.manual_seed(11)                                               # (unseeded rows: the whole-buffer draw of the global generator)
        return gen.generate_batch(texts, speakers, [[], [], []], max_audio_length_ms=6 * 80, temperature=temperature, topk=topk)
    got = run([t for t, _ in pairs], [k for _, k in pairs])
    assert gen._model._decode_state.row_sampling == pairs
    ref = {p: run(*p) for p in set(pairs)}
    assert gen._model._decode_state.row_sampling is None                    # two numbers: the one-pair path
    for b, p in enumerate(pairs):
        assert got[b].numel() > 0 and torch.equal(got[b], ref[p][b]), (b, p)
    mixed = run(0.9, [50, 1, 50])                                           # a number for one of the two
    assert torch.equal(mixed[0], ref[(0.9, 50)][0]) and torch.equal(mixed[1], ref[(0.6, 1)][1])    # (greedy: any temperature)


def test_conversation_keeps_its_pair_from_slot_to_slot(world):
    from csm.generator import Segment
    gen = world["plain"]
    ctx = [Segment(0, "hi", torch.randn(5 * 1920, generator=torch.Generator().manual_seed(3)) * 0.2)]
    MS = 6 * 80

    def turn(srv, conv, text, **kw):
        r = conv.say(text, 0, max_audio_length_ms=MS, **kw)
        srv.step()
        slot = r.slot
        while not r.done:
            srv.step()
        assert r.codes().shape == (K, 6)
        return r, slot
    # alone on a default server made with the conversation's pair
    srv = gen.serve(slots=16, chunk_frames=4, temperature=0.7, topk=8)
    conv = srv.conversation(context=ctx, seed=77)
    want = [turn(srv, conv, "one"), turn(srv, conv, "two two")]
    assert [s for _, s in want] == [0, 0]
    # on a row_sampling server (0.9 / 50) with slot 0 taken between its turns
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True)
    conv = srv.conversation(context=ctx, seed=77, temperature=0.7, topk=8)
    t1, s1 = turn(srv, conv, "one")
    blocker = srv.submit("somebody else", 2, [], seed=5, max_audio_length_ms=40 * 80, temperature=1.3, topk=200)
    srv.step()
    assert s1 == 0 and blocker.slot == 0
    t2, s2 = turn(srv, conv, "two two")
    assert s2 == 1 and srv._state.row_sampling[:2] == [(1.3, 200), (0.7, 8)]
    _same(t1, want[0][0])
    _same(t2, want[1][0])
    # a turn that names its own: say > conversation.  Its history (tokens and parked K / V) goes to a default topk = 1 server
    hist = dict(_tokens=conv.tokens.clone(), _mask=conv.mask.clone(), _turns=list(conv._turns), _cached=conv.cached,
                _parked=conv._parked.clone())
    t3, s3 = turn(srv, conv, "three", topk=1)
    assert s3 == 1 and (t3.temperature, t3.topk) == (0.7, 1) and srv._state.row_sampling[1] == (0.7, 1)
    assert not blocker.done
    srv = gen.serve(slots=16, chunk_frames=4, temperature=0.7, topk=1)
    conv = srv.conversation(seed=77)
    for name, value in hist.items():
        setattr(conv, name, value)
    r3, s = turn(srv, conv, "three")
    assert s == 0
    _same(t3, r3)
    assert not torch.equal(t3.codes(), t2.codes())
