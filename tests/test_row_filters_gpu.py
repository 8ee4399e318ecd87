"""Per-request top-p / min-p on the GPU (``Generator.serve(row_sampling=True, row_filters=True)``, ``DecodeState.set_row_filters``,
the filtered rows sampler), on the tiny model of tests/test_row_sampling_gpu.py: a server whose requests keep (1, 0) is the
``row_sampling`` server bit for bit; a seeded request with its own four parameters has the same codes alone and among fifteen
others with theirs; ``min_p = 1`` and ``top_p = 1e-6`` are greedy; ``generate_batch`` takes one value per utterance; the defaults
are today's path; a change of parameters replays the same captured graph.  Everything is compared with torch.equal."""
import pytest
import torch

from test_row_sampling_gpu import K, OTHERS, PROBE, _finish, _same, world  # noqa: F401  (world: the module fixture, built here)

pytestmark = pytest.mark.gpu
FILTERS = [(0.9, 0.0), (1.0, 0.05), (0.6, 0.01), (1.0, 0.0), (0.3, 0.0), (0.95, 0.2), (1.0, 1.0), (1e-6, 0.0)]


def test_filters_kept_off_is_the_row_sampling_server(world):
    gen, ctx = world["plain"], world["ctx"]

    def run(**kw):
        srv = gen.serve(slots=16, chunk_frames=4, temperature=0.8, topk=12, row_sampling=True, **kw)
        reqs = [srv.submit("n" * (3 + 2 * i), i % 3, ctx if i == 1 else [], seed=40 + i, max_audio_length_ms=(5 + 3 * i) * 80,
                           **({} if i != 2 else dict(temperature=1.2, topk=200)))
                for i in range(3)]
        srv.step()
        reqs.append(srv.submit("a late one", 1, [], seed=50, max_audio_length_ms=6 * 80))
        _finish(srv)
        assert all(r.done and r.codes().shape == (K, r.max_audio_frames) for r in reqs)
        return srv, reqs
    srv_r, want = run()
    srv_f, got = run(row_filters=True)
    assert srv_r._state.row_filters is None and srv_r._state.graph_key == (None, None)
    assert srv_f._state.row_filters == [(1.0, 0.0)] * 16 and srv_f._state.graph_key == (None, None, "filters")
    for a, b in zip(got, want):
        _same(a, b)


@pytest.mark.parametrize("four", [(0.6, 50, 0.8, 0.02), (1.2, 2051, 0.7, 0.0)])      # the one-wave and the block-wide filter
def test_four_parameters_follow_the_request(world, four):
    gen, ctx = world["banked"], world["ctx"]
    mine = dict(temperature=four[0], topk=four[1], top_p=four[2], min_p=four[3])

    def probe(srv, **kw):
        return srv.submit(PROBE["text"], PROBE["speaker"], ctx, seed=PROBE["seed"], max_audio_length_ms=PROBE["frames"] * 80, **kw)
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True, row_filters=True)      # alone, in slot 0
    a = probe(srv, **mine)
    _finish(srv)
    assert a.done and a.slot is None and a.codes().shape == (K, PROBE["frames"])
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True)                        # ... and the filters do something
    plain = probe(srv, temperature=four[0], topk=four[1])
    _finish(srv)
    assert not torch.equal(plain.codes(), a.codes())
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True, row_filters=True, top_p=0.97, min_p=0.001)

    def other(i):
        t, k = OTHERS[i % len(OTHERS)]
        p, mp = FILTERS[i % len(FILTERS)]
        kw = {} if i % len(OTHERS) == 1 else dict(temperature=t, topk=k, top_p=p, min_p=mp)     # (one in eight names nothing)
        frames = 14 if i == 0 else 3 + (i * 5) % 9                                      # (slot 0 stays taken: the probe sits elsewhere)
        return srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], adapter="a1" if i % 5 == 2 else None,
                          seed=i if i % 2 else None, max_audio_length_ms=frames * 80, **kw)
    others = [other(i) for i in range(15)]
    srv.step()
    b = probe(srv, **mine)
    others += [other(i) for i in range(15, 21)]                                         # these wait for slots
    srv.step()
    st = srv._state
    assert b.slot not in (None, 0) and len(srv.active) >= 8 and srv.queued > 0
    assert st.row_filters[b.slot] == (four[2], four[3]) and len(set(st.row_filters)) >= 5
    row_p, row_m = st.sampler.params[2:4]                                               # [K, B]: every codebook's row of the buffers
    assert torch.equal(row_p.cpu(), torch.tensor([p for p, _ in st.row_filters]).expand(K, -1))
    assert torch.equal(row_m.cpu(), torch.tensor([m_ for _, m_ in st.row_filters]).expand(K, -1))
    _finish(srv)
    assert b.done and all(o.done for o in others) and (b.temperature, b.topk, b.top_p, b.min_p) == four
    _same(b, a)


def test_extreme_filters_are_greedy(world):
    gen, ctx = world["plain"], world["ctx"]
    srv = gen.serve(slots=16, chunk_frames=4, row_sampling=True, row_filters=True)

    def probe(**kw):
        return srv.submit(PROBE["text"], PROBE["speaker"], ctx, seed=PROBE["seed"], max_audio_length_ms=PROBE["frames"] * 80, **kw)
    reqs = [probe(topk=1), probe(min_p=1.0), probe(top_p=1e-6), probe(topk=2051, min_p=1.0), probe(topk=2051, top_p=1e-6), probe()]
    _finish(srv)
    assert all(r.done for r in reqs)
    for r in reqs[1:5]:
        _same(r, reqs[0])
    assert not torch.equal(reqs[5].codes(), reqs[0].codes())


def test_generate_batch_with_one_value_per_utterance(world):
    """Row b of a call with one value per utterance equals row b of the same batch run with row b's four values for everybody
    (unseeded rows draw their noise for the whole batch at once, so it is the batch of the same size that has the same noise)."""
    gen = world["plain"]
    texts, speakers = ["one voice", "another voice here", "a third"], [0, 1, 2]
    fours = [(0.9, 50, 0.8, 0.0), (0.7, 2051, 1.0, 0.05), (0.9, 50, 1.0, 0.0)]

    def run(**kw):
        torch.manual_seed(11)
        return gen.generate_batch(texts, speakers, [[], [], []], max_audio_length_ms=6 * 80, **kw)
    got = run(temperature=[f[0] for f in fours], topk=[f[1] for f in fours], top_p=[f[2] for f in fours], min_p=[f[3] for f in fours])
    st = gen._model._decode_state
    assert st.row_filters == [f[2:] for f in fours] and st.row_sampling == [f[:2] for f in fours]
    for b, f in enumerate(fours):
        ref = run(temperature=f[0], topk=f[1], top_p=f[2], min_p=f[3])
        assert got[b].numel() > 0 and torch.equal(got[b], ref[b]), (b, f)
    plain = run(temperature=0.9, topk=50)                                   # row 2 names (1, 0): the unfiltered codes
    assert gen._model._decode_state.row_filters is None and gen._model._decode_state.row_sampling is None
    assert torch.equal(got[2], plain[2]) and not torch.equal(got[0], plain[0])
    mixed = run(temperature=0.9, topk=50, top_p=[0.8, 1.0, 1.0])            # a number for one of the two
    assert torch.equal(mixed[0], got[0]) and torch.equal(mixed[2], plain[2])


def test_defaults_are_todays_generate(world):
    gen, ctx = world["plain"], world["ctx"]

    def run(fn, **kw):
        torch.manual_seed(5)
        out = fn("say it plainly", 1, ctx, max_audio_length_ms=6 * 80, temperature=0.8, topk=20, **kw)
        return out if torch.is_tensor(out) else torch.cat(list(out))
    want = run(gen.generate)
    got = run(gen.generate, top_p=1.0, min_p=0.0)
    st = gen._model._decode_state
    assert st.row_filters is None and st.row_sampling is None and torch.equal(got, want)
    cut = run(gen.generate, top_p=0.5, min_p=0.05)
    st = gen._model._decode_state
    assert st.row_filters == [(0.5, 0.05)] and st.row_sampling == [(0.8, 20)] and cut.numel() > 0 and not torch.equal(cut, want)
    assert torch.equal(run(gen.generate_stream, top_p=0.5, min_p=0.05), cut)
    assert torch.equal(run(gen.generate_stream, top_p=1.0, min_p=0.0), want)
    conv = gen.conversation(context=ctx)
    torch.manual_seed(5)
    c1 = conv.generate("say it plainly", 1, max_audio_length_ms=6 * 80, temperature=0.8, topk=20, top_p=0.5, min_p=0.05)
    assert conv._state.row_filters == [(0.5, 0.05)] and c1.numel() > 0
    conv2 = gen.conversation(context=ctx)
    torch.manual_seed(5)
    c2 = conv2.generate("say it plainly", 1, max_audio_length_ms=6 * 80, temperature=0.8, topk=20)
    torch.manual_seed(5)
    c3 = gen.conversation(context=ctx).generate("say it plainly", 1, max_audio_length_ms=6 * 80, temperature=0.8, topk=20,
                                                top_p=1.0, min_p=0.0)
    assert conv2._state.row_filters is None and torch.equal(c2, c3) and not torch.equal(c1, c2)


def test_a_change_of_parameters_replays_the_same_graph_and_bad_values_leave_the_server_usable(world):
    gen, m, ctx = world["plain"], world["m"], world["ctx"]
    srv = gen.serve(slots=6, chunk_frames=4, row_sampling=True, row_filters=True)
    st = srv._state
    reqs = [srv.submit("the first", 0, ctx, seed=1, max_audio_length_ms=20 * 80, temperature=0.7, topk=8, top_p=0.9)]
    srv.step()                                     # the tail, one eager frame (warm-up), the captured frame, its first replay
    graph = st.graph
    assert (graph is not None) == getattr(m, "use_hip_graph", True)
    for i, (t, k, p, mp) in enumerate([(1.2, 200, 0.5, 0.0), (0.5, 1, 1.0, 0.0), (0.95, 2051, 0.8, 0.01)]):
        for bad in (dict(top_p=0.0), dict(min_p=float("nan")), dict(top_p=1.01), dict(min_p=-1)):
            with pytest.raises(ValueError, match="top_p must be|min_p must be"):
                srv.submit("refused", 0, [], seed=3, max_audio_length_ms=10 * 80, **bad)
        assert srv.queued == 0
        reqs.append(srv.submit(f"joiner {i}", i % 3, [], seed=10 + i, max_audio_length_ms=(10 + 2 * i) * 80, temperature=t, topk=k,
                               top_p=p, min_p=mp))
        srv.step()
        assert st.graph is graph and reqs[-1].slot == i + 1 and st.row_filters[i + 1] == (p, mp) and st.row_sampling[i + 1] == (t, k)
        if graph is not None:
            assert st.graph_key == (None, None, "filters")
    _finish(srv)
    assert st.graph is graph and all(r.done for r in reqs)
    # the engine's own rule
    from csm.engine import DecodeState
    s3 = DecodeState(m.engine, 3)
    with pytest.raises(RuntimeError, match="set_row_filters first"):
        s3.sampler.need(2)
    assert s3.sampling_args(0.8, 5, top_p=[0.9, 1.0, 0.5]) == (None, None)
    assert s3.row_filters == [(0.9, 0.0), (1.0, 0.0), (0.5, 0.0)] and s3.row_sampling == [(0.8, 5)] * 3
    s3.set_row_filters(1, 0.25, 0.5)
    row_p, row_m = s3.sampler.params[2:4]
    assert row_p.tolist() == [[pytest.approx(0.9), 0.25, 0.5]] * K and row_m.tolist() == [[0.0, 0.5, 0.0]] * K
    with pytest.raises(ValueError, match="one value per row"):
        s3.sampling_args(0.8, 5, top_p=[0.9, 1.0])
    with pytest.raises(ValueError, match="top_p must be"):
        s3.sampling_args(0.8, 5, top_p=[0.9, 1.0, 0.0])
    assert s3.row_filters == [(0.9, 0.0), (0.25, 0.5), (0.5, 0.0)]
