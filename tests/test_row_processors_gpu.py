"""A windowed repetition penalty and per-codebook sampling parameters on the GPU (``Generator.serve(row_sampling=True,
row_processors=True)``, ``DecodeState.set_row_processors``, the processed rows sampler), on the tiny model of
tests/test_row_sampling_gpu.py: a server whose requests keep penalty 1 is the ``row_filters`` server bit for bit; a seeded request
with a penalty and acoustic parameters of its own has the same codes alone and among fifteen others, whoever joins beside it;
each slot's ring holds its request's last 64 frames and a new request in the slot never sees them; a conversation's turn has the
codes it has alone, in whichever slot it resumes; the graph is the eager frame and a change of parameters never recaptures it;
``generate_batch`` rows are their one-utterance runs; the defaults are today's path.  Everything is compared with torch.equal."""
import pytest
import torch

from test_row_sampling_gpu import K, OTHERS, PROBE, _finish, _same, world  # noqa: F401  (world: the module fixture, built here)

pytestmark = pytest.mark.gpu
FILTERS = [(0.9, 0.0), (1.0, 0.05), (0.6, 0.01), (1.0, 0.0), (0.3, 0.0), (0.95, 0.2), (1.0, 1.0), (1e-6, 0.0)]
PENALTIES = [(1.0, 64), (1.3, 16), (2.0, 64), (0.8, 4), (1.1, 0), (1.5, 33), (1.0, 0), (3.0, 1)]
ACOUSTIC_T = [0.7] + [0.55] * (K - 1)             # codebook 0 (semantic), codebooks 1..K-1 (acoustic)
ACOUSTIC_K = [50] + [20] * (K - 1)
MINE = dict(temperature=ACOUSTIC_T, topk=ACOUSTIC_K, top_p=0.9, repetition_penalty=1.3, repetition_window=16)
PROC = dict(row_sampling=True, row_processors=True)


def _probe(srv, ctx, **kw):
    return srv.submit(PROBE["text"], PROBE["speaker"], ctx, seed=PROBE["seed"], max_audio_length_ms=PROBE["frames"] * 80, **kw)


def _mirrors_equal_buffers(st):
    for j, buf in enumerate(st.sampler.params[:6]):                        # (the seventh, typical_p, is not level 3's)
        want = torch.tensor([st.row_processors[b][j] for b in range(st.B)], dtype=buf.dtype).t()
        assert buf.shape == (K, st.B) and torch.equal(buf.cpu(), want), j


def test_penalty_one_is_the_row_filters_server(world):
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
    srv_f, want = run(row_filters=True)
    srv_p, got = run(row_processors=True)
    assert srv_f._state.row_processors is None and srv_f._state.graph_key == (None, None, "filters")
    st = srv_p._state
    assert st.row_processors is not None and st.graph_key == (None, None, "processors")
    assert st.sampler.code_hist.shape == (16, K, 64) and st.sampler.hist_frame.shape == (16,) and st.sampler.hist_live.shape == (16,)
    assert all(r.repetition_penalty == 1.0 and r.repetition_window == 64 for r in got)
    for a, b in zip(got, want):
        _same(a, b)


def test_a_request_has_its_codes_in_any_slot_among_any_neighbours(world):
    gen, ctx = world["banked"], world["ctx"]
    srv = gen.serve(slots=16, chunk_frames=4, **PROC)                                   # alone, in slot 0
    a = _probe(srv, ctx, **MINE)
    _finish(srv)
    assert a.done and a.slot is None and a.codes().shape == (K, PROBE["frames"])
    for change in (dict(repetition_penalty=1.0), dict(temperature=0.7, topk=50)):       # ... the penalty and the acoustic pair matter
        srv = gen.serve(slots=16, chunk_frames=4, **PROC)
        other_run = _probe(srv, ctx, **{**MINE, **change})
        _finish(srv)
        assert not torch.equal(other_run.codes(), a.codes()), change
    srv = gen.serve(slots=16, chunk_frames=4, top_p=0.97, min_p=0.001, repetition_penalty=1.2, repetition_window=32, **PROC)

    def other(i):
        t, k = OTHERS[i % len(OTHERS)]
        p, mp = FILTERS[i % len(FILTERS)]
        r, w = PENALTIES[i % len(PENALTIES)]
        kw = {} if i % len(OTHERS) == 1 else dict(temperature=t, topk=[k] + [max(1, k // 2)] * (K - 1), top_p=p, min_p=mp,
                                                  repetition_penalty=r, repetition_window=w)   # (one in eight names nothing)
        frames = 14 if i == 0 else 3 + (i * 5) % 9                                      # (slot 0 stays taken: the probe sits elsewhere)
        return srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], adapter="a1" if i % 5 == 2 else None,
                          seed=i if i % 2 else None, max_audio_length_ms=frames * 80, **kw)
    others = [other(i) for i in range(15)]
    srv.step()
    b = _probe(srv, ctx, **MINE)
    others += [other(i) for i in range(15, 21)]                                         # these wait for slots ...
    srv.step()
    st = srv._state
    assert b.slot not in (None, 0) and len(srv.active) >= 8 and srv.queued > 0
    waiting = srv.queued
    _mirrors_equal_buffers(st)
    assert st.row_processors[b.slot][0] == tuple(ACOUSTIC_T) and st.row_processors[b.slot][4] == (1.3,) * K
    assert len(set(st.row_processors)) >= 5
    srv.step()                                                                          # ... and join while the probe is mid-utterance
    assert srv.queued < waiting and b.slot is not None and not b.done
    assert int(st.sampler.hist_frame[b.slot]) == b._sampled                                     # (their first-frame tail did not count for it)
    _mirrors_equal_buffers(st)
    _finish(srv)
    assert b.done and all(o.done for o in others)
    assert (b.temperature, b.topk, b.top_p, b.repetition_penalty, b.repetition_window) == (tuple(ACOUSTIC_T), tuple(ACOUSTIC_K), 0.9,
                                                                                          1.3, 16)
    _same(b, a)


def test_ring_holds_the_last_64_frames_and_a_new_request_never_sees_them(world):
    gen, ctx = world["plain"], world["ctx"]
    F = 70
    srv = gen.serve(slots=4, chunk_frames=4, **PROC)
    st = srv._state
    long = srv.submit("a long one", 0, [], seed=7, max_audio_length_ms=F * 80)
    _finish(srv)
    codes = long.codes()
    assert long.done and codes.shape == (K, F) and long._sampled == F
    assert int(st.sampler.hist_frame[0]) == F and st.sampler.hist_frame[1:].tolist() == [0, 0, 0]
    ring = st.sampler.code_hist[0].cpu().long()                                                 # [K, 64]
    for f in range(F - 64, F):
        assert torch.equal(ring[:, f % 64], codes[:, f].cpu()), f
    assert not bool(st.sampler.code_hist[1:].any())                                             # (idle rows wrote nothing)
    second = _probe(srv, ctx, repetition_penalty=1.5, repetition_window=64)             # into slot 0, over the stale ring
    srv.step()
    assert second.slot == 0 and int(st.sampler.hist_frame[0]) == second._sampled == 4
    _finish(srv)
    fresh_srv = gen.serve(slots=4, chunk_frames=4, **PROC)
    fresh = _probe(fresh_srv, ctx, repetition_penalty=1.5, repetition_window=64)
    _finish(fresh_srv)
    _same(second, fresh)
    off_srv = gen.serve(slots=4, chunk_frames=4, **PROC)
    off = _probe(off_srv, ctx)
    _finish(off_srv)
    assert not torch.equal(off.codes(), fresh.codes())


def test_a_conversation_turn_has_its_codes_in_any_slot_and_its_window_is_its_own(world):
    gen, ctx = world["plain"], world["ctx"]
    pen = dict(repetition_penalty=1.6, repetition_window=64, topk=[40] + [15] * (K - 1))

    def talk(srv, busy):
        conv = srv.conversation(context=ctx, seed=21, **pen)
        t1 = conv.say("the first line", 1, max_audio_length_ms=6 * 80)
        _finish(srv)
        blockers = []
        if busy:                                                                        # slots 0, 1 taken: the turn resumes in slot 2
            blockers = [srv.submit("x" * (4 + i), i, [], seed=60 + i, max_audio_length_ms=40 * 80, repetition_penalty=1.2 + i)
                        for i in range(2)]
            srv.step()
        t2 = conv.say("and the second", 1, max_audio_length_ms=9 * 80)
        srv.step()
        slot = t2.slot
        assert int(srv._state.sampler.hist_frame[slot]) == t2._sampled == 4                     # the turn's own frames only
        _finish(srv)
        assert t1.done and t2.done and all(b.done for b in blockers)
        return t1, t2, slot
    a1, a2, slot_a = talk(gen.serve(slots=4, chunk_frames=4, **PROC), busy=False)
    b1, b2, slot_b = talk(gen.serve(slots=4, chunk_frames=4, **PROC), busy=True)
    assert (slot_a, slot_b) == (0, 2)
    _same(b1, a1)
    _same(b2, a2)                                                                       # (slot 2's ring never held turn 1)
    # ... and the penalty does something in the turn
    srv = gen.serve(slots=4, chunk_frames=4, **PROC)
    conv = srv.conversation(context=ctx, seed=21, topk=pen["topk"])
    c1 = conv.say("the first line", 1, max_audio_length_ms=6 * 80)
    _finish(srv)
    assert not torch.equal(c1.codes(), a1.codes())


def test_graph_is_the_eager_frame_and_a_change_never_recaptures(world):
    gen, m, ctx = world["plain"], world["m"], world["ctx"]

    def run():
        srv = gen.serve(slots=6, chunk_frames=4, **PROC)
        st = srv._state
        reqs = [srv.submit("the first", 0, ctx, seed=1, max_audio_length_ms=20 * 80, temperature=0.7, topk=8, top_p=0.9,
                           repetition_penalty=1.3)]
        srv.step()                                 # the tail, one eager frame (warm-up), the captured frame, its first replay
        graph = st.graph
        assert (graph is not None) == getattr(m, "use_hip_graph", True)
        changes = [dict(temperature=1.2), dict(topk=[200] + [3] * (K - 1)), dict(top_p=0.5), dict(min_p=0.02),
                   dict(repetition_penalty=2.5), dict(repetition_window=3)]
        for i, kw in enumerate(changes[:5]):
            reqs.append(srv.submit(f"joiner {i}", i % 3, [], seed=10 + i, max_audio_length_ms=(10 + 2 * i) * 80, **kw))
            srv.step()
            assert st.graph is graph and reqs[-1].slot is not None
            if graph is not None:
                assert st.graph_key == (None, None, "processors")
        for b, kw in enumerate(changes):           # ... and written straight to a running row, between steps
            now = dict(zip(("temperature", "topk", "top_p", "min_p", "repetition_penalty", "repetition_window"), st.row_processors[b]))
            st.set_row_processors(b, **{**now, **kw})
            srv.step()
            assert st.graph is graph
        _mirrors_equal_buffers(st)
        _finish(srv)
        assert st.graph is graph and all(r.done for r in reqs)
        return reqs
    graphed = run()
    was = getattr(m, "use_hip_graph", True)
    m.use_hip_graph = False
    try:
        eager = run()
    finally:
        m.use_hip_graph = was
    for a, b in zip(graphed, eager):
        _same(a, b)


def test_generate_batch_rows_are_their_one_utterance_runs(world):
    gen = world["plain"]
    texts, speakers = ["one voice", "another voice here"], [0, 1]
    temp = [0.8] + [0.6] * (K - 1)

    def noise(seed):
        torch.manual_seed(seed)

    # seeded rows (a server's): each row of two is the row it is alone
    srv = gen.serve(slots=2, chunk_frames=4, **PROC)
    want = [srv.submit(texts[0], 0, [], seed=5, max_audio_length_ms=6 * 80, repetition_penalty=1.4, temperature=temp),
            srv.submit(texts[1], 1, [], seed=6, max_audio_length_ms=6 * 80)]
    _finish(srv)
    alone = []
    for i, kw in enumerate((dict(repetition_penalty=1.4, temperature=temp), {})):
        s1 = gen.serve(slots=1, chunk_frames=4, **PROC)
        alone.append(s1.submit(texts[i], i, [], seed=5 + i, max_audio_length_ms=6 * 80, **kw))
        _finish(s1)
    for a, b in zip(want, alone):
        _same(a, b)
    # generate_batch itself: the values reach the rows, the first utterance's penalty leaves the second's row as it is
    noise(11)
    got = gen.generate_batch(texts, speakers, [[], []], max_audio_length_ms=6 * 80, temperature=[temp, 0.9], topk=50,
                             repetition_penalty=[1.4, 1.0])
    st = gen._model._decode_state
    assert st.graph_key in (None, (None, None, "processors"))
    assert st.row_processors[0][0] == tuple(temp) and st.row_processors[0][4] == (1.4,) * K
    assert st.row_processors[1] == ((0.9,) * K, (50,) * K, (1.0,) * K, (0.0,) * K, (1.0,) * K, (64,) * K)
    assert st.sampler.hist_frame.tolist() == [6, 6] and st.sampler.hist_live.tolist() == [1, 1]
    noise(11)
    base = gen.generate_batch(texts, speakers, [[], []], max_audio_length_ms=6 * 80, temperature=[0.8, 0.9], topk=50)
    assert gen._model._decode_state.row_processors is None
    assert got[0].numel() > 0 and torch.equal(got[1], base[1]) and not torch.equal(got[0], base[0])
    # one utterance: generate with the row's values is the batch's row (B <= 4: rows are batch-invariant), under the row's noise
    for b, kw in enumerate((dict(temperature=temp, repetition_penalty=1.4), dict(temperature=0.9))):
        noise(23)
        one = gen.generate(texts[b], speakers[b], [], max_audio_length_ms=6 * 80, topk=50, **kw)
        noise(23)
        row = gen.generate_batch([texts[b]], [speakers[b]], [[]], max_audio_length_ms=6 * 80, topk=50,
                                 **{k_: [v] for k_, v in kw.items()})
        assert one.numel() > 0 and torch.equal(row[0], one), b


def test_defaults_are_todays_generate_and_the_new_arguments_reach_every_entry_point(world):
    gen, ctx = world["plain"], world["ctx"]

    def run(fn, **kw):
        torch.manual_seed(5)
        out = fn("say it plainly", 1, ctx, max_audio_length_ms=12 * 80, temperature=0.8, topk=20, **kw)
        return out if torch.is_tensor(out) else torch.cat(list(out))
    want = run(gen.generate)
    got = run(gen.generate, repetition_penalty=1.0, repetition_window=64)
    st = gen._model._decode_state
    assert st.row_processors is None and st.row_sampling is None and st.sampler.code_hist is None and torch.equal(got, want)
    assert st.graph_key in (None, (0.8, 20))
    pen = run(gen.generate, repetition_penalty=3.0, repetition_window=48)
    st = gen._model._decode_state
    assert st.row_processors[0][4:] == ((3.0,) * K, (48,) * K) and int(st.sampler.hist_frame[0]) == 12 and pen.numel() > 0
    assert bool(st.sampler.code_hist[0, :, :12].any()) and not bool(st.sampler.code_hist[0, :, 12:].any())      # the ring took the twelve frames
    assert torch.equal(run(gen.generate_stream, repetition_penalty=3.0, repetition_window=48), pen)
    assert torch.equal(run(gen.generate_stream, repetition_penalty=1.0), want)
    torch.manual_seed(5)
    per = gen.generate("say it plainly", 1, ctx, max_audio_length_ms=12 * 80, temperature=[0.8] + [0.5] * (K - 1), topk=20)
    assert gen._model._decode_state.row_processors[0][0] == (0.8,) + (0.5,) * (K - 1) and not torch.equal(per, want)
    conv = gen.conversation(context=ctx)
    torch.manual_seed(5)
    c1 = conv.generate("say it plainly", 1, max_audio_length_ms=12 * 80, temperature=0.8, topk=20, repetition_penalty=3.0,
                       repetition_window=48)
    assert conv._state.row_processors[0][4] == (3.0,) * K and c1.numel() > 0
    torch.manual_seed(6)
    conv.generate("and again", 1, max_audio_length_ms=5 * 80, temperature=0.8, topk=20, repetition_penalty=3.0, repetition_window=48)
    assert int(conv._state.sampler.hist_frame[0]) == 5                               # the second turn counted from 0
    conv2 = gen.conversation(context=ctx)
    torch.manual_seed(5)
    c2 = conv2.generate("say it plainly", 1, max_audio_length_ms=12 * 80, temperature=0.8, topk=20)
    assert conv2._state.row_processors is None and c2.numel() > 0


def test_refusals(world):
    gen, m, ctx = world["plain"], world["m"], world["ctx"]
    with pytest.raises(ValueError, match="row_sampling=True"):
        gen.serve(slots=2, row_processors=True)
    with pytest.raises(ValueError, match="row_processors=True"):
        gen.serve(slots=2, row_sampling=True, row_filters=True, repetition_penalty=1.3)
    srv = gen.serve(slots=2, chunk_frames=4, row_sampling=True, row_filters=True)
    conv = srv.conversation()
    for kw in (dict(repetition_penalty=1.3), dict(repetition_window=16), dict(temperature=[0.9] * K)):
        with pytest.raises(ValueError, match="row_processors=True"):
            srv.submit("a", 0, [], **kw)
        with pytest.raises(ValueError, match="row_processors=True"):
            srv.conversation(**kw)
        with pytest.raises(ValueError, match="row_processors=True"):
            conv.say("a", 0, **kw)
    srv = gen.serve(slots=2, chunk_frames=4, **PROC)
    conv = srv.conversation()
    bad = [dict(repetition_penalty=0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=101), dict(repetition_window=65),
           dict(repetition_window=-1), dict(repetition_window=2.5), dict(temperature=[0.9] * (K - 1)), dict(topk=[5] * (K + 1)),
           dict(top_p=[0.9] * 3), dict(repetition_penalty=[1.3] * (K + 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            srv.submit("a", 0, [], **kw)
        with pytest.raises(ValueError):
            conv.say("a", 0, **kw)
        for fn in (gen.generate, gen.generate_stream):
            with pytest.raises(ValueError):
                out = fn("a", 0, [], max_audio_length_ms=3 * 80, **kw)
                if not torch.is_tensor(out):
                    list(out)
        srv._check()                                                          # (a refused generate took nothing over)
    assert srv.queued == 0
    r = srv.submit("still usable", 0, [], seed=1, max_audio_length_ms=3 * 80, repetition_penalty=1.3)
    _finish(srv)
    assert r.done and r.codes().shape == (K, 3)
    # the recompute path has neither
    was = getattr(m, "use_kv_cache", True)
    m.use_kv_cache = False
    try:
        for kw in (dict(repetition_penalty=1.3), dict(repetition_window=8), dict(temperature=[0.9] * K)):
            with pytest.raises(ValueError, match="recompute path"):
                gen.generate("a", 0, [], max_audio_length_ms=2 * 80, **kw)
    finally:
        m.use_kv_cache = was
    # the engine's own rules
    from csm.engine import DecodeState
    s3 = DecodeState(m.engine, 3)
    with pytest.raises(RuntimeError, match="set_row_processors first"):
        s3.reset_row_history(0)
    assert s3.sampling_args(0.8, 5) == (0.8, 5) and s3.row_processors is None
    assert s3.sampling_args(0.8, 5, repetition_penalty=[1.3, 1.0, 2.0]) == (None, None)
    assert [p[4][0] for p in s3.row_processors] == [1.3, 1.0, 2.0] and s3.sampler.params[4].shape == (K, 3)
    with pytest.raises(ValueError, match="one entry per row"):
        s3.sampling_args(0.8, 5, repetition_penalty=[1.3, 1.0])
    with pytest.raises(ValueError, match="repetition_window must be"):
        s3.sampling_args(0.8, 5, repetition_window=[1, 2, 65])
    assert [p[5][0] for p in s3.row_processors] == [64, 64, 64]             # (all checked before any is written)
    s3.set_row_processors(1, 0.8, 5, 1.0, 0.0, [1.0 + 0.01 * i for i in range(K)], 7)
    assert s3.sampler.params[4][:, 1].cpu().tolist() == pytest.approx([1.0 + 0.01 * i for i in range(K)])
    assert s3.sampler.params[4][:, 0].cpu().tolist() == pytest.approx([1.3] * K) and s3.sampler.params[5][:, 1].tolist() == [7] * K
