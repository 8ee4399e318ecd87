"""Locally typical sampling per request on the GPU (``Generator.serve(row_sampling=True, row_typical=True)``,
``DecodeState.set_row_typical``, the typical rows sampler), on the tiny model of tests/test_row_sampling_gpu.py: a server whose
requests keep ``typical_p = 1`` is the ``row_processors`` server bit for bit; a seeded request at 0.2 has the same codes alone, in
another slot among fifteen neighbours with other values, as a served conversation's first turn and through ``generate``; they differ
from its codes at 1; every code of one frame lies in the float64 reference's typical set for that draw's logits; a change of
``typical_p`` replays the same captured frame; per-codebook values reach the buffer.  Codes are compared with torch.equal."""
import pytest
import torch

import sampling_typical_ref as T
from test_row_sampling_gpu import K, OTHERS, PROBE, _finish, _same, world  # noqa: F401  (world: the module fixture, built here)

pytestmark = pytest.mark.gpu
TYP = dict(row_sampling=True, row_typical=True)
TYPICALS = [0.9, 1.0, 0.5, 0.05, [0.3] + [0.95] * (K - 1), 0.99, 1e-6, 0.7]
MINE = dict(temperature=0.9, topk=50, typical_p=0.2)


def _probe(srv, ctx, **kw):
    return srv.submit(PROBE["text"], PROBE["speaker"], ctx, seed=PROBE["seed"], max_audio_length_ms=PROBE["frames"] * 80, **kw)


def _mirror_equals_buffer(st):
    want = torch.tensor([st.row_typical[b][6] for b in range(st.B)], dtype=torch.float32).t()
    assert st.sampler.params[6].shape == (K, st.B) and torch.equal(st.sampler.params[6].cpu(), want)
    for j, buf in enumerate(st.sampler.params):
        want = torch.tensor([st.row_typical[b][j] for b in range(st.B)], dtype=buf.dtype).t()
        assert torch.equal(buf.cpu(), want), j


def test_typical_p_one_is_the_row_processors_server(world):
    gen, ctx = world["plain"], world["ctx"]

    def run(**kw):
        srv = gen.serve(slots=16, chunk_frames=4, temperature=0.8, topk=12, row_sampling=True, repetition_penalty=1.3,
                        repetition_window=16, **kw)
        reqs = [srv.submit("n" * (3 + 2 * i), i % 3, ctx if i == 1 else [], seed=40 + i, max_audio_length_ms=(5 + 3 * i) * 80,
                           **({} if i != 2 else dict(temperature=1.2, topk=200, top_p=0.9)))
                for i in range(3)]
        srv.step()
        reqs.append(srv.submit("a late one", 1, [], seed=50, max_audio_length_ms=6 * 80))
        _finish(srv)
        assert all(r.done and r.codes().shape == (K, r.max_audio_frames) for r in reqs)
        return srv, reqs
    srv_p, want = run(row_processors=True)
    srv_t, got = run(row_typical=True)
    assert srv_p._state.row_typical is None and srv_p._state.graph_key == (None, None, "processors")
    st = srv_t._state
    assert srv_t.row_typical and srv_t.row_processors and srv_t.row_filters
    assert st.row_typical is not None and st.row_processors is None and st.graph_key == (None, None, "typical")
    assert st.sampler.level == 4 and st.sampler.params[6].shape == (K, 16) and bool((st.sampler.params[6] == 1.0).all())
    assert all(r.typical_p == 1.0 for r in got)
    for a, b in zip(got, want):
        _same(a, b)


def test_a_request_has_its_codes_in_any_slot_as_a_first_turn_and_through_generate(world):
    gen, ctx = world["banked"], world["ctx"]
    srv = gen.serve(slots=16, chunk_frames=4, **TYP)                                    # alone, in slot 0
    a = _probe(srv, ctx, **MINE)
    _finish(srv)
    assert a.done and a.slot is None and a.codes().shape == (K, PROBE["frames"]) and a.typical_p == 0.2
    srv = gen.serve(slots=16, chunk_frames=4, **TYP)                                    # ... and typical_p matters
    off = _probe(srv, ctx, **{**MINE, "typical_p": 1.0})
    _finish(srv)
    assert not torch.equal(off.codes(), a.codes())
    srv = gen.serve(slots=16, chunk_frames=4, typical_p=0.97, repetition_penalty=1.2, repetition_window=32, **TYP)

    def other(i):
        t, k = OTHERS[i % len(OTHERS)]
        kw = {} if i % len(OTHERS) == 1 else dict(temperature=t, topk=k, typical_p=TYPICALS[i % len(TYPICALS)])
        frames = 14 if i == 0 else 3 + (i * 5) % 9                                      # (slot 0 stays taken: the probe sits elsewhere)
        return srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], adapter="a1" if i % 5 == 2 else None,
                          seed=i if i % 2 else None, max_audio_length_ms=frames * 80, **kw)
    others = [other(i) for i in range(15)]
    srv.step()
    b = _probe(srv, ctx, repetition_penalty=1.0, **MINE)
    others += [other(i) for i in range(15, 21)]                                         # these wait for slots ...
    srv.step()
    st = srv._state
    assert b.slot not in (None, 0) and len(srv.active) >= 8 and srv.queued > 0
    _mirror_equals_buffer(st)
    assert st.row_typical[b.slot][6] == (0.2,) * K and len({r[6] for r in st.row_typical}) >= 5
    srv.step()                                                                          # ... and join while the probe is mid-utterance
    _mirror_equals_buffer(st)
    _finish(srv)
    assert b.done and all(o.done for o in others)
    _same(b, a)
    # a served conversation's first turn: the request's prompt, the request's noise
    srv = gen.serve(slots=16, chunk_frames=4, **TYP)
    conv = srv.conversation(context=ctx, seed=PROBE["seed"], temperature=0.9, topk=50, typical_p=0.5)
    turn = conv.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=PROBE["frames"] * 80, typical_p=0.2)
    _finish(srv)
    assert turn.done and turn.typical_p == 0.2 and conv.typical_p == 0.5
    assert torch.equal(turn.codes(), a.codes())
    # generate: a one-slot server's request under the request's noise (one row: the one-utterance kernels)
    one = gen.serve(slots=1, chunk_frames=4, **TYP)
    c = _probe(one, ctx, **MINE)
    _finish(one)
    torch.manual_seed(PROBE["seed"])
    audio = gen.generate(PROBE["text"], PROBE["speaker"], ctx, max_audio_length_ms=PROBE["frames"] * 80, adapter=None, **MINE)
    st = gen._model._decode_state
    assert st.row_typical[0][6] == (0.2,) * K and st.graph_key in (None, (None, None, "typical"))
    assert int(st.sampler.hist_frame[0]) == PROBE["frames"]
    ring = st.sampler.code_hist[0, :, :PROBE["frames"]].cpu().long()                    # the codes generate drew, frame by frame
    assert torch.equal(ring, c.codes().cpu().long()), (ring[:4, :6], c.codes()[:4, :6])
    torch.manual_seed(PROBE["seed"])
    chunks = list(gen.generate_stream(PROBE["text"], PROBE["speaker"], ctx, max_audio_length_ms=PROBE["frames"] * 80, **MINE))
    assert torch.equal(torch.cat(chunks), audio)
    torch.manual_seed(PROBE["seed"])
    plain = gen.generate(PROBE["text"], PROBE["speaker"], ctx, max_audio_length_ms=PROBE["frames"] * 80, temperature=0.9, topk=50,
                         typical_p=1.0)
    assert gen._model._decode_state.row_typical is None and gen._model._decode_state.sampler.level == 0
    assert not torch.equal(plain, audio)


def test_every_code_of_a_frame_lies_in_the_reference_typical_set(world, monkeypatch):
    """One generated frame per row of a batch of three: each draw's logits are taken as the sampler gets them (``RowSampler.draw``
    recorded) and the drawn code must be in the float64 reference's T for them - never in what typical sampling dropped.  Only
    draws whose margins lie inside the kernel's derived bounds are left out, at most one in ten."""
    from csm.sampling import RowSampler
    gen = world["plain"]
    seen = []
    draw = RowSampler.draw

    def recording(self, logits, i, q):
        out = draw(self, logits, i, q)
        seen.append((i, logits.detach().float().cpu().clone(), out.detach().cpu().clone()))
        return out
    monkeypatch.setattr(RowSampler, "draw", recording)
    temps, topks, typs = [0.9, 1.2, 0.7], [50, 2051, 200], [0.2, 0.6, [0.9] + [0.3] * (K - 1)]
    torch.manual_seed(3)
    gen.generate_batch(["one voice", "another voice here", "a third"], [0, 1, 2], [[], [], []], max_audio_length_ms=80,
                       temperature=temps, topk=topks, typical_p=typs)
    assert len(seen) == K and [i for i, _, _ in seen] == list(range(K))
    draws = skipped = outside_argmax = 0
    for i, logits, codes in seen:
        assert logits.shape[0] == 3
        for b in range(3):
            x = logits[b, :2051]
            tp = typs[b][i] if isinstance(typs[b], list) else typs[b]
            ref = T.reference(x, topks[b], temps[b], 1.0, 0.0, tp, torch.ones(x.shape[0]))     # (frame 0: no penalty reaches a code)
            draws += 1
            if ref["mass_margin"] < ref["mass_bound"] or ref["order_margin"] < ref["delta_bound"]:
                skipped += 1
                continue
            code = int(codes[b])
            assert ref["T"][code], (i, b, code, int(ref["T"].sum()), int(ref["N"].sum()))
            outside_argmax += ref["drops_argmax"]
    print("draws %d, skipped %d, typical sets without the argmax %d" % (draws, skipped, outside_argmax))
    assert draws == 3 * K and 10 * skipped <= draws, (draws, skipped)


def test_a_change_of_typical_p_replays_the_same_graph_and_per_codebook_values_reach_the_buffer(world):
    gen, m, ctx = world["plain"], world["m"], world["ctx"]
    srv = gen.serve(slots=6, chunk_frames=4, **TYP)
    st = srv._state
    reqs = [srv.submit("the first", 0, ctx, seed=1, max_audio_length_ms=20 * 80, temperature=0.7, topk=8, typical_p=0.9)]
    srv.step()                                     # the tail, one eager frame (warm-up), the captured frame, its first replay
    graph, key = st.graph, st.graph_key
    assert (graph is not None) == getattr(m, "use_hip_graph", True)
    per = [0.25] + [0.75] * (K - 1)
    for i, ty in enumerate([0.3, per, 1.0, 1e-3]):
        for bad in (dict(typical_p=0.0), dict(typical_p=float("nan")), dict(typical_p=1.01), dict(typical_p=[0.5] * (K - 1))):
            with pytest.raises(ValueError, match="typical_p"):
                srv.submit("refused", 0, [], seed=3, max_audio_length_ms=10 * 80, **bad)
        assert srv.queued == 0
        reqs.append(srv.submit(f"joiner {i}", i % 3, [], seed=10 + i, max_audio_length_ms=(24 + 2 * i) * 80, typical_p=ty))
        srv.step()
        want = tuple(ty) if isinstance(ty, list) else (ty,) * K
        assert st.graph is graph and st.graph_key == key and reqs[-1].slot == i + 1 and st.row_typical[i + 1][6] == want
        assert st.sampler.params[6][:, i + 1].cpu().tolist() == pytest.approx(list(want))
        if graph is not None:
            assert key == (None, None, "typical")
    st.set_row_typical(0, 0.7, 8, 1.0, 0.0, 1.0, 64, per)                            # ... and written straight to a running row
    srv.step()
    assert st.graph is graph and st.sampler.params[6][:, 0].cpu().tolist() == pytest.approx(per)
    _mirror_equals_buffer(st)
    _finish(srv)
    assert st.graph is graph and all(r.done for r in reqs)
    # refusals: a server without row_typical, the recompute path, the engine's own rule
    with pytest.raises(ValueError, match="row_sampling=True"):
        gen.serve(slots=2, row_typical=True)
    with pytest.raises(ValueError, match="row_typical=True"):
        gen.serve(slots=2, row_sampling=True, row_processors=True, typical_p=0.9)
    srv = gen.serve(slots=2, chunk_frames=4, row_sampling=True, row_processors=True)
    with pytest.raises(ValueError, match="row_typical=True"):
        srv.submit("a", 0, [], typical_p=0.9)
    ok = srv.submit("a", 0, [], seed=1, max_audio_length_ms=3 * 80, typical_p=1.0)
    _finish(srv)
    assert ok.done and ok.typical_p == 1.0 and srv._state.row_typical is None
    was = getattr(m, "use_kv_cache", True)
    m.use_kv_cache = False
    try:
        with pytest.raises(ValueError, match="recompute path"):
            gen.generate("a", 0, [], max_audio_length_ms=2 * 80, typical_p=0.9)
    finally:
        m.use_kv_cache = was
    from csm.engine import DecodeState
    s3 = DecodeState(m.engine, 3)
    with pytest.raises(RuntimeError, match="set_row_typical first"):
        s3.sampler.need(4)
    assert s3.sampling_args(0.8, 5, typical_p=[0.9, per, 1.0]) == (None, None)
    assert [r[6] for r in s3.row_typical] == [(0.9,) * K, tuple(per), (1.0,) * K] and s3.row_processors is None
    assert s3.sampler.params[6][:, 1].cpu().tolist() == pytest.approx(per)
    with pytest.raises(ValueError, match="typical_p must be"):
        s3.sampling_args(0.8, 5, typical_p=[0.9, 0.0, 1.0])
    assert [r[6][0] for r in s3.row_typical] == [0.9, 0.25, 1.0]                       # (all checked before any is written)
