"""Per-request sampling statistics end to end (``return_stats=`` / ``serve(stats=True)`` / ``DecodeState.enable_stats``).

Engine level, on ``gen_frame_ref.CFG`` (``O.tiny_cfg()`` with 8 codebooks: the model whose logits tests/gen_frame_ref.py bounds)
and its weights, one prompt of ``gen_frame_ref.inputs``, FRAMES seeded frames:
  2. each frame's statistics lie within the kernel bound (tests/sample_stats_ref.py) of the float64 reference applied to that
     frame's own ``logits_all`` and codes; the eager run and the graph replay give the same codes and the same bits.
  3. ``logprob`` against the CPU oracle (``gen_frame_ref._run`` in fp32, teacher-forced with the generated codes: the text
     test_gen_frame_ref_cpu.py proves against ``oracle/csm_oracle.py``): |difference| <= 2 x the logit bound of gen_frame_ref - per
     logits vector ``L * max(|emulated - float64|_2, 2^-10 |float64|_2)``, a bound on the max norm too - because log-softmax is
     2-Lipschitz in the max norm.
  4. the negated sum of a frame's K log-probabilities equals ``compute_loss(..., return_rows=True)`` under the next-frame
     objective on the generated utterance, row by row.  Tolerance per frame: the CPU oracle's own fp32-against-float64 difference
     of that sum (measured in the test on the generated codes; on ``gen_frame_ref.inputs``' forced codes it measured 4.5e-6 at
     worst over five frames) plus the margin of item 3 summed over the frame's codebooks.

Generator level, on the tiny model, Mimi and probe of tests/test_serving_gpu.py:
  1. a seeded ``generate(..., return_stats=True)`` returns the codes and the audio of the call without it (torch.equal), with the
     scalar sampler and at sampler level 4; so do ``generate_stream`` and ``generate_batch``.
  5. on a server with ``stats=True`` a seeded request has torch.equal statistics alone, among 15 neighbours in another slot, and
     parked at least twice under ``streams``.
  6. ``cancel(heard_frames=k)`` leaves k frames of statistics.
"""
from dataclasses import replace

import pytest
import torch

import gen_frame_ref as G
import sample_stats_ref as R
import train_step_ref as T
from test_serve_streams_gpu import _among, _run, _submit_probe
from test_serving_gpu import PROBE, TEMP, TOPK, K, world  # noqa: F401  (world: the module fixture, built here)

pytestmark = pytest.mark.gpu
FRAMES = 5
CASE = replace(G.CASES["plain_b1"], frames=FRAMES)
_memo = {}


# ------------------------------------------------------------------------------------------------------------ engine level
def _frames(dev, graph, level4=False):
    """FRAMES seeded frames of the one-row case on the engine in statistics mode: codes [F, K], stats [F, 3, K], logits_all
    [F, K, V] - all on the CPU - and the state."""
    key = (graph, level4)
    if key in _memo:
        return _memo[key]
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", G.CFG.text_vocab, G.V, G.K), device="cuda")
    m.load_state_dict(G.params(torch.float32))
    m.use_hip_graph = graph
    m.setup_caches(1)
    m.reset_caches()
    inp = G.inputs(CASE)
    tok, msk = inp["tokens"][0].unsqueeze(0).to(dev), inp["masks"][0].unsqueeze(0).to(dev)
    pos = torch.arange(tok.shape[1]).unsqueeze(0)
    kw = dict(typical_p=0.9, repetition_penalty=1.2, repetition_window=8) if level4 else {}
    noise = torch.empty(FRAMES, G.K, 1, G.V).exponential_(1, generator=torch.Generator().manual_seed(77)).to(dev)
    codes, stats, logits = [], [], []
    for f in range(FRAMES):
        c = m.generate_frame(tok, msk, pos, G.TEMP, G.TOPK, noise=list(noise[f]), stats=True, **kw)
        st = m._decode_state
        codes.append(c[0].cpu().long())
        stats.append(st.frame_stats()[:, :, 0].cpu())
        logits.append(st.logits_all[:, 0, :G.V].cpu())
        tok = torch.cat([c.long(), torch.zeros(1, 1, dtype=torch.long, device=dev)], 1).unsqueeze(1)
        msk = torch.cat([torch.ones(1, G.K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1).to(dev)
        pos = pos[:, -1:] + 1
    out = dict(codes=torch.stack(codes), stats=torch.stack(stats), logits=torch.stack(logits), key=st.graph_key, m=m,
               level=st.sampler.level)
    _memo[key] = out
    return out


@pytest.mark.parametrize("level4", [False, True], ids=["scalar", "level4"])
def test_frame_statistics_are_the_reference_of_their_own_logits_eager_and_replayed(dev, level4):
    eager, graph = _frames(dev, False, level4), _frames(dev, True, level4)
    assert eager["level"] == graph["level"] == (4 if level4 else 0)
    assert graph["key"] == ((None, None, "typical", "stats") if level4 else (G.TEMP, G.TOPK, "stats")), graph["key"]
    assert torch.equal(eager["codes"], graph["codes"])
    assert torch.equal(eager["logits"].view(torch.int32), graph["logits"].view(torch.int32))
    assert torch.equal(eager["stats"].view(torch.int32), graph["stats"].view(torch.int32))
    worst = {n: 0.0 for n in R.OUTPUTS}
    for f in range(FRAMES):
        ref = R.reference(graph["logits"][f], graph["codes"][f])
        for j, n in enumerate(R.OUTPUTS):
            val, bound = ref[n]
            err = (graph["stats"][f, j].double() - val).abs()
            assert bool(torch.isfinite(graph["stats"][f, j]).all()) and bool((bound > 0).all())
            worst[n] = max(worst[n], float((err / bound).max()))
    print("RATIO gen_stats frame", "level4" if level4 else "scalar", " ".join(f"{n} {w:.4f}" for n, w in worst.items()))
    assert all(w <= 1.0 for w in worst.values()), worst


def _oracle(codes):
    """The teacher-forced runs of gen_frame_ref on the generated codes: float64, emulated bf16 stores, and the fp32 oracle."""
    if "oracle" not in _memo:
        inp = dict(G.inputs(CASE))
        inp["forced"] = codes.view(FRAMES, G.K, 1).clone()
        x64 = G._run(CASE, T.Rounder(False), inp=inp).logits[:, :, 0]
        emu = G._run(CASE, T.Rounder(True, None), inp=inp).logits[:, :, 0]
        x32 = G._run(CASE, T.Rounder(False), P=G.params(torch.float32), inp=inp).logits[:, :, 0]
        _memo["oracle"] = (x64, emu, x32.double())
    return _memo["oracle"]


def _margin(x64, emu):
    """2 x the logit bound of gen_frame_ref per (frame, codebook): ``judge``'s denominator times L."""
    return 2.0 * G.L * torch.maximum((emu - x64).norm(dim=-1), 2.0 ** -10 * x64.norm(dim=-1))


def test_logprob_is_the_oracles_teacher_forced_log_softmax(dev):
    got = _frames(dev, True)
    codes = got["codes"]
    x64, emu, x32 = _oracle(codes)
    want = torch.log_softmax(x32, -1).gather(-1, codes.unsqueeze(-1)).squeeze(-1)             # [F, K]
    margin = _margin(x64, emu)
    err = (got["stats"][:, 0].double() - want).abs()
    print("RATIO gen_stats oracle logprob: worst |err| / margin", float((err / margin).max()), "worst |err|", float(err.max()),
          "smallest margin", float(margin.min()))
    assert bool((err <= margin).all()), (err, margin)


def test_negated_logprob_sum_is_the_next_frame_loss(dev):
    """Measured on the CPU oracle (fp32 against float64, the per-frame sum of K negative log-likelihoods): printed below as
    ``cpu``; 4.5e-6 at worst on gen_frame_ref.inputs' own forced codes, 6.6e-6 on the codes the MI355X generated (2026-10-21),
    where the per-frame differences were 0.010 .. 0.070 nats against tolerances of 9.5 .. 12.7 - the margin of item 3 is wide,
    being eight codebooks' worth of an L2 bound on 67 logits - and the worst single logprob was 0.028 off the oracle's."""
    from csm.data import collate_variable_length, to_next_frame
    from csm.data.training_data import IGNORE_INDEX
    from csm.training.utils import compute_loss
    got = _frames(dev, True)
    codes, m = got["codes"], got["m"]
    x64, emu, x32 = _oracle(codes)
    nll64 = -torch.log_softmax(x64, -1).gather(-1, codes.unsqueeze(-1)).squeeze(-1).sum(1)   # [F]
    nll32 = -torch.log_softmax(x32.float(), -1).double().gather(-1, codes.unsqueeze(-1)).squeeze(-1).sum(1)
    cpu = (nll32 - nll64).abs()
    tol = cpu + _margin(x64, emu).sum(1)
    inp = G.inputs(CASE)
    S = inp["tokens"][0].shape[0]
    item = to_next_frame({"input_tokens": inp["tokens"][0].long(), "input_masks": inp["masks"][0].bool(),
                          "target_audio_tokens": codes}, "target")
    batch = collate_variable_length([item], target_pad=IGNORE_INDEX)
    m.acoustic_mode, m.target_ignore_index = "all", IGNORE_INDEX
    with torch.no_grad():
        _, det = compute_loss(m, batch["input_tokens"], batch["input_masks"], batch["target_audio_tokens"], return_rows=True)
    sem = det["semantic_rows"][0].double().cpu()                                               # [S + F + 1]
    idx = det["acoustic_row_index"].cpu().tolist()
    ac = det["acoustic_rows"].double().cpu()
    loss = torch.stack([sem[S - 1 + f] + ac[idx.index(S - 1 + f)].sum() for f in range(FRAMES)])   # position S-1+f predicts frame f
    mine = -got["stats"][:, 0].double().sum(1)
    err = (mine - loss).abs()
    print("RATIO gen_stats loss: per-frame |(-sum logprob) - loss|", err.tolist(), "cpu fp32 vs float64", cpu.tolist(), "tol", tol.tolist())
    assert bool((err <= tol).all()), (err, tol)
    assert abs(float(mine.sum() - loss.sum())) <= float(tol.sum())


# --------------------------------------------------------------------------------------------------------- generator level
L4 = dict(temperature=0.9, topk=50, typical_p=0.9, repetition_penalty=1.2, repetition_window=16)


def _check_shape(stats, frames):
    assert len(stats) == frames
    for t in (stats.logprob, stats.entropy, stats.pmax):
        assert t.shape == (frames, K) and t.dtype == torch.float32 and t.device.type == "cpu" and bool(torch.isfinite(t).all())
    assert bool((stats.logprob <= 0).all()) and bool((stats.pmax > 0).all()) and bool((stats.pmax <= 1).all())
    assert bool((stats.entropy > -1e-3).all()) and bool((stats.logprob.exp() <= stats.pmax * (1 + 1e-4)).all())


@pytest.mark.parametrize("kw", [dict(temperature=TEMP, topk=TOPK), L4], ids=["scalar", "level4"])
def test_return_stats_changes_neither_codes_nor_audio(world, monkeypatch, kw):
    gen, ctx, codec = world["plain"], world["ctx"], world["codec"]
    seen = []
    decode = codec.decode
    monkeypatch.setattr(codec, "decode", lambda c: (seen.append(c.clone()), decode(c))[1])
    args = (PROBE["text"], PROBE["speaker"], ctx)
    ms = PROBE["frames"] * 80
    torch.manual_seed(PROBE["seed"])
    audio = gen.generate(*args, max_audio_length_ms=ms, **kw)
    assert gen._model._decode_state.stats is None
    torch.manual_seed(PROBE["seed"])
    audio2, stats = gen.generate(*args, max_audio_length_ms=ms, return_stats=True, **kw)
    st = gen._model._decode_state
    assert st.stats is not None and st.graph_key[-1] == "stats" and st.sampler.level == (4 if "typical_p" in kw else 0)
    assert len(seen) == 2 and torch.equal(seen[0], seen[1]) and torch.equal(audio, audio2)
    _check_shape(stats, seen[0].shape[2])
    torch.manual_seed(PROBE["seed"])
    parts = list(gen.generate_stream(*args, max_audio_length_ms=ms, chunk_frames=4, return_stats=True, **kw))
    assert torch.equal(torch.cat([a for a, _ in parts]), audio)
    assert sum(len(s) for _, s in parts) == len(stats) and all(len(s) <= 4 for _, s in parts)
    for name in ("logprob", "entropy", "pmax"):
        assert torch.equal(torch.cat([getattr(s, name) for _, s in parts]), getattr(stats, name)), name
    torch.manual_seed(PROBE["seed"])
    (one,), (bstats,) = gen.generate_batch([args[0]], [args[1]], [ctx], max_audio_length_ms=ms, return_stats=True, **kw)
    torch.manual_seed(PROBE["seed"])
    (want,) = gen.generate_batch([args[0]], [args[1]], [ctx], max_audio_length_ms=ms, **kw)
    assert torch.equal(one, want)
    _check_shape(bstats, len(stats))


def test_recompute_path_refuses_return_stats(world):
    gen, ctx = world["plain"], world["ctx"]
    gen._model.use_kv_cache = False
    try:
        with pytest.raises(ValueError, match="return_stats"):
            gen.generate(PROBE["text"], PROBE["speaker"], ctx, max_audio_length_ms=160, return_stats=True)
        with pytest.raises(ValueError, match="return_stats"):
            gen.serve(stats=True)
    finally:
        gen._model.use_kv_cache = True


def _same_stats(a, b):
    assert len(a.stats) == len(b.stats) == a.codes().shape[1]
    for name in ("logprob", "entropy", "pmax"):
        assert torch.equal(getattr(a.stats, name).view(torch.int32), getattr(b.stats, name).view(torch.int32)), name


def test_a_served_request_has_its_statistics_alone_among_neighbours_and_parked(world):
    gen, ctx = world["plain"], world["ctx"]
    srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK, stats=True)               # alone
    a = _submit_probe(srv, ctx)
    seen = []
    for req, _, _ in srv.run():
        seen.append(len(req.stats))
    assert a.done and seen == [4, 8, 12, 14] and srv._state.graph_key == (TEMP, TOPK, "stats")     # grows chunk by chunk
    _check_shape(a.stats, PROBE["frames"])
    off = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)                           # the server without: same codes
    c = _submit_probe(off, ctx)
    _run(off)
    assert c.stats is None and off._state.stats is None and off._state.graph_key == (TEMP, TOPK)
    assert torch.equal(c.codes(), a.codes()) and torch.equal(c.audio(), a.audio())
    srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK, stats=True)               # among 15, in another slot
    others = [srv.submit("n" * (3 + 2 * i), i % 3, ctx if i % 4 == 0 else [], seed=i if i % 2 else None,
                         max_audio_length_ms=(14 if i == 0 else 6 + (i * 5) % 9) * 80) for i in range(15)]
    srv.step()
    assert sum(not o.done for o in others) == 15                                                     # all still speak: slots 0..14
    b = _submit_probe(srv, ctx)
    srv.step()
    assert b.slots_held == [15] and srv.last_join_rows == 1
    _run(srv)
    assert b.done and all(o.done and len(o.stats) == o.codes().shape[1] for o in others)
    assert torch.equal(b.codes(), a.codes())
    _same_stats(b, a)
    p, _, psrv = _among(gen, ctx, stats=True)                                                        # parked under streams
    _run(psrv)
    assert p.done and p.preemptions >= 2 and len(set(p.slots_held)) >= 2, (p.preemptions, p.slots_held)
    assert torch.equal(p.codes(), a.codes())
    _same_stats(p, a)


def test_cancel_cuts_the_statistics_to_the_heard_frames(world):
    gen, ctx = world["plain"], world["ctx"]
    srv = gen.serve(slots=4, chunk_frames=4, temperature=TEMP, topk=TOPK, stats=True)
    conv = srv.conversation(context=ctx, seed=5)
    turn = conv.say(PROBE["text"], PROBE["speaker"], max_audio_length_ms=PROBE["frames"] * 80)
    srv.step()
    srv.step()
    assert not turn.done and len(turn.stats) == 8
    full = turn.stats.logprob.clone()
    srv.cancel(turn, heard_frames=5)
    assert turn.done and turn.cancelled and len(turn.stats) == 5 and torch.equal(turn.stats.logprob, full[:5])
    assert turn.stats.entropy.shape == turn.stats.pmax.shape == (5, K)
