"""Every logits vector of every generated frame - all codebooks, rows and frames - and every K / V row a frame writes, against the
float64 reference of tests/gen_frame_ref.py, in every decode mode, eagerly and through the captured HIP graph.

The engine is observed, not changed: ``Engine._frame_tail_body`` (and the recompute body) import ``sample_topk`` from
csm.models.model at each call and, with (None, None), call ``st.sampler.draw``; both are patched with a stand-in that works on
persistent device buffers allocated before the run - it calls the real sampler and copies its result into ``picked[i]``, copies
the logits into ``rec[i]`` and returns ``forced[i]``.  These are device-to-device copies between persistent tensors: they are
captured into the frame graph and run again on every replay.  The test writes ``forced`` before each frame, outside the graph, as
the engine fills ``noise_buf``, and reads ``rec`` after it.

Asserted per case, eagerly and (but for the recompute path) through the graph: every ratio of ``gen_frame_ref.judge`` <= L and
every exact condition; the graph run's logits and caches equal the eager run's bit for bit; ``picked`` equals the fp32 oracle
sampler on the recorded device logits with that frame's noise row and the parameters that row should get.  L is measured on the
reference alone (gen_frame_ref.L, proven by test_gen_frame_ref_cpu.py) and is not fitted to what runs here."""
import pytest
import torch

import gen_frame_ref as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K, V = G.K, G.V


class Recorder:
    """The stand-in of the two samplers and its persistent buffers."""

    def __init__(self, B, dev, real_topk, real_draw):
        self.rec = torch.zeros(K, B, V, dtype=torch.float32, device=dev)
        self.picked = torch.zeros(K, B, 1, dtype=torch.int32, device=dev)
        self.forced = torch.zeros(K, B, 1, dtype=torch.int32, device=dev)
        self.real_topk, self.real_draw, self.i = real_topk, real_draw, 0

    def _take(self, i, lg, code):
        self.picked[i].copy_(code)
        self.rec[i].copy_(lg)
        return self.forced[i]

    def topk(self, lg, topk, temperature, q=None):
        i, self.i = self.i, self.i + 1               # (no codebook argument: the frame body calls it once per codebook, in order)
        return self._take(i, lg, self.real_topk(lg, topk, temperature, q))

    def draw(self, sampler, lg, i, q):
        return self._take(i, lg, self.real_draw(sampler, lg, i, q))

    def feed(self, codes):
        """codes [K, B] (CPU): the codes this frame continues from."""
        self.forced.copy_(codes.to(torch.int32).unsqueeze(-1))
        self.i = 0


def build(case, dev):
    """The tiny 8-codebook model on the reference's weights, its adapters holding ``make_adapter``'s values."""
    from csm.models.model import Model, ModelArgs
    from csm.training.lora import LoRAState, apply_lora_to_model
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", G.CFG.text_vocab, V, K), device="cuda")
    m.load_state_dict(G.params(torch.float32))

    def fill(state, spec):
        values, named = G.make_adapter(spec), dict(state.named_tensors())
        assert sorted(named) == sorted(values)
        with torch.no_grad():
            for k, t in named.items():
                t.copy_(values[k].to(BF))

    rows = None
    if case.live is not None:
        sp = case.live
        apply_lora_to_model(m, r=sp.r, alpha=sp.alpha, target_modules=list(sp.modules), use_bias=sp.bias, seed=sp.seed)
        fill(m.lora, sp)
    elif case.rows is not None:
        bank = [LoRAState(m, sp.r, sp.alpha, 0.0, list(sp.modules), None, sp.bias, seed=sp.seed, grad=False) for sp in case.bank]
        for st, sp in zip(bank, case.bank):
            fill(st, sp)
        rows = [bank[a] if a >= 0 else None for a in case.rows]
    if case.fp8:
        m.decode_weights = "fp8"
        m.fp8_adapters = case.rows is not None
    return m, rows


def _quantised(st):
    """The weights the state holds as e4m3 codes, under the reference's names."""
    out = set()
    for prefix, stack in (("backbone", st.bb), ("decoder", st.dc)):
        for name in (stack.w8 or {}):
            layer, rest = name.split(".attn.") if ".attn." in name else name.split(".mlp.")
            sub = "attn" if ".attn." in name else "mlp"
            mods = {"qkv": ("q_proj", "k_proj", "v_proj"), "w13": ("w1", "w3")}.get(rest, (rest.replace(".weight", ""),))
            out |= {f"{prefix}.{layer}.{sub}.{mod}.weight" for mod in mods}
    return frozenset(out)


def _frame_inputs(codes, live, dev):
    """codes [K, B] -> tokens / masks [B, 1, K+1] of the fed-back audio frame; rows not in ``live`` get zeros (idle rows)."""
    B = codes.shape[1]
    on = torch.tensor([b in live for b in range(B)])
    tok = torch.cat([codes.t(), torch.zeros(B, 1, dtype=torch.int64)], 1) * on[:, None]
    msk = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1) & on[:, None]
    return tok.unsqueeze(1).to(dev), msk.unsqueeze(1).to(dev)


def run(case, dev, graph, monkeypatch, real):
    """The case's frames on the engine -> (Result, picked [F, K, B], the noise each frame sampled with [F, K, B, V], the host
    position mirror after every frame [F][B], whether every cache slot from S_KEEP on is still zero)."""
    import csm.models.model as MM
    from csm.engine import DecodeState
    from csm.sampling import RowSampler
    m, ads = build(case, dev)
    inp = G.inputs(case)
    B, Fn = case.B, case.frames
    rec = Recorder(B, m.device, *real)
    monkeypatch.setattr(MM, "sample_topk", rec.topk)
    monkeypatch.setattr(RowSampler, "draw", lambda self, lg, i, q: rec.draw(self, lg, i, q))
    m.use_hip_graph, m.use_kv_cache = graph, case.kv_cache
    m.setup_caches(B)
    m.reset_caches()
    toks, msks, noise = inp["tokens"], inp["masks"], inp["noise"]
    logits, picked, used, kvs, poss, host = [], [], [], [], [], []

    def qs(f):
        return [noise[f, i] for i in range(K)]

    def snap(st):
        logits.append(rec.rec.cpu())
        picked.append(rec.picked.cpu()[..., 0])
        if st is not None:
            used.append(st.noise_buf.cpu())
            kvs.append(st.bb.kv[..., :G.S_KEEP, :].cpu())
            poss.append(st.bb.pos.cpu().long())
            host.append(list(st.row_pos))

    st = None
    with torch.no_grad():
        if not case.kv_cache:
            S = inp["lens"][0]
            for f in range(Fn):
                rec.feed(inp["forced"][f])
                if f == 0:
                    m.generate_frame(torch.stack(toks), torch.stack(msks), torch.arange(S)[None].repeat(B, 1), G.TEMP, G.TOPK, noise=qs(f))
                else:
                    tk, mk = _frame_inputs(inp["forced"][f - 1], range(B), dev)
                    m.generate_frame(tk, mk, torch.full((B, 1), S + f - 1), G.TEMP, G.TOPK, noise=qs(f))
                snap(None)
                used.append(noise[f])
        elif case.sampling is not None:
            # a served batch: every row its own (temperature, topk), the first frame over all rows, then the idle rows idle
            torch.manual_seed(1000 + case.seed)
            m.engine._need()
            st = DecodeState(m.engine, B)
            for b, (t, k) in enumerate(case.sampling):
                st.set_row_sampling(b, t, k)
            last = st.prefill_ragged(toks, msks)
            rec.feed(inp["forced"][0])
            st.serve_first(last, range(B), None, None)
            snap(st)
            st.set_active(case.active(1))
            for f in range(1, Fn):
                rec.feed(inp["forced"][f])
                st.serve_frame(*_frame_inputs(inp["forced"][f - 1], case.active(f), dev), None, None)
                snap(st)
        else:
            for f in range(Fn):
                rec.feed(inp["forced"][f])
                if f == 0:
                    m.engine.generate_first_frames(toks, msks, G.TEMP, G.TOPK, noise=qs(f), adapters=ads)
                    st = m._decode_state
                else:
                    tk, mk = _frame_inputs(inp["forced"][f - 1], range(B), dev)
                    m.generate_frame(tk, mk, torch.ones(B, 1, dtype=torch.long), G.TEMP, G.TOPK, noise=qs(f))
                snap(st)
                assert torch.equal(used[-1], noise[f]), "the frame sampled with the noise it was given"
    if st is None:
        return G.Result(torch.stack(logits).double(), None, None), torch.stack(picked), torch.stack(used), None, True
    if graph:
        assert st.graph is not None, "frames 2.. must have gone through the captured graph"
    # the mode the case is named for really ran
    assert st.dc.fuse_attn == (B == 1) and not st.bb.fuse_attn
    assert (st.bb.w8 is not None) == (st.dc.w8 is not None) == case.fp8
    for stack in (st.bb, st.dc):
        assert (stack.lora_rows is not None) == (case.rows is not None)
        assert (stack.lora is not None) == (case.rows is not None or case.live is not None)
    rest_zero = not bool(st.bb.kv[..., G.S_KEEP:, :].any())
    got = G.Result(torch.stack(logits).double(), torch.stack(kvs).double(), torch.stack(poss), _quantised(st))
    return got, torch.stack(picked), torch.stack(used), host, rest_zero


def check(case, x64, emu, got, picked, used, host, rest_zero, tag):
    v = G.judge(got, x64, emu, case)
    ratios = dict(v.ratios)
    ratios.update({(f, "kv"): r for f, r in v.kv_ratios.items()})
    at = max(ratios, key=ratios.get)
    print(f"WORST {case.name} {tag} {ratios[at]:.3f} at (frame, codebook) {at}; L = {G.L}; {v.n_logits} logits vectors, {v.n_kv} K / V rows")
    assert (v.n_logits, v.n_kv) == G.expected_counts(case)
    assert not v.broken, v.broken[:8]
    assert rest_zero, "a cache slot from S_KEEP on was written"
    assert v.worst <= G.L, (case.name, tag, at, v.worst)
    if host is not None:
        lens = G.inputs(case)["lens"]
        for f in range(case.frames):
            for b in range(case.B):
                want = int(x64.pos[f, b]) if b in case.active(f) else lens[b] - 1     # (an idle row's host mirror does not move)
                assert host[f][b] == want, (f, b, host[f][b], want)
    # which noise and which parameters reached which codebook and row: the oracle sampler on the recorded device logits
    ref = G.sampled_codes(got.logits, used, case)
    bad = [(f, i, b, int(picked[f, i, b]), int(ref[f, i, b])) for f in range(case.frames) for i in range(K) for b in case.active(f)
           if int(picked[f, i, b]) != int(ref[f, i, b])]
    assert not bad, (case.name, tag, bad[:8])


@pytest.mark.parametrize("name", list(G.CASES))
def test_frame_logits_against_float64(dev, name, monkeypatch):
    case = G.CASES[name]
    import csm.models.model as MM
    from csm.sampling import RowSampler
    real = (MM.sample_topk, RowSampler.draw)               # (before the first patch: the second run must not wrap the first's stand-in)
    x64, emu = G.frame64(case), G.frame_emulated(case)
    eager = run(case, dev, False, monkeypatch, real)
    check(case, x64, emu, *eager, "eager")
    if not case.kv_cache:
        return                                             # (the recompute path captures nothing)
    graph = run(case, dev, True, monkeypatch, real)
    check(case, x64, emu, *graph, "graph")
    assert torch.equal(graph[0].logits, eager[0].logits), "the captured graph's logits differ from the eager frames'"
    assert torch.equal(graph[0].kv, eager[0].kv) and torch.equal(graph[0].pos, eager[0].pos)
    if case.sampling is None:
        assert torch.equal(graph[1], eager[1])
