"""Per-utterance LoRA adapters (a bank of adapters, one per batch row): the gathered decode kernels (csm_lora_project_rows_bf16,
csm_gemv_bf16_kext_rows) against fp32 and bit for bit against the one-adapter kernels, the engine's per-row decode state against
one-utterance runs with the adapter live as model.lora, and the public interface (Generator adapters, csm-generate
--lora-adapter)."""
import wave

import pytest
import torch

from oracle import csm_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TINY = O.tiny_cfg()
ALL7 = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]


def gclose(name, got, ref, tol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-20
    assert err <= tol * scale, f"{name}: max abs err {err:.4g} vs max |ref| {scale:.4g}"


def ptrs(ts, dev):
    return torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64, device=dev)


def xhat(x, w):
    return O.rmsnorm(x.float().cpu(), w.float().cpu(), 1e-5).to(BF).float()


# ----------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("K", [1024, 2048, 8192])
def test_project_rows_vs_fp32_and_one_row(dev, K):
    from csm.hip import ops
    g = torch.Generator().manual_seed(K + 1)
    kx, A = 32, 3
    At = [(torch.randn(K, kx, generator=g) / K ** 0.5).to(BF).to(dev) for _ in range(A)]
    scale = torch.tensor([2.0, 0.5, 1.25], dtype=torch.float32, device=dev)
    tab = ptrs(At, dev)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    for B in (1, 3, 4, 5, 9, 16):
        x = torch.randn(B, K, generator=g).to(BF).to(dev)
        ids = torch.tensor([(b % (A + 1)) - 1 for b in range(B)] if B > 1 else [1], dtype=torch.int32)
        ids = ids[torch.randperm(B, generator=g)]
        ra = ids.to(dev)
        for norm in (None, w):
            t = torch.full((B, kx), 7.0, dtype=BF, device=dev)
            ops.lora_project_rows(x, tab, t, ra, scale, kx, kx, norm_scale=norm, eps=1e-5)
            xr = xhat(x, w) if norm is not None else x.float().cpu()
            for b in range(B):
                a = int(ids[b])
                if a < 0:
                    assert torch.equal(t[b], torch.zeros(kx, dtype=BF, device=dev)), ("-1 row must be zeros", B, b)
                    continue
                gclose(f"project rows K={K} B={B} row {b}", t[b], float(scale[a]) * (xr[b] @ At[a].float().cpu()), 1e-2)
                t1 = torch.empty(1, kx, dtype=BF, device=dev)
                ops.lora_project(x[b:b + 1], At[a], t1, float(scale[a]), norm_scale=norm, eps=1e-5)
                assert torch.equal(t1[0], t[b]), ("row equals the one-row projection", K, B, b, norm is not None)


class Bank:
    """A adapters of one fused product: Bx [N, kx] (W's row order) and biases, plus their device tables."""

    def __init__(self, g, dev, N, kx=32, A=3, bias=True):
        self.Bx = [(torch.randn(N, kx, generator=g) * 0.05).to(BF).to(dev) for _ in range(A)]
        self.bias = [(torch.randn(N, generator=g) * 0.1).to(BF).to(dev) if bias and a != 1 else None for a in range(A)]
        self.Bx_tab, self.bias_tab = ptrs(self.Bx, dev), ptrs(self.bias, dev)
        self.kx = kx


def product(ops, form, W, w, table, x, R, idx, y, ext=None):
    """One decode product in ``form``; ``ext`` = None (gemv_ex), ("one", t, Bx, bias) (gemv_kext) or ("rows", t, bank, ra)."""
    kw = {"plain": {}, "residual": {"residual": R}, "norm": {"norm_scale": w, "eps": 1e-5, "residual": R},
          "norm+swiglu": {"norm_scale": w, "eps": 1e-5, "swiglu": True}, "f32": {"norm_scale": w, "eps": 1e-5},
          "gather": {"row_index": idx, "row_offset": 7}}[form]
    xin = table if form == "gather" else x
    if ext is None:
        return ops.gemv_ex(xin, W, y, **kw)
    if ext[0] == "one":
        return ops.gemv_kext(xin, W, y, ext[1], ext[2], bias=ext[3], **kw)
    _, t, bank, ra = ext
    return ops.gemv_kext_rows(xin, W, y, t, bank.Bx_tab, ra, bank.kx, bank.kx, bias_tab=bank.bias_tab, **kw)


def out_for(form, B, N, dev):
    return torch.empty(B, N // 2 if form == "norm+swiglu" else N, dtype=torch.float32 if form == "f32" else BF, device=dev)


def reference(form, W, w, table, x, R, idx, t, bank, ids):
    """fp32 reference of the per-row extended product."""
    Wf = W.float().cpu()
    xin = table[idx.long() + 7] if form == "gather" else x
    xr = xhat(x, w) if form in ("norm", "norm+swiglu", "f32") else xin.float().cpu()
    acc = xr @ Wf.t()
    for b, a in enumerate(ids.tolist()):
        if a >= 0:
            acc[b] += t[b].float().cpu() @ bank.Bx[a].float().cpu().t()
            if bank.bias[a] is not None:
                acc[b] += bank.bias[a].float().cpu()
    if form == "norm+swiglu":
        gu = acc.to(BF).float()
        return torch.nn.functional.silu(gu[:, 0::2]) * gu[:, 1::2]
    if form in ("residual", "norm"):
        acc = acc + R.float().cpu()
    return acc


# CSM-1B's decode products (N, K, form) and a tiny shape that takes the LDS kernel
SHAPES = [(3072, 2048, "norm"), (2048, 2048, "residual"), (16384, 2048, "norm+swiglu"), (2048, 8192, "residual"),
          (2112, 2048, "f32"), (1024, 2048, "gather"), (1536, 1024, "norm"), (16384, 1024, "norm+swiglu"),
          (1024, 8192, "residual"), (512, 8192, "f32"), (512, 256, "norm+swiglu"), (512, 256, "gather")]


def _setup(N, K, seed, dev, Bmax):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF).to(dev)
    w = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)
    table = torch.randn(64, K, generator=g).to(BF).to(dev)
    bank = Bank(g, dev, N)
    x = torch.randn(Bmax, K, generator=g).to(BF).to(dev)
    R = torch.randn(Bmax, N, generator=g).to(BF).to(dev)
    idx = torch.randint(0, 50, (Bmax,), generator=g).to(torch.int32).to(dev)
    t = torch.randn(Bmax, bank.kx, generator=g).to(BF).to(dev)
    return g, W, w, table, bank, x, R, idx, t


@pytest.mark.parametrize("N,K,form", SHAPES, ids=[f"{n}x{k}-{f}" for n, k, f in SHAPES])
def test_kext_rows_small_batch_bits(dev, N, K, form):
    """B <= 4: row b is the one-row gemv_kext with its adapter; a -1 row is gemv_ex at the same B."""
    from csm.hip import ops
    g, W, w, table, bank, x, R, idx, t = _setup(N, K, N + K, dev, 4)
    for B, ids in ((1, [2]), (1, [-1]), (2, [1, -1]), (3, [0, 2, 0]), (4, [2, -1, 0, 1])):
        ra = torch.tensor(ids, dtype=torch.int32, device=dev)
        xs, Rs, ix, ts = x[:B].contiguous(), R[:B].contiguous(), idx[:B].contiguous(), t[:B].contiguous()
        y = product(ops, form, W, w, table, xs, Rs, ix, out_for(form, B, N, dev), ("rows", ts, bank, ra))
        plain = product(ops, form, W, w, table, xs, Rs, ix, out_for(form, B, N, dev))
        gclose(f"{form} B={B}", y, reference(form, W, w, table, xs, Rs, ix, ts, bank, ra.cpu()), 2e-2)
        for b, a in enumerate(ids):
            if a < 0:
                assert torch.equal(y[b], plain[b]), (form, N, K, B, b, "-1 row vs gemv_ex")
                continue
            y1 = product(ops, form, W, w, table, xs[b:b + 1], Rs[b:b + 1], ix[b:b + 1], out_for(form, 1, N, dev),
                         ("one", ts[b:b + 1], bank.Bx[a], bank.bias[a]))
            assert torch.equal(y1[0], y[b]), (form, N, K, B, b, "row vs one-row gemv_kext")


WIDE = [(3072, 2048, "norm"), (16384, 2048, "norm+swiglu"), (2048, 8192, "residual"), (2112, 1024, "f32"), (1024, 2048, "gather"),
        (512, 256, "norm+swiglu"), (300, 512, "residual")]


@pytest.mark.parametrize("N,K,form", WIDE, ids=[f"{n}x{k}-{f}" for n, k, f in WIDE])
def test_kext_rows_wide_batch(dev, N, K, form):
    """B = 5..16: fp32 accuracy; a row keeps its bits across B, positions, batch-mates and their adapters; -1 rows are gemv_ex."""
    from csm.hip import ops
    g, W, w, table, bank, x, R, idx, t = _setup(N, K, 3 * N + K, dev, 16)
    ids = torch.tensor([0, -1, 2, 1, 1, 0, -1, 2, 0, 1, 2, -1, 0, 2, 1, 0], dtype=torch.int32)

    def run(xs, Rs, ix, ts, rid):
        B = xs.shape[0]
        return product(ops, form, W, w, table, xs.contiguous(), Rs.contiguous(), ix.contiguous(), out_for(form, B, N, dev),
                       ("rows", ts.contiguous(), bank, rid.to(dev).contiguous()))

    y16 = run(x, R, idx, t, ids)
    gclose(f"{form} B=16", y16, reference(form, W, w, table, x, R, idx, t, bank, ids), 2e-2)
    plain16 = product(ops, form, W, w, table, x, R, idx, out_for(form, 16, N, dev))
    for b in range(16):
        if ids[b] < 0:
            assert torch.equal(y16[b], plain16[b]), (form, b, "-1 row vs gemv_ex at B = 16")
    perm = torch.tensor([9, 2, 15, 0, 7])
    y5 = run(x[perm], R[perm], idx[perm], t[perm], ids[perm])
    assert torch.equal(y5, y16[perm]), (form, "B = 5 subset vs B = 16")
    plain5 = product(ops, form, W, w, table, x[perm].contiguous(), R[perm].contiguous(), idx[perm].contiguous(), out_for(form, 5, N, dev))
    for j, b in enumerate(perm.tolist()):
        if ids[b] < 0:
            assert torch.equal(y5[j], plain5[j]), (form, "-1 row vs gemv_ex at B = 5")
    # other positions, other batch-mates with other adapters
    at = torch.tensor([4, 13, 1, 8, 11])
    x3 = torch.randn(16, K, generator=g).to(BF).to(dev)
    R3 = torch.randn(16, N, generator=g).to(BF).to(dev)
    t3 = torch.randn(16, bank.kx, generator=g).to(BF).to(dev)
    idx3 = torch.randint(0, 50, (16,), generator=g).to(torch.int32).to(dev)
    ids3 = torch.tensor([2, 1, 0, -1] * 4, dtype=torch.int32)
    x3[at], R3[at], t3[at], idx3[at], ids3[at] = x[perm], R[perm], t[perm], idx[perm], ids[perm]
    y3 = run(x3, R3, idx3, t3, ids3)
    assert torch.equal(y3[at], y16[perm]), (form, "other positions and batch-mates")
    for B in (6, 12):
        assert torch.equal(run(x[:B], R[:B], idx[:B], t[:B], ids[:B]), y16[:B]), (form, B)


def test_rows_abi_limits(dev):
    from csm.hip import ops
    g = torch.Generator().manual_seed(5)
    W = (torch.randn(64, 256, generator=g) * 0.02).to(BF).to(dev)
    bank = Bank(g, dev, 64, A=1)
    x = torch.randn(17, 256, generator=g).to(BF).to(dev)
    t = torch.zeros(17, 32, dtype=BF, device=dev)
    ra = torch.zeros(17, dtype=torch.int32, device=dev)
    with pytest.raises(Exception, match="B=17"):
        ops.gemv_kext_rows(x, W, torch.empty(17, 64, dtype=BF, device=dev), t, bank.Bx_tab, ra, 32, 32)
    with pytest.raises(Exception, match="B=17"):
        ops.lora_project_rows(x, ptrs([torch.zeros(256, 32, dtype=BF, device=dev)], dev), t, ra,
                              torch.ones(1, device=dev), 32, 32)
    with pytest.raises(Exception, match="bad extension"):
        ops.gemv_kext_rows(x[:4], W, torch.empty(4, 64, dtype=BF, device=dev), t[:4], bank.Bx_tab, ra[:4], 12, 32)


# ----------------------------------------------------------------------------------------------------------- engine
def tiny_model(seed=11):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", TINY.text_vocab, TINY.audio_vocab, TINY.n_codebooks), device="cuda")
    m.load_state_dict(O.init_params(TINY, seed=seed))
    return m


def adapter(m, seed, modules=ALL7, r=8, alpha=16.0, use_bias=False, b_scale=0.05):
    """A generation-only adapter set of ``m`` with non-zero B (and bias)."""
    from csm.training.lora import LoRAState
    st = LoRAState(m, r, alpha, 0.0, list(modules), None, use_bias, seed=seed, grad=False)
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    with torch.no_grad():
        for ad in st.adapters.values():
            ad.B[:, :r].copy_((torch.randn(ad.B.shape[0], r, generator=g, device="cuda") * b_scale).to(BF))
            if ad.bias is not None:
                ad.bias.copy_((torch.randn(ad.bias.shape[0], generator=g, device="cuda") * b_scale).to(BF))
    return st


def noise(step, B):
    g = torch.Generator().manual_seed(500 + step)
    return [torch.empty(16, TINY.audio_vocab).exponential_(1, generator=g)[:B] for _ in range(TINY.n_codebooks)]


def run_ragged(m, tk, mk, rows, adapters=None, graph=True, n=5):
    """``n`` frames of a ragged batch (prompts ``tk`` / ``mk``) with the noise rows ``rows`` of a 16-row draw."""
    B, K = len(tk), TINY.n_codebooks
    m.use_hip_graph = graph
    m.setup_caches(B)
    m.reset_caches()
    amask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1)
    try:
        out = [m.engine.generate_first_frames(tk, mk, 0.8, 12, noise=[q[rows] for q in noise(0, 16)], adapters=adapters).cpu()]
        for step in range(1, n):
            cur = torch.cat([out[-1].long(), torch.zeros(B, 1, dtype=torch.long)], 1).unsqueeze(1)
            out.append(m.generate_frame(cur, amask.repeat(B, 1, 1), torch.ones(B, 1, dtype=torch.long), 0.8, 12,
                                        noise=[q[rows] for q in noise(step, 16)]).cpu())
    finally:
        m.use_hip_graph = True
    return torch.stack(out)


def prompts(B, seed):
    tokens, mask, _ = O.synthetic_batch(TINY, B, 20, seed=seed)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(8, 20, (B,), generator=g).tolist()
    return [tokens[b, :lens[b]] for b in range(B)], [mask[b, :lens[b]] for b in range(B)]


def live_single(m, state, tk, mk, b, graph):
    """Today's path: row b alone, with ``state`` live as model.lora (or no adapters)."""
    prev = m.lora
    m.lora = state
    try:
        return run_ragged(m, tk[b:b + 1], mk[b:b + 1], [b], graph=graph)[:, 0]
    finally:
        m.lora = prev


def check_mixed_small(m, states, graph_modes=(False, True), seed=21):
    tk, mk = prompts(len(states), seed)
    rows = list(range(len(states)))
    outs = {}
    for graph in graph_modes:
        got = run_ragged(m, tk, mk, rows, adapters=states, graph=graph)
        for b, st in enumerate(states):
            ref = live_single(m, st, tk, mk, b, graph)
            assert torch.equal(got[:, b], ref), f"row {b} (graph={graph}) differs from its one-utterance run with the adapter live"
        outs[graph] = got
    return outs


def test_mixed_batch_small_matches_live_single(dev):
    """adapters = [a, b, None, a] at B = 4: every row equals its one-utterance run with that adapter live as model.lora (None: no
    adapters), eager and graph."""
    m = tiny_model()
    a, b = adapter(m, 1), adapter(m, 2)
    outs = check_mixed_small(m, [a, b, None, a])
    assert torch.equal(outs[False], outs[True])
    # the adapters change the output (otherwise nothing above is tested)
    tk, mk = prompts(4, 21)
    assert not torch.equal(run_ragged(m, tk, mk, [0, 1, 2, 3], graph=False), outs[False])


def test_sixteen_rows_mixed(dev):
    """16 rows, 4 distinct adapters and some None: batch invariance of the per-row path, graph == eager, and against the recompute
    path (training forward with the row's adapter as model.lora, teacher-forced)."""
    m = tiny_model()
    bank = [adapter(m, s) for s in (1, 2, 3, 4)]
    B, K = 16, TINY.n_codebooks
    assign = [0, 1, None, 2, 3, 0, None, 1, 2, 3, 0, None, 1, 3, 2, 0]
    states = [None if a is None else bank[a] for a in assign]
    tokens, mask, _ = O.synthetic_batch(TINY, B, 20, seed=12)
    amask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], dim=1).unsqueeze(1)

    def run(st_rows, graph=False, use_cache=True, history=None, order=None, n=6):
        order = list(range(B)) if order is None else order
        m.use_hip_graph, m.use_kv_cache = graph, use_cache
        m.setup_caches(B)
        m.reset_caches()
        ct, cm, cp = tokens[order, :11], mask[order, :11], torch.arange(11).unsqueeze(0).repeat(B, 1)
        out = []
        try:
            for step in range(n):
                f = m.generate_frame(ct, cm, cp, 0.8, 12, noise=[q[order] for q in noise(step, 16)], adapters=st_rows).cpu()
                out.append(f)
                nxt = history[step][order] if history is not None else f
                ct, cm, cp = torch.cat([nxt.long(), torch.zeros(B, 1, dtype=torch.long)], 1).unsqueeze(1), amask, cp[:, -1:] + 1
        finally:
            m.use_hip_graph, m.use_kv_cache = True, True
        return torch.stack(out)

    eager = run(states)
    graph = run(states, graph=True)
    assert torch.equal(eager, graph), "graph replay must reproduce the eager frames with per-row adapters"
    # the same utterances in another order (other positions, other batch-mates): the same frames per utterance
    order = [5, 11, 0, 14, 2, 9, 7, 1, 15, 3, 12, 6, 10, 4, 13, 8]
    again = run([states[o] for o in order], graph=True, order=order)
    assert torch.equal(again, eager[:, order]), "a row's frames depend on its own utterance and adapter only"
    # recompute path: each adapter (and None) in turn as model.lora over the whole batch, teacher-forced on the decode frames
    rc = torch.empty_like(eager)
    for st in bank + [None]:
        m.lora = st
        try:
            r = run(None, use_cache=False, history=eager)
        finally:
            m.lora = None
        for b in range(B):
            if states[b] is st:
                rc[:, b] = r[:, b]
    assert torch.equal(eager[0, :, 0], rc[0, :, 0]), "the prefill frame's first codebook"
    agree = (eager == rc).float().mean().item()
    assert agree >= 0.9, f"per-row KV-cache path and recompute agree on only {agree:.1%} of the codes"
    plain = run(None)
    assert not torch.equal(plain, eager)


def test_bank_bias_ranks_errors_and_updates(dev):
    from csm.lora_bank import LoRABank
    m = tiny_model()
    # biases, and different r / alpha under one padded rank (r = 5 and 8 -> r_pad 8): per-row scales
    a = adapter(m, 5, r=8, alpha=16.0, use_bias=True)
    b = adapter(m, 6, r=5, alpha=7.0, use_bias=True)
    check_mixed_small(m, [b, None, a], graph_modes=(True,), seed=23)
    bank = LoRABank(m)
    bank.add("a", a)
    bank.add("b", b)
    with pytest.raises(ValueError, match="use_bias"):
        bank.add("c", adapter(m, 7))
    with pytest.raises(ValueError, match="target_modules"):
        bank.add("c", adapter(m, 7, modules=["q_proj", "v_proj"], use_bias=True))
    with pytest.raises(ValueError, match="r_pad"):
        bank.add("c", adapter(m, 7, r=12, use_bias=True))
    with pytest.raises(ValueError, match="unknown LoRA adapter"):
        bank.resolve(["a", "nope"])
    # a live model.lora together with per-row adapters
    tk, mk = prompts(2, 24)
    m.lora = adapter(m, 8)
    try:
        with pytest.raises(ValueError, match="model.lora"):
            run_ragged(m, tk, mk, [0, 1], adapters=[a, None])
    finally:
        m.lora = None
    # new weights written into a bank entry between calls are seen (also by a new capture); restoring them restores the output
    ref = run_ragged(m, tk, mk, [0, 1], adapters=[a, b])
    with torch.no_grad():
        for ad in a.adapters.values():
            ad.B.mul_(-1.0)
    assert not torch.equal(run_ragged(m, tk, mk, [0, 1], adapters=[a, b]), ref)
    with torch.no_grad():
        for ad in a.adapters.values():
            ad.B.mul_(-1.0)
    assert torch.equal(run_ragged(m, tk, mk, [0, 1], adapters=[a, b]), ref)


def test_sixteen_mixed_rows_at_csm1b_width_eager_vs_graph(dev):
    """One-layer stacks of CSM-1B's width, all seven modules, 16 rows with four adapters and some None: eager == graph."""
    from csm.models.model import Model, ModelArgs
    from csm.training.lora import LoRAState
    m = Model(ModelArgs("llama-1B-L1", "llama-100M-L1", 300, 2051, 32), device="cuda", seed=0)
    bank = []
    for s in range(4):
        st = LoRAState(m, 8, 16.0, 0.0, ALL7, None, False, seed=s, grad=False)
        g = torch.Generator(device="cuda").manual_seed(40 + s)
        with torch.no_grad():
            for ad in st.adapters.values():
                ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=g, device="cuda") * 0.02).to(BF))
        bank.append(st)
    states = [bank[i % 4] if i % 5 else None for i in range(16)]
    K, B = 32, 16
    g = torch.Generator().manual_seed(2)
    tokens = torch.zeros(B, 12, K + 1, dtype=torch.long)
    tokens[:, :, K] = torch.randint(0, 300, (B, 12), generator=g)
    mask = torch.zeros(B, 12, K + 1, dtype=torch.bool)
    mask[:, :, K] = True
    amask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1)

    def run(graph):
        m.use_hip_graph = graph
        m.reset_caches()
        out = []
        ct, cm, cp = tokens, mask, torch.arange(12).unsqueeze(0).repeat(B, 1)
        try:
            for step in range(4):
                gq = torch.Generator().manual_seed(700 + step)
                q = [torch.empty(B, 2051).exponential_(1, generator=gq) for _ in range(K)]
                f = m.generate_frame(ct, cm, cp, 0.9, 50, noise=q, adapters=states).cpu()
                out.append(f)
                ct, cm, cp = torch.cat([f.long(), torch.zeros(B, 1, dtype=torch.long)], 1).unsqueeze(1), amask, cp[:, -1:] + 1
        finally:
            m.use_hip_graph = True
        return torch.stack(out)

    m.setup_caches(B)
    assert torch.equal(run(False), run(True))


# ----------------------------------------------------------------------------------------------------------- API
class _Tok:
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


def _tiny32(seed=2):
    from csm.models.model import Model, ModelArgs
    return Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 32), device="cuda", seed=seed)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    S, K = 16, 32
    tokens = torch.zeros(2, S, K + 1, dtype=torch.long)
    tokens[:, :, :K] = torch.randint(0, 2051, (2, S, K), generator=g)
    tokens[:, :, K] = torch.randint(0, 300, (2, S), generator=g)
    masks = torch.ones(2, S, K + 1, dtype=torch.bool)
    targets = torch.randint(0, 2051, (2, S, K), generator=g)
    return {"input_tokens": tokens, "input_masks": masks, "target_audio_tokens": targets}


def test_adapter_files_generator_and_cli(dev, tmp_path, monkeypatch):
    """A trainer's saved adapter, loaded into the bank, speaks exactly as the trainer's live adapter; generate_batch with unknown
    names or the wrong length raises; csm-generate --lora-adapter writes what Generator.generate(adapter=...) gives."""
    from csm.cli import generate as cli
    from csm.codec import MimiCodec
    from csm.generator import Generator
    from csm.training.lora_trainer import CSMLoRATrainer
    codec = MimiCodec(_hf_mimi(5).state_dict(), device="cuda")
    tr = CSMLoRATrainer("", str(tmp_path / "o"), model=_tiny32(), device="cuda", learning_rate=5e-3, target_modules=ALL7)
    for s in (1, 2):
        tr.train_step(_batch(s))
    path = tr.save_model(str(tmp_path / "voice.safetensors"), "lora")
    m = tr.model
    gen = Generator(m, text_tokenizer=_Tok(), audio_tokenizer=codec)
    torch.manual_seed(3)
    live = gen.generate("hello there", 0, [], max_audio_length_ms=400)
    live_state = m.lora
    m.lora = None
    try:
        gen.load_adapter("voice", path)
        gen.add_adapter("trainer", live_state)
        assert gen.adapters == ["voice", "trainer"]
        torch.manual_seed(3)
        banked = gen.generate("hello there", 0, [], max_audio_length_ms=400, adapter="voice")
        assert torch.equal(banked, live), "a loaded adapter must speak as the trainer's live one"
        torch.manual_seed(3)
        assert torch.equal(gen.generate("hello there", 0, [], max_audio_length_ms=400, adapter="trainer"), live)
        torch.manual_seed(3)
        plain = gen.generate("hello there", 0, [], max_audio_length_ms=400)
        assert not torch.equal(plain, live), "the trained adapter changes the output"
        with pytest.raises(ValueError, match="unknown LoRA adapter"):
            gen.generate_batch(["a", "b"], [0, 1], [[], []], max_audio_length_ms=400, adapters=["voice", "nope"])
        with pytest.raises(ValueError, match="adapter names"):
            gen.generate_batch(["a", "b"], [0, 1], [[], []], max_audio_length_ms=400, adapters=["voice"])
        outs = gen.generate_batch(["a", "b", "c"], [0, 1, 0], [[], [], []], max_audio_length_ms=400, adapters=["voice", None, "trainer"])
        assert len(outs) == 3
        # streaming with an adapter: the chunks are generate()'s audio
        torch.manual_seed(3)
        chunks = list(gen.generate_stream("hello there", 0, [], max_audio_length_ms=400, chunk_frames=2, adapter="voice"))
        assert torch.equal(torch.cat(chunks), live)
        # the CLI
        monkeypatch.setattr(cli, "load_csm_1b", lambda *a, **k: gen)
        argv = ["--model-path", "m.pt", "--text", "hi there", "--mimi-weights", "x", "--text-tokenizer", "y", "--max-audio-length-ms", "400",
                "--lora-adapter", path]
        torch.manual_seed(4)
        assert cli.main(argv + ["--output", str(tmp_path / "cli.wav")]) == 0
        torch.manual_seed(4)
        assert cli.main(argv + ["--output", str(tmp_path / "cli_stream.wav"), "--stream", "--chunk-frames", "2"]) == 0
        torch.manual_seed(4)
        ref = gen.generate("hi there", 0, [], max_audio_length_ms=400, adapter="voice")
        gen.save_wav(str(tmp_path / "ref.wav"), ref)
        with wave.open(str(tmp_path / "ref.wav")) as w:
            assert w.getnframes() > 0
        want = (tmp_path / "ref.wav").read_bytes()
        assert (tmp_path / "cli.wav").read_bytes() == want
        assert (tmp_path / "cli_stream.wav").read_bytes() == want
    finally:
        m.lora = live_state
        # free the captured frame graph now: it was captured under inference mode (Generator.generate), and while it lives the
        # graph-safe RNG state it registered would refuse a later capture outside inference mode (the model is in a reference
        # cycle, so it is not freed on return)
        m.reset_caches()
        import gc
        gc.collect()
