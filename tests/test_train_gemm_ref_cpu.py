"""Proves tests/train_gemm_ref.py, the judge of the training GEMM kernels, on the CPU:
  * its references against torch's own float64 machinery (einsum, F.silu, autograd) and the oracle's rope, to 1e-12;
  * that fp32 restatements of the kernels' arithmetic - accumulation over K in blocks of 32 in forward, reversed and 4-way-split
    order, the epilogue in fp32, one bf16 rounding - fit EVERY bound of EVERY case, guards included;
  * that every listed wrong restatement is rejected on at least one case of its branch;
  * that the restated tile lists of the grouped launches cover every tile exactly once;
  * that no case's bound is vacuous, and that the case table reaches the branches it names."""
import pytest
import torch
import torch.nn.functional as Fn

import train_gemm_ref as G

F64, BF16 = torch.float64, torch.bfloat16
_memo = {}


def _ref(c):
    """Inputs and embedded reference of a case, once per data key."""
    k = c.data_key()
    if k not in _memo:
        i = G.inputs(c)
        _memo[k] = (i, G.embedded_reference(i))
    return _memo[k]


def _close(name, a, b):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-12 * scale, f"{name}: {float((a - b).abs().max()):.3e}"


def _independent(i):
    """The same contracts through other torch machinery: einsum for the products, F.silu and autograd for SwiGLU, the oracle's
    rope for the rotation, autograd for the two gradients of a Linear layer."""
    from oracle import csm_oracle as O
    c = i["c"]
    d = lambda t: t.double()                                      # noqa: E731
    if c.kind == "gemm":
        a = d(i["A"]).transpose(1, 2) if c.ta else d(i["A"])
        b = d(i["B"]) if c.tb else d(i["B"]).transpose(1, 2)
        acc = torch.einsum("bmk,bkn->bmn", a, b)
        if c.kx:
            acc = acc + torch.einsum("mk,nk->mn", d(i["xA"]), d(i["xB"]))
        if c.epi == 2:
            gu = d(i["gu"]).requires_grad_(True)
            (Fn.silu(gu[:, 0::2]) * gu[:, 1::2]).backward(c.alpha * acc[0])
            return {"C": gu.grad[None]}
        v = c.alpha * acc + (d(i["R"]) if c.R is not None else 0.0)
        if c.epi == 1:
            return {"C": v, "act": Fn.silu(v[..., 0::2]) * v[..., 1::2]}
        if c.epi == 3 and c.p0:
            pos = (torch.arange(c.M) % c.S)[None]
            rot = O.rope(v[..., :c.p0].reshape(1, c.M, c.p0 // c.hd, c.hd), i["table"].double(), pos).reshape(1, c.M, c.p0)
            v = torch.cat([rot, v[..., c.p0:]], -1)
        return {"C": v}
    if c.kind == "pair":
        x, w = d(i["X"]).requires_grad_(True), d(i["W"]).requires_grad_(True)
        if c.epi == 2:                                            # y = act w2^T, act = silu(g) up
            gu = d(i["gu"]).requires_grad_(True)
            (Fn.silu(gu[:, 0::2]) * gu[:, 1::2] @ w.t()).backward(d(i["dY"]))
            dX = gu.grad
            x2 = d(i["X"])
            dW = d(i["dY"]).t() @ x2
        else:
            (x @ w.t()).backward(d(i["dY"]))
            dX, dW = x.grad, w.grad
        return {"dX": dX, "dW": c.alpha * dW + (d(i["dW0"]) if c.acc else 0.0)}
    if c.kind == "wgrads":
        out = {}
        for k in range(len(c.probs)):
            w = torch.zeros(*c.probs[k], dtype=F64, requires_grad=True)
            (d(i["X"][k]) @ w.t()).backward(d(i["dY"][k]))
            out[f"dW{k}"] = c.alpha * w.grad + (d(i["dW0"][k]) if c.acc else 0.0)
        return out
    if c.kind == "splitk":
        return {"dW": c.alpha * torch.einsum("mn,mk->nk", d(i["dY"]), d(i["X"])) + (d(i["dW0"]) if c.acc else 0.0)}
    return {"out": c.alpha * torch.einsum("mk,nk->mn", d(i["X"]), d(i["Wt"]))}


SMALL = [c for c in G.CASES if not c.big]


@pytest.mark.parametrize("branch", G.BRANCHES)
def test_reference_matches_torch(branch):
    n = 0
    for c in [c for c in SMALL if c.branch == branch] or [c for c in G.CASES if c.branch == branch][-1:]:
        i = _ref(c)[0]
        r, ind = G.reference(i), _independent(i)
        assert set(r) == set(ind) == set(G.layouts(c))
        for k in r:
            _close(f"{c.name}.{k}", r[k][0].reshape(ind[k].shape), ind[k])
            assert bool((r[k][1] >= 0).all()) and bool(torch.isfinite(r[k][1]).all()), f"{c.name}.{k}: slack"
        n += 1
    assert n


@pytest.mark.parametrize("branch", G.BRANCHES)
def test_fp32_restatements_fit_every_bound(branch):
    worst = 0.0
    for c in {c.data_key(): c for c in G.CASES if c.branch == branch}.values():       # (cases that differ in the kernel only share one)
        i, emb = _ref(c)
        for order in G.ORDERS:
            worst = max(worst, G.judge_case(f"restate.{order}", c, G.restate(i, order), emb))
    assert worst <= 1.0


def _applies(mut, c):
    if mut == "transposed":
        return c.kind == "gemm" and c.M == c.N and c.epi != 2
    if mut == "drop_k64":
        return c.kind == "gemm" and c.K >= 128
    if mut in ("alpha_after_residual", "residual_twice"):
        return c.kind == "gemm" and c.R is not None and (mut == "residual_twice" or c.alpha != 1.0)
    if mut == "kext_after_epilogue":
        return c.kx > 0 and c.epi != 0
    if mut == "bwd_no_factor":
        return c.epi == 2
    if mut == "accumulate_ignored":
        return c.acc == 1
    if mut == "drop_last_k":
        return c.kind in ("gemm", "pair", "skinny")
    if mut == "clamp_last_row":
        return c.kind == "gemm"
    return True


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_wrong_restatements_are_rejected(mut):
    for branch in G.MUTANT_BRANCH[mut]:
        cases = [c for c in SMALL if c.branch == branch and _applies(mut, c)]
        assert cases, f"{mut}: no case of branch {branch} to try it on"
        rejected = 0
        for c in cases:
            i, emb = _ref(c)
            try:
                G.judge_case(f"mutant.{mut}", c, G.restate(i, "fwd", mut), emb)
            except AssertionError:
                rejected += 1
        print(f"MUTANT {mut} {branch}: rejected on {rejected} of {len(cases)} cases")
        assert rejected >= 1, f"{mut} passes every case of branch {branch}"
        if mut == "guard_overwritten":
            assert rejected == len(cases), f"a guard element may change unnoticed in branch {branch}"


def test_tile_lists_cover_every_tile_once():
    for c in (c for c in G.CASES if c.kind in ("pair", "wgrads")):
        t = G.grouped_tiles(c)
        items = G.pair_map(*t) if c.kind == "pair" else G.multi_map(t)
        assert G.covers_once(items, t), c.name
    for na in list(range(1, 80)) + [96, 128, 160, 512]:           # beyond the cases: every ratio, whole periods and both run-out tails
        for nb in list(range(1, 80)) + [96, 128, 160, 512]:
            assert G.covers_once(G.pair_map(na, nb), [na, nb]), (na, nb)
    seen = set()
    for c in (c for c in G.CASES if c.kind == "pair"):
        na, nb = G.grouped_tiles(c)
        ra, rb = G.pair_ratio(na, nb)
        seen.add(("a" if ra > 8 else "b" if rb > 8 else "=", min(na // ra, nb // rb) > 0))
    assert {("a", False), ("b", False), ("a", True), ("b", True), ("=", False)} <= seen, seen
    for tiles in ([1], [3, 1], [1] * 12, [5, 0 + 2, 7], [40, 1, 1, 9]):
        assert G.covers_once(G.multi_map(tiles), tiles), tiles


def test_no_case_has_a_vacuous_bound():
    """Median over a buffer's judged window of bound / hulp(|ref|) - the bound in units of the output's own rounding, which is
    at least as strict as bound / max(|ref|, hulp) - stays below 4 for every bf16 output."""
    for c in G.CASES:
        emb = _ref(c)[1]
        for name, l in G.layouts(c).items():
            if l.dtype != BF16:
                continue
            ref, sl = G.view(emb[name][0], l), G.view(emb[name][1], l)
            h = G.hulp(ref)
            ratio = (G.hulp(ref.abs() + sl) + sl) / h
            assert float(ratio.median()) < 4.0, f"{c.name}.{name}: median bound / hulp {float(ratio.median()):.2f}"
            assert float((G.hulp(ref.abs() + sl) + sl).reshape(-1).median() / torch.maximum(ref.abs(), h).reshape(-1).median()) < 4.0


def test_case_table_reaches_its_branches():
    k = {c.name: G.expected_kernel(c) for c in G.CASES}
    for c in G.CASES:
        if c.kind != "gemm":
            continue
        v = 1 if c.route == "pinned" else c.variant
        want = {0: "gemm_kernel", 1: "gemm_kernel", 3: "gemm256p_kernel", 4: "gemm256w4"}[v]
        if c.kx and dict(c.tuning).get(7, 1) == 0:
            want = "gemm256p_kernel"
        assert k[c.name].startswith(want), (c.name, k[c.name])
        assert k[c.name].endswith("false>") == (v == 0 or (v == 1 and c.K % 64 != 0)) or not k[c.name].startswith("gemm_kernel"), c.name
    for c in (c for c in G.CASES if c.branch == "n6"):
        on = dict(c.tuning).get(8, 1)
        assert G.n6_rule(c, 1), c.name                            # the shape selects the 256 x 192 tile ...
        assert k[c.name] == ("gemm256w4n6_kernel<0>" if on else "gemm256w4_kernel<0, 0, unsigned short>"), c.name   # ... the switch takes it away
    for c in (c for c in G.CASES if c.branch == "rounds"):
        assert G.tiles256(c.M, c.N) > 256 and not G.n6_rule(c), c.name
    for c in (c for c in G.CASES if c.kind == "splitk"):
        assert G.splitk_splits(c.M, c.N, c.K) == 8 and k[c.name] == "gemm_kernel<1, 1, float, true>", c.name
    for c in (c for c in G.CASES if c.kind == "wgrads"):
        assert ("fallback" in c.name) == (not k[c.name].startswith("gemm256w4_") and c.route == "multi"), (c.name, k[c.name])
    # every operand order on every tile kernel, and the alignment classes of the output base
    for v in G.TILE_VARIANTS:
        assert {(c.ta, c.tb) for c in G.CASES if c.branch == "orders" and c.variant == v} == set(G.ORDER4)
    offs = {(c.off_c % 8, (G.layouts(c)["C"].ld) % 8) for c in G.CASES if c.branch == "align"}
    assert {(1, 0), (4, 0), (0, 0), (0, 4)} <= offs and any(ld % 2 for _, ld in offs)
    assert G.prefer_256(8192, 8192, 2048, 1) and not G.prefer_256(200, 136, 64, 1) and not G.prefer_256(8192, 8192, 72, 1)


def test_guards_surround_every_window():
    for c in SMALL[::7]:
        for name, l in G.layouts(c).items():
            ref, sl = _ref(c)[1][name]
            w = torch.zeros(G.flat_len(l), dtype=torch.bool)
            G.view(w, l).fill_(True)
            assert int(w.sum()) == l.batch * l.rows * l.cols and bool((sl[~w] == -1).all()) and bool((sl[w] >= 0).all())
            assert not bool(w[:l.off + G.GR * l.ld].any()) and not bool(w[-(G.GR * l.ld):].any())
            assert bool((ref[~w] == float(G.sentinel(l.dtype))).all())
