"""Proves tests/train_ops_ref.py - the float64 reference, the bounds and the cases of the training step's bandwidth kernels -
with no GPU and no kernel involved:

  * every float64 reference agrees with torch's own float64 machinery (autograd, F.cross_entropy, optim.AdamW, index_add_) to
    1e-12 of the row's largest value;
  * an fp32 torch restatement of every kernel (the same operations at statement level, torch's fp32 exp / rsqrt / log) passes
    ``judge`` on every case: the bounds are not too tight for a correct implementation.  The worst |err| / bound per kernel is
    printed (``UTIL``) and recorded in DESIGN.md;
  * deliberately wrong restatements fail ``judge`` on at least one case each: the bounds and the cases are not too weak."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as T

F64 = torch.float64
_cache = {}


def _case(op, k):
    """(inputs, reference) of case k of an op, computed once."""
    if (op, k) not in _cache:
        o = T.OPS[op]
        inp = o.inputs(o.cases[k])
        _cache[(op, k)] = (inp, o.ref(inp))
    return _cache[(op, k)]


def _close(a, b, what, scale=None):
    if scale is None:
        scale = torch.maximum(a.abs(), b.abs()).reshape(a.shape[0], -1).amax(1).reshape(-1, *[1] * (a.dim() - 1)) if a.dim() > 1 else torch.maximum(a.abs(), b.abs())
    bad = (a - b).abs() > 1e-12 * scale
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ by more than 1e-12 of the row's maximum; worst {float(((a - b).abs() / scale.clamp(min=1e-300)).max()):.2e}"


# ------------------------------------------------------------------------------------------------------- against torch float64
@pytest.mark.parametrize("c", [T.RmsCase(5, 264, True, True, True), T.RmsCase(5, 2056, False, True, True), T.RmsCase(1, 8, True, True, True)], ids=str)
def test_rmsnorm_reference_is_torch_autograd(c):
    i = T.rms_inputs(c)
    x = i["x"].double().requires_grad_()
    w = i["w"].double().requires_grad_()
    r = torch.rsqrt((x * x).mean(1) + T.EPS)
    y = x * r[:, None] * w
    fwd = T.rms_fwd_ref(i)
    _close(fwd["y"][0], y.detach(), "y")
    _close(fwd["rstd"][0], r.detach(), "rstd")
    dx, dw = torch.autograd.grad(y, (x, w), i["dy"].double())
    bwd = T.rms_bwd_ref(dict(i, rstd=r.detach()))
    _close(bwd["dx"][0], dx + (i["dres"].double() if c.dres else 0), "dx")
    _close(bwd["dscale"][0], dw, "dscale")


@pytest.mark.parametrize("c", T.SWIGLU_CASES[:6], ids=str)
def test_swiglu_reference_is_torch_autograd(c):
    i = T.swiglu_inputs(c)
    gu = i["gu"].double().requires_grad_()
    out = F.silu(gu[:, 0::2]) * gu[:, 1::2]
    _close(T.swiglu_fwd_ref(i)["out"][0], out.detach(), "out")
    (dgu,) = torch.autograd.grad(out, gu, i["dout"].double())
    _close(T.swiglu_bwd_ref(i)["dgu"][0], dgu, "dgu")


@pytest.mark.parametrize("c", T.ROPE_CASES[:-1], ids=lambda c: c.name)
def test_rope_reference_is_a_complex_rotation_and_its_transpose(c):
    i = T.rope_inputs(c)
    W = c.nh * c.hd
    x = i["qkv"][:, :W].double().requires_grad_()
    t = i["table"].double()[i["pos"].long()][:, None]
    rot = torch.view_as_real(torch.view_as_complex(x.reshape(c.M, c.nh, c.hd // 2, 2)) * torch.complex(t[..., 0], t[..., 1])).reshape(c.M, W)
    if not c.inverse:
        _close(T.rope_ref(i)["rot"][0], rot.detach(), "rotation")
    else:                                                     # the inverse is the gradient of the forward rotation
        (gx,) = torch.autograd.grad(rot, x, x.detach())
        _close(T.rope_ref(i)["rot"][0], gx, "transpose rotation")
    assert torch.equal(T.rope_ref(i)["rest"][0], i["qkv"][:, W:])


@pytest.mark.parametrize("k", range(len(T.CE_CASES)), ids=lambda k: f"{T.CE_CASES[k].name}_R{T.CE_CASES[k].R}")
def test_ce_reference_is_torch_cross_entropy(k):
    c = T.CE_CASES[k]
    i, ref = _case("ce_fwd_bwd", k)
    x = i["logits"][:, :c.V].double().requires_grad_()
    loss = F.cross_entropy(x, i["targets"].clamp(min=-100).where(i["targets"] >= 0, torch.tensor(-100)), reduction="none", ignore_index=-100)
    _close(ref["loss_rows"][0], loss.detach(), "loss_rows", scale=x.detach().abs().amax(1))      # lse - x_t cancels: of the logits' size
    if c.has_d:
        (gx,) = torch.autograd.grad(loss.sum() * T.CE_GSCALE, x)
        _close(ref["dlogits"][0][:, :c.V], gx, "dlogits", scale=torch.tensor(T.CE_GSCALE))        # p - onehot cancels: of the terms' size
        assert bool((ref["dlogits"][0][:, c.V:] == 0).all()) and bool((ref["dlogits"][1][:, c.V:] < 0).all())        # pad columns: exactly 0
    kernels = {T.ce_kernel_chain(cc)[0] for cc in T.CE_CASES}
    assert kernels == {"wave4", "wave9", "wave12", "block"}
    assert T.ce_kernel_chain(c)[0] == {"nc4": "wave4", "nc9": "wave9", "nc12": "wave12", "ldd_lt_ldl": "wave4", "no_dlogits": "wave9",
                                       "pad_garbage": "wave4"}.get(c.name, "block")


@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adamw_reference_is_torch_adamw(wd):
    g = torch.Generator().manual_seed(3)
    p = torch.randn(64, generator=g, dtype=F64)
    ref_p = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref_p], lr=T.ADAM_LR, betas=(T.ADAM_B1, T.ADAM_B2), eps=T.ADAM_EPS, weight_decay=wd)
    m, v = torch.zeros(64, dtype=F64), torch.zeros(64, dtype=F64)
    for step in (1, 2, 3, 4):
        grad = torch.randn(64, generator=g, dtype=F64)
        ref_p.grad = grad.clone()
        opt.step()
        bc1, bc2 = 1 - T.ADAM_B1 ** step, 1 - T.ADAM_B2 ** step
        h = dict(decay=1 - T.ADAM_LR * wd, coef=1.0, omb1=1 - T.ADAM_B1, omb2=1 - T.ADAM_B2, bc2s=math.sqrt(bc2), step_size=T.ADAM_LR / bc1)
        p, m, v, _ = T.adam_step_exact(p, m, v, grad, h)
        _close(p, ref_p.detach(), f"step {step}")


@pytest.mark.parametrize("k", range(len(T.EMBED_BWD_CASES)), ids=lambda k: T.EMBED_BWD_CASES[k].name)
def test_embed_bwd_reference_is_index_add(k):
    i, ref = _case("embed_bwd_sorted", k)
    n_rows = T.EB_TEXT + T.EB_AUDIO
    live = i["rows"] < n_rows
    tab = torch.cat([i["g_text"], i["g_audio"]]).double()
    tab.index_add_(0, i["rows"][live], torch.cat([i["dh"], i["dseq"]]).double()[i["src"][live]])
    _close(torch.cat([ref["g_text"][0], ref["g_audio"][0]]), tab, "gradient tables")
    touched = torch.zeros(n_rows, dtype=torch.bool)
    touched[i["rows"][live]] = True
    slack = torch.cat([ref["g_text"][1], ref["g_audio"][1]])
    assert bool((slack[~touched] < 0).all()) and bool((slack[touched] >= 0).all())            # untouched rows are judged bit for bit


@pytest.mark.parametrize("k", range(len(T.EMBED_CASES)), ids=lambda k: str(T.EMBED_CASES[k]))
def test_embed_fwd_reference_is_masked_embedding_sum(k):
    c = T.EMBED_CASES[k]
    i, ref = _case("embed_fwd", k)
    tab = torch.cat([i["audio"], i["text"]]).double()
    off = torch.cat([torch.arange(c.K) * T.VA, torch.tensor([c.K * T.VA])])
    _close(ref["out"][0], (F.embedding(i["tokens"] + off, tab) * i["mask"][..., None].double()).sum(1), "out")
    assert float(ref["out"][0][0].abs().max()) == 0.0                                       # the row with no live slot


def test_sums_references_are_torch_sums():
    for op, k in (("colsum", 9), ("colsum", len(T.COLSUM_CASES) - 1), ("colsum_rows", 20), ("sumsq", 4), ("reduce_sum", 2)):
        i, ref = _case(op, k)
        if op == "colsum":
            for j, (p, d) in enumerate(zip(i["partials"], i["dst"])):
                _close(ref[f"dst{j}"][0], p.double().sum(0) + d.double() * int(i["c"].acc), op)
        elif op == "colsum_rows":
            c = i["c"]
            for sl in range(c.S):
                rows = [r for r in range(c.M) if (r // 4) % c.S == sl]
                _close(ref["partials"][0][sl], i["x"].double()[rows, :c.D].sum(0), op)
        elif op == "sumsq":
            assert abs(float(ref["partials"][0].sum()) - float((i["g"].double() ** 2).sum())) <= 1e-12 * float((i["g"].double() ** 2).sum())
        else:
            _close(ref["out"][0], (i["x"].double().sum() * T.REDUCE_SCALE).reshape(1), op)


# ------------------------------------------------------------------------------------------------------- dropout restatement
def test_dropout_restatement_keeps_the_right_fraction_and_is_layout_free():
    for p in (0.0, 0.1, 0.5, 0.9):
        M, D = 512, 520
        thresh, scale = T.dropout_thresh_scale(p)
        keep = T.dropout_keep(0x5eed, M, D, p)
        q = 1 - thresh / 65536
        sd = math.sqrt(q * (1 - q) / (M * D))
        assert abs(float(keep.double().mean()) - q) <= 5 * sd + 1e-15, (p, float(keep.double().mean()), q, sd)
        assert float(scale) == float(np.float32(1) / np.float32(q))
        assert torch.equal(T.dropout_keep(0x5eed, 7, D, p), keep[:7])                       # a row slice is the first rows
        assert p == 0.0 or not torch.equal(T.dropout_keep(0x5eee, M, D, p), keep)
    c = T.DropCase(5, 72, 80, 88, 0.0, 1, False)
    i = T.drop_inputs(c)
    assert torch.equal(T.drop_f32(i)["out"][:, :72], i["x"][:, :72])                         # p = 0 is the identity


# ------------------------------------------------------------------------------------------------------- fp32 restatements pass
@pytest.mark.parametrize("op", sorted(T.OPS))
def test_fp32_restatement_is_inside_every_bound(op):
    o = T.OPS[op]
    worst = 0.0
    for k in range(len(o.cases)):
        inp, ref = _case(op, k)
        got = o.f32(inp)
        worst = max(worst, max(T.judge(f"{op}.{key}", got[key], val, slack) for key, (val, slack) in ref.items()))
    print(f"UTIL {op} {worst:.4f} over {len(o.cases)} cases; measured function errors (ulp) {dict(T.measured)}")
    assert worst <= 1.0


@pytest.mark.parametrize("op,mut", [(op, m) for op in sorted(T.OPS) for m in T.OPS[op].mutants])
def test_mutant_is_rejected(op, mut):
    o = T.OPS[op]
    for k in range(len(o.cases)):
        inp, ref = _case(op, k)
        got = o.f32(inp, mut)
        try:
            for key, (val, slack) in ref.items():
                T.judge(f"{op}.{key}", got[key], val, slack)
        except AssertionError:
            return
    raise AssertionError(f"{op}: the mutant {mut} passes every case: a bound or the case list is too weak")


def _adam_run(c, mut=None):
    """The fp32 restatement over ADAM_STEPS, each step judged from the restatement's own previous state.  -> worst ratio."""
    i = T.adam_inputs(c)
    state = {k: i[k].clone() for k in ("master", "m", "v")}
    worst = 0.0
    for step, g in zip(T.ADAM_STEPS, i["grads"]):
        ref = T.adam_ref(state, g, c, step)
        new = T.adam_f32(state, g, c, step, mut)
        worst = max(worst, max(T.judge(f"adamw.{k}", new[k], *ref[k]) for k in ref))
        state = new
    return worst


def test_adamw_restatement_is_inside_every_bound_and_mutants_are_not():
    worst = max(_adam_run(c) for c in T.ADAM_CASES)
    print(f"UTIL adamw {worst:.4f} over {len(T.ADAM_CASES)} cases x {len(T.ADAM_STEPS)} steps; measured function errors (ulp) {dict(T.measured)}")
    assert worst <= 1.0
    for mut in T.ADAM_MUTANTS:
        rejected = 0
        for c in T.ADAM_CASES:
            try:
                _adam_run(c, mut)
            except AssertionError:
                rejected += 1
        assert rejected, f"adamw: the mutant {mut} passes every case"


def test_split_master_round_trips():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    x[:4] = torch.tensor([1.00390625, -1.00390625, 0.0, 1.0])               # exact ties of the bf16 rounding, both signs
    param, lo = T.split_master(x)
    assert torch.equal(T.join_master(param, lo).view(torch.int32), x.view(torch.int32))
    assert float(param[0]) == 1.0078125 and float(param[1]) == -1.0078125    # half up in magnitude, where to-nearest-even gives 1.0
    assert bool(((param.double() - x.double()).abs() <= T.hulp(x.double()) * 1.0000001).all())


def test_judge_counts_every_element_and_reports_the_worst():
    ref = torch.tensor([1.0, 2.0, 0.0], dtype=F64)
    slack = torch.tensor([1e-3, 1e-3, -1.0], dtype=F64)
    assert T.judge("t", torch.tensor([1.0005, 2.0, 0.0], dtype=F64), ref, slack) == pytest.approx(0.5)
    with pytest.raises(AssertionError, match=r"worst element \(2,\)"):
        T.judge("t", torch.tensor([1.0, 2.0, 1e-30]), ref, slack)         # a negative slack demands the exact value
    with pytest.raises(AssertionError, match="worst element"):
        T.judge("t", torch.tensor([1.0, float("nan"), 0.0]), ref, slack)
    with pytest.raises(AssertionError, match="elements for"):
        T.judge("t", torch.tensor([1.0, 2.0]), ref, slack)
    with pytest.raises(AssertionError, match="differ"):
        T.judge("t", torch.tensor([1.0, 2.0]).bfloat16(), torch.tensor([1.0, 2.5]).bfloat16(), None)
    bits = torch.tensor([1, -2, 3], dtype=torch.int32)                    # raw bits (the split-master checks) count per element
    assert T.judge("t", bits.clone(), bits, None) == 0.0 and T.judge("t", bits.to(torch.int16), bits.to(torch.int16), None) == 0.0
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        T.judge("t", torch.tensor([1, -2, 4], dtype=torch.int32), bits, None)
    # a bf16 result is allowed half a bf16 ulp of the reference on top of the slack, and no more
    assert T.judge("t", torch.tensor([1.0]).bfloat16(), torch.tensor([1.0 + 2.0 ** -8], dtype=F64), torch.zeros(1, dtype=F64)) <= 1.0
    with pytest.raises(AssertionError):
        T.judge("t", torch.tensor([1.0]).bfloat16(), torch.tensor([1.0 + 2.0 ** -7], dtype=F64), torch.zeros(1, dtype=F64))
