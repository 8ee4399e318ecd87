"""Proves tests/codec_ref.py - the float64 reference that test_codec_kernels_gpu.py judges the Mimi codec kernels by - against
torch's own float64 kernels, at every case the GPU file runs (the grid-stride lengths on a 4096-column slice), and proves the
premise of the one-hot attention cases.  Tolerance: 1e-12 of each case's largest magnitude (float64 against float64, different
summation orders).  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import codec_ref as R

TOL = 1e-12


def _close(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max())
    assert err <= TOL * scale, f"{what}: {err:.3e} vs {TOL * scale:.3e}"


def _torch_conv(c, x, w, b, res):
    x64 = x.double()[None]
    if c.elu:
        x64 = F.elu(x64)                                                        # ELU(0) = 0 and ELU commutes with replication
    need = (c.T_out - 1) * c.stride + (c.k - 1) * c.dil + 1 - c.pad_left        # input columns the last output reaches
    right = max(need - c.T_in, 0)
    xp = F.pad(x64, (c.pad_left, right), mode="replicate" if c.pad_mode == 1 else "constant")
    y = F.conv1d(xp, w.double(), None if b is None else b.double(), stride=c.stride, dilation=c.dil, groups=c.groups)[0][:, :c.T_out]
    return y if res is None else y + res.double()


@pytest.mark.parametrize("c", R.conv_cases(), ids=lambda c: c.name)
def test_conv1d(c):
    inp = R.conv_inputs(c)
    ref = R.conv_ref(c, inp)
    assert ref.out.shape == (c.C_out, c.T_out)
    _close(ref.out, _torch_conv(c, *inp), c.name)
    assert bool((R.conv_bound(ref) >= 0).all())
    if c.neg:
        assert float(inp[0].max()) < 0


def test_conv1d_loop_slice():
    c = R.CONV_LOOP
    x, w, b, _ = R.conv_inputs(c)
    t = torch.arange(c.T_out - 4096, c.T_out)
    ref = R.conv_ref(c, (x, w, b, None), t_idx=t)
    xs = x[:, c.T_out - 4096 - c.pad_left:].double()[None]                      # causal: output t reads x[t - 2 .. t]
    _close(ref.out, F.conv1d(xs, w.double(), b.double())[0], "loop")
    cols = R.loop_columns(c.T_out)
    assert cols.min() >= 0 and cols.max() == c.T_out - 1 and c.T_out > R.LOOP


def _torch_convt(c, x, w, b):
    x64 = F.elu(x.double()) if c.elu else x.double()
    y = F.conv_transpose1d(x64[None], w.double(), None if b is None else b.double(), stride=c.stride, groups=c.groups)[0]
    return y[:, c.crop:c.crop + c.T_out]


@pytest.mark.parametrize("c", R.convt_cases(), ids=lambda c: c.name)
def test_conv_transpose1d(c):
    inp = R.convt_inputs(c)
    ref = R.convt_ref(c, inp)
    assert c.crop + c.T_out <= (c.T_in - 1) * c.stride + c.k or c.k < c.stride
    want = _torch_convt(c, *inp)
    if want.shape[1] < c.T_out:                                                 # k < stride: torch's full output ends before T_in * stride
        want = F.pad(want, (0, c.T_out - want.shape[1]))
        if inp[2] is not None:
            want[:, -(c.T_out - _torch_convt(c, *inp).shape[1]):] = inp[2].double()[:, None]
    _close(ref.out, want, c.name)
    if c.k < c.stride:
        assert not bool(ref.reached.all()) and bool(ref.reached.any())


def test_conv_transpose1d_loop_slice():
    c = R.CONVT_LOOP
    x, w, b = R.convt_inputs(c)
    t = torch.arange(c.T_out - 4096, c.T_out)
    ref = R.convt_ref(c, (x, w, b), t_idx=t)
    n_in = 4096 // c.stride + 1                                                 # one extra input column on the left: k = 2 stride
    y = F.conv_transpose1d(x[:, -n_in:].double()[None], w.double(), b.double(), stride=c.stride)[0]
    _close(ref.out, y[:, c.stride:c.stride + 4096], "loop")
    assert c.T_out > R.LOOP and c.T_out == c.T_in * c.stride


@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layernorm(case):
    x, w, b = R.ln_inputs(case)
    ref = R.layernorm(x, w, b, R.LN_EPS)
    _close(ref.out, F.layer_norm(x.double(), (x.shape[1],), w.double(), b.double(), R.LN_EPS), str(case))
    bound = R.layernorm_bound(ref)
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
    if case[2] == "const":
        assert float(ref.var[case[0] // 2]) == 0.0
        _close(ref.out[case[0] // 2], b.double(), "constant row")
    if case[2] == "offset":
        assert abs(float(ref.mean[1]) - 1e3) < 1 and 0.5 < float(ref.var[1]) < 2


@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("shape", R.LIN_TILED + R.LIN_ROWS, ids=str)
def test_linear(shape, epi):
    T, N, K, pad = shape
    x, W, scale, res, act = R.linear_inputs(T, N, K, pad, epi)
    assert x.shape[1] == K + pad and (pad == 0 or bool(torch.isnan(x[:, K:]).all()))
    ref = R.linear(x, W, scale, res, act, K)
    v = x[:, :K].double() @ W.double().t()
    if act:
        v = F.gelu(v, approximate="none")
    if scale is not None:
        v = res.double() + scale.double() * v
    elif res is not None:
        v = v + res.double()
    _close(ref.out, v, f"{shape} {epi}")
    assert bool(torch.isfinite(R.linear_bound(ref)).all())
    if epi == "gelu" and T == 16 and N >= 255:
        assert float(ref.pre.min()) <= -6 and float(ref.pre.max()) >= 6, (float(ref.pre.min()), float(ref.pre.max()))


def _hf_rope(qkv, H, hd, base, pos0):
    from transformers.models.mimi.modeling_mimi import apply_rotary_pos_emb
    T = qkv.shape[0]
    x = qkv.double().reshape(T, 3, H, hd)
    q, k = x[:, 0].permute(1, 0, 2)[None], x[:, 1].permute(1, 0, 2)[None]        # [1, H, T, hd]
    inv_freq = 1.0 / (torch.tensor(base, dtype=torch.float64) ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    freqs = (pos0 + torch.arange(T, dtype=torch.float64))[:, None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)[None]
    qe, ke = apply_rotary_pos_emb(q, k, emb.cos(), emb.sin())
    out = x.clone()
    out[:, 0], out[:, 1] = qe[0].permute(1, 0, 2), ke[0].permute(1, 0, 2)
    return out.reshape(T, 3 * H * hd)


@pytest.mark.parametrize("pos0", R.ROPE_POS)
@pytest.mark.parametrize("geom", R.ROPE_GEOMS, ids=str)
def test_rope_half(geom, pos0):
    H, hd = geom
    qkv = R.rope_inputs(5, H, hd, pos0)
    ref = R.rope_half(qkv, H, hd, R.ROPE_BASE, pos0)
    _close(ref.out, _hf_rope(qkv, H, hd, R.ROPE_BASE, pos0), f"{geom} {pos0}")
    assert torch.equal(ref.out[:, 2 * H * hd:], qkv.double()[:, 2 * H * hd:])
    bound = R.rope_bound(ref)
    assert bool((bound[:, 2 * H * hd:] == 0).all()) and bool((bound[:, :2 * H * hd] > 0).all())


def test_rope_half_loop_size():
    T, H, hd, pos0 = R.ROPE_LOOP
    assert T * 2 * H * (hd // 2) > R.LOOP
    qkv = R.rope_inputs(T, H, hd, pos0)[-64:]                                   # the last rows only
    ref = R.rope_half(qkv, H, hd, R.ROPE_BASE, pos0 + T - 64)
    _close(ref.out, _hf_rope(qkv, H, hd, R.ROPE_BASE, pos0 + T - 64), "loop")


def _torch_attn(qkv, H, hd, window):
    T = qkv.shape[0]
    x = qkv.double().reshape(T, 3, H, hd)
    q, k, v = (x[:, i].permute(1, 0, 2) for i in range(3))
    i = torch.arange(T)
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64)
    mask[(i[None, :] <= i[:, None]) & (i[:, None] - i[None, :] < window)] = 0.0
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd) + mask, dim=-1)
    return (p @ v).permute(1, 0, 2).reshape(T, H * hd), p


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attn_window_random(case):
    H, window = case
    qkv = R.attn_random(H, window)
    ref = R.attn_window(qkv, H, R.ATTN_HD, window)
    out, p = _torch_attn(qkv, H, R.ATTN_HD, window)
    _close(ref.out, out, str(case))
    _close(ref.probs, p, str(case))
    n = (ref.probs > 0).sum(-1)                                                 # keys each query sees: 1, .., window
    assert int(n.max()) == window and int(n[0, 0]) == 1 and int(n[0, -1]) == window
    if window == 250:
        assert {64, 65}.issubset(set(n[0].tolist()))
    assert bool(torch.isfinite(R.attn_bound(ref)).all())


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attn_onehot_premise(case):
    """Every one-hot case of the GPU file: the aligned key leads every other key of its window by >= 40 in the float64 reference
    (inside cases), and lies outside the window - zero probability - in the outside cases."""
    H, window = case
    for q in R.onehot_queries(window):
        qkv, pos = R.onehot_case(H, window, q)
        assert pos == max(q - window + 1, 0)
        ref = R.attn_window(qkv, H, R.ATTN_HD, window)
        if window > 1:
            assert R.onehot_lead(ref, q, pos) >= R.ONEHOT_GAP, (case, q, R.onehot_lead(ref, q, pos))
        v = qkv.reshape(-1, 3, H, R.ATTN_HD)[pos, 2].reshape(-1)
        assert float(v.min()) >= 1.0 and float(v.max()) < 2.0
        assert float((ref.out[q] - v.double()).abs().max()) < 2.0 ** -25         # the float64 result rounds to the value row
        out, _ = _torch_attn(qkv, H, R.ATTN_HD, window)
        _close(ref.out, out, f"{case} {q}")
        qkv_o, pos_o = R.onehot_case(H, window, q, outside=True)
        if qkv_o is None:
            assert q - window < 0
            continue
        assert pos_o == q - window
        ref_o = R.attn_window(qkv_o, H, R.ATTN_HD, window)
        assert float(ref_o.probs[:, q, pos_o].max()) == 0.0
        raw = (qkv_o.double().reshape(-1, 3, H, R.ATTN_HD)[q, 0] * qkv_o.double().reshape(-1, 3, H, R.ATTN_HD)[pos_o, 1]).sum(-1) / 8
        assert float((raw - ref_o.scores[:, q].amax(-1)).min()) >= R.ONEHOT_GAP  # it WOULD win if it were admitted


def test_transpose():
    for Rr in R.TRANSPOSE_SIZES:
        for Cn in R.TRANSPOSE_SIZES:
            x = torch.randn(3, Rr, Cn, generator=torch.Generator().manual_seed(Rr * 100 + Cn))
            assert torch.equal(R.transpose(x), x.transpose(1, 2).contiguous())
            assert torch.equal(R.transpose(x[0]), x[0].t().contiguous())


def test_allowances_are_measured():
    """Every elementary-function allowance is 4 x a measured worst ulp error of at least 0.5 and - torch's float32 functions being
    good to a few ulp - stays small; a figure beyond 16 ulp would mean the measurement itself is off."""
    x = torch.linspace(-6, 6, 4097)
    for name, arg in (("expm1f", x[x <= 0]), ("erff", x), ("expf", -x.abs() * 17), ("rsqrtf", x.abs() + 1e-5), ("sincosf", x.abs() * 700)):
        a = R.allowance(name, arg)
        assert 2.0 <= a <= 16.0, (name, a)
    a = R.allowance("powf", torch.full((32,), 10000.0), -torch.arange(32) / 32.0)
    assert 2.0 <= a <= 16.0, a
