"""A float64 reference of the fp32 Mimi codec kernels of csrc/codec.hip, a rounding-error bound for each, and the seeded cases
the codec-kernel tests run (test_codec_ref_cpu.py proves this module against torch's own float64 kernels;
test_codec_kernels_gpu.py judges the kernels by it).

Everything here is plain torch on the CPU, in float64, written from the index formula in the comment above each kernel.  The
inputs are float32 tensors cast to float64, so every reference is the exact operation on the kernel's own operands.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  A serial chain of L fp32 multiply-adds (fused or not) over terms t_i errs by
at most gamma_L sum|t_i| <= (L + 2) u sum|t_i| for the L used here (L u << 1); bias and residual count among the terms.  A
device elementary function is allowed ``A`` ulp of its value, A * 2u |value| at most: see ``allowance``."""
import math
from collections import namedtuple

import torch

from test_stream_gpu import CONV_CASES, CONVT_CASES

U = 2.0 ** -24
F64 = torch.float64
LOOP = 4096 * 256                                      # outputs one pass of a grid-stride loop covers (4096 blocks x 256)


# ------------------------------------------------------------------------------------------------- elementary functions
# No copy of the HIP math API accuracy table ships with the ROCm install this was written on (searched share/, docs and
# headers for the function names next to "ulp"), so no figure is quoted from memory.  Instead every allowance is measured:
# torch's float32 CPU evaluation of the same function against float64 on the very inputs of the case, worst error in ulp of
# the value, times 4.  The factor 4 is a margin over that reference implementation and is not fitted to the kernels.  The
# worst error is never taken below 0.5 ulp - the error of a correctly rounded float32 result - so a case whose few inputs
# happen to evaluate exactly (rsqrt(64)) does not demand more than correct rounding could give: every allowance is >= 2 ulp.
ALLOWANCE_SOURCE = "4 x worst ulp error of torch float32 CPU vs float64 on the case's own inputs (>= 4 x 0.5 ulp)"
_F32 = {"expm1f": torch.expm1, "erff": torch.erf, "expf": torch.exp, "rsqrtf": torch.rsqrt, "sinf": torch.sin, "cosf": torch.cos,
        "sqrtf": torch.sqrt, "logf": torch.log}         # the last two serve train_ops_ref.py
measured = {}                                          # name -> worst ulp error seen so far (for the records)


def _ulp(v64):
    """ulp of the float32 nearest to |v| (normal range)."""
    return torch.exp2(torch.floor(torch.log2(v64.abs().clamp(min=2.0 ** -126))) - 23)


def allowance(name, x32, y32=None):
    """Allowed error of the device function ``name`` (expm1f, erff, expf, rsqrtf, sincosf, powf) in ulp of its value."""
    x32 = x32.detach().float().reshape(-1)
    if x32.numel() == 0:
        return 2.0
    if name == "powf":
        got, ref = torch.pow(x32, y32.float().reshape(-1)), torch.pow(x32.double(), y32.float().reshape(-1).double())
        worst = float(((got.double() - ref).abs() / _ulp(ref)).max())
    elif name == "sincosf":
        worst = max(float(((_F32[f](x32).double() - _F32[f](x32.double())).abs() / _ulp(_F32[f](x32.double()))).max()) for f in ("sinf", "cosf"))
    else:
        ref = _F32[name](x32.double())
        worst = float(((_F32[name](x32).double() - ref).abs() / _ulp(ref)).max())
    worst = max(worst, 0.5)
    measured[name] = max(measured.get(name, 0.0), worst)
    return 4.0 * worst


def elu(x64):
    return torch.where(x64 > 0, x64, torch.expm1(x64))


# ------------------------------------------------------------------------------------------------------------- conv1d
ConvRef = namedtuple("ConvRef", "out sabs L elu_x reached")


def conv1d(x, w, bias=None, res=None, *, T_out, stride=1, dilation=1, pad_left=0, pad_mode=0, groups=1, elu_in=False, t_idx=None):
    """y[co][t] = bias[co] + sum_{ci in group} sum_j w[co][ci][j] act(xpad[ci][t stride + j dil - pad_left]) (+ res[co][t]);
    xpad outside [0, T_in) is 0 (pad_mode 0) or the edge column (pad_mode 1).  x [C_in, T_in], w [C_out, C_in/groups, k],
    res [C_out, T_out].  ``t_idx``: only these output columns (res is indexed by them)."""
    x64, w64 = x.double(), w.double()
    C_in, T_in = x.shape
    C_out, cin_g, k = w.shape
    cout_g = C_out // groups
    assert cin_g * groups == C_in and cout_g * groups == C_out
    t = torch.arange(T_out) if t_idx is None else torch.as_tensor(t_idx).long()
    y = torch.zeros(C_out, t.numel(), dtype=F64)
    sabs = torch.zeros_like(y)
    for j in range(k):
        p = t * stride + j * dilation - pad_left
        inside = (p >= 0) & (p < T_in)
        col = x64[:, p.clamp(0, T_in - 1)]                          # the edge column where p is outside
        if pad_mode == 0:
            col = col * inside
        if elu_in:
            col = elu(col)
        for g in range(groups):
            wg = w64[g * cout_g:(g + 1) * cout_g, :, j]             # [cout_g, cin_g]
            xg = col[g * cin_g:(g + 1) * cin_g]
            y[g * cout_g:(g + 1) * cout_g] += wg @ xg
            sabs[g * cout_g:(g + 1) * cout_g] += wg.abs() @ xg.abs()
    reached = sabs > 0
    L = cin_g * k
    if bias is not None:
        y += bias.double()[:, None]
        sabs += bias.double().abs()[:, None]
    if res is not None:
        r = res.double()[:, t]
        y += r
        sabs += r.abs()
        L += 1
    return ConvRef(y, sabs, L, x if elu_in else None, reached)


def conv_bound(ref):
    """|got - ref| <= (L + 2) u S + A_expm1 2u S.  S = |bias| + sum |w| |act(x)| + |res|, L = cin_g k multiply-adds (+ 1 for
    the residual): the chain bound of the module docstring.  With the fused ELU every tap with x < 0 carries the relative
    error A_expm1 2u of expm1f, so the taps' part of S (bounded by S) is charged that much more."""
    b = (ref.L + 2) * U * ref.sabs
    if ref.elu_x is not None:
        b = b + allowance("expm1f", ref.elu_x[ref.elu_x <= 0]) * 2 * U * ref.sabs
    return b


def conv_transpose1d(x, w, bias=None, *, T_out, stride, crop_left=0, groups=1, elu_in=False, t_idx=None):
    """y[co][t] = bias[co] + sum_ci sum_{j : (t + crop_left - j) % stride == 0} act(x[ci][(t + crop_left - j) / stride]) w[ci][co_g][j]
    over the taps whose input column lies in [0, T_in).  w in the torch layout [C_in, C_out/groups, k]."""
    x64, w64 = x.double(), w.double()
    C_in, T_in = x.shape
    _, cout_g, k = w.shape
    cin_g, C_out = C_in // groups, cout_g * groups
    t = torch.arange(T_out) if t_idx is None else torch.as_tensor(t_idx).long()
    y = torch.zeros(C_out, t.numel(), dtype=F64)
    sabs = torch.zeros_like(y)
    for j in range(k):
        num = t + crop_left - j
        ti = torch.div(num, stride, rounding_mode="floor")
        valid = (num >= 0) & (num - ti * stride == 0) & (ti < T_in)
        col = x64[:, ti.clamp(0, T_in - 1)]
        if elu_in:
            col = elu(col)
        col = col * valid
        for g in range(groups):
            wg = w64[g * cin_g:(g + 1) * cin_g, :, j]               # [cin_g, cout_g]
            xg = col[g * cin_g:(g + 1) * cin_g]
            y[g * cout_g:(g + 1) * cout_g] += wg.t() @ xg
            sabs[g * cout_g:(g + 1) * cout_g] += wg.abs().t() @ xg.abs()
    reached = sabs > 0
    if bias is not None:
        y += bias.double()[:, None]
        sabs += bias.double().abs()[:, None]
    return ConvRef(y, sabs, cin_g * ((k + stride - 1) // stride), x if elu_in else None, reached)


convt_bound = conv_bound        # the same chain: L = cin_g ceil(k / stride) multiply-adds, at most that many taps reach one output


# ------------------------------------------------------------------------------------------------------------- layernorm
LnRef = namedtuple("LnRef", "out x w b mean var eps")


def layernorm(x, w, b, eps):
    """y[t][c] = (x[t][c] - mean_t) / sqrt(var_t + eps) w[c] + b[c], var the mean of squared deviations."""
    x64 = x.double()
    D = x.shape[1]
    mean = x64.sum(1, keepdim=True) / D
    d = x64 - mean
    var = (d * d).sum(1, keepdim=True) / D
    return LnRef(d / torch.sqrt(var + eps) * w.double() + b.double(), x64, w.double(), b.double(), mean, var, float(eps))


def layernorm_bound(ref):
    """The kernel sums a row on 64 lanes (ceil(D/64) serial adds each) and a 6-step butterfly: a chain of Ls = ceil(D/64) + 6.
    mean:  dm <= (Ls + 1) u sum|x| / D   (the chain and the division).
    var:   the exact mean square deviation about a mean off by dm is var + dm^2; each deviation is rounded (its square: 2u),
           the square is rounded (u), the chain (Ls u) and the division (u):  dvar <= dm^2 + (Ls + 4) u (var + dm^2).
    r = rsqrtf(var + eps):  dr / r <= dvar / (2 (var + eps)) + u (the add) + A_rsqrt 2u.
    y = (x - mean) r w + b with d = x - mean:  the deviation is off by dm + u |d|, two products and one add round (u each):
           |dy| <= |w| r dm + |d| r |w| (dr / r + 4u) + u (|d r w| + |b|)."""
    D = ref.x.shape[1]
    Ls = (D + 63) // 64 + 6
    dm = (Ls + 1) * U * ref.x.abs().sum(1, keepdim=True) / D
    dvar = dm * dm + (Ls + 4) * U * (ref.var + dm * dm)
    r = 1.0 / torch.sqrt(ref.var + ref.eps)
    a = allowance("rsqrtf", (ref.var + ref.eps).float())
    dr_rel = dvar / (2 * (ref.var + ref.eps)) + U + a * 2 * U
    term = (ref.x - ref.mean).abs() * r * ref.w.abs()
    return ref.w.abs() * r * dm + term * (dr_rel + 4 * U) + U * (term + ref.b.abs())


# ------------------------------------------------------------------------------------------------------------- linear
LinRef = namedtuple("LinRef", "out pre sabs K act scale res")


def linear(x, W, scale=None, res=None, act=0, K=None):
    """y[t][n] = epilogue(sum_{k < K} x[t][k] W[n][k]); x [T, ldx >= K] (columns >= K are not read).  Epilogue: act 1 = exact
    GELU g(v) = v (1 + erf(v / sqrt 2)) / 2; scale -> res + scale[n] g; else g (+ res)."""
    N, Kw = W.shape
    K = Kw if K is None else K
    assert Kw == K and x.shape[1] >= K
    x64, W64 = x.double()[:, :K], W.double()
    pre = x64 @ W64.t()
    sabs = x64.abs() @ W64.abs().t()
    v = pre
    if act == 1:
        v = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if scale is not None:
        v = res.double() + scale.double()[None, :] * v
    elif res is not None:
        v = v + res.double()
    return LinRef(v, pre, sabs, K, act, None if scale is None else scale.double(), None if res is None else res.double())


def linear_bound(ref):
    """Product: dv <= (K + 2) u sum_k |x||W| (a chain of K multiply-adds from 0).
    GELU g = 0.5 v (1 + erf(z)), z = v c with c = fl(1/sqrt 2): z carries 2u |z| (the constant and the product), erff its
    allowance A_erf 2u |erf z|, the add u |1 + erf z|, the two products 2u |g|; the error of v itself passes through
    |g'(v)| = |(1 + erf z)/2 + v exp(-z^2)/sqrt(2 pi)|:
        dg <= |g'| dv + |v|/2 (2/sqrt(pi) exp(-z^2) 2u |z| + A_erf 2u |erf z| + u |1 + erf z|) + 2u |g|.
    For v << 0 the sum 1 + erf z cancels and the A_erf term dominates: that is the kernel's formula, not slack.
    Layer scale / residual: res + scale g has one product and one add: |scale| dg + 2u (|scale g| + |res|); a plain residual one add."""
    v = ref.pre
    dv = (ref.K + 2) * U * ref.sabs
    g = v
    if ref.act == 1:
        z = v / math.sqrt(2.0)
        erfz = torch.erf(z)
        g = 0.5 * v * (1.0 + erfz)
        gp = (0.5 * (1.0 + erfz) + v * torch.exp(-z * z) / math.sqrt(2 * math.pi)).abs()
        a = allowance("erff", z.float())
        inner = 2 / math.sqrt(math.pi) * torch.exp(-z * z) * 2 * U * z.abs() + a * 2 * U * erfz.abs() + U * (1.0 + erfz).abs()
        dv = gp * dv + 0.5 * v.abs() * inner + 2 * U * g.abs()
    if ref.scale is not None:
        s = ref.scale.abs()[None, :]
        return s * dv + 2 * U * (s * g.abs() + ref.res.abs())
    if ref.res is not None:
        return dv + U * (g.abs() + ref.res.abs()) + U * ref.out.abs()
    return dv


# ------------------------------------------------------------------------------------------------------------- rope
RopeRef = namedtuple("RopeRef", "out qkv angle pos H hd base")


def rope_half(qkv, H, hd, base, pos0):
    """Rotate-half RoPE on the q and k thirds of qkv [T, 3 H hd]: for i < hd/2, theta_i = base^(-2i/hd), a = (pos0 + t) theta_i,
    (x[i], x[i + hd/2]) -> (x[i] cos a - x[i + hd/2] sin a, x[i + hd/2] cos a + x[i] sin a); the v third is untouched."""
    T = qkv.shape[0]
    half = hd // 2
    x = qkv.double().reshape(T, 3 * H, hd).clone()
    theta = torch.tensor([float(base) ** (-2.0 * i / hd) for i in range(half)], dtype=F64)
    angle = (pos0 + torch.arange(T, dtype=F64))[:, None] * theta[None, :]               # [T, half]
    cs, sn = torch.cos(angle)[:, None, :], torch.sin(angle)[:, None, :]
    a, b = x[:, :2 * H, :half].clone(), x[:, :2 * H, half:].clone()
    x[:, :2 * H, :half] = a * cs - b * sn
    x[:, :2 * H, half:] = b * cs + a * sn
    return RopeRef(x.reshape(T, 3 * H * hd), qkv.double().reshape(T, 3 * H, hd), angle, pos0 + torch.arange(T, dtype=F64), H, hd, float(base))


def rope_bound(ref):
    """The fp32 angle: theta = powf(base, e) with e = -2i/hd rounded (u |e| ln(base) relative on theta) and A_pow 2u from powf,
    the position times theta rounds once more: da <= a (2 A_pow + 1 + ln(base) 2i/hd) u = (pos0 + t) theta c u.
    cos and sin then err by da + A_sincos 2u (|value| <= 1), and each output is a chain of L = 2 products:
    |dy| <= (|a| + |b|) (da + A_sincos 2u) + (L + 2) u (|a| + |b|).  Zero on the v third (untouched bit for bit)."""
    H, hd = ref.H, ref.hd
    half = hd // 2
    i = torch.arange(half, dtype=F64)
    e32 = (-2.0 * i / hd).float()
    a_pow = allowance("powf", torch.full((half,), ref.base), e32)
    theta32 = torch.pow(torch.full((half,), ref.base, dtype=F64), e32.double()).float()
    a_sc = allowance("sincosf", ref.pos.float()[:, None] * theta32[None, :])                  # the kernel's own fp32 angles
    da = ref.angle * ((2 * a_pow + 1 + math.log(ref.base) * 2 * i / hd) * U)[None, :]
    mag = ref.qkv[:, :2 * H, :half].abs() + ref.qkv[:, :2 * H, half:].abs()            # [T, 2H, half]
    b = mag * ((da + a_sc * 2 * U)[:, None, :] + 4 * U)
    out = torch.zeros_like(ref.qkv)
    out[:, :2 * H, :half] = b
    out[:, :2 * H, half:] = b
    return out.reshape(ref.out.shape)


# ------------------------------------------------------------------------------------------------------------- attention
AttnRef = namedtuple("AttnRef", "out absv probs scores sabs window hd")


def attn_window(qkv, H, hd, window):
    """Causal sliding-window attention on qkv [T, 3 H hd] (q | k | v, head-major): query t sees keys in (t - window, t], scores
    q.k / sqrt(hd).  -> out [T, H hd], absv = sum_s p_s |v_s|, probs / scores [H, T, T] (0 / -inf outside the window),
    sabs = sum_c |q_c| |k_c| per (head, query, key)."""
    T = qkv.shape[0]
    x = qkv.double().reshape(T, 3, H, hd)
    q, k, v = (x[:, i].permute(1, 0, 2) for i in range(3))                              # [H, T, hd]
    ti, si = torch.arange(T)[:, None], torch.arange(T)[None, :]
    band = (si <= ti) & (si > ti - window)
    scores = (q @ k.transpose(1, 2) / math.sqrt(hd)).masked_fill(~band, float("-inf"))
    sabs = (q.abs() @ k.abs().transpose(1, 2)) * band
    m = scores.amax(-1, keepdim=True)
    e = torch.exp(scores - m)
    probs = e / e.sum(-1, keepdim=True)
    out = (probs @ v).permute(1, 0, 2).reshape(T, H * hd)
    absv = (probs @ v.abs()).permute(1, 0, 2).reshape(T, H * hd)
    return AttnRef(out, absv, probs, scores, sabs, window, hd)


def attn_bound(ref):
    """Scores: a chain of hd multiply-adds, then the product with rsqrtf(hd):
        ds <= (hd + 2) u sum_c |q_c||k_c| / sqrt(hd) + |s| (1 + 2 A_rsqrt) u;  Ds = the largest ds of the query's window.
    Softmax: the exponent s - max carries 2 Ds and its own rounding u |s - max|, expf A_exp 2u: every numerator is off by the
    factor E = 2 Ds + u max|s - max| + A_exp 2u at most (first order; |s - max| is capped at 104, beyond which exp is 0 in
    fp32 and float64 alike to the bound's resolution), the denominator (a sum of positive terms on 64 lanes and a butterfly,
    Ln = ceil(n/64) + 6 adds) by E + (Ln + 1) u; a probability therefore by p (2E + (Ln + 1) u).
    Output: sum_s p_s v_s is a chain of n <= window multiply-adds and one division:
        |dy| <= ((n + 2) u + (Ln + 2) u + 2E) sum_s p_s |v_s|,   n = min(t + 1, window)."""
    H, T, _ = ref.scores.shape
    hd = ref.hd
    a_rs = allowance("rsqrtf", torch.tensor([float(hd)]))
    finite = torch.isfinite(ref.scores)
    s0 = torch.where(finite, ref.scores, torch.zeros_like(ref.scores))
    ds = ((hd + 2) * U * ref.sabs / math.sqrt(hd) + s0.abs() * (1 + 2 * a_rs) * U).amax(-1)       # [H, T]
    m = ref.scores.amax(-1, keepdim=True)
    gap = torch.where(finite, (m - ref.scores).clamp(max=104.0), torch.zeros_like(s0))
    a_exp = allowance("expf", -gap[finite].float())
    E = 2 * ds + U * gap.amax(-1) + a_exp * 2 * U                                               # [H, T]
    n = torch.arange(1, T + 1).clamp(max=ref.window).double()[None, :]
    Ln = torch.ceil(n / 64) + 6
    rel = (n + 2) * U + (Ln + 2) * U + 2 * E                                                    # [H, T]
    return (rel.t()[:, :, None] * ref.absv.reshape(T, H, hd)).reshape(T, H * hd)


def transpose(x):
    """out[b][c][r] = in[b][r][c] (exact)."""
    R, Cn = x.shape[-2:]
    out = torch.empty(*x.shape[:-2], Cn, R, dtype=x.dtype)
    for r in range(R):
        out[..., :, r] = x[..., r, :]
    return out


def worst_ratio(got, ref_out, bound):
    """max over ALL elements of |got - ref| / bound; inf for a non-finite result or an error where the bound is 0."""
    got = got.detach().cpu().double().reshape(ref_out.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref_out).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------- cases
def _gen(*xs):
    s = 4242
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


ConvCase = namedtuple("ConvCase", "name C_in C_out k stride dil groups elu res bias pad_left pad_mode T_in T_out neg")


def conv_cases():
    cs = []
    for i, (C_in, C_out, k, dil, groups, elu_, res, bias) in enumerate(CONV_CASES):      # the stream tests' shapes, causal
        cs.append(ConvCase(f"stream{i}", C_in, C_out, k, 1, dil, groups, elu_, res, bias, (k - 1) * dil, 0, 41, 41, False))
    for s, C_in, C_out, k, dil, groups in ((2, 4, 6, 4, 1, 1), (4, 3, 5, 8, 1, 1), (8, 2, 4, 16, 1, 1), (2, 4, 4, 3, 2, 1),
                                           (2, 6, 4, 4, 1, 2), (4, 8, 8, 8, 1, 8), (2, 5, 3, 1, 1, 1)):
        for pm in (0, 1):                               # the encoder's padding: the last taps run past T_in
            pad = (k - 1) * dil + 1 - s
            if pad < 0:
                pad = 0
            cs.append(ConvCase(f"s{s}k{k}d{dil}g{groups}pm{pm}", C_in, C_out, k, s, dil, groups, pm == 1, False, True, pad, pm, 41, -(-41 // s), False))
    cs.append(ConvCase("depthwise", 7, 7, 3, 1, 1, 7, False, True, True, 2, 0, 41, 41, False))
    cs.append(ConvCase("edge_both", 3, 4, 7, 1, 1, 1, True, False, True, 3, 1, 41, 45, False))       # replicate left and right
    cs.append(ConvCase("T1_edge", 3, 4, 7, 1, 1, 1, False, False, True, 3, 1, 1, 4, False))          # every tap reads the edge
    cs.append(ConvCase("T1_zero", 3, 4, 7, 1, 1, 1, False, False, True, 3, 0, 1, 4, False))
    for pm in (0, 1):
        cs.append(ConvCase(f"pad_gt_T_pm{pm}", 2, 3, 3, 1, 1, 1, False, False, True, 9, pm, 5, 12, False))
    cs.append(ConvCase("elu_neg", 5, 6, 3, 1, 1, 1, True, True, True, 2, 0, 41, 41, True))
    return cs


CONV_LOOP = ConvCase("loop", 1, 2, 3, 1, 1, 1, False, False, True, 2, 0, LOOP + 257, LOOP + 257, False)


def conv_inputs(c):
    g = _gen(1, c.C_in, c.C_out, c.k, c.stride, c.dil, c.groups, c.pad_left, c.pad_mode, c.T_in, c.T_out)
    x = torch.randn(c.C_in, c.T_in, generator=g)
    if c.neg:
        x = -x.abs() - 0.1
    w = torch.randn(c.C_out, c.C_in // c.groups, c.k, generator=g)
    b = torch.randn(c.C_out, generator=g) if c.bias else None
    res = torch.randn(c.C_out, c.T_out, generator=g) if c.res else None
    return x, w, b, res


def conv_ref(c, inputs, t_idx=None):
    x, w, b, res = inputs
    return conv1d(x, w, b, res, T_out=c.T_out, stride=c.stride, dilation=c.dil, pad_left=c.pad_left, pad_mode=c.pad_mode,
                  groups=c.groups, elu_in=c.elu, t_idx=t_idx)


ConvtCase = namedtuple("ConvtCase", "name C_in C_out k stride groups elu bias crop T_in T_out")


def convt_cases():
    cs = []
    for i, (C_in, C_out, k, s, groups, elu_, bias) in enumerate(CONVT_CASES):
        T = 29
        cs.append(ConvtCase(f"stream{i}", C_in, C_out, k, s, groups, elu_, bias, 0, T, T * s))           # causal: the decoder's crop
        cs.append(ConvtCase(f"full{i}", C_in, C_out, k, s, groups, elu_, bias, 0, T, (T - 1) * s + k))
        cs.append(ConvtCase(f"crop{i}", C_in, C_out, k, s, groups, elu_, bias, max(k - s, 1), T, T * s - 5))
    cs.append(ConvtCase("k_lt_s_bias", 3, 5, 2, 3, 1, False, True, 0, 29, 29 * 3))                        # gaps no tap reaches
    cs.append(ConvtCase("k_lt_s_nobias", 3, 5, 2, 5, 1, True, False, 1, 29, 28 * 5 + 2))
    return cs


CONVT_LOOP = ConvtCase("loop", 1, 2, 4, 2, 1, False, True, 0, LOOP // 2 + 129, LOOP + 258)


def convt_inputs(c):
    g = _gen(2, c.C_in, c.C_out, c.k, c.stride, c.groups, c.crop, c.T_in, c.T_out)
    x = torch.randn(c.C_in, c.T_in, generator=g)
    w = torch.randn(c.C_in, c.C_out // c.groups, c.k, generator=g)
    b = torch.randn(c.C_out, generator=g) if c.bias else None
    return x, w, b


def convt_ref(c, inputs, t_idx=None):
    x, w, b = inputs
    return conv_transpose1d(x, w, b, T_out=c.T_out, stride=c.stride, crop_left=c.crop, groups=c.groups, elu_in=c.elu, t_idx=t_idx)


def loop_columns(T_out):
    """The columns of a grid-stride case that are judged: 600 around the first index of the second pass and the last 600."""
    cols = torch.cat([torch.arange(LOOP - 300, LOOP + 300), torch.arange(T_out - 600, T_out)])
    return torch.unique(cols[cols < T_out])                        # the two ranges overlap when T_out is LOOP + a few hundred


LN_EPS = 1e-5
LN_CASES = [(T, D, "randn") for D in (1, 63, 64, 65, 512) for T in (1, 3, 4, 5)] + [(3, 65, "offset"), (5, 512, "offset"),
                                                                                     (3, 65, "const"), (4, 64, "const")]


def ln_inputs(case):
    T, D, kind = case
    g = _gen(3, T, D, len(kind))
    x = torch.randn(T, D, generator=g)
    if kind == "offset":
        x[1] = 1e3 + torch.randn(D, generator=g)                   # mean 1e3, spread 1
    if kind == "const":
        x[T // 2] = 3.7                                            # variance 0: eps alone keeps the result finite
    return x, torch.randn(D, generator=g), torch.randn(D, generator=g)


EPILOGUES = ("plain", "res", "gelu", "scale")
LIN_TILED = [(65, 70, 17, 0), (1, 1, 1, 0), (17, 64, 32, 0), (65, 70, 17, 5)]                        # T, N, K, ldx - K
LIN_ROWS = [(T, N, K, pad) for T in (1, 16) for K in (32, 64, 2048) for N in (1, 255, 256, 257) for pad in (0,)] + \
           [(16, 257, 64, 3), (1, 255, 32, 8)]


def linear_inputs(T, N, K, pad, epi):
    """x [T, K + pad] (NaN in the pad columns, which are never read), W, scale, res.  GELU cases scale the rows so that the
    pre-activations span [-6, 6] (checked by the CPU test where N allows it)."""
    g = _gen(4, T, N, K, pad, EPILOGUES.index(epi))
    x = torch.full((T, K + pad), float("nan"))
    x[:, :K] = torch.randn(T, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    if epi == "gelu":
        x[:, :K] *= torch.linspace(3.0, 0.25, T)[:, None] if T > 1 else 3.0
    res = torch.randn(T, N, generator=g) if epi in ("res", "scale") else None
    scale = torch.randn(N, generator=g) if epi == "scale" else None
    return x, W, scale, res, int(epi == "gelu")


ROPE_BASE = 10000.0
ROPE_GEOMS = ((8, 64), (2, 8))
ROPE_POS = (0, 1, 249, 250, 4095)
ROPE_LOOP = (2049, 8, 64, 3)                                       # T, H, hd, pos0: 2049 * 2 * 8 * 32 > 4096 * 256


def rope_inputs(T, H, hd, pos0):
    return torch.randn(T, 3 * H * hd, generator=_gen(5, T, H, hd, pos0))


ATTN_HD = 64
ATTN_CASES = [(H, w) for H in (1, 8) for w in (1, 2, 37, 250)]
ONEHOT_GAP = 40.0                                                  # the least lead of the target key's score in its window


def attn_T(window):
    return window + 70


def attn_random(H, window):
    return torch.randn(attn_T(window), 3 * H * ATTN_HD, generator=_gen(6, H, window))


def value_pattern(T, H, hd):
    """v[t][h][d] = 1 + m / 128 in [1, 2), m = (t + d (1 + (t >> 7)) + 41 h) mod 128: no two (position, head) rows are equal."""
    t = torch.arange(T).view(-1, 1, 1)
    h = torch.arange(H).view(1, -1, 1)
    d = torch.arange(hd).view(1, 1, -1)
    return (1.0 + ((t + d * (1 + (t >> 7)) + 41 * h) % 128).float() / 128.0)


def onehot_queries(window):
    T = attn_T(window)
    return sorted({q for q in (0, window - 1, window, window + 1, T - 1) if 0 <= q < T})


def onehot_case(H, window, q, outside=False):
    """qkv [T, 3 H 64] with randn q / k, pattern values, and ONE key aligned with query ``q``: c q_h per head, c the power of two
    that makes its score c |q_h|^2 / 8 at least 64.  inside: the key sits at max(q - window + 1, 0), the oldest key of the window,
    and the output row q is that key's value row bit for bit (exp(-40) 2 window < 2^-25).  outside: it sits at q - window, which
    the window excludes; the reference ignores it and the ordinary bound judges row q.  -> (qkv, key position or None)."""
    T, hd = attn_T(window), ATTN_HD
    x = torch.randn(T, 3, H, hd, generator=_gen(7, H, window, q, int(outside)))
    x[:, 2] = value_pattern(T, H, hd)
    pos = q - window if outside else max(q - window + 1, 0)
    if pos < 0:
        return None, None
    for h in range(H):
        n2 = float(x[q, 0, h].double().pow(2).sum())
        c = 2.0 ** math.ceil(math.log2(64.0 * 8.0 / n2))
        x[pos, 1, h] = c * x[q, 0, h]
    return x.reshape(T, 3 * H * hd).contiguous(), pos


def onehot_lead(ref, q, pos):
    """The least lead of key ``pos`` over every other key in query q's window, over the heads (float64 reference scores)."""
    s = ref.scores[:, q, :].clone()                                # [H, T]
    target = s[:, pos].clone()
    s[:, pos] = float("-inf")
    return float((target - s.amax(-1)).min())


TRANSPOSE_SIZES = (1, 31, 32, 33, 65)
