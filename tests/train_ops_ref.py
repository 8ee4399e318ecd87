"""A float64 reference of the training step's bandwidth kernels of csrc/ops.hip, a rounding-error bound for each output element
and the seeded cases the two train-ops tests share (test_train_ops_ref_cpu.py proves this module against torch's own float64
machinery, proves that a correct fp32 implementation fits the bounds and that wrong ones do not; test_train_ops_kernels_gpu.py
judges the kernels by it).

Everything is plain torch on the CPU in float64, written from the formula in the comment above each kernel.  The inputs are the
kernel's own operands (bf16 tensors, the fp32 rstd / table / logits / moments) cast to float64, so every reference is the exact
operation on what the kernel read.  A reference returns, per output, ``(value, slack)``: the exact value and the fp32 slack of
the expression, built from ``sabs`` - the sum of the absolute values of the terms added to form the value.

The judge.  ``judge(name, got, ref, slack)`` compares EVERY element: |got - ref| <= bound.  ``slack is None``: bit-for-bit
equality with ``ref`` (a tensor of the output's own type).  An element whose slack is negative must equal the reference exactly
(bound 0): zeroed pad columns, excluded rows, rows that must stay untouched.

Bounds, u = 2^-24 (unit roundoff of fp32), first order in u; none is fitted to a kernel's output.
  bf16 output   bound = hulp(|ref| + slack) + slack, hulp(v) = 2^(floor(log2 v) - 8) = half a bf16 ulp at v (taken at
                |ref| + slack so that an fp32 value just across a binade edge from the reference is covered).
  chain         L fp32 additions over terms t_i err by at most (L + 2) u sum|t_i|.  L is counted from the kernel:
                  row in registers (RMSNorm, CE wave kernel): 8 (4) adds per 16-byte chunk, ceil(chunks / 64) chunks per lane,
                  + 6 butterfly steps; block_sum adds the wave count (4 for 256 threads, 16 for 1024);
                  colsum: each of ns = 16 (rows >= 64) or 4 slices sums c = ceil(rows / ns) rows in four partial sums
                  (c // 4 + c % 4 adds in the longest), 2 adds join them, ns adds join the slices, 1 more with accumulate.
                Products of two bf16 values (16 significant bits) and of such a product with a third bf16 (24 bits) are exact in
                fp32, so x*x, dy*x and dy*x*w carry no rounding of their own.
  functions     rsqrtf, sqrtf, logf and the host's powf / sqrtf: ``codec_ref.allowance`` (4 x the worst ulp error of torch's
                float32 against float64 on the case's own arguments, never below 2 ulp); A ulp <= A 2u of the value.
  __expf(d)     = exp2(d log2 e) on the hardware unit: (|d| + 4) 2u of its value (|d|: the rounding of the product in the
                exponent, 4: the unit), plus u |d| where d itself is a rounded difference: (3|d| + 8) u in all.
  fast_sigmoid  s = rcp(1 + __expf(-g)): ds = s ((1 - s)(|g| + 4) 2u + u + 4u) + 2^-126.  (1 - s) = e / (1 + e) is the weight of
                the exponential in the sum, u the add, 4u = 2 ulp for v_rcp_f32.  2^-126: where exp(-g) leaves the fp32 range
                (g = -90) or 1 / (1 + e) is subnormal, the unit returns 0; the true value is below 2^-126 there.
  RMSNorm fwd   arg = ss / D + eps: (Ls + 2) u + 2u relative, r = rsqrtf(arg): dr / r = half of that + A_rsqrt 2u;
                y = (x r) w: |y| (dr / r + 2u).
  RMSNorm bwd   dot = sum dy x w (exact products): ddot = (Ls + 2) u sum|dy x w|; k = r r r dot / D has 4 roundings:
                dk = r^3 / D ddot + 5u |k|.  dx = r (dy w) - k x + dres: |x| dk + 4u (|r dy w| + |k x| + |dres|) (two products,
                two adds).  dscale = sum_rows dy x r: one rounding per term, then ceil(M / 2048) adds in the row loop of a wave,
                8 to join the waves and the colsum chain over 256 partial rows: (L + 3) u sum|dy x r|.
  RoPE          contraction is off: x0 c - x1 s is two rounded products and one add: 3u (|x0 c| + |x1 s|).
  SwiGLU fwd    silu = g s (u), out = silu up (u): |up| (|g| ds + u |g s|) + u |out|.
  SwiGLU bwd    A = d up s: dA = |d up| ds + 2u |A|.  B = 1 + g (1 - s): dB = |g| (ds + u |1 - s|) + u |g (1 - s)| + u |B| (for
                g >> 0, 1 - s cancels and |g| ds dominates: that is the kernel's formula, not slack).  d gate = A B:
                |B| dA + |A| dB + u |A B|;  d up = d g s: |d g| ds + 2u |d g s|.
  embedding     forward: a chain of one add per live slot; backward: one add per occurrence of the row and one into the table.
  CE            sum = sum exp(x - mx): dsum / sum = sum e_i (3|d_i| + 8) u / sum + (L + 2) u + V 2^-126 / sum, L = 4 NC + 6 (wave
                kernel) or ceil(V / 256) + 6 + 4 (block kernel).  lse = mx + logf(sum): dlse = A_log 2u |log sum| + dsum / sum
                + u |lse|.  loss = lse - x_t: dlse + u |loss|.  p = __expf(x - lse): dp = p (dlse + (3|d| + 8) u) + 2^-126;
                dlogit = (p - onehot) gscale: |gscale| (dp + u |p - onehot|) + u |dlogit|.
  reduce_sum    ceil(n / 1024) + 6 + 16 adds and the product with scale.
  sumsq         exact squares; 8 adds per vector, ceil(nvec / (8192 256)) vectors per thread, 1 tail add, 6 + 4 to join.
  clip_coef     acc: 8 + 6 + 16 adds; norm = sqrtf(acc): dacc / (2 norm) + A_sqrt 2u norm; q = max_norm / (norm + 1e-6f):
                dq = q (dnorm + u (norm + 1e-6)) / (norm + 1e-6) + u q; coef = min(1, q) is exactly 1 where q - dq > 1.
  AdamW         contraction is off, every operation rounds once.  c = 1 - lr wd, 1 - beta1, 1 - beta2, lr / bc1 and the gradient
                factor are fp32 scalars and are recomputed exactly (numpy float32); bc1 = 1 - powf(beta1, t) and
                bc2s = sqrtf(1 - powf(beta2, t)) come from the host's libm: rel(bc1) = (A_pow 2u beta1^t + u bc1) / bc1,
                rel(bc2s) = (A_pow 2u beta2^t + u bc2) / (2 bc2) + A_sqrt 2u.
                  p1 = p c:                         u |p1|
                  g' = g coef:                      u |g'|
                  m' = b1 m + (1 - b1) g':          dm = u (|b1 m| + 2 |(1 - b1) g'| + |m'|)
                  v' = b2 v + ((1 - b2) g') g':     dv = u (|b2 v| + 4 |(1 - b2) g'^2| + |v'|)
                  den = sqrtf(v') / bc2s + eps:     dden = sqrt(v') / bc2s (dv / (2 v') + A_sqrt 2u + u + rel(bc2s)) + u den
                  p' = p1 - (lr / bc1) (m' / den):  dupd = |upd| (rel(bc1) + dden / den + 3u) + (lr / bc1) dm / den,
                                                    dp = u |p1| + dupd + u |p'|.
                Each step is judged from the device's own previous state, so the bounds do not compound.
Exact results (``slack is None``): rows_take, rows_add and bias_add (one fp32 add, one rounding), decoder_input_fwd, the columns
RoPE leaves alone, zero_grad, the bf16 working weight, dropout (an integer restatement of the mask, the host's fp32 scale)."""
import math
from collections import namedtuple

import numpy as np
import torch

from codec_ref import allowance, measured                     # noqa: F401  (measured: the record of the function errors)

U = 2.0 ** -24
TINY = 2.0 ** -126
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = float(np.float32(1e-5))                                 # RMSNorm eps as the kernel receives it
utilisation = {}                                              # name -> worst |err| / bound seen by judge (for the records)


def hulp(v64):
    """Half a bf16 ulp at |v| (normal range)."""
    return torch.exp2(torch.floor(torch.log2(v64.abs().clamp(min=TINY))) - 8)


def trunc_bf16(t32):
    """fp32 -> bf16 by dropping the low 16 bits (a mutant's conversion: the kernels round to nearest even)."""
    return (t32.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def judge(name, got, ref, slack):
    """Every element of ``got`` against ``ref``; -> worst |err| / bound.  See the module docstring."""
    got = got.detach().cpu()
    assert got.numel() == ref.numel(), f"{name}: {got.numel()} elements for {ref.numel()} reference values"
    got = got.reshape(ref.shape)
    if slack is None:
        assert got.dtype == ref.dtype, f"{name}: {got.dtype} judged against {ref.dtype}"
        same = got == ref                                     # integer tensors (raw bits) element by element
        if got.is_floating_point():                          # +0 and -0 are the same value; NaN equals NaN
            same = same | (torch.isnan(got) & torch.isnan(ref))
        judged = int(same.numel())
        assert judged == ref.numel()
        if not bool(same.all()):
            i = int((~same.reshape(-1)).nonzero()[0])
            raise AssertionError(f"{name}: {int((~same).sum())} of {judged} elements differ; first at {i}: got {got.reshape(-1)[i].item()!r}, "
                                 f"reference {ref.reshape(-1)[i].item()!r} (exact)")
        utilisation[name] = max(utilisation.get(name, 0.0), 0.0)
        return 0.0
    ref, slack = ref.double(), slack.double().expand(ref.shape)
    g64 = got.double()
    bound = torch.where(slack < 0, torch.zeros_like(slack), (hulp(ref.abs() + slack) + slack) if got.dtype == BF16 else slack)
    err = (g64 - ref).abs()
    err = torch.where(torch.isfinite(g64), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    judged = int((ratio >= 0).sum())                          # a NaN ratio would be an element that no comparison reaches
    assert judged == ref.numel(), f"{name}: {ref.numel() - judged} elements skipped"
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(j) for j in np.unravel_index(i, tuple(ref.shape))) if ref.dim() else ()
        raise AssertionError(f"{name}: worst element {idx}: got {g64.reshape(-1)[i].item()!r}, reference {ref.reshape(-1)[i].item()!r}, "
                             f"bound {bound.reshape(-1)[i].item():.3e} (|err| / bound = {worst:.3f}; {int((ratio > 1).sum())} of {judged} outside)")
    utilisation[name] = max(utilisation.get(name, 0.0), worst)
    return worst


def judge_all(op, got, ref, what=""):
    """``got`` and ``ref`` are dicts keyed by output name; every output of the reference must be there."""
    worst = 0.0
    for key, (val, slack) in ref.items():
        assert key in got, f"{op}: output {key} missing"
        worst = max(worst, judge(f"{op}.{key}", got[key], val, slack))
    print(f"RATIO {op} {worst:.4f} {what}")
    return worst


def _gen(*xs):
    s = 777
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _rb(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def _lane_chain(D):
    """Adds on the way to a wave-wide sum over a row of D bf16 held in registers."""
    return -(-(D // 8) // 64) * 8 + 6


def colsum_chain(rows, accumulate):
    ns = 16 if rows >= 64 else 4
    c = -(-rows // ns)
    return c // 4 + c % 4 + 2 + ns + int(bool(accumulate))


Op = namedtuple("Op", "cases inputs ref f32 mutants")
OPS = {}


# ------------------------------------------------------------------------------------------------------------- RMSNorm
RmsCase = namedtuple("RmsCase", "M D dres dsc rstd")
RMS_D = (8, 264, 512, 520, 1032, 2048, 2056, 3080, 4096)


def _rms_cases():
    cs = [RmsCase(M, D, a, b, a != b) for D in RMS_D for M in (1, 5) for a in (False, True) for b in (False, True)]
    cs += [RmsCase(2053, D, i % 2 == 0, i % 3 != 1, i % 2 == 1) for i, D in enumerate(RMS_D)]      # two trips of the backward's row loop
    return cs


RMS_BWD_CASES = _rms_cases() + [RmsCase(4101, 264, True, True, True)]                              # three trips
RMS_FWD_CASES = [RmsCase(M, D, False, False, r) for D in RMS_D for M in (1, 5, 2053) for r in ((False, True) if M < 2053 else (D % 16 == 0,))] + \
                [RmsCase(16390, 8, False, False, True)]                                            # past 4096 blocks x 4 rows


def rms_inputs(c):
    g = _gen(10, c.M, c.D)
    x = _rb(g, c.M, c.D)
    if c.M >= 5:
        x[1] = 0                                               # rstd = 1 / sqrt(eps)
        x[3] = (x[3].float() * 2.0 ** 40).to(BF16)
    w = (1.0 + 0.5 * torch.randn(c.D, generator=g)).to(BF16)
    dy, dres = _rb(g, c.M, c.D), _rb(g, c.M, c.D)
    rstd = torch.rsqrt((x.float() ** 2).sum(1) / c.D + EPS)    # the backward's fp32 operand
    return dict(c=c, x=x, w=w, dy=dy, dres=dres if c.dres else None, rstd=rstd)


def rms_fwd_ref(i):
    c, x, w = i["c"], i["x"].double(), i["w"].double()
    ss = (x * x).sum(1)
    arg = ss / c.D + EPS
    r = 1.0 / torch.sqrt(arg)
    drel = 0.5 * ((_lane_chain(c.D) + 2) * U + 2 * U) + allowance("rsqrtf", arg.float()) * 2 * U
    y = x * r[:, None] * w
    out = {"y": (y, y.abs() * (drel + 2 * U))}
    if c.rstd:
        out["rstd"] = (r, r * drel)
    return out


def rms_fwd_f32(i, mut=None):
    c, x, w = i["c"], i["x"].float(), i["w"].float()
    ss = (x * x).sum(1)
    r = torch.rsqrt(ss / (c.D + 8 if mut == "mean_D8" else c.D) + (0.0 if mut == "no_eps" else EPS))
    y = x * r[:, None] * w
    return {"y": trunc_bf16(y) if mut == "trunc" else y.to(BF16), "rstd": r}


def rms_bwd_ref(i):
    c, x, w, g, r = i["c"], i["x"].double(), i["w"].double(), i["dy"].double(), i["rstd"].double()
    res = i["dres"].double() if c.dres else torch.zeros_like(x)
    gw = g * w
    dot, sdot = (gw * x).sum(1), (gw * x).abs().sum(1)
    k = r ** 3 * dot / c.D
    dk = r ** 3 / c.D * (_lane_chain(c.D) + 2) * U * sdot + 5 * U * k.abs()
    t1, t2 = r[:, None] * gw, k[:, None] * x
    out = {"dx": (t1 - t2 + res, x.abs() * dk[:, None] + 4 * U * (t1.abs() + t2.abs() + res.abs()))}
    if c.dsc:
        terms = g * x * r[:, None]
        L = -(-c.M // 2048) + 8 + colsum_chain(256, False)
        out["dscale"] = (terms.sum(0), (L + 3) * U * terms.abs().sum(0))
    return out


def rms_bwd_f32(i, mut=None):
    c, x, w, g, r = i["c"], i["x"].float(), i["w"].float(), i["dy"].float(), i["rstd"]
    res = i["dres"].float() if c.dres else torch.zeros_like(x)
    gx = g * x
    dot = (gx * w).sum(1)
    k = (r * r if mut == "rstd_sq" else r * r * r) * dot / (c.D - 8 if mut == "div_D8" else c.D)
    o = r[:, None] * (g * w) - k[:, None] * x + res
    ds = (gx * r[:, None])[:-1 if mut == "drop_row" else None].sum(0)
    return {"dx": trunc_bf16(o) if mut == "trunc" else o.to(BF16), "dscale": ds.to(BF16)}


OPS["rmsnorm_fwd"] = Op(RMS_FWD_CASES, rms_inputs, rms_fwd_ref, rms_fwd_f32, ("mean_D8", "no_eps", "trunc"))
OPS["rmsnorm_bwd"] = Op(RMS_BWD_CASES, rms_inputs, rms_bwd_ref, rms_bwd_f32, ("div_D8", "rstd_sq", "trunc", "drop_row"))


# ------------------------------------------------------------------------------------------------------------- colsum
ColsumCase = namedtuple("ColsumCase", "rows D acc n")
COLSUM_CASES = [ColsumCase(r, D, a, 1) for r in (1, 3, 4, 17, 63, 64, 65, 256) for D in (8, 64, 72, 2048) for a in (False, True)] + \
               [ColsumCase(r, 72, a, n) for r in (17, 65) for n in (1, 3, 8) for a in (False, True)]


def colsum_inputs(c):
    g = _gen(20, *c)
    return dict(c=c, partials=[torch.randn(c.rows, c.D, generator=g) for _ in range(c.n)], dst=[_rb(g, c.D) for _ in range(c.n)])


def colsum_ref(i):
    c, out = i["c"], {}
    for k, (p, d) in enumerate(zip(i["partials"], i["dst"])):
        p, d = p.double(), d.double() * int(c.acc)
        out[f"dst{k}"] = (p.sum(0) + d, (colsum_chain(c.rows, c.acc) + 2) * U * (p.abs().sum(0) + d.abs()))
    return out


def colsum_f32(i, mut=None):
    c, out = i["c"], {}
    ns = 16 if c.rows >= 64 else 4
    used = c.rows - c.rows % (4 * ns) if mut == "drop_remainder" else c.rows
    for k, (p, d) in enumerate(zip(i["partials"], i["dst"])):
        t = p[:used].sum(0) + (d.float() if c.acc and mut != "no_acc" else 0.0)
        out[f"dst{k}"] = trunc_bf16(t) if mut == "trunc" else t.to(BF16)
    return out


OPS["colsum"] = Op(COLSUM_CASES, colsum_inputs, colsum_ref, colsum_f32, ("drop_remainder", "no_acc", "trunc"))

ColsumRowsCase = namedtuple("ColsumRowsCase", "M S D ld")
COLSUM_ROWS_CASES = [ColsumRowsCase(M, S, D, D + pad) for M in (1, 3, 4, 5, 1000) for S in (1, 2, 64) for D, pad in ((8, 0), (72, 0), (72, 24))]


def colsum_rows_inputs(c):
    return dict(c=c, x=_rb(_gen(21, *c), c.M, c.ld))


def _slice_of_row(c):
    return (torch.arange(c.M) // 4) % c.S


def colsum_rows_ref(i):
    c, x = i["c"], i["x"].double()[:, :i["c"].D]
    sl = _slice_of_row(c)
    val = torch.zeros(c.S, c.D, dtype=F64).index_add_(0, sl, x)
    sabs = torch.zeros(c.S, c.D, dtype=F64).index_add_(0, sl, x.abs())
    return {"partials": (val, (-(-c.M // (4 * c.S)) + 3 + 2) * U * sabs)}


def colsum_rows_f32(i, mut=None):
    c, x = i["c"], i["x"].float()[:, :i["c"].D]
    sl = _slice_of_row(c)
    if mut == "drop_q3":
        x = x * (torch.arange(c.M) % 4 != 3)[:, None]
    if mut == "slice_mod":
        sl = torch.arange(c.M) % c.S
    return {"partials": torch.zeros(c.S, c.D).index_add_(0, sl, x)}


OPS["colsum_rows"] = Op(COLSUM_ROWS_CASES, colsum_rows_inputs, colsum_rows_ref, colsum_rows_f32, ("drop_q3", "slice_mod"))


# ------------------------------------------------------------------------------------------------------------- dropout, bias
DropCase = namedtuple("DropCase", "M D ld_in ld_out p seed acc")
DROP_CASES = [DropCase(M, D, D + a, D + b, p, seed, acc) for (M, D) in ((1, 8), (5, 72), (37, 520)) for (a, b) in ((0, 0), (8, 16))
              for p, seed in ((0.0, 1), (0.1, 0x123456789abcdef), (0.5, 2 ** 64 - 1), (0.9, 7)) for acc in (False, True)] + \
             [DropCase(8200, 2048, 2048, 2048, 0.25, 99, False)]                       # past 8192 blocks x 256 chunks
_M64 = np.uint64


def dropout_thresh_scale(p):
    """The host's fp32 arithmetic: thresh = (uint32)(p 65536 + 0.5), scale = 1 / (1 - thresh / 65536)."""
    thresh = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    assert thresh == int(float(np.float32(p)) * 65536 + 0.5)
    return thresh, np.float32(1.0) / (np.float32(1.0) - np.float32(thresh) / np.float32(65536.0))


def dropout_keep(seed, M, D, p):
    """keep[row][col]: 16 bits of splitmix64(seed ^ (e 0xd1342543de82ef95)), e = (row D + col) >> 2, field (row D + col) & 3."""
    thresh, _ = dropout_thresh_scale(p)
    idx = np.arange(M * D, dtype=np.uint64)
    z = (np.full(1, seed, dtype=np.uint64) ^ ((idx >> _M64(2)) * _M64(0xd1342543de82ef95))) + _M64(0x9e3779b97f4a7c15)
    z = (z ^ (z >> _M64(30))) * _M64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> _M64(27))) * _M64(0x94d049bb133111eb)
    z = z ^ (z >> _M64(31))
    bits = (z >> ((idx & _M64(3)) * _M64(16))) & _M64(0xffff)
    return torch.from_numpy((bits >= _M64(thresh)).reshape(M, D))


def drop_inputs(c):
    g = _gen(30, c.M, c.D, c.ld_in, c.ld_out, int(c.p * 100), c.acc)
    return dict(c=c, x=_rb(g, c.M, c.ld_in), out0=_rb(g, c.M, c.ld_out))


def drop_f32(i, mut=None):
    c = i["c"]
    _, scale = dropout_thresh_scale(c.p)
    keep = dropout_keep(c.seed ^ (1 if mut == "seed" else 0), c.M, c.D, c.p)
    v = torch.where(keep, i["x"][:, :c.D].float() * (1.0 if mut == "no_scale" else float(scale)), torch.zeros(()))
    if c.acc:
        v = i["out0"][:, :c.D].float() + v
    out = i["out0"].clone()                                 # columns >= D of the output stay as they were
    out[:, :c.D] = v.to(BF16)
    return {"out": out}


def drop_ref(i):
    return {"out": (drop_f32(i)["out"], None)}


OPS["dropout"] = Op(DROP_CASES, drop_inputs, drop_ref, drop_f32, ("no_scale", "seed"))

BiasCase = namedtuple("BiasCase", "M D ld")
BIAS_CASES = [BiasCase(M, D, D + pad) for M in (1, 5, 37) for D, pad in ((8, 0), (72, 8), (520, 0))] + [BiasCase(8200, 2048, 2048)]


def bias_inputs(c):
    g = _gen(31, *c)
    return dict(c=c, y=_rb(g, c.M, c.ld), bias=_rb(g, c.D))


def bias_f32(i, mut=None):
    c, out = i["c"], i["y"].clone()
    t = i["y"][:, :c.D].float() + i["bias"].float() * (0.0 if mut == "no_bias" else 1.0)
    out[:, :c.D] = trunc_bf16(t) if mut == "trunc" else t.to(BF16)
    return {"y": out}


OPS["bias_add"] = Op(BIAS_CASES, bias_inputs, lambda i: {"y": (bias_f32(i)["y"], None)}, bias_f32, ("no_bias", "trunc"))


# ------------------------------------------------------------------------------------------------------------- RoPE
RopeCase = namedtuple("RopeCase", "name M S nh nv hd extra use_pos inverse P")
ROPE_CASES = [RopeCase(f"hd{hd}_{'pos' if up else 'rows'}_{'inv' if inv else 'fwd'}_x{extra}", 7, 3, 3, 1, hd, extra, up, inv, 16)
              for hd in (64, 128) for up in (False, True) for inv in (False, True) for extra in (0, 24)] + \
             [RopeCase("grid_loop", 16400, 11, 16, 1, 64, 0, False, False, 16)]         # 16400 x 16 x 8 chunks > 8192 x 256


def rope_inputs(c):
    from oracle.csm_oracle import rope_table
    g = _gen(40, c.M, c.S, c.nh, c.hd, c.extra, c.use_pos, c.inverse)
    pos = torch.randint(0, c.P, (c.M,), generator=g).int()
    pos[0], pos[-1] = 0, c.P - 1                              # the first and the last table row
    if not c.use_pos:
        assert c.M % c.S and c.S <= c.P
        pos = (torch.arange(c.M) % c.S).int()
    return dict(c=c, qkv=_rb(g, c.M, (c.nh + c.nv) * c.hd + c.extra), table=rope_table(c.P, c.hd), pos=pos)


def _rope(i, dt, mut=None):
    c = i["c"]
    W = c.nh * c.hd
    x = i["qkv"][:, :W].to(dt).reshape(c.M, c.nh, c.hd // 2, 2)
    t = i["table"].to(dt)[i["pos"].long()][:, None]           # [M, 1, hd/2, 2]
    cs, sn = t[..., 0], t[..., 1] * (-1.0 if c.inverse and mut != "inv_sign" else 1.0)
    x0, x1 = (x[..., 1], x[..., 0]) if mut == "swap" else (x[..., 0], x[..., 1])
    a, b, d, e = x0 * cs, x1 * sn, x1 * cs, x0 * sn
    return torch.stack([a - b, d + e], -1).reshape(c.M, W), torch.stack([a.abs() + b.abs(), d.abs() + e.abs()], -1).reshape(c.M, W)


def rope_ref(i):
    c = i["c"]
    val, sabs = _rope(i, F64)
    return {"rot": (val, 3 * U * sabs), "rest": (i["qkv"][:, c.nh * c.hd:].clone(), None)}


def rope_f32(i, mut=None):
    c = i["c"]
    val, _ = _rope(i, F32, mut)
    return {"rot": trunc_bf16(val) if mut == "trunc" else val.to(BF16), "rest": i["qkv"][:, c.nh * c.hd:].clone()}


OPS["rope"] = Op(ROPE_CASES, rope_inputs, rope_ref, rope_f32, ("swap", "inv_sign", "trunc"))


# ------------------------------------------------------------------------------------------------------------- SwiGLU
SwigluCase = namedtuple("SwigluCase", "M F")
SWIGLU_CASES = [SwigluCase(M, F) for M in (1, 7) for F in (8, 24, 1024)] + [SwigluCase(8200, 1024)]      # 8200 x 256 > 8192 x 256
PLANTED_GATES = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0)


def swiglu_inputs(c):
    g = _gen(50, *c)
    gate, up, dout = torch.randn(c.M, c.F, generator=g) * 3, torch.randn(c.M, c.F, generator=g), torch.randn(c.M, c.F, generator=g)
    gate[:, :6] = torch.tensor(PLANTED_GATES)
    gate[-1, 2:8] = torch.tensor(PLANTED_GATES)               # next to random ones, in the last row as well
    up[:, 1], dout[:, 3], up[-1, 7], dout[-1, 6] = 0, 0, 0, 0
    return dict(c=c, gu=torch.stack([gate, up], -1).reshape(c.M, 2 * c.F).to(BF16), dout=dout.to(BF16))


def _sig(g):
    s = torch.sigmoid(g)
    return s, s * ((1 - s) * (g.abs() + 4) * 2 * U + 5 * U) + TINY


def swiglu_fwd_ref(i):
    gu = i["gu"].double()
    g, up = gu[:, 0::2], gu[:, 1::2]
    s, ds = _sig(g)
    out = g * s * up
    return {"out": (out, up.abs() * (g.abs() * ds + U * (g * s).abs()) + U * out.abs())}


def swiglu_fwd_f32(i, mut=None):
    gu = i["gu"].float()
    g, up = (gu[:, 1::2], gu[:, 0::2]) if mut == "swap" else (gu[:, 0::2], gu[:, 1::2])
    s = 1.0 / (1.0 + torch.exp(-g))
    out = (s if mut == "sigmoid_only" else g * s) * up
    return {"out": trunc_bf16(out) if mut == "trunc" else out.to(BF16)}


def swiglu_bwd_ref(i):
    gu, d = i["gu"].double(), i["dout"].double()
    g, up = gu[:, 0::2], gu[:, 1::2]
    s, ds = _sig(g)
    A, B = d * up * s, 1 + g * (1 - s)
    dA = (d * up).abs() * ds + 2 * U * A.abs()
    dB = g.abs() * (ds + U * (1 - s).abs()) + U * (g * (1 - s)).abs() + U * B.abs()
    og, ou = A * B, d * g * s
    sg, su = B.abs() * dA + A.abs() * dB + U * og.abs(), (d * g).abs() * ds + 2 * U * ou.abs()
    return {"dgu": (torch.stack([og, ou], -1).reshape(gu.shape), torch.stack([sg, su], -1).reshape(gu.shape))}


def swiglu_bwd_f32(i, mut=None):
    gu, d = i["gu"].float(), i["dout"].float()
    g, up = gu[:, 0::2], gu[:, 1::2]
    s = 1.0 / (1.0 + torch.exp(-g))
    og = d * up * s * (1.0 if mut == "no_gt_term" else 1.0 + g * (1.0 - s))
    ou = d * g * s
    o = torch.stack([ou, og] if mut == "swap" else [og, ou], -1).reshape(gu.shape)
    return {"dgu": trunc_bf16(o) if mut == "trunc" else o.to(BF16)}


OPS["swiglu_fwd"] = Op(SWIGLU_CASES, swiglu_inputs, swiglu_fwd_ref, swiglu_fwd_f32, ("swap", "sigmoid_only", "trunc"))
OPS["swiglu_bwd"] = Op(SWIGLU_CASES, swiglu_inputs, swiglu_bwd_ref, swiglu_bwd_f32, ("no_gt_term", "swap", "trunc"))


# ------------------------------------------------------------------------------------------------------------- embedding
VT, VA = 11, 7                                                # text rows, rows per audio codebook
EmbCase = namedtuple("EmbCase", "K D")
EMBED_CASES = [EmbCase(K, D) for K in (1, 32) for D in (8, 264, 2048)]


def embed_inputs(c):
    g = _gen(60, *c)
    K, M = c.K, 8
    tok = torch.randint(0, VA, (M, K + 1), generator=g)
    tok[:, K] = torch.randint(0, VT, (M,), generator=g)
    mask = (torch.rand(M, K + 1, generator=g) < 0.5).to(torch.uint8)
    mask[0] = 0                                               # no live slot: a zero row
    mask[1] = 1                                               # all live
    mask[2] = 0; mask[2, K] = 1                               # only text
    mask[3] = 0; mask[3, K - 1] = 1                           # only the last audio slot
    tok[4] = 0; mask[4] = 1                                   # token 0 everywhere
    tok[5, :K] = VA - 1; tok[5, K] = VT - 1; mask[5] = 1      # the last token of every codebook and of the text table
    return dict(c=c, tokens=tok, mask=mask, text=_rb(g, VT, c.D), audio=_rb(g, K * VA, c.D))


def _embed(i, dt, mut=None):
    c, tok, mask = i["c"], i["tokens"], i["mask"]
    out, sabs = torch.zeros(tok.shape[0], c.D, dtype=dt), torch.zeros(tok.shape[0], c.D, dtype=dt)
    for s in range(c.K + 1):
        if s == c.K:
            if mut == "skip_text":
                continue
            row = i["text"].to(dt)[tok[:, s]]
        else:
            row = i["audio"].to(dt)[tok[:, s] + (0 if mut == "no_codebook_offset" else s * VA)]
        row = row * mask[:, s, None].to(dt)
        out, sabs = out + row, sabs + row.abs()
    return out, sabs


def embed_ref(i):
    out, sabs = _embed(i, F64)
    return {"out": (out, (i["mask"].sum(1, keepdim=True).double() + 2) * U * sabs)}


def embed_f32(i, mut=None):
    out = _embed(i, F32, mut)[0]
    return {"out": trunc_bf16(out) if mut == "trunc" else out.to(BF16)}


OPS["embed_fwd"] = Op(EMBED_CASES, embed_inputs, embed_ref, embed_f32, ("skip_text", "no_codebook_offset", "trunc"))

EmbBwdCase = namedtuple("EmbBwdCase", "name D runs pad zero_tab")            # runs: (embedding row, occurrences), ascending rows
EB_TEXT, EB_AUDIO, EB_M, EB_MS = 5, 6, 6, 5                                    # table rows; rows of dh and of dseq
EMBED_BWD_CASES = [
    EmbBwdCase("one", 8, ((3, 1),), 0, False), EmbBwdCase("two_same", 264, ((0, 2),), 0, False),
    EmbBwdCase("two_rows", 264, ((4, 1), (5, 1)), 0, False),                   # the last text row and the first audio row
    EmbBwdCase("three", 2048, ((2, 3),), 0, False), EmbBwdCase("five", 8, ((1, 2), (10, 3)), 0, False),
    EmbBwdCase("n41", 264, ((0, 1), (3, 17), (7, 22), (10, 1)), 0, False), EmbBwdCase("n41_zero", 264, ((0, 1), (3, 17), (7, 22), (10, 1)), 0, True),
    EmbBwdCase("run300", 264, ((2, 300), (6, 3)), 2, False), EmbBwdCase("pad_end", 2048, ((1, 2),), 3, False),
    EmbBwdCase("only_pad", 8, (), 4, False), EmbBwdCase("d4096", 4096, ((0, 1), (9, 4)), 1, False),
]


def embed_bwd_inputs(c):
    g = _gen(61, c.D, len(c.runs), c.pad, c.zero_tab, sum(n for _, n in c.runs))
    rows = [r for r, n in c.runs for _ in range(n)] + [EB_TEXT + EB_AUDIO] * c.pad
    n_occ = len(rows)
    src = (torch.randperm(max(n_occ, EB_M + EB_MS), generator=g)[:n_occ]) % (EB_M + EB_MS)      # both sources
    tab = torch.zeros(EB_TEXT + EB_AUDIO, c.D, dtype=BF16) if c.zero_tab else _rb(g, EB_TEXT + EB_AUDIO, c.D)
    return dict(c=c, rows=torch.tensor(rows, dtype=torch.int64), src=src.long(), dh=_rb(g, EB_M, c.D), dseq=_rb(g, EB_MS, c.D),
                g_text=tab[:EB_TEXT].clone(), g_audio=tab[EB_TEXT:].clone())


def _embed_bwd(i, dt, mut=None):
    c = i["c"]
    grads = torch.cat([i["dh"], i["dseq"]]).to(dt)
    tab = torch.cat([i["g_text"], i["g_audio"]]).to(dt)
    acc, sabs, cnt = torch.zeros_like(tab), torch.zeros_like(tab), torch.zeros(tab.shape[0])
    rows = i["rows"].tolist()
    for k, r in enumerate(rows):
        if r >= tab.shape[0] or (mut == "drop_last" and (k + 1 == len(rows) or rows[k + 1] != r)):
            continue
        row = grads[int(i["src"][k])]
        acc[r], sabs[r], cnt[r] = acc[r] + row, sabs[r] + row.abs(), cnt[r] + 1
    return tab + acc, tab.abs() + sabs, cnt


def embed_bwd_ref(i):
    val, sabs, cnt = _embed_bwd(i, F64)
    slack = torch.where(cnt[:, None] > 0, (cnt[:, None].double() + 3) * U * sabs, torch.full_like(sabs, -1.0))   # untouched rows: exact
    return {"g_text": (val[:EB_TEXT], slack[:EB_TEXT]), "g_audio": (val[EB_TEXT:], slack[EB_TEXT:])}


def embed_bwd_f32(i, mut=None):
    val = _embed_bwd(i, F32, mut)[0]
    val = trunc_bf16(val) if mut == "trunc" else val.to(BF16)
    return {"g_text": val[:EB_TEXT], "g_audio": val[EB_TEXT:]}


OPS["embed_bwd_sorted"] = Op(EMBED_BWD_CASES, embed_bwd_inputs, embed_bwd_ref, embed_bwd_f32, ("drop_last", "trunc"))


# ------------------------------------------------------------------------------------------------------------- row moves
RowsCase = namedtuple("RowsCase", "D N stride")
ROWS_CASES = [RowsCase(D, N, s) for D in (8, 520, 2048) for N in (1, 4, 5) for s in (1, 32)]
ROWS_T = 9


def rows_inputs(c):
    g = _gen(70, *c)
    rows = torch.randperm(ROWS_T, generator=g)[:c.N].int()
    if c.N >= 4:
        rows[1], rows[c.N - 1] = -1, -3                       # padding entries
    return dict(c=c, table=_rb(g, ROWS_T, c.D), rows=rows, src=_rb(g, c.N * c.stride, c.D))


def rows_add_f32(i, mut=None):
    c, out = i["c"], i["table"].clone()
    for n, r in enumerate(i["rows"].tolist()):
        if r >= 0:
            t = out[r].float() + i["src"][n * (1 if mut == "stride1" else c.stride)].float()
            out[r] = trunc_bf16(t) if mut == "trunc" else t.to(BF16)
    return {"dst": out}


def rows_take_f32(i, mut=None):
    c, tab = i["c"], i["table"].clone()
    out = torch.zeros(c.N, c.D, dtype=BF16)
    for n, r in enumerate(i["rows"].tolist()):
        if r >= 0:
            out[n] = tab[r]
            if mut != "no_zero":
                tab[r] = 0
    return {"out": out, "table": tab}


def _exact(f32):
    return lambda i: {k: (v, None) for k, v in f32(i).items()}


OPS["rows_add"] = Op(ROWS_CASES, rows_inputs, _exact(rows_add_f32), rows_add_f32, ("stride1", "trunc"))
OPS["rows_take"] = Op([c for c in ROWS_CASES if c.stride == 1], rows_inputs, _exact(rows_take_f32), rows_take_f32, ("no_zero",))

DecInCase = namedtuple("DecInCase", "D N K")
DECIN_CASES = [DecInCase(D, N, K) for D in (8, 520, 2048) for N in (1, 4, 5) for K in (1, 32)]


def decin_inputs(c):
    g = _gen(71, *c)
    codes = torch.randint(0, VA, (c.N, c.K), generator=g)
    codes[0] = 0
    codes[-1] = VA - 1
    return dict(c=c, hidden=_rb(g, 7, c.D), rows=torch.randint(0, 7, (c.N,), generator=g).int(), codes=codes, audio=_rb(g, c.K * VA, c.D))


def decin_f32(i, mut=None):
    c = i["c"]
    out = torch.zeros(c.N, c.K, c.D, dtype=BF16)
    out[:, 0] = i["hidden"][i["rows"].long()]
    for k in range(1, c.K):
        out[:, k] = i["audio"][i["codes"][:, k - 1] + (k if mut == "codebook_off_by_one" else k - 1) * VA]
    if mut == "row0":
        out[:, 0] = i["hidden"][0]
    return {"out": out}


OPS["decoder_input_fwd"] = Op(DECIN_CASES, decin_inputs, _exact(decin_f32), decin_f32, ("codebook_off_by_one", "row0"))


# ------------------------------------------------------------------------------------------------------------- cross-entropy
CeCase = namedtuple("CeCase", "name V ldl ldd has_d offset R")
_CE_PATHS = (("nc4", 1000, 1024, 1024, True, 0), ("nc9", 2051, 2112, 2112, True, 0), ("nc12", 3000, 3072, 3072, True, 0),
             ("block_odd_stride", 2051, 2051, 2051, True, 0), ("block_width", 3100, 3104, 3104, True, 0),
             ("block_misaligned", 1000, 1024, 1024, True, 1), ("ldd_lt_ldl", 1001, 1024, 1004, True, 0),
             ("ldd_gt_ldl", 1001, 1024, 1032, True, 0), ("no_dlogits", 2051, 2112, 0, False, 0), ("pad_garbage", 1001, 1024, 1024, True, 0))
CE_CASES = [CeCase(*p, R) for p in _CE_PATHS for R in (1, 5, 9)]
CE_GSCALE = float(np.float32(1.0 / 7.0))
CE_GARBAGE = 1e30                                             # what the pad columns of the logits hold: large, finite, never to be read


def ce_kernel_chain(c, aligned=True):
    """The dispatch of csm_ce_fwd_bwd: -> (kernel, adds on the way to the row's sum)."""
    width = max(c.ldl, c.ldd) if c.has_d else c.ldl
    vec = c.ldl % 4 == 0 and c.offset == 0 and aligned and (not c.has_d or (c.ldd % 4 == 0 and c.ldd <= c.ldl))
    if vec and width <= 256 * 12:
        nc = 4 if width <= 1024 else 9 if width <= 2304 else 12
        return f"wave{nc}", 4 * nc + 6
    return "block", -(-c.V // 256) + 6 + 4


def ce_inputs(c):
    g = _gen(80, c.V, c.ldl, c.ldd, c.has_d, c.offset, c.R)
    x = torch.randn(c.R, c.V, generator=g) * 2
    tg = torch.randint(0, c.V, (c.R,), generator=g)
    if c.R >= 5:
        tg[0] = 0
        tg[1] = -1                                            # not part of the loss
        x[2, tg[2]] += 40.0                                   # the target holds almost all the mass: loss near 0
        x[3] = torch.rand(c.V, generator=g) * 80 - 40         # logits spread over +-40
        tg[4] = c.V - 1
    else:
        tg[0] = c.V - 1
    if c.R > 5:
        tg[c.R - 1] = -7                                      # an excluded row in the last block
    buf = torch.full((c.R, c.ldl), CE_GARBAGE)
    buf[:, :c.V] = x
    return dict(c=c, logits=buf, targets=tg)


def ce_ref(i):
    c, tg = i["c"], i["targets"]
    x = i["logits"][:, :c.V].double()
    live = tg >= 0
    t = tg.clamp(min=0)
    mx = x.amax(1)
    d0 = x - mx[:, None]
    e = torch.exp(d0)
    s = e.sum(1)
    logs = torch.log1p(e.scatter(1, x.argmax(1, keepdim=True), 0.0).sum(1))       # log(sum) with the leading 1 kept apart
    lse = mx + logs
    L = ce_kernel_chain(c)[1]
    relsum = (e * (3 * d0.abs() + 8) * U).sum(1) / s + (L + 2) * U + c.V * TINY / s
    dlse = allowance("logf", s.float()) * 2 * U * logs + relsum + U * lse.abs()
    loss = lse - x.gather(1, t[:, None])[:, 0]
    out = {"loss_rows": (loss * live, torch.where(live, dlse + U * loss.abs(), torch.full_like(loss, -1.0)))}
    if c.has_d:
        d = x - lse[:, None]
        p = torch.exp(d)
        dp = p * (dlse[:, None] + (3 * d.abs() + 8) * U) + TINY
        oh = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
        gr = (p - oh) * CE_GSCALE
        val, slack = torch.zeros(c.R, c.ldd, dtype=F64), torch.full((c.R, c.ldd), -1.0, dtype=F64)       # pad columns: exactly 0
        val[:, :c.V] = gr * live[:, None]
        slack[:, :c.V] = torch.where(live[:, None], CE_GSCALE * (dp + U * (p - oh).abs()) + U * gr.abs(), torch.full_like(gr, -1.0))
        out["dlogits"] = (val, slack)
    return out


def ce_f32(i, mut=None):
    c, tg = i["c"], i["targets"]
    x = i["logits"][:, :c.V + (1 if mut == "read_pad" and c.ldl > c.V else 0)]
    live = tg >= 0
    t = tg.clamp(min=0)
    mx = x.amax(1)
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(1))
    out = {"loss_rows": (lse - x.gather(1, t[:, None])[:, 0]) * live}
    p = torch.exp(x - lse[:, None])[:, :c.V]
    oh = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    gr = (p - (0.0 if mut == "no_onehot" else oh)) * CE_GSCALE
    if mut == "no_gscale_target":
        gr = torch.where(oh > 0, p - oh, gr)
    full = torch.zeros(c.R, max(c.ldd, c.V))
    full[:, :c.V] = gr * live[:, None]
    out["dlogits"] = (trunc_bf16(full) if mut == "trunc" else full.to(BF16))[:, :c.ldd]
    return out


OPS["ce_fwd_bwd"] = Op(CE_CASES, ce_inputs, ce_ref, ce_f32, ("no_onehot", "no_gscale_target", "read_pad", "trunc"))

REDUCE_N = (1, 1023, 1025)
REDUCE_SCALE = float(np.float32(1.0 / 3.0))


def reduce_inputs(n):
    return dict(c=n, x=torch.randn(n, generator=_gen(81, n)))


def reduce_ref(i):
    x, n = i["x"].double(), i["x"].numel()
    val = x.sum() * REDUCE_SCALE
    return {"out": (val.reshape(1), ((-(-n // 1024) + 6 + 16 + 2) * U * x.abs().sum() * REDUCE_SCALE + U * val.abs()).reshape(1))}


def reduce_f32(i, mut=None):
    x = i["x"][:-1] if mut == "drop_last" and i["x"].numel() > 1 else i["x"]
    return {"out": (x.sum() * (1.0 if mut == "no_scale" else REDUCE_SCALE)).reshape(1)}


OPS["reduce_sum"] = Op(REDUCE_N, reduce_inputs, reduce_ref, reduce_f32, ("drop_last", "no_scale"))


# ------------------------------------------------------------------------------------------------------------- sumsq, clip
SUMSQ_BLOCKS, SUMSQ_STRIDE = 8192, 8192 * 256
SumsqCase = namedtuple("SumsqCase", "n offset")
SUMSQ_BIG = SumsqCase(8 * (4 * SUMSQ_STRIDE + 5) + 3, 0)      # the unrolled-by-4 loop, 5 vectors of remainder loop, a tail of 3
SUMSQ_CASES = [SumsqCase(n, 0) for n in (1, 7, 8, 13, 2051, 8000)] + [SumsqCase(2051, 8), SUMSQ_BIG]


def sumsq_inputs(c):
    g = _gen(90, *c)
    buf = torch.randn(c.n + c.offset, generator=g).to(BF16)
    return dict(c=c, buf=buf, g=buf[c.offset:])


def _sumsq(i, dt, mut=None):
    c, g = i["c"], i["g"]
    nvec = c.n // 8
    if mut == "drop_last_unroll":
        nvec = min(nvec, 3 * SUMSQ_STRIDE)
    per_vec = torch.empty(-(-max(nvec, 1) // SUMSQ_STRIDE) * SUMSQ_STRIDE, dtype=dt).zero_()
    for a in range(0, nvec, 1 << 20):                         # in pieces: the large case is 67 M values
        b = min(nvec, a + (1 << 20))
        per_vec[a:b] = (g[a * 8:b * 8].to(dt).view(-1, 8) ** 2).sum(1)
    out = per_vec.view(-1, SUMSQ_BLOCKS, 256).sum((0, 2))
    if mut != "no_tail":
        out[0] += (g[(c.n // 8) * 8:].to(dt) ** 2).sum()
    return out


def sumsq_ref(i):
    val = _sumsq(i, F64)
    return {"partials": (val, (-(-(i["c"].n // 8) // SUMSQ_STRIDE) * 8 + 1 + 6 + 4 + 2) * U * val)}


OPS["sumsq"] = Op(SUMSQ_CASES, sumsq_inputs, sumsq_ref, lambda i, mut=None: {"partials": _sumsq(i, F32, mut)}, ("no_tail", "drop_last_unroll"))

ClipCase = namedtuple("ClipCase", "name scale max_norm")
CLIP_CASES = [ClipCase("off", 1.0, 0.0), ClipCase("negative", 1.0, -1.0), ClipCase("below", 1.0, 1e4), ClipCase("above", 1.0, 1.0),
              ClipCase("zero_norm", 0.0, 1.0), ClipCase("tiny_norm", 1e-6, 1.0)]
CLIP_EPS = float(np.float32(1e-6))


def clip_inputs(c):
    return dict(c=c, partials=torch.rand(SUMSQ_BLOCKS, generator=_gen(91, len(c.name))) * c.scale ** 2, max_norm=float(np.float32(c.max_norm)))


def clip_ref(i):
    p, mn = i["partials"].double(), i["max_norm"]
    acc = p.sum()
    norm = torch.sqrt(acc)
    dacc = (8 + 6 + 16 + 2) * U * acc
    dnorm = (dacc / (2 * norm) if float(norm) > 0 else torch.zeros(())) + allowance("sqrtf", acc.float().reshape(1)) * 2 * U * norm
    if mn <= 0:
        coef, dcoef = torch.ones((), dtype=F64), -1.0
    else:
        q = mn / (norm + CLIP_EPS)
        dq = q * (dnorm + U * (norm + CLIP_EPS)) / (norm + CLIP_EPS) + U * q
        coef, dcoef = q.clamp(max=1.0), (-1.0 if float(q - dq) > 1.0 else float(dq))
    return {"norm_and_coef": (torch.stack([norm, coef]), torch.stack([dnorm.double().reshape(()), torch.tensor(dcoef, dtype=F64)]))}


def clip_f32(i, mut=None):
    acc, mn = i["partials"].sum(), i["max_norm"]
    norm = acc if mut == "no_sqrt" else torch.sqrt(acc)
    q = torch.tensor(mn, dtype=F32) / (norm + torch.tensor(CLIP_EPS, dtype=F32))
    coef = (q if mut == "unclamped" else q.clamp(max=1.0)) if mn > 0 else torch.ones(())
    return {"norm_and_coef": torch.stack([norm, coef.float()])}


OPS["clip_coef"] = Op(CLIP_CASES, clip_inputs, clip_ref, clip_f32, ("no_sqrt", "unclamped"))


# ------------------------------------------------------------------------------------------------------------- AdamW
AdamCase = namedtuple("AdamCase", "n wd gmul coef zero_grad one_block")
ADAM_STEPS = (1, 2, 3, 100000)
ADAM_CASES = [AdamCase(8, 0.01, 1.0, None, False, False), AdamCase(2048, 0.0, 0.25, 0.37, True, False),
              AdamCase(2056, 0.01, 0.25, None, True, True), AdamCase(8000, 0.0, 1.0, 0.37, False, True),
              AdamCase(8000, 0.01, 1.0, 1.0, True, False), AdamCase(2056, 0.0, 1.0, None, False, False)]
_f = np.float32
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (float(_f(v)) for v in (1e-3, 0.9, 0.999, 1e-8))


def adam_inputs(c):
    g = _gen(100, c.n, int(c.wd * 100), int(c.gmul * 100), c.zero_grad, c.one_block)
    n = c.n
    m0, v0 = 0.01 * torch.randn(n, generator=g), (0.01 * torch.randn(n, generator=g)) ** 2
    grads = [_rb(g, n) for _ in ADAM_STEPS]
    for gr in grads:
        gr[:4] = 0                                            # zero gradient on zero moments: v stays 0, the denominator is eps
        gr[4:8] = (gr[4:8].float() * 2.0 ** -13).to(BF16)     # small gradients: sqrt(v) is of the order of eps
    m0[:4], v0[:4] = 0, 0
    m0[4:8], v0[4:8] = 0, 0
    return dict(c=c, master=torch.randn(n, generator=g), m=m0, v=v0, grads=grads)


def adam_host_scalars(c, step):
    """The fp32 scalars of one launch, recomputed as the C code does, and the relative allowances of the two libm results."""
    b1, b2, t = torch.tensor([ADAM_B1], dtype=F32), torch.tensor([ADAM_B2], dtype=F32), torch.tensor([float(step)], dtype=F32)
    pw1, pw2 = torch.pow(b1, t), torch.pow(b2, t)
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    bc2s = torch.sqrt(bc2)
    a_pow = max(allowance("powf", b1, t), allowance("powf", b2, t))
    a_sqrt = allowance("sqrtf", bc2)
    rel1 = float((a_pow * 2 * U * pw1.double() + U * bc1.double()) / bc1.double())
    rel2 = float((a_pow * 2 * U * pw2.double() + U * bc2.double()) / (2 * bc2.double())) + a_sqrt * 2 * U
    coef = _f(1.0 if c.coef is None else c.coef) * _f(c.gmul)
    return dict(bc1=float(bc1), bc2s=float(bc2s), rel1=rel1, rel2=rel2, coef=float(coef), decay=float(_f(1.0) - _f(ADAM_LR) * _f(c.wd)),
                omb1=float(_f(1.0) - _f(ADAM_B1)), omb2=float(_f(1.0) - _f(ADAM_B2)), step_size=float(_f(ADAM_LR) / _f(float(bc1))))


def adam_step_exact(p, m, v, g, h, eps=ADAM_EPS):
    """One step in float64 from float64 state; ``h``: decay, omb1, omb2, coef, bc2s, step_size (any floats).  -> p', m', v' and
    the intermediate values the bound needs."""
    p1 = p * h["decay"]
    g1 = g * h["coef"]
    m1 = ADAM_B1 * m + h["omb1"] * g1
    v1 = ADAM_B2 * v + h["omb2"] * g1 * g1
    root = torch.sqrt(v1) / h["bc2s"]
    den = root + eps
    upd = h["step_size"] * (m1 / den)
    return p1 - upd, m1, v1, dict(p1=p1, g1=g1, root=root, den=den, upd=upd)


def adam_ref(state, g, c, step):
    """state: the fp32 master / m / v a step starts from (the device's own), g: the bf16 gradient."""
    h = adam_host_scalars(c, step)
    p, m, v, g = state["master"].double(), state["m"].double(), state["v"].double(), g.double()
    p2, m1, v1, w = adam_step_exact(p, m, v, g, h)
    dm = U * ((ADAM_B1 * m).abs() + 2 * (h["omb1"] * w["g1"]).abs() + m1.abs())
    dv = U * ((ADAM_B2 * v).abs() + 4 * (h["omb2"] * w["g1"] ** 2).abs() + v1.abs())
    a_sqrt = allowance("sqrtf", v1.float())
    dden = w["root"] * (dv / (2 * v1.clamp(min=1e-300)) + a_sqrt * 2 * U + U + h["rel2"]) + U * w["den"]
    dupd = w["upd"].abs() * (h["rel1"] + dden / w["den"] + 3 * U) + h["step_size"] * dm / w["den"]
    return {"master": (p2, U * w["p1"].abs() + dupd + U * p2.abs()), "m": (m1, dm), "v": (v1, dv)}


def adam_f32(state, g, c, step, mut=None):
    h = adam_host_scalars(c, step)
    t = lambda x: torch.tensor(x, dtype=F32)                   # noqa: E731
    p, m, v = state["master"].clone(), state["m"].clone(), state["v"].clone()
    g1 = g.float() * t(h["coef"])
    if mut == "coupled":
        g1 = g1 + t(float(_f(c.wd))) * p
    else:
        p = p * t(h["decay"])
    m = t(ADAM_B1) * m + t(h["omb1"]) * g1
    v = t(ADAM_B2) * v + (t(h["omb2"]) * g1) * g1
    bc2s, step_size = (t(1.0), t(ADAM_LR)) if mut == "no_bias_correction" else (t(h["bc2s"]), t(h["step_size"]))
    den = torch.sqrt(v + t(ADAM_EPS)) / bc2s if mut == "eps_inside" else torch.sqrt(v) / bc2s + t(ADAM_EPS)
    p = p - step_size * (m / den)
    return {"master": p, "m": m, "v": v}


ADAM_MUTANTS = ("eps_inside", "coupled", "no_bias_correction")


def split_master(master):
    """fp32 master -> (bf16 working weight rounded half up, low 16 bits): the storage of csm_adamw_step_split."""
    bits = master.contiguous().view(torch.int32).long() & 0xffffffff
    hi = ((bits + 0x8000) >> 16) & 0xffff
    lo = bits & 0xffff
    as16 = lambda x: torch.where(x >= 0x8000, x - 0x10000, x).to(torch.int16)         # noqa: E731
    return as16(hi).view(BF16), as16(lo)


def join_master(param, lo):
    """The fp32 master a split pair stands for: ((hi - (lo >> 15)) << 16) | lo."""
    hi, lo = param.contiguous().view(torch.int16).long() & 0xffff, lo.long() & 0xffff
    bits = (((hi - (lo >> 15)) & 0xffff) << 16) | lo
    return torch.where(bits >= 0x80000000, bits - 0x100000000, bits).to(torch.int32).view(F32)
