"""A float64 reference of the decode-step product kernels (csrc/generate.hip, csrc/quant.hip: csm_gemv_bf16, _ex, _kext,
_kext_rows, csm_gemv_fp8w, csm_gemv_t_bf16, csm_lora_project_bf16, _rows_bf16), a rounding-error bound for every output element,
the memory each launch must leave alone, a restatement of the host dispatch and the seeded cases the two decode-gemv tests
share.  test_decode_gemv_ref_cpu.py proves this module against torch's own float64 machinery, proves that correct fp32
restatements of the kernels' arithmetic fit the bounds and that wrong ones do not; test_decode_gemv_kernels_gpu.py judges the
kernels by it.

Everything is plain torch on the CPU in float64, seeded, the same on every machine, written from the K15 block of
include/csm_hip.h.  The inputs are the kernels' own operands (bf16, e4m3 codes, fp32 scales) cast to float64.

Contracts (x^ = the product's left operand, acc[b][n] = sum_k x^[b][k] W[n][k])
  plain / residual / fp32   y = acc (+ R), one rounding to bf16 or none (fp32 output).  R is [B][ldy]: it shares ldy with y.
  RMSNorm prologue          x^ = bf16(x rstd w), rstd = rsqrt(mean(x^2) + eps), mean over K.
  SwiGLU                    W holds N = 2F interleaved gate / up rows; g = bf16(acc[2i]), u = bf16(acc[2i+1]);
                            y[b][i] = silu(g) u (+ R[b][i]), y is [B][N/2] with ldy.  bf16 output only.
  gather                    x^ row b is row row_index[b] + row_offset of a table with ldx.
  K-extension               acc += sum_j t[b][j] Bx[n][j] (+ bias[n]) BEFORE the epilogue (Bx / bias rows in W's order).  Per row
                            (kext_rows): adapter a = row_adapter[b]; a = -1 or a >= n_adapters is "none" (the plain product);
                            the bias table, or an adapter's entry of it, may be NULL.
  lora_project / _rows      t[b] = bf16(scale x^[b] At), At [K][lda]; rows without an adapter give exact zeros.
  gemv_t                    y = x W with K-major weights W [K][ldw]; bf16 or fp32 output.
  FP8                       y = epilogue(scale[n] sum_k x^[b][k] q[n][k]); q decoded exactly with csm.quant.dequantize_rows_fp8's
                            table; the scale is applied once after the sum and before the epilogue (SwiGLU: before the bf16
                            rounding of g and u).

The judge is ``train_ops_ref.judge``: EVERY element, |got - ref| <= bound; bf16 output: bound = hulp(|ref| + slack) + slack; fp32
output: bound = slack; an element with NEGATIVE slack must equal the reference exactly.  The functions below return ``slack``.

Untouched memory.  Every output lives in a sentinel buffer (train_gemm_ref's): guard rows above and below, with ``pad`` 8 guard
columns (ldy = cols + 8) and a base moved by 8 elements (16 bytes: the alignment the kernels need stays).  The guards carry
slack -1 and the WHOLE buffer is judged.  With ``pad`` the inputs are strided too: ldx = K + 8, ldw = K + 8 (FP8: ldw8 = K + 16),
ld_ext_t = ld_ext_B = kx + 8, lda = kx + 8; every route has contiguous twins (pad = 0).

Bounds.  U = 2^-24.  None is fitted to a kernel's output.
  accumulation   products of two bf16 (or bf16 x e4m3) values are exact in fp32.  A sum of L products in fp32 in ANY order errs by
                 at most (L + 2) UA sum |a b|.  L is counted from the kernels: K + kx products, + 6 for the wave butterfly (VALU
                 kernels, gemv_t: none), + 8 for the eight waves' partials joined in LDS (MFMA kernels, lora_project: 6 + 8).
                 UA = U for the VALU kernels (fmaf / mul + add chains), UA = 2 U for the MFMA kernels for the reason
                 train_gemm_ref gives (the guides do not say how v_mfma_f32_16x16x32_bf16 rounds inside its adder tree).
  one U each     for the FP8 scale, the bias add, the residual add and lora_project's scale (of the result's magnitude).
  SwiGLU         train_gemm_ref.swiglu_fwd on (g, u) with dg = slack(g) + hulp(|g| + slack(g)) and du likewise: the kernel rounds
                 both to bf16 before silu.
  RMSNorm, wide  sum of squares: K products and K + 6 additions of positive terms, relative (K + 8) U; the division and the
                 addition of eps U each; rsqrtf allowance("rsqrtf") ulp (codec_ref measures it against float64 on the CPU):
                 d(rstd) / rstd = ((K + 8) U + 2 U) / 2 + A 2 U.  x rstd w takes two more roundings: delta = |x^| (d(rstd) / rstd
                 + 2 U); then the bf16 rounding: dx^ = hulp(|x^| + delta) + delta, carried as sum_k |W[n][k]| dx^[k].  The wide
                 reference multiplies with the UNROUNDED float64 x^.  This term is most of the wide slack (it is a rounding the
                 kernel is entitled to), so the wide judgement alone cannot see an accumulation error:
  RMSNorm, tight a second reference for every normalised case takes x^ as GIVEN bf16 numbers - the GPU test passes the output
                 of ops.rmsnorm_fwd on the same rows (pinned by test_train_ops_kernels_gpu.py; the gemv prologues promise its
                 arithmetic and order), the CPU proof an fp32 restatement's - and the float64 product of that x^ gets the
                 plain-form bound.  csm_rmsnorm_fwd takes D <= 4096; for K above it (4104, 4608, 8192, 8224) the given x^ is the
                 fp32 restatement's on the CPU and an element may differ from it by one bf16 ulp - but only where the unrounded
                 float64 value lies within 2 delta of a rounding boundary (about one element in 2^12), carried as above.
  SwiGLU, tight  likewise: ``swiglu_tight`` is the float64 SwiGLU of GIVEN bf16 (g, u) - the GPU test passes the output of the
                 same product launched without the SwiGLU epilogue - with train_ops_ref's forward terms (+ R, U).
  integer        operands that are integers in [-8, 8] (FP8: integer codes, power-of-two scales): every product and every sum,
                 in any order, is exact in fp32 (|sum| <= 64 (8192 + 512) < 2^20), so the output must equal RNE-bf16 of the exact
                 value (fp32 output: the exact value) bit for bit: slack -1.

Inputs, three families per case, keyed by ``Case.data_key`` (what is computed, not which kernel computes it)
  random   randn operands, W scaled by 1 / sqrt(K); row scales cycle through 1, 1e-3 (rms ~ 1e-3: eps decides rstd), 30, 1.
  planted  the random inputs + spikes in x (4 x the row's scale; FP8: x max(1, sqrt(K) / 16)) and W (1.0; FP8: code 448; SwiGLU: the up row, and an eighth of
           it in the gate row with the sign that adds + 1/2 to g, so that silu(g) never sleeps through a dropped chunk), one
           per aligned 8-chunk of k in: the first and the last chunk, the chunks on either side of every multiple of 512, the
           chunks of [K - 32, K).  Any single dropped (or duplicated) chunk of those moves some output by about 4 - far above its
           bound (test_decode_gemv_ref_cpu.py proves it for each chunk of each case).
  integer  see above.

Measured utilisation (worst |err| / bound per route on the MI355X over all cases; a record only - no bound is moved towards
it.  A bf16 result whose exact value sits next to a rounding boundary errs by its own half ulp, so 0.99.. is what a correct
kernel shows on bf16 outputs; ``wide`` is small because its slack is mostly the x^ rounding allowance)

  route                      plain forms   wide     tight    (g, u)   (g, u) tight   SwiGLU of given (g, u)
  gemv_reg_kernel            0.9783        0.2894   0.7700   0.8552   0.9126         0.9993
  gemv_regn_kernel           0.9850        0.3911   0.8812   0.9010   0.8773         0.9987
  gemv_kernel                0.9879        0.5562   0.9792   0.9612   0.9884         0.9981
  gemv_mfma_kernel           0.9993        0.7481   0.9844   0.9936   0.9810         0.9999
  gemv_fp8_kernel            0.9971        0.7138   0.9951   0.8400   0.7901         0.9998
  gemv_fp8_mfma_kernel       0.9978        0.7266   0.9871   0.9885   0.9917         0.9997
  lora_project_kernel        0.9985        0.8083   0.9933
  lora_project_rows_kernel   0.9955        0.8422   0.9979
  gemv_t_kernel              0.9999
No guard element changed, every integer case came back bit for bit, every case ran on the kernel ``expected_kernel`` names.
"""
import zlib

import torch

import train_gemm_ref as G
from codec_ref import allowance
from train_ops_ref import EPS, U, hulp, judge, trunc_bf16, utilisation      # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
UA_MFMA = 2 * U
ROW_SCALES = (1.0, 1e-3, 30.0, 1.0)
N_ADAPTERS = 3
ADAPTER_ROWS = (0, 1, -1, N_ADAPTERS, 2)                          # row b's adapter: two real ones, none, out of range (none), a third
T_EXTRA = 5                                                       # rows of a gather table beyond B
ROW_OFFSET = 2
PROJ_SCALE = 1.75                                                 # lora_project's host scalar (exact in fp32)


# ------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One launch.  kind: gemv | fp8 | gemv_t | proj | proj_rows.  ``tag`` keeps a derived launch on another case's operands
    (the SwiGLU cases' product without the epilogue) apart from the table's case of the same shape."""
    D = dict(kind="gemv", B=1, K=0, N=0, res=0, f32=0, norm=0, swiglu=0, gather=0, ext=0, kx=0, bias=0, arot=0, fam="random", pad=1,
             tuning=(), route="", big=False, tag="")

    def __init__(self, name, **kw):
        self.name = name
        for k, v in self.D.items():
            setattr(self, k, kw.pop(k, v))
        assert not kw, kw

    def data_key(self):
        """What the inputs and the reference depend on (not: which kernel computes it)."""
        skip = ("tuning", "route", "big")
        return tuple((k, getattr(self, k)) for k in self.D if k not in skip)

    def with_(self, name, **kw):
        d = {k: getattr(self, k) for k in self.D}
        d.update(kw)
        return Case(name, **d)

    @property
    def no(self):
        """Output columns."""
        return self.kx if self.kind in ("proj", "proj_rows") else (self.N // 2 if self.swiglu else self.N)

    @property
    def mfma(self):
        return self.kind in ("gemv", "fp8") and (self.B > 4 or (self.kind == "gemv" and self.B >= 2 and dict(self.tuning).get(4, 0) and self.K % 32 == 0
                                                               and self.ext != 1))

    def __repr__(self):
        return self.name


def adapters(c):
    """Row b's adapter as the launch passes it."""
    return [ADAPTER_ROWS[(b + c.arot) % len(ADAPTER_ROWS)] for b in range(c.B)]


def live_adapter(a):
    return a if 0 <= a < N_ADAPTERS else -1


def layout(c):
    """The Layout (train_gemm_ref) of the case's one output buffer."""
    dt = F32 if c.f32 else BF16
    return G.Layout(c.B, c.no, c.no + 8 * c.pad, 8 * c.pad, 1, 0, dt)


def strides(c):
    """Leading dimensions of the inputs."""
    p = c.pad
    return dict(ldx=c.K + 8 * p, ldw=(-(-c.N // 8) * 8 + 8 * p) if c.kind == "gemv_t" else (c.K + (16 if c.kind == "fp8" else 8) * p),
                ldt=c.kx + 8 * p, ldb=c.kx + 8 * p, lda=c.kx + 8 * p, ldy=c.no + 8 * p)


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(repr(c.data_key()).encode()) & 0x7FFFFFFF)


def _rb(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def _ri(g, *shape, dtype=BF16):
    return torch.randint(-8, 9, shape, generator=g).to(dtype)


def planted_chunks(K):
    """The aligned 8-chunks of k that carry a spike (see the module docstring)."""
    if K % 8:
        return []
    nc = K // 8
    s = {0, nc - 1}
    for m in range(512, K, 512):
        s.update((m // 8 - 1, m // 8))
    s.update(range(max(0, (K - 32) // 8), nc))
    return sorted(s)


def row_scales(c):
    rot = (c.N + c.K // 8) % 3 if c.B == 1 else 0
    sc = [ROW_SCALES[(b + rot) % 4] for b in range(c.B)]
    if c.fam == "planted" and c.swiglu and not c.norm:            # (silu(g) u ~ g u / 2 ~ 1e-6 on a row of 1e-3: nothing planted would show)
        sc = [1.0 if s == 1e-3 else s for s in sc]
    return sc


def x_rows(c, i):
    """Which rows of i['x'] the batch rows are."""
    return [int(r) + ROW_OFFSET for r in i["row_index"]] if c.gather else list(range(c.B))


def inputs(c):
    """-> dict of the case's operands (CPU; bf16 / uint8 codes / fp32 scales / int32 indices), seeded by the data fields alone.
    Matrices are COMPACT here; the tests lay them out with ``strides``.  'R' is the whole [B][ldy] residual buffer."""
    g = _gen(c)
    i = dict(c=c)
    integer = c.fam == "integer"
    B, K, N = c.B, c.K, c.N
    rows = B + T_EXTRA if c.gather else B
    if c.gather:
        i["row_index"] = torch.randperm(rows - ROW_OFFSET, generator=g)[:B].to(torch.int32)
    xr = x_rows(c, i)
    sc = row_scales(c)
    x = _ri(g, rows, K).float() if integer else torch.randn(rows, K, generator=g)
    if not integer:
        for b, r in enumerate(xr):
            x[r] *= sc[b]
    if c.kind in ("gemv", "fp8"):
        W = _ri(g, N, K).float() if integer else torch.randn(N, K, generator=g) / K ** 0.5
        if c.kind == "fp8" and not integer:
            W *= 1.0 + 0.5 * (torch.arange(N) % 3)[:, None]        # neighbouring rows' scales differ by a quarter at least
        wshape = "nk"
    elif c.kind == "gemv_t":
        W = _ri(g, K, N).float() if integer else torch.randn(K, N, generator=g) / K ** 0.5
        wshape = "kn"
    else:
        na = N_ADAPTERS if c.kind == "proj_rows" else 1
        W = _ri(g, na, K, c.kx).float() if integer else torch.randn(na, K, c.kx, generator=g) / K ** 0.5
        wshape = "akn"
    spike_w = 1.0
    if c.kind == "fp8":
        from csm.quant import quantize_rows_fp8
        if integer:
            i["scale"] = torch.exp2(torch.tensor([float((n * 5) % 3 - 1) for n in range(N)])).float()
            codes = W.to(torch.float8_e4m3fn).view(torch.uint8)
        else:
            codes, i["scale"] = quantize_rows_fp8(W.to(BF16))
        W = codes.view(torch.float8_e4m3fn).float()             # the decoded codes; the scale stays apart
        spike_w = 448.0
    if c.fam == "planted":
        outs = c.no
        xs = 4.0 * (max(1.0, K ** 0.5 / 16) if c.kind == "fp8" else 1.0)      # (FP8: the largest code is the row's amax ~ 4 / sqrt(K))
        for j, ch in enumerate(planted_chunks(K)):
            k, o, sg, sx = ch * 8 + j % 8, j % outs, (-1.0 if j % 3 == 2 else 1.0), (1.0 if j % 2 == 0 else -1.0)
            for b, r in enumerate(xr):
                x[r, k] = xs * sc[b] * sx
            if wshape == "nk" and c.swiglu:                       # the gate takes + 1/2 per spike (silu stays awake), the up row -+ 4
                W[2 * o, k], W[2 * o + 1, k] = sx * spike_w / 8, sg * spike_w
            elif wshape == "nk":
                W[o, k] = sg * spike_w
            elif wshape == "kn":
                W[k, o] = sg
            else:
                W[:, k, o] = sg
    i["x"] = x.to(BF16)
    if c.kind == "fp8":
        i["W8"] = W.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        i["W"] = W.to(BF16)
    if c.norm:
        i["nw"] = (1.0 + 0.5 * torch.randn(K, generator=g)).to(BF16)
        if c.fam == "planted":                                    # (a norm weight near zero must not switch a spike off)
            for j, ch in enumerate(planted_chunks(K)):
                i["nw"][ch * 8 + j % 8] = 1.0
    if c.res:
        ldy = strides(c)["ldy"]
        i["R"] = _ri(g, B, ldy) if integer else _rb(g, B, ldy)
    if c.ext:
        na = N_ADAPTERS if c.ext == 2 else 1
        i["t"] = _ri(g, B, c.kx) if integer else _rb(g, B, c.kx)
        i["Bx"] = _ri(g, na, N, c.kx) if integer else _rb(g, na, N, c.kx, scale=1.0 / (K + c.kx) ** 0.5)
        if c.bias:
            i["bias"] = _ri(g, na, N) if integer else _rb(g, na, N)
            i["bias_null"] = [a == 1 for a in range(na)] if c.ext == 2 else [False]      # adapter 1's entry of the table is NULL
    if c.kind == "proj_rows":
        i["pscale"] = torch.tensor([PROJ_SCALE, 0.5, -1.25]).float()
    return i


# ------------------------------------------------------------------------------------------------------------- reference
def rms_wide(x, w, K, flips=False):
    """-> (x^ unrounded float64, dx^) of rows x [B, K] (float64 of the bf16 operands).  ``flips``: dx^ not against the unrounded
    x^ but against ANOTHER correct fp32 evaluation's bf16 x^ (see RMS_TIGHT_MAX_K): zero, except where the unrounded value lies
    within 2 delta of a bf16 rounding boundary (or rounds to a power of two, where the spacing changes) - there one bf16 ulp."""
    arg = (x * x).sum(1) / K + EPS
    r = 1.0 / torch.sqrt(arg)
    drel = 0.5 * ((K + 8) * U + 2 * U) + allowance("rsqrtf", arg.float()) * 2 * U
    xh = x * r[:, None] * w
    delta = xh.abs() * (drel + 2 * U)
    if not flips:
        return xh, hulp(xh.abs() + delta) + delta
    rd = xh.to(BF16).double()
    h = hulp(rd)
    near = ((h - (xh - rd).abs()).abs() <= 2 * delta) | (rd.abs() == torch.exp2(torch.floor(torch.log2(rd.abs().clamp(min=2.0 ** -126)))))
    return xh, torch.where(near, 2 * hulp(xh.abs() + delta), torch.zeros_like(xh))


RMS_TIGHT_MAX_K = 4096            # csm_rmsnorm_fwd takes D <= 4096: beyond it the tight x^ is ``xhat32`` (fp32 on the CPU) with ``flips``


def acc_len(c):
    """L of the accumulation bound and the unit of one addition, counted from the kernel that takes the case."""
    if c.kind == "gemv_t":
        return c.K, U
    if c.kind in ("proj", "proj_rows"):
        return c.K + 6 + 8, U
    if c.mfma:
        return c.K + c.kx + 8, UA_MFMA
    return c.K + c.kx + 6, U


def _round_exact(v, f32):
    return v if f32 else v.to(BF16).double()                      # (integer family: v is exact in float64, one RNE to bf16)


def swiglu_tight(gu, R=None):
    """SwiGLU of GIVEN bf16 (g, u) interleaved [B, N] (+ R [B, N/2]) -> (value, slack)."""
    v, s = G.swiglu_fwd(gu.double(), torch.zeros(gu.shape, dtype=F64))
    if R is not None:
        v = v + R.double()
        s = s + U * v.abs()
    return v, s


def reference(i, xhat=None, flips=False):
    """-> (value, slack) [B, cols] of the case's output.  ``xhat`` None: x^ from the inputs (normalised cases: the WIDE
    judgement); ``xhat`` bf16 [B, K]: the TIGHT judgement of a normalised case with x^ given - the kernel's own x^ must be those
    bits (``flips`` False: x^ from rmsnorm_fwd_kernel, whose arithmetic and order the prologues promise) or may differ from them
    by one bf16 ulp where two correct fp32 evaluations can round apart (``flips`` True, see ``rms_wide``)."""
    c = i["c"]
    B, K = c.B, c.K
    x = i["x"].double()[x_rows(c, i)]
    dxh = None
    if xhat is not None:
        assert c.norm
        if flips:
            dxh = rms_wide(x, i["nw"].double(), K, flips=True)[1]
        x = xhat.double()
    elif c.norm:
        x, dxh = rms_wide(x, i["nw"].double(), K)
    L, ua = acc_len(c)
    ad = [live_adapter(a) for a in adapters(c)] if (c.ext == 2 or c.kind == "proj_rows") else [0] * B
    if c.kind in ("proj", "proj_rows"):
        val, sl = torch.zeros(B, c.kx, dtype=F64), torch.full((B, c.kx), -1.0, dtype=F64)
        for b in range(B):
            if ad[b] < 0:
                continue                                          # exact zeros
            At = i["W"][ad[b]].double()
            s = float(i["pscale"][ad[b]]) if c.kind == "proj_rows" else PROJ_SCALE
            acc, sabs = x[b] @ At, x[b].abs() @ At.abs()
            e = (L + 2) * ua * sabs + (dxh[b] @ At.abs() if dxh is not None else 0.0)
            val[b] = s * acc
            sl[b] = abs(s) * e + U * val[b].abs()
        if c.fam == "integer":
            return _round_exact(val, False), torch.full_like(sl, -1.0)
        return val, sl
    if c.kind == "gemv_t":
        W = i["W"].double()
        val, sabs = x @ W, x.abs() @ W.abs()
        sl = (L + 2) * ua * sabs
    else:
        W = (i["W8"].view(torch.float8_e4m3fn).float() if c.kind == "fp8" else i["W"]).double()
        val, sabs = x @ W.t(), x.abs() @ W.abs().t()
        wide = dxh @ W.abs().t() if dxh is not None else 0.0
        if c.ext:
            t = i["t"].double()
            for b in range(B):
                if ad[b] < 0:
                    continue
                Bx = i["Bx"][ad[b]].double()
                val[b] = val[b] + t[b] @ Bx.t()
                sabs[b] = sabs[b] + t[b].abs() @ Bx.abs().t()
        sl = (L + 2) * ua * sabs + wide
        if c.kind == "fp8":
            s = i["scale"].double()
            val, sl = val * s, sl * s.abs()
            sl = sl + U * val.abs()
        if c.ext and c.bias:
            for b in range(B):
                if ad[b] >= 0 and not i["bias_null"][ad[b]]:
                    val[b] = val[b] + i["bias"][ad[b]].double()
                    sl[b] = sl[b] + U * val[b].abs()
        if c.swiglu:
            val, sl = G.swiglu_fwd(val, sl + hulp(val.abs() + sl))
    if c.res:
        val = val + i["R"].double()[:, :c.no]
        sl = sl + U * val.abs()
    if c.fam == "integer":
        assert not c.swiglu and not c.norm
        return _round_exact(val, c.f32), torch.full_like(sl, -1.0)
    return val, sl


def embedded(c, val, slack):
    """(reference, slack) of the whole sentinel buffer."""
    return G.embed(layout(c), val, slack)


# ------------------------------------------------------------------------------------------------------------- dispatch
def expected_kernel(c):
    """What csm_gemv_last_kernel() must answer after the case's launch, from gemv_launch, gemv_mfma_launch and csm_gemv_fp8w."""
    tun = dict(c.tuning)
    reg, nt_on, rpw, regn = tun.get(0, 1), tun.get(1, 1), tun.get(2, 1), tun.get(3, 1)
    t = "float" if (c.f32 and not c.swiglu) else "bf16"
    B, K, N, sw = c.B, c.K, c.N, int(bool(c.swiglu))
    if c.kind == "gemv_t":
        return f"gemv_t_kernel<{B}, {t}>"
    if c.kind == "proj":
        return f"lora_project_kernel<{B}>"
    if c.kind == "proj_rows":
        return f"lora_project_rows_kernel<{min(B, 4)}>"
    spw = -(-(-(-K // 64)) // 8)
    seg = 1 if spw <= 1 else 2 if spw <= 2 else 4 if spw <= 4 else 8
    wide = K == 2048 or (K == 8192 and N == 2048)
    if c.kind == "fp8":
        if B > 4:
            return f"gemv_fp8_mfma_kernel<{seg}, {t}, {sw}, {int(wide)}>"
        kc = 1 if K <= 1024 else 2 if K <= 2048 else 8
        return f"gemv_fp8_kernel<{kc}, {B}, {t}, {sw}, {int(wide and kc != 1)}>"
    nt = int(bool(nt_on and wide))
    if c.mfma:
        return f"gemv_mfma_kernel<{seg}, {t}, {sw}, {nt}, ext{c.ext}>"
    if B == 1 and reg and K in (1024, 2048, 8192):
        r = rpw if (sw and K == 1024 and not nt and rpw > 1 and c.no >= 2048) else 1
        return f"gemv_reg_kernel<{K // 512}, {t}, {sw}, {nt}, {2 if r == 2 else 4 if r > 1 else 1}, ext{c.ext}>"
    if B >= 2 and reg and regn and (K in (1024, 2048) or (K == 8192 and not sw and not c.f32)):
        return f"gemv_regn_kernel<{K // 512}, {B}, {t}, {sw}, {int(nt and K != 1024)}, {2 if K == 1024 else 4}, ext{c.ext}>"
    return f"gemv_kernel<{B}, {t}, {sw}, ext{c.ext}>"


def route_of(c):
    return expected_kernel(c).split("<")[0]


def dynamic_lds_bytes(c):
    """Dynamic LDS of the launch (the > 64 KB path sets a function attribute first)."""
    k = route_of(c)
    if k == "gemv_regn_kernel":
        return c.B * c.K * 4
    if k == "gemv_fp8_kernel" and c.B > 1:
        return c.B * (1 if c.K <= 1024 else 2 if c.K <= 2048 else 8) * 1024 * 4
    return c.B * c.K * 2 if k == "gemv_kernel" else 0


# ------------------------------------------------------------------------------------------------------------- restatements
ORDERS = ("lanes", "rev")
MUTANTS = ("chunk", "drop_last32", "trunc", "residual_after_rounding", "gate_up_swapped", "no_eps", "row_offset_ignored", "residual_ld_n",
           "bias_dropped", "adapter_on_none", "scale_next_row")


def applies(mut, c):
    """Which cases a wrong restatement must be caught on (each on at least one element)."""
    prod = c.kind in ("gemv", "fp8")
    # a wrong ROUNDING moves an element by less than a bf16 ulp, and only about every third one beyond half an ulp: it needs a
    # few elements, and an accumulation slack (any order, worst case: ~ K^1.5 U |y|) below half a bf16 ulp (2^-9 |y|): K <= 1024
    many = c.B * c.no >= 16 and c.K + c.kx <= (512 if (c.mfma or c.B > 4) else 1024) and not c.swiglu
    rows_ad = adapters(c) if (c.ext == 2 or c.kind == "proj_rows") else [0] * c.B
    has_none = (c.ext == 2 or c.kind == "proj_rows") and any(live_adapter(a) < 0 for a in rows_ad)
    sc = row_scales(c)
    big_row = bool(c.norm) or any(s >= 1 for s in sc)            # silu(g) u ~ g u / 2 is symmetric in (g, u) on a row of 1e-3
    live_big = any(s >= 1 and live_adapter(a) >= 0 for s, a in zip(sc, rows_ad))
    return {"chunk": c.fam == "planted" and c.K % 8 == 0,
            "drop_last32": c.fam == "planted" and c.K % 64 == 32 and c.kind != "gemv_t",
            "trunc": not c.f32 and c.fam == "random" and many and (live_big or bool(c.norm)) and (c.kind != "proj_rows" or live_big),
            # (integer operands: sums below 256 are exact in bf16 - rounding them first changes nothing; |sum| ~ 27 sqrt(K))
            "residual_after_rounding": bool(c.res) and not c.f32 and many and any(s >= 1 for s in sc) and
            (c.fam == "random" or (c.fam == "integer" and c.K >= 512)),
            "gate_up_swapped": bool(c.swiglu) and big_row,
            "no_eps": bool(c.norm) and any(s == 1e-3 and live_adapter(a) >= 0 for s, a in zip(sc, rows_ad)),
            "row_offset_ignored": bool(c.gather),
            "residual_ld_n": bool(c.res) and c.pad and c.B >= 2,
            "bias_dropped": prod and c.ext and c.bias and any(live_adapter(a) in (0, 2) for a in (adapters(c) if c.ext == 2 else [0])),
            "adapter_on_none": has_none,
            "scale_next_row": c.kind == "fp8"}[mut]


def _bf(t, mut):
    return trunc_bf16(t) if mut == "trunc" else t.to(BF16)


def _sum_chunks(P, order):
    """P [.., C] fp32 partial sums of the 8-chunks of k -> their fp32 sum in one of two orders, neither torch.matmul's:
    'lanes': chunk c on lane c % 64, a lane's chunks in ascending order, then the lanes pairwise; 'rev': one descending chain."""
    C = P.shape[-1]
    if order == "rev":
        acc = torch.zeros(P.shape[:-1], dtype=F32)
        for j in range(C - 1, -1, -1):
            acc = acc + P[..., j]
        return acc
    pad = -C % 64
    Pp = torch.cat([P, torch.zeros(*P.shape[:-1], pad, dtype=F32)], -1).reshape(*P.shape[:-1], -1, 64)
    lanes = torch.zeros(*P.shape[:-1], 64, dtype=F32)
    for j in range(Pp.shape[-2]):
        lanes = lanes + Pp[..., j, :]
    w = 32
    while w >= 1:
        lanes = lanes[..., :w] + lanes[..., w:2 * w]
        w //= 2
    return lanes[..., 0]


def _dot32(x, W, order, mut, chunk):
    """x [B, K] W [N, K] fp32 -> [B, N]: products summed inside 8-chunks, the chunks by ``_sum_chunks``."""
    B, K = x.shape
    if K % 8:
        return (x[:, None, :] * W[None]).flip(-1).cumsum(-1)[..., -1]
    P = (x.reshape(B, 1, K // 8, 8) * W.reshape(1, W.shape[0], K // 8, 8)).sum(-1)
    if mut == "chunk":
        P[..., chunk] = 0
    if mut == "drop_last32":
        P[..., -4:] = 0
    return _sum_chunks(P, order)


def _silu32(g):
    return g * (1.0 / (1.0 + torch.exp(-g)))


def xhat32(i, mut=None, rows=None):
    """The bf16 x^ [B, K] of a normalised case as the prologues compute it, in fp32 (the CPU proof's stand-in for rmsnorm_fwd)."""
    c = i["c"]
    x = i["x"].float()[x_rows(c, i) if rows is None else rows]
    ss = (x * x).sum(1)
    r = torch.rsqrt(ss / c.K + (0.0 if mut == "no_eps" else EPS))
    return _bf(x * r[:, None] * i["nw"].float(), mut)


def restate(i, order="lanes", mut=None, chunk=0):
    """The kernels' arithmetic in fp32 -> the whole sentinel buffer as the launch would leave it.  ``mut``: one of MUTANTS
    (``chunk``: which aligned 8-chunk of k 'chunk' zeroes)."""
    c = i["c"]
    B = c.B
    rows = x_rows(c, i)
    if mut == "row_offset_ignored":
        rows = [r - ROW_OFFSET for r in rows]
    x = i["x"].float()[rows]
    if c.norm:
        x = xhat32(i, mut, rows).float()
    raw = adapters(c) if (c.ext == 2 or c.kind == "proj_rows") else [0] * B
    ad = [(a if 0 <= a < N_ADAPTERS else (0 if mut == "adapter_on_none" else -1)) for a in raw]
    if c.kind in ("proj", "proj_rows"):
        out = torch.zeros(B, c.kx, dtype=F32)
        for b in range(B):
            if ad[b] >= 0:
                s = float(i["pscale"][ad[b]]) if c.kind == "proj_rows" else PROJ_SCALE
                out[b] = torch.tensor(s, dtype=F32) * _dot32(x[b:b + 1], i["W"][ad[b]].float().t().contiguous(), order, mut, chunk)[0]
        return G.place(layout(c), _bf(out, mut))
    if c.kind == "gemv_t":
        v = _dot32(x, i["W"].float().t().contiguous(), order, mut, chunk)
    else:
        W = i["W8"].view(torch.float8_e4m3fn).float() if c.kind == "fp8" else i["W"].float()
        v = _dot32(x, W, order, mut, chunk)
        if c.ext:
            for b in range(B):
                if ad[b] >= 0:
                    v[b] = v[b] + _dot32(i["t"].float()[b:b + 1], i["Bx"][ad[b]].float(), order, None, 0)[0]
        if c.kind == "fp8":
            s = i["scale"].float()
            v = v * (torch.roll(s, -1) if mut == "scale_next_row" else s)
        if c.ext and c.bias and mut != "bias_dropped":
            for b in range(B):
                if ad[b] >= 0 and not i["bias_null"][ad[b]]:
                    v[b] = v[b] + i["bias"][ad[b]].float()
        if c.swiglu:
            g, u = _bf(v[:, 0::2], mut).float(), _bf(v[:, 1::2], mut).float()
            if mut == "gate_up_swapped":
                g, u = u, g
            v = _silu32(g) * u
    if c.res:
        R = i["R"].float()
        R = R.reshape(-1)[:B * c.no].reshape(B, c.no) if mut == "residual_ld_n" else R[:, :c.no]
        v = (v.to(BF16).float() + R) if mut == "residual_after_rounding" else v + R
    return G.place(layout(c), v if c.f32 else _bf(v, mut))


def judge_case(tag, c, got, emb, what=""):
    """Every element of the case's buffer.  ``emb``: embedded(...).  -> worst ratio."""
    worst = judge(tag, got, *emb)
    print(f"RATIO {tag} {worst:.4f} {c.name} {what}")
    return worst


# ------------------------------------------------------------------------------------------------------------- the case table
FORMS = {"plain": {}, "res": dict(res=1), "f32": dict(f32=1), "norm": dict(norm=1), "swiglu": dict(swiglu=1), "gather": dict(gather=1, res=1),
         "all": dict(norm=1, swiglu=1, res=1, gather=1)}
SIX = ("plain", "res", "f32", "norm", "swiglu", "gather")
PLANTED_FORMS = ("plain", "norm", "swiglu")
INTEGER_FORMS = ("plain", "res", "f32", "gather")
EXT_FORMS = {"res_bias": dict(res=1, bias=1), "norm_f32": dict(norm=1, f32=1), "norm_swiglu_bias": dict(norm=1, swiglu=1, bias=1)}


def _cases():
    cs = []

    def add(name, **kw):
        cs.append(Case(name, **kw))

    def forms(prefix, kind, combos, Ns, swNs, names=SIX + ("all",), **kw):
        """combos: (K, [B, ...]); every form at every K, B and N rotating; random always, planted / integer where they apply."""
        for ki, (K, Bs) in enumerate(combos):
            for fi, f in enumerate(names):
                fl = FORMS[f]
                B = Bs[(fi + ki) % len(Bs)]
                N = 2 * swNs[(fi + ki) % len(swNs)] if fl.get("swiglu") else Ns[(fi + ki) % len(Ns)]
                fams = ("random",) + (("planted",) if f in PLANTED_FORMS else ()) + (("integer",) if f in INTEGER_FORMS else ())
                for fam in fams:
                    add(f"{prefix}_K{K}_B{B}_{f}_{fam}", kind=kind, B=B, K=K, N=N, fam=fam, **fl, **kw)
            add(f"{prefix}_K{K}_B{Bs[-1]}_res_contig", kind=kind, B=Bs[-1], K=K, N=Ns[ki % len(Ns)], res=1, pad=0, **kw)

    # gemv_reg_kernel: one row, KCH 2 / 4 / 16
    forms("reg", "gemv", ((1024, [1]), (2048, [1]), (8192, [1])), (6, 9, 22), (5, 9))
    # ... two and four gate / up pairs per wave (key 2): 2050 outputs leave a tail of 2 in the last wave of either
    for r in (2, 4):
        add(f"reg_rpw{r}", B=1, K=1024, N=2 * 2050, norm=1, swiglu=1, tuning=((2, r),))
        add(f"reg_rpw{r}_planted", B=1, K=1024, N=2 * 2050, norm=1, swiglu=1, fam="planted", tuning=((2, r),))
    add("reg_rpw1", B=1, K=1024, N=2 * 2050, norm=1, swiglu=1)    # the same data one pair per wave
    # the three big launches: the non-temporal instantiations at K = 8192 need N = 2048
    add("reg_nt_K8192", B=1, K=8192, N=2048, res=1, big=True)
    add("regn_nt_K8192", B=3, K=8192, N=2048, res=1, big=True)
    add("mfma_nt_K8192", B=5, K=8192, N=2048, res=1, big=True)
    # gemv_regn_kernel: two to four rows; K = 8192 without SwiGLU / fp32 output (B = 3, 4: more than 64 KB of dynamic LDS)
    forms("regn", "gemv", ((1024, [2, 3, 4]), (2048, [3, 4, 2])), (6, 9, 22), (5, 9))
    forms("regn", "gemv", ((8192, [2, 3, 4]),), (6, 9, 22), (5, 9), names=("plain", "res", "norm", "gather"))
    # NT off (key 1) on the K = 2048 cases: the same bits (test_nontemporal_loads_change_nothing)
    for c in [c for c in cs if c.K == 2048 and c.fam == "random"]:
        cs.append(c.with_(c.name + "_nt0", tuning=((1, 0),)))
    # gemv_kernel: every B, K outside the register kernels' three; K = 8192 with SwiGLU / fp32 output at B >= 2
    forms("lds", "gemv", ((8, [1, 2, 3, 4]), (96, [2, 3, 4, 1]), (520, [3, 4, 1, 2]), (1032, [4, 1, 2, 3]), (4104, [1, 3, 2, 4])), (3, 6, 22), (3, 11))
    add("lds_K8192_B2_swiglu", B=2, K=8192, N=2 * 5, swiglu=1)
    add("lds_K8192_B3_f32", B=3, K=8192, N=9, f32=1)
    add("lds_K8192_B4_swiglu_planted", B=4, K=8192, N=2 * 9, swiglu=1, norm=1, fam="planted")
    # ... and the register kernels' cases with key 0 (B = 1) or key 3 (B >= 2) off: gemv_kernel on the same data
    for c in [c for c in cs if c.name.startswith(("reg_K", "regn_K")) and c.K in (1024, 2048) and c.fam != "integer" and not c.tuning]:
        cs.append(c.with_(c.name + "_lds", tuning=((0, 0),) if c.B == 1 else ((3, 0),)))
    # gemv_mfma_kernel SEG 1 / 2 / 4 / 8 (K % 64 == 32: 32, 96, 544, 8224), N % 16 != 0
    forms("mfma", "gemv", ((32, [5, 11, 16]), (96, [11, 16, 5]), (512, [16, 5, 11]), (544, [5, 16, 11]), (1024, [11, 5, 16]), (2048, [16, 11, 5]),
                           (4608, [5, 11, 16]), (8224, [11, 16, 5])), (10, 16, 34), (5, 17))
    for c in [c for c in cs if c.name.startswith("mfma_K2048") and c.fam == "random"]:
        cs.append(c.with_(c.name + "_nt0", tuning=((1, 0),)))
    # ... two and four rows through it (key 4)
    forms("mfma4", "gemv", ((96, [2, 4]), (1024, [4, 2])), (10, 34), (5, 17), names=("res", "norm", "swiglu"), tuning=((4, 1),))
    # GemvExt on the three B <= 4 routes; kx 8 / 40 / 512
    for K, pre in ((1024, "r"), (520, "l")):
        for ei, (en, ef) in enumerate(EXT_FORMS.items()):
            for B in (1, 2, 3, 4):
                kx = (8, 40, 512)[(B + ei) % 3]
                N = (6, 22)[(B + ei) % 2] * (2 if ef.get("swiglu") else 1)
                add(f"ext1{pre}_K{K}_B{B}_{en}_kx{kx}", B=B, K=K, N=N, ext=1, kx=kx, **ef)
                if en == "res_bias":
                    add(f"ext1{pre}_K{K}_B{B}_{en}_kx{kx}_integer", B=B, K=K, N=N, ext=1, kx=kx, fam="integer", **ef)
                if en == "norm_f32":
                    add(f"ext1{pre}_K{K}_B{B}_{en}_kx{kx}_planted", B=B, K=K, N=N, ext=1, kx=kx, fam="planted", **ef)
        add(f"ext1{pre}_K{K}_contig", B=2, K=K, N=22, ext=1, kx=40, res=1, bias=1, pad=0)
    # GemvExtRows on all four routes, adapters mixed per row; bias: the table with one NULL entry, or no table
    for K in (1024, 96):
        for ei, (en, ef) in enumerate(EXT_FORMS.items()):
            for B in (1, 2, 3, 4, 5, 9, 16):
                kx = (8, 40, 512)[(B + ei) % 3]
                N = (10, 34)[(B + ei) % 2] * (2 if ef.get("swiglu") else 1)
                for arot in ((0, 1, 2, 3) if B == 1 else (0,)):
                    add(f"ext2_K{K}_B{B}_{en}_kx{kx}_a{arot}", B=B, K=K, N=N, ext=2, kx=kx, arot=arot, **ef)
                if en == "res_bias":
                    add(f"ext2_K{K}_B{B}_{en}_kx{kx}_integer", B=B, K=K, N=N, ext=2, kx=kx, fam="integer", **ef)
        add(f"ext2_K{K}_B4_contig", B=4, K=K, N=34, ext=2, kx=40, res=1, bias=1, pad=0)
        add(f"ext2_K{K}_B9_contig", B=9, K=K, N=34, ext=2, kx=40, res=1, bias=1, pad=0)
    # lora_project / _rows
    for K in (8, 520, 1024):
        for kx in (8, 40):
            for norm in (0, 1):
                for B in (1, 2, 3, 4):
                    fam = ("random", "planted", "integer")[(B + kx // 8 + norm) % 3] if not norm else ("random", "planted")[B % 2]
                    add(f"proj_K{K}_kx{kx}_n{norm}_B{B}_{fam}", kind="proj", B=B, K=K, kx=kx, norm=norm, fam=fam)
                for B in (1, 5, 16):
                    for arot in ((0, 2) if B == 1 else (0,)):
                        add(f"projrows_K{K}_kx{kx}_n{norm}_B{B}_a{arot}", kind="proj_rows", B=B, K=K, kx=kx, norm=norm, arot=arot,
                            fam="planted" if (B == 5 and K >= 520) else "random")
    add("proj_contig", kind="proj", B=3, K=520, kx=40, pad=0)
    add("projrows_contig", kind="proj_rows", B=5, K=520, kx=40, norm=1, pad=0)
    # gemv_t
    for K in (1, 7, 100):
        for N in (3, 8, 21):
            for B in (1, 2, 3, 4):
                f32 = (B + N) % 2
                add(f"gemvt_K{K}_N{N}_B{B}_{'f32' if f32 else 'bf16'}", kind="gemv_t", B=B, K=K, N=N, f32=f32, fam=("random", "integer")[(B + K) % 2])
    add("gemvt_contig", kind="gemv_t", B=2, K=100, N=21, pad=0)
    # gemv_fp8_kernel KC 1 / 2 / 8 (B = 3, 4 at KC 8: more than 64 KB of dynamic LDS), gemv_fp8_mfma_kernel SEG 1 / 2 / 4 / 8
    forms("fp8", "fp8", ((16, [1, 2, 3, 4]), (528, [2, 3, 4, 1]), (1024, [3, 4, 1, 2]), (2048, [4, 1, 2, 3]), (8192, [1, 3, 4, 2])), (6, 22), (3, 11))
    forms("fp8m", "fp8", ((32, [5, 16]), (96, [16, 5]), (1024, [16, 5]), (2048, [5, 16]), (8192, [16, 5])), (10, 34), (5, 17))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


CASES = _cases()
CASE = {c.name: c for c in CASES}
ROUTES = tuple(dict.fromkeys(route_of(c) for c in CASES))
