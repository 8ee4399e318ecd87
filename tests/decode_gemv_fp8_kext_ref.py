"""A float64 reference of csm_gemv_fp8w_kext_rows (csrc/quant.hip: gemv_fp8_kernel / gemv_fp8_mfma_kernel with the per-row
K-extension pack), a rounding-error bound for every output element and the seeded cases its two tests share.  Everything that is
not new here - the case class, the inputs, the sentinel layouts, the judge, the RMSNorm and SwiGLU treatment - is
decode_gemv_ref's (imported, not copied); test_decode_gemv_fp8_kext_ref_cpu.py proves this module, and
test_decode_gemv_fp8_kext_kernels_gpu.py judges the kernels by it.

Contract (decode_gemv_ref's FP8 line + its K-extension line, the scale on the base sum ONLY):
    y[b][n] = epilogue(scale[n] * sum_k x^[b][k] q[n][k]  +  sum_j t[b][j] Bx[a][n][j]  +  bias[a][n]),   a = row_adapter[b]
a = -1 or a >= n_adapters: no extension and no bias - the row is csm_gemv_fp8w's.  The bias table, or an adapter's entry of it, may
be NULL.  Epilogue: SwiGLU (gate and up each rounded to bf16 AFTER extension and bias), residual, bf16 or fp32 store.

Bounds (U = 2^-24; decode_gemv_ref's accumulation rule: a sum of L exact products in fp32 in any order errs by at most
(L + 2) UA sum |a b|), L counted from the arithmetic quant.hip's header documents:
  VALU kernel, B <= 4   K + kx products, + 6 for the base butterfly, + 6 for the extension's OWN butterfly (the kernel sums the
                        extension's lane partials from zero in a second butterfly and adds the finished sum to the scaled base
                        sum): L = K + kx + 12, UA = U.
  MFMA kernel, B = 5..16  K + kx products (ext_dot: one fmaf per j onto the scaled sum), + 8 for the LDS join: L = K + kx + 8,
                        UA = 2 U (decode_gemv_ref: the MFMA adder tree's rounding is not documented).
  a row without adapter  takes no extension: L = K + 6 / K + 8 - decode_gemv_ref's FP8 bound, unchanged.
  one U each            for the scale (of |scale * base|), the base + extension add, the bias add, the residual add (each of the
                        magnitude of its result).
  The base term carries |scale[n]|: (L + 2) UA (|scale| sum |x^ q| + sum |t Bx|).
  SwiGLU, RMSNorm wide / tight: decode_gemv_ref's, unchanged (the wide x^ allowance rides on the base weights and carries
  |scale|; the extension's t is a given bf16 operand).
  integer               integer codes, power-of-two scales, integer t / Bx / bias in [-8, 8]: every product, scaling and sum is
                        exact in fp32 in any order; the output is RNE-bf16 of the exact value (fp32: the value), slack -1.
None is fitted to a kernel's output.

Families: ``random``; ``planted`` - decode_gemv_ref's FP8 spikes plus one spike pair (t, Bx) per aligned 8-chunk of the
extension (every chunk: the first, the last = chunk kx / 8 - 1, and all between), t = +-4 max(1, sqrt(K) / 16) max(1, row scale),
Bx = +-1 (SwiGLU: the up row, an eighth with the gate-opening sign in the gate row) - a dropped chunk moves an output of every
row that has an adapter by at least 4; ``integer``.

Measured utilisation (worst |err| / bound on the MI355X, a record only): see DESIGN.md, 'FP8 weights'.
"""
import torch

import decode_gemv_ref as D
import train_gemm_ref as G
from decode_gemv_ref import BF16, F32, F64, N_ADAPTERS, U, UA_MFMA, Case, hulp      # noqa: F401

BIAS_NONE, BIAS_ONE_NULL, BIAS_ALL = 0, 1, 2                      # Case.bias: no table / adapter 1's entry NULL / every entry


# ------------------------------------------------------------------------------------------------------------- inputs
def ext_chunks(c):
    """The aligned 8-chunks of the extension: every one carries a spike in the planted family."""
    return list(range(c.kx // 8))


def ext_spike(c, b):
    """|t| of row b's planted extension spikes (exact in bf16 after the cast; what matters is that it is large)."""
    return 4.0 * max(1.0, c.K ** 0.5 / 16) * max(1.0, D.row_scales(c)[b])


def inputs(c):
    """decode_gemv_ref.inputs of the case (kind fp8, ext 2) + the bias table's third form + the planted extension spikes."""
    assert c.kind == "fp8" and c.ext == 2 and c.kx % 8 == 0 and 0 < c.kx <= 512
    i = D.inputs(c)
    if c.bias == BIAS_ALL:
        i["bias_null"] = [False] * N_ADAPTERS
    if c.fam == "planted":
        t, Bx = i["t"].float(), i["Bx"].float()
        for ch in ext_chunks(c):
            j, o, sg, sx = ch * 8 + ch % 8, (ch * 5 + 1) % c.no, (-1.0 if ch % 3 == 2 else 1.0), (1.0 if ch % 2 == 0 else -1.0)
            for b in range(c.B):
                t[b, j] = ext_spike(c, b) * sx
            if c.swiglu:
                Bx[:, 2 * o, j], Bx[:, 2 * o + 1, j] = sx / 8, sg
            else:
                Bx[:, o, j] = sg
        i["t"], i["Bx"] = t.to(BF16), Bx.to(BF16)
    return i


def live_rows(c):
    """Row b's adapter, -1 where it has none."""
    return [D.live_adapter(a) for a in D.adapters(c)]


# ------------------------------------------------------------------------------------------------------------- reference
def acc_len(c, live=True):
    """(L, UA) of a row's accumulation bound, counted from the arithmetic quant.hip documents (module docstring)."""
    kx = c.kx if live else 0
    if c.mfma:
        return c.K + kx + 8, UA_MFMA
    return c.K + kx + 6 + (6 if live else 0), U


def reference(i, xhat=None, flips=False):
    """-> (value, slack) [B, cols], as decode_gemv_ref.reference (``xhat`` / ``flips``: its tight judgement of a normalised case)."""
    c = i["c"]
    B, K = c.B, c.K
    x = i["x"].double()[D.x_rows(c, i)]
    dxh = None
    if xhat is not None:
        assert c.norm
        if flips:
            dxh = D.rms_wide(x, i["nw"].double(), K, flips=True)[1]
        x = xhat.double()
    elif c.norm:
        x, dxh = D.rms_wide(x, i["nw"].double(), K)
    W = i["W8"].view(torch.float8_e4m3fn).float().double()
    s = i["scale"].double()
    base, sabs = (x @ W.t()) * s, (x.abs() @ W.abs().t()) * s.abs()
    wide = (dxh @ W.abs().t()) * s.abs() if dxh is not None else torch.zeros_like(base)
    val, sl = base.clone(), torch.zeros_like(base)
    t = i["t"].double()
    for b, a in enumerate(live_rows(c)):
        L, ua = acc_len(c, a >= 0)
        if a < 0:
            sl[b] = (L + 2) * ua * sabs[b] + wide[b] + U * base[b].abs()
            continue
        Bx = i["Bx"][a].double()
        e, eabs = t[b] @ Bx.t(), t[b].abs() @ Bx.abs().t()
        sl[b] = (L + 2) * ua * (sabs[b] + eabs) + wide[b] + U * base[b].abs()       # the sums, then the scale's rounding
        val[b] = base[b] + e
        sl[b] = sl[b] + U * val[b].abs()                                            # base + extension
        if c.bias and not i["bias_null"][a]:
            val[b] = val[b] + i["bias"][a].double()
            sl[b] = sl[b] + U * val[b].abs()
    if c.swiglu:
        val, sl = G.swiglu_fwd(val, sl + hulp(val.abs() + sl))
    if c.res:
        val = val + i["R"].double()[:, :c.no]
        sl = sl + U * val.abs()
    if c.fam == "integer":
        assert not c.swiglu and not c.norm
        return (val if c.f32 else val.to(BF16).double()), torch.full_like(sl, -1.0)
    return val, sl


def embedded(c, val, slack):
    return G.embed(D.layout(c), val, slack)


# ------------------------------------------------------------------------------------------------------------- dispatch
def expected_kernel(c):
    """csm_gemv_last_kernel() after the case's launch: csm_gemv_fp8w's name with a trailing ext2."""
    k = D.expected_kernel(c)
    assert k.startswith("gemv_fp8_") and k.endswith(">")
    return k[:-1] + ", ext2>"


def route_of(c):
    return expected_kernel(c).split("<")[0]


# ------------------------------------------------------------------------------------------------------------- restatements
MUTANTS = ("ext_chunk", "scale_on_ext", "bias_before_scale", "adapter_of_next_row", "out_of_range_is_adapter_0")


def applies(mut, c):
    """Which cases a wrong restatement must be caught on."""
    raw, live = D.adapters(c), live_rows(c)
    nxt = [live[(b + 1) % c.B] for b in range(c.B)]
    return {"ext_chunk": c.fam == "planted" and any(a >= 0 for a in live),
            # (the planted spikes make the extension large against every bound; scales are 1/4 apart at least from 1, an
            #  integer case's are 1/2, 1, 2: two rows in three move)
            "scale_on_ext": c.fam in ("planted", "integer") and any(a >= 0 for a in live),
            "bias_before_scale": bool(c.bias) and c.fam == "integer" and any(a in (0, 2) or (a == 1 and c.bias == BIAS_ALL) for a in live),
            "adapter_of_next_row": c.B >= 2 and c.fam in ("planted", "integer") and any(a != n for a, n in zip(live, nxt)),
            "out_of_range_is_adapter_0": c.fam in ("planted", "integer") and any(a >= N_ADAPTERS for a in raw)}[mut]


def _ext32(v, t, Bx, onto, order, drop):
    """The extension of one row in fp32.  t [kx], Bx [N, kx], v [N] the scaled base sum.  ``onto`` (MFMA kernel): one fused
    multiply-add per j onto v in ascending j (products of two bf16 are exact in fp32: fmaf is the rounded add).  Otherwise (VALU
    kernel): the extension summed from zero - chunk l on lane l, then the butterfly - and the finished sum added to v."""
    if drop is not None:
        t = t.clone()
        t[8 * drop:8 * drop + 8] = 0
    if onto:
        for j in range(t.numel()):
            v = v + t[j] * Bx[:, j]
        return v
    return v + D._dot32(t[None], Bx, order, None, 0)[0]


def restate(i, order="lanes", mut=None, chunk=0):
    """The documented arithmetic in fp32 -> the whole sentinel buffer as the launch would leave it.  ``mut``: one of MUTANTS
    (``chunk``: the extension chunk 'ext_chunk' drops)."""
    c = i["c"]
    B = c.B
    x = i["x"].float()[D.x_rows(c, i)]
    if c.norm:
        x = D.xhat32(i).float()
    raw = D.adapters(c)
    if mut == "adapter_of_next_row":
        raw = [raw[(b + 1) % B] for b in range(B)]
    ad = [(a if 0 <= a < N_ADAPTERS else (0 if (mut == "out_of_range_is_adapter_0" and a >= N_ADAPTERS) else -1)) for a in raw]
    W = i["W8"].view(torch.float8_e4m3fn).float()
    s = i["scale"].float()
    base = D._dot32(x, W, order, None, 0)
    v = base * s
    for b in range(B):
        a = ad[b]
        if a < 0:
            continue
        bias = i["bias"][a].float() if (c.bias and not i["bias_null"][a]) else None
        t, Bx = i["t"].float()[b], i["Bx"][a].float()
        drop = chunk if mut == "ext_chunk" else None
        if mut == "scale_on_ext":
            r = _ext32(base[b], t, Bx, c.mfma, order, drop) * s
        elif mut == "bias_before_scale" and bias is not None:
            r = _ext32((base[b] + bias) * s, t, Bx, c.mfma, order, drop)
            bias = None
        else:
            r = _ext32(v[b], t, Bx, c.mfma, order, drop)
        v[b] = r if bias is None else r + bias
    if c.swiglu:
        g, u = v[:, 0::2].to(BF16).float(), v[:, 1::2].to(BF16).float()
        v = D._silu32(g) * u
    if c.res:
        v = v + i["R"].float()[:, :c.no]
    return G.place(D.layout(c), v if c.f32 else v.to(BF16))


# ------------------------------------------------------------------------------------------------------------- the case table
KS = (96, 1024, 2048, 8192)                                       # KC 1 (a partial 64-k step) / 1 / 2 (NT) / 8; SEG 1 / 2 / 4 / 8
BS = (1, 2, 3, 4, 5, 16)
KXS = (8, 16, 56, 512)
N_OUT = 302                                                       # 75 blocks of four waves + 2; 18 MFMA tiles + 14 rows
FORMS = {"res": dict(res=1), "f32": dict(f32=1), "norm": dict(norm=1), "swiglu": dict(swiglu=1), "gather": dict(gather=1, res=1),
         "norm_swiglu_res": dict(norm=1, swiglu=1, res=1)}


def _cases():
    cs = []

    def add(name, K, B, form, kx, bias, **kw):
        fl = FORMS[form]
        cs.append(Case(f"{name}_K{K}_B{B}_{form}_kx{kx}_bias{bias}", kind="fp8", ext=2, K=K, B=B, N=2 * N_OUT if fl.get("swiglu") else N_OUT,
                       kx=kx, bias=bias, **fl, **kw))

    names = list(FORMS)
    # random: every K with every B, the forms, kx and the bias table's three shapes rotating against them
    for ki, K in enumerate(KS):
        for bi, B in enumerate(BS):
            add("rand", K, B, names[(bi + ki) % 6], KXS[(bi + 2 * ki + 1) % 4], (bi + ki) % 3)
    # ... every form on both kernels at the two widths of the models' stacks
    for ki, K in enumerate((1024, 2048)):
        for fi, f in enumerate(names):
            add("form", K, (2, 3, 4)[(fi + ki) % 3], f, KXS[(fi + ki) % 4], (fi + ki + 1) % 3, arot=1)
            add("form", K, (5, 16)[(fi + ki) % 2], f, KXS[(fi + ki + 2) % 4], (fi + ki + 2) % 3, arot=1)
    # one row alone: a real adapter, another, none, out of range
    for arot in (1, 2, 3):
        add(f"one_a{arot}", 1024, 1, "res", 16, BIAS_ONE_NULL, arot=arot)
        add(f"one_a{arot}", 2048, 1, "norm_swiglu_res", 56, BIAS_ALL, arot=arot)
    # planted: every extension chunk carries a spike (kx = 512: all 64 lanes)
    for K, B, f, kx, bias in ((96, 2, "res", 512, 1), (96, 16, "swiglu", 512, 0), (1024, 3, "norm", 56, 2), (1024, 5, "res", 16, 1),
                              (2048, 4, "swiglu", 16, 1), (2048, 16, "norm", 56, 0), (8192, 1, "res", 8, 2), (8192, 5, "norm", 8, 1),
                              (1024, 4, "res", 512, 2), (2048, 5, "f32", 512, 1)):
        add("planted", K, B, f, kx, bias, fam="planted")
    # integer: bit for bit
    for K, B, f, kx, bias in ((96, 4, "res", 56, 1), (96, 5, "f32", 8, 2), (1024, 1, "gather", 512, 2), (1024, 16, "res", 16, 1),
                              (2048, 3, "f32", 16, 2), (2048, 16, "gather", 512, 0), (8192, 2, "res", 8, 1), (8192, 5, "res", 56, 2),
                              (1024, 4, "gather", 8, 1), (2048, 5, "res", 56, 1)):
        add("integer", K, B, f, kx, bias, fam="integer")
    # contiguous twins on both routes
    add("contig", 1024, 4, "res", 56, 1, pad=0)
    add("contig", 2048, 1, "norm_swiglu_res", 16, 2, pad=0)
    add("contig", 96, 5, "res", 56, 1, pad=0)
    add("contig", 2048, 16, "norm_swiglu_res", 512, 1, pad=0)
    ns = [c.name for c in cs]
    assert len(set(ns)) == len(ns), [n for n in ns if ns.count(n) > 1]
    return cs


CASES = _cases()
CASE = {c.name: c for c in CASES}
ROUTES = tuple(dict.fromkeys(route_of(c) for c in CASES))
