"""Float64 reference of ``csm_sample_stats_rows`` (csrc/generate.hip), a rounding-error bound per output and the seeded cases its
tests share (test_sample_stats_ref_cpu.py proves this module against torch's float64 ``log_softmax``;
test_sample_stats_kernel_gpu.py judges the kernel by it, test_gen_stats_gpu.py the generated frames).

One row: x (V fp32 logits, cast to float64: the exact operation on the kernel's own operands) and a code c.  With m = max x,
d_i = x_i - m <= 0, e_i = exp(d_i), S = sum e_i and A = sum e_i d_i (a column at -inf adds nothing):

    logprob = d_c - ln S  (-inf for c outside [0, V)),   entropy = ln S - A / S,   pmax = 1 / S.

Bounds.  U = 2^-24, TINY = 2^-126 (a result below the normal range may be flushed or denormal: at most TINY off).  The kernel's
steps, each with the error it is allowed - counted from the operations, none fitted to the kernel's output:

  d_i      one fp32 subtraction of exact operands (the max of fp32 values is exact): |d_i| U.
  e_i      expf: Ae ulp of its value (``codec_ref.allowance("expf", d)``: 4 x the worst error of torch's fp32 CPU exp against
           float64 on the case's own d, never below 2 ulp) = 2 Ae U relative, plus the argument's error carried through exp:
           eps_i = (2 Ae + |d_i|) U relative, + TINY absolute.
  S        V terms added in fp32 in any order: (V + 2) U S on top of the terms' own errors:
           dS = sum e_i eps_i + V TINY + (V + 2) U S.
  ln S     logf: Al ulp of its value (``allowance("logf", S)``, measured the same way), and S's error through ln:
           dln = dS / S + 2 Al U |ln S|.
  logprob  d_c's rounding, dln and the last subtraction's rounding: |d_c| U + dln + U |logprob|.
  A        each term e_i d_i: eps_i, d_i's rounding and the product's (fused or not): eps_i + 2 U relative, + |d_i| TINY; V terms
           added: dA = sum |e_i d_i| (eps_i + 2 U) + sum |d_i| TINY + (V + 2) U |A|.
  entropy  dln + dA / S + |A| / S * dS / S + U |A / S| (the division) + U |entropy| (the subtraction).
  pmax     dS / S^2 + U / S (the division).

All are first-order; the products of two such terms are below 2^-11 of them at V <= 4096 and are covered by HIGHER = 1.01.
The chain lengths are the row's V although the kernel's longest chain is 16 + 6 + 3 additions: the bound holds for any order.

Untouched memory.  The logits sit in a NaN-filled buffer - GR guard rows above and below, columns V .. ldl-1 of every row - so a
kernel that reads one element too many returns NaN, which no bound admits.  Every output lives in ``train_gemm_ref``'s sentinel
buffer (guard rows above and below) and the WHOLE buffer is judged by ``train_ops_ref.judge``: the guards must come back bit for
bit.  A row whose code lies outside [0, V) must hold exactly -inf; ``judge_outputs`` checks that and then judges the rest.

Worst |err| / bound of the kernel over all 27 cases (MI355X, test_sample_stats_kernel_gpu.py, 2026-10-21): logprob 0.6248
(V65_ldl67_rows512; 0.09 at V >= 2051, where (V + 2) U S dominates the bound), entropy 0.1363 and pmax 0.1690 (both
V2_ldl2_rows512).  RECORD below holds the same figures.
"""
import math

import torch

import train_gemm_ref as G
from codec_ref import allowance
from train_ops_ref import judge

U = 2.0 ** -24
TINY = 2.0 ** -126
HIGHER = 1.01
F64, F32 = torch.float64, torch.float32
GR = G.GR
OUTPUTS = ("logprob", "entropy", "pmax")
# (from the GPU run of test_sample_stats_kernel_gpu.py; the tests do not read it)
RECORD = {"logprob": 0.6248, "entropy": 0.1363, "pmax": 0.1690}

# V -> ldl: 2051 in 2112 columns is the model's padded vocabulary; 2304 / 2305 straddle the two register tilings (9 / 16 per thread)
SHAPES = ((1, 4), (2, 2), (63, 64), (64, 72), (65, 67), (2051, 2112), (2304, 2305), (2305, 2308), (4096, 4100))
ROWS = (1, 3, 512)
KINDS = ("randn", "plus80", "minus80", "mixed", "onehot", "const")
CODES = ("first", "last", "minus1", "V", "random")


def reference(x32, codes):
    """``x32`` fp32 [rows, V], ``codes`` int [rows] -> {name: (value float64 [rows], bound float64 [rows])}.  ``logprob`` of a code
    outside [0, V) is -inf with bound 0."""
    x = x32.detach().cpu().to(F64)
    rows, V = x.shape
    codes = torch.as_tensor(codes).long().reshape(rows)
    m = x.max(1, keepdim=True).values
    d = x - m
    e = torch.exp(d)
    t = torch.where(e > 0, e * d, torch.zeros_like(e))
    S, A = e.sum(1), t.sum(1)
    lnS = torch.log(S)
    inside = (codes >= 0) & (codes < V)
    dc = d.gather(1, codes.clamp(0, V - 1).view(-1, 1)).view(-1)
    lp = torch.where(inside, dc - lnS, torch.full_like(lnS, -math.inf))
    ent = lnS - A / S
    pm = 1.0 / S
    dfin = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    Ae = allowance("expf", dfin.float())
    Al = allowance("logf", S.float())
    eps = (2.0 * Ae + dfin.abs()) * U
    dS = (e * eps).sum(1) + V * TINY + (V + 2) * U * S
    dln = dS / S + 2.0 * Al * U * lnS.abs()
    b_lp = torch.where(inside, dc.abs() * U + dln + U * torch.where(inside, lp, torch.zeros_like(lp)).abs(), torch.zeros_like(lnS))
    dA = (t.abs() * (eps + 2.0 * U)).sum(1) + dfin.abs().sum(1) * TINY + (V + 2) * U * A.abs()
    b_ent = dln + dA / S + A.abs() / S * dS / S + U * (A / S).abs() + U * ent.abs()
    b_pm = dS / S ** 2 + U / S
    return {"logprob": (lp, HIGHER * b_lp), "entropy": (ent, HIGHER * b_ent), "pmax": (pm, HIGHER * b_pm)}


# ------------------------------------------------------------------------------------------------------------------ cases
def _gen(*xs):
    s = 4242
    for x in xs:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def make_rows(V, rows, shift=0):
    """(x fp32 [rows, V], codes int32 [rows], kinds, code kinds): row r is of kind ``KINDS[(r + shift) % 6]`` with a code of
    kind ``CODES[(7 r + shift) % 5]`` - 512 rows hold every pair.  A one-hot row's "random" code is its hot column."""
    g = _gen(V, rows, shift)
    x = torch.empty(rows, V, dtype=F32)
    codes = torch.empty(rows, dtype=torch.int32)
    kinds, ckinds = [], []
    for r in range(rows):
        kind, ck = KINDS[(r + shift) % len(KINDS)], CODES[(7 * r + shift) % len(CODES)]
        z = torch.randn(V, generator=g)
        hot = int(torch.randint(V, (1,), generator=g))
        if kind == "randn":
            x[r] = 3.0 * z
        elif kind == "plus80":
            x[r] = 80.0 + 4.0 * z
        elif kind == "minus80":
            x[r] = -80.0 + 4.0 * z
        elif kind == "mixed":
            x[r] = torch.where(torch.rand(V, generator=g) < 0.5, 80.0, -80.0) + z
        elif kind == "onehot":
            x[r] = -80.0
            x[r, hot] = 80.0
        else:
            x[r] = 3.25
        codes[r] = {"first": 0, "last": V - 1, "minus1": -1, "V": V, "random": hot}[ck]
        kinds.append(kind)
        ckinds.append(ck)
    return x, codes, kinds, ckinds


class Case:
    def __init__(self, V, ldl, rows, shift):
        self.V, self.ldl, self.rows, self.shift = V, ldl, rows, shift
        self.name = f"V{V}_ldl{ldl}_rows{rows}"
        self._made = None

    def __repr__(self):
        return self.name

    @property
    def made(self):
        """Built once: x, codes, kinds, the reference, the NaN-framed logits buffer and the outputs' layout."""
        if self._made is None:
            x, codes, kinds, ckinds = make_rows(self.V, self.rows, self.shift)
            buf = torch.full((self.rows + 2 * GR, self.ldl), math.nan, dtype=F32)
            buf[GR:GR + self.rows, :self.V] = x
            lay = G.Layout(self.rows, 1, 1, 0, 1, self.rows, F32)
            self._made = dict(x=x, codes=codes, kinds=kinds, ckinds=ckinds, ref=reference(x, codes), logits=buf, layout=lay)
        return self._made


CASES = [Case(V, ldl, rows, i) for i, (V, ldl) in enumerate(SHAPES) for rows in ROWS]
CASE = {c.name: c for c in CASES}


def logits_window(buf, c):
    """The [rows, V] window (row stride ldl) of a case's NaN-framed logits buffer, on whatever device ``buf`` is."""
    return buf[GR:GR + c.rows, :c.V]


def output_buffers(c, device="cpu"):
    """{name: a fresh sentinel buffer}; ``window`` gives the [rows] part a launch writes."""
    return {n: G.sentinel_buffer(c.made["layout"]).to(device) for n in OUTPUTS}


def window(flat, c):
    return G.view(flat, c.made["layout"]).view(-1)


def judge_outputs(c, got, names=OUTPUTS, what=""):
    """``got``: {name: the WHOLE sentinel buffer after the launch}.  -> {name: worst |err| / bound}."""
    m = c.made
    worst = {}
    for n in names:
        val, bound = m["ref"][n]
        g = got[n].detach().cpu().clone()
        if n == "logprob":
            bad = ~torch.isfinite(val)
            gw = window(g, c)
            assert bool((gw[bad] == -math.inf).all()), f"{c}{what}: a code outside [0, V) must give logprob = -inf, got {gw[bad].tolist()[:4]}"
            gw[bad] = 0.0                                              # (judged above: exact)
            val = torch.where(bad, torch.zeros_like(val), val)
            bound = torch.where(bad, torch.full_like(bound, -1.0), bound)
        ref, slack = G.embed(m["layout"], val, bound)
        worst[n] = judge(f"sample_stats.{n} {c}{what}", g, ref, slack)
    return worst


# ------------------------------------------------------------------------------------------------- fp32 restatements (CPU)
MUTANTS = ("no_max", "entropy_of_code", "reads_padding")


def restate(c, mut=None):
    """The kernel's arithmetic in torch fp32 on the CPU, as the launch would leave the three sentinel buffers.  ``mut``: one of
    MUTANTS - no max subtraction; the entropy formed from the drawn code alone (-p_c ln p_c); the sums run over all ldl columns."""
    m = c.made
    x = logits_window(m["logits"], c) if mut != "reads_padding" else m["logits"][GR:GR + c.rows]
    codes = m["codes"].long()
    mx = x.max(1, keepdim=True).values if mut != "no_max" else torch.zeros(c.rows, 1)
    d = x - mx
    e = torch.exp(d)
    S = e.sum(1)
    A = torch.where(e > 0, e * d, torch.zeros_like(e)).sum(1)
    lnS = torch.log(S)
    inside = (codes >= 0) & (codes < c.V)
    dc = d.gather(1, codes.clamp(0, c.V - 1).view(-1, 1)).view(-1)
    lp = torch.where(inside, dc - lnS, torch.full_like(lnS, -math.inf))
    ent = lnS - A / S
    if mut == "entropy_of_code":
        ent = torch.where(inside, -torch.exp(lp) * lp, torch.zeros_like(lp))
    out = {"logprob": lp, "entropy": ent, "pmax": 1.0 / S}
    return {n: G.place(m["layout"], v.float()) for n, v in out.items()}
