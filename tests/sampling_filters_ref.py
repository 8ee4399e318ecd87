"""Float64 reference of the filtered rows sampler (``csm_sample_filtered_rows``) and the cases its tests share.

One row: logits ``x`` (fp32), ``v = x / temperature`` (the fp32 quotient the kernel forms, then float64), ``e_i = exp(v_i - max v)``.

1. ``K = { i : v_i >= k-th largest v }`` - the set top-k keeps, ties included.
2. ``M = { i in K : e_i >= min_p }`` (p_i >= min_p * p_max); ``min_p = 0``: ``M = K``.
3. ``P_i = e_i / sum_{j in M} e_j``; ``N = { i in M : sum_{j in M, v_j > v_i} P_j < top_p }`` - a token stays while the mass of the
   strictly larger values is below ``top_p``: the token that crosses it is kept, equal values stay or go together, no index
   enters; ``top_p = 1``: ``N = M``.
4. log_softmax -> softmax over ``N``; the winner is ``argmax p_i / q_i``, the lower index on ties.

The kernel's error.  It forms ``e_i`` as ``expf(v_i - max v)`` in fp32 - the difference d_i = max v - v_i is
rounded once (relative 2^-24, which moves e_i by a factor within d_i 2^-24 of one) and ``expf`` is good to one ulp (2^-23) - and
sums mass as integers of quantum 2^-40 (each value truncated: less than one quantum lost per token, the sums exact).  Hence

* ``|e_i(kernel) / e_i - 1| <= (2 + d_i) 2^-24``                                                       (``minp_bound``)
* ``|sum P_j (kernel) - sum P_j| <= 2 (V 2^-40 + (2 + dbar) 2^-24)``, dbar = sum_{j in M} P_j d_j          (``topp_bound``)

(numerator and denominator are each off by at most sum_M e_j (2 + d_j) 2^-24 + V 2^-40, and the denominator is >= 1: the largest
value has e = 1).  A threshold that lies further than this from every token's mass - the margins below - is decided by the kernel
as by this reference.
"""
import math

import numpy as np
import torch

ROWS = 16
VS = (2051, 4096)
SETS = ("drawn", "tied", "quant")
KINDS = ("top_p", "min_p", "both")
TEMP = [0.9, 0.5, 0.8, 0.9, 1.0, 1.3, 0.7, 1.0, 0.25, 2.0, 0.9, 0.9, 1.5, 0.6, 1.1, 0.95]      # tests/test_row_sampling_kernel_gpu.py
TOPK = [1, 2, 12, 50, 64, 65, 200, 2051, 50, 50, 64, 65, 1, 7, 300, 33]                        # (its top-k: the filters-off test)
# the number of distinct-value groups each row's thresholds are built to keep ...
GROUPS = [1, 2, 5, 37, 64, 65, 200, 537, 3, 1500, 11, 167, 900, 2, 300, 33]
# ... out of what this top-k keeps (0: the whole vocabulary - a pure nucleus / min-p request).  Both sides of 64: rows 0, 2, 3,
# 10, 13, 15 filter in the one-wave finish; the others block-wide, and of those rows 4, 8 come down to <= 64 values (the one-wave
# finish after the block-wide filter) while rows 5, 6, 7, 9, 11, 12, 14 stay above (the block-wide finish).
TOPK_F = [50, 0, 12, 50, 0, 0, 300, 0, 65, 0, 50, 200, 0, 2, 0, 64]
QUANT_CAP = 12            # the quantised set has ~60 distinct values per row, the lowest with ~1e-9 of mass: stay in the upper ones
EPS24, QUANTUM = 2.0 ** -24, 2.0 ** -40
HEADROOM = 4.0            # margins must clear the derived bounds by this factor (they are derived, not measured)


def minp_bound(d):
    return (2.0 + d) * EPS24


def topp_bound(V, dbar):
    return 2.0 * (V * QUANTUM + (2.0 + dbar) * EPS24)


def scaled(x, temperature):
    """v as the kernel has it: the fp32 quotient, widened."""
    return (x.float() / torch.tensor(float(temperature), dtype=torch.float32)).double().numpy()


def reference(x, topk, temperature, top_p, min_p, q):
    """One row.  ``top_p`` / ``min_p`` are taken as the fp32 numbers the device arrays hold.  Returns a dict: ``winner``; the bool
    masks ``K``, ``M``, ``N``; ``runner_up`` (winner's p / q over the second's; inf with one kept token); ``topp_margin`` (smallest
    ``|sum_{v_j > v_i} P_j - top_p|`` over i in M; inf at top_p = 1, where step 3 is skipped), ``minp_margin`` (smallest
    ``|e_i / min_p - 1|`` over i in K; inf at min_p = 0), the two bounds for this row, and ``last_kept`` / ``first_dropped``: the
    index lists of the lowest kept value group and of the highest dropped one (empty if nothing is dropped)."""
    v = scaled(x, temperature)
    V = v.shape[0]
    top_p, min_p = float(np.float32(top_p)), float(np.float32(min_p))
    kth = np.sort(v)[V - int(topk)]
    K = v >= kth
    d = v.max() - v
    e = np.exp(-d)
    M = K & (e >= min_p)
    S = e[M].sum()
    vals, inv = np.unique(v[M], return_inverse=True)                     # ascending distinct values of M
    gmass = np.bincount(inv, weights=e[M], minlength=len(vals))
    above_g = np.concatenate([np.cumsum(gmass[::-1])[::-1][1:], [0.0]])  # mass strictly above each group
    above = np.zeros(V)
    above[M] = above_g[inv] / S
    N = M & (above < top_p) if top_p < 1.0 else M.copy()
    assert N[int(np.argmax(v))]
    y = np.where(N, v, -np.inf)
    ls = y - y.max() - math.log(np.exp(y[N] - y.max()).sum())            # log_softmax
    p = np.where(N, np.exp(ls - ls[N].max()), 0.0)
    p = p / p.sum()                                                      # softmax of it
    r = p / q.double().numpy()
    winner = int(np.argmax(r))                                           # (argmax: the first of equal maxima)
    rest = np.delete(r, winner)
    second = rest.max() if rest.size else 0.0
    out = dict(winner=winner, K=K, M=M, N=N, runner_up=(r[winner] / second if second > 0 else math.inf), p=p,
               topp_margin=(float(np.abs(above[M] - top_p).min()) if top_p < 1.0 else math.inf),
               minp_margin=(float(np.abs(e[K] / min_p - 1.0).min()) if min_p > 0.0 else math.inf),
               topp_bound=topp_bound(V, float((e[M] * d[M]).sum() / S)), minp_bound=minp_bound(float(d[K].max())))
    lo = v[N].min()
    out["last_kept"] = np.nonzero(v == lo)[0].tolist()
    out["first_dropped"] = np.nonzero(v == v[~N].max())[0].tolist() if (~N).any() else []
    return out


def thresholds(x, topk, temperature, n, kind):
    """(top_p, min_p) as fp32 numbers that keep ``n`` distinct-value groups of what ``topk`` keeps (fewer if there are not n + 1:
    the boundary must lie between two groups).  ``top_p``: the fp32 midpoint of the masses above group n - 1 and above group n;
    ``min_p``: the geometric midpoint of their e.  kind "both": min_p built for 2n groups, then top_p for n groups of that M."""
    v = scaled(x, temperature)
    kth = np.sort(v)[v.shape[0] - int(topk)]
    e = np.exp(v - v.max())

    def build(mask, n):
        vals = np.unique(v[mask])[::-1]                                  # descending distinct values
        if len(vals) < 2:
            return 0.5, 0.5, 1                                            # one group: any threshold keeps it
        n = max(1, min(n, len(vals) - 1))
        S = e[mask].sum()
        a = e[mask & (v > vals[n - 1])].sum() / S
        b = e[mask & (v > vals[n])].sum() / S
        return float(np.float32((a + b) / 2)), float(np.float32(math.sqrt(math.exp(vals[n - 1] - v.max()) * math.exp(vals[n] - v.max())))), n

    K = v >= kth
    if kind == "top_p":
        return build(K, n)[0], 0.0
    if kind == "min_p":
        return 1.0, build(K, n)[1]
    _, mp, _ = build(K, 2 * n)
    M = K & (e >= float(np.float32(mp)))
    return build(M, n)[0], mp


def inputs(V):
    """The existing kernel test's inputs: seed 48, 16 rows, randn * 2, its three sets and its Exp(1) noise."""
    g = torch.Generator().manual_seed(48)
    lg = torch.randn(ROWS, V, generator=g) * 2
    q = torch.empty(ROWS, V).exponential_(1, generator=g)
    tied = lg.clone()
    tied[:, 100:400] = tied[:, 100:101]
    tied[:8, 100:400] += 3.0
    return {"drawn": lg, "tied": tied, "quant": (lg * 4).round() / 4}, q


_cases = {}


def cases(V):
    """{(set, kind): dict(x [16, V], q, topk, temperature, top_p, min_p (lists of 16), ref (16 ``reference`` results))}, built once."""
    if V not in _cases:
        sets, q = inputs(V)
        out = {}
        for name in SETS:
            for kind in KINDS:
                x = sets[name]
                topk = [k or V for k in TOPK_F]
                tp, mp = [], []
                for r in range(ROWS):
                    n = min(GROUPS[r], QUANT_CAP) if name == "quant" else GROUPS[r]
                    a, b = thresholds(x[r], topk[r], TEMP[r], n, kind)
                    tp.append(a)
                    mp.append(b)
                ref = [reference(x[r], topk[r], TEMP[r], tp[r], mp[r], q[r]) for r in range(ROWS)]
                out[(name, kind)] = dict(x=x, q=q, topk=topk, temperature=TEMP, top_p=tp, min_p=mp, ref=ref)
        _cases[V] = out
    return _cases[V]
