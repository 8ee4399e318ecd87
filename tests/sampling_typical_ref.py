"""Float64 reference of the typical rows sampler (``csm_sample_typical_rows``) and the cases its tests share.

One row goes through: the penalised row (``sampling_processors_ref.penalised``) -> ``sampling_filters_ref.reference`` (its K, M and
N: steps 1 to 3 there) -> locally typical sampling (Meister et al. 2022) on N -> the finish.  With ``v = x / temperature``,
``d_i = max v - v_i`` and ``e_i = exp(-d_i)``:

* ``P_i = e_i / sum_{j in N} e_j`` - the distribution renormalised over N;
* ``h_i = -ln P_i = d_i + ln sum_{j in N} e_j``, ``H = sum_{i in N} P_i h_i``, ``delta_i = |h_i - H|``;
* ``T = { i in N : sum_{j in N, delta_j < delta_i} P_j < typical_p }`` - a token stays while the mass of the strictly more typical
  tokens is below ``typical_p``: the token that crosses it is kept, equal values have equal delta and stay or go together, no index
  enters, and T is never empty (nothing lies below the smallest delta) - but it need not hold the argmax.  ``typical_p = 1``:
  ``T = N``, the processed sampler.
* log_softmax -> softmax over ``T``; the winner is ``argmax p_i / q_i``, the lower index on ties.

The kernel's error.  ``ln sum_N e_j`` is in h_i and in H alike, so ``delta_i = |d_i - D|`` with
``D = sum_N P_i d_i``, and that is what the kernel forms: ``d_i`` is one fp32 subtraction (relative 2^-24 = eps), ``e_i`` is ``expf``
of it (one ulp: with the rounding of d_i, relative (2 + d_i) eps, as in the filters), ``e_i d_i`` one more fp32 product (relative
(4 + d_i) eps with its factors' errors); both are summed as integers of quantum q = 2^-40, each term truncated (less than one quantum
lost per token, the sums exact and independent of their order).  So with D2 = sum_N P_i d_i^2 and sum_N e_j >= 1

* ``|W' - W| <= S ((4 D + D2) eps) + V q`` and ``|S' - S| <= S ((2 + D) eps) + V q`` for W = sum e_i d_i, S = sum e_i, hence
  ``|W'/S' - D| <= a (1 + O(eps))``, ``a = (6 D + D2 + D^2) eps + (1 + D) V q``;
* D is rounded to fp32 once (D eps), d_i carries d_i eps, the last subtraction rounds once more (at most max(d_i, D) eps <= dmax eps,
  dmax the largest d in N):  ``|delta_i (kernel) - delta_i| <= 2 a + (2 dmax + D) eps``, and the gap between two tokens'
  deltas is off by at most twice that                                                                      (``delta_bound``)
* the masses are the nucleus's: ``|sum P_j (kernel) - sum P_j| <= 2 (V q + (2 + D) eps)``  (``mass_bound`` = ``topp_bound(V, D)``)

Why two margins decide T.  Let A be the delta groups before the last kept group B, and C the dropped ones.  (1) If the delta gaps
(B - the group before it) and (first dropped - B) exceed ``delta_bound``, the kernel's deltas still put every token of A
below every token of B below every token of C, and B - one value, so one kernel delta - stays one group.  (2) Then the kernel's
"mass strictly more typical" is at most mass(A) for a token of A or B and at least mass(A + B) for a token of C, whatever the order
inside A or inside C is: flips elsewhere cannot change T.  (3) ``typical_p`` lies further than ``mass_bound`` from mass(A) and from
mass(A + B) = mass(T), so the kernel's integer comparison falls as the exact one does.
"""
import math

import numpy as np

import sampling_filters_ref as R
import sampling_processors_ref as P

KINDS = ("typical", "chain")
SEARCH = 16               # the group count of a case lies within this many delta groups of its target
EPS24, QUANTUM, HEADROOM = R.EPS24, R.QUANTUM, R.HEADROOM
RUNNER_UP = 1.001         # the winner's p / q over the second's: the filters and processors cases' bar


def delta_bound(V, D, D2, dmax):
    a = (6.0 * D + D2 + D * D) * EPS24 + (1.0 + D) * V * QUANTUM
    return 2.0 * (2.0 * a + (2.0 * dmax + D) * EPS24)                  # (a gap: two tokens' errors)


def _groups(v, N):
    """The delta groups of N, most typical first: (delta per token (inf outside N), ascending distinct deltas, each token of N's
    group, the groups' masses, D, D2, dmax)."""
    d = v.max() - v
    e = np.exp(-d)
    S = e[N].sum()
    Pn = e[N] / S
    h = d[N] + math.log(S)
    H = float((Pn * h).sum())
    delta = np.full(v.shape[0], np.inf)
    delta[N] = np.abs(h - H)
    dvals, inv = np.unique(delta[N], return_inverse=True)
    gmass = np.bincount(inv, weights=Pn, minlength=len(dvals))
    return delta, dvals, inv, gmass, float((Pn * d[N]).sum()), float((Pn * d[N] ** 2).sum()), float(d[N].max())


def _margins(dvals, gmass, n, tp):
    """(mass_margin, order_margin) of keeping the first ``n`` delta groups with ``tp``."""
    below = float(gmass[:n - 1].sum())
    mass = tp - below
    order = dvals[n - 1] - dvals[n - 2] if n > 1 else math.inf
    if n < len(dvals):
        mass = min(mass, below + float(gmass[n - 1]) - tp)
        order = min(order, dvals[n] - dvals[n - 1])
    return mass, float(order)


def reference(x, topk, temperature, top_p, min_p, typical_p, q):
    """One row (``x``: the penalised logits).  ``typical_p`` is taken as the fp32 number the device array holds.  Returns
    ``sampling_filters_ref.reference``'s dict for (K, M, N) with ``winner``, ``p`` and ``runner_up`` taken over T, plus ``T``,
    ``last_kept`` / ``first_dropped`` (the index lists of the least typical kept delta group and of the most typical dropped one;
    empty if typical drops nothing), ``single`` (the last kept group holds one distinct value), ``mass_margin`` (the distance of
    ``typical_p`` from the mass below the last kept group and - if anything is dropped - from the mass of T), ``order_margin`` (the
    smaller of the delta gaps around the last kept group), ``mass_bound`` / ``delta_bound``, ``groups`` (delta groups kept) and
    ``drops_argmax``.  At ``typical_p = 1`` the step is skipped: T = N and the margins are inf."""
    out = R.reference(x, topk, temperature, top_p, min_p, q)
    v = R.scaled(x, temperature)
    V = v.shape[0]
    N = out["N"]
    tp = float(np.float32(typical_p))
    delta, dvals, inv, gmass, D, D2, dmax = _groups(v, N)
    out.update(mass_bound=R.topp_bound(V, D), delta_bound=delta_bound(V, D, D2, dmax))
    if tp < 1.0:
        below_g = np.concatenate([[0.0], np.cumsum(gmass)[:-1]])
        below = np.full(V, np.inf)
        below[N] = below_g[inv]
        T = N & (below < tp)
        n = int((below_g < tp).sum())                                    # (a prefix: below_g ascends)
        out["mass_margin"], out["order_margin"] = _margins(dvals, gmass, n, tp)
    else:
        T, n = N.copy(), len(dvals)
        out["mass_margin"], out["order_margin"] = math.inf, math.inf
    assert T.any()
    y = np.where(T, v, -np.inf)
    ls = y - y.max() - math.log(np.exp(y[T] - y.max()).sum())            # log_softmax
    p = np.where(T, np.exp(ls - ls[T].max()), 0.0)
    p = p / p.sum()                                                      # softmax of it
    r = p / q.double().numpy()
    winner = int(np.argmax(r))
    rest = np.delete(r, winner)
    second = rest.max() if rest.size else 0.0
    out.update(winner=winner, p=p, T=T, groups=n, runner_up=(r[winner] / second if second > 0 else math.inf),
               drops_argmax=not bool(T[int(np.argmax(v))]))
    out["last_kept"] = np.nonzero(delta == dvals[n - 1])[0].tolist()
    out["first_dropped"] = np.nonzero(delta == dvals[n])[0].tolist() if n < len(dvals) else []
    out["single"] = len(np.unique(v[out["last_kept"]])) == 1
    return out


def cut(x, topk, temperature, top_p, min_p, target, q):
    """``typical_p`` (an fp32 number) that keeps the number of delta groups nearest ``target``, within ``SEARCH`` of it, whose two
    margins clear ``HEADROOM`` times the bounds and whose winner under ``q`` is decisive (``RUNNER_UP``) - the fp32 midpoint
    between the mass below the last kept group and the mass of T.
    A row whose N is one delta group gets 0.5 (any value keeps it).  Raises if no group count in the range will do."""
    v = R.scaled(x, temperature)
    N = R.reference(x, topk, temperature, top_p, min_p, q)["N"]
    delta, dvals, inv, gmass, D, D2, dmax = _groups(v, N)
    G = len(dvals)
    if G < 2:
        return 0.5
    mb, db = R.topp_bound(v.shape[0], D), delta_bound(v.shape[0], D, D2, dmax)
    cum = np.concatenate([[0.0], np.cumsum(gmass)])
    target = max(1, min(int(target), G - 1))
    for off in sorted(range(-SEARCH, SEARCH + 1), key=lambda o: (abs(o), o)):
        n = target + off
        if not 1 <= n <= G - 1:
            continue
        tp = float(np.float32((cum[n - 1] + cum[n]) / 2))
        if not 0.0 < tp < 1.0:
            continue
        mass, order = _margins(dvals, gmass, n, tp)
        vals = v[N][inv == n - 1]
        if (mass >= HEADROOM * mb and order >= HEADROOM * db and (vals == vals[0]).all()
                and reference(x, topk, temperature, top_p, min_p, tp, q)["runner_up"] >= RUNNER_UP):
            return tp
    raise AssertionError(f"no cut within {SEARCH} delta groups of {target} clears the bounds")


_cases = {}


def cases(V):
    """{(set, kind): dict(x [16, V] (raw), xp (penalised), q, topk, temperature, top_p, min_p, typical_p, penalty, window, frame
    (lists of 16), hist int32 [16, 64], ref (16 ``reference`` results), proc (the same rows at typical_p = 1))}, built once.  Kind
    "typical": top_p 1, min_p 0; "chain": min-p and top-p from ``R.thresholds(.., 2 n, "both")``, then typical for n delta groups
    of that N (n: the filters cases' group targets)."""
    if V not in _cases:
        base = P.cases(V)
        out = {}
        for name in R.SETS:
            c = base[(name, "both")]
            xp, q, topk = c["xp"], c["q"], c["topk"]
            for kind in KINDS:
                tp, mp, yp = [], [], []
                for r in range(R.ROWS):
                    n = min(R.GROUPS[r], R.QUANT_CAP) if name == "quant" else R.GROUPS[r]
                    a, b = (1.0, 0.0) if kind == "typical" else R.thresholds(xp[r], topk[r], R.TEMP[r], 2 * n, "both")
                    tp.append(a)
                    mp.append(b)
                    yp.append(cut(xp[r], topk[r], R.TEMP[r], a, b, n, q[r]))
                ref = [reference(xp[r], topk[r], R.TEMP[r], tp[r], mp[r], yp[r], q[r]) for r in range(R.ROWS)]
                proc = [reference(xp[r], topk[r], R.TEMP[r], tp[r], mp[r], 1.0, q[r]) for r in range(R.ROWS)]
                out[(name, kind)] = dict(x=c["x"], xp=xp, q=q, topk=topk, temperature=R.TEMP, top_p=tp, min_p=mp, typical_p=yp,
                                         penalty=P.PEN, window=P.WINDOW, frame=P.FRAME, hist=c["hist"], ref=ref, proc=proc)
        _cases[V] = out
    return _cases[V]
