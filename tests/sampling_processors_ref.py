"""Reference of the processed rows sampler (``csm_sample_processed_rows``) and the cases its tests share.

One row with penalty r, window w and frame f: n = min(w, f, 64); T = the distinct ids among ring[(f - 1 - j) % 64], j < n, that lie
in [0, V); for t in T  x_t = x_t > 0 ? x_t / r : x_t * r  - one correctly rounded fp32 operation, formed here with torch float32
``/`` and ``*``, so the reference holds the very fp32 numbers the kernel holds.  The penalised row then goes to
``sampling_filters_ref.reference`` and the thresholds come from ``sampling_filters_ref.thresholds`` on the penalised row, so that
module's error bounds and ``HEADROOM`` apply unchanged (tests/test_sampling_processors_ref_cpu.py proves the margins).

The cases: both V, the three input sets and the three kinds of the filters cases, with their temperatures, top-k and group counts,
and per row the penalty / window / frame below - window 0 and frame 0 (n = 0), a frame below the window, n = 64 with the slot read
last and the slot written coinciding, wrap-around, the penalty off (row 10), penalties below 1.  Row r's ring is built from its own
logits (``window_entries``): the argmax, both sides of the top-k boundary, a negative logit, a duplicate and three ids out of
range, then seeded random ids; every slot the window does not reach holds the third-largest logit's id as a poison, so a kernel
that reads past its window picks another winner.
"""
import torch

import sampling_filters_ref as R

HIST = 64
PEN = [1.3, 1.1, 2.0, 1.5, 1.2, 1.05, 3.0, 1.3, 0.8, 1.3, 1.0, 1.3, 1.7, 1.3, 1.15, 0.5]
WINDOW = [1, 2, 8, 16, 32, 64, 64, 64, 5, 64, 64, 0, 33, 64, 64, 7]
FRAME = [1, 5, 8, 100, 31, 64, 65, 200, 3, 127, 50, 40, 1000, 64, 63, 0]
SEED = 2000               # (base 1000 leaves one row's margin at 1.1x its bound)


def depth(r):
    """n of row r: the ring entries its window reaches."""
    return min(WINDOW[r], FRAME[r], HIST)


def window_entries(x, topk, r):
    """Row r's window, newest first (74 entries; the row uses the first ``depth(r)``)."""
    V = x.shape[0]
    order = torch.sort(x, descending=True, stable=True).indices.tolist()
    head = [order[0], order[1], order[topk - 1], order[min(topk, V - 1)], order[V // 2], order[-1], order[0], -1, V, 2 ** 30]
    tail = torch.randint(0, V, (HIST,), generator=torch.Generator().manual_seed(SEED + r)).tolist()
    return head + tail, order[2]


def ring(x, topk, r):
    """Row r's ring, int32 [64]: entry j of the window in slot (FRAME[r] - 1 - j) % 64, the poison everywhere else."""
    entries, poison = window_entries(x, topk, r)
    out = torch.full((HIST,), poison, dtype=torch.int32)
    for j in range(depth(r)):
        out[(FRAME[r] - 1 - j) % HIST] = entries[j]
    return out


def penalised(x, ring_row, penalty, window, frame):
    """The row after step 1, fp32: what the kernel divides by the temperature."""
    x = x.float().clone()
    V = x.shape[0]
    n = min(max(int(window), 0), max(int(frame), 0), HIST)
    rep = torch.tensor(float(penalty), dtype=torch.float32)
    if n == 0 or float(rep) == 1.0:
        return x
    ids = sorted({int(ring_row[(frame - 1 - j) % HIST]) for j in range(n)})
    ids = torch.tensor([t for t in ids if 0 <= t < V], dtype=torch.long)
    if ids.numel():
        x[ids] = torch.where(x[ids] > 0, x[ids] / rep, x[ids] * rep)
    return x


_cases = {}


def cases(V):
    """{(set, kind): dict(x [16, V] (raw), xp [16, V] (penalised), q, topk, temperature, top_p, min_p, penalty, window, frame (lists of
    16), hist int32 [16, 64], ref (16 ``sampling_filters_ref.reference`` results on the penalised rows), raw (the same on the raw
    rows, with the same thresholds: what the draw is without the penalty))}, built once."""
    if V not in _cases:
        sets, q = R.inputs(V)
        out = {}
        for name in R.SETS:
            x = sets[name]
            topk = [k or V for k in R.TOPK_F]
            hist = torch.stack([ring(x[r], topk[r], r) for r in range(R.ROWS)])
            xp = torch.stack([penalised(x[r], hist[r], PEN[r], WINDOW[r], FRAME[r]) for r in range(R.ROWS)])
            for kind in R.KINDS:
                tp, mp = [], []
                for r in range(R.ROWS):
                    n = min(R.GROUPS[r], R.QUANT_CAP) if name == "quant" else R.GROUPS[r]
                    a, b = R.thresholds(xp[r], topk[r], R.TEMP[r], n, kind)
                    tp.append(a)
                    mp.append(b)
                ref = [R.reference(xp[r], topk[r], R.TEMP[r], tp[r], mp[r], q[r]) for r in range(R.ROWS)]
                raw = [R.reference(x[r], topk[r], R.TEMP[r], tp[r], mp[r], q[r]) for r in range(R.ROWS)]
                out[(name, kind)] = dict(x=x, xp=xp, q=q, topk=topk, temperature=R.TEMP, top_p=tp, min_p=mp, penalty=PEN,
                                         window=WINDOW, frame=FRAME, hist=hist, ref=ref, raw=raw)
        _cases[V] = out
    return _cases[V]
