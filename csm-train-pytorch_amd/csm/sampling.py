"""Sampling parameters, host side: the rules a value is held to (``check_*``), the one normaliser of what a call names
(``normalise``) and the per-row state of a ``DecodeState`` (``RowSampler``).

A state samples at one of five levels, and the level only rises: 0 - the scalar path, two numbers per frame call
(``csm_sample_topk``); 1 - each row its own temperature / top-k (``csm_sample_topk_rows``); 2 - and its own top-p / min-p
(``csm_sample_filtered_rows``); 3 - all six per row and per codebook, with the windowed repetition penalty and the rows' rings of
sampled codes (``csm_sample_processed_rows``); 4 - and locally typical sampling, ``typical_p`` per row and per codebook
(``csm_sample_typical_rows``).  Whatever the level, the parameters sit in the same six [K, B] device buffers
(codebook-major: codebook i's draw hands row i of each to the kernel, which reads ``topk[row]`` from the pointer it is given) and
in one host mirror; below level 3 the K entries of a column are equal.  Level 4's seventh buffer and mirror stand beside them.
"""
import math
import numbers

import torch

HIST_FRAMES = 64        # SMP_HIST of csrc/generate.hip: the frames a row's ring of sampled codes holds, per codebook
PROCESSOR_NAMES = ("temperature", "topk", "top_p", "min_p", "repetition_penalty", "repetition_window")
DTYPES = (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32)
# what a parameter is before a write names it: no nucleus, no min-p cut, no penalty (the pair's placeholders are never read - the
# first write brings a pair)
IDENTITY = (1.0, 1, 1.0, 0.0, 1.0, HIST_FRAMES)
_FIRST = (None, "temperature = topk = None samples each row with its own pair: call set_row_sampling first",
          "no row filters: call set_row_filters first", "no row processors: call set_row_processors first",
          "no row typical sampling: call set_row_typical first")


def _is_number(x):
    """One value for all rows: a real number, or a 0-d tensor / array of one (what ``float()`` / ``int()`` take)."""
    return (isinstance(x, numbers.Real) and not isinstance(x, bool)) or getattr(x, "ndim", None) == 0


def _as_list(x):
    """A sequence of per-row values (list / tuple / 1-D tensor or array) as a list; None for anything else."""
    if isinstance(x, (str, bytes)) or x is None:
        return None
    if hasattr(x, "tolist"):
        x = x.tolist()
    return list(x) if isinstance(x, (list, tuple)) else None


def check_sampling(temperature, topk, vocab):
    """The rule for one row's sampling parameters: ``temperature`` a finite number > 0, ``topk`` an integer in 1..vocab (the
    audio vocabulary).  Returns (float, int); raises ValueError with the offending value."""
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        t = float("nan")
    if isinstance(temperature, bool) or not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    try:
        k = int(topk)
        whole = not isinstance(topk, bool) and k == topk
    except (TypeError, ValueError, OverflowError):
        k, whole = 0, False
    if not whole or not 1 <= k <= int(vocab):
        raise ValueError(f"topk must be an integer in 1..{int(vocab)} (the audio vocabulary), got {topk!r}")
    return t, k


def check_filters(top_p, min_p):
    """The rule for one row's sampling filters: ``top_p`` a number in (0, 1] (1: no nucleus cut), ``min_p`` a number in [0, 1]
    (0: no min-p cut).  Returns (float, float); raises ValueError with the offending value."""
    out = []
    for name, v, ok, rule in (("top_p", top_p, lambda f: 0.0 < f <= 1.0, "in (0, 1]"),
                              ("min_p", min_p, lambda f: 0.0 <= f <= 1.0, "in [0, 1]")):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if isinstance(v, (bool, str, bytes)) or not ok(f):
            raise ValueError(f"{name} must be a number {rule}, got {v!r}")
        out.append(f)
    return out[0], out[1]


def check_processors(repetition_penalty, repetition_window):
    """The rule for one row's repetition penalty: ``repetition_penalty`` a finite number with 0 < r <= 100 (1: off; above 1 a
    code of the window becomes less likely, below 1 more), ``repetition_window`` an integer in 0..64 (the most recent frames
    looked at; 0: off).  Returns (float, int); raises ValueError with the offending value."""
    try:
        r = float(repetition_penalty)
    except (TypeError, ValueError):
        r = float("nan")
    if isinstance(repetition_penalty, (bool, str, bytes)) or not (math.isfinite(r) and 0.0 < r <= 100.0):
        raise ValueError(f"repetition_penalty must be a finite number with 0 < r <= 100, got {repetition_penalty!r}")
    try:
        w = int(repetition_window)
        whole = not isinstance(repetition_window, (bool, str, bytes)) and w == repetition_window
    except (TypeError, ValueError, OverflowError):
        w, whole = 0, False
    if not whole or not 0 <= w <= HIST_FRAMES:
        raise ValueError(f"repetition_window must be an integer in 0..{HIST_FRAMES} (frames), got {repetition_window!r}")
    return r, w


def check_typical(typical_p):
    """The rule for one row's locally typical sampling: ``typical_p`` a number in (0, 1] (1: off).  Returns a float; raises
    ValueError with the offending value."""
    try:
        f = float(typical_p)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(typical_p, (bool, str, bytes)) or not 0.0 < f <= 1.0:
        raise ValueError(f"typical_p must be a number in (0, 1], got {typical_p!r}")
    return f


def per_codebook(name, value, K):
    """``value`` - a number (every codebook) or a sequence of K numbers (one per codebook) - as a list of K entries."""
    if _is_number(value):
        return [value] * K
    vs = _as_list(value)
    if vs is None or len(vs) != K or not all(_is_number(v) for v in vs):
        raise ValueError(f"{name} is a number or a sequence of one number per codebook ({K} codebooks), got {value!r}")
    return vs


def check_row_processors(K, vocab, temperature, topk, top_p, min_p, repetition_penalty, repetition_window):
    """One row's six sampling parameters, each a number or K numbers, held to ``check_sampling`` / ``check_filters`` /
    ``check_processors`` codebook by codebook.  Returns six tuples of K values (floats; ints for topk and the window)."""
    cols = [per_codebook(n, v, K) for n, v in zip(PROCESSOR_NAMES, (temperature, topk, top_p, min_p, repetition_penalty,
                                                                     repetition_window))]
    out = [[] for _ in cols]
    for i in range(K):
        vals = (check_sampling(cols[0][i], cols[1][i], vocab) + check_filters(cols[2][i], cols[3][i])
                + check_processors(cols[4][i], cols[5][i]))
        for o, v in zip(out, vals):
            o.append(v)
    return tuple(tuple(o) for o in out)


def check_row_typical(K, typical_p):
    """One row's ``typical_p``, a number or K numbers, held to ``check_typical`` codebook by codebook: a tuple of K floats."""
    return tuple(check_typical(v) for v in per_codebook("typical_p", typical_p, K))


def names_processors(*values, repetition_penalty=None, repetition_window=None):
    """Whether a call names what only the processed sampler has: a penalty, a window, or a per-codebook sequence among
    ``values`` (each a number, None, a flat sequence of numbers - per row, today's meaning - or a sequence holding sequences)."""
    if repetition_penalty is not None or repetition_window is not None:
        return True
    for v in values:
        vs = _as_list(v)
        if vs is not None and any(_as_list(x) is not None for x in vs):
            return True
    return False


def normalise(B, K, vocab, temperature, topk, top_p=None, min_p=None, repetition_penalty=None, repetition_window=None, *,
              level=0, unit="row", typical_p=None):
    """What a frame call's six sampling values ask for: (the level the call needs, per row six entries - a tuple of K validated
    values each, or None for a parameter the call leaves as it is).  Level 0: two numbers, or None for both - the call passes them
    through and writes nothing (no rows come back).  Each value is None (not named), a number (every row) or B entries; at level 3
    an entry is a number or K numbers, one per codebook.  Level 1 (a sequence in the pair) writes the pair; level 2 (``top_p`` /
    ``min_p`` named) the filters - the one not named at its identity - and the pair, unless both are None; level 3 (a penalty, a
    window or a per-codebook entry named, or anything beyond a plain pair on a state whose ``level`` is 3: it draws every rows
    frame through the processors) all six, those not named at their identity.  Everything is checked here, so the caller writes
    all rows or none.  Level 4 (``typical_p`` named - a number, B entries, or per entry K numbers - or anything beyond a plain
    pair on a state whose ``level`` is 4): rows of SEVEN entries, the six of level 3 and ``typical_p`` (1.0 if not named).
    ``unit``: what the errors call a row ("utterance": the generator's calls, checked before any cache is taken
    over)."""
    many = f"{B} rows" if unit == "row" else f"{B}"

    def rows_of(v, what):
        vs = [v] * B if _is_number(v) else _as_list(v)
        if vs is None or len(vs) != B:
            raise ValueError(what)
        return vs

    plain = (temperature is None and topk is None) or (_is_number(temperature) and _is_number(topk))
    if typical_p is not None or (level == 4 and not (plain and top_p is None and min_p is None and repetition_penalty is None
                                                      and repetition_window is None)):
        if temperature is None or topk is None:
            raise ValueError("typical_p, per-codebook parameters and the repetition penalty need temperature and topk named")
        seven = [ident if v is None else v for ident, v in zip(IDENTITY + (1.0,), (temperature, topk, top_p, min_p, repetition_penalty,
                                                                                   repetition_window, typical_p))]
        cols = [rows_of(v, f"{name} is a number or a sequence of one entry per {unit} ({many}; an entry is a number or one number "
                           f"per codebook), got {v!r}") for name, v in zip(PROCESSOR_NAMES + ("typical_p",), seven)]
        return 4, [check_row_processors(K, vocab, *[vs[b] for vs in cols[:6]]) + (check_row_typical(K, cols[6][b]),)
                   for b in range(B)]
    if names_processors(temperature, topk, top_p, min_p, repetition_penalty=repetition_penalty,
                        repetition_window=repetition_window) or (level == 3 and not (plain and top_p is None and min_p is None)):
        if temperature is None or topk is None:
            raise ValueError("per-codebook parameters and the repetition penalty need temperature and topk named")
        six = [IDENTITY[j] if v is None else v
               for j, v in enumerate((temperature, topk, top_p, min_p, repetition_penalty, repetition_window))]
        cols = [rows_of(v, f"{name} is a number or a sequence of one entry per {unit} ({many}; an entry is a number or one number "
                           f"per codebook), got {v!r}") for name, v in zip(PROCESSOR_NAMES, six)]
        return 3, [check_row_processors(K, vocab, *[vs[b] for vs in cols]) for b in range(B)]
    if top_p is None and min_p is None:
        if plain:
            return 0, None
        filters = [(None, None)] * B
    else:
        what = (f"top_p and min_p are numbers or sequences of one value per {unit} ({many}): got top_p={top_p!r}, "
                f"min_p={min_p!r}")
        ps, ms = rows_of(1.0 if top_p is None else top_p, what), rows_of(0.0 if min_p is None else min_p, what)
        filters = [tuple((v,) * K for v in check_filters(p, m)) for p, m in zip(ps, ms)]
    if temperature is None and topk is None:
        pairs = [(None, None)] * B
    else:
        what = (f"temperature and topk are numbers or sequences of one value per {unit} ({many}): got "
                f"temperature={temperature!r}, topk={topk!r}")
        ts, ks = rows_of(temperature, what), rows_of(topk, what)
        pairs = [tuple((v,) * K for v in check_sampling(t, k, vocab)) for t, k in zip(ts, ks)]
    return (1 if top_p is None and min_p is None else 2), [pr + f + (None, None) for pr, f in zip(pairs, filters)]


class RowSampler:
    """The per-row sampling state of a ``DecodeState`` (the module docstring): ``level``, the six parameter buffers ``params``
    ([K, B], made by the first write), the host mirror ``rows`` (per row, six tuples of K values) and, from level 3 on, what the
    processed rows sampler keeps: ``code_hist`` int32 [B, K, 64] (slot f % 64 of [b, i]: the code row b drew for codebook i in
    frame f of its utterance), ``hist_frame`` int32 [B] (f) and ``hist_live`` int32 [B] (the rows that write their ring and count
    the frame).  At level 4 the seventh parameter stands beside the six: ``typical`` ([K, B] fp32, made at the rise and filled
    with 1.0) with its mirror ``typical_rows`` (per row, K values).  Every write happens outside the captured frame graph, so a change of parameters never recaptures; a rise of the
    level does (``graph_key``): make it before the first capture."""

    def __init__(self, B, K, vocab, device):
        self.B, self.K, self.vocab, self.device = B, K, vocab, device
        self.level, self.params, self.rows = 0, None, None
        self.code_hist, self.hist_frame, self.hist_live, self.live_rows = None, None, None, None
        self.typical, self.typical_rows = None, None

    def need(self, level):
        if self.level < level:
            raise RuntimeError(_FIRST[level])

    def write(self, b, level, *values):
        """Row ``b``'s parameters of ``level`` from its next frame on - ``set_row_sampling``'s two, ``set_row_filters``' two or
        ``set_row_processors``' six or ``set_row_typical``'s seven (each a number or K numbers) - held to their rule first."""
        if level == 4:
            vals = check_row_processors(self.K, self.vocab, *values[:6]) + (check_row_typical(self.K, *values[6:]),)
        elif level == 3:
            vals = check_row_processors(self.K, self.vocab, *values)
        else:
            two = check_sampling(*values, self.vocab) if level == 1 else check_filters(*values)
            two = tuple((v,) * self.K for v in two)
            vals = two + (None,) * 4 if level == 1 else (None, None) + two + (None, None)
        self.store(b, level, vals)

    def store(self, b, level, vals):
        """Validated values (``normalise``'s entries: None leaves a parameter as it is) into column ``b`` of the buffers and the
        mirror; only what changed is written.  A write that raises the level gives its values to every row (a row that is never set
        still samples with valid parameters: the kernels run on all B rows).  A buffer whose K values agree is written with one
        fill (launch-only); only K different values - level 3 on - take a small blocking host-to-device copy.  A seventh value
        is ``typical_p`` (level 4)."""
        b = int(b)
        if not 0 <= b < self.B:
            raise ValueError(f"row {b} out of range (the state has {self.B})")
        if self.params is None:
            if vals[0] is None or vals[1] is None:           # (filters before pairs: the rows path starts with a pair)
                raise RuntimeError(_FIRST[1])
            self.params = tuple(torch.full((self.K, self.B), v, dtype=dt, device=self.device) for v, dt in zip(IDENTITY, DTYPES))
            self.rows = [tuple((v,) * self.K for v in IDENTITY)] * self.B
        rising = level > self.level
        cols, rows = (slice(None), range(self.B)) if rising else (slice(b, b + 1), (b,))
        for j, new in enumerate(vals[:6]):
            if new is not None and (rising or new != self.rows[b][j]):
                self.put(j, cols, new)
        for r in rows:
            self.rows[r] = tuple(old if new is None else new for old, new in zip(self.rows[r], vals))
        if level == 4:
            if self.typical is None:
                self.typical = torch.full((self.K, self.B), 1.0, dtype=torch.float32, device=self.device)
                self.typical_rows = [(1.0,) * self.K] * self.B
            if rising or vals[6] != self.typical_rows[b]:
                self.put(6, cols, vals[6])
            for r in rows:
                self.typical_rows[r] = vals[6]
        if level >= 3 and self.level < 3:
            self.code_hist = torch.zeros(self.B, self.K, HIST_FRAMES, dtype=torch.int32, device=self.device)
            self.hist_frame = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.hist_live = torch.ones(self.B, dtype=torch.int32, device=self.device)
            self.live_rows = list(range(self.B))
        self.level = max(self.level, level)

    def put(self, j, cols, new):
        """Parameter ``j``'s K values ``new`` into the columns ``cols`` of its buffer."""
        view = (self.typical if j == 6 else self.params[j])[:, cols]
        if len(set(new)) == 1:
            view.fill_(new[0])
        else:
            view.copy_(torch.tensor(new, dtype=view.dtype).view(-1, 1))

    def args(self, temperature, topk, top_p=None, min_p=None, repetition_penalty=None, repetition_window=None, typical_p=None):
        """``DecodeState.sampling_args``: what the call names goes to the rows (all of them checked before any is written) and
        (None, None) comes back; two numbers, or None for both, with nothing else named pass through."""
        level, rows = normalise(self.B, self.K, self.vocab, temperature, topk, top_p, min_p, repetition_penalty,
                                repetition_window, level=self.level, typical_p=typical_p)
        if level == 0:
            return temperature, topk
        for b, vals in enumerate(rows):
            self.store(b, level, vals)
        return None, None

    def reset_history(self, b):
        self.need(3)
        self.hist_frame[int(b):int(b) + 1].zero_()

    def set_live(self, rows):
        if self.level < 3:
            return
        rows = sorted(int(b) for b in rows)
        if rows != self.live_rows:
            self.hist_live.copy_(torch.tensor([1 if b in rows else 0 for b in range(self.B)], dtype=torch.int32))
            self.live_rows = rows

    def draw(self, logits, i, q):
        """Codebook ``i``'s codes for [B, V] ``logits`` and the Exp(1) draws ``q``, each row with its own parameters: int32
        [B, 1].  From level 3 on the draw also writes the live rows' rings, and the last codebook's counts the frame."""
        from .models.model import sample_filtered_rows, sample_processed_rows, sample_topk_rows, sample_typical_rows
        self.need(1)
        t, k, p, m, r, w = (buf[i] for buf in self.params)
        if self.level == 1:
            return sample_topk_rows(logits, k, t, q)
        if self.level == 2:
            return sample_filtered_rows(logits, k, t, p, m, q)
        if self.level == 4:
            return sample_typical_rows(logits, k, t, p, m, r, w, self.code_hist[:, i], self.hist_frame, self.hist_live,
                                       self.typical[i], advance=(i == self.K - 1), q=q)
        return sample_processed_rows(logits, k, t, p, m, r, w, self.code_hist[:, i], self.hist_frame, self.hist_live,
                                     advance=(i == self.K - 1), q=q)

    def graph_key(self, temperature, topk):
        """The key of the captured frame graph a frame call with these two replays: the pair itself, or - None for both - what
        tells the rows samplers apart (the kernels read the parameters from the buffers: any change of them replays the graph)."""
        if temperature is None and topk is None:
            return (None, None) + ((), (), ("filters",), ("processors",), ("typical",))[self.level]
        return (float(temperature), int(topk))

    @property
    def row_sampling(self):
        """[(temperature, topk)] * B at levels 1 and 2, else None."""
        return [(r[0][0], r[1][0]) for r in self.rows] if self.level in (1, 2) else None

    @property
    def row_filters(self):
        """[(top_p, min_p)] * B at level 2, else None."""
        return [(r[2][0], r[3][0]) for r in self.rows] if self.level == 2 else None

    @property
    def row_processors(self):
        """Per row, six tuples of K values at level 3, else None."""
        return list(self.rows) if self.level == 3 else None

    @property
    def row_typical(self):
        """Per row, seven tuples of K values - the six and ``typical_p`` - at level 4, else None."""
        return [r + (y,) for r, y in zip(self.rows, self.typical_rows)] if self.level == 4 else None
