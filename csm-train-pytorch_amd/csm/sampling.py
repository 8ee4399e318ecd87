"""Sampling parameters, host side: the rules a value is held to (``check_*``), the one normaliser of what a call names
(``normalise``) and the per-row state of a ``DecodeState`` (``RowSampler``).

A state samples at one of five levels, and the level only rises: 0 - the scalar path, two numbers per frame call
(``csm_sample_topk``); 1 - each row its own temperature / top-k (``csm_sample_topk_rows``); 2 - and its own top-p / min-p
(``csm_sample_filtered_rows``); 3 - all six per row and per codebook, with the windowed repetition penalty and the rows' rings of
sampled codes (``csm_sample_processed_rows``); 4 - and locally typical sampling, ``typical_p`` per row and per codebook
(``csm_sample_typical_rows``).  Whatever the level, every parameter sits in its own [K, B] device buffer (codebook-major:
codebook i's draw hands row i of each to the kernel, which reads ``topk[row]`` from the pointer it is given) and in one host
mirror; below level 3 the K entries of a column are equal, and a parameter the level's kernel does not read stays at its identity.

What a parameter is and what a level is stands in two tables, ``PARAMS`` and ``LEVELS`` (below the rules); the state, the
normaliser, the launch wrappers (csm/hip/ops.py, csm/models/model.py), the server (csm/serving.py) and the command line
(csm/cli/generate.py) walk them.
"""
import math
import numbers
from collections import namedtuple

import torch


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


# A parameter, in the kernels' order (the entry points alone put top-k before the temperature): its buffer's dtype, what it is
# before a write names it (no nucleus, no min-p cut, no penalty, no typical cut; the pair's placeholders are never read - the first
# write brings a pair), its rule and its position among the rule's arguments and results, and whether a request may name the
# identity on a server below the parameter's level (typical_p = 1 asks for nothing; the older six are refused whenever named).
Param = namedtuple("Param", "name dtype identity rule pos identity_ok")
PARAMS = (
    Param("temperature", torch.float32, 1.0, check_sampling, 0, False),
    Param("topk", torch.int32, 1, check_sampling, 1, False),
    Param("top_p", torch.float32, 1.0, check_filters, 0, False),
    Param("min_p", torch.float32, 0.0, check_filters, 1, False),
    Param("repetition_penalty", torch.float32, 1.0, check_processors, 0, False),
    # (SMP_HIST of csrc/generate.hip: the frames a row's ring of sampled codes holds, per codebook)
    Param("repetition_window", torch.int32, 64, check_processors, 1, False),
    Param("typical_p", torch.float32, 1.0, check_typical, 0, True),
)
# A level, by its number: ``fn`` - the launch that draws (its name in csm.hip.ops and csm.models.model; "csm_" + fn is the entry
# point); ``reads`` - how many leading parameters its kernel reads; ``writes`` - those a ``set_row_*`` of the level brings;
# ``rings`` - whether the kernel keeps the rows' rings of sampled codes; ``tag`` - what it adds to the captured frame graph's key;
# ``flag`` - the ``serve()`` keyword that asks for it ("set_" + flag is the state's writer); and the texts that speak of it:
# ``first`` (the state is below it), ``needs`` (serve: the flag without row_sampling), ``value`` (serve: a value of its own
# without the flag), ``refusal`` (a request names what is its own on a server below it; temperature / topk there: the server's).
Level = namedtuple("Level", "fn reads writes rings tag flag first needs value refusal")
LEVELS = (
    Level(None, 0, (), False, None, None, None, None, None, None),
    Level("sample_topk_rows", 2, (0, 1), False, (), "row_sampling",
          "temperature = topk = None samples each row with its own pair: call set_row_sampling first", None, None,
          "{what}: temperature / topk per request need a server made with serve(row_sampling=True) (this server samples every row "
          "with temperature={temperature}, topk={topk})"),
    Level("sample_filtered_rows", 4, (2, 3), False, ("filters",), "row_filters", "no row filters: call set_row_filters first",
          "serve(row_filters=True) needs row_sampling=True: top-p / min-p live in the rows sampler",
          "top_p={top_p!r} / min_p={min_p!r} need a server made with serve(row_filters=True) (and row_sampling=True)",
          "{what}: top_p / min_p per request need a server made with serve(row_filters=True) (with row_sampling=True; this server "
          "samples without filters)"),
    Level("sample_processed_rows", 6, (0, 1, 2, 3, 4, 5), True, ("processors",), "row_processors",
          "no row processors: call set_row_processors first",
          "serve(row_processors=True) needs row_sampling=True: the repetition penalty and per-codebook parameters live in the rows sampler",
          "repetition_penalty={repetition_penalty!r} / repetition_window={repetition_window!r} and a sequence of values per codebook "
          "need a server made with serve(row_processors=True) (and row_sampling=True)",
          "{what}: repetition_penalty / repetition_window and a sequence of values per codebook need a server made with "
          "serve(row_processors=True) (with row_sampling=True)"),
    Level("sample_typical_rows", 7, (0, 1, 2, 3, 4, 5, 6), True, ("typical",), "row_typical",
          "no row typical sampling: call set_row_typical first",
          "serve(row_typical=True) needs row_sampling=True: typical sampling lives in the rows sampler",
          "typical_p={typical_p!r} needs a server made with serve(row_typical=True) (and row_sampling=True)",
          "{what}: typical_p needs a server made with serve(row_typical=True) (with row_sampling=True)"),
)
# the first level of whole rows: a write brings everything the kernel reads, a value may be K numbers (one per codebook), the
# kernel keeps the rings - and the entry points take the ring arguments after the parameters this level reads
FULL_LEVEL = next(n for n, lv in enumerate(LEVELS) if lv.rings)
NAMES = tuple(p.name for p in PARAMS)
PROCESSOR_NAMES = NAMES[:LEVELS[FULL_LEVEL].reads]                    # (the six of the processed sampler, under their old names)
DTYPES = tuple(p.dtype for p in PARAMS[:len(PROCESSOR_NAMES)])
IDENTITY = tuple(p.identity for p in PARAMS[:len(PROCESSOR_NAMES)])
HIST_FRAMES = PARAMS[NAMES.index("repetition_window")].identity      # (the widest window is the ring)


def own_params(level):
    """The indices of the parameters ``level`` is the first to read."""
    return range(LEVELS[level - 1].reads, LEVELS[level].reads)


def _row(indices, vals):
    """One entry per parameter: ``vals`` at ``indices``, None (left as it is) elsewhere."""
    return tuple(vals[indices.index(j)] if j in indices else None for j in range(len(PARAMS)))


def check_row(K, vocab, indices, values, each=True):
    """One row's ``values`` of the parameters ``indices`` (a rule's parameters come together), each a number or K numbers, held to
    their rules codebook by codebook.  Returns one tuple of K values per index (floats; ints for topk and the window).  ``each``
    False (below ``FULL_LEVEL``): a value is one number for every codebook and goes to its rule as it is."""
    indices = tuple(indices)
    if len(values) != len(indices):
        raise TypeError(f"{len(indices)} values ({', '.join(NAMES[j] for j in indices)}), got {len(values)}")
    cols = {j: per_codebook(NAMES[j], v, K) if each else [v] for j, v in zip(indices, values)}
    out = {j: [] for j in indices}
    groups = [[g for g in indices if PARAMS[g].rule is PARAMS[j].rule] for j in indices if PARAMS[j].pos == 0]
    for i in range(K if each else 1):
        for group in groups:
            rule = PARAMS[group[0]].rule
            got = rule(*[cols[g][i] for g in group], *([vocab] if rule is check_sampling else []))   # (top-k's bound is the vocabulary)
            for g, v in zip(group, got if isinstance(got, tuple) else (got,)):
                out[g].append(v)
    return tuple(tuple(out[j]) * (1 if each else K) for j in indices)


def check_row_processors(K, vocab, temperature, topk, top_p, min_p, repetition_penalty, repetition_window):
    """``check_row`` of the six parameters of the processed sampler."""
    return check_row(K, vocab, range(len(PROCESSOR_NAMES)), (temperature, topk, top_p, min_p, repetition_penalty, repetition_window))


def check_row_typical(K, typical_p):
    """``check_row`` of ``typical_p`` alone: a tuple of K floats."""
    return check_row(K, None, (NAMES.index("typical_p"),), (typical_p,))[0]


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
    """What a frame call's sampling values ask for: (the level the call needs, per row ``len(PARAMS)`` entries - a tuple of K
    validated values each, or None for a parameter the call leaves as it is).  Level 0: two numbers, or None for both - the call
    passes them through and writes nothing (no rows come back).  Each value is None (not named), a number (every row) or B
    entries; from ``FULL_LEVEL`` on an entry is a number or K numbers, one per codebook.  Level 1 (a sequence in the pair) writes
    the pair; level 2 (``top_p`` / ``min_p`` named) the filters - the one not named at its identity - and the pair, unless both
    are None.  Everything goes to the rows - all the level's kernel reads, those not named at their identity - when a penalty, a
    window, a per-codebook entry or a higher level's parameter (``typical_p``) is named, or anything beyond a plain pair on a
    state at ``FULL_LEVEL`` or above: at the highest of ``FULL_LEVEL``, the state's ``level`` and the level of what is named.
    All is checked here, so the caller writes all rows or none.  ``unit``: what the errors call a row ("utterance": the
    generator's calls, checked before any cache is taken over)."""
    many = f"{B} rows" if unit == "row" else f"{B}"

    def rows_of(v, what):
        vs = [v] * B if _is_number(v) else _as_list(v)
        if vs is None or len(vs) != B:
            raise ValueError(what)
        return vs

    given = (temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p)
    plain = (temperature is None and topk is None) or (_is_number(temperature) and _is_number(topk))
    above = [n for n in range(FULL_LEVEL + 1, len(LEVELS)) if any(given[j] is not None for j in own_params(n))]
    if (above or names_processors(temperature, topk, top_p, min_p, repetition_penalty=repetition_penalty,
                                  repetition_window=repetition_window)
            or (level >= FULL_LEVEL and not (plain and top_p is None and min_p is None))):
        target = max([FULL_LEVEL, level] + above)
        idx = LEVELS[target].writes
        if temperature is None or topk is None:
            higher = "".join(name + ", " for name in NAMES[LEVELS[FULL_LEVEL].reads:LEVELS[target].reads])
            raise ValueError(f"{higher}per-codebook parameters and the repetition penalty need temperature and topk named")
        cols = []
        for j in idx:
            v = PARAMS[j].identity if given[j] is None else given[j]
            cols.append(rows_of(v, f"{NAMES[j]} is a number or a sequence of one entry per {unit} ({many}; an entry is a number or "
                                   f"one number per codebook), got {v!r}"))
        return target, [_row(idx, check_row(K, vocab, idx, [vs[b] for vs in cols])) for b in range(B)]
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
    both = LEVELS[1].writes + LEVELS[2].writes
    return (1 if top_p is None and min_p is None else 2), [_row(both, pr + f) for pr, f in zip(pairs, filters)]


class RowSampler:
    """The per-row sampling state of a ``DecodeState`` (the module docstring): ``level``, one parameter buffer per ``PARAMS``
    record in ``params`` ([K, B] each, made by the first write at the identities), the host mirror ``rows`` (per row, one tuple
    of K values per parameter) and, from the first level that keeps them on, the rings: ``code_hist`` int32 [B, K, 64] (slot
    f % 64 of [b, i]: the code row b drew for codebook i in frame f of its utterance), ``hist_frame`` int32 [B] (f) and
    ``hist_live`` int32 [B] (the rows that write their ring and count the frame).  Every write happens outside the captured
    frame graph, so a change of parameters never recaptures; a rise of the level does (``graph_key``): make it before the first
    capture."""

    def __init__(self, B, K, vocab, device):
        self.B, self.K, self.vocab, self.device = B, K, vocab, device
        self.level, self.params, self.rows = 0, None, None
        self.code_hist, self.hist_frame, self.hist_live, self.live_rows = None, None, None, None
        self.stats = False                                # (DecodeState.enable_stats: the frame body also writes the statistics)

    def need(self, level):
        if self.level < level:
            raise RuntimeError(LEVELS[level].first)

    @property
    def keeps_history(self):
        """Whether the state's draws keep the rows' rings of sampled codes."""
        return LEVELS[self.level].rings

    def write(self, b, level, *values):
        """Row ``b``'s parameters of ``level`` from its next frame on - what ``LEVELS[level]`` writes: ``set_row_sampling``'s two,
        ``set_row_filters``' two, ``set_row_processors``' six or ``set_row_typical``'s seven (below ``FULL_LEVEL`` a number each,
        from there on a number or K numbers) - held to their rule first."""
        lv = LEVELS[level]
        self.store(b, level, _row(lv.writes, check_row(self.K, self.vocab, lv.writes, values, each=lv.rings)))

    def store(self, b, level, vals):
        """Validated values (``normalise``'s entries: None leaves a parameter as it is) into column ``b`` of the buffers and the
        mirror; only what changed is written.  A write that raises the level gives its values to every row (a row that is never set
        still samples with valid parameters: the kernels run on all B rows).  A buffer whose K values agree is written with one
        fill (launch-only); only K different values - ``FULL_LEVEL`` on - take a small blocking host-to-device copy."""
        b = int(b)
        if not 0 <= b < self.B:
            raise ValueError(f"row {b} out of range (the state has {self.B})")
        if self.params is None:
            if any(vals[j] is None for j in LEVELS[1].writes):    # (filters before pairs: the rows path starts with a pair)
                raise RuntimeError(LEVELS[1].first)
            self.params = tuple(torch.full((self.K, self.B), p.identity, dtype=p.dtype, device=self.device) for p in PARAMS)
            self.rows = [tuple((p.identity,) * self.K for p in PARAMS)] * self.B
        rising = level > self.level
        cols, rows = (slice(None), range(self.B)) if rising else (slice(b, b + 1), (b,))
        for j, new in enumerate(vals):
            if new is not None and (rising or new != self.rows[b][j]):
                self.put(j, cols, new)
        for r in rows:
            self.rows[r] = tuple(old if new is None else new for old, new in zip(self.rows[r], vals))
        if LEVELS[level].rings and not self.keeps_history:
            self.code_hist = torch.zeros(self.B, self.K, HIST_FRAMES, dtype=torch.int32, device=self.device)
            self.hist_frame = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.hist_live = torch.ones(self.B, dtype=torch.int32, device=self.device)
            self.live_rows = list(range(self.B))
        self.level = max(self.level, level)

    def put(self, j, cols, new):
        """Parameter ``j``'s K values ``new`` into the columns ``cols`` of its buffer."""
        view = self.params[j][:, cols]
        if len(set(new)) == 1:
            view.fill_(new[0])
        else:
            view.copy_(torch.tensor(new, dtype=view.dtype).view(-1, 1))

    def args(self, temperature, topk, top_p=None, min_p=None, repetition_penalty=None, repetition_window=None, typical_p=None):
        """``DecodeState.sampling_args``: what the call names goes to the rows (all of them checked before any is written) and
        (None, None) comes back; two numbers, or None for both, with nothing else named pass through."""
        level, rows = normalise(self.B, self.K, self.vocab, temperature, topk, top_p, min_p, repetition_penalty,
                                repetition_window, level=self.level, typical_p=typical_p)
        if not level:
            return temperature, topk
        for b, vals in enumerate(rows):
            self.store(b, level, vals)
        return None, None

    def reset_history(self, b):
        self.need(FULL_LEVEL)
        self.hist_frame[int(b):int(b) + 1].zero_()

    def park_history(self, rows):
        """The rings and frame counters of ``rows`` (<= 16, distinct) as one packed int32 tensor [R, K * 64 + 1] - ONE launch
        (``ops.sample_hist_move_rows``); None below the levels that keep rings.  The state is only read."""
        if not self.keeps_history:
            return None
        from .hip import ops
        packed = torch.empty(len(rows), self.K * HIST_FRAMES + 1, dtype=torch.int32, device=self.device)
        return ops.sample_hist_move_rows(self.code_hist, self.hist_frame, packed, rows, False)

    def resume_history(self, rows, packed):
        """``packed`` (``park_history``'s format, row r for ``rows[r]``) back into the named rows' rings and counters - ONE
        launch; the counters are restored, not reset.  The buffers keep their addresses, the level and ``hist_live`` stay."""
        self.need(FULL_LEVEL)
        from .hip import ops
        ops.sample_hist_move_rows(self.code_hist, self.hist_frame, packed.contiguous(), rows, True)

    def set_live(self, rows):
        if not self.keeps_history:
            return
        rows = sorted(int(b) for b in rows)
        if rows != self.live_rows:
            self.hist_live.copy_(torch.tensor([1 if b in rows else 0 for b in range(self.B)], dtype=torch.int32))
            self.live_rows = rows

    def draw(self, logits, i, q):
        """Codebook ``i``'s codes for [B, V] ``logits`` and the Exp(1) draws ``q``, each row with its own parameters: int32
        [B, 1].  Where the level keeps rings the draw also writes the live rows', and the last codebook's counts the frame."""
        from .models.model import _sample_rows
        self.need(1)
        lv = LEVELS[self.level]
        ring = (self.code_hist[:, i], self.hist_frame, self.hist_live) if lv.rings else ()
        return _sample_rows(self.level, logits, [buf[i] for buf in self.params[:lv.reads]], ring, i == self.K - 1, q)

    def graph_key(self, temperature, topk):
        """The key of the captured frame graph a frame call with these two replays: the pair itself, or - None for both - what
        tells the rows samplers apart (the kernels read the parameters from the buffers: any change of them replays the graph)."""
        tag = ("stats",) if self.stats else ()              # (statistics mode is another frame body: DecodeState.enable_stats)
        if temperature is None and topk is None:
            return (None, None) + (LEVELS[self.level].tag or ()) + tag
        return (float(temperature), int(topk)) + tag

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
        return [r[:LEVELS[3].reads] for r in self.rows] if self.level == 3 else None

    @property
    def row_typical(self):
        """Per row, seven tuples of K values - the six and ``typical_p`` - at level 4, else None."""
        return [r[:LEVELS[4].reads] for r in self.rows] if self.level == 4 else None


class SampleStats:
    """What the model thought of the codes of an utterance (``return_stats=True`` / ``serve(stats=True)``): ``logprob``,
    ``entropy`` (nats) and ``pmax``, fp32 [frames, K] each on the CPU - per frame and codebook, the log-probability of the drawn
    code and the entropy and largest probability of the distribution it was drawn from, at temperature 1 with no filter and no
    penalty (``csm_sample_stats_rows``).  The frames are the frames of the codes: what lies past EOS or the length limit is cut.
    ``-logprob.sum()`` is the next-frame training objective's loss on the utterance, summed over its rows."""

    NAMES = ("logprob", "entropy", "pmax")

    def __init__(self, K, data=None):
        self.K = int(K)
        self._data = torch.zeros(3, 0, self.K) if data is None else data          # [3, frames, K]

    @classmethod
    def of_frames(cls, K, frames, b=0):
        """From per-frame device tensors [3, K, B] (``DecodeState.frame_stats``), column ``b``: one host copy."""
        if not len(frames):
            return cls(K)
        return cls(K, torch.stack([f[:, :, b] for f in frames], 1).float().cpu())

    logprob = property(lambda self: self._data[0])
    entropy = property(lambda self: self._data[1])
    pmax = property(lambda self: self._data[2])

    def __len__(self):
        return self._data.shape[1]

    def extend(self, other):
        """The frames of ``other`` after this one's (a served request grows chunk by chunk)."""
        self._data = torch.cat([self._data, other._data], 1)
        return self

    def cut(self, frames):
        """Keep the first ``frames`` frames."""
        self._data = self._data[:, :max(int(frames), 0)]
        return self

    def summary(self):
        """The command line's JSON object (``--stats-file``): per frame, codebook 0's three numbers; per frame, the sum of all
        K log-probabilities; and their mean over every code of the utterance (None for no frames)."""
        n = len(self)
        return {"codebook0": {name: [float(v) for v in self._data[j, :, 0]] for j, name in enumerate(self.NAMES)},
                "frame_logprob": [float(v) for v in self.logprob.double().sum(1)],
                "mean_logprob": float(self.logprob.double().mean()) if n else None}
