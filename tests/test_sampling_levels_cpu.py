"""The one normaliser of the sampling values and the one per-row state (csm/sampling.py), host side: the level a call needs and
each row's validated values, every error text, nothing written after a refused call, and the generator's pre-checks held to the
same table as ``sampling_args``.  The state's buffers are ordinary tensors, so all of it runs on the CPU."""
import re

import pytest
import torch

from test_row_sampling_cpu import K, VOCAB, RowsCodec, StubModel, Tok

B = 3
NAN = float("nan")
ACOUSTIC = [0.9, 0.7, 0.7, 0.7]                     # K values: one per codebook


def _all(v):
    return (v,) * K


def _six(t, k, p, m, r, w, y=None):
    """A row as ``normalise`` gives it: the six and ``typical_p``, which no case below names (None: left as it is)."""
    return tuple(v if v is None or isinstance(v, tuple) else _all(v) for v in (t, k, p, m, r, w, y))


# (what the call names, the level it needs, per row the entries - None: left as it is)
ACCEPTED = [
    (dict(temperature=0.9, topk=50), 0, None),
    (dict(temperature=None, topk=None), 0, None),
    (dict(temperature=[0.9, 0.8, 0.7], topk=5), 1, [_six(t, 5, None, None, None, None) for t in (0.9, 0.8, 0.7)]),
    (dict(temperature=1, topk=torch.tensor([5, 6, 64])), 1, [_six(1.0, k, None, None, None, None) for k in (5, 6, 64)]),
    (dict(temperature=0.8, topk=5, top_p=[0.9, 1.0, 0.5]), 2, [_six(0.8, 5, p, 0.0, None, None) for p in (0.9, 1.0, 0.5)]),
    (dict(temperature=[0.8, 0.7, 0.6], topk=5, min_p=0.1), 2, [_six(t, 5, 1.0, 0.1, None, None) for t in (0.8, 0.7, 0.6)]),
    (dict(temperature=None, topk=None, top_p=0.5, min_p=[0.0, 0.1, 1]), 2,
     [_six(None, None, 0.5, m, None, None) for m in (0.0, 0.1, 1.0)]),
    (dict(temperature=0.8, topk=5, repetition_penalty=1.3), 3, [_six(0.8, 5, 1.0, 0.0, 1.3, 64)] * B),
    (dict(temperature=0.8, topk=[5, 6, 7], top_p=0.9, repetition_window=[0, 16, 64]), 3,
     [_six(0.8, k, 0.9, 0.0, 1.0, w) for k, w in ((5, 0), (6, 16), (7, 64))]),
    (dict(temperature=[ACOUSTIC, 0.8, 0.8], topk=50), 3,
     [_six(tuple(ACOUSTIC), 50, 1.0, 0.0, 1.0, 64)] + [_six(0.8, 50, 1.0, 0.0, 1.0, 64)] * 2),
    (dict(temperature=0.8, topk=5, min_p=[0.1, [0.0, 0.1, 0.1, 0.1], 0.2]), 3,
     [_six(0.8, 5, 1.0, m, 1.0, 64) for m in (0.1, (0.0, 0.1, 0.1, 0.1), 0.2)]),
]
# (what the call names, the text of the refusal - "row" stands for the unit word)
REFUSED = [
    (dict(temperature=[0.9, 0.8], topk=5), "one value per row"),
    (dict(temperature=0.9, topk=[5, 6, 7, 8]), "one value per row"),
    (dict(temperature=(), topk=5), "one value per row"),
    (dict(temperature=0.9, topk="555"), "one value per row"),
    (dict(temperature=None, topk=5), "one value per row"),
    (dict(temperature=0.8, topk=5, top_p=[0.9, 1.0]), "one value per row"),
    (dict(temperature=0.8, topk=5, min_p=[0.1] * 4), "one value per row"),
    (dict(temperature=[0.8, 0.7], topk=5, top_p=0.9), "one value per row"),
    (dict(temperature=0.8, topk=5, repetition_penalty=[1.3, 1.3]), "one entry per row"),
    (dict(temperature=[ACOUSTIC, 0.8], topk=50), "one entry per row"),
    (dict(temperature=0.8, topk=5, top_p="0.9", repetition_window=16), "one entry per row"),
    (dict(temperature=[ACOUSTIC[:2], 0.8, 0.8], topk=50), "one number per codebook"),
    (dict(temperature=None, topk=None, repetition_penalty=1.3), "need temperature and topk named"),
    # a bad value at the last row
    (dict(temperature=[0.9, 0.8, NAN], topk=5), "temperature must be"),
    (dict(temperature=0.9, topk=[5, 6, 0]), "topk must be"),
    (dict(temperature=0.9, topk=[5, 6, VOCAB + 1], min_p=0.1), "topk must be"),
    (dict(temperature=0.9, topk=5, top_p=[0.9, 1.0, 0.0]), "top_p must be"),
    (dict(temperature=0.9, topk=5, min_p=[0.0, 0.1, NAN]), "min_p must be"),
    (dict(temperature=0.9, topk=5, repetition_penalty=[1.3, 1.0, 0]), "repetition_penalty must be"),
    (dict(temperature=0.9, topk=5, repetition_window=[64, 0, 65]), "repetition_window must be"),
    (dict(temperature=[0.8, 0.8, ACOUSTIC[:3] + [0.0]], topk=50), "temperature must be"),
]


def Recording(level=0):
    """A ``RowSampler`` at ``level`` whose buffer writes from here on are recorded in ``puts``."""
    from csm.sampling import RowSampler

    class _Recording(RowSampler):
        def put(self, j, cols, new):
            self.puts.append((j, cols, new))
            super().put(j, cols, new)
    s = _Recording(B, K, VOCAB, "cpu")
    s.puts = []
    if level >= 1:
        s.write(0, 1, 0.5, 9)
    if level >= 2:
        s.write(0, 2, 0.95, 0.02)
    if level >= 3:
        s.write(0, 3, 0.5, 9, 0.95, 0.02, 1.1, 8)
    if level >= 4:
        s.write(0, 4, 0.5, 9, 0.95, 0.02, 1.1, 8, 0.9)
    del s.puts[:]
    return s


@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: repr(c[0])[:60])
def test_the_level_a_call_needs_and_each_rows_values(case):
    from csm.sampling import normalise
    kw, level, rows = case
    got = normalise(B, K, VOCAB, **kw)
    assert got == (level, rows)
    if rows is not None:
        assert all(type(v) is (int if j in (1, 5) else float) for r in got[1] for j, e in enumerate(r) if e is not None for v in e)
    assert normalise(B, K, VOCAB, unit="utterance", **kw) == got           # (the unit word is in the errors only)


def test_a_state_with_processors_takes_everything_there():
    from csm.sampling import normalise
    assert normalise(B, K, VOCAB, 0.9, 50, level=3) == (0, None) and normalise(B, K, VOCAB, None, None, level=3) == (0, None)
    assert normalise(B, K, VOCAB, [0.9, 0.8, 0.7], 5, level=3) == (3, [_six(t, 5, 1.0, 0.0, 1.0, 64) for t in (0.9, 0.8, 0.7)])
    assert normalise(B, K, VOCAB, 0.9, 5, top_p=0.5, level=3) == (3, [_six(0.9, 5, 0.5, 0.0, 1.0, 64)] * B)
    assert normalise(B, K, VOCAB, 0.9, 5, top_p=0.5, level=2)[0] == 2
    with pytest.raises(ValueError, match="need temperature and topk named"):
        normalise(B, K, VOCAB, None, None, top_p=0.5, level=3)


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: repr(c[0])[:60])
def test_every_refusal_has_its_text_and_nothing_is_written(case):
    from csm.sampling import normalise
    kw, text = case
    with pytest.raises(ValueError, match=re.escape(text)):
        normalise(B, K, VOCAB, **kw)
    with pytest.raises(ValueError, match=re.escape(text.replace("per row", "per utterance"))):
        normalise(B, K, VOCAB, unit="utterance", **kw)
    for level in (0, 1, 2, 3, 4):
        s = Recording(level)
        before = (s.level, None if s.rows is None else list(s.rows), None if s.params is None else [p.clone() for p in s.params])
        with pytest.raises(ValueError):
            s.args(**kw)
        assert s.puts == [] and s.level == before[0] == level
        assert (s.rows, s.params) == (None, None) if level == 0 else (
            s.rows == before[1] and all(torch.equal(p, q) for p, q in zip(s.params, before[2])))


def test_the_writers_check_before_they_write():
    for level in (0, 1, 2, 3, 4):
        s = Recording(level)
        for call in (lambda: s.write(1, 1, 0.0, 5), lambda: s.write(1, 1, 0.9, VOCAB + 1), lambda: s.write(1, 2, 1.5, 0.0),
                     lambda: s.write(1, 3, 0.9, 5, 1.0, 0.0, 1.3, 65), lambda: s.write(1, 3, ACOUSTIC[:3], 5, 1.0, 0.0, 1.3, 16),
                     lambda: s.write(B, 1, 0.9, 5), lambda: s.write(-1, 3, 0.9, 5, 1.0, 0.0, 1.3, 16),
                     lambda: s.write(1, 4, 0.9, 5, 1.0, 0.0, 1.3, 16, 0.0), lambda: s.write(1, 4, 0.9, 5, 1.0, 0.0, 1.3, 16, ACOUSTIC[:3]),
                     lambda: s.write(B, 4, 0.9, 5, 1.0, 0.0, 1.3, 16, 0.9)):
            with pytest.raises(ValueError):
                call()
        assert s.puts == [] and s.level == level
    s = Recording(0)
    with pytest.raises(RuntimeError, match="set_row_sampling first"):       # filters before pairs
        s.write(0, 2, 0.9, 0.1)
    with pytest.raises(RuntimeError, match="set_row_sampling first"):
        s.args(None, None, top_p=0.9)
    assert s.puts == [] and s.level == 0 and s.params is None


def test_the_two_tables_are_coherent():
    from csm import sampling as S
    from csm.hip import ops
    assert len(S.LEVELS) == 5 and tuple(lv.reads for lv in S.LEVELS) == (0, 2, 4, 6, 7) and len(S.PARAMS) == S.LEVELS[-1].reads
    for n, lv in enumerate(S.LEVELS):
        assert set(lv.writes) <= set(range(lv.reads)), n                   # a level writes only what its kernel reads
        assert (lv.fn is None and lv.flag is None and lv.first is None) if n == 0 else (
            callable(getattr(ops, lv.fn)) and lv.flag.startswith("row_") and lv.first.endswith(f"call set_{lv.flag} first")), n
    assert S.LEVELS[0].writes == () and S.LEVELS[0].tag is None and [lv.rings for lv in S.LEVELS] == [False, False, False, True, True]
    assert S.PROCESSOR_NAMES == ("temperature", "topk", "top_p", "min_p", "repetition_penalty", "repetition_window")
    assert S.DTYPES == (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32)
    assert S.IDENTITY == (1.0, 1, 1.0, 0.0, 1.0, 64) and S.HIST_FRAMES == 64
    assert tuple(p.name for p in S.PARAMS) == S.PROCESSOR_NAMES + ("typical_p",) and S.PARAMS[6].identity == 1.0
    for j, p in enumerate(S.PARAMS):                                       # the identity passes its own rule, at its position
        got = S.check_row(K, VOCAB, range(len(S.PARAMS)), [q.identity for q in S.PARAMS])[j]
        assert got == _all(p.identity) and type(got[0]) is (float if p.dtype.is_floating_point else int), p.name


def _mirror_is_buffers(s):
    for j, buf in enumerate(s.params):
        want = torch.tensor([s.rows[b][j] for b in range(B)], dtype=buf.dtype).t()
        assert buf.shape == (K, B) and torch.equal(buf, want), j


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[1]], ids=lambda c: repr(c[0])[:60])
def test_accepted_values_reach_the_buffers_and_the_mirror(case):
    kw, level, rows = case
    s = Recording(1 if kw["temperature"] is None else 0)
    assert s.args(**kw) == (None, None) and s.level == level
    _mirror_is_buffers(s)
    for b, want in enumerate(rows):
        assert all(w is None or w == got for w, got in zip(want, s.rows[b])), b
    assert (s.row_sampling is not None, s.row_filters is not None, s.row_processors is not None) == (level < 3, level == 2, level == 3)
    puts = len(s.puts)
    assert s.args(**kw) == (None, None) and len(s.puts) == puts            # the same values again: nothing is written


def test_the_write_that_raises_the_level_gives_its_values_to_every_row():
    s = Recording(0)
    s.write(1, 1, 1.25, 7)
    assert s.row_sampling == [(1.25, 7)] * B and s.row_filters is None and s.graph_key(None, None) == (None, None)
    s.write(0, 1, 0.5, 3)
    assert s.row_sampling == [(0.5, 3), (1.25, 7), (1.25, 7)]
    s.write(2, 2, 0.5, 0.1)
    assert s.row_filters == [(0.5, 0.1)] * B and s.row_sampling == [(0.5, 3), (1.25, 7), (1.25, 7)]
    assert s.graph_key(None, None) == (None, None, "filters") and s.graph_key(0.9, 50.0) == (0.9, 50)
    _mirror_is_buffers(s)
    s.set_live([0])                                                        # (nothing below level 3)
    with pytest.raises(RuntimeError, match="set_row_processors first"):
        s.reset_history(0)
    assert s.hist_live is None
    s.write(0, 3, ACOUSTIC, 9, 0.9, 0.0, 1.3, 16)
    assert s.row_processors == [_six(tuple(ACOUSTIC), 9, 0.9, 0.0, 1.3, 16)[:6]] * B and s.row_sampling is None and s.row_filters is None
    assert s.graph_key(None, None) == (None, None, "processors")
    assert s.code_hist.shape == (B, K, 64) and s.hist_frame.tolist() == [0] * B and s.hist_live.tolist() == [1] * B
    del s.puts[:]
    s.write(1, 3, ACOUSTIC, 9, 0.9, 0.0, 2.0, 16)                          # one parameter of one row: one write
    assert [(j, cols) for j, cols, _ in s.puts] == [(4, slice(1, 2))] and s.row_processors[1][4] == _all(2.0)
    _mirror_is_buffers(s)
    s.set_live([2, 0])
    assert s.hist_live.tolist() == [1, 0, 1]


# ------------------------------------------------------------------------------------------ the generator's pre-checks
def _generator_side(kw):
    """The call ``generate_batch`` makes of ``kw`` (its defaults where the table names nothing)."""
    from csm.generator import Generator, sampling_kwargs
    gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    d = dict(top_p=1.0, min_p=0.0, repetition_penalty=1.0, repetition_window=64)
    return sampling_kwargs(gen, kw["temperature"], kw["topk"], *[d[n] if kw.get(n) is None else kw[n] for n in d], B=B)


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[0]["temperature"] is not None], ids=lambda c: repr(c[0])[:60])
def test_what_the_generator_lets_through_the_state_takes_as_the_direct_call(case):
    kw, level, rows = case
    t, k, more = _generator_side(kw)
    direct, through = Recording(0), Recording(0)
    assert through.args(t, k, **more) == direct.args(**kw)
    assert (through.level, through.rows) == (direct.level, direct.rows) and direct.level == level
    if level == 0:
        assert (t, k, more) == (kw["temperature"], kw["topk"], {})         # nothing new named: untouched


@pytest.mark.parametrize("case", [c for c in REFUSED if c[0]["temperature"] is not None or c[0]["topk"] is not None],
                         ids=lambda c: repr(c[0])[:60])
def test_what_the_state_refuses_the_generator_refuses_with_its_unit_word(case):
    kw, text = case
    with pytest.raises(ValueError, match=re.escape(text.replace("per row", "per utterance"))):
        _generator_side(kw)
    with pytest.raises(ValueError, match=re.escape(text)):
        Recording(0).args(**kw)
