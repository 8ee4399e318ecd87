"""Locally typical sampling per request, host side: ``check_typical``; level 4 of ``sampling.normalise`` and ``RowSampler`` (what is
accepted and refused, nothing written after a refusal, one write per changed parameter, the mirror equal to the buffer, the graph
key); ``sampling_kwargs`` at ``typical_p = 1.0`` is what it was; say > conversation > server on a ``row_typical`` server and the
refusal without it; the entry point's declaration; the command-line flag and the serve-file key."""
import os
import re
import types

import pytest
import torch

from test_row_sampling_cpu import K, LONG, MS, VOCAB, RowsCodec, State, StubModel, Tok
from test_sampling_processors_ref_cpu import ProcState

NAN, INF = float("nan"), float("inf")
SIX = (0.9, 50, 1.0, 0.0, 1.0, 64)


def _tup(*vals):
    return tuple((v,) * K if not isinstance(v, tuple) else v for v in vals)


def test_check_typical_rule():
    from csm.engine import check_typical
    assert check_typical(1) == 1.0 and check_typical(0.2) == 0.2 and check_typical(1e-9) == 1e-9
    assert isinstance(check_typical(1), float) and check_typical(torch.tensor(0.5)) == 0.5
    for bad in (0, 0.0, -0.1, 1.0000001, 2, NAN, INF, -INF, True, False, "0.9", None, [0.9], b"1"):
        with pytest.raises(ValueError, match=r"typical_p must be a number in \(0, 1\], got "):
            check_typical(bad)


def test_entry_point_declared_exported_and_wired():
    from csm import hip, models
    from csm.engine import DecodeState
    from csm.hip import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csm_hip.h")).read()
    decl = re.search(r"\bint csm_sample_typical_rows\(([^;]*)\);", header)
    assert decl, "csm_sample_typical_rows is not declared in include/csm_hip.h"
    args = re.sub(r"\s+", " ", decl.group(1))
    assert args == ("const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk, "
                    "const float* temperature, const float* top_p, const float* min_p, const float* penalty, const int* window, "
                    "int* hist, int ldh, int* frame, const int* live, int advance, const float* typical_p, csm_stream_t stream")
    assert "csm_sample_typical_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_sample_typical_rows")
    assert len(hip.lib.csm_sample_typical_rows.argtypes) == 19
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    assert callable(ops.sample_typical_rows) and callable(models.sample_typical_rows)
    assert callable(DecodeState.set_row_typical) and isinstance(DecodeState.row_typical, property)


# ------------------------------------------------------------------------------------------------------------- normalise
def test_normalise_level_4_accepts():
    from csm.sampling import normalise
    level, rows = normalise(2, K, VOCAB, 0.9, 50, typical_p=0.9)
    assert level == 4 and rows == [_tup(*SIX, 0.9)] * 2 and all(len(r) == 7 for r in rows)
    per = [0.2] + [1.0] * (K - 1)
    level, rows = normalise(2, K, VOCAB, [0.9, 0.7], 50, 0.8, None, 1.3, None, typical_p=[0.5, per])
    assert level == 4
    assert rows[0] == _tup(0.9, 50, 0.8, 0.0, 1.3, 64, 0.5) and rows[1] == _tup(0.7, 50, 0.8, 0.0, 1.3, 64, tuple(per))
    level, rows = normalise(1, K, VOCAB, [[0.9, 0.6, 0.6, 0.6]], 50, typical_p=torch.tensor(1.0))
    assert level == 4 and rows[0][0] == (0.9, 0.6, 0.6, 0.6) and rows[0][6] == (1.0,) * K      # 1.0 named is still level 4
    # a level-4 state: anything beyond a plain pair goes to level 4, typical_p at its identity if not named
    assert normalise(2, K, VOCAB, 0.9, 50, level=4) == (0, None) and normalise(2, K, VOCAB, None, None, level=4) == (0, None)
    for kw in (dict(top_p=0.9), dict(min_p=0.1), dict(repetition_penalty=1.3), dict(repetition_window=8)):
        level, rows = normalise(2, K, VOCAB, 0.9, 50, level=4, **kw)
        assert level == 4 and rows[0][6] == (1.0,) * K and len(rows[0]) == 7, kw
    level, rows = normalise(2, K, VOCAB, [0.9, 0.8], 50, level=4)
    assert level == 4 and [r[0][0] for r in rows] == [0.9, 0.8]
    # below level 4 nothing changed
    assert normalise(2, K, VOCAB, 0.9, 50, 0.9, level=3)[0] == 3 and normalise(2, K, VOCAB, 0.9, 50, 0.9, level=3)[1][0][6] is None
    assert normalise(2, K, VOCAB, 0.9, 50, 0.9)[0] == 2 and normalise(2, K, VOCAB, [0.9, 0.8], 50)[0] == 1


@pytest.mark.parametrize("kw,text", [
    (dict(typical_p=0.0), r"typical_p must be a number in \(0, 1\], got 0.0"),
    (dict(typical_p=1.5), r"typical_p must be a number in \(0, 1\], got 1.5"),
    (dict(typical_p=NAN), r"typical_p must be a number in \(0, 1\], got nan"),
    (dict(typical_p=True), "typical_p is a number or a sequence of one entry per row"),
    (dict(typical_p="0.9"), "typical_p is a number or a sequence of one entry per row"),
    (dict(typical_p=[0.9]), r"typical_p is a number or a sequence of one entry per row \(2 rows; an entry is a number or one number "
                            r"per codebook\), got \[0.9\]"),
    (dict(typical_p=[0.9, [0.5] * (K - 1)]), "typical_p is a number or a sequence of one number per codebook"),
    (dict(typical_p=[0.9, [0.5, 0.5, 0.0, 0.5]]), r"typical_p must be a number in \(0, 1\], got 0.0"),
    (dict(typical_p=0.9, top_p=1.5), "top_p must be a number"),
    (dict(typical_p=0.9, repetition_window=65), "repetition_window must be"),
])
def test_normalise_level_4_refuses(kw, text):
    from csm.sampling import normalise
    with pytest.raises(ValueError, match=text):
        normalise(2, K, VOCAB, 0.9, 50, **kw)


def test_normalise_level_4_needs_the_pair_named():
    from csm.sampling import normalise
    for t, k in ((None, None), (0.9, None), (None, 50)):
        with pytest.raises(ValueError, match="need temperature and topk named"):
            normalise(2, K, VOCAB, t, k, typical_p=0.9)
    with pytest.raises(ValueError, match=r"one entry per utterance \(2;"):
        normalise(2, K, VOCAB, 0.9, 50, typical_p=[0.9], unit="utterance")


# ------------------------------------------------------------------------------------------------------------ RowSampler
class Counting:
    """A RowSampler on the CPU whose buffer writes are counted per parameter."""

    def __init__(self, B=3):
        from csm.sampling import RowSampler
        self.s = RowSampler(B, K, VOCAB, "cpu")
        self.writes = []
        put = self.s.put
        self.s.put = lambda j, cols, new: (self.writes.append(j), put(j, cols, new))[1]

    def check_mirror(self):
        s = self.s
        for j, buf in enumerate(s.params):
            assert torch.equal(buf, torch.tensor([s.rows[b][j] for b in range(s.B)], dtype=buf.dtype).t()), j
        assert s.params[6].dtype == torch.float32 and s.params[6].shape == (K, s.B)


def test_row_sampler_level_4():
    c = Counting()
    s = c.s
    assert s.params is None and s.row_typical is None
    with pytest.raises(RuntimeError, match="call set_row_typical first"):
        s.need(4)
    s.write(1, 3, *SIX)                                                   # level 3 first: the seventh buffer is at its identity
    assert s.level == 3 and s.params[6].tolist() == [[1.0] * 3] * K and s.row_processors is not None and s.graph_key(None, None) == (None, None, "processors")
    hist = s.code_hist
    del c.writes[:]
    s.write(0, 4, *SIX, 0.5)                                              # the rise: every row gets the seven
    assert s.level == 4 and sorted(c.writes) == [0, 1, 2, 3, 4, 5, 6]
    assert s.code_hist is hist                                            # (the rings of level 3 stay)
    assert s.params[6].tolist() == [[0.5] * 3] * K and [r[6] for r in s.rows] == [(0.5,) * K] * 3
    assert len(s.params) == 7 and len(s.rows[0]) == 7
    assert s.row_typical == [_tup(*SIX, 0.5)] * 3
    assert s.row_processors is None and s.row_filters is None and s.row_sampling is None
    assert s.graph_key(None, None) == (None, None, "typical") and s.graph_key(0.9, 50) == (0.9, 50)
    c.check_mirror()
    del c.writes[:]
    s.write(0, 4, *SIX, 0.5)                                              # nothing changed: nothing written
    assert c.writes == []
    per = (0.2,) + (1.0,) * (K - 1)
    s.write(2, 4, *SIX, list(per))                                        # one parameter changed: one write, one column
    assert c.writes == [6] and s.params[6][:, 2].tolist() == pytest.approx(list(per)) and s.params[6][:, :2].tolist() == [[0.5] * 2] * K
    assert [r[6] for r in s.rows] == [(0.5,) * K, (0.5,) * K, per]
    del c.writes[:]
    s.write(1, 4, 0.7, 50, 1.0, 0.0, 1.0, 64, 0.5)                        # ... the temperature alone
    assert c.writes == [0] and s.rows[1][0] == (0.7,) * K
    c.check_mirror()
    # refusals write nothing
    del c.writes[:]
    before = (s.params[6].clone(), list(s.rows))
    for bad in (0.0, 1.01, NAN, True, "1", [0.5] * (K + 1), [0.5, 0.5, 0.5, -1]):
        with pytest.raises(ValueError, match="typical_p"):
            s.write(1, 4, *SIX, bad)
    with pytest.raises(ValueError, match="temperature must be"):
        s.write(1, 4, 0.0, 50, 1.0, 0.0, 1.0, 64, 0.5)
    with pytest.raises(ValueError, match="out of range"):
        s.write(3, 4, *SIX, 0.5)
    assert c.writes == [] and torch.equal(s.params[6], before[0]) and s.rows == before[1]
    # the level only rises: a level-3 write on a level-4 state keeps the seventh as it is
    s.write(2, 3, 0.9, 50, 0.8, 0.0, 1.0, 64)
    assert s.level == 4 and s.rows[2][6] == per and s.rows[2][2] == (0.8,) * K
    c.check_mirror()


def test_row_sampler_args_rise_straight_to_level_4():
    c = Counting(2)
    s = c.s
    assert s.args(0.9, 50) == (0.9, 50) and s.level == 0                  # two numbers pass through
    assert s.args(0.9, 50, typical_p=[0.3, 1.0]) == (None, None)
    assert s.level == 4 and s.code_hist.shape == (2, K, 64) and s.hist_frame.tolist() == [0, 0] and s.hist_live.tolist() == [1, 1]
    assert s.params[6].tolist() == [[pytest.approx(0.3), 1.0]] * K and [r[6][0] for r in s.row_typical] == [0.3, 1.0]
    c.check_mirror()
    with pytest.raises(ValueError, match="typical_p must be"):
        s.args(0.9, 50, typical_p=[0.3, 0.0])
    with pytest.raises(ValueError, match="one entry per row"):
        s.args(0.9, 50, typical_p=[0.3])
    assert [r[6][0] for r in s.row_typical] == [0.3, 1.0]
    del c.writes[:]
    assert s.args(0.9, 50, top_p=0.9) == (None, None)                     # beyond a plain pair on a level-4 state: level 4,
    # typical_p at its identity: top_p changes in both rows, typical_p in the row that was not at 1
    assert s.level == 4 and sorted(c.writes) == [2, 2, 6] and s.params[6].tolist() == [[1.0, 1.0]] * K
    assert s.args(0.9, 50) == (0.9, 50)


def test_levels_below_4_are_what_they_were():
    from csm.sampling import DTYPES, IDENTITY, PROCESSOR_NAMES, RowSampler
    assert len(PROCESSOR_NAMES) == len(DTYPES) == len(IDENTITY) == 6
    s = RowSampler(2, K, VOCAB, "cpu")
    s.write(0, 1, 0.9, 50)
    assert s.graph_key(None, None) == (None, None) and s.row_sampling == [(0.9, 50)] * 2 and s.row_typical is None
    s.write(0, 2, 0.9, 0.0)
    assert s.graph_key(None, None) == (None, None, "filters") and s.row_filters == [(0.9, 0.0)] * 2
    s.write(0, 3, *SIX)
    assert s.graph_key(None, None) == (None, None, "processors") and s.row_processors == [_tup(*SIX)] * 2
    assert s.params[6].tolist() == [[1.0] * 2] * K and [r[6] for r in s.rows] == [(1.0,) * K] * 2 and s.code_hist is not None


def test_generation_keywords_are_todays_at_typical_p_one():
    from csm.generator import Generator, sampling_kwargs
    gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    assert sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, typical_p=1.0) == sampling_kwargs(gen, 0.9, 50, 1.0, 0.0) == (0.9, 50, {})
    assert sampling_kwargs(gen, 0.9, 50, 0.9, 0.0, 1.0, 64, typical_p=1.0) == (0.9, 50, {"top_p": 0.9, "min_p": 0.0})
    assert sampling_kwargs(gen, 0.9, 50, 0.9, 0.0, 1.0, 64, None, 1) == (0.9, 50, {"top_p": 0.9, "min_p": 0.0})     # (B positional)
    t, k, kw = sampling_kwargs(gen, 0.9, [50, 20, 20, 20], 1.0, 0.0, 1.3, 16, typical_p=1.0)
    assert (t, k) == ([0.9], [[50, 20, 20, 20]]) and "typical_p" not in kw
    assert sampling_kwargs(gen, [0.9, 0.7], 50, 1.0, 0.0, B=2, typical_p=1.0) == ([0.9, 0.7], 50, {})
    # named: all seven go to the rows
    t, k, kw = sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, typical_p=0.2)
    assert (t, k) == ([0.9], [50])
    assert kw == {"top_p": [1.0], "min_p": [0.0], "repetition_penalty": [1.0], "repetition_window": [64], "typical_p": [0.2]}
    t, k, kw = sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, typical_p=[0.2, 1.0, 1.0, 1.0])
    assert kw["typical_p"] == [[0.2, 1.0, 1.0, 1.0]]
    t, k, kw = sampling_kwargs(gen, [0.9, 0.7], 50, 1.0, 0.0, B=2, typical_p=[0.2, [0.5, 1.0, 1.0, 1.0]])
    assert t == [0.9, 0.7] and k == [50, 50] and kw["typical_p"] == [0.2, [0.5, 1.0, 1.0, 1.0]]
    for bad in (0, 1.5, NAN, True, "0.9", [0.2] * (K + 1)):
        with pytest.raises(ValueError):
            sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, typical_p=bad)
    with pytest.raises(ValueError):
        sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, B=2, typical_p=[0.2, 0.3, 0.4])


# --------------------------------------------------------------------------------------------------------------- the server
class TypState(ProcState):
    """The recording state of the processors test, plus typical sampling."""

    def set_row_typical(self, b, *seven):
        self.proc[b] = seven
        self.log.append(("typical", b) + seven)


@pytest.fixture
def make(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    State.made, State.scripts = [], {}

    def _make(scripts, state=TypState, **kw):
        monkeypatch.setattr(S, "DecodeState", state)
        State.scripts = scripts
        gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
        return gen, gen.serve(**kw), State.made[-1]
    return _make


SERVER = dict(slots=2, chunk_frames=2, temperature=0.8, topk=12, row_sampling=True, row_typical=True, top_p=0.9, min_p=0.05,
              repetition_penalty=1.2, repetition_window=32, typical_p=0.95)
DEFAULT = (0.8, 12, 0.9, 0.05, 1.2, 32, 0.95)


def _seven(req):
    return (req.temperature, req.topk, req.top_p, req.min_p, req.repetition_penalty, req.repetition_window, req.typical_p)


def test_say_over_conversation_over_server(make):
    gen, srv, st = make({s: LONG for s in range(6)}, **SERVER)
    assert srv.row_typical and srv.row_processors and srv.row_filters and srv.row_sampling and srv.typical_p == 0.95
    assert st.log == [("typical", 0) + DEFAULT, ("typical", 1) + DEFAULT]      # every row starts with the server's seven
    per = [0.3, 1.0, 1.0, 1.0]
    plain = srv.submit("a", 0, [], max_audio_length_ms=2 * 80)
    own = srv.submit("b", 1, [], max_audio_length_ms=2 * 80, typical_p=per, repetition_penalty=1.5)
    same = srv.submit("c", 1, [], max_audio_length_ms=2 * 80, typical_p=[0.4] * K)
    assert _seven(plain) == DEFAULT and _seven(own) == (0.8, 12, 0.9, 0.05, 1.5, 32, tuple(per)) and same.typical_p == 0.4
    conv = srv.conversation(typical_p=0.6, seed=3)
    assert conv.typical_p == 0.6 and conv.repetition_penalty == 1.2
    del st.log[:]
    for _ in srv.run():
        pass
    admitted = [e for e in st.log if e[0] in ("typical", "processors", "reset", "filters", "sampling")]
    assert admitted[:4] == [("typical", 0) + _seven(plain), ("reset", 0), ("typical", 1) + _seven(own), ("reset", 1)]
    assert not [e for e in admitted if e[0] in ("processors", "filters", "sampling")]
    assert all(e[2:4] == (None, None) for e in st.log if e[0] in ("first", "frame"))
    t1 = conv.say("one", 2, max_audio_length_ms=2 * 80)
    assert _seven(t1) == DEFAULT[:6] + (0.6,)
    for _ in srv.run():
        pass
    t2 = conv.say("two", 2, max_audio_length_ms=2 * 80, typical_p=1.0, topk=7)
    assert _seven(t2) == (0.8, 7, 0.9, 0.05, 1.2, 32, 1.0)
    assert _seven(srv.conversation().say("three", 3, max_audio_length_ms=2 * 80)) == DEFAULT


def test_bad_values_raise_at_the_call_and_queue_nothing(make):
    gen, srv, st = make({s: LONG for s in range(6)}, **SERVER)
    conv = srv.conversation()
    for bad in (0, 0.0, -0.5, 1.5, NAN, INF, True, "0.9", [0.5] * (K - 1), [0.5, 0.5, 0.5, 0.0], [[0.5] * K]):
        kw = dict(typical_p=bad)
        with pytest.raises(ValueError, match="typical_p"):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError, match="typical_p"):
            srv.conversation(**kw)
        with pytest.raises(ValueError, match="typical_p"):
            conv.say("a", 0, max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError, match="typical_p"):
            gen.serve(**{**SERVER, **kw})
        srv._check()                                                       # (a refused server took nothing over)
    assert srv.queued == 0 and conv._open is None and conv.tokens.shape[0] == 0


def test_a_server_without_row_typical_says_which_flag_is_missing(make):
    with pytest.raises(ValueError, match="row_sampling=True"):
        make({}, row_typical=True)
    with pytest.raises(ValueError, match=r"typical_p=0.9 needs a server made with serve\(row_typical=True\)"):
        make({}, state=ProcState, row_sampling=True, row_processors=True, typical_p=0.9)
    gen, srv, st = make({s: LONG for s in range(6)}, state=ProcState, slots=2, chunk_frames=2, row_sampling=True, row_processors=True)
    assert srv.row_typical is False and srv.typical_p == 1.0
    conv = srv.conversation()
    for bad in (0.9, [0.9] * K, 0.0, "1"):
        with pytest.raises(ValueError, match=r"submit: typical_p needs a server made with serve\(row_typical=True\)"):
            srv.submit("a", 0, [], max_audio_length_ms=MS, typical_p=bad)
        with pytest.raises(ValueError, match=r"conversation: typical_p needs .*row_typical=True"):
            srv.conversation(typical_p=bad)
        with pytest.raises(ValueError, match=r"say: typical_p needs .*row_typical=True"):
            conv.say("a", 0, max_audio_length_ms=MS, typical_p=bad)
    assert srv.queued == 0 and conv._open is None
    # ... None and 1 are the server it was: the processors call, no typical call
    r = srv.submit("a", 0, [], max_audio_length_ms=2 * 80, typical_p=1.0, top_p=0.8)
    r2 = srv.submit("b", 1, [], max_audio_length_ms=2 * 80, typical_p=None)
    assert r.typical_p == 1.0 and r2.typical_p == 1.0
    for _ in srv.run():
        pass
    assert [e[0] for e in st.log if e[0] in ("typical", "processors")] == ["processors"] * 4      # (two at the start, two admitted)


# -------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flag_and_serve_file_key(tmp_path):
    from csm.cli import generate as G
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav")]
    args = G.parse_args(base + ["--text", "x"])
    assert args.typical_p == 1.0 and G.sampling_kw(args, K) == dict(temperature=0.9, topk=50, top_p=1.0, min_p=0.0)
    for mode in (["--text", "x"], ["--text", "x", "--stream"], ["--text", "x", "--next-text", "y"]):
        args = G.parse_args(base + mode + ["--typical-p", "0.9"])
        assert args.typical_p == 0.9
        assert G.sampling_kw(args, K) == dict(temperature=0.9, topk=50, top_p=1.0, min_p=0.0, typical_p=0.9)
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "typical_p": 0.4}\n{"text": "two", "conversation": "c", "typical_p": [0.2, 1, 1.0, 1.0]}\n'
                 '{"text": "three", "top_p": 0.6}\n')
    lines = G.read_serve_file(str(p), K)
    assert lines[0]["typical_p"] == 0.4 and lines[1]["typical_p"] == [0.2, 1.0, 1.0, 1.0] and "typical_p" not in lines[2]
    assert G.line_typical(lines[0]) == {"typical_p": 0.4} and G.line_typical(lines[2]) == {}
    for bad in ('{"text": "x", "typical_p": "0.9"}', '{"text": "x", "typical_p": true}', '{"text": "x", "typical_p": [0.9, 0.9]}',
                '{"text": "x", "typical_p": [0.9, 0.9, true, 0.9]}'):
        q = tmp_path / "bad.jsonl"
        q.write_text(bad + "\n")
        with pytest.raises(ValueError, match="bad.jsonl:1"):
            G.read_serve_file(str(q), K)
    calls = []
    keys = ("temperature", "topk", "top_p", "min_p", "repetition_penalty", "repetition_window", "typical_p")

    class Srv:
        queued, active = 0, []

        def submit(self, text, speaker, context, **kw):
            calls.append(("submit", text, {k: kw[k] for k in keys if k in kw}))
            return object()

        def conversation(self, **kw):
            calls.append(("conversation", {k: kw[k] for k in keys if k in kw}))
            return types.SimpleNamespace(say=lambda text, speaker, **kw: calls.append(
                ("say", text, {k: kw[k] for k in keys if k in kw})) or object())

    model = types.SimpleNamespace(args=types.SimpleNamespace(audio_num_codebooks=K))
    gen = types.SimpleNamespace(sample_rate=24000, load_adapter=None, _model=model, serve=lambda **kw: calls.append(
        ("serve", {k: kw[k] for k in ("row_sampling", "row_filters", "row_processors", "row_typical") + keys if k in kw})) or Srv())
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])          # the file names it: row_typical=True
    assert calls == [("serve", dict(row_sampling=True, row_filters=True, row_typical=True, temperature=0.9, topk=50, top_p=1.0,
                                    min_p=0.0)),
                     ("submit", "one", {"typical_p": 0.4}), ("conversation", {}),
                     ("say", "two", {"typical_p": [0.2, 1.0, 1.0, 1.0]}), ("submit", "three", {"top_p": 0.6})]
    del calls[:]
    p.write_text('{"text": "one"}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p), "--typical-p", "0.9"]), [])      # the command line does
    assert calls == [("serve", dict(row_sampling=True, row_typical=True, temperature=0.9, topk=50, top_p=1.0, min_p=0.0,
                                    typical_p=0.9)), ("submit", "one", {})]
    del calls[:]
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", dict(temperature=0.9, topk=50)), ("submit", "one", {})]      # nothing named: the server it was
