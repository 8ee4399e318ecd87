"""Per-request top-p / min-p, host side (``Generator.serve(row_sampling=True, row_filters=True)``): the rule of ``check_filters``,
say > conversation > server, every admitted slot gets its resolved filters before its first frame, a server without
``row_filters`` refuses them and is the server it was, the entry point's declaration, and the serve-file / command-line rule."""
import os
import re
import types

import pytest

from test_row_sampling_cpu import LONG, MS, VOCAB, RowsCodec, State, StubModel, Tok

NAN, INF = float("nan"), float("inf")
BAD = [dict(top_p=0), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=NAN), dict(top_p=INF), dict(top_p=True),
       dict(top_p="0.9"), dict(min_p=-0.01), dict(min_p=1.01), dict(min_p=NAN), dict(min_p=INF), dict(min_p=False),
       dict(min_p="0")]


class FilterState(State):
    """The recording state of the row-sampling test, plus the filters."""

    def __init__(self, engine, B, adapters=None, bank=None):
        super().__init__(engine, B, adapters, bank)
        self.filters = [None] * B

    def set_row_filters(self, b, top_p, min_p):
        self.filters[b] = (top_p, min_p)
        self.log.append(("filters", b, top_p, min_p))

    def serve_first(self, last_h, rows, temperature, topk):
        self.log.append(("first-filters", tuple(rows), tuple(self.filters[b] for b in rows)))
        return super().serve_first(last_h, rows, temperature, topk)


class NoFilterState(State):
    """A state from before the filters: any access to ``set_row_filters`` raises."""
    set_row_filters = property()


@pytest.fixture
def make(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    State.made, State.scripts = [], {}

    def _make(scripts, state=FilterState, **kw):
        monkeypatch.setattr(S, "DecodeState", state)
        State.scripts = scripts
        gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
        return gen, gen.serve(**kw), State.made[-1]
    return _make


def test_entry_point_declared_exported_and_wired():
    from csm import hip
    from csm.engine import DecodeState
    from csm.hip import ops
    from csm.models import model
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csm_hip.h")).read()
    decl = re.search(r"\bint csm_sample_filtered_rows\(([^;]*)\);", header)
    assert decl, "csm_sample_filtered_rows is not declared in include/csm_hip.h"
    assert re.sub(r"\s+", " ", decl.group(1)) == (
        "const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk, const float* temperature, "
        "const float* top_p, const float* min_p, csm_stream_t stream")
    assert "csm_sample_filtered_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_sample_filtered_rows")
    assert len(hip.lib.csm_sample_filtered_rows.argtypes) == 11
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    assert callable(ops.sample_filtered_rows) and callable(model.sample_filtered_rows)
    assert callable(DecodeState.set_row_filters) and isinstance(DecodeState.row_filters, property)


def test_check_filters_rule():
    from csm.engine import check_filters
    assert check_filters(1, 0) == (1.0, 0.0) and check_filters(0.9, 0.05) == (0.9, 0.05) and check_filters(1e-6, 1) == (1e-6, 1.0)
    assert all(type(v) is float for v in check_filters(1, 0))
    for bad in BAD:
        kw = {**dict(top_p=0.9, min_p=0.1), **bad}
        with pytest.raises(ValueError, match=re.escape(repr(list(bad.values())[0]))):
            check_filters(kw["top_p"], kw["min_p"])
    for p, m in ((None, 0.0), (1.0, None), ([0.9], 0.0), (0.9, {})):
        with pytest.raises(ValueError):
            check_filters(p, m)


def test_resolution_order_and_admission(make):
    gen, srv, st = make({s: LONG for s in range(6)}, slots=2, chunk_frames=2, row_sampling=True, row_filters=True, top_p=0.95,
                        min_p=0.02)
    assert srv.row_filters is True and (srv.top_p, srv.min_p) == (0.95, 0.02)
    # the rows start with the server's filters, after its pair
    assert st.log == [("sampling", 0, 0.9, 50), ("sampling", 1, 0.9, 50), ("filters", 0, 0.95, 0.02), ("filters", 1, 0.95, 0.02)]
    del st.log[:]
    reqs = [srv.submit("a", 0, [], max_audio_length_ms=2 * 80),
            srv.submit("b", 1, [], max_audio_length_ms=4 * 80, top_p=0.5),
            srv.submit("c", 2, [], max_audio_length_ms=4 * 80, top_p=1, min_p=0, temperature=0.7),
            srv.submit("d", 3, [], max_audio_length_ms=2 * 80, min_p=1)]
    assert [(r.top_p, r.min_p) for r in reqs] == [(0.95, 0.02), (0.5, 0.02), (1.0, 0.0), (0.95, 1.0)]
    assert all(type(r.top_p) is float and type(r.min_p) is float for r in reqs)
    for _ in srv.run():
        pass
    assert all(r.done for r in reqs)
    firsts = [e for e in st.log if e[0] == "first-filters"]
    assert [e[1:] for e in firsts] == [((0, 1), ((0.95, 0.02), (0.5, 0.02))), ((0,), ((1.0, 0.0),)), ((1,), ((0.95, 1.0),))]
    for e in firsts:                                                       # written at admission, next to the pair, before the prefill
        for b in e[1]:
            before = [x[0] for x in st.log[:st.log.index(e)] if x[0] in ("sampling", "filters", "prefill") and x[1] == b]
            assert before[-3:] == ["sampling", "filters", "prefill"]
    assert all(e[2:4] == (None, None) for e in st.log if e[0] in ("first", "frame"))
    assert sum(e[0] == "filters" for e in st.log) == 4                     # once per admission, nothing else
    # say > conversation > server
    conv = srv.conversation(min_p=0.1)
    assert (conv.top_p, conv.min_p) == (0.95, 0.1)
    t1 = conv.say("one", 4, max_audio_length_ms=2 * 80, top_p=0.3)
    assert (t1.top_p, t1.min_p) == (0.3, 0.1)
    for _ in srv.run():
        pass
    t2 = conv.say("two", 4, max_audio_length_ms=2 * 80)
    assert (t2.top_p, t2.min_p) == (0.95, 0.1)
    plain = srv.conversation()
    assert (plain.top_p, plain.min_p) == (0.95, 0.02)


def test_bad_values_raise_before_they_queue(make):
    gen, srv, st = make({0: LONG}, slots=2, chunk_frames=2, row_sampling=True, row_filters=True)
    conv = srv.conversation()
    for bad in BAD:
        value = re.escape(repr(list(bad.values())[0]))
        with pytest.raises(ValueError, match=value):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **bad)
        with pytest.raises(ValueError, match=value):
            srv.conversation(**bad)
        with pytest.raises(ValueError, match=value):
            conv.say("a", 0, max_audio_length_ms=MS, **bad)
        with pytest.raises(ValueError, match=value):                        # the server's own defaults, under the same rule
            gen.serve(slots=2, chunk_frames=2, row_sampling=True, row_filters=True, **bad)
        srv._check()                                                       # (a refused server took nothing over)
    assert srv.queued == 0 and conv._open is None and conv.tokens.shape[0] == 0
    srv.submit("a", 0, [], max_audio_length_ms=MS, top_p=1, min_p=1)       # the bounds themselves are fine
    assert srv.queued == 1


@pytest.mark.parametrize("kw", [dict(), dict(row_sampling=True)])
def test_a_server_without_row_filters_refuses_them_and_is_unchanged(make, kw):
    gen, srv, st = make({0: LONG, 1: LONG}, state=NoFilterState, slots=2, chunk_frames=2, **kw)
    assert srv.row_filters is False
    conv = srv.conversation()
    for f in (dict(top_p=0.9), dict(min_p=0.1), dict(top_p=0.9, min_p=0.1), dict(top_p=1.0), dict(min_p=0.0)):
        with pytest.raises(ValueError, match=re.escape("serve(row_filters=True)")):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **f)
        with pytest.raises(ValueError, match=re.escape("serve(row_filters=True)")):
            srv.conversation(**f)
        with pytest.raises(ValueError, match=re.escape("serve(row_filters=True)")):
            conv.say("a", 0, max_audio_length_ms=MS, **f)
    assert srv.queued == 0 and conv._open is None
    r = srv.submit("a", 0, [], max_audio_length_ms=4 * 80)
    t = conv.say("b", 1, max_audio_length_ms=4 * 80)
    for _ in srv.run():
        pass
    assert r.done and t.done and (r.top_p, r.min_p) == (1.0, 0.0)
    want = (None, None) if kw else (0.9, 50)
    assert all(e[2:4] == want for e in st.log if e[0] in ("first", "frame"))


def test_row_filters_needs_row_sampling(make):
    with pytest.raises(ValueError, match="row_sampling=True"):
        make({0: LONG}, slots=2, row_filters=True)
    for f in (dict(top_p=0.9), dict(min_p=0.1)):
        with pytest.raises(ValueError, match=re.escape("serve(row_filters=True)")):
            make({0: LONG}, slots=2, row_sampling=True, **f)


def test_generate_calls_check_filters_before_they_take_the_caches():
    from csm.generator import Generator, filter_kwargs
    m = StubModel()
    resets = []
    m.reset_caches = lambda: resets.append(1)
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    assert filter_kwargs(1.0, 0.0) == {} and filter_kwargs(1, 0) == {} and filter_kwargs(0.9, 0.0) == {"top_p": 0.9, "min_p": 0.0}
    assert filter_kwargs([1.0, 0.5], 0.1, 2) == {"top_p": [1.0, 0.5], "min_p": 0.1}
    for bad in BAD:
        with pytest.raises(ValueError, match=re.escape(repr(list(bad.values())[0]))):
            gen.generate("a", 0, [], max_audio_length_ms=MS, **bad)
        with pytest.raises(ValueError, match=re.escape(repr(list(bad.values())[0]))):
            gen.generate_stream("a", 0, [], max_audio_length_ms=MS, **bad)
    for kw in (dict(top_p=[0.9, 0.8]), dict(min_p=[0.1] * 4), dict(top_p=()), dict(min_p="555")):
        with pytest.raises(ValueError, match="one value per utterance"):
            gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, **kw)
    with pytest.raises(ValueError, match="top_p must be"):
        gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, top_p=[0.5, 0.0, 0.7])
    with pytest.raises(ValueError, match="min_p must be"):
        gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, min_p=[0.5, 0.1, NAN])
    assert not resets and gen._run == 0


def test_serve_file_lines_carry_filters(tmp_path):
    from csm.cli.generate import line_filters, line_sampling, read_serve_file, serve_filters, serve_sampling
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "top_p": 0.9, "min_p": 0.05}\n'
                 '{"text": "two", "conversation": "c", "min_p": 1}\n'
                 '{"text": "three", "topk": 20}\n'
                 '{"text": "four", "seed": 2}\n')
    lines = read_serve_file(str(p))
    assert lines[0] == {"text": "one", "speaker": 0, "adapter": None, "seed": None, "top_p": 0.9, "min_p": 0.05}
    assert lines[1]["min_p"] == 1.0 and type(lines[1]["min_p"]) is float and "top_p" not in lines[1]
    assert [line_filters(ln) for ln in lines] == [{"top_p": 0.9, "min_p": 0.05}, {"min_p": 1.0}, {}, {}]
    assert line_sampling(lines[0]) == {}                                   # (the pair's keys stay the pair's)
    on = {"row_sampling": True, "row_filters": True, "top_p": 1.0, "min_p": 0.0}
    assert serve_filters(lines) == on
    assert serve_filters(lines[2:]) == {} and serve_sampling(lines[2:]) == {"row_sampling": True}      # no line names a filter
    assert serve_filters(lines[3:]) == {} and serve_sampling(lines[3:]) == {}                          # today's server
    assert serve_filters(lines[3:], 0.8, 0.0) == {**on, "top_p": 0.8}      # the command line's --top-p / --min-p ask for it too
    assert serve_filters(lines[3:], 1.0, 0.1) == {**on, "min_p": 0.1}
    for bad in ('{"text": "x", "top_p": "0.9"}', '{"text": "x", "min_p": true}', '{"text": "x", "top_k": 5}'):
        p.write_text(bad + "\n")
        with pytest.raises(ValueError, match="lines.jsonl:1"):
            read_serve_file(str(p))


def test_serve_file_makes_a_row_filters_server_only_when_asked(tmp_path):
    """``serve_to_wavs`` against a recording generator: the serve keywords and each submit / say's."""
    from csm.cli import generate as G
    calls = []
    keys = ("temperature", "topk", "top_p", "min_p")

    class Srv:
        queued, active = 0, []

        def submit(self, text, speaker, context, **kw):
            calls.append(("submit", text, {k: kw[k] for k in keys if k in kw}))
            return object()

        def conversation(self, **kw):
            calls.append(("conversation", {k: kw[k] for k in keys if k in kw}))
            return types.SimpleNamespace(say=lambda text, speaker, **kw: calls.append(
                ("say", text, {k: kw[k] for k in keys if k in kw})) or object())

    gen = types.SimpleNamespace(sample_rate=24000, load_adapter=None, serve=lambda **kw: calls.append(
        ("serve", {k: kw[k] for k in ("row_sampling", "row_filters", "top_p", "min_p") if k in kw})) or Srv())
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav")]
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one"}\n{"text": "two", "conversation": "c", "min_p": 0.2}\n{"text": "three", "top_p": 0.6, "topk": 9}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p), "--top-p", "0.9"]), [])
    assert calls == [("serve", {"row_sampling": True, "row_filters": True, "top_p": 0.9, "min_p": 0.0}), ("submit", "one", {}),
                     ("conversation", {}), ("say", "two", {"min_p": 0.2}), ("submit", "three", {"topk": 9, "top_p": 0.6})]
    del calls[:]
    p.write_text('{"text": "one"}\n{"text": "two", "topk": 3}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", {"row_sampling": True}), ("submit", "one", {}), ("submit", "two", {"topk": 3})]
    del calls[:]
    p.write_text('{"text": "one"}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", {}), ("submit", "one", {})]
    args = G.parse_args(base + ["--text", "x", "--top-p", "0.8", "--min-p", "0.05"])
    assert (args.top_p, args.min_p) == (0.8, 0.05)
    args = G.parse_args(base + ["--text", "x"])
    assert (args.top_p, args.min_p) == (1.0, 0.0)
