"""The shared cases of the processed rows sampler (tests/sampling_processors_ref.py): every row's thresholds clear the derived
bounds of tests/sampling_filters_ref.py by its ``HEADROOM`` on the penalised logits, every winner is decisive, the penalty changes
winners and kept sets, and the rows it must not touch are untouched - so the GPU test may ask for the reference's winner and kept
set exactly.  Plus the host side: ``check_processors``, per-codebook values, and say > conversation > server on a
``row_processors`` server."""
import math
import os
import re

import pytest
import torch

import sampling_filters_ref as R
import sampling_processors_ref as P
from test_row_sampling_cpu import K, LONG, MS, VOCAB, RowsCodec, State, StubModel, Tok

NAN, INF = float("nan"), float("inf")
IDENTITY_ROWS = [r for r in range(R.ROWS) if P.PEN[r] == 1.0 or P.depth(r) == 0]


def test_the_case_table_covers_what_it_says():
    assert len(P.PEN) == len(P.WINDOW) == len(P.FRAME) == R.ROWS
    assert IDENTITY_ROWS == [10, 11, 15] and P.PEN[10] == 1.0 and P.WINDOW[11] == 0 and P.FRAME[15] == 0
    assert any(P.FRAME[r] < P.WINDOW[r] and P.FRAME[r] > 0 for r in range(R.ROWS))                  # a frame below the window
    full = [r for r in range(R.ROWS) if P.depth(r) == 64]
    assert full and all((P.FRAME[r] - 64) % 64 == P.FRAME[r] % 64 for r in full)                   # oldest slot read = slot written
    assert any(P.FRAME[r] % 64 < P.depth(r) for r in range(R.ROWS) if P.FRAME[r] >= 64)            # the window wraps around
    assert any(p < 1.0 for p in P.PEN)


@pytest.mark.parametrize("V", R.VS)
def test_rings_hold_the_window_and_poison_elsewhere(V):
    c = P.cases(V)[("drawn", "both")]
    for r in range(R.ROWS):
        entries, poison = P.window_entries(c["x"][r], c["topk"][r], r)
        n, f = P.depth(r), P.FRAME[r]
        reached = {(f - 1 - j) % 64 for j in range(n)}
        for s in range(64):
            if s not in reached:
                assert int(c["hist"][r, s]) == poison, (r, s)
        got = [int(c["hist"][r, (f - 1 - j) % 64]) for j in range(n)]
        assert got == entries[:n], r
        if n >= 10:                                                       # the argmax twice, and three ids out of range
            assert entries[0] == entries[6] and entries[7] == -1 and entries[8] == V and entries[9] == 2 ** 30
            assert float(c["x"][r, entries[5]]) < 0                       # a negative logit


@pytest.mark.parametrize("V", R.VS)
def test_penalty_is_one_fp32_operation_on_the_window_ids_only(V):
    c = P.cases(V)[("drawn", "top_p")]
    for r in range(R.ROWS):
        x, xp = c["x"][r], c["xp"][r]
        assert xp.dtype == torch.float32
        changed = set((x != xp).nonzero().view(-1).tolist())
        n, f = P.depth(r), P.FRAME[r]
        ids = {int(c["hist"][r, (f - 1 - j) % 64]) for j in range(n)}
        ids = {t for t in ids if 0 <= t < V}
        if r in IDENTITY_ROWS:
            assert not changed, r
            continue
        assert changed <= ids and changed, r                              # (an id whose logit is 0 would not change)
        rep = torch.tensor(P.PEN[r], dtype=torch.float32)
        for t in ids:
            want = x[t] / rep if float(x[t]) > 0 else x[t] * rep
            assert float(xp[t]) == float(want), (r, t)                    # once: an id that is in the window twice included


def test_case_margins_clear_the_derived_bounds_and_the_penalty_matters():
    worst = [math.inf, math.inf, math.inf]
    rows = winners = kept = 0
    for V in R.VS:
        base = R.cases(V)
        for (name, kind), c in P.cases(V).items():
            for r, (ref, raw) in enumerate(zip(c["ref"], c["raw"])):
                where = (V, name, kind, r)
                rows += 1
                assert 0.0 < c["top_p"][r] <= 1.0 and 0.0 <= c["min_p"][r] <= 1.0, where
                assert ref["topp_margin"] >= R.HEADROOM * ref["topp_bound"], (where, ref["topp_margin"], ref["topp_bound"])
                assert ref["minp_margin"] >= R.HEADROOM * ref["minp_bound"], (where, ref["minp_margin"], ref["minp_bound"])
                assert ref["runner_up"] >= 1.001, (where, ref["runner_up"])                        # (the filters test's bar)
                # the boundary probes of the GPU test are decisive, as in the filters cases
                last = ref["last_kept"][0]
                others = torch.cat([torch.from_numpy(ref["p"][:last]), torch.from_numpy(ref["p"][last + 1:])]) / torch.cat(
                    [c["q"][r, :last], c["q"][r, last + 1:]]).double()
                assert ref["p"][last] / 1e-30 >= 1e3 * float(others.max()) and ref["p"][last] >= 1e-30, where
                worst = [min(worst[0], ref["topp_margin"] / ref["topp_bound"]), min(worst[1], ref["minp_margin"] / ref["minp_bound"]),
                         min(worst[2], ref["runner_up"])]
                winners += ref["winner"] != raw["winner"]
                kept += not (ref["N"] == raw["N"]).all()
                if r in IDENTITY_ROWS:                                    # r = 1 or n = 0: the unpenalised draw, and the filters case
                    assert ref["winner"] == raw["winner"] and (ref["N"] == raw["N"]).all(), where
                    old = base[(name, kind)]["ref"][r]
                    assert (c["top_p"][r], c["min_p"][r]) == (base[(name, kind)]["top_p"][r], base[(name, kind)]["min_p"][r]), where
                    assert ref["winner"] == old["winner"] and (ref["N"] == old["N"]).all(), where
    print("rows %d, margins / bound: top-p %.1fx, min-p %.1fx; runner-up %.4f; winners changed %d, kept sets changed %d"
          % (rows, worst[0], worst[1], worst[2], winners, kept))
    assert rows == 288 and winners >= 60 and kept >= 150, (rows, winners, kept)


# ---------------------------------------------------------------------------------------------------------------- host side
def test_check_processors_rule():
    from csm.engine import check_processors
    assert check_processors(1, 64) == (1.0, 64) and check_processors(100.0, 0) == (100.0, 0) and check_processors(0.5, 7.0) == (0.5, 7)
    assert isinstance(check_processors(2, 3)[0], float) and isinstance(check_processors(2, 3.0)[1], int)
    for bad in (0, 0.0, -1.3, 100.5, NAN, INF, -INF, True, "1.3", None, [1.3]):
        with pytest.raises(ValueError, match="repetition_penalty"):
            check_processors(bad, 16)
    for bad in (-1, 65, 1.5, NAN, INF, True, "16", None, [16]):
        with pytest.raises(ValueError, match="repetition_window"):
            check_processors(1.3, bad)


def test_check_row_processors_takes_numbers_or_one_per_codebook():
    from csm.engine import check_row_processors
    six = check_row_processors(K, VOCAB, 0.9, [50, 20, 20, 20], 1.0, 0.0, (1.3, 1.0, 1.0, 1.0), 16)
    assert six == ((0.9,) * K, (50, 20, 20, 20), (1.0,) * K, (0.0,) * K, (1.3, 1.0, 1.0, 1.0), (16,) * K)
    for bad in (dict(temperature=[0.9] * (K - 1)), dict(topk=[50] * (K + 1)), dict(repetition_penalty=[1.3, 0, 1.0, 1.0]),
                dict(repetition_window=[16, 16, 65, 16]), dict(top_p=[1.0, 1.0, 1.5, 1.0]), dict(topk=[50, VOCAB + 1, 1, 1]),
                dict(temperature=[[0.9] * K]), dict(min_p="0.1")):
        kw = dict(temperature=0.9, topk=50, top_p=1.0, min_p=0.0, repetition_penalty=1.0, repetition_window=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_row_processors(K, VOCAB, **kw)


def test_entry_point_declared_exported_and_wired():
    from csm import hip, models
    from csm.engine import DecodeState
    from csm.hip import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csm_hip.h")).read()
    decl = re.search(r"\bint csm_sample_processed_rows\(([^;]*)\);", header)
    assert decl, "csm_sample_processed_rows is not declared in include/csm_hip.h"
    args = re.sub(r"\s+", " ", decl.group(1))
    assert args == ("const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk, "
                    "const float* temperature, const float* top_p, const float* min_p, const float* penalty, const int* window, "
                    "int* hist, int ldh, int* frame, const int* live, int advance, csm_stream_t stream")
    assert "csm_sample_processed_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_sample_processed_rows")
    assert len(hip.lib.csm_sample_processed_rows.argtypes) == 18
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    assert callable(ops.sample_processed_rows) and callable(models.sample_processed_rows)
    assert callable(DecodeState.set_row_processors) and callable(DecodeState.reset_row_history)


class ProcState(State):
    """The recording state of the row-sampling test, plus the processors."""

    def __init__(self, engine, B, adapters=None, bank=None):
        super().__init__(engine, B, adapters, bank)
        self.proc = [None] * B

    def set_row_processors(self, b, *six):
        self.proc[b] = six
        self.log.append(("processors", b) + six)

    def reset_row_history(self, b):
        self.log.append(("reset", b))

    def set_row_filters(self, b, top_p, min_p):
        self.log.append(("filters", b, top_p, min_p))

    def serve_first(self, last_h, rows, temperature, topk):
        self.log.append(("first-processors", tuple(rows), tuple(self.proc[b] for b in rows)))
        return super().serve_first(last_h, rows, temperature, topk)


@pytest.fixture
def make(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    State.made, State.scripts = [], {}

    def _make(scripts, state=ProcState, **kw):
        monkeypatch.setattr(S, "DecodeState", state)
        State.scripts = scripts
        gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
        return gen, gen.serve(**kw), State.made[-1]
    return _make


SERVER = dict(slots=2, chunk_frames=2, temperature=0.8, topk=12, row_sampling=True, row_processors=True, top_p=0.9, min_p=0.05,
              repetition_penalty=1.2, repetition_window=32)
DEFAULT = (0.8, 12, 0.9, 0.05, 1.2, 32)


def _six(req):
    return (req.temperature, req.topk, req.top_p, req.min_p, req.repetition_penalty, req.repetition_window)


def test_say_over_conversation_over_server_and_every_joining_row_is_set_and_reset(make):
    gen, srv, st = make({s: LONG for s in range(6)}, **SERVER)
    assert srv.row_processors and srv.row_filters and srv.row_sampling
    # every row starts with the server's six (before the first capture), through the processors alone
    assert st.log == [("processors", 0) + DEFAULT, ("processors", 1) + DEFAULT]
    acoustic = [0.8, 0.6, 0.6, 0.6]
    plain = srv.submit("a", 0, [], max_audio_length_ms=2 * 80)
    own = srv.submit("b", 1, [], max_audio_length_ms=2 * 80, temperature=acoustic, repetition_penalty=1.5, repetition_window=[8, 8, 8, 8])
    assert _six(plain) == DEFAULT
    assert _six(own) == ((0.8, 0.6, 0.6, 0.6), 12, 0.9, 0.05, 1.5, 8)      # one number where the codebooks agree, K values where not
    conv = srv.conversation(topk=[12, 5, 5, 5], repetition_penalty=1.4, seed=3)
    assert (conv.topk, conv.repetition_penalty, conv.repetition_window, conv.temperature) == ((12, 5, 5, 5), 1.4, 32, 0.8)
    del st.log[:]
    for _ in srv.run():
        pass
    admitted = [e for e in st.log if e[0] in ("processors", "reset", "filters", "sampling")]
    assert admitted == [("processors", 0) + _six(plain), ("reset", 0), ("processors", 1) + _six(own), ("reset", 1)]
    first = next(e for e in st.log if e[0] == "first-processors")
    assert first[1] == (0, 1) and first[2] == (_six(plain), _six(own))    # written before the first frame
    assert all(e[2:4] == (None, None) for e in st.log if e[0] in ("first", "frame"))
    # a conversation: its own defaults over the server's, a turn's over the conversation's
    t1 = conv.say("one", 2, max_audio_length_ms=2 * 80)
    assert _six(t1) == (0.8, (12, 5, 5, 5), 0.9, 0.05, 1.4, 32)
    for _ in srv.run():
        pass
    blocker = srv.submit("x", 1, [], max_audio_length_ms=30 * 80)           # takes slot 0: turn 2 resumes in slot 1
    srv.step()
    del st.log[:]
    t2 = conv.say("two", 2, max_audio_length_ms=6 * 80, repetition_penalty=2.0, topk=7, repetition_window=0)
    assert _six(t2) == (0.8, 7, 0.9, 0.05, 2.0, 0)
    srv.step()
    assert t2.slot == 1 and blocker.slot == 0
    assert ("resume", 1) in st.log                                          # a resumed turn is set and reset like any joining row
    assert [e for e in st.log if e[0] in ("processors", "reset")] == [("processors", 1) + _six(t2), ("reset", 1)]
    t3_defaults = srv.conversation()
    assert _six(t3_defaults.say("three", 3, max_audio_length_ms=2 * 80)) == DEFAULT


def test_bad_values_raise_at_the_call_and_queue_nothing(make):
    gen, srv, st = make({s: LONG for s in range(6)}, **SERVER)
    conv = srv.conversation()
    bad = [dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=100.5), dict(repetition_penalty=NAN),
           dict(repetition_penalty=INF), dict(repetition_penalty=True), dict(repetition_window=65), dict(repetition_window=-1),
           dict(repetition_window=1.5), dict(temperature=[0.9] * (K + 1)), dict(topk=[5] * (K - 1)), dict(top_p=[1.0, 1.0, 0.0, 1.0]),
           dict(min_p=[0.0] * (K + 2)), dict(repetition_penalty=[1.3] * (K - 1)), dict(repetition_window=[16, 16, 16, 70])]
    for kw in bad:
        with pytest.raises(ValueError):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError):
            srv.conversation(**kw)
        with pytest.raises(ValueError):
            conv.say("a", 0, max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError):
            gen.serve(**{**SERVER, **kw})
        srv._check()                                                       # (a refused server took nothing over)
    assert srv.queued == 0 and conv._open is None and conv.tokens.shape[0] == 0


def test_a_server_without_row_processors_says_which_flag_is_missing(make):
    from test_row_filters_cpu import FilterState
    with pytest.raises(ValueError, match="row_sampling=True"):
        make({}, state=ProcState, row_processors=True)
    for kw in (dict(repetition_penalty=1.3), dict(repetition_window=16), dict(temperature=[0.9] * K)):
        with pytest.raises(ValueError, match="row_processors=True"):
            make({}, state=FilterState, row_sampling=True, row_filters=True, **kw)
    gen, srv, st = make({s: LONG for s in range(6)}, state=FilterState, slots=2, chunk_frames=2, row_sampling=True, row_filters=True)
    assert srv.row_processors is False
    conv = srv.conversation()
    for kw in (dict(repetition_penalty=1.3), dict(repetition_window=16), dict(repetition_penalty=1.0), dict(temperature=[0.9] * K),
               dict(topk=[5] * K), dict(top_p=[0.9] * K), dict(min_p=[0.1] * K)):
        with pytest.raises(ValueError, match="row_processors=True"):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError, match="row_processors=True"):
            srv.conversation(**kw)
        with pytest.raises(ValueError, match="row_processors=True"):
            conv.say("a", 0, max_audio_length_ms=MS, **kw)
    assert srv.queued == 0 and conv._open is None
    # ... and is the server it was: the pair and the filters, no processors call
    r = srv.submit("a", 0, [], max_audio_length_ms=2 * 80, top_p=0.8)
    assert _six(r) == (0.9, 50, 0.8, 0.0, 1.0, 64)
    for _ in srv.run():
        pass
    assert not [e for e in st.log if e[0] in ("processors", "reset")]


def test_generation_keywords_are_todays_at_the_defaults():
    from csm.generator import Generator, sampling_kwargs
    gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    assert sampling_kwargs(gen, 0.9, 50, 1.0, 0.0) == (0.9, 50, {})
    assert sampling_kwargs(gen, 0.9, 50, 0.9, 0.0, 1.0, 64) == (0.9, 50, {"top_p": 0.9, "min_p": 0.0})
    t, k, kw = sampling_kwargs(gen, 0.9, [50, 20, 20, 20], 1.0, 0.0, 1.3, 16)
    assert (t, k) == ([0.9], [[50, 20, 20, 20]])
    assert kw == {"top_p": [1.0], "min_p": [0.0], "repetition_penalty": [1.3], "repetition_window": [16]}
    # a batch: a flat list of B numbers is one value per utterance and, alone, today's path
    assert sampling_kwargs(gen, [0.9, 0.7], 50, 1.0, 0.0, B=2) == ([0.9, 0.7], 50, {})
    t, k, kw = sampling_kwargs(gen, [[0.9, 0.7, 0.7, 0.7], 0.8], 50, 1.0, 0.0, [1.4, 1.0], 64, B=2)
    assert t == [[0.9, 0.7, 0.7, 0.7], 0.8] and k == [50, 50] and kw["repetition_penalty"] == [1.4, 1.0]
    assert kw["repetition_window"] == [64, 64]
    for bad in (dict(repetition_penalty=0), dict(repetition_window=65), dict(temperature=[0.9] * (K + 1)), dict(topk=[5] * (K - 1))):
        args = dict(temperature=0.9, topk=50, top_p=1.0, min_p=0.0, repetition_penalty=1.0, repetition_window=64)
        args.update(bad)
        with pytest.raises(ValueError):
            sampling_kwargs(gen, **args)
    with pytest.raises(ValueError):
        sampling_kwargs(gen, 0.9, 50, 1.0, 0.0, [1.3, 1.3, 1.3], 64, B=2)


# -------------------------------------------------------------------------------------------------------------- command line
def test_command_line_flags_and_serve_file_keys(tmp_path):
    import types
    from csm.cli import generate as G
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav")]
    args = G.parse_args(base + ["--text", "x"])
    assert (args.repetition_penalty, args.repetition_window, args.acoustic_temperature, args.acoustic_topk) == (1.0, 64, None, None)
    assert G.sampling_kw(args, K) == dict(temperature=0.9, topk=50, top_p=1.0, min_p=0.0) and not G.uses_processors(args)
    args = G.parse_args(base + ["--text", "x", "--repetition-penalty", "1.3", "--repetition-window", "16", "--acoustic-temperature",
                                "0.6", "--acoustic-topk", "20", "--top-p", "0.9"])
    assert G.uses_processors(args)
    assert G.sampling_kw(args, lambda: K) == dict(temperature=[0.9, 0.6, 0.6, 0.6], topk=[50, 20, 20, 20], top_p=0.9, min_p=0.0,
                                                  repetition_penalty=1.3, repetition_window=16)
    # the serve file: the two keys, a list of K numbers for the four others, a wrong length refused when the file is read
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "repetition_penalty": 1.4}\n{"text": "two", "conversation": "c", "repetition_window": 8, '
                 '"temperature": [0.9, 0.6, 0.6, 0.6]}\n{"text": "three", "topk": [9, 3, 3, 3], "top_p": 0.6}\n')
    lines = G.read_serve_file(str(p), K)
    assert lines[0]["repetition_penalty"] == 1.4 and lines[1]["repetition_window"] == 8
    assert lines[1]["temperature"] == [0.9, 0.6, 0.6, 0.6] and lines[2]["topk"] == [9, 3, 3, 3]
    for bad in ('{"text": "x", "temperature": [0.9, 0.6]}', '{"text": "x", "topk": [5, 5, 5, 5, 5]}', '{"text": "x", "topk": [5, 5, 5, 0.5]}',
                '{"text": "x", "repetition_penalty": "1.3"}', '{"text": "x", "repetition_window": 1.5}',
                '{"text": "x", "top_p": [0.9, true, 0.9, 0.9]}', '{"text": "x", "repetition_penalty": [1.3, 1.3, 1.3, 1.3]}'):
        q = tmp_path / "bad.jsonl"
        q.write_text(bad + "\n")
        with pytest.raises(ValueError, match="bad.jsonl:1"):
            G.read_serve_file(str(q), K)
    # ``serve_to_wavs`` against a recording generator: the serve keywords and each submit / say's
    calls = []
    keys = ("temperature", "topk", "top_p", "min_p", "repetition_penalty", "repetition_window")

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
        ("serve", {k: kw[k] for k in ("row_sampling", "row_filters", "row_processors") + keys if k in kw})) or Srv())
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p), "--acoustic-topk", "7"]), [])
    assert calls == [("serve", dict(row_sampling=True, row_filters=True, row_processors=True, temperature=0.9, topk=[50, 7, 7, 7],
                                    top_p=1.0, min_p=0.0)),
                     ("submit", "one", {"repetition_penalty": 1.4}), ("conversation", {}),
                     ("say", "two", {"temperature": [0.9, 0.6, 0.6, 0.6], "repetition_window": 8}),
                     ("submit", "three", {"topk": [9, 3, 3, 3], "top_p": 0.6})]
    del calls[:]
    p.write_text('{"text": "one"}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p), "--repetition-penalty", "1.2"]), [])
    assert calls == [("serve", dict(row_sampling=True, row_processors=True, temperature=0.9, topk=50, top_p=1.0, min_p=0.0,
                                    repetition_penalty=1.2, repetition_window=64)), ("submit", "one", {})]
    del calls[:]
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", dict(temperature=0.9, topk=50)), ("submit", "one", {})]      # nothing named: the server it was
