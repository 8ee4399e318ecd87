"""Per-request sampling statistics, host side: ``SampleStats``, the graph-key tag, ``Request.stats`` on a ``serve(stats=True)``
server against the stub decode state of tests/test_serve_streams_cpu.py (growth with the codes, the EOS cut, park / resume,
``cancel(heard_frames=)``), ``--stats-file``'s JSON in every mode, the recompute path's refusal, and the new entry point's
declaration and export."""
import json
import os
import re
import types

import pytest
import torch

from test_serve_streams_cpu import INF, K, State, StubModel, Tok, RowsCodec, _script, make  # noqa: F401  (make: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StatsState(State):
    """The stub state in statistics mode: a frame's statistics say which code each row drew - logprob = -code, entropy = code / 2,
    pmax = 1 / (1 + code) for every codebook of a row that sampled, junk (NaN) for the others."""
    enabled = 0

    def enable_stats(self):
        StatsState.enabled += 1
        self.stats_on = True

    def _next(self, rows):
        out = State._next(self, rows)
        self.last = torch.full((3, K, self.B), float("nan"))
        for b in rows:
            c = float(out[b, 0])
            self.last[:, :, b] = torch.tensor([-c, c / 2, 1 / (1 + c)]).view(3, 1)
        return out

    def frame_stats(self):
        assert getattr(self, "stats_on", False)
        return self.last.clone()


def _agrees(req):
    codes = req.codes()[0].float()
    assert len(req.stats) == codes.numel()
    assert torch.equal(req.stats.logprob, (-codes).view(-1, 1).expand(-1, K))
    assert torch.equal(req.stats.entropy, (codes / 2).view(-1, 1).expand(-1, K))
    assert torch.equal(req.stats.pmax, (1 / (1 + codes)).view(-1, 1).expand(-1, K))


def test_sample_stats_bookkeeping():
    from csm.sampling import SampleStats
    s = SampleStats(K)
    assert len(s) == 0 and s.logprob.shape == (0, K) and s.summary() == {
        "codebook0": {"logprob": [], "entropy": [], "pmax": []}, "frame_logprob": [], "mean_logprob": None}
    frames = [torch.arange(3 * K * 2, dtype=torch.float32).view(3, K, 2) + 100 * f for f in range(5)]
    t = SampleStats.of_frames(K, frames, b=1)
    assert len(t) == 5 and t.logprob.shape == t.entropy.shape == t.pmax.shape == (5, K)
    assert t.logprob[2].tolist() == [201.0 + 2 * i for i in range(K)] and t.pmax[0, 0] == 2 * K * 2 + 1
    s.extend(SampleStats.of_frames(K, frames[:2], b=1)).extend(SampleStats.of_frames(K, frames[2:], b=1))
    assert torch.equal(s.logprob, t.logprob) and torch.equal(s.pmax, t.pmax)
    assert len(s.cut(3)) == 3 and len(s.cut(7)) == 3 and len(s.cut(0)) == 0
    d = t.summary()
    assert sorted(d) == ["codebook0", "frame_logprob", "mean_logprob"] and sorted(d["codebook0"]) == ["entropy", "logprob", "pmax"]
    assert d["codebook0"]["logprob"] == [1.0 + 100 * f for f in range(5)]
    assert d["frame_logprob"] == [float(t.logprob[f].sum()) for f in range(5)]
    assert d["mean_logprob"] == pytest.approx(float(t.logprob.mean()))
    json.dumps(d)


def test_graph_key_carries_the_tag():
    from csm.sampling import RowSampler
    s = RowSampler(2, K, 67, "cpu")
    assert s.graph_key(0.9, 50) == (0.9, 50) and s.graph_key(None, None) == (None, None)
    s.stats = True
    assert s.graph_key(0.9, 50) == (0.9, 50, "stats") and s.graph_key(None, None) == (None, None, "stats")
    s.stats = False
    s.write(0, 1, 0.8, 12)
    s.write(0, 2, 0.9, 0.0)
    assert s.graph_key(None, None) == (None, None, "filters")
    s.stats = True
    assert s.graph_key(None, None) == (None, None, "filters", "stats")


def test_request_stats_grow_with_the_codes_and_stop_at_eos(make):
    StatsState.enabled = 0
    gen, srv, st, codec = make({0: _script(0, frames=6), 1: _script(1, frames=9), 2: _script(2)}, state=StatsState, slots=4,
                               chunk_frames=4, stats=True)
    assert StatsState.enabled == 1 and srv.sample_stats and srv.stats["steps"] == 0          # (server.stats: the counters)
    a, b = srv.submit("x", 0, [], max_audio_length_ms=INF), srv.submit("x", 1, [], max_audio_length_ms=INF)
    c = srv.submit("x", 2, [], max_audio_length_ms=5 * 80)
    assert len(a.stats) == 0
    srv.step()
    assert [len(r.stats) for r in (a, b, c)] == [4, 4, 4]
    d = srv.submit("x", 2, [], max_audio_length_ms=3 * 80)                                    # joins at a chunk boundary
    srv.step()
    assert [len(r.stats) for r in (a, b, c, d)] == [6, 8, 5, 3] and a.done and c.done and d.done
    for _ in srv.run():
        pass
    assert b.done and len(b.stats) == 9
    for r in (a, b, c, d):
        _agrees(r)


def test_server_without_stats_is_the_server_it_was(make):
    StatsState.enabled = 0
    gen, srv, st, codec = make({0: _script(0, frames=3)}, state=StatsState, slots=2, chunk_frames=4)
    r = srv.submit("x", 0, [], max_audio_length_ms=INF)
    for _ in srv.run():
        pass
    assert r.done and r.stats is None and not srv.sample_stats and StatsState.enabled == 0


def test_stats_survive_park_and_resume_and_cancel_cuts_them(make):
    scripts = {s: _script(s) for s in range(6)}
    gen, srv, st, codec = make(scripts, state=StatsState, slots=2, streams=6, chunk_frames=4, stats=True)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(6)]
    for _ in range(9):
        srv.step()
    assert sum(r.preemptions for r in reqs) >= 6 and all(len(r.stats) >= 8 for r in reqs)
    for r in reqs:
        _agrees(r)
    r = max(reqs, key=lambda q: len(q.stats))
    n = len(r.stats)
    srv.cancel(r, heard_frames=n - 3)
    assert r.done and r.cancelled and len(r.stats) == n - 3
    assert torch.equal(r.stats.logprob[:, 0], -r.codes()[0, :n - 3].float())
    q = reqs[0] if reqs[0] is not r else reqs[1]
    m = len(q.stats)
    srv.cancel(q)                                                                             # None: every frame emitted stays
    assert q.done and len(q.stats) == m
    with pytest.raises(ValueError, match="heard_frames"):
        srv.cancel(reqs[2] if reqs[2] not in (r, q) else reqs[3], heard_frames=-1)


def test_recompute_path_refuses_return_stats():
    from csm.generator import Generator
    model = StubModel()
    model.use_kv_cache = False
    gen = Generator(model, text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    for call in (lambda: gen.generate("x", 0, [], return_stats=True), lambda: gen.generate_stream("x", 0, [], return_stats=True),
                 lambda: gen.generate_batch(["x"], [0], [[]], return_stats=True), lambda: gen.serve(stats=True)):
        with pytest.raises(ValueError, match="use_kv_cache = False.*return_stats"):
            call()
    import inspect
    from csm.conversation import Conversation
    from csm.engine import Engine
    for fn in (Generator.generate, Generator.generate_stream, Generator.generate_batch, Conversation.generate,
               Conversation.generate_stream):
        assert inspect.signature(fn).parameters["return_stats"].default is False, fn
    assert inspect.signature(Generator.serve).parameters["stats"].default is False
    src = inspect.getsource(Engine.generate_frame)
    assert "has no return_stats" in src


# -------------------------------------------------------------------------------------------------------------- command line
def _base(tmp_path):
    return ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav"),
            "--stats-file", str(tmp_path / "s" / "stats.jsonl")]


def _read(tmp_path):
    return [json.loads(ln) for ln in (tmp_path / "s" / "stats.jsonl").read_text().splitlines()]


def _stats(frames, first=0):
    from csm.sampling import SampleStats
    return SampleStats.of_frames(K, [torch.full((3, K, 1), float(-(first + f))) for f in range(frames)])


def test_stats_file_of_generate_stream_and_turns(tmp_path, monkeypatch):
    from csm.cli import generate as G
    calls = []

    def generate(**kw):
        calls.append(("generate", kw.get("return_stats")))
        return torch.zeros(8), _stats(3)

    def generate_stream(**kw):
        calls.append(("stream", kw.get("return_stats")))
        return iter([(torch.zeros(4), _stats(2)), (torch.zeros(4), _stats(1, 2))])

    class Conv:
        def generate(self, text, spk, **kw):
            calls.append(("turn", text, kw.get("return_stats")))
            return torch.zeros(4), _stats(2 if text == "x" else 1)

        def generate_stream(self, text, spk, **kw):
            calls.append(("turn_stream", text, kw.get("return_stats")))
            return iter([(torch.zeros(4), _stats(2)), (torch.zeros(2), _stats(1, 2))])

    from csm.generator import Generator
    model = types.SimpleNamespace(args=types.SimpleNamespace(audio_num_codebooks=K))
    gen = types.SimpleNamespace(sample_rate=24000, _model=model, generate=generate, generate_stream=generate_stream,
                                conversation=lambda **kw: Conv())
    gen.save_wav = lambda path, audio, **kw: Generator.save_wav(gen, path, audio, **kw)
    monkeypatch.setattr(G, "load_csm_1b", lambda *a, **kw: gen)
    want3 = {"codebook0": {"logprob": [0.0, -1.0, -2.0], "entropy": [0.0, -1.0, -2.0], "pmax": [0.0, -1.0, -2.0]},
             "frame_logprob": [0.0, -1.0 * K, -2.0 * K], "mean_logprob": -1.0}
    assert G.main(_base(tmp_path) + ["--text", "x"]) == 0
    assert calls == [("generate", True)] and _read(tmp_path) == [want3]
    assert G.main(_base(tmp_path) + ["--text", "x", "--stream"]) == 0
    assert calls[-1] == ("stream", True) and _read(tmp_path) == [want3]                      # the chunks' statistics, joined
    assert G.main(_base(tmp_path) + ["--text", "x", "--next-text", "y"]) == 0
    got = _read(tmp_path)
    assert [o["turn"] for o in got] == [0, 1] and got[0]["frame_logprob"] == [0.0, -1.0 * K] and got[1]["frame_logprob"] == [0.0]
    assert G.main(_base(tmp_path) + ["--text", "x", "--next-text", "y", "--stream"]) == 0
    got = _read(tmp_path)
    assert [o["turn"] for o in got] == [0, 1] and all(o["frame_logprob"] == want3["frame_logprob"] for o in got)
    assert all(sorted(o) == ["codebook0", "frame_logprob", "mean_logprob", "turn"] for o in got)
    del calls[:]
    args = G.parse_args([a for a in _base(tmp_path)[:-2]] + ["--text", "x"])                 # without the flag: the calls they were
    assert args.stats_file is None and G.stats_kw(args) == {}


def test_stats_file_of_a_serve_file(tmp_path, make):
    from csm.cli import generate as G
    gen, _, _, _ = make({0: _script(0, frames=6), 1: _script(1, frames=3)}, state=StatsState, slots=2, chunk_frames=4, stats=True)
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "speaker": 0}\n{"text": "two", "speaker": 1}\n')
    kept = {}
    serve = gen.serve
    gen.serve = lambda **kw: kept.setdefault("srv", serve(**{**kw, "slots": 2}))
    assert G.serve_to_wavs(gen, G.parse_args(_base(tmp_path) + ["--serve-file", str(p), "--max-audio-length-ms", str(INF)]), []) == 0
    assert kept["srv"].sample_stats
    got = _read(tmp_path)
    assert [o["line"] for o in got] == [0, 1]
    assert got[0]["codebook0"]["logprob"] == [-(1000.0 + i) for i in range(6)] and len(got[1]["frame_logprob"]) == 3
    assert got[1]["frame_logprob"] == [-K * (2000.0 + i) for i in range(3)]
    assert got[1]["mean_logprob"] == pytest.approx(-2001.0)
    assert all(sorted(o) == ["codebook0", "frame_logprob", "line", "mean_logprob"] for o in got)


# ------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "csm_hip.h")).read()
    decl = re.search(r"\bint csm_sample_stats_rows\(([^;]*)\);", header)
    assert decl, "csm_sample_stats_rows is not declared in include/csm_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 9 and params[0] == "const float* logits" and params[1] == "const int* codes"
    assert params[2:5] == ["float* logprob", "float* entropy", "float* pmax"] and params[-1] == "csm_stream_t stream"
    from csm import hip
    from csm.hip import ops
    assert "csm_sample_stats_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_sample_stats_rows")
    assert len(hip.lib.csm_sample_stats_rows.argtypes) == 9 and callable(ops.sample_stats_rows)
    # refusals need no device: nothing is launched
    f, i = torch.zeros(4), torch.zeros(1, dtype=torch.int32)
    for args in ((None, i.data_ptr(), f.data_ptr(), None, None, 1, 4, 4), (f.data_ptr(), None, f.data_ptr(), None, None, 1, 4, 4),
                 (f.data_ptr(), i.data_ptr(), None, None, None, 1, 4, 4), (f.data_ptr(), i.data_ptr(), f.data_ptr(), None, None, 0, 4, 4),
                 (f.data_ptr(), i.data_ptr(), f.data_ptr(), None, None, 1, 0, 4), (f.data_ptr(), i.data_ptr(), f.data_ptr(), None, None, 1, 4097, 4097),
                 (f.data_ptr(), i.data_ptr(), f.data_ptr(), None, None, 1, 4, 3), (f.data_ptr() + 2, i.data_ptr(), f.data_ptr(), None, None, 1, 4, 4)):
        assert hip.lib.csm_sample_stats_rows(*args, None) == 1, args
        assert b"csm_sample_stats_rows" in hip.lib.csm_last_error()
