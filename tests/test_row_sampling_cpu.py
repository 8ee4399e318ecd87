"""Per-request sampling parameters, host side (``Generator.serve(row_sampling=True)``, csm/serving.py): every admitted request's
slot gets its resolved (temperature, topk) before its first frame, the frame calls get None, None, a default server is today's
server, bad requests raise before they queue; plus the new library entry point's declaration and the serve-file keys."""
import os
import re
import types

import pytest
import torch

K = 4                       # codebooks of the stub model
VOCAB = 64                  # its audio vocabulary
MAX_SEQ = 96
SPF = 4                     # samples per frame of the stub codec
MS = 40 * 80
LONG = list(range(1, 90))


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


class RowsCodec:
    sample_rate = 24000

    def encode(self, audio):
        T = audio.shape[-1] // SPF
        return (torch.arange(K * T).reshape(1, K, T) % 7) + 1

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(SPF, -1)

    def decode_stream_rows(self, slots=16, max_chunk_frames=32):
        return types.SimpleNamespace(open=lambda slot: None, step=lambda rows, codes: codes.float().sum(1).repeat_interleave(SPF, -1))


def _speaker(tk):
    """The speaker of the LAST text segment of a feed ("[<speaker>]text" through Tok: BOS, '[', the digit)."""
    start = int((tk[:, K] == 1).nonzero()[-1])
    return int(tk[start + 2, K]) - 3 - ord("0")


class State:
    """What BatchServer uses of DecodeState, recording every call in order.  Row b samples the script of the speaker of its
    latest feed (frame i = K copies of the script's i-th int, 0 = the EOS frame)."""
    scripts = {}
    made = []

    def __init__(self, engine, B, adapters=None, bank=None):
        self.B, self.log = B, []
        self.active_rows = list(range(B))
        self.active = torch.ones(B, dtype=torch.int32)
        self.script, self.at, self.sampling = [None] * B, [0] * B, [None] * B
        State.made.append(self)

    def _start(self, b, tk):
        self.script[b], self.at[b] = State.scripts[_speaker(tk)], 0

    def _next(self, rows):
        out = torch.full((self.B, K), 99, dtype=torch.int32)
        for b in rows:
            out[b] = self.script[b][self.at[b]]
            self.at[b] += 1
        return out

    def prefill_row(self, b, tk, mk):
        self._start(b, tk)
        self.log.append(("prefill", b))
        return torch.zeros(8)

    def append_rows(self, rows, tokens_list, masks_list):
        for b, tk in zip(rows, tokens_list):
            self._start(b, tk)
        self.log.append(("append_rows", tuple(rows)))
        return torch.zeros(len(rows), 8)

    def park_row(self, b, length):
        return ("parked", b, length)

    def resume_row(self, b, parked):
        self.log.append(("resume", b))

    def set_row_adapter(self, b, state):
        pass

    def new_row_generator(self, seed):
        return ["generator", seed]

    def set_row_seed(self, b, seed, generator=None):
        pass

    def set_row_sampling(self, b, temperature, topk):
        self.sampling[b] = (temperature, topk)
        self.log.append(("sampling", b, temperature, topk))

    def set_active(self, rows):
        self.active_rows = sorted(rows)
        self.active = torch.tensor([1 if b in rows else 0 for b in range(self.B)], dtype=torch.int32)

    def serve_first(self, last_h, rows, temperature, topk):
        self.log.append(("first", tuple(rows), temperature, topk, tuple(self.sampling[b] for b in rows)))
        return self._next(rows)

    def serve_frame(self, tokens, masks, temperature, topk):
        self.log.append(("frame", tuple(self.active_rows), temperature, topk))
        return self._next(self.active_rows)


class LegacyState(State):
    """A state from before per-row sampling (the stub of tests/test_serving_cpu.py has no such method)."""
    set_row_sampling = property()                                     # any access raises AttributeError


class StubModel:
    device = torch.device("cpu")

    def __init__(self):
        self.args = types.SimpleNamespace(audio_num_codebooks=K, audio_vocab_size=VOCAB)
        self.bb = types.SimpleNamespace(max_seq_len=MAX_SEQ)
        self.engine = types.SimpleNamespace(_need=lambda: None)
        self._decode_state = None

    def setup_caches(self, n):
        pass

    def reset_caches(self):
        self._decode_state = None


@pytest.fixture
def make(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    State.made, State.scripts = [], {}

    def _make(scripts, state=State, **kw):
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
    decl = re.search(r"\bint csm_sample_topk_rows\(([^;]*)\);", header)
    assert decl, "csm_sample_topk_rows is not declared in include/csm_hip.h"
    args = re.sub(r"\s+", " ", decl.group(1))
    assert args == ("const float* logits, const float* q, int* out, int rows, int V, int ldl, const int* topk, "
                    "const float* temperature, csm_stream_t stream")
    assert "csm_sample_topk_rows" in hip.EXPORTS and hasattr(hip.lib, "csm_sample_topk_rows")
    assert len(hip.lib.csm_sample_topk_rows.argtypes) == 9
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    assert callable(ops.sample_topk_rows) and callable(model.sample_topk_rows) and callable(DecodeState.set_row_sampling)


def test_every_admitted_slot_gets_its_resolved_pair_before_its_first_frame(make):
    gen, srv, st = make({s: LONG for s in range(6)}, slots=2, chunk_frames=2, temperature=0.8, topk=12, row_sampling=True)
    # the rows start with the server's pair (a free row samples too: the kernel runs on all of them)
    assert st.log == [("sampling", 0, 0.8, 12), ("sampling", 1, 0.8, 12)]
    del st.log[:]
    reqs = [srv.submit("a", 0, [], max_audio_length_ms=2 * 80),                                # the server's pair
            srv.submit("b", 1, [], max_audio_length_ms=4 * 80, temperature=0.5),               # one of the two
            srv.submit("c", 2, [], max_audio_length_ms=4 * 80, temperature=1.3, topk=1),       # waits for a slot
            srv.submit("d", 3, [], max_audio_length_ms=2 * 80, topk=VOCAB)]
    assert [(r.temperature, r.topk) for r in reqs] == [(0.8, 12), (0.5, 12), (1.3, 1), (0.8, VOCAB)]
    assert all(type(r.temperature) is float and type(r.topk) is int for r in reqs)
    for _ in srv.run():
        pass
    assert all(r.done for r in reqs)
    firsts = [e for e in st.log if e[0] == "first"]
    # each first frame is sampled with the joiners' own pairs already in their slots; c and d took the slots a and b left
    assert [(e[1], e[4]) for e in firsts] == [((0, 1), ((0.8, 12), (0.5, 12))), ((0,), ((1.3, 1),)), ((1,), ((0.8, VOCAB),))]
    for e in firsts:
        for b in e[1]:                                                     # ... set at admission: before the slot is filled and the tail runs
            i = st.log.index(e)
            assert [x[0] for x in st.log[:i] if x[0] in ("sampling", "prefill") and x[1] == b][-2:] == ["sampling", "prefill"]
    assert all(e[2:4] == (None, None) for e in st.log if e[0] in ("first", "frame"))
    assert sum(e[0] == "sampling" for e in st.log) == 4                    # once per admission, nothing else


def test_conversation_turns_carry_their_pair_from_slot_to_slot(make):
    gen, srv, st = make({0: [7, 8, 0] + [3] * 40, 1: LONG}, slots=2, chunk_frames=2, row_sampling=True)
    conv = srv.conversation(temperature=0.7, topk=8, seed=3)
    t1 = conv.say("one", 0, max_audio_length_ms=MS)
    assert (t1.temperature, t1.topk) == (0.7, 8)
    for _ in srv.run():
        pass
    assert t1.done
    blocker = srv.submit("x", 1, [], max_audio_length_ms=30 * 80)           # takes slot 0: turn 2 resumes in slot 1
    srv.step()
    del st.log[:]
    t2 = conv.say("two", 0, max_audio_length_ms=MS, topk=1)                 # say > conversation > server
    assert (t2.temperature, t2.topk) == (0.7, 1)
    srv.step()
    assert t2.slot == 1 and blocker.slot == 0
    first = [e for e in st.log if e[0] == "first"][0]
    assert first[1] == (1,) and first[4] == ((0.7, 1),) and ("resume", 1) in st.log[:st.log.index(first)]
    assert ("sampling", 1, 0.7, 1) in st.log[:st.log.index(first)]
    for _ in srv.run():
        pass
    t3 = conv.say("three", 0, max_audio_length_ms=MS)                      # back to the conversation's pair
    assert (t3.temperature, t3.topk) == (0.7, 8)
    plain = srv.conversation()
    assert (plain.temperature, plain.topk) == (0.9, 50)                    # nothing named: the server's


def test_default_server_is_todays_server(make):
    gen, srv, st = make({0: LONG, 1: LONG}, state=LegacyState, slots=2, chunk_frames=2, temperature=0.8, topk=12)
    assert srv.row_sampling is False
    r = srv.submit("a", 0, [], max_audio_length_ms=4 * 80)
    conv = srv.conversation()
    t = conv.say("b", 1, max_audio_length_ms=4 * 80)
    for _ in srv.run():
        pass
    assert r.done and t.done and (r.temperature, r.topk) == (0.8, 12) == (t.temperature, t.topk)
    calls = [e for e in st.log if e[0] in ("first", "frame")]
    assert calls and all(e[2:4] == (0.8, 12) for e in calls)
    assert not any(e[0] == "sampling" for e in st.log)


BAD = [dict(temperature=0), dict(temperature=0.0), dict(temperature=-0.5), dict(temperature=float("nan")),
       dict(temperature=float("inf")), dict(topk=0), dict(topk=-3), dict(topk=VOCAB + 1), dict(topk=2.5)]


def test_bad_requests_raise_before_they_queue(make):
    gen, srv, st = make({0: LONG}, slots=2, chunk_frames=2, row_sampling=True)
    conv = srv.conversation()
    for bad in BAD:
        value = repr(list(bad.values())[0])
        with pytest.raises(ValueError, match=re.escape(value)):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **bad)
        with pytest.raises(ValueError, match=re.escape(value)):
            srv.conversation(**bad)
        with pytest.raises(ValueError, match=re.escape(value)):
            conv.say("a", 0, max_audio_length_ms=MS, **bad)
        with pytest.raises(ValueError, match=re.escape(value)):            # the server's own defaults, under the same rule
            gen.serve(slots=2, chunk_frames=2, row_sampling=True, **{**dict(temperature=0.9, topk=10), **bad})
        srv._check()                                                       # (a refused server took nothing over)
    assert srv.queued == 0 and conv._open is None and conv.tokens.shape[0] == 0
    srv.submit("a", 0, [], max_audio_length_ms=MS, temperature=1, topk=VOCAB)      # the bounds themselves are fine
    assert srv.queued == 1


def test_a_default_server_refuses_request_parameters(make):
    gen, srv, st = make({0: LONG}, slots=2, chunk_frames=2)
    conv = srv.conversation()
    for kw in (dict(temperature=0.7), dict(topk=5), dict(temperature=0.7, topk=5)):
        with pytest.raises(ValueError, match=r"row_sampling=True"):
            srv.submit("a", 0, [], max_audio_length_ms=MS, **kw)
        with pytest.raises(ValueError, match=r"row_sampling=True"):
            srv.conversation(**kw)
        with pytest.raises(ValueError, match=r"row_sampling=True"):
            conv.say("a", 0, max_audio_length_ms=MS, **kw)
    assert srv.queued == 0 and conv._open is None and conv.tokens.shape[0] == 0


def test_set_row_sampling_rule():
    from csm.engine import check_sampling
    assert check_sampling(0.7, 5, VOCAB) == (0.7, 5) and check_sampling(1, VOCAB, VOCAB) == (1.0, VOCAB)
    assert check_sampling(0.7, 5.0, VOCAB) == (0.7, 5)                     # an integer value, whatever its type
    for bad in BAD:
        kw = dict(temperature=0.9, topk=10)
        kw.update(bad)
        with pytest.raises(ValueError, match=re.escape(repr(list(bad.values())[0]))):
            check_sampling(kw["temperature"], kw["topk"], VOCAB)
    for t, k in ((None, 5), ("warm", 5), (0.9, None), (0.9, "all"), (True, 5), (0.9, True)):
        with pytest.raises(ValueError):
            check_sampling(t, k, VOCAB)


def test_generate_batch_sequences_of_the_wrong_length():
    from csm.generator import Generator
    m = StubModel()
    resets = []
    m.reset_caches = lambda: resets.append(1)
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=RowsCodec())
    for kw in (dict(temperature=[0.9, 0.8]), dict(topk=[5, 6, 7, 8]), dict(temperature=[0.9, 0.8, 0.7], topk=[5]),
               dict(temperature=()), dict(topk="555")):
        with pytest.raises(ValueError, match="one value per utterance"):
            gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, **kw)
    with pytest.raises(ValueError, match="topk must be"):                  # the right length, a bad value
        gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, topk=[5, 0, 7])
    with pytest.raises(ValueError, match="temperature must be"):
        gen.generate_batch(["a", "b", "c"], [0, 1, 2], [[], [], []], max_audio_length_ms=MS, temperature=[0.5, 0.6, float("nan")])
    assert not resets and gen._run == 0                                    # refused before the caches were taken over


def test_serve_file_lines_carry_temperature_and_topk(tmp_path):
    from csm.cli.generate import line_sampling, read_serve_file, serve_sampling
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one", "temperature": 0.7, "topk": 20}\n'
                 '{"text": "two", "conversation": "c", "topk": 1}\n'
                 '{"text": "three", "conversation": "c", "temperature": 1}\n'
                 '{"text": "four", "seed": 2}\n')
    lines = read_serve_file(str(p))
    assert lines[0] == {"text": "one", "speaker": 0, "adapter": None, "seed": None, "temperature": 0.7, "topk": 20}
    assert lines[1] == {"text": "two", "speaker": 0, "adapter": None, "seed": None, "conversation": "c", "topk": 1}
    assert lines[2]["temperature"] == 1.0 and type(lines[2]["temperature"]) is float and "topk" not in lines[2]
    assert lines[3] == {"text": "four", "speaker": 0, "adapter": None, "seed": 2}
    assert [line_sampling(ln) for ln in lines] == [{"temperature": 0.7, "topk": 20}, {"topk": 1}, {"temperature": 1.0}, {}]
    assert serve_sampling(lines) == {"row_sampling": True}
    assert serve_sampling(lines[3:]) == {}                                 # no line names one: today's server
    for bad in ('{"text": "x", "topk": 2.5}', '{"text": "x", "topk": "5"}', '{"text": "x", "temperature": "hot"}',
                '{"text": "x", "temperature": true}'):
        p.write_text(bad + "\n")
        with pytest.raises(ValueError, match="lines.jsonl:1"):
            read_serve_file(str(p))


def test_serve_file_makes_a_row_sampling_server_only_when_a_line_asks(tmp_path, monkeypatch):
    """``serve_to_wavs`` against a recording generator: the serve keywords and each submit / say's."""
    from csm.cli import generate as G
    calls = []

    class Srv:
        queued, active = 0, []

        def submit(self, text, speaker, context, **kw):
            calls.append(("submit", text, {k: kw[k] for k in ("temperature", "topk") if k in kw}))
            return object()

        def conversation(self, **kw):
            calls.append(("conversation", {k: kw[k] for k in ("temperature", "topk") if k in kw}))
            return types.SimpleNamespace(say=lambda text, speaker, **kw: calls.append(
                ("say", text, {k: kw[k] for k in ("temperature", "topk") if k in kw})) or object())

    gen = types.SimpleNamespace(sample_rate=24000, load_adapter=None,
                                serve=lambda **kw: calls.append(("serve", kw.get("row_sampling", False))) or Srv())
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", str(tmp_path / "o.wav")]
    p = tmp_path / "lines.jsonl"
    p.write_text('{"text": "one"}\n{"text": "two", "conversation": "c", "topk": 1}\n{"text": "three", "temperature": 0.6}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", True), ("submit", "one", {}), ("conversation", {}), ("say", "two", {"topk": 1}),
                     ("submit", "three", {"temperature": 0.6})]
    del calls[:]
    p.write_text('{"text": "one"}\n')
    G.serve_to_wavs(gen, G.parse_args(base + ["--serve-file", str(p)]), [])
    assert calls == [("serve", False), ("submit", "one", {})]
