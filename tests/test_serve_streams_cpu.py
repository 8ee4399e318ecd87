"""More listeners than slots, host side: the schedule of ``serve(streams=)`` (csm/serving.py) against a stub decode state that
models each row's cache as the frames fed to it, with ``park_rows`` / ``resume_rows`` that log, a stub rows codec with
``state_slots``, and a fake clock and sleep.  The stub state checks on every frame that a row is fed the frame it sampled last,
so a request that comes back from a park with anything but its own state fails there."""
import os
import re
import types

import pytest
import torch

import serve_streams_order as ORDER

K = 4                       # codebooks of the stub model
MAX_SEQ = 256
SPF = 4                     # samples per frame of the stub codec
LONG = list(range(1, 200))
INF = 150 * 80              # a max_audio_length nobody reaches


class Tok:
    def encode(self, text):
        return [1] + [3 + (b % 200) for b in text.encode()] + [2]


def _speaker(tk):
    """The speaker of the LAST text segment of a feed ("[<speaker>]text" through Tok: BOS, '[', the digits, ']')."""
    i, n = int((tk[:, K] == 1).nonzero()[-1]) + 2, 0
    while int(tk[i, K]) != 3 + ord("]"):
        n, i = 10 * n + int(tk[i, K]) - 3 - ord("0"), i + 1
    return n


class RowsCodec:
    """decode_stream_rows protocol with ``state_slots``: SPF samples per frame, each the sum of the frame's codes; per slot the
    frames decoded since ``open``."""
    sample_rate = 24000

    def __init__(self):
        self.log, self.made = [], []

    def encode(self, audio):
        T = audio.shape[-1] // SPF
        return (torch.arange(K * T).reshape(1, K, T) % 7) + 1

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(SPF, -1)

    def decode_stream_rows(self, slots=16, max_chunk_frames=32, state_slots=None):
        codec = self
        self.made.append(dict(slots=slots, max_chunk_frames=max_chunk_frames, state_slots=state_slots))
        n_slots = slots if state_slots is None else state_slots

        class Rows:
            pos = [None] * n_slots

            def open(self, slot):
                assert 0 <= slot < n_slots
                codec.log.append(("open", slot))
                self.pos[slot] = 0

            def step(self, rows, codes):
                assert codes.shape[0] == len(rows) == len(set(rows)) <= slots and all(self.pos[s] is not None for s in rows)
                codec.log.append(("step", tuple(rows), codes.shape[2]))
                for s in rows:
                    self.pos[s] += codes.shape[2]
                return codes.float().sum(1).repeat_interleave(SPF, -1)
        return Rows()


class OldCodec(RowsCodec):
    """The rows codec as it was: no ``state_slots`` keyword - a server without ``streams`` must still take it."""

    def decode_stream_rows(self, slots=16, max_chunk_frames=32):
        return RowsCodec.decode_stream_rows(self, slots, max_chunk_frames)


class Parked:
    def __init__(self, kv, script, at, gen):
        self.kv, self.hist, self.gen, self.script, self.at = kv, None, gen, script, at


class State:
    """What BatchServer uses of DecodeState.  ``cache[b]``: the frames row b's cache holds, position by position ([L, K + 1]; a
    parked history is the same as [1, 1, 1, L, K + 1]).  A row samples the script of the speaker of its latest feed
    (``scripts[speaker]``: a list of scripts, one per turn of that speaker); frame i = K copies of the i-th value, 0 = EOS."""
    scripts = {}
    made = []

    def __init__(self, engine, B, adapters=None, bank=None):
        self.B, self.bank, self.log = B, bank, []
        self.active_rows = list(range(B))
        self.active = torch.ones(B, dtype=torch.int32)
        self.script, self.at, self.adapter, self.gen = [None] * B, [0] * B, [None] * B, [None] * B
        self.cache = [torch.zeros(0, K + 1, dtype=torch.long) for _ in range(B)]
        self.turn = {}
        State.made.append(self)

    def _start(self, b, tk):
        sp = _speaker(tk)
        t = self.turn.get(sp, 0)
        self.turn[sp] = t + 1
        scr = State.scripts[sp]
        self.script[b], self.at[b] = scr[t % len(scr)], 0

    def _next(self, rows):
        out = torch.full((self.B, K), 99, dtype=torch.int32)          # rows that do not sample: junk the server must ignore
        for b in rows:
            out[b] = self.script[b][self.at[b]]
            self.at[b] += 1
        return out

    def prefill_row(self, b, tk, mk):
        self.cache[b] = tk.clone().long()
        self._start(b, tk)
        self.log.append(("prefill", b))
        return torch.zeros(8)

    def append_rows(self, rows, tokens_list, masks_list):
        for b, tk in zip(rows, tokens_list):
            assert self.cache[b].shape[0] > 0
            self.cache[b] = torch.cat([self.cache[b], tk.long()], 0)
            self._start(b, tk)
        self.log.append(("append_rows", tuple(rows)))
        return torch.zeros(len(rows), 8)

    def park_row(self, b, length):
        assert 1 <= length <= self.cache[b].shape[0]
        self.log.append(("park", b, length))
        return self.cache[b][:length].clone().view(1, 1, 1, length, K + 1)

    def resume_row(self, b, parked):
        self.cache[b] = parked.reshape(-1, K + 1).clone()
        self.log.append(("resume", b, parked.shape[3]))

    def park_rows(self, rows):
        rows = list(rows)
        assert 1 <= len(rows) == len(set(rows)) <= 16 and all(self.script[b] is not None for b in rows)
        self.log.append(("park_rows", tuple(rows)))
        out = [Parked(self.cache[b].clone().view(1, 1, 1, -1, K + 1), self.script[b], self.at[b], self.gen[b]) for b in rows]
        for b in rows:                                                 # (what is left in the row is junk from now on)
            self.script[b], self.gen[b], self.cache[b] = None, None, torch.zeros(0, K + 1, dtype=torch.long)
        return out

    def resume_rows(self, rows, parked):
        rows = list(rows)
        assert 1 <= len(rows) == len(set(rows)) == len(parked) <= 16
        self.log.append(("resume_rows", tuple(rows)))
        for b, p in zip(rows, parked):
            self.cache[b], self.script[b], self.at[b], self.gen[b] = p.kv.reshape(-1, K + 1).clone(), p.script, p.at, p.gen

    def set_row_adapter(self, b, state):
        self.adapter[b] = state

    def new_row_generator(self, seed):
        return ["generator", seed]

    def set_row_seed(self, b, seed, generator=None):
        self.gen[b] = generator if generator is not None else seed

    def set_active(self, rows):
        self.active_rows = sorted(rows)
        self.active = torch.tensor([1 if b in rows else 0 for b in range(self.B)], dtype=torch.int32)

    def serve_first(self, last_h, rows, temperature, topk):
        self.log.append(("first", tuple(rows)))
        return self._next(rows)

    def serve_frame(self, tokens, masks, temperature, topk):
        rows = self.active_rows
        for b in range(self.B):
            if b in rows:                                               # an active row is fed the frame it sampled last
                assert tokens[b, 0, :K].tolist() == [self.script[b][self.at[b] - 1]] * K, (b, tokens[b])
                self.cache[b] = torch.cat([self.cache[b], tokens[b].long()], 0)
            else:
                assert not tokens[b].any()                              # idle rows: zero tokens
                c = self.cache[b]                                       # (the device writes a zero token at position 1)
                self.cache[b] = torch.cat([c[:1], torch.zeros(1, K + 1, dtype=torch.long)], 0) if c.shape[0] else c
        self.log.append(("frame", tuple(rows)))
        return self._next(rows)


class OldState(State):
    """The state as it was: a server without ``streams`` must not miss the new calls."""
    park_rows = resume_rows = None


class StubModel:
    device = torch.device("cpu")
    use_kv_cache = True

    def __init__(self):
        self.args = types.SimpleNamespace(audio_num_codebooks=K)
        self.bb = types.SimpleNamespace(max_seq_len=MAX_SEQ)
        self.engine = types.SimpleNamespace(_need=lambda: None)
        self._decode_state = None

    def setup_caches(self, n):
        pass

    def reset_caches(self):
        self._decode_state = None


class Clock:
    """A clock that moves only when somebody sleeps (or the test sets it)."""

    def __init__(self):
        self.now, self.slept, self.reads = 100.0, [], 0

    def __call__(self):
        self.reads += 1
        return self.now

    def sleep(self, s):
        assert s > 0
        self.slept.append(s)
        self.now += s


@pytest.fixture
def make(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    State.made, State.scripts = [], {}

    def _make(scripts, state=State, codec=RowsCodec, **kw):
        monkeypatch.setattr(S, "DecodeState", state)
        State.scripts = scripts
        codec = codec()
        gen = Generator(StubModel(), text_tokenizer=Tok(), audio_tokenizer=codec)
        srv = gen.serve(**kw)
        return gen, srv, State.made[-1], codec
    return _make


def _audio(values):
    return torch.tensor([float(K * v) for v in values]).repeat_interleave(SPF)


def _script(s, frames=None):
    """Speaker s says 1000 * (s + 1) + i in frame i (never 0: no EOS), or ``frames`` of them and then EOS."""
    body = [1000 * (s + 1) + i for i in range(len(LONG) if frames is None else frames)]
    return [body + [0] * 8]


def _holders(srv):
    return [None if r is None else r.id for r in srv._rows]


def _launches(st):
    return [e for e in st.log if e[0] in ("park_rows", "resume_rows")]


# ------------------------------------------------------------------------------------------------------------- the schedule
def test_fair_share_schedule_of_24_requests_on_16_slots(make):
    gen, srv, st, codec = make({s: _script(s) for s in range(24)}, slots=16, streams=24, chunk_frames=4)
    assert codec.made == [dict(slots=16, max_chunk_frames=4, state_slots=24)]
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(24)]
    lo, hi, mid = list(range(0, 8)), list(range(16, 24)), list(range(8, 16))
    want = [                                    # who holds slot 0..15 in steps 1..6 (tests/serve_streams_order.py's derivation)
        (lo + mid, [], []),
        (lo + hi, [("park_rows", tuple(range(8, 16)))], []),
        (mid + hi, [("park_rows", tuple(range(0, 8)))], [("resume_rows", tuple(range(0, 8)))]),
        (mid + lo, [("park_rows", tuple(range(8, 16)))], [("resume_rows", tuple(range(8, 16)))]),
        (hi + lo, [("park_rows", tuple(range(0, 8)))], [("resume_rows", tuple(range(0, 8)))]),
        (hi + mid, [("park_rows", tuple(range(8, 16)))], [("resume_rows", tuple(range(8, 16)))]),
    ]
    for step, (holders, parks, resumes) in enumerate(want, 1):
        del st.log[:]
        out = srv.step()
        assert _holders(srv) == holders, step
        assert sorted(r.id for r, _, _ in out) == sorted(holders) and all(a.numel() == 4 * SPF for _, a, _ in out)
        assert _launches(st) == parks + resumes, step                      # ONE launch out and ONE in, the park first
        # scheduling comes before the running rows' first frame, and resumed rows are running rows of the step
        frames = [e for e in st.log if e[0] in ("park_rows", "resume_rows", "frame", "first")]
        assert [e[0] for e in frames[:len(parks + resumes)]] == [e[0] for e in parks + resumes]
        if step > 2:                                                         # (nobody joins any more: all 16 rows run all 4 frames)
            assert frames[len(parks + resumes):] == [("frame", tuple(range(16)))] * 4
    assert srv.stats == {"steps": 6, "parks": 40, "resumes": 32, "park_launches": 5, "resume_launches": 4}
    assert [r.preemptions for r in reqs] == [2] * 8 + [2] * 8 + [1] * 8
    assert reqs[8].slots_held == [8, 0, 8] and reqs[0].slots_held == [0, 8] and reqs[16].slots_held == [8, 0]
    assert [r.state for r in reqs] == ["parked"] * 8 + ["running"] * 16
    assert sorted(r.id for r in srv.in_flight) == list(range(24)) and srv.queued == 0
    # a request keeps ONE codec slot for its whole life - its admission order here - whichever decode slot it sits in
    assert [r._cslot for r in reqs] == list(range(24))
    assert [e for e in codec.log if e[0] == "open"] == [("open", c) for c in range(24)]
    assert codec.log[-1] == ("step", tuple(range(16, 24)) + tuple(range(8, 16)), 4)
    # everybody got the frames of their own script, in order, through every move
    for s, r in enumerate(reqs):
        assert r.codes()[0].tolist() == _script(s)[0][:r._emitted] and r._emitted in (12, 16)
        assert torch.equal(r.audio(), _audio(_script(s)[0][:r._emitted]))


def test_streams_requests_finish_with_their_own_audio_and_free_their_codec_slots(make):
    lens = [3 + (5 * s) % 23 for s in range(30)]
    gen, srv, st, codec = make({s: _script(s, lens[s]) for s in range(30)}, slots=4, streams=7, chunk_frames=3)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(30)]
    peak, cslots = 0, {}
    while srv.next_due() is not None:
        before = len(_launches(st))
        out = srv.step()
        new = [e[0] for e in _launches(st)[before:]]
        assert out and new in ([], ["park_rows"], ["resume_rows"], ["park_rows", "resume_rows"])      # one launch each at most
        peak = max(peak, len(srv.in_flight))
        assert len(srv.in_flight) <= 7 and len(srv.active) <= 4
        for r in srv.in_flight:
            assert cslots.setdefault(r.id, r._cslot) == r._cslot and 0 <= r._cslot < 7     # never moved, inside the arenas
        assert len({r._cslot for r in srv.in_flight}) == len(srv.in_flight)                 # and never shared
        assert sorted(srv._cfree + [r._cslot for r in srv.in_flight]) == list(range(7))
    assert peak == 7 and all(r.done and r.state == "done" and not r.cancelled for r in reqs) and srv._cfree == list(range(7))
    for s, r in enumerate(reqs):
        assert torch.equal(r.audio(), _audio(_script(s)[0][:lens[s]])), s
    assert sum(r.preemptions for r in reqs) == srv.stats["parks"] > 0 and srv.stats["resumes"] == srv.stats["parks"]
    assert srv.step() == [] and list(srv.run()) == []
    # FIFO admission under the cap: codec slots are opened in request order, and request 7 only after somebody ended
    opens = [e for e in codec.log if e[0] == "open"]
    assert len(opens) == 30
    admitted = sorted(reqs, key=lambda r: (codec.log.index(("open", r._cslot)) if r.id < 7 else 10 ** 6, r.id))
    assert [r.id for r in admitted] == list(range(30))


def test_fifo_admission_under_the_streams_cap(make):
    gen, srv, st, codec = make({s: _script(s, 6 if s == 1 else None) for s in range(6)}, slots=2, streams=3, chunk_frames=2)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(6)]
    srv.step()
    assert [r.state for r in reqs] == ["running", "running"] + ["queued"] * 4
    srv.step()                                                               # room for one more stream: request 2, not more
    assert [r.state for r in reqs] == ["running", "parked", "running"] + ["queued"] * 3 and srv.queued == 3
    for _ in range(12):
        srv.step()
        assert len(srv.in_flight) <= 3
        if reqs[1].done:
            break
    assert reqs[1].done and reqs[3].state == "queued"
    srv.step()
    assert reqs[3].state != "queued" and reqs[4].state == "queued"      # 3 took the place 1 left - in order
    assert reqs[3]._cslot == 1                                                           # ... and its codec slot


def test_nothing_is_parked_when_the_requests_fit_the_slots(make):
    gen, srv, st, codec = make({s: _script(s) for s in range(6)}, slots=4, streams=9, chunk_frames=2)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(4)]
    for _ in range(3):
        srv.step()
    assert not _launches(st) and _holders(srv) == [0, 1, 2, 3]               # four candidates on four slots: nobody moves
    reqs += [srv.submit("x", s, [], max_audio_length_ms=INF) for s in (4, 5)]
    srv.step()                                                               # six candidates: the two newcomers and two of the four
    assert _launches(st) == [("park_rows", (2, 3))] and _holders(srv) == [0, 1, 4, 5]
    gen, srv, st, codec = make({s: _script(s, 5 + s) for s in range(4)}, slots=4, streams=9, chunk_frames=2)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(4)]
    for _ in srv.run():
        pass
    assert all(r.done and r.preemptions == 0 for r in reqs) and not _launches(st) and srv.stats["parks"] == srv.stats["resumes"] == 0
    for s, r in enumerate(reqs):
        assert torch.equal(r.audio(), _audio(_script(s)[0][:5 + s])) and r.slots_held == [s]


def test_probe_of_the_gpu_contract_is_parked_twice_and_moves(make):
    """The submission order of tests/test_serve_streams_gpu.py (serve_streams_order.submit_all), on the stub: the probe is
    parked at least twice and holds at least two different slots, whatever the others say - so the GPU comparison is not vacuous."""
    scripts = {s: _script(s) for s in range(24)}
    gen, srv, st, codec = make(scripts, slots=ORDER.SLOTS, streams=ORDER.STREAMS, chunk_frames=ORDER.CHUNK)
    probe, others = ORDER.submit_all(
        lambda: srv.submit("probe", 23, [], seed=1234, max_audio_length_ms=ORDER.PROBE_FRAMES * 80),
        lambda i: srv.submit("o" * (1 + i), i, [], seed=i, max_audio_length_ms=ORDER.OTHER_FRAMES * 80))
    assert probe.id == ORDER.PROBE_AT and len(others) == ORDER.OTHERS
    for _ in srv.run():
        pass
    assert probe.done and probe.preemptions >= 2 and len(set(probe.slots_held)) >= 2
    assert probe.slots_held == [8, 0, 8] and probe.codes().shape == (K, ORDER.PROBE_FRAMES)
    assert torch.equal(probe.audio(), _audio(_script(23)[0][:ORDER.PROBE_FRAMES]))
    assert all(o.done and o.codes().shape[1] == ORDER.OTHER_FRAMES for o in others)
    seeds = [e for e in st.log if e[0] == "resume_rows"]
    assert seeds and st.gen == [None] * 16                                  # every generator left with its request


# ----------------------------------------------------------------------------------------------------------------- pacing
def test_pacing_skips_who_is_ahead_and_sleeps_exactly_until_somebody_is_due(make):
    clock = Clock()
    gen, srv, st, codec = make({s: _script(s) for s in range(3)}, slots=2, streams=3, chunk_frames=2,
                               max_lead_ms=400, clock=clock, sleep=clock.sleep)
    a, b = [srv.submit("x", s, [], max_audio_length_ms=frames * 80) for s, frames in ((0, 14), (1, 6))]
    assert srv.next_due() == 0.0
    srv.step()                                                               # 160 ms each; their listeners start now (t0 = 100)
    assert a._t0 == b._t0 == 100.0 and srv.next_due() == 0.0
    srv.step()                                                               # 320 ms
    srv.step()                                                               # 480 ms: at or over 400 - nobody is a candidate
    assert a._emitted == b._emitted == 6 and b.done
    before = list(st.log)
    assert srv.next_due() == pytest.approx(0.080) and srv.step() == [] and st.log == before      # nothing runs, nothing moves
    assert a.state == "running" and a.preemptions == 0                        # (an idle step parks nobody)
    clock.now += 0.080                                                       # lead = 400 exactly: at the bound is not below it
    assert srv.step() == [] and srv.next_due() == pytest.approx(0.001)
    clock.now += 0.001
    assert srv.next_due() == 0.0 and [r.id for r, _, _ in srv.step()] == [0]   # lead 399 -> 559 (640 ms emitted, 81 ms heard)
    assert srv.next_due() == pytest.approx(0.159)
    # a newcomer has no listener yet: it is a candidate at once, and runs alone - the one ahead is parked, not idled
    c = srv.submit("x", 2, [], max_audio_length_ms=6 * 80)
    assert srv.next_due() == 0.0
    assert [r.id for r, _, _ in srv.step()] == [2] and a.state == "parked" and a.preemptions == 1 and c._t0 == clock.now
    assert [[r.id for r, _, _ in srv.step()] for _ in range(2)] == [[2], [2]] and c.done and not clock.slept
    # run(): sleeps exactly next_due, steps when somebody is due, returns when all are done
    due = srv.next_due()
    assert due == pytest.approx(0.159)
    it = srv.run()
    first = next(it)
    # (after sleeping 0.159 s the lead is 400 to rounding: below the bound, or one more millisecond's sleep away from it)
    assert clock.slept[0] == due and sum(clock.slept) == pytest.approx(0.160, abs=0.0011) and first[0] is a and a.state == "running"
    for _ in it:
        pass
    # every chunk of 160 ms is made 160 ms after the one before: the listener is never more than the bound plus a chunk ahead
    assert a.done and srv.next_due() is None and sum(clock.slept) == pytest.approx(3 * 0.160, abs=0.0011)
    assert 3 <= len(clock.slept) <= 6 and all(s >= 0.001 for s in clock.slept)
    assert torch.equal(a.audio(), _audio(_script(0)[0][:14])) and torch.equal(c.audio(), _audio(_script(2)[0][:6]))
    assert a.preemptions == 1 and a.slots_held == [0, 0]                     # (c had left slot 0 when a came back)


def test_fair_share_never_reads_the_clock(make):
    def clock():
        raise AssertionError("the fair-share schedule reads no clock")
    gen, srv, st, codec = make({s: _script(s, 7) for s in range(5)}, slots=2, streams=5, chunk_frames=2, clock=clock, sleep=clock)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(5)]
    assert srv.next_due() == 0.0
    for _ in srv.run():
        pass
    assert all(r.done for r in reqs) and srv.next_due() is None


# ------------------------------------------------------------------------------------------------- pause / resume / cancel
def test_pause_and_resume_in_every_state(make):
    gen, srv, st, codec = make({s: _script(s, 10) for s in range(4)}, slots=2, streams=3, chunk_frames=2)
    r0, r1, r2, r3 = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(4)]
    r3.pause()                                                               # queued: passed over at admission
    assert r3.state == "paused"
    srv.step()                                                               # 0 and 1 run
    r0.pause()                                                               # running: parked at the next step
    assert r0.state == "paused" and r0.slot == 0
    srv.step()
    assert r0.slot is None and r0.preemptions == 1 and ("park_rows", (0,)) in st.log
    assert [r.state for r in (r0, r1, r2, r3)] == ["paused", "running", "running", "paused"]
    assert r2.slot == 0 and srv.queued == 1 and len(srv.in_flight) == 3       # r3 is still queued, behind its pause
    srv.step()
    srv.step()
    assert r0._emitted == 2 and r1._emitted == 8 and r2._emitted == 6          # two candidates on two slots: nobody moved
    r1.pause()
    r2.pause()
    before = list(st.log)
    assert srv.next_due() is None and srv.step() == [] and list(srv.run()) == [] and st.log == before     # all are paused
    r0.resume()                                                              # parked while paused: back through resume_rows
    srv.step()
    assert r0.state == "running" and r0._emitted == 4 and r1.state == r2.state == "paused" and r1.slot is None
    r1.resume()
    r2.resume()
    r3.resume()
    r1.pause()
    r1.resume()                                                              # (a pause that never saw a step changes nothing)
    for _ in srv.run():
        pass
    for s, r in enumerate((r0, r1, r2, r3)):
        assert r.done and torch.equal(r.audio(), _audio(_script(s)[0][:10])), s
    r0.pause()                                                               # done: nothing happens
    r0.resume()
    assert r0.state == "done"


def test_pause_of_a_parked_request_and_cancel_of_paused_ones(make):
    gen, srv, st, codec = make({s: _script(s, 10) for s in range(5)}, slots=2, streams=3, chunk_frames=2)
    r0, r1, r2, r3, r4 = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(5)]
    srv.step()
    srv.step()                                                               # 2 joins, 0 stays, 1 is parked
    assert [r.state for r in (r0, r1, r2)] == ["running", "parked", "running"]
    r1.pause()                                                               # parked: it stays where it is, out of the schedule
    assert r1.state == "paused" and r1._row is not None and r1.slot is None
    srv.step()
    srv.step()                                                               # it has the least audio by far, and is never resumed
    assert (r0._emitted, r1._emitted, r2._emitted) == (8, 2, 6) and not any(e[0] == "resume_rows" for e in st.log)
    assert r1.preemptions == 1 and len(srv.in_flight) == 3 and srv.queued == 2   # (paused ones count against ``streams``)
    r1.resume()
    assert r1.state == "parked"
    srv.step()                                                               # 1 and 2 run; 0, the furthest ahead, is parked
    assert r1.state == "running" and r1.slot == 0 and r1._emitted == 4 and r0.state == "parked"
    r0.pause()
    srv.cancel(r0)                                                           # paused and parked
    assert r0.done and r0.cancelled and r0.state == "done" and r0._row is None and not r0._paused
    assert srv._cfree == [0] and [r.id for r in srv.in_flight] == [1, 2]
    assert torch.equal(r0.audio(), _audio(_script(0)[0][:8]))
    r4.pause()
    srv.cancel(r4)                                                           # paused and still queued
    assert r4.done and r4.cancelled and r4.state == "done" and srv.queued == 1 and r4.audio().numel() == 0
    for _ in srv.run():
        pass
    for s, r in ((1, r1), (2, r2), (3, r3)):
        assert r.done and not r.cancelled and torch.equal(r.audio(), _audio(_script(s)[0][:10])), s
    assert r3._cslot == 0 and srv.in_flight == [] and srv._cfree == [0, 1, 2]


def test_cancel_in_every_state(make):
    gen, srv, st, codec = make({s: _script(s, 10) for s in range(6)}, slots=2, streams=3, chunk_frames=2)
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(6)]
    srv.cancel(reqs[5])                                                      # queued
    assert reqs[5].done and reqs[5].cancelled and srv.queued == 5 and reqs[5].audio().numel() == 0
    srv.step()
    srv.step()                                                               # 0 running, 1 parked, 2 running
    assert [r.state for r in reqs[:3]] == ["running", "parked", "running"]
    srv.cancel(reqs[1])                                                      # parked
    assert reqs[1].done and reqs[1].cancelled and reqs[1]._row is None and srv._cfree == [1] and len(srv.in_flight) == 2
    srv.cancel(reqs[0])                                                      # running
    assert reqs[0].done and reqs[0].slot is None and srv._rows[0] is None and srv._cfree == [0, 1]
    assert torch.equal(reqs[0].audio(), _audio(_script(0)[0][:4]))             # what it said stays
    reqs[2].pause()
    srv.cancel(reqs[2])                                                      # paused (still in its slot)
    assert reqs[2].done and reqs[2].state == "done" and srv.active == [] and srv.in_flight == []
    srv.cancel(reqs[2])                                                      # done: idempotent
    srv.cancel(reqs[0], heard_frames=1)
    for _ in srv.run():
        pass
    assert reqs[3].done and reqs[4].done and not reqs[3].cancelled
    assert torch.equal(reqs[3].audio(), _audio(_script(3)[0][:10]))
    assert [e for e in codec.log if e[0] == "open"] == [("open", 0), ("open", 1), ("open", 2), ("open", 0), ("open", 1)]
    other = make({0: _script(0)}, slots=2)[1]
    with pytest.raises(ValueError, match="not a request of this server"):
        other.cancel(reqs[3])
    r = other.submit("x", 0, [], max_audio_length_ms=INF)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="heard_frames must be an integer >= 0"):
            other.cancel(r, heard_frames=bad)
    assert not r.done


def test_cancel_works_on_a_server_without_streams(make):
    gen, srv, st, codec = make({s: _script(s, 9) for s in range(3)}, state=OldState, codec=OldCodec, slots=2, chunk_frames=2)
    r0, r1, r2 = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(3)]
    srv.step()
    srv.cancel(r0)                                                           # running: its slot is free at once
    assert r0.done and r0.cancelled and srv._rows[0] is None and r0.state == "done"
    srv.step()
    assert r2.slot == 0 and r2.state == "running"
    srv.cancel(r1)
    for _ in srv.run():
        pass
    assert r2.done and torch.equal(r2.audio(), _audio(_script(2)[0][:9])) and torch.equal(r1.audio(), _audio(_script(1)[0][:4]))
    with pytest.raises(RuntimeError, match=r"pause\(\) / resume\(\) need a server made with serve\(streams=\)"):
        r2.pause()
    with pytest.raises(RuntimeError, match="need a server made with"):
        r2.resume()


def test_cancelled_turn_keeps_what_was_heard_and_the_next_turn_works(make):
    scripts = {0: [[11, 12, 13, 14, 15, 16, 17, 18, 19] + [0] * 8, [21, 22, 0] + [3] * 8], 1: _script(1), 2: _script(2)}
    gen, srv, st, codec = make(scripts, slots=2, streams=3, chunk_frames=2)
    conv = srv.conversation(seed=5)
    t1 = conv.say("hello", 0, max_audio_length_ms=20 * 80)
    fill = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in (1, 2)]
    base = conv.tokens.shape[0]
    srv.step()
    srv.step()                                                               # t1 runs in steps 1 and 2: 4 frames
    srv.step()                                                               # ... and is parked in step 3 (the others have less)
    assert t1._emitted == 4 and t1.preemptions == 1 and t1.state == "parked"   # cancelled while it holds no slot
    srv.cancel(t1, heard_frames=3)
    assert t1.done and t1.cancelled and conv._open is t1
    # the history: the text, the 3 frames that were heard, one EOS frame; the cache: base + 3 positions out of the parked row
    assert conv.tokens.shape[0] == base + 4 and conv.tokens[base:base + 3, 0].tolist() == [11, 12, 13]
    assert not conv.tokens[base + 3].any() and conv.cached == base + 3
    assert conv._parked.shape == (1, 1, 1, base + 3, K + 1)
    assert torch.equal(conv._parked.reshape(-1, K + 1), conv.tokens[:base + 3])
    t2 = conv.say("again", 0, max_audio_length_ms=20 * 80)                     # fed: the EOS frame and the new text
    assert t2._tokens.shape[0] == 1 + len("[0]again") + 2
    for _ in srv.run():
        if t2.done:
            break
    assert t2.done and t2.codes()[0].tolist() == [21, 22] and conv.cached == conv.tokens.shape[0] - 1      # (all but the EOS frame)
    # a running turn, cancelled with more frames than it emitted: all emitted are kept; a queued turn: the text and EOS only
    t3 = conv.say("third", 0, max_audio_length_ms=20 * 80)
    n3 = conv.tokens.shape[0]
    srv.cancel(t3, heard_frames=2)
    assert t3.done and conv.tokens.shape[0] == n3 + 1 and not conv.tokens[-1].any()
    cached = conv.cached
    t4 = conv.say("fourth", 0, max_audio_length_ms=20 * 80)
    assert conv.cached == cached and t4._tokens.shape[0] == conv.tokens.shape[0] - cached
    for f in fill:
        srv.cancel(f)
    srv.step()
    assert t4.state == "running" and t4._emitted == 2
    n4 = conv.tokens.shape[0]
    srv.cancel(t4, heard_frames=50)
    assert conv.tokens.shape[0] == n4 + 3 and conv.cached == n4 + 1                # 2 sampled: one was fed back
    assert st.gen == [None, None]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(make):
    for kw, msg in ((dict(streams=3), "streams must be an integer in slots..256"),
                    (dict(streams=257), "streams must be an integer in slots..256"),
                    (dict(streams=16.0), "streams must be an integer"),
                    (dict(streams=True), "streams must be an integer"),
                    (dict(max_lead_ms=500), "max_lead_ms belongs to the schedule"),
                    (dict(clock=lambda: 0.0), "clock belongs to the schedule"),
                    (dict(sleep=lambda s: None), "sleep belongs to the schedule"),
                    (dict(streams=8, max_lead_ms=0), "max_lead_ms must be a finite number > 0"),
                    (dict(streams=8, max_lead_ms=float("inf")), "max_lead_ms must be a finite number > 0"),
                    (dict(streams=8, max_lead_ms="1"), "max_lead_ms must be a finite number > 0"),
                    (dict(streams=8, clock=3), "clock must be callable"),
                    (dict(streams=8, sleep=3), "sleep must be callable")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            make({}, slots=4, **kw)
    with pytest.raises(ValueError, match="slots must be an integer in 1..16"):
        make({}, slots=17, streams=20)
    gen, srv, st, codec = make({}, slots=4, streams=4)                       # streams = slots is allowed: pause and pacing alone
    assert srv.streams == 4 and codec.made[-1]["state_slots"] == 4


def test_state_slots_refusals_of_the_rows_objects():
    from csm.codec.mimi import MimiDecodeStreamRows
    from csm.codec.resample import ResampleStreamRows
    for bad in (3, 0, -1, 4.5, True):
        with pytest.raises(ValueError, match="state_slots must be an integer >= slots = 4"):
            MimiDecodeStreamRows(None, 4, 8, state_slots=bad)
        with pytest.raises(ValueError, match="state_slots must be an integer >= slots = 4"):
            ResampleStreamRows(None, 4, 100, state_slots=bad)
    with pytest.raises(ValueError, match=re.escape("slots must be 1..16 (the rows kernels take at most 16 rows a launch), got 17")):
        MimiDecodeStreamRows(None, 17, 8, state_slots=40)                    # today's refusals keep their text
    with pytest.raises(ValueError, match=re.escape("slots must be 1..16 (the rows kernel takes at most 16 rows a launch), got 17")):
        ResampleStreamRows(None, 17, 100, state_slots=40)


# ---------------------------------------------------------------------------------------------------- streams=None is today
def test_without_streams_nothing_new_is_called(make):
    """The old state (no park_rows / resume_rows) and the old codec (no ``state_slots`` keyword) serve as before."""
    gen, srv, st, codec = make({s: _script(s, 3 + s) for s in range(5)}, state=OldState, codec=OldCodec, slots=2, chunk_frames=2)
    assert srv.streams is None and not hasattr(srv, "_clock")
    reqs = [srv.submit("x", s, [], max_audio_length_ms=INF) for s in range(5)]
    assert srv.next_due() == 0.0
    for _ in srv.run():
        pass
    assert srv.next_due() is None and all(r.done and r.preemptions == 0 and len(r.slots_held) == 1 for r in reqs)
    assert all(r._cslot == r.slots_held[0] for r in reqs)                     # the codec slot is the decode slot
    assert not _launches(st) and srv.in_flight == [] and srv.stats["parks"] == 0
    for s, r in enumerate(reqs):
        assert torch.equal(r.audio(), _audio(_script(s)[0][:3 + s]))


def test_exports_and_cli_flag():
    from csm import hip
    from csm.cli import generate as G
    from csm.engine import DecodeState, ParkedRow
    from csm.hip import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "csm_hip.h")).read()
    for name, n in (("csm_kv_park_rows", 11), ("csm_sample_hist_move_rows", 9)):
        decl = re.search(rf"int\s+{name}\s*\(([^)]*)\)", header)
        assert decl and len(decl.group(1).split(",")) == n == len(hip._SIGS[name][0]), name
        assert name in hip.EXPORTS and hasattr(hip.lib, name)
    assert hip.lib.csm_abi_version() == 3
    assert callable(ops.kv_park_rows) and callable(ops.sample_hist_move_rows)
    assert callable(DecodeState.park_rows) and callable(DecodeState.resume_rows) and ParkedRow(1, 2, 3).gen == 3
    common = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t", "--output", "o.wav"]
    base = common + ["--serve-file", "f.jsonl"]
    assert G.parse_args(base).streams is None and G.parse_args(base + ["--streams", "40"]).streams == 40
    assert G.parse_args(base + ["--slots", "4", "--streams", "4"]).streams == 4
    for bad in (["--streams", "8"], ["--streams", "257"]):
        with pytest.raises(SystemExit):
            G.parse_args(base + bad)
    with pytest.raises(SystemExit):
        G.parse_args(common + ["--text", "hi", "--streams", "20"])
