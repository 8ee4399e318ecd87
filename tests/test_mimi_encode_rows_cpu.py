"""The rows form of the Mimi encode stream, host side: the new export, the peel schedule that brings ragged slots to one chunk
size per launch, and the server's hear_slots bookkeeping (slots taken and freed, feed that only buffers, step() that drains,
end_heard all-or-nothing) against the stubs of test_serve_conversation_cpu and a Python fake of ``encode_stream_rows``."""
import os
import re

import pytest
import torch

import test_serve_conversation_cpu as S
from test_mimi_encode_stream_cpu import FakeEncodeStream, SPF, _segment
from test_conversation_cpu import K, Tok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the export
def test_strided_rows_symbol_declared_bound_and_exported():
    import ctypes
    from csm import hip
    name = "csm_conv1d_stream_strided_rows_f32"
    header = open(os.path.join(ROOT, "include", "csm_hip.h")).read()
    assert re.search(rf"\bint {name}\(", header)
    assert name in hip.EXPORTS and name in hip._SIGS and hasattr(ctypes.CDLL(hip.LIB_PATH), name)
    assert len(hip._SIGS[name][0]) == len(getattr(hip.lib, name).argtypes) == 20
    decl = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == 20                                      # the binding has the header's argument count
    assert hip.lib.csm_abi_version() == 3                                  # additive: the ABI number stays
    from csm.codec.mimi import MimiCodec, MimiEncodeStreamRows
    assert callable(hip.ops.conv1d_stream_strided_rows_f32) and callable(MimiCodec.encode_stream_rows)
    for m in ("open", "close", "step", "feed", "pending", "drain"):
        assert callable(getattr(MimiEncodeStreamRows, m)), m


# ------------------------------------------------------------------------------------------------------------- the schedule
def _check_schedule(pending, mcf):
    """Every slot's total is right, every launch has a single n in 1..mcf and distinct slots that all had work, and there are no
    more launches than distinct pending counts plus the max_chunk_frames splits.  Returns the schedule."""
    from csm.codec.mimi import peel_schedule
    sched = peel_schedule(pending, mcf)
    total = dict.fromkeys(pending, 0)
    for n, slots in sched:
        assert isinstance(n, int) and 1 <= n <= mcf
        assert len(slots) == len(set(slots)) >= 1 and len(slots) <= 16
        for s in slots:
            assert total[s] + n <= pending[s]                              # only slots that still have n frames left
            total[s] += n
    assert total == dict(pending)
    distinct = len({p for p in pending.values() if p > 0})
    splits = max([(p - 1) // mcf for p in pending.values() if p > 0], default=0)     # cuts a backlog above mcf needs
    assert len(sched) <= distinct + splits
    return sched


def test_peel_schedule():
    from csm.codec.mimi import peel_schedule
    assert _check_schedule({}, 32) == []
    assert _check_schedule({0: 0, 5: 0}, 32) == []                         # nothing pending: nothing launched
    assert _check_schedule({2: 4, 0: 4, 7: 4}, 32) == [(4, [0, 2, 7])]     # all equal: one launch, all rows
    assert _check_schedule({0: 1, 1: 5, 2: 3, 3: 9}, 32) == [(1, [0, 1, 2, 3]), (2, [1, 2, 3]), (2, [1, 3]), (4, [3])]
    assert _check_schedule({0: 40, 1: 3}, 32) == [(3, [0, 1]), (32, [0]), (5, [0])]          # one above max_chunk_frames
    assert _check_schedule({4: 70}, 32) == [(32, [4]), (32, [4]), (6, [4])]
    assert _check_schedule({0: 4, 1: 4, 2: 0}, 4) == [(4, [0, 1])]
    _check_schedule({s: (s * 7) % 11 for s in range(16)}, 4)
    _check_schedule({s: 33 + s for s in range(16)}, 32)
    assert peel_schedule([(3, 2), (1, 2)], 8) == [(2, [1, 3])]             # any mapping form
    with pytest.raises(ValueError):
        peel_schedule({0: 1}, 0)


# ------------------------------------------------------------------------------------------------------------- the server
class FakeEncodeRows:
    """encode_stream_rows protocol in Python: SPF samples per frame; frame f of an utterance has the codes f % 7 + 1 + codebook
    (what FakeEncodeStream gives).  Logs every call; only ``drain`` stands for launches."""

    def __init__(self, log, slots, max_chunk_frames):
        self.log, self.slots = log, slots
        self.pos, self.count, self.live = [0] * slots, [0] * slots, [False] * slots
        log.append(("rows", slots))

    def open(self, slot):
        assert not self.live[slot]
        self.pos[slot], self.count[slot], self.live[slot] = 0, 0, True
        self.log.append(("open", slot))

    def close(self, slot):
        assert self.live[slot]
        self.count[slot], self.live[slot] = 0, False
        self.log.append(("close", slot))

    def feed(self, slot, wav):
        assert self.live[slot] and wav.dim() == 1
        self.count[slot] += wav.numel()
        self.log.append(("feed", slot, wav.numel()))
        return self.count[slot] // SPF

    def pending(self, slot):
        return self.count[slot] // SPF

    def drain(self, slots=None, flush=()):
        slots = [s for s in range(self.slots) if self.live[s]] if slots is None else list(slots)
        assert len(set(slots)) == len(slots) and all(self.live[s] for s in slots) and set(flush) <= set(slots)
        self.log.append(("drain", tuple(slots), tuple(flush)))
        out = {}
        for s in slots:
            if s in flush and self.count[s] % SPF:
                self.count[s] += SPF - self.count[s] % SPF
            n, self.count[s] = self.count[s] // SPF, self.count[s] % SPF
            f = torch.arange(self.pos[s], self.pos[s] + n)
            self.pos[s] += n
            out[s] = (f[None, :] % 7) + 1 + torch.arange(K)[:, None]
        return out


class ServeCodec(S.RowsCodec):
    def encode(self, audio):
        s = FakeEncodeStream([])
        return torch.cat([s.feed(audio.reshape(1, 1, -1)), s.flush()], 2)

    def encode_stream(self, max_chunk_frames=32):
        return FakeEncodeStream(self.log)

    def encode_stream_rows(self, slots=16, max_chunk_frames=32):
        return FakeEncodeRows(self.log, slots, max_chunk_frames)


@pytest.fixture
def make(monkeypatch):
    import csm.conversation as conv_mod
    import csm.serving as srv_mod
    from csm.generator import Generator
    monkeypatch.setattr(srv_mod, "DecodeState", S.State)
    monkeypatch.setattr(conv_mod, "DecodeState", S.ConvState)
    S.State.made, S.State.scripts = [], {0: [[5, 6, 7, 0] + [9] * 8] * 3, 2: [S.LONG]}

    def _make(**kw):
        codec = ServeCodec()
        gen = Generator(S.StubModel(), text_tokenizer=Tok(), audio_tokenizer=codec)
        return gen, gen.serve(slots=2, chunk_frames=2, **kw), codec
    return _make


def _drains(codec):
    return [e for e in codec.log if e[0] == "drain"]


def test_hear_slots_taken_and_freed(make):
    gen, srv, codec = make(hear_slots=2)
    assert codec.log == [("rows", 2)]
    a, b, c = srv.conversation(), srv.conversation(), srv.conversation()
    ta, tb = a.hear(1), b.hear(1)
    assert (ta.slot, tb.slot) == (0, 1) and srv._hearing == [ta, tb]
    with pytest.raises(RuntimeError, match="hear_slots"):                   # exhausted
        c.hear(1)
    assert c._heard is None
    with pytest.raises(RuntimeError, match="heard turn open"):
        a.hear(1)
    ta.cancel()                                                            # cancel frees
    ta.cancel()                                                            # (idempotent)
    assert srv._hearing == [None, tb] and a._heard is None and ta.closed and ta.pending == 0
    tc = c.hear(0)
    assert tc.slot == 0
    tb.end("yo")                                                           # end frees
    assert srv._hearing == [tc, None] and b._heard is None and tb.closed
    c.close()                                                              # close frees
    assert srv._hearing == [None, None] and tc.closed and c.closed
    assert [e for e in codec.log if e[0] in ("open", "close")] == [("open", 0), ("open", 1), ("close", 0), ("open", 0), ("close", 1),
                                                                  ("close", 0)]
    for call in (lambda: ta.feed(torch.zeros(SPF)), lambda: ta.end("x"), lambda: tb.end("x")):
        with pytest.raises(RuntimeError, match="ended or cancelled"):
            call()
    for bad in (-1, 17, 1.5):
        with pytest.raises(ValueError, match="hear_slots"):
            gen.serve(hear_slots=bad)
    bare = S.RowsCodec()                                                   # a codec without a rows encoder
    from csm.generator import Generator
    with pytest.raises(TypeError, match="encode_stream_rows"):
        Generator(S.StubModel(), text_tokenizer=Tok(), audio_tokenizer=bare).serve(hear_slots=1)


def test_feed_only_buffers_and_step_drains(make):
    gen, srv, codec = make(hear_slots=3)
    ref, a, b = srv.conversation(), srv.conversation(), srv.conversation()
    other = srv.conversation()
    other.say("elsewhere", 2, max_audio_length_ms=12 * 80)
    ref.add(_segment(3 * SPF + 1))
    ta, tb = a.hear(1), b.hear(1)
    ta.feed(torch.zeros(SPF + 1))
    ta.feed(torch.zeros(0))
    tb.feed(torch.zeros(3 * SPF))
    assert _drains(codec) == [] and (ta.frames, ta.pending, tb.frames, tb.pending) == (0, 1, 0, 3)      # nothing was launched
    assert a.tokens.shape[0] == 0
    srv.step()                                                             # another conversation speaks; step() drains first
    assert _drains(codec) == [("drain", (0, 1), ())]
    assert (ta.frames, ta.pending, tb.frames, tb.pending) == (1, 0, 3, 0)
    ta.feed(torch.zeros(SPF - 2))                                          # still inside the second frame: nothing to encode
    srv.step()
    assert len(_drains(codec)) == 1                                        # no whole frame waits: no drain
    ta.feed(torch.zeros(SPF + 2))
    assert srv.hear_step() == 2 and _drains(codec)[-1] == ("drain", (0,), ()) and srv.hear_step() == 0
    assert ta.frames == 3 and ta.pending == 0
    ta.end("yo")                                                           # one sample waits: flushed into a fourth frame
    assert _drains(codec)[-1] == ("drain", (0,), (0,)) and ta.frames == 4
    assert torch.equal(a.tokens, ref.tokens) and torch.equal(a.mask, ref.mask) and a._turns == ref._turns
    tb.cancel()
    assert b.tokens.shape[0] == 0


def test_end_heard_is_all_or_nothing(make):
    gen, srv, codec = make(hear_slots=4)
    _, srv0, _ = make(hear_slots=0)
    convs = [srv.conversation() for _ in range(3)]
    refs = [srv.conversation() for _ in range(3)]
    sizes = [2 * SPF, 3 * SPF + 2, 1]
    turns = []
    for c, r, n in zip(convs, refs, sizes):
        r.add(_segment(n, "t", 1))
        t = c.hear(1)
        t.feed(torch.zeros(n))
        turns.append(t)
    srv.hear_step()
    n_drains = len(_drains(codec))
    req = convs[1].say("hi", 0, max_audio_length_ms=20 * 80)                # its own turn is open: end is refused, as add is

    def untouched():
        assert len(_drains(codec)) == n_drains and srv._hearing[:3] == turns
        assert all(not t.closed for t in turns) and all(c._heard is t for c, t in zip(convs, turns))
        assert convs[0].tokens.shape[0] == 0 and convs[2].tokens.shape[0] == 0
        assert [t.frames for t in turns] == [2, 3, 0]

    with pytest.raises(RuntimeError, match="still open"):
        srv.end_heard([(turns[0], "t"), (turns[1], "t"), (turns[2], "t")])
    untouched()
    foreign = srv.conversation().hear(1)
    foreign._srv = srv0                                                     # a turn of another server
    with pytest.raises(ValueError, match="not a heard turn of this server"):
        srv.end_heard([(turns[0], "t"), (foreign, "t")])
    foreign._srv = srv
    own = srv0.conversation().hear(1)                                       # hear_slots = 0: a plain HeardTurn
    with pytest.raises(ValueError, match="not a heard turn of this server"):
        srv.end_heard([(turns[0], "t"), (own, "t")])
    foreign.cancel()
    with pytest.raises(RuntimeError, match="ended or cancelled"):           # a closed turn
        srv.end_heard([(turns[0], "t"), (foreign, "t")])
    with pytest.raises(ValueError, match="named twice"):
        srv.end_heard([(turns[0], "t"), (turns[2], "t"), (turns[0], "t")])
    untouched()
    srv.end_heard([])
    untouched()
    while not req.done:
        srv.step()
    L = convs[1].tokens.shape[0]
    n_drains = len(_drains(codec))
    srv.end_heard([(turns[2], "t"), (turns[0], "t"), (turns[1], "t")])      # one batched drain, every slot flushed
    assert _drains(codec)[n_drains:] == [("drain", (2, 0, 1), (2, 0, 1))]
    assert all(t.closed for t in turns) and srv._hearing == [None] * 4
    assert [t.frames for t in turns] == [2, 4, 1]
    for i in (0, 2):
        assert torch.equal(convs[i].tokens, refs[i].tokens) and torch.equal(convs[i].mask, refs[i].mask)
    assert torch.equal(convs[1].tokens[L:], refs[1].tokens) and torch.equal(convs[1].mask[L:], refs[1].mask)
    assert convs[3 - 1].hear(1).slot == 0                                   # and the slots serve again


def test_hear_slots_zero_never_makes_a_rows_encoder(make):
    gen, srv, codec = make()
    assert srv.hear_slots == 0 and srv._hear is None
    a, ref = srv.conversation(), srv.conversation()
    ref.add(_segment(2 * SPF + 1))
    turn = a.hear(1)
    assert not hasattr(turn, "slot") and turn.pending == 0
    turn.feed(torch.zeros(2 * SPF + 1))
    assert turn.frames == 2 and turn.pending == 0                          # encoded at feed, as before
    assert srv.hear_step() == 0
    srv.step()
    turn.end("yo")
    assert torch.equal(a.tokens, ref.tokens)
    assert codec.log == ["new", ("feed", 2 * SPF + 1), ("flush", 1)]        # its own encode stream; no ("rows", ...) entry
    a.close()


def test_generate_cli_hear_slots(tmp_path):
    from csm.cli.generate import parse_args
    base = ["--model-path", "m", "--mimi-weights", "w", "--text-tokenizer", "t"]
    assert parse_args(base + ["--serve-file", "f"]).hear_slots == 0
    assert parse_args(base + ["--serve-file", "f", "--hear-slots", "16"]).hear_slots == 16
    for bad in (["--serve-file", "f", "--hear-slots", "17"], ["--text", "x", "--hear-slots", "2"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
