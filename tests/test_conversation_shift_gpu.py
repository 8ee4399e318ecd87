"""``on_overflow="shift"`` / ``keep_turns`` end to end on the tiny model of tests/test_conversation_gpu.py (its backbone holds 128
positions): a conversation driven past the length limit keeps its KV cache - ``DecodeState.shift_row`` / ``shift_parked`` take
the dropped turn out and rotate the keys behind it back -, is fed by ``append`` / the one stacked ``append_rows`` and is never
prefilled again; ``drop_oldest`` and ``error`` next to it take the paths they took before."""
import pytest
import torch

import kv_shift_ref as R
from test_serving_gpu import TEMP, TOPK, Tok, _hf_mimi

pytestmark = pytest.mark.gpu

K = 32
MS = 6 * 80                                        # six frames per in-limit turn
MAX_SEQ = 128                                      # llama-tiny-backbone
VOICE, SECOND, SPOKEN, ADDED = 13, 28, 15, 30      # the turns of the history ``_drive`` builds, in positions


@pytest.fixture(scope="module")
def world(dev):
    from csm.codec import MimiCodec
    from csm.generator import Generator
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, K), device="cuda", seed=2)
    m.engine._need()
    assert m.bb.max_seq_len == MAX_SEQ
    return dict(m=m, gen=Generator(m, text_tokenizer=Tok(), audio_tokenizer=MimiCodec(_hf_mimi().state_dict(), device="cuda")))


def _seg(seed, frames, speaker, text):
    from csm.generator import Segment
    return Segment(speaker, text, torch.randn(frames * 1920, generator=torch.Generator().manual_seed(seed)) * 0.2)


def _context(seed=2):
    """The voice prompt (13 positions: the kept head) and a second turn (28 positions: the one that goes)."""
    return [_seg(1, 5, 0, "hi"), _seg(seed, 20, 1, "hi")]


class _Scripted:
    """The real frames run - the caches are fed - but scripted codes are handed out, so that two conversations that take
    different paths through the cache still write the same history."""

    def __init__(self, m):
        self.m, self.n = m, 0
        self.frame, self.tail = m.generate_frame, m.engine._frame_tail

    def _code(self, out):
        self.n += 1
        return torch.full_like(out, 1 + self.n % 97)

    def __enter__(self):
        self.m.generate_frame = lambda *a, **k: self._code(self.frame(*a, **k))
        self.m.engine._frame_tail = lambda *a, **k: self._code(self.tail(*a, **k))
        return self

    def __exit__(self, *exc):
        del self.m.engine._frame_tail
        del self.m.generate_frame


def _watch(st, log, rec=None):
    """Log the state's prefill / append / shift_row calls; ``rec`` gets the row's history before and after the shift."""
    for name in ("prefill", "append"):
        def wrapped(*a, _f=getattr(st, name), _n=name, **k):
            log.append(_n)
            return _f(*a, **k)
        setattr(st, name, wrapped)
    orig = st.shift_row

    def shift_row(b, keep, drop):
        log.append(("shift", keep, drop))
        if rec is not None:
            rec["before"] = st.park_row(b, st.row_pos[b] + 1).cpu()
            rec["others"] = (st.dc.kv.clone(), st.graph)
        orig(b, keep, drop)
        if rec is not None:
            rec["pos"] = (int(st.bb.pos[b]), st.row_pos[b])
            rec["after"] = st.park_row(b, st.row_pos[b] + 1).cpu()
            rec["untouched"] = torch.equal(st.dc.kv, rec["others"][0]) and st.graph is rec["others"][1]
    st.shift_row = shift_row


def _drive(world, mode, keep_turns, rec=None):
    """context, a spoken turn, an added turn, then a line that fits only without the second turn; -> (conversation, call log of
    the overflowing turn, history length before it)."""
    gen, m = world["gen"], world["m"]
    conv = gen.conversation(context=_context(), on_overflow=mode, keep_turns=keep_turns)
    log = []
    with _Scripted(m):
        conv.generate("one", 0, max_audio_length_ms=MS)
        conv.add(_seg(3, 20, 1, "and?"))
        L = conv.tokens.shape[0]
        assert conv._turns == [VOICE, SECOND, SPOKEN, ADDED] and conv.cached == VOICE + SECOND + SPOKEN - 2
        _watch(conv._state, log, rec)
        try:
            conv.generate("two", 0, max_audio_length_ms=(MAX_SEQ - L) * 80)      # history + text + frames >= max_seq_len
        finally:
            for name in ("prefill", "append", "shift_row"):
                conv._state.__dict__.pop(name, None)
    return conv, log, L


def test_shift_keeps_the_cache_and_appends(world):
    m = world["m"]
    rec = {}
    conv, log, L = _drive(world, "shift", 1, rec)
    old, old_log, _ = _drive(world, "drop_oldest", 1)
    # the same bookkeeping as drop_oldest with the same keep_turns after the same calls
    assert torch.equal(conv.tokens, old.tokens) and torch.equal(conv.mask, old.mask) and conv._turns == old._turns
    T = len(Tok().encode("[0]two"))
    frames = MAX_SEQ - L
    assert conv._turns == [VOICE, SPOKEN, ADDED, T + frames + 1] and conv.tokens.shape[0] == L - SECOND + T + frames + 1
    # ... but the cache was kept: one shift_row, one append, no prefill - and drop_oldest prefilled again
    cached = VOICE + SPOKEN - 2                                                  # what the shift left of the 54 cached positions
    assert log == [("shift", VOICE, SECOND), "append"] and old_log == ["prefill"]
    st = conv._state
    assert conv.cached > 0 and conv.cached == conv.tokens.shape[0] - 2 == int(st.bb.pos[0]) + 1 == st.row_pos[0] + 1
    # right after the shift: device position and host mirror at the new length - 1, nothing else of the state touched
    assert rec["pos"] == (cached - 1, cached - 1) and rec["untouched"]
    assert rec["before"].shape[3] == cached + SECOND and rec["after"].shape[3] == cached
    # the row's K after the shift is kv_shift_ref of a clone taken before, within the helper's bound; V and the head bit for bit
    worst = R.judge_shift("conversation", rec["after"], rec["before"], m.rope_table("backbone").cpu(), VOICE, SECOND)
    print(f"RATIO conversation_shift {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_drop_oldest_and_error_take_their_old_paths(world):
    """Next to a shift conversation in the same process: drop_oldest (keep_turns = 0, as before) drops the leading turn and
    prefills what is left from position 0, error raises the reference's message and changes nothing."""
    gen, m = world["gen"], world["m"]
    _drive(world, "shift", 1)
    old, log, L = _drive(world, "drop_oldest", 0)
    assert log == ["prefill"] and old._turns[:3] == [SECOND, SPOKEN, ADDED]       # the voice prompt went first
    assert old.cached == old.tokens.shape[0] - 2 == int(old._state.bb.pos[0]) + 1
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_audio_frames"):
        _drive(world, "error", 0)
    with pytest.raises(ValueError, match="keep_turns"):
        gen.conversation(on_overflow="shift", keep_turns=-1)
    assert "generate_frame" not in m.__dict__ and "_frame_tail" not in m.engine.__dict__


# ------------------------------------------------------------------------------------------------------------------ serving
def _finish(srv):
    for _ in srv.run():
        pass


def _served(world, plain_before, plain_after, others):
    """A seeded probe conversation and ``others`` more, all with on_overflow="shift", keep_turns=1 and the same turn lengths, so
    that their second lines overflow at the same boundary; ``plain_before`` / ``plain_after`` plain requests are queued around
    the probe's ``say``.  -> (probe, [codes of its two turns], its slot in round 2, append_rows log, prefill_row log, shift log)."""
    srv = world["gen"].serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)
    st = srv._state
    appends, prefills, shifts = [], [], []
    orig_append, orig_prefill, orig_shift = st.append_rows, st.prefill_row, st.shift_parked

    def append_rows(rows, *a):
        appends.append(list(rows))
        return orig_append(rows, *a)

    def prefill_row(b, *a):
        prefills.append(b)
        return orig_prefill(b, *a)

    def shift_parked(parked, keep, drop):
        shifts.append((parked.shape[3], keep, drop))
        return orig_shift(parked, keep, drop)
    st.append_rows, st.prefill_row, st.shift_parked = append_rows, prefill_row, shift_parked
    convs = [srv.conversation(context=_context(40 + i), on_overflow="shift", keep_turns=1, seed=900 + i) for i in range(others)]
    probe = srv.conversation(context=_context(), on_overflow="shift", keep_turns=1, seed=1234)
    first = [c.say("one", 0, max_audio_length_ms=MS) for c in convs + [probe]]
    _finish(srv)
    assert all(r.done and r.codes().shape == (K, 6) for r in first)
    for i, c in enumerate(convs + [probe]):
        c.add(_seg(60 + i if c is not probe else 3, 20, 1, "and?"))
        # (a served turn samples to the end of its chunk: all six kept frames were fed back, only the EOS frame is pending)
        assert c._turns == [VOICE, SECOND, SPOKEN, ADDED] and c.cached == VOICE + SECOND + SPOKEN - 1 and c._parked is not None
    L = probe.tokens.shape[0]
    big = (MAX_SEQ - L - 3) * 80                                                 # say charges chunk_frames - 1 = 3 more
    del appends[:], prefills[:]
    for c in convs:
        c.say("two", 0, max_audio_length_ms=big)
    for i in range(plain_before):
        srv.submit("filler", 2, [], seed=i, max_audio_length_ms=(4 + i % 5) * 80)
    r = probe.say("two", 0, max_audio_length_ms=big)
    for i in range(plain_after):
        srv.submit("late filler", 1, [], seed=70 + i, max_audio_length_ms=7 * 80)
    # at say: the parked cache slid, the history lost its second turn, the cache is still there
    cached = VOICE + SPOKEN - 1
    assert all(c._turns[:3] == [VOICE, SPOKEN, ADDED] and c.cached == cached and c._parked.shape[3] == cached for c in convs + [probe])
    srv.step()
    slot = r.slot
    _finish(srv)
    assert r.done
    world["m"]._decode_state = None
    return probe, [first[-1].codes(), r.codes()], slot, appends, prefills, shifts


def test_served_conversations_overflow_at_one_boundary(world):
    alone, codes_a, slot_a, app_a, pre_a, sh_a = _served(world, 3, 0, 0)
    among, codes_b, slot_b, app_b, pre_b, sh_b = _served(world, 7, 4, 4)
    assert slot_a == 3 and slot_b == 11
    # one stacked append_rows admits every overflowing turn; only the plain requests are prefilled
    assert app_a == [[3]] and sorted(pre_a) == [0, 1, 2]
    assert app_b == [[0, 1, 2, 3, 11]] and sorted(pre_b) == [4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15]
    full = VOICE + SECOND + SPOKEN - 1
    assert sh_a == [(full, VOICE, SECOND)] and sh_b == [(full, VOICE, SECOND)] * 5
    # the seeded conversation: the same codes in slot 3 alone and in slot 11 among 15 others
    for a, b in zip(codes_a, codes_b):
        assert a.shape[0] == K and torch.equal(a, b)
    assert codes_a[1].shape[1] > 6
    assert torch.equal(alone.tokens, among.tokens) and alone.cached == among.cached > 0 and alone._turns == among._turns
