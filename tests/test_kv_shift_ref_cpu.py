"""The KV-cache context shift without a GPU: tests/kv_shift_ref.py proved against the oracle's rope and against wrong restatements,
and the host bookkeeping of ``on_overflow="shift"`` / ``keep_turns`` of both conversation classes against the stub states of
tests/test_conversation_cpu.py and tests/test_serve_conversation_cpu.py (extended by the shift only)."""
import pytest
import torch

import kv_shift_ref as R
import test_conversation_cpu as TC
import test_serve_conversation_cpu as TS

CPU_CASES = [c for c in R.CASES if c[3] <= 65] + [(2, 2, 64, 200, 7, 64), (1, 2, 128, 200, 1, 63)]


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("hd", [64, 128])
def test_reference_composes_with_the_oracle_rope(hd):
    """rope(k_raw, p + d) rotated by -d is rope(k_raw, p): exact float64 table, through oracle.rope."""
    O = R.oracle()
    theta = O.llama3_inv_freq(hd, 500_000.0, 32.0).double()
    ang = torch.arange(2048, dtype=torch.float64)[:, None] * theta[None]
    table = torch.stack([torch.cos(ang), torch.sin(ang)], -1)                       # [2048, hd/2, 2] float64
    g = torch.Generator().manual_seed(5)
    k_raw = torch.randn(1, 1, 3, hd, generator=g, dtype=torch.float64)              # [B, S, heads, hd]
    for p, d in ((0, 1), (7, 64), (100, 1500), (546, 1500), (1, 2046)):
        at = O.rope(k_raw, table, torch.tensor([[p + d]]))
        back = R.rotate_back64(at, table[d])
        want = O.rope(k_raw, table, torch.tensor([[p]]))
        assert float((back - want).abs().max()) < 1e-12, (p, d)
        # ... and the oracle's own rope with the sine negated says the same
        neg = table.clone()
        neg[..., 1] = -neg[..., 1]
        assert float((O.rope(at, neg, torch.tensor([[d]])) - want).abs().max()) < 1e-12


@pytest.mark.parametrize("case", CPU_CASES + [R.LATE], ids=lambda c: "x".join(map(str, c)))
def test_fp32_restatement_fits_every_bound(case):
    layers, KV, HD, length, keep, drop = case
    src, table = R.random_src(layers, KV, HD, length), R.rope_table(R.TABLE_ROWS, HD)
    before = src.clone()
    dst = R.restate_fp32(src, table, keep, drop)
    worst = R.judge_shift("restate", dst, src, table, keep, drop)
    assert worst <= 1.0 and torch.equal(src, before)
    if length - drop - keep > 0:
        assert worst > 0.0                                                          # the tail's keys were really rounded


MUTANTS = ("plus_d", "no_rotation", "half_split", "v_rotated", "head_rotated", "src_row_minus_1", "table_row_plus_1", "truncate")


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("case", [(2, 2, 64, 65, 7, 8), (1, 2, 128, 64, 7, 8), (2, 1, 64, 200, 1, 63)], ids=lambda c: "x".join(map(str, c)))
def test_wrong_restatements_are_rejected(case, mutant):
    layers, KV, HD, length, keep, drop = case
    src, table = R.random_src(layers, KV, HD, length, seed=1), R.rope_table(R.TABLE_ROWS, HD)
    assert R.judge_shift("right", R.restate_fp32(src, table, keep, drop), src, table, keep, drop) <= 1.0
    with pytest.raises(AssertionError):
        R.judge_shift(mutant, R.restate_fp32(src, table, keep, drop, mutant), src, table, keep, drop)


@pytest.mark.parametrize("geom,pos,d", R.INVARIANCE)
def test_invariance_tolerance_takes_the_restatement_and_rejects_wrong_rotations(geom, pos, d):
    """Float64 attention over the fp32 restatement's shifted cache (the kernel's roundings: q and the new k rotated at pos - d)
    fits the invariance tolerance; a shift by +d, by the next table row or by nothing does not."""
    import decode_attn_ref as D
    c, src = R.invariance_problem(geom, pos, d)
    ref, tol = R.invariance_reference(c, src, d)

    def ratio(mutant):
        kc, vc = R.shifted_caches(c, R.restate_fp32(src, c.table, 0, d, mutant), d)
        sim = D.ref_decode_attention(c.qkv, kc, vc, [pos - d], c.H, c.KV, c.HD, c.table)
        return R.invariance_ratio(sim.out.float().to(R.BF16), ref, tol)
    assert ratio(None) <= 1.0
    for mutant in ("plus_d", "table_row_plus_1", "no_rotation"):
        assert ratio(mutant) > 1.0, mutant


def test_cases_cover_the_shapes_asked_for():
    cs = R.CASES
    assert {c[0] for c in cs} == {1, 2} and {c[1] for c in cs} == {1, 2} and {c[2] for c in cs} == {64, 128}
    assert {c[3] for c in cs} == {2, 9, 64, 65, 200} and {c[4] for c in cs} >= {0, 1, 7} and {c[5] for c in cs} >= {1, 8, 63, 64}
    assert any(k + d == n - 1 for _, _, _, n, k, d in cs) and R.LATE[3:] == (2047, 1, 1500)
    assert all(d >= 1 and k >= 0 and k + d <= n and n - d >= 1 for _, _, _, n, k, d in cs + [R.LATE])


# ----------------------------------------------------------------------------------------------- Conversation bookkeeping
class ShiftState(TC.State):
    """tests/test_conversation_cpu.py's stub plus ``shift_row``: the cache loses positions keep .. keep+drop-1."""

    def shift_row(self, b, keep, drop):
        flat = self.content()
        assert b == 0 and drop >= 1 and keep >= 0 and keep + drop <= flat.shape[0] and flat.shape[0] - drop >= 1
        self.fed = [torch.cat([flat[:keep], flat[keep + drop:]], 0)]
        self.cur -= drop
        self.log.append(("shift", keep, drop))


@pytest.fixture
def make(monkeypatch):
    import csm.conversation as C
    from csm.generator import Generator
    monkeypatch.setattr(C, "DecodeState", ShiftState)
    TC.State.made = []

    def _make(**kw):
        gen = Generator(TC.StubModel(TC._frames(40)), text_tokenizer=TC.Tok(), audio_tokenizer=TC.Codec())
        return gen, gen.conversation(**kw)
    return _make


def _seg_len(gen, seg):
    return gen._tokenize_segment(seg)[0].shape[0]


def _text_len(gen, text, speaker=0):
    return gen._tokenize_text_segment(text, speaker)[0].shape[0]


def _frames_to_lose(conv, gen, text, lose):
    """A frame budget with which ``text`` fits only once the first ``lose`` positions after the kept head are gone."""
    L, T = conv.tokens.shape[0], _text_len(gen, text)
    f = TC.MAX_SEQ - (L - lose) - T - 1
    assert f > 0
    return f


CTX = lambda: [TC._seg(3, "a"), TC._seg(4, "b"), TC._seg(2, "c")]              # noqa: E731


@pytest.mark.parametrize("keep_turns", [0, 1, 2])
def test_which_turns_go(make, keep_turns):
    gen, conv = make(context=CTX(), on_overflow="shift", keep_turns=keep_turns)
    _, old = make(context=CTX(), on_overflow="drop_oldest", keep_turns=keep_turns)
    lens = [_seg_len(gen, s) for s in CTX()]
    for c in (conv, old):
        c.generate("hi", 0, max_audio_length_ms=3 * 80)
    before, turns = conv.tokens.clone(), list(conv._turns)
    head, gone = sum(lens[:keep_turns]), turns[keep_turns]                      # exactly the first turn after the kept head goes
    f = _frames_to_lose(conv, gen, "next", gone)
    assert before.shape[0] + _text_len(gen, "next") + f >= TC.MAX_SEQ
    for c in (conv, old):
        c.generate("next", 0, max_audio_length_ms=f * 80)
    n0 = before.shape[0] - gone
    assert torch.equal(conv.tokens[:n0], torch.cat([before[:head], before[head + gone:]], 0))
    assert torch.equal(conv.tokens, old.tokens) and torch.equal(conv.mask, old.mask) and conv._turns == old._turns
    assert conv._turns[:len(turns) - 1] == turns[:keep_turns] + turns[keep_turns + 1:]
    TC._check_cache(conv)
    TC._check_cache(old)
    # the shift kept the cache: one shift_row, then an append - and drop_oldest prefilled again
    ops = [e for e in conv._state.log if e[0] in ("prefill", "append", "shift")]
    assert ops[1:] == [("shift", head, gone), ("append", 2 + _text_len(gen, "next"))]
    assert [e[0] for e in old._state.log if e[0] in ("prefill", "append", "shift")] == ["prefill", "prefill"]
    assert ("prefill", n0 + _text_len(gen, "next")) in old._state.log


def test_cached_after_shift_all_dropped_positions_cached(make):
    gen, conv = make(context=CTX(), on_overflow="shift", keep_turns=1)
    a, b = _seg_len(gen, CTX()[0]), _seg_len(gen, CTX()[1])
    conv.generate("hi", 0, max_audio_length_ms=3 * 80)
    L, c = conv.tokens.shape[0], conv.cached
    assert c == L - 2 and a + b <= c                                            # the last frame and the EOS frame are pending
    conv.generate("next", 0, max_audio_length_ms=_frames_to_lose(conv, gen, "next", b) * 80)
    log = conv._state.log
    i = log.index(("shift", a, b))
    assert log[i + 1] == ("append", 2 + _text_len(gen, "next"))                  # fed by append, not prefilled again
    assert sum(e[0] == "prefill" for e in log) == 1 and len(TC.State.made) == 1
    TC._check_cache(conv)


def test_cached_after_shift_some_dropped_positions_pending(make):
    gen, conv = make(context=[TC._seg(3, "a")], on_overflow="shift", keep_turns=1)
    a = _seg_len(gen, TC._seg(3, "a"))
    conv.generate("hi", 0, max_audio_length_ms=20 * 80)                          # turn 1: cached but for its last two frames
    L, c = conv.tokens.shape[0], conv.cached
    spoken = conv._turns[1]
    assert c == L - 2 and a < c
    f = _frames_to_lose(conv, gen, "next", spoken)
    conv.generate("next", 0, max_audio_length_ms=f * 80)
    log = conv._state.log
    i = log.index(("shift", a, c - a))                                           # only what was cached is shifted out ...
    assert log[i + 1] == ("append", _text_len(gen, "next"))                      # ... the pending frames just leave the feed
    assert sum(e[0] == "prefill" for e in log) == 1
    TC._check_cache(conv)


def test_dropped_positions_all_pending_leave_the_cache_alone(make):
    gen, conv = make(context=[TC._seg(3, "a")], on_overflow="shift", keep_turns=2)
    conv.generate("hi", 0, max_audio_length_ms=3 * 80)
    conv.add(TC._seg(4, "b"))
    conv.add(TC._seg(2, "c"))
    c, b = conv.cached, conv._turns[2]
    pending = conv.tokens.shape[0] - c
    conv.generate("next", 0, max_audio_length_ms=_frames_to_lose(conv, gen, "next", b) * 80)
    log = conv._state.log
    assert not any(e[0] == "shift" for e in log) and sum(e[0] == "prefill" for e in log) == 1
    assert ("append", pending - b + _text_len(gen, "next")) in log
    TC._check_cache(conv)


def test_nothing_cached_is_kept_behaves_as_drop_oldest(make):
    gen, conv = make(on_overflow="shift")
    conv.generate("hi", 0, max_audio_length_ms=20 * 80)
    conv.add(TC._seg(3, "b"))
    first = conv._turns[0]
    assert 0 < conv.cached < first
    L = conv.tokens.shape[0]
    conv.generate("next", 0, max_audio_length_ms=_frames_to_lose(conv, gen, "next", first) * 80)
    log = [e for e in conv._state.log if e[0] in ("prefill", "append", "shift")]
    assert log == [("prefill", _text_len(gen, "hi")), ("prefill", L - first + _text_len(gen, "next"))]
    TC._check_cache(conv)


def test_empty_cache_behaves_as_drop_oldest(make):
    gen, conv = make(context=CTX(), on_overflow="shift", keep_turns=1)
    a, b = _seg_len(gen, CTX()[0]), _seg_len(gen, CTX()[1])
    L = conv.tokens.shape[0]
    conv.generate("next", 0, max_audio_length_ms=_frames_to_lose(conv, gen, "next", b) * 80)     # a first turn that overflows
    assert conv._state.log[0] == ("prefill", L - b + _text_len(gen, "next")) and not any(e[0] == "shift" for e in conv._state.log)
    TC._check_cache(conv)
    gen, conv = make(context=CTX(), on_overflow="shift", keep_turns=1)              # ... and after reset()
    conv.generate("hi", 0, max_audio_length_ms=3 * 80)
    assert conv.cached > a + b
    conv.reset()
    assert conv.cached == 0
    L = conv.tokens.shape[0]
    conv.generate("next", 0, max_audio_length_ms=_frames_to_lose(conv, gen, "next", b) * 80)
    log = TC.State.made[-1].log
    assert log[0] == ("prefill", L - b + _text_len(gen, "next")) and not any(e[0] == "shift" for e in log)
    TC._check_cache(conv)


def test_drop_oldest_without_keep_turns_leaves_todays_log(make):
    """The scenario of tests/test_conversation_cpu.py::test_overflow_error_and_drop_oldest, log and all."""
    gen, conv = make(context=[TC._seg(5, "a"), TC._seg(6, "b")], on_overflow="drop_oldest")
    conv.generate("hi", 0, max_audio_length_ms=3 * 80)
    first = _seg_len(gen, TC._seg(5, "a"))
    before = conv.tokens.clone()
    L, T = before.shape[0], _text_len(gen, "next")
    frames = TC.MAX_SEQ - (L - first) - T - 1
    conv.generate("next", 0, max_audio_length_ms=frames * 80)
    assert torch.equal(conv.tokens[:L - first], before[first:])
    assert [e for e in conv._state.log if e[0] != "truncate"] == [("prefill", L - 3 - 1), ("prefill", L - first + T)]
    assert conv._keep_turns == 0
    TC._check_cache(conv)


@pytest.mark.parametrize("mode", ["shift", "drop_oldest"])
def test_inputs_too_long_when_the_kept_head_does_not_fit(make, mode):
    gen, conv = make(context=CTX(), on_overflow=mode, keep_turns=3)
    before, turns = conv.tokens.clone(), list(conv._turns)
    with pytest.raises(ValueError, match=r"Inputs too long, must be below max_seq_len - max_audio_frames: 14"):
        conv.generate("hi", 0, max_audio_length_ms=50 * 80)                      # every turn is kept: nothing may go
    assert torch.equal(conv.tokens, before) and conv._turns == turns and conv.cached == 0
    gen, conv = make(context=CTX(), on_overflow=mode, keep_turns=1)
    with pytest.raises(ValueError, match="Inputs too long"):                     # the head alone is too long for this line
        conv.generate("x" * 40, 0, max_audio_length_ms=10 * 80)
    assert torch.equal(conv.tokens, before) and conv._turns == turns


@pytest.mark.parametrize("bad", [-1, 1.0, "1", None, True])
def test_bad_keep_turns(make, bad):
    gen, _ = make()
    with pytest.raises(ValueError, match="keep_turns"):
        gen.conversation(keep_turns=bad)
    with pytest.raises(ValueError, match="keep_turns"):
        gen.conversation(on_overflow="shift", keep_turns=bad)


def test_overflow_values():
    from csm.conversation import OVERFLOW
    assert OVERFLOW == ("error", "drop_oldest", "shift")


# ----------------------------------------------------------------------------------------- ServedConversation bookkeeping
class ShiftServeState(TS.State):
    """tests/test_serve_conversation_cpu.py's stub plus ``shift_parked`` on its parked histories (the frames themselves)."""

    def shift_parked(self, parked, keep, drop):
        assert drop >= 1 and keep >= 0 and keep + drop <= parked.shape[0] and parked.shape[0] - drop >= 1
        self.log.append(("shift", keep, drop))
        return torch.cat([parked[:keep], parked[keep + drop:]], 0)


@pytest.fixture
def serve(monkeypatch):
    import csm.serving as S
    from csm.generator import Generator
    monkeypatch.setattr(S, "DecodeState", ShiftServeState)
    TS.State.made, TS.State.scripts = [], {}

    def _make(scripts, **kw):
        TS.State.scripts = scripts
        gen = Generator(TS.StubModel(), text_tokenizer=TS.Tok(), audio_tokenizer=TS.RowsCodec())
        srv = gen.serve(**kw)
        return gen, srv, TS.State.made[-1]
    return _make


SCRIPT = {0: [[1, 2, 3, 0] + [9] * 8]}


def _served_pair(serve, keep_turns, context):
    gen, srv, st = serve(SCRIPT, slots=2, chunk_frames=4)
    conv = srv.conversation(context=context(), on_overflow="shift", keep_turns=keep_turns)
    old = srv.conversation(context=context(), on_overflow="drop_oldest", keep_turns=keep_turns)
    for c in (conv, old):
        c.say("one", 0, max_audio_length_ms=8 * 80)
        TS._run(srv)
    return gen, srv, st, conv, old


@pytest.mark.parametrize("keep_turns", [0, 1, 2])
def test_served_which_turns_go_and_the_turn_is_appended(serve, keep_turns):
    ctx = lambda: [TS._seg(20, "first", 1), TS._seg(10, "second", 1)]          # noqa: E731
    gen, srv, st, conv, old = _served_pair(serve, keep_turns, ctx)
    assert conv.cached > 0 and conv._parked is not None and torch.equal(conv.tokens, old.tokens)
    before, turns, c = conv.tokens.clone(), list(conv._turns), conv.cached
    head, gone = sum(turns[:keep_turns]), turns[keep_turns]
    T = gen._tokenize_text_segment("two", 0)[0].shape[0]
    # the frame budget with which "two" fits only without the first turn after the kept head (say charges chunk_frames - 1 more)
    f = TS.MAX_SEQ - (before.shape[0] - gone) - T - 1 - 3
    assert f > 0 and before.shape[0] + T + f + 3 >= TS.MAX_SEQ
    del st.log[:]
    r = conv.say("two", 0, max_audio_length_ms=f * 80)
    old.say("two", 0, max_audio_length_ms=f * 80)
    assert torch.equal(conv.tokens, old.tokens) and torch.equal(conv.mask, old.mask) and conv._turns == old._turns
    assert conv._turns == turns[:keep_turns] + turns[keep_turns + 1:] + [T]
    assert old.cached == 0 and old._parked is None
    out = min(c, head + gone) - head
    if c - out >= 1:
        assert st.log == [("shift", head, out)] and conv.cached == c - out > 0
        assert torch.equal(conv._parked, conv.tokens[:conv.cached])              # the first ``cached`` positions of the new history
    else:
        assert st.log == [] and conv.cached == 0 and conv._parked is None
    srv.step()
    if c - out >= 1:
        # both overflowed at this boundary: the shifted one is resumed and appended, the other prefilled from position 0
        assert ("resume", 0, c - out) in st.log and ("append_rows", (0,), (before.shape[0] - gone - (c - out) + T,)) in st.log
        assert ("prefill", 1, before.shape[0] - gone + T) in st.log and not any(e[:2] == ("prefill", 0) for e in st.log)
    assert r.done


def test_served_nothing_cached_kept_and_empty_cache(serve):
    gen, srv, st = serve(SCRIPT, slots=2, chunk_frames=4)
    conv = srv.conversation(context=[TS._seg(20, "first", 1), TS._seg(30, "second", 1)], on_overflow="shift")
    L, first = conv.tokens.shape[0], conv._turns[0]
    T = gen._tokenize_text_segment("one", 0)[0].shape[0]
    f = TS.MAX_SEQ - (L - first) - T - 1 - 3
    assert L + T + f + 3 >= TS.MAX_SEQ
    conv.say("one", 0, max_audio_length_ms=f * 80)                               # a first turn that overflows: nothing parked yet
    assert conv.cached == 0 and conv._parked is None and conv.tokens.shape[0] == L - first + T
    srv.step()
    assert st.log[0] == ("prefill", 0, L - first + T) and not any(e[0] == "shift" for e in st.log)


def test_served_inputs_too_long_and_bad_keep_turns(serve):
    gen, srv, st = serve(SCRIPT, slots=2, chunk_frames=4)
    conv = srv.conversation(context=[TS._seg(20, "first", 1), TS._seg(30, "second", 1)], on_overflow="shift", keep_turns=2)
    before = conv.tokens.clone()
    with pytest.raises(ValueError, match="Inputs too long, must be below max_seq_len - max_audio_frames"):
        conv.say("one", 0, max_audio_length_ms=40 * 80)
    assert torch.equal(conv.tokens, before) and srv.queued == 0
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="keep_turns"):
            srv.conversation(keep_turns=bad)
    with pytest.raises(ValueError):
        srv.conversation(on_overflow="slide")


# ------------------------------------------------------------------------------------------------------- CLI and exports
def test_generate_cli_overflow_flags():
    from csm.cli.generate import parse_args
    base = ["--model-path", "c.pt", "--mimi-weights", "m", "--text-tokenizer", "t"]
    a = parse_args(base + ["--text", "hi"])
    assert a.on_overflow == "error" and a.keep_turns == 0
    a = parse_args(base + ["--text", "hi", "--next-text", "x", "--on-overflow", "shift", "--keep-turns", "2"])
    assert a.on_overflow == "shift" and a.keep_turns == 2
    a = parse_args(base + ["--serve-file", "f.jsonl", "--on-overflow", "drop_oldest", "--keep-turns", "1"])
    assert a.on_overflow == "drop_oldest" and a.keep_turns == 1
    for bad in (["--on-overflow", "slide"], ["--keep-turns", "-1"], ["--keep-turns", "x"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--text", "hi"] + bad)


def test_library_exports_kv_shift():
    import os
    import re
    from csm import hip
    from csm.engine import DecodeState
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "csm_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+csm_kv_shift\s*\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 11 == len(hip._SIGS["csm_kv_shift"][0])
    assert "csm_kv_shift" in hip.EXPORTS and hasattr(hip.lib, "csm_kv_shift") and callable(hip.ops.kv_shift)
    assert callable(DecodeState.shift_parked) and callable(DecodeState.shift_row)
    assert hip.lib.csm_abi_version() == 3                                        # additive: the ABI number stays
