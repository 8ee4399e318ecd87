"""Served conversations on the GPU: csm_attn_append_rows (the ragged append) against the one-row kernel and fp32, DecodeState
append_rows / park_row / resume_row, and BatchServer.conversation - a seeded conversation's codes and audio do not depend on its
slot, its neighbours, the appends stacked with its own or where it is resumed.

Everything that compares our own paths with each other is torch.equal.  The two accuracy bounds are the ones of
tests/test_conversation_gpu.py, built the same way: the rows kernel may err at most 2x what csm_attn_fwd errs against fp32
attention over the same cases, and the served cache at most 2x what one from-scratch prefill errs against the fp32 oracle."""
import pytest
import torch

from test_conversation_gpu import HD, S_MAX, _bits, _caches, _rand_qkv, _ref_rows, _split
from test_serving_gpu import TEMP, TOPK, Tok, _adapter, _hf_mimi

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K = 32
GUARD = 0.1005859375
KSHAPES = [(32, 8), (8, 8), (8, 4)]               # (H, KV): H / KV = 4, 1, 2


# ------------------------------------------------------------------------------------------------------------- kernel
def _segments(R):
    """(cache row, pos0, n) of R segments: mixed lengths and positions, cache rows in non-ascending order."""
    ns = [130, 1, 17, 16, 15, 3, 64, 1, 33, 16, 130, 2, 17, 1, 15, 48]
    p0 = [63, 0, 64, S_MAX - 16, 1000, S_MAX - 3, 0, 63, 64, 1, 500, S_MAX - 2, 0, 2047, 127, 65]
    rows = [(7 * r + 5) % 17 for r in range(16)]                      # 5, 12, 2, 9, 16, 6, ... : distinct mod 17, not sorted
    segs = [(rows[r], p0[r], ns[r]) for r in range(R)]
    assert all(p + n <= S_MAX for _, p, n in segs) and len({b for b, _, _ in segs}) == R
    return segs


def _problem(segs, H, KV, B, seed):
    """Per segment a random sequence of pos0 + n positions: its first pos0 in its cache row, the rest stacked into qkv."""
    kc = torch.full((B, KV, S_MAX, HD), GUARD, dtype=BF, device="cuda")
    vc = torch.full((B, KV, S_MAX, HD), GUARD, dtype=BF, device="cuda")
    new, full = [], []
    for j, (b, pos0, n) in enumerate(segs):
        qkv = _rand_qkv(pos0 + n, H, KV, seed=seed + 31 * j)
        _, k, v = _split(qkv, H, KV)
        kc[b, :, :pos0] = k[:pos0].permute(1, 0, 2)
        vc[b, :, :pos0] = v[:pos0].permute(1, 0, 2)
        new.append(qkv[pos0:])
        full.append(qkv)
    return torch.cat(new, 0).contiguous(), kc, vc, full


def _rows_launch(qkv, kc, vc, segs, H, KV):
    from csm.hip import ops
    out = torch.full((qkv.shape[0], H * HD), 3.0, dtype=BF, device="cuda")
    ops.attn_append_rows(qkv, kc, vc, out, [b for b, _, _ in segs], [p for _, p, _ in segs], [n for _, _, n in segs], H, KV, HD)
    return out


@pytest.mark.parametrize("H,KV", KSHAPES)
@pytest.mark.parametrize("R", [1, 3, 16])
def test_rows_kernel_equals_one_row_kernel(dev, H, KV, R):
    from csm.hip import ops
    segs = _segments(R)
    B = 17
    qkv, kc, vc, _ = _problem(segs, H, KV, B, seed=100 * R + H)
    k0, v0 = kc.clone(), vc.clone()
    kc1, vc1 = kc.clone(), vc.clone()
    got = _rows_launch(qkv, kc, vc, segs, H, KV)
    want, off = [], 0
    for b, pos0, n in segs:                                            # the same segments one by one through csm_attn_append
        o = torch.empty(n, H * HD, dtype=BF, device="cuda")
        ops.attn_append(qkv[off:off + n].contiguous(), kc1, vc1, o, b, pos0, H, KV, HD)
        want.append(o)
        off += n
    assert torch.equal(_bits(got), _bits(torch.cat(want, 0)))
    assert torch.equal(_bits(kc), _bits(kc1)) and torch.equal(_bits(vc), _bits(vc1))
    listed = {b for b, _, _ in segs}
    rest = [b for b in range(B) if b not in listed]
    assert torch.equal(_bits(kc[rest]), _bits(k0[rest])) and torch.equal(_bits(vc[rest]), _bits(v0[rest]))
    for b, pos0, n in segs:                                            # and inside a listed row only positions pos0 .. pos0+n-1
        keep = torch.ones(S_MAX, dtype=torch.bool, device="cuda")
        keep[pos0:pos0 + n] = False
        assert torch.equal(_bits(kc[b][:, keep]), _bits(k0[b][:, keep])) and torch.equal(_bits(vc[b][:, keep]), _bits(v0[b][:, keep]))
        assert not torch.equal(_bits(kc[b][:, pos0:pos0 + n]), _bits(k0[b][:, pos0:pos0 + n]))


def test_rows_kernel_accuracy_vs_fp32(dev):
    """The cases, the fp32 reference and the bound of test_conversation_gpu.py::test_attn_append_accuracy_vs_fp32 (with the 8/8
    and 8/4 shapes added), the seven positions of one length stacked into one rows launch.
    Measured on one MI355X, max abs error: H/KV = 4/2 rows kernel 7.9e-3, csm_attn_fwd 8.4e-3; 32/8 9.0e-3, 9.2e-3; 8/8 7.8e-3,
    7.8e-3; 8/4 8.4e-3, 9.2e-3 (bound 1.85e-2)."""
    from csm.hip import ops
    worst_app, worst_fwd = 0.0, 0.0
    for H, KV in [(4, 2), (32, 8), (8, 8), (8, 4)]:
        w_app, w_fwd = 0.0, 0.0
        for n in (1, 5, 16, 17, 64, 200):
            p0s = (0, 1, 63, 64, 65, 1000, S_MAX - n)
            segs = [(6 - j, pos0, n) for j, pos0 in enumerate(p0s)]
            kc = torch.zeros(7, KV, S_MAX, HD, dtype=BF, device="cuda")
            vc = torch.zeros(7, KV, S_MAX, HD, dtype=BF, device="cuda")
            seqs = []
            for b, pos0, _ in segs:
                qkv = _rand_qkv(pos0 + n, H, KV, seed=1000 * n + pos0 + H)
                k1, v1 = _caches(qkv, H, KV, pos0)
                kc[b], vc[b] = k1[0], v1[0]
                seqs.append(qkv)
            got = _rows_launch(torch.cat([q[p:] for q, (_, p, _) in zip(seqs, segs)], 0).contiguous(), kc, vc, segs, H, KV)
            for j, (qkv, (_, pos0, _)) in enumerate(zip(seqs, segs)):
                S = pos0 + n
                ref = _ref_rows(qkv, H, KV, pos0)
                full = torch.empty(S, H * HD, dtype=BF, device="cuda")
                lse = torch.empty(1, H, S, dtype=torch.float32, device="cuda")
                ops.attn_fwd(qkv, full, lse, 1, S, H, KV, HD)
                e_app = float((got[j * n:(j + 1) * n].float() - ref).abs().max())
                e_fwd = float((full[pos0:].float() - ref).abs().max())
                assert e_app == e_app, (H, KV, n, pos0)                  # NaN
                w_app, w_fwd = max(w_app, e_app), max(w_fwd, e_fwd)
        print(f"attn_append_rows H={H} KV={KV}: max |err| vs fp32 rows {w_app:.3e}, attn_fwd {w_fwd:.3e}")
        worst_app, worst_fwd = max(worst_app, w_app), max(worst_fwd, w_fwd)
    print(f"attn_append_rows all cases: rows {worst_app:.3e}, attn_fwd {worst_fwd:.3e}, bound {2 * worst_fwd:.3e}")
    assert worst_app <= 2 * worst_fwd, (worst_app, worst_fwd)


def test_rows_kernel_bad_arguments(dev):
    import ctypes
    from csm.hip import CsmHipError, check, lib, ops
    H, KV, s_max, B = 4, 2, 64, 3
    qkv = _rand_qkv(16, H, KV, seed=5)
    kc = torch.full((B, KV, s_max, HD), 0.5, dtype=BF, device="cuda")
    vc = torch.full((B, KV, s_max, HD), 0.5, dtype=BF, device="cuda")
    k0, v0 = kc.clone(), vc.clone()
    out = torch.full((16, H * HD), 3.0, dtype=BF, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def raw(rows=(1, 0), pos0=(0, 0), n=(8, 8), R=None, hd=HD, h=H, kv=KV, q=qkv.data_ptr(), tab=True):
        arr = ctypes.c_int * 17
        r_, p_, n_ = arr(*rows), arr(*pos0), arr(*n)
        return lib.csm_attn_append_rows(q, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), r_ if tab else None, p_, n_,
                                        len(rows) if R is None else R, h, kv, hd, s_max, 0.125, stream)

    def refused(rc, *words):
        msg = lib.csm_last_error()
        assert rc == 1 and msg.startswith(b"csm_attn_append_rows") and all(w in msg for w in words), (rc, msg)

    refused(raw(q=None), b"null pointer")
    refused(raw(tab=False), b"null pointer")
    refused(raw(rows=(), pos0=(), n=()), b"0 segments")
    refused(raw(R=17), b"17 segments")
    refused(raw(n=(8, 0)), b"n = 0 new positions")
    refused(raw(n=(8, -2)), b"new positions")
    refused(raw(pos0=(0, s_max - 7)), b"outside the cache")
    refused(raw(pos0=(-1, 0)), b"outside the cache")
    refused(raw(hd=128), b"head_dim 128 unsupported")
    refused(raw(h=16, kv=2), b"8 query heads per kv head unsupported")
    refused(raw(h=5), b"bad shape")
    refused(raw(rows=(1, 1)), b"batch row 1 appears in two segments")
    refused(raw(rows=(-1, 0)), b"batch row -1")
    for rows in ((0, 3), (-1, 0)):                                     # a row outside the cache batch: ops.attn_append_rows
        with pytest.raises(CsmHipError, match="outside the caches"):
            ops.attn_append_rows(qkv, kc, vc, out, rows, (0, 0), (8, 8), H, KV, HD)
    with pytest.raises(CsmHipError, match="two segments"):
        ops.attn_append_rows(qkv, kc, vc, out, (2, 2), (0, 0), (8, 8), H, KV, HD)
    with pytest.raises(CsmHipError, match="qkv has 16 rows"):
        ops.attn_append_rows(qkv, kc, vc, out, (0, 1), (0, 0), (8, 7), H, KV, HD)
    torch.cuda.synchronize()
    assert torch.equal(kc, k0) and torch.equal(vc, v0) and bool((out == 3.0).all())          # nothing was launched
    check(raw(pos0=(0, s_max - 8)), "csm_attn_append_rows")                                  # the last legal position is fine
    torch.cuda.synchronize()
    assert not torch.equal(kc, k0) and torch.equal(kc[2], k0[2])


# ------------------------------------------------------------------------------------------------------------- engine
def _tiny(seed=2):
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, K), device="cuda", seed=seed)
    m.engine._need()
    return m


def _frames(S, seed):
    """[S, K+1] tokens / mask: a text segment, then audio frames."""
    g = torch.Generator().manual_seed(seed)
    nt = max(1, S // 3)
    tk = torch.zeros(S, K + 1, dtype=torch.long)
    mk = torch.zeros(S, K + 1, dtype=torch.bool)
    tk[:nt, K] = torch.randint(3, 300, (nt,), generator=g)
    mk[:nt, K] = True
    tk[nt:, :K] = torch.randint(0, 2051, (S - nt, K), generator=g)
    mk[nt:, :K] = True
    return tk.cuda(), mk.cuda()


def _kv(st):
    return st.bb.kv.clone()


@pytest.mark.parametrize("adapter", [False, True])
def test_append_rows_one_segment_equals_append(dev, adapter):
    from csm.engine import DecodeState
    m = _tiny()
    ads = [_adapter(m, 1)] if adapter else None
    tk, mk = _frames(60, seed=3)
    outs = []
    for rows_form in (False, True):
        st = DecodeState(m.engine, 1, ads)
        st.prefill(tk[:23].unsqueeze(0), mk[:23].unsqueeze(0))
        hs = []
        for lo, hi in ((23, 30), (30, 31), (31, 60)):                  # 7 (below the GEMM's 8-row threshold), 1 and 29 positions
            if rows_form:
                h = st.append_rows([0], [tk[lo:hi]], [mk[lo:hi]])
                assert h.shape == (1, m.bb.embed_dim)
            else:
                h = st.append(tk[lo:hi], mk[lo:hi])
            assert st.cur == hi - 1 and int(st.bb.pos[0]) == hi - 1
            hs.append(h.clone())
        outs.append((torch.cat(hs, 0), _kv(st)))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    assert torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    with pytest.raises(RuntimeError, match="holds nothing"):
        DecodeState(m.engine, 2).append_rows([1], [tk[:4]], [mk[:4]])


def test_append_rows_stacked_equals_alone_and_refusals(dev):
    """A segment's hidden row and cache rows do not depend on what is stacked with it - 11 segments with three adapters (two
    forwards of four, one of three) against each segment alone on its row."""
    from csm.engine import DecodeState
    m = _tiny()
    bank = [_adapter(m, 1), _adapter(m, 2)]
    rows = [9, 0, 15, 3, 4, 12, 7, 1, 14, 6, 10]
    pre = [5 + 3 * j for j in range(11)]
    new = [1, 7, 40, 16, 17, 3, 33, 8, 2, 25, 9]

    def state():
        st = DecodeState(m.engine, 16, bank=bank)
        for j, b in enumerate(rows):
            st.set_row_adapter(b, [None, bank[0], bank[1]][j % 3])
            tk, mk = _frames(pre[j] + new[j], seed=50 + j)
            st.prefill_row(b, tk[:pre[j]], mk[:pre[j]])
        return st

    feeds = [_frames(pre[j] + new[j], seed=50 + j) for j in range(11)]
    st = state()
    h = st.append_rows(rows, [f[0][pre[j]:] for j, f in enumerate(feeds)], [f[1][pre[j]:] for j, f in enumerate(feeds)])
    assert [st.row_pos[b] for b in rows] == [pre[j] + new[j] - 1 for j in range(11)]
    assert st.bb.pos.tolist() == [st.row_pos[b] if b in rows else 0 for b in range(16)]
    one = state()
    for j, b in enumerate(rows):
        hj = one.append_rows([b], [feeds[j][0][pre[j]:]], [feeds[j][1][pre[j]:]])
        assert torch.equal(_bits(hj[0]), _bits(h[j])), (j, b)
    assert torch.equal(_bits(_kv(st)), _bits(_kv(one)))
    tk, mk = feeds[0]
    with pytest.raises(ValueError, match="distinct"):
        st.append_rows([9, 9], [tk[:2], tk[:2]], [mk[:2], mk[:2]])
    with pytest.raises(RuntimeError, match="holds nothing"):
        st.append_rows([2], [tk[:2]], [mk[:2]])
    with pytest.raises(ValueError, match="max_seq_len"):
        st.append_rows([9], [tk.repeat(40, 1)], [mk.repeat(40, 1)])


def test_park_resume_reproduces_cache_and_next_frame(dev):
    from csm.engine import DecodeState
    m = _tiny()
    st = DecodeState(m.engine, 16)
    tk, mk = _frames(37, seed=8)
    st.prefill_row(2, tk, mk)
    other_t, other_m = _frames(11, seed=9)
    st.prefill_row(5, other_t, other_m)
    parked = st.park_row(2, 37)
    L, KV = m.bb.num_layers, m.bb.num_kv_heads
    assert parked.shape == (L, 2, KV, 37, HD) and parked.is_contiguous()
    for i in range(L):
        assert torch.equal(_bits(parked[i, 0]), _bits(st.bb.k[i][2, :, :37])) and torch.equal(_bits(parked[i, 1]), _bits(st.bb.v[i][2, :, :37]))
    five = st.bb.kv[:, :, 5].clone()
    st.resume_row(11, parked)
    assert st.row_pos[11] == 36 and int(st.bb.pos[11]) == 36
    assert torch.equal(_bits(st.bb.kv[:, :, 11, :, :37]), _bits(parked)) and torch.equal(_bits(st.bb.kv[:, :, 5]), _bits(five))
    # the next frame of the resumed row equals the next frame of the row it was parked from
    tok = torch.zeros(16, 1, K + 1, dtype=torch.long, device="cuda")
    frame = torch.randint(0, 2051, (K,), generator=torch.Generator().manual_seed(4)).cuda()
    tok[2, 0, :K] = frame
    tok[11, 0, :K] = frame
    msk = torch.cat([torch.ones(16, 1, K, dtype=torch.bool), torch.zeros(16, 1, 1, dtype=torch.bool)], 2).cuda()
    st.set_row_seed(2, 99)
    st.set_row_seed(11, 99)
    st.set_active([2, 11])
    out = st.serve_frame(tok, msk, TEMP, TOPK)
    assert torch.equal(out[2], out[11])
    assert torch.equal(_bits(st.bb.kv[:, :, 2, :, :38]), _bits(st.bb.kv[:, :, 11, :, :38]))
    with pytest.raises(ValueError):
        st.park_row(2, 40)
    with pytest.raises(ValueError):
        st.resume_row(3, parked[:, :1])
    m._decode_state = None


# ------------------------------------------------------------------------------------------------------------ serving
MS = 6 * 80                                        # six frames per turn: ends inside the second chunk of 4
LINES = [("one", 0), ("two two", 0), ("three", 0)]


@pytest.fixture(scope="module")
def world(dev):
    from csm.codec import MimiCodec
    from csm.generator import Generator
    codec = MimiCodec(_hf_mimi().state_dict(), device="cuda")
    m = _tiny()
    banked = Generator(m, text_tokenizer=Tok(), audio_tokenizer=codec)
    for name, seed in (("a1", 1), ("a2", 2)):
        banked.add_adapter(name, _adapter(m, seed))
    return dict(m=m, codec=codec, gen=banked)


def _seg(seed, frames=3, speaker=1, text="and?"):
    from csm.generator import Segment
    return Segment(speaker, text, torch.randn(frames * 1920, generator=torch.Generator().manual_seed(seed)) * 0.2)


def _serve(gen):
    return gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)


def _finish(srv):
    for _ in srv.run():
        pass


def _dialogue(srv, adapter=None, before=lambda t: None, after=lambda t: None):
    """The probe: a seeded conversation of three spoken turns with an added turn between them; ``before`` / ``after`` queue the
    neighbours of turn t around the probe's ``say`` (all of them start at the same chunk boundary).  Returns (conversation,
    [(codes, audio, slot) per turn])."""
    conv = srv.conversation(context=[_seg(1, 5, 0, "hi")], adapter=adapter, seed=1234)
    turns = []
    for t, (text, speaker) in enumerate(LINES):
        if t:
            conv.add(_seg(10 + t))
        before(t)
        r = conv.say(text, speaker, max_audio_length_ms=MS)
        after(t)
        srv.step()
        slot = r.slot
        _finish(srv)
        assert r.done and r.codes().shape == (K, 6) and r.audio().numel() == 6 * 1920
        turns.append((r.codes(), r.audio(), slot))
    return conv, turns


def _same(a, b):
    for (ca, aa, _), (cb, ab, _) in zip(a, b):
        assert torch.equal(ca, cb) and torch.equal(aa, ab)


@pytest.fixture(scope="module")
def alone(world):
    conv, turns = _dialogue(_serve(world["gen"]))
    assert [s for _, _, s in turns] == [0, 0, 0]
    return conv, turns


def test_conversation_among_fifteen_others(world, alone):
    """15 neighbours whose turns start at the probe's boundaries: 11 seeded conversations (their resumed turns are stacked with
    the probe's into one append_rows from the second round on) and 4 plain requests."""
    srv = _serve(world["gen"])
    names = [None, "a1", "a2"]
    others = [srv.conversation(context=[_seg(30 + i, 2 + i % 4, 0, "c" * (1 + i))] if i % 2 else [], adapter=names[i % 3], seed=500 + i)
              for i in range(11)]
    log = []
    orig = srv._state.append_rows

    def counting(rows, *a):
        log.append(list(rows))
        return orig(rows, *a)
    srv._state.append_rows = counting

    def say(i, t):
        return others[i].say(f"line {t} of {i}", i % 3, max_audio_length_ms=(3 + (i + t) % 6) * 80)

    def before(t):
        for i in range(6):
            say(i, t)
        for i in range(2):
            srv.submit("plain " * (1 + i), 2, [_seg(3)] if i else [], adapter=names[(i + t) % 3], seed=t if i else None, max_audio_length_ms=(5 + 4 * i) * 80)

    def after(t):
        for i in range(6, 11):
            say(i, t)
        for i in range(2):
            srv.submit("late plain", 1, [], seed=70 + i, max_audio_length_ms=7 * 80)
    conv, turns = _dialogue(srv, before=before, after=after)
    assert [s for _, _, s in turns] == [8, 8, 8]
    assert [len(r) for r in log] == [12, 12]                            # rounds 2 and 3: twelve resumed turns in one call each
    _same(turns, alone[1])
    assert torch.equal(conv.tokens, alone[0].tokens) and conv.cached == alone[0].cached


def test_conversation_resumed_in_a_different_slot_each_turn(world, alone):
    srv = _serve(world["gen"])

    def before(t):                                                      # 3, 1, 6 plain requests take the lowest slots first
        for i in range((3, 1, 6)[t]):
            srv.submit("filler", 2, [], seed=i, max_audio_length_ms=(4 + i) * 80)
    conv, turns = _dialogue(srv, before=before)
    assert [s for _, _, s in turns] == [3, 1, 6]
    _same(turns, alone[1])


def test_conversation_with_adapter_among_other_adapters(world, alone):
    gen = world["gen"]
    conv_a, turns_a = _dialogue(_serve(gen), adapter="a1")
    assert not torch.equal(turns_a[0][0], alone[1][0][0])              # the adapter changes what is said
    srv = _serve(gen)
    others = [srv.conversation(adapter=[None, "a2", "a1", "a2"][i % 4], seed=900 + i) for i in range(9)]

    def before(t):
        for i in range(5):
            others[i].say(f"o{i} {t}", 1, max_audio_length_ms=(4 + i) * 80)

    def after(t):
        for i in range(5, 9):
            others[i].say(f"o{i} {t}", 2, max_audio_length_ms=(4 + i % 3) * 80)
    conv_b, turns_b = _dialogue(srv, adapter="a1", before=before, after=after)
    assert [s for _, _, s in turns_b] == [5, 5, 5]
    _same(turns_b, turns_a)


def test_plain_request_not_disturbed_by_conversations(world):
    gen = world["gen"]

    def plain(srv):
        return srv.submit("the line we follow", 1, [_seg(1, 5, 0, "hi")], seed=77, max_audio_length_ms=14 * 80)
    srv = _serve(gen)
    a = plain(srv)
    _finish(srv)
    srv = _serve(gen)
    convs = [srv.conversation(seed=i, adapter=[None, "a1"][i % 2]) for i in range(6)]
    for i, c in enumerate(convs):
        c.say(f"first {i}", 0, max_audio_length_ms=(3 + i) * 80)
    _finish(srv)
    for i, c in enumerate(convs[:3]):
        c.say(f"second {i}", 0, max_audio_length_ms=(9 + i) * 80)
    srv.step()
    b = plain(srv)
    for i, c in enumerate(convs[3:]):
        c.say(f"second late {i}", 0, max_audio_length_ms=(5 + i) * 80)     # resumed at the boundary the plain request joins at
    _finish(srv)
    assert b.done and a.codes().shape == (K, 14)
    assert torch.equal(a.codes(), b.codes()) and torch.equal(a.audio(), b.audio())


def _script_eos(srv, slot, at_call):
    """The real frames (the cache is fed), with row ``slot``'s result of serve_frame call number ``at_call`` replaced by zeros."""
    st = srv._state
    orig, calls = st.serve_frame, []

    def scripted(*a, **k):
        out = orig(*a, **k)
        calls.append(1)
        if len(calls) == at_call:
            out = out.clone()
            out[slot] = 0
        return out
    st.serve_frame = scripted
    return lambda: setattr(st, "serve_frame", orig)


def test_parked_history_equals_a_fresh_feed(world):
    """After a turn that ends at its length limit in the middle of a chunk and after one that ends by EOS, the parked K / V are
    those of a fresh state fed the same history the same way (prefill, the kept frames one decode frame each, the next feed by
    append_rows) - bit for bit, position 1 included: the row was never idled while it held the history."""
    from csm.engine import DecodeState
    gen, m = world["gen"], world["m"]
    srv = _serve(gen)
    srv.submit("neighbour", 2, [], seed=1, max_audio_length_ms=40 * 80)               # slot 0: runs through both turns
    conv = srv.conversation(context=[_seg(1, 5, 0, "hi")], seed=5)
    fresh = DecodeState(m.engine, 16, bank=list(gen._bank.entries.values()))
    msk = torch.cat([torch.ones(16, 1, K, dtype=torch.bool), torch.zeros(16, 1, 1, dtype=torch.bool)], 2).cuda()
    row = 7

    def replay(req, first):
        if first:
            fresh.prefill_row(row, req._tokens, req._mask)
        else:
            fresh.append_rows([row], [req._tokens], [req._mask])
        assert fresh.row_pos[row] == req._base - 1
        for f in range(conv.cached - req._base):                       # the kept frames that were fed back, one decode frame each
            tok = torch.zeros(16, 1, K + 1, dtype=torch.long, device="cuda")
            tok[row, 0, :K] = req.codes()[:, f]
            fresh.set_active([row])
            fresh.serve_frame(tok, msk, TEMP, TOPK)
        m._decode_state = srv._state
        assert fresh.row_pos[row] == conv.cached - 1
        mine = fresh.park_row(row, conv.cached)
        assert torch.equal(_bits(mine), _bits(conv._parked))

    r1 = conv.say("one", 0, max_audio_length_ms=MS)                     # length limit: 6 frames, the row samples 8
    _finish_one = lambda r: [srv.step() for _ in range(8) if not r.done]       # noqa: E731
    _finish_one(r1)
    assert r1.done and r1._sampled == 8 and r1.codes().shape == (K, 6) and conv.cached == r1._base + 6
    replay(r1, True)
    conv.add(_seg(11))
    r2 = conv.say("two two", 0, max_audio_length_ms=30 * 80)
    undo = _script_eos(srv, 1, at_call=6)                               # serve_frame calls 1 .. 4: the first chunk; 6: frame 6 = EOS
    try:
        _finish_one(r2)
    finally:
        undo()
    assert r2.done and r2.slot is None and r2.codes().shape == (K, 5) and conv.cached == r2._base + 5
    assert not conv.tokens[-1].any() and bool(conv.tokens[-2].any())
    replay(r2, False)
    _finish(srv)


# ------------------------------------------------------------------------------------------- closeness to a from-scratch prefill
class SumRowsCodec:
    """A rows codec for the oracle's 4-codebook tiny model (Mimi has 32): Mimi's protocol, arithmetic that does not matter here."""
    sample_rate = 24000

    def __init__(self, k, vocab):
        self.k, self.vocab = k, vocab

    def encode(self, audio):
        T = audio.shape[-1] // 1920
        g = torch.Generator().manual_seed(T)
        return torch.randint(0, self.vocab, (1, self.k, T), generator=g).to(audio.device)

    def decode(self, codes):
        return codes.float().sum(1, keepdim=True).repeat_interleave(1920, -1)

    def decode_stream_rows(self, slots=16, max_chunk_frames=32):
        return type("Rows", (), {"open": lambda s, slot: None, "step": lambda s, rows, codes: codes.float().sum(1).repeat_interleave(1920, -1)})()


def test_served_cache_vs_one_prefill_against_oracle(dev):
    """The bound of tests/test_conversation_gpu.py::test_append_vs_one_prefill_against_oracle: the codebook-0 logits the served
    cache gives at the last position may err against the fp32 oracle at most 2x what ONE from-scratch prefill of ``conv.tokens``
    errs.  Measured on one MI355X (92 positions, 91 of them cached, max |logit| 0.76): served 4.5e-3, one prefill 4.9e-3."""
    from csm.engine import DecodeState
    from csm.generator import Generator
    from test_conversation_gpu import _c0_logits, _oracle, _tiny_oracle_model
    O, T = _oracle()
    m, p32 = _tiny_oracle_model()
    gen = Generator(m, text_tokenizer=Tok(), audio_tokenizer=SumRowsCodec(T.n_codebooks, T.audio_vocab))
    srv = gen.serve(slots=16, chunk_frames=4, temperature=TEMP, topk=TOPK)
    srv.submit("neighbour", 2, [], seed=1, max_audio_length_ms=60 * 80)
    conv = srv.conversation(context=[_seg(1, 5, 0, "hi")], seed=3)
    for t, (text, speaker) in enumerate(LINES):
        if t:
            conv.add(_seg(10 + t, 4))
        r = conv.say(text, speaker, max_audio_length_ms=MS)
        while not r.done:
            srv.step()
    assert conv.cached < conv.tokens.shape[0] and conv._parked is not None
    st = srv._state
    with torch.inference_mode():                                       # (the server's state was made under it)
        st.resume_row(9, conv._parked)
        h = st.append_rows([9], [conv.tokens[conv.cached:]], [conv.mask[conv.cached:]])
        got = _c0_logits(m, h)
    one = _c0_logits(m, DecodeState(m.engine, 1).prefill(conv.tokens.unsqueeze(0), conv.mask.unsqueeze(0)))
    with torch.no_grad():
        hid = O.backbone_hidden(p32, T, conv.tokens.cpu().unsqueeze(0), conv.mask.cpu().unsqueeze(0))
        ref = hid[0, -1].float() @ p32["codebook0_head.weight"].t().float()
    e_srv, e_one = float((got.cpu() - ref).abs().max()), float((one.cpu() - ref).abs().max())
    print(f"served cache vs oracle after {len(LINES)} turns ({conv.tokens.shape[0]} positions, {conv.cached} cached): served "
          f"{e_srv:.3e}, one prefill {e_one:.3e}, max |logit| {float(ref.abs().max()):.3e}")
    m._decode_state = None
    assert e_srv <= 2 * e_one, (e_srv, e_one)
