"""Several speakers' LoRA adapters in one batch, everything that needs no device: the float64 reference of the row-selected skinny
product (tests/lora_rows_ref.py) against a restatement in the kernel's order and against wrong restatements, the proof that the
stacked-and-masked K-extension form IS the per-row dense LoRA form (values and every adapter's own gradients, float64 autograd),
and the host logic - stack layout and its 256-column limit, ``sel`` from adapter ids (padded and packed), the collate
pass-through, the speaker rotation."""
import types

import pytest
import torch

import lora_rows_ref as R
from csm import hip
from csm.data.training_data import collate_packed, collate_variable_length
from csm.engine import adapter_rows
from csm.training.lora import KX_MAX, LoRAState, stack_width
from csm.training.multi_speaker_lora import rotation_draws

F64 = torch.float64
_inputs = {}


def _in(name):
    if name not in _inputs:
        _inputs[name] = R.inputs(R.CASE[name])
    return _inputs[name]


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_what_it_must():
    cs = R.CASES
    assert {c.M for c in cs} == set(R.MS) and {c.K for c in cs} == set(R.KS)
    assert {(c.N, c.blk) for c in cs} == {(32, 8), (32, 16), (64, 16), (96, 24), (256, 16), (256, 32)}
    assert {(c.N, c.blk, c.pattern) for c in cs} >= {(N, b, p) for N, b, _ in R.SHAPES for p in R.PATTERNS}
    for c in cs:
        assert c.N % 32 == 0 and 32 <= c.N <= 256 and c.blk % 8 == 0 and c.K % 128 == 0 and c.A * c.blk <= c.N
        sel = R.sel_of(c)
        assert sel.dtype == torch.int32 and sel.shape == (c.M,) and int(sel.min()) >= -1 and int(sel.max()) < c.A
    by = {p: [c for c in cs if c.pattern == p] for p in R.PATTERNS}
    assert all((R.sel_of(c) == -1).all() for c in by["all_none"])
    for c in by["dead_tile"]:
        assert bool((R.sel_of(c)[16:32] == -1).all()) and c.M >= 33
    for c in by["runs_mid"]:                                       # a change strictly inside a 16-row tile
        s = R.sel_of(c)
        assert any(int(s[m]) != int(s[m - 1]) and m % 16 for m in range(1, c.M))
    for c in by["last_partial"]:
        assert c.M % 16 and int(R.sel_of(c)[-1]) == c.A - 1
    for c in by["poison"]:
        i = _in(c.name)
        rows = i["sel"] < 0
        assert bool(rows.any()) and not bool(torch.isfinite(i["X"][rows].float()).all(1).any())
        assert bool(torch.isfinite(i["X"][~rows].float()).all())
    assert any(c.A * c.blk < c.N for c in cs)                      # padding columns exist somewhere


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_restatement_in_kernel_order_fits_the_bound(name):
    c, i = R.CASE[name], _in(name)
    worst = R.judge_bits(f"restate.{name}", c, i, R.restate(i))
    print(f"RATIO restate {name} {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_wrong_restatements_fail(mut):
    hit = [c for c in R.CASES if R.MUTANT_CASES[mut](c)]
    assert hit, mut
    for c in hit:
        i = _in(c.name)
        with pytest.raises(AssertionError):
            R.judge_bits(f"{mut}.{c.name}", c, i, R.restate(i, mut))


def test_guard_overwrite_is_seen():
    c = R.CASES[0]
    i = _in(c.name)
    buf = R.restate(i)
    buf.view(torch.int16)[0] = 0
    with pytest.raises(AssertionError, match="guard"):
        R.judge_bits("guard", c, i, buf)
    buf = R.restate(i)
    R.window(c, buf)[0, (int(i["sel"][0]) + 1) % (c.N // c.blk) * c.blk] = -0.0       # -0 is not the +0 the contract names
    with pytest.raises(AssertionError):
        R.judge_bits("negzero", c, i, buf)


# ------------------------------------------------------------------------------------------------------------ the LoRA form
@pytest.mark.parametrize("members,r,A,sel", [
    (2, 8, 3, [0, 2, -1, 1, 1, 0, 2, 2, -1, 0]),                   # q|v, three adapters
    (3, 8, 2, [1, 1, 0, -1, 0, 1, 0]),                             # q|k|v
    (1, 16, 4, [3, 0, 1, 2, 2, -1]),                               # a one-member group (w2)
])
def test_stacked_masked_form_is_the_per_row_dense_form(members, r, A, sel):
    g = torch.Generator().manual_seed(members * 100 + A)
    in_f, out_each, M = 40, 12, len(sel)
    N_out = members * out_each
    rows_of = [slice(j * out_each, (j + 1) * out_each) for j in range(members)]
    blk, s = members * r, 2.0
    kx = stack_width(members, r, A)
    As = [[torch.randn(r, in_f, generator=g, dtype=F64).requires_grad_() for _ in range(members)] for _ in range(A)]
    Bs = [[torch.randn(out_each, r, generator=g, dtype=F64).requires_grad_() for _ in range(members)] for _ in range(A)]
    x = torch.randn(M, in_f, generator=g, dtype=F64, requires_grad=True)
    W0 = torch.randn(N_out, in_f, generator=g, dtype=F64)
    dy = torch.randn(M, N_out, generator=g, dtype=F64)
    sel_t = torch.tensor(sel)
    At, Bx, mask = R.stacked_operands([[a.detach() for a in row] for row in As], [[b.detach() for b in row] for row in Bs],
                                      rows_of, N_out, blk, kx)
    y_s = R.stacked_forward(x, W0, At, Bx, sel_t, blk, s)
    y_d = R.dense_forward(x, W0, As, Bs, rows_of, sel_t, s)
    tol = 1e-12 * float(y_d.abs().max())
    assert float((y_s - y_d).abs().max()) <= tol
    (gx_s, gAt, gBx) = torch.autograd.grad((y_s * dy).sum(), (x, At, Bx))
    flat = [t for row in As for t in row] + [t for row in Bs for t in row]
    used = sorted({a for a in sel if a >= 0})
    grads = torch.autograd.grad((y_d * dy).sum(), [x] + flat, allow_unused=True)
    gx_d, gA, gB = grads[0], grads[1:1 + A * members], grads[1 + A * members:]
    assert float((gx_s - gx_d).abs().max()) <= 1e-12 * float(gx_d.abs().max())
    gBx = gBx * mask                                               # (the mask mechanism of LoRAGroup.backward)
    big = max(float(gAt.abs().max()), float(gBx.abs().max()))
    for a in range(A):
        for j in range(members):
            c0 = a * blk + j * r
            wantA = gA[a * members + j] if gA[a * members + j] is not None else torch.zeros(r, in_f, dtype=F64)
            wantB = gB[a * members + j] if gB[a * members + j] is not None else torch.zeros(out_each, r, dtype=F64)
            assert float((gAt[:, c0:c0 + r].t() - wantA).abs().max()) <= 1e-12 * big
            assert float((gBx[rows_of[j], c0:c0 + r] - wantB).abs().max()) <= 1e-12 * big
            if a not in used:                                      # an adapter no row names: exactly zero, not merely small
                assert not bool(gAt[:, c0:c0 + r].any()) and not bool(gBx[:, a * blk:(a + 1) * blk].any())
    assert not bool((gBx * (1 - mask)).any()) and not bool(gAt[:, A * blk:].any())


# ------------------------------------------------------------------------------------------------------------ layout
def test_stack_width_and_the_256_limit():
    assert stack_width(2, 8) == 32 and stack_width(3, 8) == 32 and stack_width(2, 16) == 32 and stack_width(5, 8) == 64   # as before
    assert stack_width(2, 8, 16) == 256 and stack_width(3, 8, 10) == 256 and stack_width(3, 8, 3) == 96 and stack_width(1, 8, 5) == 64
    assert KX_MAX == 256
    with pytest.raises(ValueError, match="at most 16 adapter sets"):
        stack_width(2, 8, 17, ["q_proj", "v_proj"])
    with pytest.raises(ValueError, match="at most 10 adapter sets"):
        stack_width(3, 8, 11)


def _fake_model():
    st = types.SimpleNamespace(num_heads=4, num_kv_heads=2, head_dim=16, embed_dim=64, intermediate_dim=128, num_layers=2)
    return types.SimpleNamespace(bb=st, dc=types.SimpleNamespace(**{**vars(st), "num_layers": 1}), device=torch.device("cpu"))


SEVEN = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"]


def test_state_limits_and_refusals():
    m = _fake_model()
    LoRAState(m, 8, 16.0, 0.0, ["q_proj", "v_proj"], None, False, n_adapters=16)
    with pytest.raises(ValueError, match="at most 16 adapter sets"):
        LoRAState(m, 8, 16.0, 0.0, ["q_proj", "v_proj"], None, False, n_adapters=17)
    LoRAState(m, 8, 16.0, 0.0, SEVEN, None, False, n_adapters=10)
    with pytest.raises(ValueError, match="at most 10 adapter sets"):
        LoRAState(m, 8, 16.0, 0.0, SEVEN, None, False, n_adapters=11)
    with pytest.raises(ValueError, match="dropout"):
        LoRAState(m, 8, 16.0, 0.1, ["q_proj"], None, False, n_adapters=2)
    with pytest.raises(ValueError, match="bias"):
        LoRAState(m, 8, 16.0, 0.0, ["q_proj"], None, True, n_adapters=2)
    with pytest.raises(ValueError):
        LoRAState(m, 8, 16.0, 0.0, ["q_proj"], None, False, n_adapters=0)


@pytest.mark.parametrize("mods,r", [(["q_proj", "v_proj"], 8), (SEVEN, 4), (["q_proj", "v_proj", "w2"], 5)])
def test_stack_layout_views_and_seeds(mods, r):
    m, A = _fake_model(), 3
    st = LoRAState(m, r, 16.0, 0.0, mods, None, False, seed=7, n_adapters=A)
    singles = [LoRAState(m, r, 16.0, 0.0, mods, None, False, seed=7 + a) for a in range(A)]
    assert LoRAState(m, r, 16.0, 0.0, mods, None, False, seed=7).arena.equal(singles[0].arena)        # the default is the old state
    for (key, G) in st.groups.items():
        G1 = singles[0].groups[key]
        members = len(G.adapters)
        assert G.blk == members * st.r_pad and G.kx == stack_width(members, st.r_pad, A) and G1.kx == stack_width(members, st.r_pad)
        assert not bool(G.At[:, A * G.blk:].any()) and not bool(G.Bx.any())                             # padding zero, B = 0
        for a in range(A):
            Ga = singles[a].groups[key]
            assert G.At[:, a * G.blk:(a + 1) * G.blk].equal(Ga.At[:, :G.blk])                           # members lie as they do alone
        if members > 1:                                            # entries outside every adapter's own (rows, columns) block
            assert G.mask is not None
            for a in range(A):
                assert G.mask[:, a * G.blk:(a + 1) * G.blk].equal(G1.mask[:, :G.blk])
            assert not bool(G.mask[:, A * G.blk:].any())
    with pytest.raises(ValueError, match="adapter=a"):
        list(st.named_tensors())
    with pytest.raises(ValueError, match="out of range"):
        list(st.named_tensors(adapter=A))
    for a in range(A):
        mine, alone = dict(st.named_tensors(adapter=a)), dict(singles[a].named_tensors())
        assert list(mine) == list(alone)
        for k in mine:
            assert mine[k].shape == alone[k].shape and mine[k].equal(alone[k]), k
    assert st.num_params() == A * singles[0].num_params()
    # export: copies, in a fresh single-adapter state
    with torch.no_grad():
        for a in range(A):
            for k, t in st.named_tensors(adapter=a):
                if k.endswith("lora_B"):
                    t.fill_(a + 1.0)
    e = st.export(1)
    assert e.n_adapters == 1 and e.grad_arena is None and not e.training and e.arena.data_ptr() != st.arena.data_ptr()
    want = dict(st.named_tensors(adapter=1))
    for k, t in e.named_tensors():
        assert t.equal(want[k]), k
    for G in e.groups.values():                                    # nothing but the adapter's own blocks is set
        if G.mask is not None:
            assert not bool((G.Bx * (1 - G.mask)).any())
    with torch.no_grad():
        next(iter(want.values())).add_(1.0)
    assert not next(iter(dict(e.named_tensors()).values())).equal(next(iter(want.values())))


# ------------------------------------------------------------------------------------------------------------ sel
def test_sel_from_example_ids():
    sel = adapter_rows([0, 2, -1, 1], 4, 5, 3)
    assert sel.dtype == torch.int32 and sel.tolist() == [0] * 5 + [2] * 5 + [-1] * 5 + [1] * 5
    assert adapter_rows(torch.tensor([1]), 1, 3, 2).tolist() == [1, 1, 1]


def test_sel_from_packed_segment_ids():
    L = torch.tensor([[3, 2, 0], [4, 0, 0], [2, 2, 2]])
    ids = torch.tensor([[1, 0, -1], [2, -1, -1], [0, -1, 2]])
    sel = adapter_rows(ids, 3, 7, 3, segment_lengths=L)
    assert sel.view(3, 7).tolist() == [[1, 1, 1, 0, 0, -1, -1], [2, 2, 2, 2, -1, -1, -1], [0, 0, -1, -1, 2, 2, -1]]
    # the id of a segment that does not exist is never read
    ids2 = ids.clone()
    ids2[1, 2] = 99
    assert adapter_rows(ids2, 3, 7, 3, segment_lengths=L).equal(sel)


@pytest.mark.parametrize("ids,kw,msg", [
    ([0, 3, 1, 1], {}, "out of range"),
    ([0, -2, 1, 1], {}, "out of range"),
    ([0, 1, 1], {}, "shape"),
    ([[0, 1], [1, 0], [0, 0], [1, 1]], {}, "shape"),
    ([0.0, 1.0, 1.0, 0.0], {}, "integers"),
    ([0, 1, 1, 0], {"segment_lengths": torch.tensor([[2, 2]] * 4)}, "shape"),
    ([[0, 5]] * 4, {"segment_lengths": torch.tensor([[2, 2]] * 4)}, "out of range"),
])
def test_sel_range_and_shape_errors(ids, kw, msg):
    with pytest.raises(ValueError, match=msg):
        adapter_rows(ids, 4, 6, 3, **kw)


# ------------------------------------------------------------------------------------------------------------ data
def _item(n, t, adapter=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    it = {"input_tokens": torch.randint(0, 50, (n, 5), generator=g), "input_masks": torch.ones(n, 5, dtype=torch.bool),
          "target_audio_tokens": torch.randint(0, 50, (t, 4), generator=g)}
    if adapter is not None:
        it["adapter"] = adapter
    return it


def test_collate_passes_adapters_through():
    plain = [_item(5, 4, seed=1), _item(3, 2, seed=2), _item(7, 6, seed=3)]
    tagged = [dict(it, adapter=a) for it, a in zip(plain, (2, 0, 1))]
    a, b = collate_variable_length(plain), collate_variable_length(tagged)
    assert "adapter_ids" not in a and set(a) == {"input_tokens", "input_masks", "target_audio_tokens"}
    assert b["adapter_ids"].tolist() == [2, 0, 1] and all(a[k].equal(b[k]) for k in a)
    assert collate_variable_length([tagged[0], plain[1]])["adapter_ids"].tolist() == [2, -1]
    pa, pb = collate_packed(plain, max_seq_len=128), collate_packed(tagged, max_seq_len=128)
    assert "adapter_ids" not in pa and all(pa[k].equal(pb[k]) for k in pa)
    assert pb["adapter_ids"].shape == pb["segment_lengths"].shape
    # first-fit by decreasing length: one row, the examples in the order 7, 5, 3
    assert pb["segment_lengths"].tolist() == [[7, 5, 3]] and pb["adapter_ids"].tolist() == [[1, 2, 0]]
    two = collate_packed([dict(_item(100, 9, seed=4), adapter=0), dict(_item(90, 9, seed=5), adapter=1), dict(_item(20, 9, seed=6), adapter=2)],
                         max_seq_len=128)
    assert two["segment_lengths"].tolist() == [[100, 20], [90, 0]] and two["adapter_ids"].tolist() == [[0, 2], [1, -1]]
    sel = adapter_rows(two["adapter_ids"], 2, 128, 3, segment_lengths=two["segment_lengths"]).view(2, 128)
    assert sel[0].tolist() == [0] * 100 + [2] * 20 + [-1] * 8 and sel[1].tolist() == [1] * 90 + [-1] * 38


def test_speaker_rotation():
    assert rotation_draws([4, 4, 4], 0, 4) == [(0, 0), (1, 0), (2, 0), (0, 1)]
    assert rotation_draws([4, 4, 4], 1, 4) == [(1, 1), (2, 1), (0, 2), (1, 2)]
    # every speaker's examples are walked in order, wrapping; a speaker without data is left out
    seen = {0: [], 2: []}
    for step in range(6):
        for sp, ex in rotation_draws([3, 0, 2], step, 2):
            seen[sp].append(ex)
    assert seen == {0: [0, 1, 2, 0, 1, 2], 2: [0, 1, 0, 1, 0, 1]}
    with pytest.raises(ValueError):
        rotation_draws([0, 0], 0, 2)


def test_entry_point_is_declared():
    assert "csm_skinny_nt_sel_bf16" in hip.EXPORTS and hasattr(hip.lib, "csm_skinny_nt_sel_bf16")
    assert len(hip._SIGS["csm_skinny_nt_sel_bf16"][0]) == 13 and hip.lib.csm_abi_version() == 3


def test_multi_cli_flags_and_config(tmp_path):
    import json
    from csm.cli import finetune_lora_multi as cli
    cfg = tmp_path / "speakers.json"
    cfg.write_text(json.dumps([{"name": "a", "speaker_id": 3, "synthetic": 8}, {"name": "b", "speaker_id": 5, "synthetic": 8}]))
    a = cli.parse_args(["--model-path", "", "--output-dir", str(tmp_path), "--speakers-config", str(cfg)])
    assert (a.lora_r, a.lora_alpha, a.batch_size, a.epochs, a.val_split, a.save_mode, a.context_turns) == (8, 16.0, 2, 5, 0.1, "lora", 2)
    assert [c["speaker_id"] for c in cli.load_speaker_configs(str(cfg))] == [3, 5]
    assert len(cli.load_speaker_configs(str(cfg), 1)) == 1
    cfg.write_text(json.dumps([{"name": "a", "speaker_id": 3, "synthetic": 8, "lora_r": 4}]))
    with pytest.raises(ValueError, match="lora_r"):
        cli.load_speaker_configs(str(cfg))
    cfg.write_text(json.dumps([{"name": "a", "speaker_id": 3, "synthetic": 8}, {"name": "b", "speaker_id": 3, "synthetic": 8}]))
    with pytest.raises(ValueError, match="distinct"):
        cli.load_speaker_configs(str(cfg))
