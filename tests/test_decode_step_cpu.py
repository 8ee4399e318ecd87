"""The launch table of ``_DecodeStack.step`` (csm/engine.py), without a GPU: ``ops`` is replaced by a recorder and the stack by a
stand-in with CPU tensors, and every mode of the decode step - plain, FP8 weights, live LoRA, per-row adapters - must issue exactly
the launches listed here, on exactly these operands.  ``ops.gemv(x, W, y, residual)`` and an ``ops.gemv_ex`` without norm, SwiGLU
and gather are the same launch (both forward to one ``gemv_launch``, csrc/generate.hip) and are recorded alike."""
import inspect
import types

import pytest
import torch

BF = torch.bfloat16
LAYERS, H, KV, HD, D, F, S_MAX, EPS = 2, 1, 1, 128, 128, 16, 8, 1e-5
QKV = (H + 2 * KV) * HD
WEIGHTS = {"attn.qkv": (QKV, D), "attn.output_proj.weight": (D, H * HD), "mlp.w13": (2 * F, D), "mlp.w2.weight": (D, F),
           "sa_norm.scale": (D,), "mlp_norm.scale": (D,)}
OUT = {"rmsnorm_fwd": "y", "attn_decode_rope": "out", "lora_project": "t", "lora_project_rows": "t"}      # every other op: "y"


class Recorder:
    """Stands in for ``csm.hip.ops``: logs (op, arguments by parameter name) and returns the op's output argument."""

    def __init__(self, real):
        self.real, self.log = real, []

    def __getattr__(self, name):
        sig = inspect.signature(getattr(self.real, name))

        def op(*a, **kw):
            if name == "quantize_rows_fp8":
                W = a[0]
                return torch.zeros(W.shape, dtype=torch.uint8), torch.ones(W.shape[0], dtype=torch.float32)
            args = dict(sig.bind(*a, **kw).arguments)
            if "norm_scale" in sig.parameters and args.get("norm_scale") is None:
                args.pop("eps", None)                      # (eps without a norm prologue means nothing)
            op_name = name
            if name == "gemv_ex" and not (set(args) - {"x", "W", "y", "residual"}):
                op_name = "gemv"
            self.log.append((op_name, args))
            return args[OUT.get(name, "y")]
        return op


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.data_ptr() == b.data_ptr() and a.shape == b.shape
                and a.stride() == b.stride() and a.dtype == b.dtype)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _check(log, want):
    """``want``: (op, arguments) in launch order.  An argument that is not listed must not have been passed (or, for the gemv
    family's trailing options, be the signature's default)."""
    assert [op for op, _ in log] == [op for op, _ in want]
    for n, ((op, got), (_, exp)) in enumerate(zip(log, want)):
        for k in set(got) | set(exp):
            if k in exp:
                assert k in got and _same(got[k], exp[k]), f"launch {n} ({op}): argument {k}"
            else:
                assert got[k] is None or got[k] is False or (k == "row_offset" and got[k] == 0), f"launch {n} ({op}): unexpected {k}"


class FakeStack:
    """What ``_DecodeStack`` uses of ``_Stack``: the configuration, the weights by name (one tensor object per name) and the model's
    device and RoPE table."""
    prefix = "decoder"

    def __init__(self):
        self.c = types.SimpleNamespace(num_layers=LAYERS, num_heads=H, num_kv_heads=KV, head_dim=HD, intermediate_dim=F, embed_dim=D,
                                       qkv_dim=QKV, norm_eps=EPS)
        self.table = torch.zeros(S_MAX, HD, dtype=torch.float32)
        self.m = types.SimpleNamespace(device=torch.device("cpu"), rope_table=lambda prefix: self.table)
        self.ws = {"norm.scale": torch.ones(D, dtype=BF)}
        for i in range(LAYERS):
            for n, shape in WEIGHTS.items():
                self.ws[f"layers.{i}.{n}"] = torch.zeros(*shape, dtype=BF)

    def w(self, name, grad=False):
        return self.ws[name]


@pytest.fixture
def make(monkeypatch):
    import csm.engine as E
    rec = Recorder(E.ops)
    monkeypatch.setattr(E, "ops", rec)
    monkeypatch.delenv("CSM_DECODE_FUSE_ATTN", raising=False)
    monkeypatch.delenv("CSM_FP8_FUSE_ATTN", raising=False)

    def _make(B):
        ds = E._DecodeStack(FakeStack(), B, S_MAX)
        ds.pos_host = 3
        return ds, rec
    return _make


def _group(kx, bias_on=None, seed=0):
    """A LoRA group stand-in of the fused q|k|v projection (training/lora.py LoRAGroup): At [K, kx], Bx [N, kx], adapters by module."""
    ads = {mod: types.SimpleNamespace(bias=torch.full((HD,), 1.0 + j + seed, dtype=BF) if mod == bias_on else None)
           for j, mod in enumerate(("q_proj", "k_proj", "v_proj"))}
    return types.SimpleNamespace(kx=kx, name=f"decoder.layers.0.attn_in#{seed}", At=torch.zeros(D, kx, dtype=BF),
                                 Bx=torch.zeros(QKV, kx, dtype=BF), adapters=ads)


def _mlp_group(gname, kx):
    n, k, mods = {"mlp_out": (D, F, ("w2",)), "mlp_in": (2 * F, D, ("w1", "w3")), "attn_out": (D, H * HD, ("output_proj",))}[gname]
    return types.SimpleNamespace(kx=kx, name=f"decoder.layers.0.{gname}", At=torch.zeros(k, kx, dtype=BF), Bx=torch.zeros(n, kx, dtype=BF),
                                 adapters={mod: types.SimpleNamespace(bias=None) for mod in mods})


def _state(groups, scaling=2.0):
    """A LoRAState stand-in: ``groups`` {(layer, group name): group}."""
    return types.SimpleNamespace(scaling=scaling, arena=torch.zeros(1, dtype=BF),
                                 group=lambda prefix, layer, gname: groups.get((layer, gname)))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _plain(ds, name, x, y, **kw):
    """One plain product: ``gemv`` (no norm, no SwiGLU) or ``gemv_ex``."""
    W = ds.stack.ws[name]
    if set(kw) <= {"residual"}:
        return [("gemv", dict(x=x, W=W, y=y, **kw))]
    return [("gemv_ex", dict(x=x, W=W, y=y, **kw))]


def _fp8(ds, name, x, y, **kw):
    q, s = ds.w8[name]
    return [("gemv_fp8w", dict(x=x, W8=q, scale=s, y=y, **kw))]


def _layer(ds, i, cur, nxt, fused, products):
    """The launches of layer ``i``; ``products``: one table function per product (qkv, output projection, w13, w2)."""
    w = ds.stack.ws
    pq, po, p13, p2 = products
    attn = dict(qkv=ds.qkv, kcache=ds.k[i], vcache=ds.v[i], pos_i32=ds.pos, table=ds.stack.table, H=H, KV=KV, HD=HD, pos_host=3)
    out = pq(ds, f"layers.{i}.attn.qkv", cur, ds.qkv, norm_scale=w[f"layers.{i}.sa_norm.scale"], eps=EPS)
    if fused:
        out += [("gemv_attn", dict(attn, W=w[f"layers.{i}.attn.output_proj.weight"], y=ds.h, residual=cur))]
    else:
        out += [("attn_decode_rope", dict(attn, out=ds.o))]
        out += po(ds, f"layers.{i}.attn.output_proj.weight", ds.o, ds.h, residual=cur)
    out += p13(ds, f"layers.{i}.mlp.w13", ds.h, ds.act, norm_scale=w[f"layers.{i}.mlp_norm.scale"], eps=EPS, swiglu=True)
    out += p2(ds, f"layers.{i}.mlp.w2.weight", ds.act, nxt, residual=ds.h)
    return out


def _run(ds, rec, layers):
    """Both ``final_norm`` settings against ``layers`` = per layer (fused, four product table functions)."""
    x = torch.zeros(ds.B, D, dtype=BF)
    bufs = [x, ds.xa, ds.xb]                                    # layer 0: x -> xa, layer 1: xa -> xb
    want = []
    for i, (fused, products) in enumerate(layers):
        want += _layer(ds, i, bufs[i], bufs[i + 1], fused, products)
    rec.log.clear()
    assert ds.step(x, final_norm=False) is ds.xb
    _check(rec.log, want)
    rec.log.clear()
    assert ds.step(x) is ds.xf
    _check(rec.log, want + [("rmsnorm_fwd", dict(x=ds.xb, scale=ds.stack.ws["norm.scale"], y=ds.xf, eps=EPS))])
    return want


@pytest.mark.parametrize("B", [1, 2])
def test_plain(make, B):
    ds, rec = make(B)
    assert ds.fuse_attn == (B == 1)
    want = _run(ds, rec, [(B == 1, [_plain] * 4)] * LAYERS)
    assert len(want) == (4 if B == 1 else 5) * LAYERS
    assert [op for op, _ in want[:len(want) // LAYERS]] == (["gemv_ex", "gemv_attn", "gemv_ex", "gemv"] if B == 1 else
                                                            ["gemv_ex", "attn_decode_rope", "gemv", "gemv_ex", "gemv"])


@pytest.mark.parametrize("B", [1, 2])
def test_fp8(make, B):
    ds, rec = make(B)
    ds.attach_fp8()
    assert ("layers.0.attn.output_proj.weight" in ds.w8) == (B == 2) and len(ds.w8) == (3 if B == 1 else 4) * LAYERS
    want = _run(ds, rec, [(B == 1, [_fp8] * 4)] * LAYERS)
    assert [op for op, _ in want[:len(want) // LAYERS]] == (["gemv_fp8w", "gemv_attn", "gemv_fp8w", "gemv_fp8w"] if B == 1 else
                                                            ["gemv_fp8w", "attn_decode_rope"] + ["gemv_fp8w"] * 3)


def _live(G, bias=None):
    def product(ds, name, x, y, **kw):
        t = ds.lt[:, :G.kx]
        norm = {k: v for k, v in kw.items() if k in ("norm_scale", "eps")}
        return [("lora_project", dict(x=x, At=G.At, t=t, scale=2.0, **norm)),
                ("gemv_kext", dict(x=x, W=ds.stack.ws[name], y=y, ext_t=t, ext_B=G.Bx, **({} if bias is None else {"bias": bias}), **kw))]
    return product


def test_live_lora_keeps_the_fused_attention(make):
    ds, rec = make(1)
    Gq, G2 = _group(16, bias_on="k_proj"), _mlp_group("mlp_out", 8)
    ds.attach_lora(_state({(0, "attn_in"): Gq, (0, "mlp_out"): G2}))
    assert ds.lora_scale == 2.0 and ds.lt.shape == (1, 16) and ds.lora_rows is None and ds.lora[1] == {}
    bias = ds.lora[0]["attn_in"][2]                            # in the fused projection's row order: q | k | v
    assert bias.tolist() == [0.0] * HD + [2.0] * HD + [0.0] * HD and ds.lora[0]["mlp_out"][2] is None
    want = _run(ds, rec, [(True, [_live(Gq, bias), _plain, _plain, _live(G2)]), (True, [_plain] * 4)])
    assert [op for op, _ in want] == ["lora_project", "gemv_kext", "gemv_attn", "gemv_ex", "lora_project", "gemv_kext",
                                      "gemv_ex", "gemv_attn", "gemv_ex", "gemv"]


def test_live_lora_attn_out_runs_unfused(make):
    ds, rec = make(1)
    Go = _mlp_group("attn_out", 8)
    ds.attach_lora(_state({(1, "attn_out"): Go}))
    want = _run(ds, rec, [(True, [_plain] * 4), (False, [_plain, _live(Go), _plain, _plain])])
    assert [op for op, _ in want[4:]] == ["gemv_ex", "attn_decode_rope", "lora_project", "gemv_kext", "gemv_ex", "gemv"]
    assert want[7][1]["residual"] is ds.xa                     # the extended output projection adds the layer's input


def test_per_row_adapters(make):
    ds, rec = make(3)
    A = [dict(q=_group(16, seed=0), m=_mlp_group("mlp_in", 8)), dict(q=_group(16, bias_on="v_proj", seed=1), m=_mlp_group("mlp_in", 8))]
    states = [_state({(0, "attn_in"): a["q"], (0, "mlp_in"): a["m"]}, scaling=1.0 + j) for j, a in enumerate(A)]
    ds.attach_lora_rows([states[1], None, states[0]])          # compacted in order of first use: states[1] is adapter 0
    ra, scale = ds.lora_rows
    assert ra.tolist() == [0, -1, 1] and ra.dtype == torch.int32 and scale.tolist() == [2.0, 1.0] and ds.lt.shape == (3, 16)
    order = [A[1], A[0]]
    assert [k for k in ds.lora_keep if k is states[0].arena or k is states[1].arena]

    def rows(key, bias_tab=None):
        Gs = [a[key] for a in order]
        kx = Gs[0].kx

        def product(ds, name, x, y, **kw):
            At_tab, Bx_tab, btab = ds.lora[0][{"q": "attn_in", "m": "mlp_in"}[key]][:3]
            assert At_tab.tolist() == [G.At.data_ptr() for G in Gs] and Bx_tab.tolist() == [G.Bx.data_ptr() for G in Gs]
            assert At_tab.dtype == Bx_tab.dtype == torch.int64 and (btab is None) == (key == "m")
            norm = {k: v for k, v in kw.items() if k in ("norm_scale", "eps")}
            return [("lora_project_rows", dict(x=x, At_tab=At_tab, t=ds.lt, row_adapter=ra, scale=scale, kx=kx, lda=kx, **norm)),
                    ("gemv_kext_rows", dict(x=x, W=ds.stack.ws[name], y=y, ext_t=ds.lt, Bx_tab=Bx_tab, row_adapter=ra, kx=kx, ldb=kx,
                                            **({} if btab is None else {"bias_tab": btab}), **kw))]
        return product

    want = _run(ds, rec, [(False, [rows("q"), _plain, rows("m"), _plain]), (False, [_plain] * 4)])
    assert [op for op, _ in want[:7]] == ["lora_project_rows", "gemv_kext_rows", "attn_decode_rope", "gemv", "lora_project_rows",
                                          "gemv_kext_rows", "gemv"]
    # the bias table: adapter 0 (states[1]) has a bias on v_proj, in the fused projection's row order; adapter 1 has none: 0
    btab = ds.lora[0]["attn_in"][2].tolist()
    bias = next(k for k in ds.lora_keep if k.data_ptr() == btab[0])
    assert btab[1] == 0 and bias.tolist() == [0.0] * (2 * HD) + [4.0] * HD


def test_attach_errors_keep_their_texts(make):
    ds, _ = make(1)
    with pytest.raises(ValueError, match=r"generate with LoRA adapters: 520 extension columns in decoder\.layers\.0\.attn_in#0 \(the "
                                         r"decode kernels take at most 512: rank x adapters per fused projection\)"):
        ds.attach_lora(_state({(0, "attn_in"): _group(520)}))
    assert ds.lora is None and ds.lt is None
    ds, _ = make(2)
    with pytest.raises(ValueError, match=r"generate with LoRA adapters: 520 extension columns in .* at most 512"):
        ds.attach_lora_rows([_state({(0, "attn_in"): _group(520)}), None])
    with pytest.raises(ValueError, match=r"per-row LoRA adapters: decoder layer 0 attn_in: the adapters do not share one layout"):
        ds.attach_lora_rows([_state({(0, "attn_in"): _group(16)}), _state({(0, "attn_in"): _group(8)})])
    with pytest.raises(ValueError, match="do not share one layout"):
        ds.attach_lora_rows([_state({(0, "attn_in"): _group(16)}), _state({})])
    assert ds.lora is None and ds.lora_rows is None
