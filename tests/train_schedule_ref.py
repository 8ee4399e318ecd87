"""The launch schedule of the train step (``_Stack.forward`` / ``_Stack.backward``, csm/engine.py) as a symbolic trace, without a
GPU: ``csm.engine.ops`` is replaced by a recorder, the model and the LoRA state by stand-ins over CPU tensors that nothing
computes on, and one forward (+ backward) becomes the ordered list of its events - every ``ops.*`` call, every call of a LoRA
group's / adapter's ``project`` / ``forward`` / ``backward``, and the two layer hooks.

An event is one string, ``name(positional, ...; keyword=value, ...)``.  Operands are named, never addressed:

  a weight / gradient block       its name (``decoder.layers.0.mlp.w13``; ``g:`` in front = the gradient block)
  any other tensor                the index of the event that first showed it (``in`` / ``din`` / ... for what the caller hands in);
                                  where it first shows, ``=dtype[shape]`` follows.  An event's second, third new tensor: ``7b``,
                                  ``7c``; what a LoRA call makes and returns: ``7r``
  a view                          ``base@offset[shape]/[stride]`` relative to that tensor's storage (elements)
  numbers, booleans, None         by value; tuples and lists element by element
  a keyword that was not passed   absent (bench.py wraps some ops with timers that know the positional arguments only, so
                                  whether ``pin`` is passed at all is part of the schedule)

Every tensor an event shows is kept alive until the trace is complete, so an address that the allocator hands out twice is
never taken for one tensor.

``MODES`` lists the recorded runs (shapes are the smallest that reach each branch); ``tests/golden/train_schedule.json`` holds
their traces as ``engine.py`` issued them before ``_Stack`` was reorganised, and tests/test_train_schedule_cpu.py compares.
To record again (from the ``tests`` directory):  python -m train_schedule_ref [path/to/train_schedule.json]
"""
import json
import os
import sys
import types
from collections import OrderedDict
from contextlib import contextmanager

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_schedule.json")
BF, F32 = torch.bfloat16, torch.float32
DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.int32: "i32", torch.int64: "i64"}
NORM_BWD_BLOCKS = 4                                     # what the stand-in of csm_rmsnorm_bwd_blocks() answers
H, KV, HD, F = 2, 1, 64, 64                             # heads and MLP width: no branch of the schedule looks at them
GROUPS = OrderedDict([("attn_in", ("q_proj", "k_proj", "v_proj")), ("attn_out", ("output_proj",)),
                      ("mlp_in", ("w1", "w3")), ("mlp_out", ("w2",))])       # training/lora.py GROUPS
ALL7 = tuple(mod for mods in GROUPS.values() for mod in mods)
R_PAD, SCALING = 8, 2.0


class Trace:
    """The events so far and the names of the tensors they showed."""

    def __init__(self):
        self.events, self.keep, self.label, self.fresh = [], [], {}, 0

    def name(self, t, label):
        """``t`` (its whole storage) goes by ``label`` from here on."""
        self.keep.append(t)
        self.label[t.untyped_storage().data_ptr()] = label
        return t

    def _tensor(self, t):
        key = t.untyped_storage().data_ptr()
        new = key not in self.label
        if new:                                         # the event's first new tensor is "n", the next ones "nb", "nc", ...
            self.name(t, str(len(self.events)) + ("" if not self.fresh else chr(ord("a") + self.fresh)))
            self.fresh += 1
        s = self.label[key]
        whole = t.storage_offset() == 0 and t.is_contiguous() and t.numel() * t.element_size() == t.untyped_storage().nbytes()
        if not whole:
            s += f"@{t.storage_offset()}{list(t.shape)}/{list(t.stride())}".replace(" ", "")
        if new:
            s += f"={DT[t.dtype]}{list(t.shape)}".replace(" ", "")
        return s

    def operand(self, v):
        if isinstance(v, torch.Tensor):
            return self._tensor(v)
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(self.operand(x) for x in v) + ")"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v) if not isinstance(v, str) else v
        raise TypeError(f"an operand the trace has no name for: {type(v)}")

    def event(self, what, a, kw, made=()):
        """Append ``what(a; kw)``; ``made``: tensors the call itself creates and returns - they first show in this event."""
        n, self.fresh = len(self.events), 0
        parts = [self.operand(x) for x in a]
        if kw:
            parts.append(";" + ",".join(f"{k}={self.operand(v)}" for k, v in kw.items()))
        for t in made:
            self.name(t, f"{n}r")
        self.events.append(f"{what}({','.join(parts)})".replace(",;", ";"))


class Recorder:
    """Stands in for ``csm.hip.ops``: every attribute is an op that logs itself; nothing of libcsm_hip.so is called.
    ``grouped``: what ``two_linear_dw`` / ``multi_linear_dw`` answer (False = "this shape has no grouped kernel")."""

    def __init__(self, trace, grouped=True):
        self._t, self._grouped = trace, grouped
        self.lib = types.SimpleNamespace(csm_rmsnorm_bwd_blocks=lambda: NORM_BWD_BLOCKS)

    @staticmethod
    def _pin(pin):                                       # (ops._pin: a helper, not a launch)
        return {"pin": True} if pin else {}

    def __getattr__(self, op):
        def call(*a, **kw):
            self._t.event(op, a, kw)
            return self._grouped if op in ("two_linear_dw", "multi_linear_dw") else None
        return call


class Adapter:
    """LoRAAdapter stand-in (training/lora.py): ``project`` / ``forward`` return t [M, r], ``backward`` nothing."""

    def __init__(self, trace, name, bias, dropout):
        self._t, self.name, self.r, self.scaling, self.dropout = trace, name, R_PAD, SCALING, dropout
        self.bias = trace.name(torch.empty(1, dtype=BF), name + ".bias") if bias else None

    def project(self, *a, **kw):
        t = a[1] if len(a) > 1 else kw.get("t")
        made = [torch.empty(a[0].shape[0], self.r, dtype=BF)] if t is None else []
        self._t.event(self.name + ".project", a, kw, made)
        return made[0] if made else t

    def forward(self, *a, **kw):
        t = torch.empty(a[0].shape[0], self.r, dtype=BF)
        self._t.event(self.name + ".forward", a, kw, [t])
        return t

    def backward(self, *a, **kw):
        self._t.event(self.name + ".backward", a, kw)


class Group:
    """LoRAGroup stand-in: ``project`` returns tx [M, KX], ``backward`` dts [M, KX]."""

    def __init__(self, trace, state, name, mods, bias, dropout):
        self._t, self.state, self.name = trace, state, name
        self.kx = (len(mods) * R_PAD + 31) // 32 * 32
        self.At, self.Bx = trace.name(torch.empty(1, self.kx, dtype=BF), name + ".At"), trace.name(torch.empty(1, self.kx, dtype=BF), name + ".Bx")
        self.adapters = OrderedDict((mod, Adapter(trace, f"{name}.{mod}", bias, dropout)) for mod in mods)

    def fusable(self):
        return all(ad.bias is None and not (ad.dropout > 0 and self.state.training) for ad in self.adapters.values())

    def project(self, *a, **kw):
        tx = torch.empty(a[0].shape[0], self.kx, dtype=BF)
        self._t.event(self.name + ".project", a, kw, [tx])
        return tx

    def backward(self, *a, **kw):
        dts = torch.empty(a[1].shape[0], self.kx, dtype=BF)
        self._t.event(self.name + ".backward", a, kw, [dts])
        return dts


class State:
    """LoRAState stand-in: adapters on ``modules`` of ``layers`` (None = all) of the stack ``prefix``."""

    def __init__(self, trace, prefix, n_layers, modules, layers=None, bias=False, dropout=0.0, training=False, n_adapters=1):
        self.n_adapters, self.training, self.merged = n_adapters, training, False
        self.groups, self.adapters = {}, {}
        for i in range(n_layers) if layers is None else layers:
            for gname, mods in GROUPS.items():
                present = [mod for mod in mods if mod in modules]
                if present:
                    G = self.groups[(prefix, i, gname)] = Group(trace, self, f"L{i}.{gname}", present, bias, dropout)
                    for mod, ad in G.adapters.items():
                        self.adapters[(prefix, i, mod)] = ad

    def get(self, prefix, layer, module):
        return self.adapters.get((prefix, layer, module))

    def group(self, prefix, layer, gname):
        return self.groups.get((prefix, layer, gname))


class Model:
    """What ``_Stack`` uses of the model: ``block(name, grad)`` (one tensor per name, shaped like the real block), the RoPE table,
    the two stacks' configurations and ``lora``."""

    def __init__(self, trace, prefix, d, n_layers):
        c = types.SimpleNamespace(num_layers=n_layers, num_heads=H, num_kv_heads=KV, head_dim=HD, intermediate_dim=F, embed_dim=d,
                                  qkv_dim=(H + 2 * KV) * HD, norm_eps=1e-5)
        self._t, self.bb, self.dc, self.lora, self._blocks = trace, c, c, None, {}
        self._shapes = {"attn.qkv": (c.qkv_dim, d), "attn.output_proj.weight": (d, H * HD), "mlp.w13": (2 * F, d), "mlp.w2.weight": (d, F)}
        self._rope = trace.name(torch.empty(64, HD // 2, dtype=F32), "rope")

    def rope_table(self, prefix):
        return self._rope

    def block(self, name, grad=False):
        key = ("g:" if grad else "") + name
        if key not in self._blocks:
            shape = next((s for k, s in self._shapes.items() if name.endswith(k)), (self.bb.embed_dim,))
            self._blocks[key] = self._t.name(torch.empty(*shape, dtype=BF), key)
        return self._blocks[key]


# ---- the recorded runs ----------------------------------------------------------------------------------------------------------------
# name -> settings: d / M / layers of the stack (B x S = M), ``train`` = train_base (None: forward only), ``lora`` = State keywords,
# ``defer`` = (DEFER_ATTN_DW, DEFER_NORM_DW), ``grouped`` = the answer of the grouped weight-gradient launches, and the forward forms
WIDE = dict(d=2048, B=2, S=2048, layers=5, train=True)
NARROW = dict(d=1024, B=2, S=2048, layers=3, train=True)
TINY = dict(d=1024, B=2, S=64, layers=2, train=True)
MODES = OrderedDict([
    ("wide", dict(WIDE)),
    ("wide_overwrite", dict(WIDE, acc=False)),
    ("wide_defer_attn_1", dict(WIDE, defer=(1, True))),
    ("wide_norms_undeferred", dict(WIDE, defer=(3, False))),
    ("wide_frozen", dict(WIDE, train=False)),
    ("narrow", dict(NARROW)),
    ("narrow_ungrouped_kernels", dict(NARROW, grouped=False)),
    ("wide_ungrouped_kernels", dict(WIDE, grouped=False)),
    ("tiny", dict(TINY)),
    ("tiny_wide", dict(TINY, d=2048)),
    ("lora_qv", dict(TINY, train=False, lora=dict(modules=("q_proj", "v_proj")))),
    ("lora_all7", dict(TINY, train=False, lora=dict(modules=ALL7))),
    ("lora_q_train_base", dict(WIDE, layers=2, lora=dict(modules=("q_proj",)))),
    ("lora_q_one_layer_train_base", dict(WIDE, layers=4, lora=dict(modules=("q_proj",), layers=(1,)))),
    ("lora_all7_train_base", dict(TINY, lora=dict(modules=ALL7))),
    ("lora_all7_unfused", dict(TINY, train=False, lora=dict(modules=ALL7), lora_fuse=False)),
    ("lora_bias", dict(TINY, train=False, lora=dict(modules=ALL7, bias=True))),
    ("lora_bias_train_base", dict(TINY, lora=dict(modules=ALL7, bias=True))),
    ("lora_dropout", dict(TINY, train=False, lora=dict(modules=ALL7, dropout=0.1, training=True))),
    ("lora_w1_dropout", dict(TINY, train=False, lora=dict(modules=("w1", "output_proj"), dropout=0.1, training=True))),
    ("lora_stack", dict(TINY, train=False, lora=dict(modules=("q_proj", "v_proj", "w1", "w2"), n_adapters=2), sel=True)),
    ("fwd_pos_unfused_rope", dict(TINY, train=None, pos=True, fuse_rope=False)),
    ("fwd_lora_pos", dict(TINY, train=None, pos=True, lora=dict(modules=("q_proj", "v_proj")))),
    ("packed", dict(TINY, seg=[[40, 24], [10, 30]])),
    ("packed_lora", dict(TINY, train=False, seg=[[40, 24], [10, 30]], lora=dict(modules=ALL7))),
    ("append", dict(TINY, B=1, S=5, train=None, append="one")),
    ("append_lora", dict(TINY, B=1, S=5, train=None, append="one", lora=dict(modules=ALL7))),
    ("append_ragged", dict(TINY, B=1, S=9, train=None, append="rows")),
    ("append_ragged_lora", dict(TINY, B=1, S=9, train=None, append="rows", lora=dict(modules=ALL7))),
    ("append_ragged_lora_bias", dict(TINY, B=1, S=9, train=None, append="rows", lora=dict(modules=ALL7, bias=True))),
])


@contextmanager
def _engine(ops, defer, lora_fuse):
    """csm.engine with ``ops`` in place of the kernel library's front end and the schedule's settings at the given values."""
    import csm.engine as E
    was = E.ops, E.DEFER_ATTN_DW, E.DEFER_NORM_DW, E.LORA_FUSE
    E.ops, (E.DEFER_ATTN_DW, E.DEFER_NORM_DW), E.LORA_FUSE = ops, defer, lora_fuse
    try:
        yield E
    finally:
        E.ops, E.DEFER_ATTN_DW, E.DEFER_NORM_DW, E.LORA_FUSE = was


def trace(mode):
    """The events of one ``forward(save=True)`` + ``backward`` of ``MODES[mode]`` (a forward alone where ``train`` is None)."""
    cfg = dict(dict(acc=True, defer=(3, True), grouped=True, lora=None, lora_fuse=True, sel=False, pos=False, fuse_rope=True,
                    seg=None, append=None), **MODES[mode])
    t = Trace()
    prefix = "backbone" if cfg["d"] >= 2048 else "decoder"
    B, S, d, L = cfg["B"], cfg["S"], cfg["d"], cfg["layers"]
    M = B * S
    model = Model(t, prefix, d, L)
    if cfg["lora"] is not None:
        model.lora = State(t, prefix, L, **cfg["lora"])
    hooks = {}
    for hook in ("on_layer_start", "on_layer_done"):
        hooks[hook] = lambda p, i, hook=hook: t.event(hook, (p, i), {})
    with _engine(Recorder(t, cfg["grouped"]), cfg["defer"], cfg["lora_fuse"]) as E:
        st = E._Stack(model, prefix)
        kw = {}
        if cfg["sel"]:
            kw["sel"] = t.name(torch.empty(M, dtype=torch.int32), "sel")
        fkw = dict(kw)
        if cfg["pos"] or cfg["append"]:
            fkw["pos"] = t.name(torch.empty(M, dtype=torch.int32), "pos")
        if not cfg["fuse_rope"]:
            fkw["fuse_rope"] = False
        if cfg["seg"] is not None:
            kw["seg"] = fkw["seg"] = E.Segments(cfg["seg"], B, S, torch.device("cpu"))
            t.name(kw["seg"].pos._base, "seg")
        if cfg["append"]:
            ds = types.SimpleNamespace(k=[t.name(torch.empty(1, dtype=BF), f"k{i}") for i in range(L)],
                                       v=[t.name(torch.empty(1, dtype=BF), f"v{i}") for i in range(L)])
            fkw["append"] = (ds, 1, 7) if cfg["append"] == "one" else (ds, [2, 0, 1], [7, 0, 3], [4, 2, 3])
        x = t.name(torch.empty(M, d, dtype=BF), "in")
        save = cfg["train"] is not None
        xf = st.forward(x, B, S, save, on_layer_start=hooks["on_layer_start"], **fkw)
        t.events.append(f"return({t.operand(xf)})")
        if save:
            dxf = t.name(torch.empty(M, d, dtype=BF), "din")
            dx = st.backward(dxf, B, S, cfg["train"], 1.0, on_layer_done=hooks["on_layer_done"], acc=cfg["acc"], **kw)
            t.events.append(f"return({t.operand(dx)})")
            assert st.acts == []
    return t.events


def record(path=GOLDEN):
    """Write every mode's trace to ``path``: run against the engine whose schedule is to be the golden one."""
    with open(path, "w") as f:
        json.dump(OrderedDict((mode, trace(mode)) for mode in MODES), f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "csm-train-pytorch_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    record(*sys.argv[1:2])
