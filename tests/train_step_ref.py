"""A float64 reference of the WHOLE train step (``Engine.forward_loss`` + ``Engine.backward``: the wiring of the kernels, not the
kernels - those have pins of their own), an emulation of the step's bf16 stores, a per-row judge and a catalogue of seeded wiring
faults.  test_train_step_ref_cpu.py proves this module (against the oracle, against itself, and that every fault is caught);
test_train_step_grads_gpu.py judges the engine by it.

Plain torch on the CPU.  ``_loss`` restates ``compute_loss`` (embedding sum -> backbone -> codebook-0 CE; frame rows -> decoder
input -> projection -> depth decoder -> per-codebook CE) in its own text, in whatever dtype the weights have (float64 everywhere
but the oracle comparison, which runs it in fp32): no ``.float()`` upcast anywhere.  Weights are the bf16 values widened.

Three evaluations of a ``Case``:
  grads64(case)               exact arithmetic, float64, autograd.
  grads_emulated(case, seed)  the same graph with a rounding hook wherever the engine STORES a bf16 tensor.  seed None: round to
                              nearest even.  An integer: stochastic rounding (one of the two neighbouring bf16 values, chosen with
                              probability by distance) - independent draws of noise of the same scale.
  judge(got, g64, g_emu)      per tensor, per row over the last dimension (a 1-D tensor is one row):
                                dead row  g64 and g_emu both exactly zero (untouched embedding rows, frozen groups, a group whose
                                          loss term is off): got must be exactly zero.
                                live row  any other: ratio = |got - g64|_2 / max(|g_emu - g64|_2, 2^-10 |g64|_2); the floor is the
                                          row's own bf16 storage rounding.
                              Every row is one or the other (asserted).  Prints ``RATIO <case> <tensor> <worst>``.

Hooks (``_hook``: an autograd.Function that rounds its value in forward and/or the incoming gradient in backward), with the line
of csm/engine.py (E) or csm/training/lora.py (L) whose store each mirrors.  fp32 tensors (logits E536-538 / E664-667, rows_loss) are
never rounded in value; their gradients are where the engine stores them in bf16.
  value and gradient
    h0            E530-532 embed_fwd           / dh0: the gradient the last norm_bwd returns, E352
    xn, hn        E230-232, E257-259           / dxn E350-351, dhn E334-335
    v             E233-238 (no rotation)       / dqkv E341-349
    q, k fused    value AFTER the rotation, once (RoPE in the GEMM epilogue, E235 / E236, E165); gradient BEFORE it, once (RoPE
                  backward in the dQ / dK epilogue, E345-346).  The pre-rotation value and the post-rotation gradient are never
                  stored: no hook there.
    q, k packed   (segment-local positions, E238, E343-344): value before AND after the rotation, gradient after AND
                  before - the stand-alone RoPE kernel reads and writes bf16 both ways.
    o             E239-245                     / do E339-340
    h, out (x)    the residual sums, one rounding of x + product: E255-256, E280-281 / dh E337, dx E352 (one rounding of
                  norm path + residual path, the fused norm_bwd)
    xf, hidden    E286-288                     / dhid after rows_add_bf16 E748-749 (a bf16 read-modify-write: the hook on
                  hidden rounds the SUM of the two branches, each already rounded below)
    seq           E657-658 (copies of bf16 values: the value rounding changes nothing) / dseq E731-732
    x0            E659-660                     / dx0: the gradient decoder.backward returns, E729
  gradient only
    logits        dlog E740-742, dl E717-719 (ce_fwd_bwd writes bf16 gradients of fp32 logits)
    hidden -> head      dhid as linear_dx stores it, E743-744, before the rows_add
    hidden -> decoder   position 0 of dseq, E731-732
    LoRA t = x A^T      dts = s dy Bx, L194-201 (the stored tensor is s dt; s is a power of two in every case here)
  value only
    LoRA tx = s x A^T   L177-188
    act (SwiGLU)        E260-278.  The forward epilogue computes it from the fp32 gate / up (gemm_common.h epi_store), the backward
                        epilogue reads the STORED bf16 gate | up and never stores d(act) (E324 / E327): ``_SwiGLU`` does exactly
                        that and rounds d(gate), d(up) = dgu once.
  inside attention (registers, not stores - the attention pins document them, train_attn_ref.py): P before the PV product, and in
  the backward P before dV and dS before dQ / dK; delta from the stored o.  ``_Attn``.
  final stores    every weight gradient is rounded once where it is written: linear_dw in ``_WgradQueue`` (E360-444) and E734 / E746, audio_head E725-727,
                  colsum_bf16 E408 / E439, embed_bwd_sorted E802 (text and audio rows, the backbone and decoder sources summed in
                  fp32 first), skinny_wgrad L51-70.  A "live" buffer is accumulated INTO: the second micro-batch stores
                  round(stored + fp32 sum) - the second rounding.  An "overwrite" (stale buffer, acc=False) rounds the same sum.

Record (measured on this module alone, 2026-10-20; ``measure`` recomputes it and test_train_step_ref_cpu.py holds it to these):
  W = worst ratio over every case of CASES, eight stochastic draws, every tensor and row, each draw judged against grads64 with
      the nearest-even draw as g_emu.  L = 2 W: the factor is for what the emulation leaves out - summation orders, fp32
      accumulation, approximated exp / rsqrt (each far below 2^-9; there are no atomics).  L is never raised to fit the GPU.
  The loss limit is |loss - loss64| <= L max over the eight draws |loss_draw - loss64|, per loss term.
  See W_RECORDED / L below, and RECORD at the end of this docstring for the GPU ratios and the fault table.

RECORD
%(record)s
"""
import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

from oracle import csm_oracle as O

F64 = torch.float64
TINY = O.tiny_cfg()
IGN = -100
PARAM_SEED = 11
GROUPS = ("backbone", "decoder", "embeddings", "other")
SEEDS = tuple(range(8))

W_RECORDED = 15.04        # measured 15.033 on 2026-10-20 (its worst case: lora_mlp_r4), written rounded up
L = 2 * W_RECORDED        # 30.08


def group_of(name: str) -> str:
    if name.startswith("backbone."):
        return "backbone"
    if name.startswith("decoder."):
        return "decoder"
    return "embeddings" if "embeddings" in name else "other"


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Lora:
    modules: Tuple[str, ...]
    r: int = 8
    alpha: float = 16.0
    decoder: bool = True                   # the engine attaches adapters to both stacks; False = backbone only (reference side)
    n_adapters: int = 1
    ids: Optional[tuple] = None            # a stack: the set of every example [B], or of every segment [R][n] (-1 = base model)
    seed: int = 1


@dataclass(frozen=True)
class Case:
    name: str
    B: int = 2
    S: int = 24
    seed: int = 5
    sw: float = 100.0
    aw: float = 1.0
    rows_stride: Optional[int] = None      # acoustic rows arange(0, B*(S-1), stride); None = every frame ("all")
    ignore: Optional[tuple] = None         # ((example, first ignored frame), ...): ragged labelled lengths, IGN beyond
    segments: Optional[tuple] = None       # a packed batch: the segment lengths of every row (B, S then describe the rows)
    frozen: Tuple[str, ...] = ()
    lora: Optional[Lora] = None
    micro: Tuple[Tuple[int, float], ...] = ()   # accumulation: (data seed, loss scale) per micro-batch; () = ((seed, 1.0),)
    prev: Optional["Case"] = None          # the step a lazy optimiser step consumed before this backward

    @property
    def ign(self):
        return IGN if (self.ignore is not None or self.segments is not None) else None

    def micros(self):
        return self.micro or ((self.seed, 1.0),)


_QV = Lora(("q_proj", "v_proj"))
_STACK = Lora(("q_proj", "v_proj", "w2"), n_adapters=3, ids=(0, 2, -1, 1))
_SEGS = ((50, 40, 33), (77,))
_LAZY0 = Case("lazy_first", seed=21)
_LAZY1 = Case("lazy_1_0", seed=22, sw=1.0, aw=0.0, prev=_LAZY0)
CASES: Dict[str, Case] = {c.name: c for c in (
    Case("full_100_1"),
    Case("full_0_1", sw=0.0, aw=1.0),
    Case("full_1_0", sw=1.0, aw=0.0),
    Case("rows_b3_s100", B=3, S=100, seed=7, rows_stride=3),
    Case("ignore_ragged", B=3, seed=11, ignore=((0, 15), (2, 7))),
    Case("packed", B=2, S=128, seed=40, segments=_SEGS),
    Case("lora_qv_100_1", seed=6, lora=_QV),
    Case("lora_qv_0_1", seed=6, sw=0.0, aw=1.0, lora=_QV),
    Case("lora_mlp_r4", seed=16, lora=Lora(("w1", "w2", "w3"), r=4, alpha=8.0, seed=11)),
    Case("lora_stack", B=4, seed=6, lora=_STACK),
    Case("lora_stack_packed", B=2, S=128, seed=40, segments=_SEGS, lora=replace(_STACK, ids=((0, -1, 2), (1,)))),
    Case("accumulate", micro=((5, 0.5), (6, 0.5))),
    _LAZY1,
    Case("lazy_100_1", seed=23, prev=_LAZY1),
    Case("frozen_backbone_embeddings", frozen=("backbone", "embeddings")),
    Case("frozen_decoder_other", frozen=("decoder", "other")),
)}


def params64(seed: int = PARAM_SEED, dtype=F64) -> Dict[str, torch.Tensor]:
    """The tiny model's weights as the GPU holds them: bf16 values, widened."""
    return {k: v.to(torch.bfloat16).to(dtype) for k, v in O.init_params(TINY, seed=seed).items()}


def make_lora(case: Case, dtype=F64) -> Optional[List[Dict[str, torch.Tensor]]]:
    """One {name.lora_A [r, in], name.lora_B [out, r]} per adapter set, bf16 values widened; B is non-zero so that every
    gradient path is live.  The GPU test copies these very values into the model's adapters."""
    sp = case.lora
    if sp is None:
        return None
    shapes = O.param_shapes(TINY)
    sets = []
    for a in range(sp.n_adapters):
        g = torch.Generator().manual_seed(1000 * sp.seed + a)
        lo = {}
        for prefix, c in (("backbone", TINY.backbone), ("decoder", TINY.decoder)):
            if prefix == "decoder" and not sp.decoder:
                continue
            for i in range(c.n_layers):
                for mod in sp.modules:
                    name = f"{prefix}.layers.{i}.{'attn' if mod.endswith('proj') else 'mlp'}.{mod}"
                    out_f, in_f = shapes[f"{name}.weight"]
                    lo[f"{name}.lora_A"] = (torch.randn(sp.r, in_f, generator=g) / math.sqrt(in_f)).to(torch.bfloat16).to(dtype)
                    lo[f"{name}.lora_B"] = (torch.randn(out_f, sp.r, generator=g) * 0.05).to(torch.bfloat16).to(dtype)
        sets.append(lo)
    return sets


def batch(case: Case, seed: int) -> dict:
    """The micro-batch of ``case`` drawn with ``seed``: tokens [B, S, K+1], mask, targets [B, S, K] (IGN where unlabelled), rows
    (over the B*(S-1) row space of compute_loss, or None), segment_lengths [B, n_max] or None, adapter_ids or None - and for a
    packed batch ``padded``: the same examples one per row, padded to the longest, as the oracle takes them."""
    K = TINY.n_codebooks
    out = dict(rows=None, segment_lengths=None, adapter_ids=None, padded=None)
    if case.segments is None:
        tokens, mask, targets = O.synthetic_batch(TINY, case.B, case.S, seed=seed)
        targets = targets.clone()
        for b, first in (case.ignore or ()):
            targets[b, first:] = IGN
        if case.rows_stride:
            out["rows"] = torch.arange(0, case.B * (case.S - 1), case.rows_stride)
    else:
        R, S = len(case.segments), case.S
        assert R == case.B and all(sum(r) <= S for r in case.segments)
        tokens = torch.zeros(R, S, K + 1, dtype=torch.int64)
        mask = torch.zeros(R, S, K + 1, dtype=torch.bool)
        targets = torch.full((R, S, K), IGN, dtype=torch.int64)
        ex, n = [], 0
        for r, lens in enumerate(case.segments):
            o = 0
            for ln in lens:
                tk, mk, tg = O.synthetic_batch(TINY, 1, ln, seed=100 * seed + n)
                tokens[r, o:o + ln], mask[r, o:o + ln], targets[r, o:o + ln - 1] = tk[0], mk[0], tg[0, :ln - 1]
                ex.append((tk[0], mk[0], tg[0, :ln - 1]))
                o, n = o + ln, n + 1
        nmax = max(len(r) for r in case.segments)
        out["segment_lengths"] = torch.tensor([list(r) + [0] * (nmax - len(r)) for r in case.segments])
        Sp = max(t.shape[0] for t, _, _ in ex)
        ptk = torch.zeros(len(ex), Sp, K + 1, dtype=torch.int64)
        pmk = torch.zeros(len(ex), Sp, K + 1, dtype=torch.bool)
        ptg = torch.full((len(ex), Sp, K), IGN, dtype=torch.int64)
        for e, (tk, mk, tg) in enumerate(ex):
            ptk[e, :tk.shape[0]], pmk[e, :tk.shape[0]], ptg[e, :tg.shape[0]] = tk, mk, tg
        out["padded"] = (ptk, pmk, ptg)
    if case.lora is not None and case.lora.ids is not None:
        ids = case.lora.ids
        if case.segments is not None:
            nmax = max(len(r) for r in ids)
            ids = [list(r) + [-1] * (nmax - len(r)) for r in ids]
        out["adapter_ids"] = torch.tensor(ids)
    out.update(tokens=tokens, mask=mask, targets=targets)
    return out


# ------------------------------------------------------------------------------------------------------------ rounding
class Rounder:
    """bf16 rounding of a float64 tensor: off, to nearest even (seed None), or stochastic (an integer seed)."""

    def __init__(self, on: bool, seed: Optional[int] = None):
        self.on = on
        self.gen = torch.Generator().manual_seed(int(seed)) if (on and seed is not None) else None

    def __call__(self, x):
        if not self.on:
            return x
        if self.gen is None:
            return x.to(torch.bfloat16).to(x.dtype)
        _, e = torch.frexp(x)                                       # |x| in [2^(e-1), 2^e): 8 significant bits -> ulp 2^(e-8)
        ulp = torch.ldexp(torch.ones_like(x), e - 8)
        q = x / ulp
        lo = torch.floor(q)
        up = torch.rand(x.shape, generator=self.gen, dtype=F64) < (q - lo)
        return (lo + up.to(x.dtype)) * ulp


class _Hook(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, R, fwd, bwd):
        ctx.R, ctx.bwd = R, bwd
        return R(x) if fwd else x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (ctx.R(g) if ctx.bwd else g), None, None, None


def _hook(x, R, fwd=True, bwd=True):
    return _Hook.apply(x, R, fwd, bwd) if R.on else x


class _SwiGLU(torch.autograd.Function):
    """act from the unrounded gate / up; the backward reads the stored (rounded) gate | up, d(act) is not stored, dgu is."""

    @staticmethod
    def forward(ctx, g, u, R):
        ctx.R = R
        ctx.save_for_backward(R(g), R(u))
        return R(g * torch.sigmoid(g) * u)

    @staticmethod
    def backward(ctx, dact):
        gt, up = ctx.saved_tensors
        sg = torch.sigmoid(gt)
        return ctx.R(dact * up * sg * (1 + gt * (1 - sg))), ctx.R(dact * gt * sg), None


class _Attn(torch.autograd.Function):
    """q, k, v [B, H, S, hd] (k / v already repeated over the group), vis [B, 1, S, S].  The kernels' scheme: P rounded before the
    PV product, the sum of the row from the unrounded P; backward from the stored out and lse, P rounded before dV, dS before
    dQ / dK."""

    @staticmethod
    def forward(ctx, q, k, v, vis, R):
        scale = 1.0 / math.sqrt(q.shape[-1])
        s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf"))
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        out = R((R(e) @ v) / l)
        ctx.R, ctx.scale = R, scale
        ctx.save_for_backward(q, k, v, out, m + torch.log(l), vis)
        return out

    @staticmethod
    def backward(ctx, dO):
        q, k, v, out, lse, vis = ctx.saved_tensors
        R, scale = ctx.R, ctx.scale
        p = torch.exp((q @ k.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf")) - lse)
        dS = R(p * (dO @ v.transpose(-1, -2) - (dO * out).sum(-1, keepdim=True)))
        return scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), R(p).transpose(-1, -2) @ dO, None, None


class _TakeRowsShifted(torch.autograd.Function):
    """FAULT: takes rows ``rows`` and scatters their gradient to ``rows + 1``."""

    @staticmethod
    def forward(ctx, x, rows):
        ctx.rows, ctx.n = rows, x.shape[0]
        return x[rows]

    @staticmethod
    def backward(ctx, g):
        out = g.new_zeros(ctx.n, g.shape[1])
        out.index_add_(0, (ctx.rows + 1).clamp(max=ctx.n - 1), g)
        return out, None


# ------------------------------------------------------------------------------------------------------------ the graph
_tables: Dict[tuple, torch.Tensor] = {}


def _table(c, dtype):
    key = (c.max_seq_len, c.head_dim, c.rope_base, c.rope_scale, dtype)
    if key not in _tables:
        _tables[key] = O.rope_table(c.max_seq_len, c.head_dim, c.rope_base, c.rope_scale).to(dtype)   # fp32 values: data
    return _tables[key]


def _rope(x, table, pos):
    """x [B, S, H, hd], interleaved pairs (2i, 2i+1) rotated by the angle of position pos [B, S]."""
    xs = x.reshape(*x.shape[:-1], -1, 2)
    t = table[pos].unsqueeze(2)
    c, s = t[..., 0], t[..., 1]
    return torch.stack([xs[..., 0] * c - xs[..., 1] * s, xs[..., 1] * c + xs[..., 0] * s], dim=-1).flatten(-2)


def _rms(x, scale, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * scale


def _stack(P, prefix, c, x, B, S, pos, vis, R, lora, sel, fused_rope):
    """One Llama stack on rows x [B*S, d] -> the final norm's output.  ``lora`` = (sets, scaling) or None; ``sel`` [B*S] the set
    of every row of a stack of sets (None: one set for every row)."""
    H, KV, hd, M = c.n_heads, c.n_kv_heads, c.head_dim, B * S
    table = _table(c, x.dtype)

    def lin(name, inp):
        y = inp @ P[f"{name}.weight"].t()
        if lora is not None:
            for a, lo in enumerate(lora[0]):
                if f"{name}.lora_A" in lo:
                    t = _hook(inp @ lo[f"{name}.lora_A"].t(), R, fwd=False)          # gradient: dts = s dy B
                    tx = _hook(lora[1] * t, R, bwd=False)                            # value: tx = s x A^T
                    if sel is not None:
                        tx = tx * (sel == a).to(tx.dtype)[:, None]
                    y = y + tx @ lo[f"{name}.lora_B"].t()
        return y

    def rotated(y, heads):
        if fused_rope:
            return _hook(_rope(_hook(y, R, fwd=False).view(B, S, heads, hd), table, pos), R, bwd=False)
        return _hook(_rope(_hook(y, R).view(B, S, heads, hd), table, pos), R)

    for i in range(c.n_layers):
        p = f"{prefix}.layers.{i}"
        xn = _hook(_rms(x, P[f"{p}.sa_norm.scale"], c.norm_eps), R)
        q = rotated(lin(f"{p}.attn.q_proj", xn), H).transpose(1, 2)
        k = rotated(lin(f"{p}.attn.k_proj", xn), KV).transpose(1, 2).repeat_interleave(H // KV, dim=1)
        v = _hook(lin(f"{p}.attn.v_proj", xn), R).view(B, S, KV, hd).transpose(1, 2).repeat_interleave(H // KV, dim=1)
        if R.on:
            o = _Attn.apply(q, k, v, vis, R)
        else:
            s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~vis, float("-inf"))
            o = torch.softmax(s, dim=-1) @ v
        o = _hook(o.transpose(1, 2).reshape(M, H * hd), R)
        h = _hook(x + lin(f"{p}.attn.output_proj", o), R)
        hn = _hook(_rms(h, P[f"{p}.mlp_norm.scale"], c.norm_eps), R)
        g, u = lin(f"{p}.mlp.w1", hn), lin(f"{p}.mlp.w3", hn)
        act = _SwiGLU.apply(g, u, R) if R.on else g * torch.sigmoid(g) * u
        x = _hook(h + lin(f"{p}.mlp.w2", act), R)
    return _hook(_rms(x, P[f"{prefix}.norm.scale"], c.norm_eps), R)


def _ce_rows(logits, tgt):
    return torch.logsumexp(logits, dim=-1) - logits.gather(1, tgt[:, None])[:, 0]


def _positions(bt, B, S):
    """(segment id [B, S], position inside the segment [B, S]); what a row's segments leave over is one more segment."""
    if bt["segment_lengths"] is None:
        return torch.zeros(B, S, dtype=torch.int64), torch.arange(S).repeat(B, 1)
    Lh = bt["segment_lengths"]
    full = torch.cat([Lh, (S - Lh.sum(1))[:, None]], 1)
    n = full.shape[1]
    seg = torch.stack([torch.repeat_interleave(torch.arange(n), full[b]) for b in range(B)])
    start = torch.stack([torch.repeat_interleave(full[b].cumsum(0) - full[b], full[b]) for b in range(B)])
    return seg, torch.arange(S)[None, :] - start


def _loss(P, case: Case, bt: dict, R: Rounder, lora=None, fault: Optional[str] = None):
    """-> (total, semantic, acoustic) of one micro-batch, differentiable w.r.t. P and the adapter tensors."""
    cfg, B, S = TINY, case.B, case.S
    K, V, M = cfg.n_codebooks, cfg.audio_vocab, B * S
    tokens, mask, targets = bt["tokens"], bt["mask"], bt["targets"]
    dt = P["projection.weight"].dtype
    # ---- the rows' adapter sets
    sel = None
    if lora is not None and case.lora.n_adapters > 1:
        ids = bt["adapter_ids"]
        if case.segments is None:
            sel = ids.repeat_interleave(S)
        else:
            Lh = bt["segment_lengths"]
            sel = torch.repeat_interleave(torch.cat([ids, torch.full((B, 1), -1)], 1).reshape(-1),
                                          torch.cat([Lh, (S - Lh.sum(1))[:, None]], 1).reshape(-1))
        if fault == "adapter_minus_one_is_zero":
            sel = sel.clamp(min=0)
    # ---- backbone
    text = P["text_embeddings.weight"][tokens[:, :, K]]
    audio = P["audio_embeddings.weight"][tokens[:, :, :K] + V * torch.arange(K)]
    e = torch.cat([audio, text.unsqueeze(2)], dim=2) * mask.unsqueeze(-1).to(dt)
    h0 = _hook(e.sum(2).reshape(M, -1), R)
    seg, pos = _positions(bt, B, S)
    vis = (torch.tril(torch.ones(S, S, dtype=torch.bool))[None] & (seg[:, :, None] == seg[:, None, :]))[:, None]
    hidden = _stack(P, "backbone", cfg.backbone, h0, B, S, pos, vis, R, lora, sel, fused_rope=case.segments is None)
    # ---- semantic term: position p < S-1 of every row against targets[p, 0]
    t0 = torch.full((B, S), -1, dtype=torch.int64)
    t0[:, :S - 1] = targets[:, :S - 1, 0]
    t0 = t0.reshape(M)
    lab = (t0 >= 0).nonzero()[:, 0]
    n_sem = B * (S - 1) if (case.ign is None or fault == "n_sem_counts_ignored") else max(1, lab.numel())
    logits = _hook(_hook(hidden, R, fwd=False)[lab] @ P["codebook0_head.weight"].t(), R, fwd=False)
    sem = _ce_rows(logits, t0[lab]).sum() / n_sem
    # ---- acoustic term: the frames' rows through the depth decoder
    if bt["rows"] is not None:
        rows = (bt["rows"] // (S - 1)) * S + bt["rows"] % (S - 1)
    else:
        rows = (torch.arange(B)[:, None] * S + torch.arange(S - 1)[None, :]).reshape(-1)
    if case.ign is not None:
        rows = rows[t0[rows] >= 0]
    N = rows.numel()
    codes = targets.reshape(M, K)[rows]
    if fault == "no_acoustic_into_backbone":
        first = hidden.detach()[rows]
    elif fault == "pos0_scattered_to_next_row":
        first = _TakeRowsShifted.apply(hidden, rows)
    else:
        first = hidden[rows]
    emb = P["audio_embeddings.weight"][codes[:, :K - 1] + V * torch.arange(K - 1)]                  # [N, K-1, d]
    if fault == "decoder_embedding_all":
        emb = emb.detach()
    elif fault == "decoder_embedding_last":
        emb = torch.cat([emb[:, :K - 2], emb[:, K - 2:].detach()], dim=1)
    seq = torch.cat([_hook(first, R, fwd=False).unsqueeze(1), _hook(emb, R, fwd=False)], dim=1).reshape(N * K, -1)
    x0 = _hook(seq @ P["projection.weight"].t(), R)
    dsel = sel[rows].repeat_interleave(K) if sel is not None else None
    dlora = lora if (lora is not None and case.lora.decoder) else None
    dvis = torch.tril(torch.ones(K, K, dtype=torch.bool))[None, None]
    xf = _stack(P, "decoder", cfg.decoder, x0, N, K, torch.arange(K).repeat(N, 1), dvis, R, dlora, dsel, fused_rope=True)
    dlogits = _hook(torch.einsum("nkd,kdv->nkv", xf.view(N, K, -1)[:, 1:], P["audio_head"]), R, fwd=False)
    ac = _ce_rows(dlogits.reshape(-1, V), codes[:, 1:].reshape(-1)).sum() / (N * (K if fault == "acoustic_mean_over_k" else K - 1))
    # the decoder's backward does not run at weight 0 (E747): no gradient, not a zero-weighted one
    total = case.sw * sem + (case.aw * ac if case.aw != 0.0 else 0.0 * ac.detach())
    return total, sem, ac


# ------------------------------------------------------------------------------------------------------------ evaluations
@dataclass
class Result:
    losses: List[Tuple[float, float, float]]       # (total, semantic, acoustic) of every micro-batch
    grads: Dict[str, torch.Tensor]                 # every model tensor; adapters as "adapter{a}.{name}.lora_A|B"


def _evaluate(case: Case, R: Rounder, params=None, lora=None, fault=None, want_grads=True) -> Result:
    P = {k: v.clone().requires_grad_(want_grads) for k, v in (params if params is not None else params64()).items()}
    dt = P["projection.weight"].dtype
    lo = None
    if case.lora is not None:
        sets = [{k: v.to(dt).clone().requires_grad_(want_grads) for k, v in s.items()} for s in (lora if lora is not None else make_lora(case))]
        lo = (sets, case.lora.alpha / case.lora.r)
    leaves = dict(P)
    if lo is not None:
        for a, s in enumerate(lo[0]):
            leaves.update({f"adapter{a}.{k}": v for k, v in s.items()})
    frozen = set(GROUPS) if lo is not None else set(case.frozen)
    grads = {k: torch.zeros_like(v, requires_grad=False) for k, v in leaves.items()}
    losses = []
    for n, (seed, scale) in enumerate(case.micros()):
        bt = batch(case, seed)
        with torch.set_grad_enabled(want_grads):
            total, sem, ac = _loss(P, case, bt, R, lo, fault)
        losses.append(tuple(float(t.detach()) for t in (total, sem, ac)))
        if not want_grads:
            continue
        names = list(leaves)
        gs = torch.autograd.grad(total * scale, [leaves[k] for k in names], allow_unused=True)
        for k, g in zip(names, gs):
            if g is None or (not k.startswith("adapter") and group_of(k) in frozen):
                continue
            if fault == "lora_b_without_scaling" and k.endswith("lora_B"):
                g = g / lo[1]
            if fault == "second_micro_overwrites_other" and n > 0 and not k.startswith("adapter") and group_of(k) == "other":
                grads[k] = R(g)
            else:
                grads[k] = R(grads[k] + g)              # the final store; a live buffer: round(stored + this backward's sum)
    if fault == "stale_decoder_survives" and want_grads and case.prev is not None and case.aw == 0.0:
        stale = _evaluate(case.prev, R, params, lora).grads
        grads.update({k: v for k, v in stale.items() if group_of(k) == "decoder" and not k.startswith("adapter")})
    return Result(losses, grads)


def grads64(case: Case, params=None, lora=None) -> Result:
    return _evaluate(case, Rounder(False), params, lora)


def grads_emulated(case: Case, seed: Optional[int] = None, params=None, lora=None, fault: Optional[str] = None,
                   hooks: bool = True) -> Result:
    return _evaluate(case, Rounder(hooks, seed), params, lora, fault)


def loss_noise(case: Case, params=None, lora=None, seeds=SEEDS):
    """max over the stochastic draws of |loss_draw - loss64| per micro-batch and loss term (forward only), and loss64."""
    ref = _evaluate(case, Rounder(False), params, lora, want_grads=False).losses
    dev = [[0.0, 0.0, 0.0] for _ in ref]
    for s in seeds:
        got = _evaluate(case, Rounder(True, s), params, lora, want_grads=False).losses
        for d, g, r in zip(dev, got, ref):
            for j in range(3):
                d[j] = max(d[j], abs(g[j] - r[j]))
    return ref, dev


# ------------------------------------------------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    ratios: Dict[str, float]                       # worst live-row ratio of every tensor (0.0: no live row)
    dead_nonzero: List[Tuple[str, int]]            # (tensor, row) of every dead row that is not exactly zero
    n_live: int
    n_dead: int

    @property
    def worst(self) -> float:
        """The worst ratio of the step: a dead row that is not exactly zero has no finite ratio."""
        return float("inf") if self.dead_nonzero else max(self.ratios.values())


def judge(got: Dict[str, torch.Tensor], g64: Dict[str, torch.Tensor], g_emu: Dict[str, torch.Tensor], case: str = "",
          quiet: bool = False) -> Verdict:
    assert set(got) == set(g64) == set(g_emu), sorted(set(g64) ^ set(got))
    ratios, bad, n_live, n_dead = {}, [], 0, 0
    for k in g64:
        last = g64[k].shape[-1]
        a, b, c = (t[k].detach().to("cpu", F64).reshape(-1, last) for t in (got, g64, g_emu))
        assert a.shape == b.shape == c.shape, k
        dead = (b == 0).all(1) & (c == 0).all(1)
        live = ~dead
        assert int(dead.sum()) + int(live.sum()) == b.shape[0] and not bool((dead & live).any()), k
        n_live, n_dead = n_live + int(live.sum()), n_dead + int(dead.sum())
        bad += [(k, int(r)) for r in (dead & ~(a == 0).all(1)).nonzero()[:, 0]]
        worst = 0.0
        if bool(live.any()):
            num = (a - b)[live].norm(dim=1)
            den = torch.maximum((c - b)[live].norm(dim=1), 2.0 ** -10 * b[live].norm(dim=1))
            ratio = torch.nan_to_num(num / den, nan=float("inf"))
            worst = float(ratio.max())
        ratios[k] = worst
        if not quiet:
            print(f"RATIO {case} {k} {worst:.3f}")
    return Verdict(ratios, bad, n_live, n_dead)


def old_criterion(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> float:
    """What the model-level tests assert (gclose): the worst max|err| / max|ref| over the tensors with a non-zero reference."""
    worst = 0.0
    for k, r in ref.items():
        scale = float(r.abs().max())
        if scale > 0:
            worst = max(worst, float((got[k].double().cpu() - r).abs().max()) / scale)
    return worst


def measure(cases=None, seeds=SEEDS, quiet=True):
    """-> (W, {case: its worst ratio}): every stochastic draw judged against grads64 with the nearest-even draw as g_emu."""
    per = {}
    for c in (cases if cases is not None else CASES.values()):
        g64, rne = grads64(c).grads, grads_emulated(c).grads
        per[c.name] = max(judge(grads_emulated(c, seed=s).grads, g64, rne, c.name, quiet=True).worst for s in seeds)
        if not quiet:
            print(f"W {c.name} {per[c.name]:.3f}")
    return max(per.values()), per


# ------------------------------------------------------------------------------------------------------------ faults
# name -> (what is wired wrongly, the cases of CASES it can show in)
FAULTS: Dict[str, Tuple[str, Tuple[str, ...]]] = {
    "no_acoustic_into_backbone": ("the acoustic loss sends no gradient into the backbone state (rows_add_bf16 of position 0 dropped)",
                                  ("full_0_1", "full_100_1")),
    "decoder_embedding_last": ("decoder-input embedding gradient missing for the last codebook", ("full_100_1",)),
    "decoder_embedding_all": ("decoder-input embedding gradient missing for every codebook (dseq never reaches the embedding backward)",
                              ("full_100_1",)),
    "pos0_scattered_to_next_row": ("position-0 gradients scattered to rows + 1", ("full_0_1", "full_100_1")),
    "n_sem_counts_ignored": ("n_sem counts the ignored rows", ("ignore_ragged", "packed")),
    "acoustic_mean_over_k": ("the acoustic mean divides by N K instead of N (K - 1)", ("full_100_1", "full_0_1")),
    "lora_b_without_scaling": ("a LoRA B gradient without alpha / r", ("lora_qv_100_1", "lora_mlp_r4")),
    "second_micro_overwrites_other": ("the second micro-batch overwrites the 'other' group instead of adding", ("accumulate",)),
    "stale_decoder_survives": ("a stale decoder buffer survives a step in which the decoder does not run", ("lazy_1_0",)),
    "adapter_minus_one_is_zero": ("an example with adapter id -1 receives adapter 0's gradient", ("lora_stack", "lora_stack_packed")),
}
OLD_CRITERION_BLIND = ("no_acoustic_into_backbone", "decoder_embedding_last", "decoder_embedding_all")   # at weights 100 / 1

RECORD = """  W = 15.033, recorded as 15.04; L = 30.08; 2 L = 60.16.  Per case: the worst ratio of the eight draws (reference alone), then the
  worst ratio of the engine on an MI355X (2026-10-20; every dead row exactly zero, every loss inside its limit):
    full_100_1 5.94 / 3.49      full_0_1 7.06 / 3.69        full_1_0 7.17 / 3.07          rows_b3_s100 4.02 / 2.45
    ignore_ragged 5.36 / 2.64   packed 4.10 / 1.95          lora_qv_100_1 8.14 / 3.77     lora_qv_0_1 14.33 / 8.15
    lora_mlp_r4 15.03 / 9.49    lora_stack 11.76 / 6.04     lora_stack_packed 13.22 / 4.68   accumulate 3.96 / 2.39
    lazy_1_0 5.37 / 3.34        lazy_100_1 6.07 / 2.51      frozen_backbone_embeddings 3.78 / 2.07   frozen_decoder_other 5.94 / 3.49
  (The largest ratios sit on rows of four or eight numbers - a lora_B row is r long - where one norm is a poor estimate of the noise.)
  No case failed and the engine was not changed.
  Fault table: worst ratio of the faulty emulation (caught at >= 2 L) and the model-level criterion max|err| / max|ref| (its limit is
  3e-2 .. 6e-2) on the same gradients.
    fault                           case                ratio     max|err| / max|ref|
    no_acoustic_into_backbone       full_0_1            296.5     1.0000
                                    full_100_1          3.6       0.0130   passes both: at 100 / 1 the path is below the noise
    decoder_embedding_last          full_100_1          170.0     0.0130   the old criterion passes it
    decoder_embedding_all           full_100_1          170.0     0.0130   the old criterion passes it
    pos0_scattered_to_next_row      full_0_1            306.1     1.4772
                                    full_100_1          3.2       0.0130   passes both, as above: (0, 1) is the case that sees it
    n_sem_counts_ignored            ignore_ragged       122.4     0.3527
                                    packed              68.5      0.2325
    acoustic_mean_over_k            full_100_1          83.6      0.2540
    lora_b_without_scaling          lora_qv_100_1       403.6     0.5024
                                    lora_mlp_r4         350.9     0.5025
    second_micro_overwrites_other   accumulate          270.6     0.9368
    stale_decoder_survives          lazy_1_0            inf       0.0110   4101 dead rows not zero; the old criterion skips zero references
    adapter_minus_one_is_zero       lora_stack          1622.1    1.6077
                                    lora_stack_packed   1086.5    2.9436
  The same two faults planted in the real engine (rows_add_bf16 skipped; dseq withheld from _embedding_backward) give the same
  figures on the MI355X: 296.5 at (0, 1) and 170.0, with max|err| / max|ref| 0.0123 at (100, 1)."""
__doc__ = __doc__.replace("%(record)s", RECORD)
