"""Explicit forward / backward schedule of the CSM train step over libcsm_hip.so.

There is no autograd tape underneath: the layer structure is fixed, so the engine walks it forwards saving the
activations the backward needs, then backwards issuing dgrad / wgrad GEMMs and the fused element-wise backward
kernels, accumulating straight into the bf16 gradient arena (wgrad GEMM epilogue ``C += alpha * dY^T X``).
It restates what autograd does for the reference hot loop ``compute_loss -> loss.backward()``
(reference src/csm/training/utils.py:56-119, src/csm/training/trainer.py:245-263).

Activations kept per layer (bf16 unless noted): x (block input), xn, qkv (post-RoPE), attn out, lse (fp32),
h (post-attention residual), hn, gate|up, swiglu out, rstd x2 (fp32)  ~= 76 KB per position per backbone layer.
With 288 GB of HBM nothing is recomputed.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, Optional

import torch

from .hip import ops
from .sampling import (RowSampler, _is_number, check_filters, check_processors, check_row_processors, check_typical,  # noqa: F401
                       check_sampling, names_processors)

BF16 = torch.bfloat16
F32 = torch.float32
import os as _os
# the attention projections' weight gradients of this many layers go out in one launch (1 = per layer); one layer's are 160
# tiles of 256 x 256 - 0.63 of a round of the 256 CUs - three layers' 480: 1.9 rounds
DEFER_ATTN_DW = int(_os.environ.get("CSM_DEFER_ATTN_DW", "3"))
# the RMSNorm scale gradients' column sums of a layer (and of the layers whose attention gradients are deferred) in one launch
DEFER_NORM_DW = _os.environ.get("CSM_DEFER_NORM_DW", "1") == "1"
# the depth decoder's fused attention + output projection takes its position as a launch argument (A/B: 0 = from device memory)
DECODE_POS_HOST = _os.environ.get("CSM_DECODE_POS_HOST", "1") == "1"
# LoRA groups ride on the frozen projections' GEMMs as K-extension operands (training/lora.py); 0 = per-adapter products
LORA_FUSE = _os.environ.get("CSM_LORA_FUSE", "1") != "0"


def _refuse_stack(lo, where: str):
    """A stack of adapter sets (LoRAState n_adapters > 1) exists for training batches that name a set per example; every
    single-adapter path takes one exported set."""
    if getattr(lo, "n_adapters", 1) > 1:
        raise ValueError(f"{where} takes one adapter set, and model.lora stacks {lo.n_adapters}: export one first "
                         "(state = model.lora.export(a), then LoRABank.add / generate_batch(adapters=[...]) / row_lora(model, state))")


def adapter_rows(adapter_ids, B: int, S: int, n_adapters: int, segment_lengths=None) -> torch.Tensor:
    """``sel`` [B*S] int32 on the host: the adapter set of every position, from ``adapter_ids`` [B] (one id per example) or,
    with ``segment_lengths`` [B, n_max], [B, n_max] (one id per segment; what a row's segments leave over is padding).
    -1 = base model only; padding is always -1.  Ids outside [-1, n_adapters) are refused here, on the host - the kernels only
    compare them."""
    ids = torch.as_tensor(adapter_ids).detach().to("cpu")
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError(f"adapter_ids must be integers, got {ids.dtype}")
    ids = ids.to(torch.int64)
    if segment_lengths is None:
        if tuple(ids.shape) != (B,):
            raise ValueError(f"adapter_ids must have shape [B={B}] (one adapter set per example), got {tuple(ids.shape)}")
        live = ids
        sel = ids.repeat_interleave(S)
    else:
        L = torch.as_tensor(segment_lengths).detach().to("cpu").to(torch.int64)
        if ids.dim() != 2 or tuple(ids.shape) != tuple(L.shape) or L.shape[0] != B:
            raise ValueError(f"adapter_ids of a packed batch must have the shape of segment_lengths {tuple(L.shape)} "
                             f"(one adapter set per segment), got {tuple(ids.shape)}")
        if bool((L < 0).any()) or bool((L.sum(1) > S).any()):
            raise ValueError("segment_lengths: negative, or more than a row holds")
        live = ids[L > 0]
        full_len = torch.cat([L, (S - L.sum(1))[:, None]], 1).reshape(-1)
        full_ids = torch.cat([ids, torch.full((B, 1), -1, dtype=torch.int64)], 1).reshape(-1)
        sel = torch.repeat_interleave(full_ids, full_len)
    if live.numel() and (int(live.min()) < -1 or int(live.max()) >= n_adapters):
        bad = live[(live < -1) | (live >= n_adapters)]
        raise ValueError(f"adapter id {int(bad[0])} out of range: {n_adapters} adapter set(s), valid ids are -1 (base model) "
                         f"and 0..{n_adapters - 1}")
    return sel.to(torch.int32)


@contextmanager
def generation_lora(model):
    """What generation does with the adapters of ``model`` around a pass through the training forward (prefill, recompute):
    yields the LoRAState to apply, or None.  Adapters are read, never trained: dropout is off (``lora.training`` False, the
    previous value restored afterwards, also on an error; no mask is drawn, ``lora.draws`` does not move) and the transposed
    copies the fused forward reads (``refresh``) are renewed, as the adapters may have moved since the last loss.  Adapters that
    ``merge_lora_weights`` folded into the base weights stay attached but are not applied a second time."""
    lo = model.lora
    if lo is None:
        yield None
        return
    _refuse_stack(lo, "generation")
    if lo.merged:
        model.lora = None
        try:
            yield None
        finally:
            model.lora = lo
        return
    was = lo.training
    lo.training = False
    try:
        if LORA_FUSE:
            lo.refresh()
        yield lo
    finally:
        lo.training = was


@contextmanager
def row_lora(model, state):
    """``generation_lora`` with ``state`` (a bank entry, csm/lora_bank.py; None = no adapter) standing in for ``model.lora`` for
    the duration: a prefill row of a per-row-adapter batch runs the training forward exactly as a one-utterance generation with
    that adapter live as ``model.lora`` would.  ``model.lora`` is restored afterwards, also on an error."""
    prev = model.lora
    model.lora = state
    try:
        with generation_lora(model) as lo:
            yield lo
    finally:
        model.lora = prev


class _Stack:
    """One Llama stack (backbone or decoder) bound to a model's arenas."""

    def __init__(self, model, prefix: str):
        self.m, self.prefix = model, prefix
        self.c = c = model.bb if prefix == "backbone" else model.dc
        self.acts: List[Dict[str, torch.Tensor]] = []
        hq, hk = c.num_heads * c.head_dim, c.num_kv_heads * c.head_dim
        # The four Linear projections of a layer: (weight, LoRA group (training/lora.py GROUPS), the saved activation that is its
        # input, {member module: its columns of the output}).  w13 keeps gate / up interleaved: g0, u0, g1, u1, ...
        self.proj = {"qkv": ("attn.qkv", "attn_in", "xn", {"q_proj": slice(0, hq), "k_proj": slice(hq, hq + hk),
                                                            "v_proj": slice(hq + hk, hq + 2 * hk)}),
                     "o": ("attn.output_proj.weight", "attn_out", "o", {"output_proj": slice(None)}),
                     "w13": ("mlp.w13", "mlp_in", "hn", {"w1": slice(0, None, 2), "w3": slice(1, None, 2)}),
                     "w2": ("mlp.w2.weight", "mlp_out", "act", {"w2": slice(None)})}

    def w(self, name, grad=False):
        return self.m.block(f"{self.prefix}.{name}", grad)

    def _pw(self, layer: int, p: str, grad=False):
        """The weight (or weight gradient) of projection ``p`` of ``layer``."""
        return self.w(f"layers.{layer}.{self.proj[p][0]}", grad)

    def _lora(self, layer: int, module: str):
        lo = self.m.lora
        return lo.get(self.prefix, layer, module) if lo is not None else None

    def _group(self, layer: int, gname: str, a=None):
        """(group, fused?) - the LoRA adapters of ``layer`` on one fused projection (lora.py GROUPS); fused = the whole
        group enters that projection's GEMMs as one K-extension operand pair.  ``a`` (the backward: the layer's saved
        activations): fused only if the forward went that way and left its extension operand."""
        lo = self.m.lora
        G = lo.group(self.prefix, layer, gname) if lo is not None else None
        return G, (G is not None and LORA_FUSE and G.fusable() and (a is None or f"tx_{gname}" in a))

    def _project(self, i, a, p, x, y, pin, sel, residual=None, **epilogue) -> bool:
        """y = x W^T (+ residual) + the adapters' part, for projection ``p`` of layer ``i``; what the backward needs of the adapters
        goes to ``a``.  A fusable group: its up-projections are extra k-steps of the same product, so ``epilogue`` (``rope=`` /
        ``swiglu_act=``, ops.gemm_kext) sees the sum, and the answer is True.  Otherwise the adapters add to their columns of y one
        by one, ``epilogue`` is NOT applied and the answer is False: the caller runs the stand-alone kernel."""
        _, gname, _, members = self.proj[p]
        G, fused = self._group(i, gname)
        if fused:
            a[f"tx_{gname}"] = G.project(x, pin=pin, sel=sel)
            ops.gemm_kext(x, self._pw(i, p), y, a[f"tx_{gname}"], G.Bx, **({} if residual is None else {"R": residual}), **epilogue, pin=pin)
            return True
        ops.linear_fwd(x, self._pw(i, p), y, **({} if residual is None else {"residual": residual}), pin=pin)
        for mod, cols in members.items():
            ad = self._lora(i, mod)
            if ad is None:
                continue
            if y[:, cols].stride(1) == 1:
                a[f"t_{mod}"] = ad.forward(x, y[:, cols], pin=pin)
            else:                                   # interleaved columns: the adapter's products want unit stride
                tmp = torch.zeros(y[:, cols].shape, dtype=BF16, device=y.device)
                a[f"t_{mod}"] = ad.forward(x, tmp, pin=pin)
                y[:, cols] += tmp
        return False

    def _input_grad(self, i, a, p, dy, dx, sel, q=None, **epilogue):
        """dx = dy W + the adapters' part (and the adapters' own gradients), for projection ``p`` of layer ``i``; fused, ``epilogue``
        (``swiglu_bwd_gu=``) sees the sum.  ``q``: the projection's weight gradient is due right behind the input-gradient product.
        (The two stay two launches: paired in one launch with interleaved tiles, ops.linear_dx_dw, every pairing measured SLOWER
        on the B=4, S=2048 step - 73.7 ms/step -> 75.7 with w2 alone, 77.4 w13, 77.1 output_proj, 78.3 qkv, 83.2 all four:
        de-phasing the CUs' epilogues does not pay for two operand sets competing for each XCD's 4 MiB L2.)"""
        _, gname, xin, members = self.proj[p]
        G, fused = self._group(i, gname, a)
        if fused:
            dts = G.backward(a[xin], dy, a[f"tx_{gname}"], sel=sel)
            ops.gemm_kext(dy, self._pw(i, p), dx, dts, G.At, transB=True, **epilogue)
        else:
            assert not epilogue
            ops.linear_dx(dy, self._pw(i, p), dx)
        if q is not None:
            q.ready(p, i, dy, a[xin], fused)
        if not fused:
            for mod, cols in members.items():
                ad = self._lora(i, mod)
                if ad is not None:
                    dym = dy[:, cols]
                    ad.backward(a[xin], dym if dym.stride(1) == 1 else dym.contiguous(), a[f"t_{mod}"], dx)

    # -------------------------------------------------------------------------------------------- forward
    def forward(self, x: torch.Tensor, B: int, S: int, save: bool, pos: Optional[torch.Tensor] = None,
                fuse_rope: bool = True, on_layer_start=None, append=None, seg=None, sel=None) -> torch.Tensor:
        """``seg`` = a ``Segments`` (packed rows): attention goes through the segment-masked kernels (``ops.attn_fwd_seg``) and RoPE
        through the un-fused path with the segment-local positions ``seg.pos``; everything else is unchanged.
        ``append`` = (decode stack, batch row, pos0): the S rows are positions pos0 .. pos0+S-1 of the sequence whose earlier
        positions sit in that stack's KV caches (B = 1, ``pos`` given, nothing saved) - every layer's attention appends its K / V
        rows to the caches and attends to them (``ops.attn_append``) instead of the from-scratch ``ops.attn_fwd``.
        The ragged form ``append`` = (decode stack, rows, pos0s, ns) with three equally long lists of host integers stacks R <= 16
        such segments, each against its own batch row: x holds ``sum(ns)`` rows, segment after segment, and ``pos`` their positions
        (``ops.attn_append_rows``).  Its products are pinned to the kernel whose rows do not see each other (``pin``, ops.gemm), so a
        segment's rows have the bits they would have in a forward of their own, whatever is stacked beside them.
        ``sel`` (int32 [M] on the device): the adapter set of every row when ``model.lora`` is a stack (training/lora.py)."""
        c, dev = self.c, x.device
        M, d = x.shape
        if seg is not None:
            assert pos is None and append is None
            pos = seg.pos
        pin = append is not None and isinstance(append[1], (list, tuple))
        H, KV, hd, F = c.num_heads, c.num_kv_heads, c.head_dim, c.intermediate_dim
        table = self.m.rope_table(self.prefix)
        rope_in_gemm = fuse_rope and pos is None     # positions = arange(S): RoPE can ride in the q|k|v projection's epilogue
        self.acts = []
        for i in range(c.num_layers):
            if on_layer_start is not None:
                on_layer_start(self.prefix, i)       # ZeRO-1: this layer's parameters have arrived (training/dp.py wait_params)
            a: Dict[str, torch.Tensor] = {}
            xn = torch.empty(M, d, dtype=BF16, device=dev)
            rstd1 = torch.empty(M, dtype=F32, device=dev)
            ops.rmsnorm_fwd(x, self.w(f"layers.{i}.sa_norm.scale"), xn, rstd1, c.norm_eps)
            qkv = torch.empty(M, c.qkv_dim, dtype=BF16, device=dev)
            if rope_in_gemm and self._group(i, "attn_in")[0] is None:
                ops.linear_rope_fwd(xn, self._pw(i, "qkv"), qkv, table, S, (H + KV) * hd, hd)
            elif not (self._project(i, a, "qkv", xn, qkv, pin, sel, rope=(table, S, (H + KV) * hd, hd) if rope_in_gemm else None)
                      and rope_in_gemm):
                ops.rope(qkv, table, S, H + KV, hd, pos=pos)
            o = torch.empty(M, H * hd, dtype=BF16, device=dev)
            if append is None:
                lse = torch.empty(B, H, S, dtype=F32, device=dev)
                if seg is not None:
                    ops.attn_fwd_seg(qkv, o, lse, seg.seg_start, B, S, H, KV, hd)
                else:
                    ops.attn_fwd(qkv, o, lse, B, S, H, KV, hd)
            else:
                assert B == 1 and pos is not None and not save
                lse = None
                if pin:
                    ds, rows, pos0s, ns = append
                    ops.attn_append_rows(qkv, ds.k[i], ds.v[i], o, rows, pos0s, ns, H, KV, hd)
                else:
                    ds, row, pos0 = append
                    ops.attn_append(qkv, ds.k[i], ds.v[i], o, row, pos0, H, KV, hd)
            h = torch.empty(M, d, dtype=BF16, device=dev)
            self._project(i, a, "o", o, h, pin, sel, residual=x)
            hn = torch.empty(M, d, dtype=BF16, device=dev)
            rstd2 = torch.empty(M, dtype=F32, device=dev)
            ops.rmsnorm_fwd(h, self.w(f"layers.{i}.mlp_norm.scale"), hn, rstd2, c.norm_eps)
            gu = torch.empty(M, 2 * F, dtype=BF16, device=dev)     # gate/up interleaved: g0,u0,g1,u1,...
            act = torch.empty(M, F, dtype=BF16, device=dev)
            G, fused = self._group(i, "mlp_in")
            if G is None:
                # SwiGLU in the GEMM epilogue (csm_gemm_bf16_ex).  A/B on one MI355X box, B=4 S=2048: 88.0 ms/step fused vs 88.9 ms
                # with the stand-alone kernel (the 256x256 GEMM runs one workgroup per CU, so most of the epilogue work is exposed;
                # the gain is what remains after that)
                ops.linear_swiglu_fwd(hn, self._pw(i, "w13"), gu, act, **ops._pin(pin))
            elif not fused and all(ad.bias is None for ad in G.adapters.values()):
                # (dropout: one mask per adapter) the adapters' (alpha/r) t B^T is written FIRST, for both at once -
                # t13 = the adapters' projections side by side, as the group's Bx expects them - and the frozen product takes it
                # in through the residual port of its SwiGLU epilogue: gate/up = acc + R, act from the sum
                first = next(iter(G.adapters.values()))
                t13 = torch.zeros(M, G.kx, dtype=BF16, device=dev)
                for j, (mod, ad) in enumerate(G.adapters.items()):
                    a[f"t_{mod}"] = ad.project(hn, t13[:, j * first.r:(j + 1) * first.r], pin=pin)
                ops.gemm(t13, G.Bx, gu, None, alpha=first.scaling, **ops._pin(pin))
                ops.linear_swiglu_fwd(hn, self._pw(i, "w13"), gu, act, residual=gu, **ops._pin(pin))
            elif not self._project(i, a, "w13", hn, gu, pin, sel, swiglu_act=act):
                ops.swiglu_fwd(gu, act)              # adapters with a bias: gate / up are complete only after the last of them
            out = torch.empty(M, d, dtype=BF16, device=dev)
            self._project(i, a, "w2", act, out, pin, sel, residual=h)
            if save:
                a.update(x=x, xn=xn, rstd1=rstd1, qkv=qkv, o=o, lse=lse, h=h, hn=hn, rstd2=rstd2, gu=gu, act=act)
                self.acts.append(a)
            x = out
        xf = torch.empty(M, d, dtype=BF16, device=dev)
        rstdf = torch.empty(M, dtype=F32, device=dev)
        ops.rmsnorm_fwd(x, self.w("norm.scale"), xf, rstdf, c.norm_eps)
        if save:
            self.final = dict(x=x, rstd=rstdf)
        return xf

    # -------------------------------------------------------------------------------------------- backward
    def backward(self, dxf: torch.Tensor, B: int, S: int, train_base: bool, alpha: float,
                 pos: Optional[torch.Tensor] = None, on_layer_done=None, acc: bool = True, seg=None, sel=None) -> torch.Tensor:
        """dxf = gradient w.r.t. the final-norm output.  Returns the gradient w.r.t. the stack input.
        Weight gradients are added to the gradient arena (``acc``) or overwrite what it holds (``acc=False``: the first
        backward after a lazy optimizer step, which left consumed gradients behind instead of zeros); the incoming
        gradient is already scaled, so ``alpha`` stays 1 unless a caller rescales."""
        c, dev = self.c, dxf.device
        M, d = dxf.shape
        H, KV, hd, F = c.num_heads, c.num_kv_heads, c.head_dim, c.intermediate_dim
        table = self.m.rope_table(self.prefix)
        nb = ops.lib.csm_rmsnorm_bwd_blocks()
        parts = torch.empty(nb, d, dtype=F32, device=dev) if train_base else None
        delta = torch.empty(2, B, H, S, dtype=F32, device=dev)   # attention-backward scratch (-delta, -lse log2e)
        q = _WgradQueue(self, M, train_base, acc, alpha, on_layer_done)

        def norm_bwd(x, name, rstd, dy, dres, defer=False):
            dx = torch.empty(M, d, dtype=BF16, device=dev)
            pp = torch.empty(nb, d, dtype=F32, device=dev) if train_base and defer else parts
            ops.rmsnorm_bwd(x, self.w(name), rstd, dy, dx, dres, pp)
            if train_base:
                q.norm_ready(pp, self.w(name, grad=True), defer)
            return dx

        dx = norm_bwd(self.final["x"], "norm.scale", self.final["rstd"], dxf, None)
        for i in reversed(range(c.num_layers)):
            a = self.acts[i]
            # ---- MLP: out = h + w2(act)
            dgu = torch.empty(M, 2 * F, dtype=BF16, device=dev)
            G, fused = self._group(i, "mlp_out", a)
            if G is None:
                ops.linear_dx_swiglu_bwd(dx, self._pw(i, "w2"), a["gu"], dgu)   # d(act) never stored
            elif fused:
                # d(act) = dx w2 + (s dx Bx) At^T inside one product, SwiGLU backward in its epilogue
                self._input_grad(i, a, "w2", dx, dgu, sel, swiglu_bwd_gu=a["gu"])
            else:
                dact = torch.empty(M, F, dtype=BF16, device=dev)
                self._input_grad(i, a, "w2", dx, dact, sel)
                ops.swiglu_bwd(a["gu"], dact, dgu)
                del dact
            q.ready("w2", i, dx, a["act"])
            dhn = torch.empty(M, d, dtype=BF16, device=dev)
            self._input_grad(i, a, "w13", dgu, dhn, sel, q)
            del dgu
            dh = norm_bwd(a["h"], f"layers.{i}.mlp_norm.scale", a["rstd2"], dhn, dx, defer=DEFER_NORM_DW)   # + residual path
            # ---- attention: h = x + output_proj(o)
            do = torch.empty(M, H * hd, dtype=BF16, device=dev)
            self._input_grad(i, a, "o", dh, do, sel, q)
            dqkv = torch.empty(M, c.qkv_dim, dtype=BF16, device=dev)
            if seg is not None:                   # packed rows: segment-masked kernels, segment-local positions
                ops.attn_bwd_seg(a["qkv"], a["o"], do, a["lse"], dqkv, delta, seg.seg_start, seg.seg_end, B, S, H, KV, hd)
                ops.rope(dqkv, table, S, H + KV, hd, pos=seg.pos, inverse=True)
            elif pos is None:                     # positions = arange(S): the RoPE backward rides in the dQ / dK epilogues
                ops.attn_bwd(a["qkv"], a["o"], do, a["lse"], dqkv, delta, B, S, H, KV, hd, rope_table=table)
            else:
                ops.attn_bwd(a["qkv"], a["o"], do, a["lse"], dqkv, delta, B, S, H, KV, hd)
                ops.rope(dqkv, table, S, H + KV, hd, pos=pos, inverse=True)
            dxn = torch.empty(M, d, dtype=BF16, device=dev)
            self._input_grad(i, a, "qkv", dqkv, dxn, sel, q)
            dx = norm_bwd(a["x"], f"layers.{i}.sa_norm.scale", a["rstd1"], dxn, dh, defer=DEFER_NORM_DW)
            self.acts[i] = None
            q.layer_done(i)
        q.flush()
        self.acts = []
        return dx


class _WgradQueue:
    """The weight gradients of one ``_Stack.backward``: each goes out when it is ready (``ready`` / ``norm_ready``) or waits here
    for others to share a launch with, until ``flush``.  What waits:

    - the two attention projections' of a layer (output projection: 64 tiles of 256 x 256, fused q|k|v: 96) go out as ONE launch
      instead of split-K slabs + column sum and a 128 x 128-tile launch - and with DEFER_ATTN_DW > 1 that many layers' together;
    - a narrow stack (the depth decoder, d = 1024): every weight gradient but w13's is a fraction of a round of 256 x 256 tiles
      (o_proj 16, q|k|v 24, w2 128) and would go through fp32 split-K slabs + a column-sum launch each.  Kept to the end of the
      stack they are one launch of 160 tiles (attention, all layers) and one of 256 per two layers (w2);
    - the RMSNorm scale gradients' column sums (DEFER_NORM_DW): one launch per flush.
    The operands stay alive until their launch.  ``on_layer_done`` hears of a layer once nothing of it is left here."""

    def __init__(self, stack, M, train_base, acc, alpha, on_layer_done):
        self.stack, self.train, self.on_layer_done = stack, train_base, on_layer_done
        self.acc, self.kw = acc, dict(accumulate=acc, alpha=alpha)
        grouped = train_base and M % 64 == 0 and M >= 4096           # what the grouped weight-gradient kernels take
        self.small = grouped and DEFER_ATTN_DW > 1 and stack.c.embed_dim < 2048
        self.pair = grouped and (stack.c.embed_dim >= 2048 or self.small)
        self.held, self.deferred = None, False     # this layer's output-projection problem waiting for its q|k|v's; the pair waits
        self.attn, self.w2, self.norms = [], [], []  # (dqkv, xn, dW_qkv, dh, o, dW_o, layer) / (dy, act, dW_w2) / (partial sums, dscale)

    def ready(self, p, i, dy, x, fused=False):
        """The weight gradient dy^T x of projection ``p`` of layer ``i`` can be launched; ``fused``: its input gradient took the
        LoRA group along - an attention projection's gradient then goes out at once, whatever else holds."""
        if not self.train:
            return
        job = (dy, x, self.stack._pw(i, p, True))
        if p == "w2" and self.small:
            self.w2.append(job)
            if len(self.w2) == 2:
                self._flush_w2()
        elif p == "o" and self.pair and not fused:
            self.held = job
        elif p == "qkv" and self.held is not None:
            held, self.held = self.held, None
            if not fused and DEFER_ATTN_DW > 1:
                self.attn.append(job + held + (i,))
                self.deferred = True
            elif fused or not ops.two_linear_dw(*job, *held, **self.kw):
                ops.linear_dw(*held, **self.kw)
                ops.linear_dw(*job, **self.kw)
        else:
            ops.linear_dw(*job, **self.kw)

    def norm_ready(self, partials, dscale, defer):
        if defer:
            self.norms.append((partials, dscale))
        else:
            ops.colsum_bf16(partials, dscale, accumulate=self.acc)

    def layer_done(self, i):
        """Layer ``i`` has issued everything else.  (Layer 0 goes alone: what is launched last is what a data-parallel all-reduce
        cannot hide behind compute; a narrow stack keeps everything to its end - the wide stack's backward follows and hides its
        all-reduce.  Mixed stacks: nothing of an earlier layer may stay pending behind this layer's hook.)"""
        if self.deferred:
            self.deferred = False
            if not self.small and (len(self.attn) >= DEFER_ATTN_DW or i <= 1):
                self.flush()
        else:
            self.flush()
            if self.on_layer_done is not None:
                self.on_layer_done(self.stack.prefix, i)

    def _flush_w2(self):
        if self.w2 and not (len(self.w2) > 1 and ops.multi_linear_dw(self.w2, **self.kw)):
            for job in self.w2:
                ops.linear_dw(*job, **self.kw)
        self.w2 = []

    def flush(self):
        for c0 in range(0, len(self.attn), 6):               # at most 12 products per launch
            chunk = self.attn[c0:c0 + 6]
            if not (len(chunk) > 1 and ops.multi_linear_dw([t[k:k + 3] for t in chunk for k in (0, 3)], **self.kw)):
                for t in chunk:
                    if not ops.two_linear_dw(*t[:6], **self.kw):
                        ops.linear_dw(*t[3:6], **self.kw)
                        ops.linear_dw(*t[:3], **self.kw)
        self._flush_w2()
        if self.norms:
            ops.colsum_bf16_multi(self.norms, accumulate=self.acc)       # the layers' norms in one launch
            self.norms = []
        if self.on_layer_done is not None:
            for t in self.attn:
                self.on_layer_done(self.stack.prefix, t[6])
        self.attn = []


class Segments:
    """The descriptor of a packed batch (several examples per row, each attending only to itself), built on the host from
    ``segment_lengths`` [B, n_max] - per row the lengths of its segments in order, zero-padded - and copied to the device once:
    ``seg_start`` / ``seg_end`` [B*S] int32 = the first / last position (row-local) of the position's segment, ``pos`` = the position
    inside the segment (RoPE restarts at 0).  What a row's segments leave over is padding and becomes one more segment, so the
    arrays are total and every attention output is finite."""

    def __init__(self, segment_lengths, B: int, S: int, device):
        L = torch.as_tensor(segment_lengths).detach().to("cpu")
        if L.dim() != 2 or L.shape[0] != B or L.is_floating_point() or L.dtype == torch.bool:
            raise ValueError(f"segment_lengths must be an integer tensor [B={B}, n_max], got {tuple(L.shape)} {L.dtype}")
        L = L.to(torch.int64)
        nz = L != 0
        if bool((L < 0).any()) or bool((nz[:, 1:] & ~nz[:, :-1]).any()):
            raise ValueError("segment_lengths: every length before a row's zero padding must be at least 1")
        tot = L.sum(1)
        if bool((tot > S).any()):
            raise ValueError(f"segment_lengths: a row's segments sum to {int(tot.max())}, more than the {S} positions of a row")
        full = torch.cat([L, (S - tot)[:, None]], 1)                           # the remainder of a row: one more segment
        lens, starts = full.reshape(-1), (full.cumsum(1) - full).reshape(-1)
        first = torch.repeat_interleave(starts, lens)                          # [B*S]: zero-length entries vanish
        last = torch.repeat_interleave(starts + lens - 1, lens)
        host = torch.stack([first, last, torch.arange(S).repeat(B) - first]).to(torch.int32)
        dev_ = host.to(device, non_blocking=True)
        self.seg_start, self.seg_end, self.pos = dev_[0], dev_[1], dev_[2]


class Engine:
    def __init__(self, model):
        self.m = model
        self.backbone = _Stack(model, "backbone")
        self.decoder = _Stack(model, "decoder")
        self.saved = None
        self.grad_hook = None   # called as hook(prefix, layer) when a layer's weight gradients are final (DP overlap)
        # called as hook(prefix, layer) right before a forward first reads that bucket's parameters, hook(None, None) before
        # anything else reads parameters (ZeRO-1: the updated shards are all-gathered behind the optimiser step, dp.py)
        self.param_hook = None
        # a list here makes the cache-free generate path append the logits [B, V] every code is drawn from (parity tests)
        self.capture_logits = None
        self._consts = {}               # index tensors that depend on shapes only (built once, reused every step)

    def _need(self, group=None, layer=None):
        if self.param_hook is not None:
            self.param_hook(group, layer)

    # -------------------------------------------------------------------------------------------- loss forward
    def forward_loss(self, tokens: torch.Tensor, masks: torch.Tensor, targets: torch.Tensor, semantic_weight: float,
                     acoustic_weight: float, save: bool, acoustic_rows: Optional[torch.Tensor] = None, segment_lengths=None,
                     adapter_ids=None, rows_out: Optional[dict] = None):
        """Forward of ``compute_loss``.  Returns (total, semantic, acoustic) as 0-d fp32 GPU tensors.
        ``rows_out``: a dict that receives the per-row losses the two means are taken over (``compute_loss(return_rows=True)``).
        ``segment_lengths`` [B, n_max] (host integers, zero-padded; ``collate_packed``) marks a packed batch: every row holds several
        examples one after the other, each attends only to itself and has RoPE positions of its own (``Segments``).  The labels
        stay position-indexed, so a packed batch needs ``model.target_ignore_index``: each segment's last position and the row
        padding carry it.
        ``adapter_ids`` (host integers): with a stack of adapter sets as ``model.lora`` (``LoRAState(n_adapters > 1)``), the set
        every example runs with - [B], or [B, n_max] beside ``segment_lengths`` (one per segment); -1 = base model only.  The
        loss stays the batch loss: the mean over the labelled rows of the whole batch, whichever sets they ran with."""
        m, a = self.m, self.m.args
        dev = m.device
        B, S, K1 = tokens.shape
        K, V, Vp = a.audio_num_codebooks, a.audio_vocab_size, m.vocab_pad
        assert K1 == K + 1, f"tokens last dim must be {K + 1}"
        if targets.shape[1] < S - 1:
            raise ValueError(f"target_audio_tokens has {targets.shape[1]} frames, needs at least seq_len-1 = {S - 1}")
        if S > m.bb.max_seq_len:
            raise ValueError(f"sequence length {S} exceeds max_seq_len {m.bb.max_seq_len}")
        M, d = B * S, m.bb.embed_dim
        tk = tokens.reshape(M, K1).to(device=dev, dtype=torch.int64).contiguous()
        mk = masks.reshape(M, K1).to(device=dev, dtype=torch.uint8).contiguous()
        ign = getattr(m, "target_ignore_index", None)     # None: reference behaviour, every row counts (utils.py:102-105)
        seg = None
        if segment_lengths is not None:
            if ign is None:
                raise ValueError("a packed batch (segment_lengths) has unlabelled positions by construction: set model.target_ignore_index")
            if m.bb.head_dim != 64:
                raise ValueError(f"packed batches need a backbone head_dim of 64 (the segment-masked attention kernels), not {m.bb.head_dim}")
            seg = Segments(segment_lengths, B, S, dev)     # built and copied once per step; nothing is cached on the layout
        self._validate_batch(tokens, masks, targets, ign)
        tg = targets.to(device=dev, dtype=torch.int64)
        sel = self._adapter_sel(adapter_ids, B, S, segment_lengths)

        if m.lora is not None and LORA_FUSE:
            m.lora.refresh()
        h0 = torch.empty(M, d, dtype=BF16, device=dev)
        self._need("embeddings", -1)
        ops.embed_fwd(tk, mk, m.block("text_embeddings.weight"), m.block("audio_embeddings.weight"), h0, V)
        hidden = self.backbone.forward(h0, B, S, save, on_layer_start=self.param_hook, seg=seg, sel=sel)

        # codebook-0 head + CE over positions [0, S-1) of every sequence (reference utils.py:96-106)
        logits = torch.empty(M, Vp, dtype=F32, device=dev)
        self._need("other", -1)
        ops.linear_fwd(hidden, m.block("codebook0_head.padded"), logits)
        t0 = torch.full((B, S), -1, dtype=torch.int64, device=dev)
        t0[:, :S - 1] = tg[:, :S - 1, 0]
        t0 = t0.reshape(M).contiguous()
        # with an ignore index the mean runs over the labelled rows only (torch CE semantics); the kernel skips t < 0
        n_sem = B * (S - 1) if ign is None else max(1, int((t0 >= 0).sum()))
        rows_loss = torch.empty(M, dtype=F32, device=dev)
        ops.ce_fwd_bwd(logits, t0, rows_loss, None, V, 0.0)
        sem = torch.empty(1, dtype=F32, device=dev)
        ops.reduce_sum(rows_loss, sem, 1.0 / n_sem)

        ac = torch.zeros(1, dtype=F32, device=dev)
        dec = None
        if m.acoustic_mode != "off":
            rows = self._acoustic_rows(B, S, acoustic_rows, t0 if ign is not None else None)
            dec = self._decoder_forward(hidden, rows, tg, B, S, save, sel=sel)
            ops.reduce_sum(dec["rows_loss"], ac, 1.0 / dec["n_rows"])
        total = semantic_weight * sem + acoustic_weight * ac
        if rows_out is not None:
            # copies: the backward runs the CE kernels again over the saved row buffers
            rows_out["semantic_rows"] = rows_loss.view(B, S).clone()                        # 0 where unlabelled
            if dec is not None:
                rows_out["acoustic_rows"] = dec["rows_loss"].view(K - 1, -1).t().contiguous()   # [N, K-1], codebooks 1..K-1
                rows_out["acoustic_row_index"] = rows.to(torch.int64)                       # b * S + p of every row
            else:
                rows_out["acoustic_rows"] = torch.zeros(0, K - 1, dtype=F32, device=dev)
                rows_out["acoustic_row_index"] = torch.zeros(0, dtype=torch.int64, device=dev)
        if save:
            self.saved = dict(B=B, S=S, tk=tk, mk=mk, hidden=hidden, logits=logits, t0=t0, n_sem=n_sem, dec=dec, seg=seg, sel=sel,
                              sw=float(semantic_weight), aw=float(acoustic_weight))
        return total[0], sem[0], ac[0]

    def _adapter_sel(self, adapter_ids, B, S, segment_lengths):
        """``sel`` [B*S] int32 on the device for a stack of adapter sets (``adapter_rows``; built on the host and copied once per
        step, like ``Segments``), None without one.  A stack and ``adapter_ids`` come together or not at all."""
        lo = self.m.lora
        stacked = lo is not None and getattr(lo, "n_adapters", 1) > 1
        if not stacked:
            if adapter_ids is not None:
                raise ValueError("adapter_ids name an adapter set per example, and model.lora is "
                                 + ("not attached" if lo is None else "a single adapter set")
                                 + ": attach a stack (apply_lora_to_model(..., n_adapters=A)) or drop adapter_ids")
            return None
        if adapter_ids is None:
            raise ValueError(f"model.lora stacks {lo.n_adapters} adapter sets: pass adapter_ids (one per example, -1 = base model "
                             "only), or export(a) one set and attach it alone")
        if not LORA_FUSE:
            raise NotImplementedError("a stack of adapter sets trains through the K-extension path only: unset CSM_LORA_FUSE=0")
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("a stack of adapter sets under a process group is not built (data parallel would all-reduce "
                                      "the stack): train it in one process")
        return adapter_rows(adapter_ids, B, S, lo.n_adapters, segment_lengths).to(self.m.device, non_blocking=True)

    def _validate_batch(self, tokens, masks, targets, ign):
        """Range checks of the integer inputs: the kernels index embedding tables, logits rows and gradient tables with
        them unchecked, so an id outside its table is an out-of-bounds device access (the reference's nn.Embedding /
        F.cross_entropy would assert).  Host batches (what a DataLoader hands over) are checked every time - min / max of
        a few hundred thousand integers on the CPU, no device sync.  Device-resident batches (benchmarks, gradient
        accumulation over one batch) cost a device sync, so a verdict is remembered for that exact tensor version."""
        a = self.m.args
        V, TV, K = a.audio_vocab_size, a.text_vocab_size, a.audio_num_codebooks

        def check(tk, mk, tg):
            if ign is None and int(tg.min()) < 0:
                raise ValueError("target_audio_tokens out of range for audio_vocab_size: negative labels and no ignore index.  A "
                                 "next-frame batch (data.to_next_frame), IGNORE_INDEX padding and packed rows mark unlabelled "
                                 "positions with -100: set model.target_ignore_index = csm.data.IGNORE_INDEX (the trainers' "
                                 "objective='next_frame' / --objective next-frame, --ignore-padding and --pack-sequences do)")
            if int(tg.max()) >= V:
                raise ValueError("target_audio_tokens out of range for audio_vocab_size")
            if ign is not None and bool(((tg < 0) & (tg != ign)).any()):
                raise ValueError(f"negative target_audio_tokens other than the ignore index {ign}")
            live = mk.bool()
            au, tx = tk[..., :K], tk[..., K]
            au_live, tx_live = au[live[..., :K]], tx[live[..., K]]
            if au_live.numel() and (int(au_live.min()) < 0 or int(au_live.max()) >= V):
                raise ValueError("input_tokens: audio code out of range for audio_vocab_size")
            if tx_live.numel() and (int(tx_live.min()) < 0 or int(tx_live.max()) >= TV):
                raise ValueError("input_tokens: text id out of range for text_vocab_size")

        if not (tokens.is_cuda or targets.is_cuda):
            check(tokens, masks, targets)
            return
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (tokens, masks, targets)) + (ign,)
        if key != getattr(self, "_validated_batch", None):
            check(tokens, masks, targets)
            self._validated_batch = key

    def _acoustic_rows(self, B, S, rows, t0=None):
        """Flattened (b*S + p) indices, p < S-1, of the positions whose frame trains the depth decoder.  ``t0`` (the
        flattened codebook-0 labels, negative = ignored) restricts the choice to labelled frames."""
        dev = self.m.device
        if rows is not None:
            r = rows.to(device=dev, dtype=torch.int64)            # given over the B*(S-1) row space of compute_loss
            b, p = r // (S - 1), r % (S - 1)
            r = b * S + p
            if t0 is not None:
                r = r[t0[r] >= 0]
            return r.to(torch.int32).contiguous()
        if t0 is None and self.m.acoustic_mode != "all":
            # a random subset of all frames: drawn on the host (torch's CPU generator) and copied over - one small copy instead of
            # ~20 launches of device randperm / sort / index kernels in front of the depth decoder
            n_all = B * (S - 1)
            n = max(1, int(round(n_all * self.m.acoustic_fraction)))
            perm = torch.randperm(n_all)[:n].sort().values
            return ((perm // (S - 1)) * S + perm % (S - 1)).to(torch.int32).to(dev, non_blocking=True)
        ck = ("allr", B, S)
        allr = self._consts.get(ck)
        if allr is None:
            allr = self._consts[ck] = (torch.arange(B, device=dev)[:, None] * S + torch.arange(S - 1, device=dev)[None, :]).reshape(-1)
        if t0 is not None:
            allr = allr[t0[allr] >= 0]
            if allr.numel() == 0:
                raise ValueError("no labelled audio frame in the batch")
        if self.m.acoustic_mode == "all":
            return allr.to(torch.int32).contiguous()
        n = max(1, int(round(allr.numel() * self.m.acoustic_fraction)))
        perm = torch.randperm(allr.numel(), device=dev)[:n].sort().values
        return allr[perm].to(torch.int32).contiguous()

    def _decoder_forward(self, hidden, rows, tg, B, S, save, sel=None):
        m, a = self.m, self.m.args
        dev = m.device
        K, V, Vp = a.audio_num_codebooks, a.audio_vocab_size, m.vocab_pad
        N = rows.numel()
        d, dd = m.bb.embed_dim, m.dc.embed_dim
        codes = tg[:, :S, :].reshape(-1, K) if tg.shape[1] >= S else None
        if codes is None:   # targets may be exactly S-1 long: index through (b, p)
            b, p = rows.long() // S, rows.long() % S
            codes = tg[b, p]
        else:
            codes = codes[rows.long()]
        codes = codes.contiguous()
        seq = torch.empty(N * K, d, dtype=BF16, device=dev)
        ops.decoder_input_fwd(hidden, rows, codes, m.block("audio_embeddings.weight"), seq, V)
        x0 = torch.empty(N * K, dd, dtype=BF16, device=dev)
        ops.linear_fwd(seq, m.block("projection.weight"), x0)
        # (a stack of adapter sets: the K rows of a frame run with the set of the frame's position)
        dsel = sel[rows.long()].repeat_interleave(K).contiguous() if sel is not None else None
        xf = self.decoder.forward(x0, N, K, save, on_layer_start=self.param_hook, sel=dsel)   # [N*K, dd]
        logits = torch.empty(K - 1, N, Vp, dtype=F32, device=dev)
        ah = m.block("audio_head.padded")                                           # [K-1, dd, Vp]
        xf2 = xf.view(N, K * dd)
        ops.gemm(xf2[:, dd:2 * dd], ah[0], logits[0], None, False, True, batch=K - 1, sA=dd, sB=dd * Vp, sC=N * Vp)
        tgt = codes[:, 1:].t().contiguous().reshape(-1)                             # [(K-1)*N]
        rows_loss = torch.empty((K - 1) * N, dtype=F32, device=dev)
        ops.ce_fwd_bwd(logits.view(-1, Vp), tgt, rows_loss, None, V, 0.0)
        out = dict(rows_loss=rows_loss, n_rows=(K - 1) * N)
        if save:
            out.update(rows=rows, codes=codes, seq=seq, xf=xf, logits=logits, tgt=tgt, N=N, sel=dsel)
        return out

    # -------------------------------------------------------------------------------------------- backward
    def backward(self, gscale: float = 1.0):
        """Gradients of ``gscale * total`` accumulated into the gradient arena (and LoRA gradient tensors).
        Which groups receive weight gradients follows ``model.trainable`` (freeze flags / LoRA)."""
        if self.saved is None:
            raise RuntimeError("backward() without a saved forward (was the forward run under no_grad?)")
        s, m, a = self.saved, self.m, self.m.args
        self.saved = None
        dev = m.device
        B, S = s["B"], s["S"]
        K, V, Vp = a.audio_num_codebooks, a.audio_vocab_size, m.vocab_pad
        M, d, dd = B * S, m.bb.embed_dim, m.dc.embed_dim
        tr = m.trainable
        train_embeddings, train_other = tr["embeddings"], tr["other"]
        m.ensure_grads()
        # Gradient-buffer states (see Model.grad_state): "live" buffers are accumulated into; "stale" ones hold the
        # gradients a lazy optimizer step consumed and are overwritten by this backward (the weight-gradient GEMMs then
        # neither read their output nor need a zero fill) - or zeroed here if this backward will not write them.
        gst = m.grad_state
        dec_runs = s["dec"] is not None and s["aw"] != 0.0
        writes = {"backbone": tr["backbone"], "decoder": dec_runs and tr["decoder"], "other": train_other,
                  "embeddings": train_embeddings}
        acc = {}
        for g_, w_ in writes.items():
            acc[g_] = gst[g_] == "live"
            if gst[g_] == "stale" and (not w_ or g_ == "embeddings"):
                o_, n_ = m.group_range(g_)
                m.grad_arena[o_:o_ + n_].zero_()
                gst[g_] = "zero"
            if w_:
                gst[g_] = "live"
        if train_other and not acc["other"] and not dec_runs:          # the decoder-side tensors of "other" get no gradient
            m.block("projection.weight", True).zero_()
            m.block("audio_head.padded", True).zero_()
        hidden = s["hidden"]
        dseq = None
        dec_pos0 = None
        # ---- depth decoder (acoustic term)
        dec = s["dec"]
        if dec is not None and s["aw"] != 0.0:
            N = dec["N"]
            dl = torch.empty(K - 1, N, Vp, dtype=BF16, device=dev)
            ops.ce_fwd_bwd(dec["logits"].view(-1, Vp), dec["tgt"], dec["rows_loss"], dl.view(-1, Vp), V,
                           gscale * s["aw"] / dec["n_rows"])
            ah = m.block("audio_head.padded")
            dxf = torch.zeros(N, K * dd, dtype=BF16, device=dev)                   # position 0 has no head: stays 0
            ops.gemm(dl[0], ah[0], dxf[:, dd:2 * dd], None, False, False, batch=K - 1, sA=N * Vp, sB=dd * Vp, sC=dd)
            xf2 = dec["xf"].view(N, K * dd)
            if train_other:
                gah = m.block("audio_head.padded", True)
                ops.gemm(xf2[:, dd:2 * dd], dl[0], gah[0], gah[0] if acc["other"] else None, True, True, batch=K - 1, sA=dd,
                         sB=N * Vp, sC=dd * Vp, sR=dd * Vp)
            del dl
            dx0 = self.decoder.backward(dxf.view(N * K, dd), N, K, tr["decoder"], 1.0, on_layer_done=self.grad_hook,
                                        acc=acc["decoder"], sel=dec.get("sel"))
            dseq = torch.empty(N * K, d, dtype=BF16, device=dev)
            ops.linear_dx(dx0, m.block("projection.weight"), dseq)
            if train_other:
                ops.linear_dw(dx0, dec["seq"], m.block("projection.weight", True), accumulate=acc["other"])
            dec_pos0 = (dseq, dec["rows"], K)          # position 0 of every frame is the backbone state: scattered below
            if self.grad_hook is not None:
                self.grad_hook("decoder", -1)

        # ---- codebook-0 head (semantic term)
        dlog = torch.empty(M, Vp, dtype=BF16, device=dev)
        rows_loss = torch.empty(M, dtype=F32, device=dev)
        ops.ce_fwd_bwd(s["logits"], s["t0"], rows_loss, dlog, V, gscale * s["sw"] / s["n_sem"])
        dhid = torch.empty(M, d, dtype=BF16, device=dev)
        ops.linear_dx(dlog, m.block("codebook0_head.padded"), dhid)
        if train_other:
            ops.linear_dw(dlog, hidden, m.block("codebook0_head.padded", True), accumulate=acc["other"])
        del dlog
        if dec_pos0 is not None:
            ops.rows_add_bf16(dhid, dec_pos0[1], dec_pos0[0], dec_pos0[2])   # rows are unique: plain bf16 read-modify-write
        if self.grad_hook is not None:
            self.grad_hook("other", -1)

        # ---- backbone
        dh0 = self.backbone.backward(dhid, B, S, tr["backbone"], 1.0, on_layer_done=self.grad_hook, acc=acc["backbone"], seg=s.get("seg"),
                                    sel=s.get("sel"))
        if train_embeddings:
            self._embedding_backward(s, dh0, dseq if (dec is not None and s["aw"] != 0.0) else None)
        if self.grad_hook is not None:
            self.grad_hook("embeddings", -1)

    def _embedding_backward(self, s, dh0, dseq):
        """d(text_embeddings), d(audio_embeddings): every (embedding row, gradient source row) occurrence - live slots of
        the backbone input and, when the decoder was trained, positions 1..K-1 of its input - is sorted by embedding row
        (torch.sort: no host sync) and reduced by ``csm_embed_bwd_sorted`` in a fixed order, straight into the bf16
        gradient arena."""
        m, a = self.m, self.m.args
        dev = m.device
        K, V = a.audio_num_codebooks, a.audio_vocab_size
        TV = a.text_vocab_size
        n_rows = TV + K * V
        tk, mk = s["tk"], s["mk"]
        M = tk.shape[0]
        # shape-only index tensors (slot offsets, source ids) are built once per shape, not once per step
        ck = ("embbwd", M, K, V, TV)
        c = self._consts.get(ck)
        if c is None:
            slot = torch.arange(K + 1, device=dev)
            c = self._consts[ck] = dict(off=torch.where(slot < K, TV + slot * V, torch.zeros_like(slot)),            # [K+1] row offset of a slot
                                        src=torch.arange(M, device=dev).unsqueeze(1).expand(M, K + 1).reshape(-1).contiguous())
        rows = torch.where(mk.bool(), tk + c["off"], torch.full_like(tk, n_rows)).reshape(-1)   # [M (K+1)]; masked-out slots -> padding id
        src = c["src"]
        n_src = M
        if dseq is not None:
            codes, N = s["dec"]["codes"], s["dec"]["N"]
            dk = ("embbwd_dec", M, N, K, V, TV)
            d = self._consts.get(dk)
            if d is None:
                d = self._consts[dk] = dict(off=TV + torch.arange(K - 1, device=dev) * V,
                                            src=(M + torch.arange(N, device=dev).unsqueeze(1) * K + torch.arange(1, K, device=dev)).reshape(-1))
            rows = torch.cat([rows, (codes[:, :K - 1] + d["off"]).reshape(-1)])
            src = torch.cat([src, d["src"]])
            n_src = M + N * K
        if n_src <= (1 << 20):
            # (row, source) pairs are unique, so ONE key sort gives the order a stable sort by row gives (sources ascend within a
            # row exactly as the occurrences were listed) - a radix sort of 64-bit keys instead of a stable merge sort (18 launches)
            # plus two gathers
            key = torch.sort((rows << 20) | src).values
            rows_s, src_s = key >> 20, key & ((1 << 20) - 1)
        else:
            order = torch.argsort(rows, stable=True)
            rows_s, src_s = rows[order].contiguous(), src[order].contiguous()
        ops.embed_bwd_sorted(rows_s, src_s, dh0, dseq,
                             m.block("text_embeddings.weight", True), m.block("audio_embeddings.weight", True))

    # -------------------------------------------------------------------------------------------- generation
    @torch.no_grad()
    def hidden_states(self, tokens: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
        """Backbone hidden states [B, S, D] (bf16) for full sequences - used by generation and by parity tests."""
        m, a = self.m, self.m.args
        B, S, K1 = tokens.shape
        M = B * S
        tk = tokens.reshape(M, K1).to(device=m.device, dtype=torch.int64).contiguous()
        mk = masks.reshape(M, K1).to(device=m.device, dtype=torch.uint8).contiguous()
        h0 = torch.empty(M, m.bb.embed_dim, dtype=BF16, device=m.device)
        self._need()
        ops.embed_fwd(tk, mk, m.block("text_embeddings.weight"), m.block("audio_embeddings.weight"), h0, a.audio_vocab_size)
        return self.backbone.forward(h0, B, S, False).view(B, S, -1)

    @torch.no_grad()
    def generate_frame(self, tokens, tokens_mask, input_pos, temperature, topk, noise=None, adapters=None, top_p=None,
                       min_p=None, repetition_penalty=None, repetition_window=None, typical_p=None, stats=False):
        """Reference model.py:140-195: backbone position(s) -> c0 -> 31 depth-decoder steps, against KV caches.

        The prompt (``input_pos`` starting at 0) is prefilled with the training forward kernels and its post-RoPE K/V
        rows are copied into the backbone cache; every later call is a single-position decode step (matrix-vector
        kernels + cache attention).  The decoder cache is reset every frame, as the reference does (model.py:181).
        ``model.use_kv_cache = False`` selects the cache-free prefix-recompute path (same arithmetic, kept as a check).
        ``adapters`` (read on the first call of a generation, ignored later): a LoRAState or None per batch row - per-utterance
        adapters from a bank (csm/lora_bank.py).
        ``temperature`` / ``topk``: two numbers - or, with caches, a sequence of B values for either one (a parameter pair per
        row, ``DecodeState.sampling_args``), or None for both (the pairs ``DecodeState.set_row_sampling`` wrote).
        ``top_p`` / ``min_p`` (with caches; None: not named): a number or B values for either one - the rows then sample through
        the filtered rows sampler (``DecodeState.set_row_filters``); give the same to every call of the generation.
        ``repetition_penalty`` / ``repetition_window`` (with caches; None: not named), or an entry per row that is K numbers in
        any of the six: the processed rows sampler (``DecodeState.sampling_args``); likewise the same to every call.
        ``typical_p`` (with caches; None: not named): a number, B entries, or per entry K numbers - locally typical sampling
        as the last filter, through the typical rows sampler (``DecodeState.set_row_typical``); likewise.
        ``stats`` (with caches; read on the first call of a generation): the state keeps every codebook's logits of the frame
        and one more launch writes each drawn code's log-probability, entropy and largest probability
        (``DecodeState.enable_stats`` / ``frame_stats``); the codes are the same.
        """
        m, a = self.m, self.m.args
        self._need()
        if int(input_pos[0, 0]) == 0:
            m._gen_adapters = list(adapters) if adapters is not None and any(x is not None for x in adapters) else None
        if not getattr(m, "use_kv_cache", True):
            if stats:
                raise ValueError("the recompute path (use_kv_cache = False) has no return_stats: the statistics need the KV-cache "
                                 "path")
            if names_processors(temperature, topk, repetition_penalty=repetition_penalty, repetition_window=repetition_window):
                raise ValueError("the recompute path (use_kv_cache = False) has no repetition penalty and no per-codebook "
                                 "parameters: they need the KV-cache path")
            if typical_p is not None:
                raise ValueError("the recompute path (use_kv_cache = False) has no typical_p: typical sampling needs the KV-cache "
                                 "path")
            if top_p is not None or min_p is not None:
                raise ValueError("the recompute path (use_kv_cache = False) has no top_p / min_p: the filters need the KV-cache path")
            return self._generate_frame_recompute(tokens, tokens_mask, input_pos, temperature, topk, noise)
        dev = m.device
        K, V, Vp = a.audio_num_codebooks, a.audio_vocab_size, m.vocab_pad
        d, dd = m.bb.embed_dim, m.dc.embed_dim
        tokens, tokens_mask = tokens.to(dev), tokens_mask.to(dev)
        Bn, Sn, K1 = tokens.shape
        first = int(input_pos[0, 0]) == 0
        st = getattr(m, "_decode_state", None)
        if not first and (st is None or st.B != Bn or st.cur < 0):
            raise RuntimeError("generate_frame: a non-first call (input_pos > 0) needs the state of a prompt prefilled with the "
                               "same batch size (call it with input_pos starting at 0 first)")
        if first:
            st = m._decode_state = DecodeState(self, Bn, adapters)
            if stats:
                st.enable_stats()
        temperature, topk = st.sampling_args(temperature, topk, top_p, min_p, repetition_penalty, repetition_window,
                                             typical_p=typical_p)
        st.set_live(range(Bn))
        if first:
            last_h = st.prefill(tokens, tokens_mask)
            return self._frame_tail(st, last_h, temperature, topk, noise)
        if Sn != 1:
            raise ValueError("generate_frame with caches: after the prompt, feed one position per call")
        if getattr(m, "use_hip_graph", True):
            return st.graph_frame(tokens, tokens_mask, temperature, topk, noise)
        st._advance()
        return self._decode_frame(st, tokens, tokens_mask, temperature, topk, noise)

    @torch.no_grad()
    def generate_first_frames(self, tokens_list, masks_list, temperature, topk, noise=None, adapters=None, top_p=None,
                              min_p=None, repetition_penalty=None, repetition_window=None, typical_p=None, stats=False):
        """Batched generation (up to 16 utterances): prefill B prompts of different lengths and sample the
        first frame of each; later frames go through ``generate_frame`` with ``[B, 1, K+1]`` tokens and a non-zero
        ``input_pos``, exactly as for one utterance.  ``temperature`` / ``topk``: two numbers, or a sequence of B values for
        either one - row b then samples with its own pair (``DecodeState.sampling_args``); give the same to ``generate_frame``.
        ``top_p`` / ``min_p`` / ``repetition_penalty`` / ``repetition_window`` / ``typical_p`` / ``stats``: as for ``generate_frame``."""
        m = self.m
        self._need()
        if stats and not getattr(m, "use_kv_cache", True):
            raise ValueError("the recompute path (use_kv_cache = False) has no return_stats: the statistics need the KV-cache path")
        st = m._decode_state = DecodeState(self, len(tokens_list), adapters)
        if stats:
            st.enable_stats()
        temperature, topk = st.sampling_args(temperature, topk, top_p, min_p, repetition_penalty, repetition_window,
                                             typical_p=typical_p)
        st.set_live(range(st.B))
        last_h = st.prefill_ragged(tokens_list, masks_list)
        return self._frame_tail(st, last_h, temperature, topk, noise)

    def _decode_frame(self, st, tokens, tokens_mask, temperature, topk, noise):
        """One decode frame, eagerly."""
        st.fill_noise(noise)
        return self._decode_frame_body(st, tokens, tokens_mask, temperature, topk)

    def _decode_frame_body(self, st, tokens, tokens_mask, temperature, topk):
        """One decode frame with no host-side dependence on device data and no random draw: this is the body a HIP graph
        captures (the frame's Exp(1) noise sits in ``st.noise_buf``, filled before the body runs / the graph replays)."""
        last_h = st.backbone_step(tokens, tokens_mask)
        return self._frame_tail_body(st, last_h, temperature, topk)

    def _frame_tail(self, st, last_h, temperature, topk, noise):
        st.fill_noise(noise)
        return self._frame_tail_body(st, last_h, temperature, topk)

    def _frame_tail_body(self, st, last_h, temperature, topk):
        m, a = self.m, self.m.args
        K, V = a.audio_num_codebooks, a.audio_vocab_size
        from .models.model import sample_topk

        qall = st.noise_buf          # all Exp(1) draws of the frame (the reference draws them one codebook at a time, model.py:79-82)

        if (temperature is None) != (topk is None):
            raise ValueError("temperature and topk are both numbers, or both None (each row's own pair: set_row_sampling)")

        def draw(lg, i):
            if temperature is None:
                # each row's own parameters, read by the sampler from the state's buffers (written outside the graph)
                return st.sampler.draw(lg[:, :V], i, qall[i])
            return sample_topk(lg[:, :V], topk, temperature, qall[i])

        # statistics mode (DecodeState.enable_stats): codebook i's logits go to their own slice and stay until the frame's end
        lg_of = (lambda i: st.logits_all[i]) if st.stats is not None else (lambda i: st.logits)
        ops.gemv(last_h, m.block("codebook0_head.padded"), lg_of(0))
        samples = [draw(lg_of(0), 0)]
        dnorm = m.block("decoder.norm.scale")
        for i in range(K):
            # decoder position i: input = backbone state (i = 0) or the embedding of code i-1; the stack's final norm is
            # applied inside the head product (position 0 has no head)
            hres = (st.decoder_step(last_h, i, final_norm=False) if i == 0 else
                    st.decoder_step(None, i, code=samples[-1].view(-1), final_norm=False))
            if i >= 1:
                # [V][d'] copy of audio_head[i-1]: row-per-wave GEMV
                ops.gemv_ex(hres, st.head_t[i - 1], lg_of(i), norm_scale=dnorm, eps=m.dc.norm_eps)
                samples.append(draw(lg_of(i), i))
        if st.stats is not None:
            # ONE launch over the frame's K * B rows (row i * B + b: codebook i, sequence b), on the codes in that order
            ops.sample_stats_rows(st.logits_all.view(K * st.B, -1), torch.cat(samples, dim=0).view(-1), st.stats[0].view(-1),
                                  st.stats[1].view(-1), st.stats[2].view(-1), V=V)
        return torch.cat(samples, dim=1)

    @torch.no_grad()
    def _generate_frame_recompute(self, tokens, tokens_mask, input_pos, temperature, topk, noise=None):
        """Reference model.py:140-195.  The KV state is the token history (prefix recompute)."""
        if not (_is_number(temperature) and _is_number(topk)):
            raise ValueError("the recompute path (use_kv_cache = False) samples every row with one temperature and one topk: "
                             "per-row sampling parameters need the KV-cache path")
        ads = getattr(self.m, "_gen_adapters", None)
        if ads is not None:
            # (the cache-free check path runs ONE adapter set for the whole batch: the training forward has no per-row adapters)
            if self.m.lora is not None and not self.m.lora.merged:
                raise ValueError("generate with per-utterance LoRA adapters while live (un-merged) adapters are attached as "
                                 "model.lora: detach or merge them first")
            if any(a is not ads[0] for a in ads):
                raise ValueError("the recompute path (use_kv_cache = False) takes one adapter for all rows, not one per row")
            with row_lora(self.m, ads[0]):
                return self._generate_frame_recompute_body(tokens, tokens_mask, input_pos, temperature, topk, noise)
        with generation_lora(self.m):
            return self._generate_frame_recompute_body(tokens, tokens_mask, input_pos, temperature, topk, noise)

    def _generate_frame_recompute_body(self, tokens, tokens_mask, input_pos, temperature, topk, noise):
        m, a = self.m, self.m.args
        dev = m.device
        K, V, Vp = a.audio_num_codebooks, a.audio_vocab_size, m.vocab_pad
        d, dd = m.bb.embed_dim, m.dc.embed_dim
        tokens = tokens.to(dev)
        tokens_mask = tokens_mask.to(dev)
        first = int(input_pos[0, 0]) == 0
        if first or m._gen_hist is None:
            hist_t, hist_m = tokens, tokens_mask
        else:
            hist_t = torch.cat([m._gen_hist[0], tokens], dim=1)
            hist_m = torch.cat([m._gen_hist[1], tokens_mask], dim=1)
        m._gen_hist = (hist_t, hist_m)
        Bn = hist_t.shape[0]
        hidden = self.hidden_states(hist_t, hist_m)                 # [B, S, d]
        last_h = hidden[:, -1, :].contiguous()                      # [B, d]
        logits = torch.empty(Bn, Vp, dtype=F32, device=dev)
        ops.linear_fwd(last_h, m.block("codebook0_head.padded"), logits)
        from .models.model import sample_topk

        def draw(lg, i):
            q = None if noise is None else noise[i].to(dev)
            if self.capture_logits is not None:                     # (parity tests: the logits each code of the frame was drawn from)
                self.capture_logits.append(lg[:, :V].clone())
            return sample_topk(lg[:, :V], topk, temperature, q)

        c0 = draw(logits, 0)                                         # [B,1] int32
        samples = [c0]
        aemb = m.block("audio_embeddings.weight")
        seq = [last_h.unsqueeze(1), aemb[c0.long() + 0 * V]]        # [B,1,d] each
        ah = m.block("audio_head.padded")
        for i in range(1, K):
            cur = torch.cat(seq, dim=1)                              # [B, L, d]
            L = cur.shape[1]
            x0 = torch.empty(Bn * L, dd, dtype=BF16, device=dev)
            ops.linear_fwd(cur.reshape(Bn * L, d).contiguous(), m.block("projection.weight"), x0)
            # (fuse_rope=False: round q/k to bf16 before the rotation, exactly as the decode kernels of the KV-cache path do, so
            #  that the two paths stay comparable bit for bit on the frame they both compute from scratch)
            xf = self.decoder.forward(x0, Bn, L, False, fuse_rope=False).view(Bn, L, dd)
            lg = torch.empty(Bn, Vp, dtype=F32, device=dev)
            ops.gemm(xf[:, -1, :].contiguous(), ah[i - 1], lg, None, False, True)
            ci = draw(lg, i)
            samples.append(ci)
            seq.append(aemb[ci.long() + i * V])
        return torch.cat(samples, dim=1)


class _DecodeStack:
    """KV caches + preallocated single-position buffers of one stack."""

    def __init__(self, stack: _Stack, B: int, s_max: int):
        c, dev = stack.c, stack.m.device
        self.stack, self.B, self.s_max = stack, B, s_max
        H, KV, hd, F, d = c.num_heads, c.num_kv_heads, c.head_dim, c.intermediate_dim, c.embed_dim
        z = lambda *shape, dt=BF16: torch.empty(*shape, dtype=dt, device=dev)   # noqa: E731
        # one allocation [layer, K | V, B, KV, s_max, hd]: a batch row's history in every layer is ONE strided slice of it
        # (DecodeState.park_row / resume_row); k[i] / v[i] are the contiguous per-layer views the kernels take
        self.kv = torch.zeros(c.num_layers, 2, B, KV, s_max, hd, dtype=BF16, device=dev)
        self.k = [self.kv[i, 0] for i in range(c.num_layers)]
        self.v = [self.kv[i, 1] for i in range(c.num_layers)]
        self.pos = torch.zeros(B, dtype=torch.int32, device=dev)
        self.xn, self.qkv, self.o, self.h, self.hn = z(B, d), z(B, c.qkv_dim), z(B, H * hd), z(B, d), z(B, d)
        self.gu, self.act, self.xa, self.xb, self.xf = z(B, 2 * F), z(B, F), z(B, d), z(B, d), z(B, d)
        # four launches per layer instead of five where the cache is short (csm_gemv_attn_bf16: S_max <= 64, head_dim 128).  Only
        # for one utterance: every workgroup of the fused launch recomputes the attention of all (row, head) pairs, which costs
        # more than the launch it saves from two rows on (measured: 149 vs 147 frames/s at B = 1, 331 vs 402 aggregate at B = 4)
        import os
        self.fuse_attn = B == 1 and s_max <= 64 and hd == 128 and os.environ.get("CSM_DECODE_FUSE_ATTN", "1") == "1"
        # the position as a host integer where the caller knows it (the depth decoder: step i is at position i): see ops.gemv_attn
        self.pos_host = None
        # LoRA groups (DecodeState.__init__): per layer {group name: (At, Bx, bias or None)}, and the [B, KX] extension operand
        self.lora, self.lora_scale, self.lt = None, 1.0, None
        # per-row adapters (attach_lora_rows): (row_adapter int32 [B], scale fp32 [A]) and the tensors the pointer tables name
        self.lora_rows, self.lora_keep = None, []
        # FP8 mode (model.decode_weights = "fp8", attach_fp8): {weight name: (e4m3 codes uint8 [N, K], scale fp32 [N])}
        self.w8 = None

    def attach_fp8(self):
        """Quantised copies of the layer products' weights (csm_quantize_rows_fp8), made from the current weights - the same
        staleness rule as ``DecodeState.head_t``.  The depth decoder's fused attention + output projection at one utterance keeps
        its bf16 weights (2 MB per launch, latency-bound: DESIGN.md section 4, 'FP8 weights'); CSM_FP8_FUSE_ATTN=0 runs it
        unfused on FP8 weights instead (measurement only)."""
        import os
        st = self.stack
        if self.fuse_attn and os.environ.get("CSM_FP8_FUSE_ATTN", "1") != "1":
            self.fuse_attn = False
        names = ["attn.qkv", "mlp.w13", "mlp.w2.weight"] + ([] if self.fuse_attn else ["attn.output_proj.weight"])
        self.w8 = {f"layers.{i}.{n}": ops.quantize_rows_fp8(st.w(f"layers.{i}.{n}")) for i in range(st.c.num_layers) for n in names}

    def weight_bytes(self):
        """Bytes of layer-product weights one decode step of this stack streams (codes + scales in FP8 mode)."""
        st, tot = self.stack, 0
        for i in range(st.c.num_layers):
            for n in ("attn.qkv", "attn.output_proj.weight", "mlp.w13", "mlp.w2.weight"):
                q = self.w8.get(f"layers.{i}.{n}") if self.w8 is not None else None
                tot += q[0].numel() + 4 * q[1].numel() if q is not None else 2 * st.w(f"layers.{i}.{n}").numel()
        return tot

    def fill_from(self, acts, B, S):
        """Copy the post-RoPE K / V rows of a prefilled prompt into the caches."""
        c = self.stack.c
        H, KV, hd = c.num_heads, c.num_kv_heads, c.head_dim
        for i, a in enumerate(acts):
            qkv = a["qkv"].view(B, S, -1)
            self.k[i][:, :, :S] = qkv[:, :, H * hd:(H + KV) * hd].reshape(B, S, KV, hd).permute(0, 2, 1, 3)
            self.v[i][:, :, :S] = qkv[:, :, (H + KV) * hd:].reshape(B, S, KV, hd).permute(0, 2, 1, 3)

    def fill_row(self, acts, b, S):
        """The same for ONE sequence (a [1, S] prefill) into batch row ``b`` of the caches: ragged batched prompts."""
        c = self.stack.c
        H, KV, hd = c.num_heads, c.num_kv_heads, c.head_dim
        for i, a in enumerate(acts):
            qkv = a["qkv"].view(S, -1)
            self.k[i][b, :, :S] = qkv[:, H * hd:(H + KV) * hd].reshape(S, KV, hd).permute(1, 0, 2)
            self.v[i][b, :, :S] = qkv[:, (H + KV) * hd:].reshape(S, KV, hd).permute(1, 0, 2)

    def step(self, x: torch.Tensor, final_norm: bool = True) -> torch.Tensor:
        """One position per batch row at ``self.pos`` (device int32).  x [B, d] -> final-normed hidden [B, d]
        (``final_norm=False``: the un-normed residual stream, for a caller that fuses the norm into its next product)."""
        st, c = self.stack, self.stack.c
        H, KV, hd = c.num_heads, c.num_kv_heads, c.head_dim
        table = st.m.rope_table(st.prefix)
        cur, nxt = x, self.xa
        for i in range(c.num_layers):
            L = self.lora[i] if self.lora is not None else {}
            # five launches per layer (four in the depth decoder): the norms ride in the prologue of the following matrix-vector
            # product, RoPE and the cache append inside the attention kernel, SwiGLU in the epilogue of the w13 product
            self._product(i, "attn.qkv", L.get("attn_in"), cur, self.qkv, norm_scale=st.w(f"layers.{i}.sa_norm.scale"), eps=c.norm_eps)
            if self.fuse_attn and "attn_out" not in L:
                # (depth decoder: <= 32 cached positions - the attention rides in the prologue of the output projection, always
                #  on its bf16 weight; an ``attn_out`` group takes the unfused attention and the extended product)
                ops.gemv_attn(self.qkv, self.k[i], self.v[i], self.pos, table, st.w(f"layers.{i}.attn.output_proj.weight"), self.h, cur,
                              H, KV, hd, pos_host=self.pos_host)
            else:
                ops.attn_decode_rope(self.qkv, self.k[i], self.v[i], self.o, self.pos, table, H, KV, hd, pos_host=self.pos_host)
                self._product(i, "attn.output_proj.weight", L.get("attn_out"), self.o, self.h, residual=cur)
            self._product(i, "mlp.w13", L.get("mlp_in"), self.h, self.act, norm_scale=st.w(f"layers.{i}.mlp_norm.scale"), eps=c.norm_eps,
                          swiglu=True)
            self._product(i, "mlp.w2.weight", L.get("mlp_out"), self.act, nxt, residual=self.h)
            cur, nxt = nxt, (self.xb if nxt is self.xa else self.xa)
        if not final_norm:
            return cur
        ops.rmsnorm_fwd(cur, st.w("norm.scale"), self.xf, None, c.norm_eps)
        return self.xf

    def _product(self, i, name, G, x, y, **kw):
        """One product of a layer step, y = epilogue(x^ W^T) with layer ``i``'s weight ``name`` and the caller's fusions (norm
        prologue, SwiGLU, residual), in the stack's mode.  With a LoRA group ``G`` on the projection: t = s x^ At, then the same
        product with (t, Bx, bias) as K-extension - two launches, over pointer tables where each row has its own adapter (or
        none).  Without: the e4m3 copy of the weight where ``attach_fp8`` made one (csm_gemv_fp8w), else the bf16 weight.
        Per-row adapters on a weight that has an e4m3 copy (``model.fp8_adapters``): the same t, then csm_gemv_fp8w_kext_rows -
        the extension joins the SCALED base sum; a weight without a copy (the depth decoder's output projection while
        ``fuse_attn`` keeps it bf16, met here only under an ``attn_out`` group) keeps the bf16 extended product."""
        name = f"layers.{i}.{name}"
        if G is None:
            if self.w8 is not None and name in self.w8:
                return ops.gemv_fp8w(x, *self.w8[name], y, **kw)
            return ops.gemv_ex(x, self.stack.w(name), y, **kw)
        W, norm = self.stack.w(name), dict(norm_scale=kw.get("norm_scale"), eps=kw.get("eps", 1e-5))
        if self.lora_rows is not None:
            At_tab, Bx_tab, bias_tab, kx, lda, ldb = G
            ra, scale = self.lora_rows
            ops.lora_project_rows(x, At_tab, self.lt, ra, scale, kx, lda, **norm)
            if self.w8 is not None and name in self.w8:
                return ops.gemv_fp8w_kext_rows(x, *self.w8[name], y, self.lt, Bx_tab, ra, kx, ldb, bias_tab=bias_tab, **kw)
            return ops.gemv_kext_rows(x, W, y, self.lt, Bx_tab, ra, kx, ldb, bias_tab=bias_tab, **kw)
        At, Bx, bias = G
        t = self.lt[:, :At.shape[1]]
        ops.lora_project(x, At, t, self.lora_scale, **norm)
        return ops.gemv_kext(x, W, y, t, Bx, bias=bias, **kw)

    def _group_bias(self, G):
        """The bias vector of LoRA group ``G`` in the fused projection's row order (q | k | v stacked, w1 / w3 interleaved), built
        once at binding (the same pattern as ``DecodeState.head_t``); None where no adapter of the group has a bias."""
        if all(ad.bias is None for ad in G.adapters.values()):
            return None
        c = self.stack.c
        hq, hk, F, d = c.num_heads * c.head_dim, c.num_kv_heads * c.head_dim, c.intermediate_dim, c.embed_dim
        rows = {"q_proj": slice(0, hq), "k_proj": slice(hq, hq + hk), "v_proj": slice(hq + hk, hq + 2 * hk), "output_proj": slice(0, d),
                "w1": slice(0, 2 * F, 2), "w3": slice(1, 2 * F, 2), "w2": slice(0, d)}
        bias = torch.zeros(G.Bx.shape[0], dtype=BF16, device=G.Bx.device)
        for mod, ad in G.adapters.items():
            if ad.bias is not None:
                bias[rows[mod]] = ad.bias
        return bias

    @staticmethod
    def _check_kx(G):
        """The K-extension kernels give each of a wave's 64 lanes one 8-element chunk of the extension: at most 512 columns."""
        if G.kx > 512:
            raise ValueError(f"generate with LoRA adapters: {G.kx} extension columns in {G.name} (the decode kernels take "
                             "at most 512: rank x adapters per fused projection)")

    def attach_lora(self, lo):
        """Bind the active adapters of this stack: arena views of every group's At / Bx (read in place, so a captured graph
        sees what ``load_lora_weights`` or an optimiser writes there) and the group's bias vector (``_group_bias``)."""
        _refuse_stack(lo, "a decode state")
        st, c = self.stack, self.stack.c
        plan, kmax = [], 0
        for i in range(c.num_layers):
            L = {}
            for gname in ("attn_in", "attn_out", "mlp_in", "mlp_out"):
                G = lo.group(st.prefix, i, gname)
                if G is None:
                    continue
                self._check_kx(G)
                L[gname] = (G.At, G.Bx, self._group_bias(G))
                kmax = max(kmax, G.kx)
            plan.append(L)
        if kmax:
            self.lora, self.lora_scale = plan, lo.scaling
            self.lt = torch.zeros(self.B, kmax, dtype=BF16, device=self.k[0].device)

    def attach_lora_rows(self, states, bank=None):
        """``attach_lora`` for one adapter per batch row (``states``: a LoRAState or None per row, bank entries of one layout).
        ``bank`` (a list of LoRAState): bind all of these, in this order, whether a row uses them yet or not - a serving state
        whose rows change adapters later (``DecodeState.set_row_adapter``); the tables are then indexed by bank position.
        The adapters used are compacted to indices 0..A-1 (``row_adapter``, -1 = none); per layer and group the device tables
        hold the addresses of each adapter's At / Bx arena views (read in place: a captured graph sees later writes to the
        adapters' weights) and of its bias vector (``_group_bias``; address 0 = none)."""
        st, c = self.stack, self.stack.c
        dev = self.k[0].device
        used, idx = list(bank or []), []
        for s in states:
            if s is None:
                idx.append(-1)
                continue
            k = next((j for j, u in enumerate(used) if u is s), None)
            if k is None:
                used.append(s)
                k = len(used) - 1
            idx.append(k)
        if not used:
            return

        def table(ptrs):
            return torch.tensor(ptrs, dtype=torch.int64, device=dev)

        plan, kmax, keep = [], 0, []
        for i in range(c.num_layers):
            L = {}
            for gname in ("attn_in", "attn_out", "mlp_in", "mlp_out"):
                Gs = [s.group(st.prefix, i, gname) for s in used]
                if all(G is None for G in Gs):
                    continue
                if any(G is None or G.kx != Gs[0].kx or G.At.stride(0) != Gs[0].At.stride(0) or G.Bx.stride(0) != Gs[0].Bx.stride(0)
                       for G in Gs):
                    raise ValueError(f"per-row LoRA adapters: {st.prefix} layer {i} {gname}: the adapters do not share one layout")
                kx = Gs[0].kx
                self._check_kx(Gs[0])
                for G in Gs:
                    if G.At.data_ptr() % 16 or G.Bx.data_ptr() % 16 or G.At.stride(1) != 1 or G.Bx.stride(1) != 1:
                        raise ValueError(f"per-row LoRA adapters: {G.name} is not a 16-byte aligned row-major arena view")
                biases = [self._group_bias(G) for G in Gs]
                keep += [b for b in biases if b is not None]
                bias_tab = table([0 if b is None else b.data_ptr() for b in biases]) if any(b is not None for b in biases) else None
                L[gname] = (table([G.At.data_ptr() for G in Gs]), table([G.Bx.data_ptr() for G in Gs]), bias_tab, kx,
                            Gs[0].At.stride(0), Gs[0].Bx.stride(0))
                kmax = max(kmax, kx)
            plan.append(L)
        if kmax:
            self.lora = plan
            self.lora_rows = (torch.tensor(idx, dtype=torch.int32, device=dev),
                              torch.tensor([s.scaling for s in used], dtype=torch.float32, device=dev))
            # the adapters' arenas must outlive the state: the tables hold raw addresses
            self.lora_keep = keep + [s.arena for s in used]
            self.lt = torch.zeros(self.B, kmax, dtype=BF16, device=dev)


_graph_rng_primed = None


def _prime_graph_rng(device):
    """The process's first graph capture creates the CUDA generator's capture-state tensors and every later capture updates
    them in place.  Created under ``torch.inference_mode`` (``Generator.generate``, a ``Conversation`` turn) they would be
    inference tensors and a later capture outside it (``Model.generate_frame`` called directly) would be refused - so the first
    capture of the process is a one-element one made here, outside inference mode, and its graph is kept for the life of the
    process (the generator drops those tensors when the last graph that registered with it goes)."""
    global _graph_rng_primed
    if _graph_rng_primed is not None:
        return
    with torch.inference_mode(False):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            torch.zeros(1, device=device)
    _graph_rng_primed = g


class ParkedRow:
    """What ``DecodeState.park_rows`` takes out of one row in the middle of an utterance and ``resume_rows`` puts back into any
    row: ``kv`` - the row's K / V in ``park_row``'s format, all the positions it held; ``hist`` - int32 [K * 64 + 1], its ring of
    sampled codes and its frame counter (None below the levels that keep rings); ``gen`` - its noise generator (None: unseeded)."""
    __slots__ = ("kv", "hist", "gen")

    def __init__(self, kv, hist, gen):
        self.kv, self.hist, self.gen = kv, hist, gen


class DecodeState:
    """Everything ``generate_frame`` keeps between calls: the two stacks' caches and small persistent buffers."""

    def __init__(self, engine: "Engine", B: int, adapters=None, bank=None):
        """``bank``: every LoRAState a row may be given later (``set_row_adapter``) - a serving state (csm/serving.py).  They are
        all bound here, once: the kernels' pointer tables and the adapter count are captured into the frame graph, so an adapter
        added to the bank afterwards needs a new state."""
        m = engine.m
        bank = list(bank) if bank else None
        if bank is not None:
            if adapters is not None and any(a is not None for a in adapters):
                raise ValueError("a serving state takes its rows' adapters through set_row_adapter, not at creation")
            adapters = [None] * B
        if not 1 <= B <= 16:
            raise ValueError(f"the decode kernels handle 1 to 16 sequences at a time (got {B})")
        # per-row adapters (csm/lora_bank.py): a LoRAState or None per row; all None is the same as no adapters
        if adapters is not None and len(adapters) != B:
            raise ValueError(f"per-row LoRA adapters: {len(adapters)} entries for {B} sequences")
        self.adapters = list(adapters) if adapters is not None and (bank is not None or any(a is not None for a in adapters)) else None
        self.bank = bank
        if self.adapters is not None and m.lora is not None and not m.lora.merged:
            raise ValueError("generate with per-utterance LoRA adapters while live (un-merged) adapters are attached as model.lora: "
                             "detach them (model.lora = None), merge them (merge_lora_weights) or add them to the bank instead")
        if B > 4 and self.adapters is None and m.lora is not None and not m.lora.merged:
            # (the K-extension kernels of live adapters take at most 4 rows: csm_gemv_bf16_kext, csm_lora_project_bf16)
            raise ValueError(f"generate with live (un-merged) LoRA adapters takes at most 4 sequences at a time (got {B}): "
                             "merge them first (merge_lora_weights) or decode at most 4 utterances")
        self.decode_weights = getattr(m, "decode_weights", "bf16")
        fp8_adapters = bool(getattr(m, "fp8_adapters", False))
        if self.decode_weights == "fp8" and m.lora is not None and not m.lora.merged and self.adapters is None and fp8_adapters:
            raise ValueError('decode_weights = "fp8" with live (un-merged) LoRA adapters as model.lora: the FP8 K-extension kernels '
                             'take per-utterance adapters only - merge the adapters first (merge_lora_weights), pass them per '
                             'utterance or through the bank instead (generate(adapter=), load_adapter), or set '
                             'model.decode_weights = "bf16"')
        if self.decode_weights == "fp8" and not fp8_adapters and (self.adapters is not None or (m.lora is not None and not m.lora.merged)):
            raise ValueError('decode_weights = "fp8" with live (un-merged) LoRA adapters or a per-utterance adapter bank: the '
                             'K-extension decode kernels are bf16-only - merge the adapters first (merge_lora_weights) or set '
                             'model.decode_weights = "bf16".  Per-utterance adapters and banks run on the quantised base with '
                             'model.fp8_adapters = True (an opt-in: the adapters were trained against the bf16 base)')
        self.e, self.B = engine, B
        dev = m.device
        self.bb = _DecodeStack(engine.backbone, B, m.bb.max_seq_len)
        self.dc = _DecodeStack(engine.decoder, B, m.args.audio_num_codebooks)
        self.h0 = torch.empty(B, m.bb.embed_dim, dtype=BF16, device=dev)
        self.proj = torch.empty(B, m.dc.embed_dim, dtype=BF16, device=dev)
        self.logits = torch.empty(B, m.vocab_pad, dtype=F32, device=dev)
        self.logits_all, self.stats = None, None             # (statistics mode: enable_stats)
        self.dpos = [torch.full((B,), i, dtype=torch.int32, device=dev) for i in range(m.args.audio_num_codebooks)]
        # each row's position on the host (-1 = nothing prefilled): the one mirror of the device-side ``bb.pos`` (no sync per frame;
        # an idle row's device position is pinned, not mirrored).  Slot lifecycle (prefill_row / set_active / serve_frame): the
        # rows that advance (host list + the device vector the idle rows' positions are pinned with), per-row noise generators
        # and the rows the next fill_noise draws for
        self.row_pos = [-1] * B
        self.active_rows = list(range(B))
        self.active = None
        self.row_gen, self.draw_rows, self.noise_stage = {}, None, None
        self.graph, self.graph_key, self.warm = None, None, 0
        # per-row sampling parameters (set_row_sampling / set_row_filters / set_row_processors): one state with a level
        self.sampler = RowSampler(B, m.args.audio_num_codebooks, m.args.audio_vocab_size, dev)
        # the frame's Exp(1) draws [K, B, V]: a PERSISTENT buffer, refilled before every frame outside the captured graph -
        # so a replayed frame can be given the same noise as an eager one (parity tests) or fresh draws (generation)
        self.noise_buf = torch.empty(m.args.audio_num_codebooks, B, m.args.audio_vocab_size, dtype=F32, device=dev)
        # audio_head is stored [K-1][d'][V] (reference layout, a K-major matrix for x @ W); the decode path wants one
        # output row per wave, so it keeps a [K-1][V][d'] copy made from the current weights when the state is created
        self.head_t = m.block("audio_head.padded").transpose(1, 2).contiguous()
        # FP8 mode: e4m3 copies + row scales of the layer products' weights, made here from the current weights like head_t
        if self.decode_weights == "fp8":
            self.bb.attach_fp8()
            self.dc.attach_fp8()
        # live LoRA adapters ride on the decode products as K-extensions (merged ones are already in the weights)
        if self.adapters is not None:
            self.bb.attach_lora_rows(self.adapters, bank)
            self.dc.attach_lora_rows(self.adapters, bank)
        elif m.lora is not None and not m.lora.merged:
            self.bb.attach_lora(m.lora)
            self.dc.attach_lora(m.lora)

    def enable_stats(self):
        """Statistics mode, before the first capture: every frame keeps its K codebooks' logits (``logits_all`` fp32
        [K, B, vocab_pad]: codebook i's head writes slice i, the draw reads it) and ends with ONE ``sample_stats_rows`` launch over
        the K * B rows that fills ``stats`` fp32 [3, K, B] - the log-probability of each drawn code, the entropy and the largest
        probability of the distribution it was drawn from, at temperature 1 with no filter and no penalty, whatever the sampler
        level.  The codes are the same bits.  The frame graph's key gets a tag (``RowSampler.graph_key``): a graph captured
        without statistics is never replayed with them - a call after the first capture costs one eager frame and a new capture,
        so make it before."""
        if self.stats is not None:
            return
        m, dev = self.e.m, self.logits.device
        K = m.args.audio_num_codebooks
        self.logits_all = torch.empty(K, self.B, m.vocab_pad, dtype=F32, device=dev)
        self.stats = torch.zeros(3, K, self.B, dtype=F32, device=dev)
        self.sampler.stats = True

    def frame_stats(self):
        """The last frame's statistics, copied out on the device (no host synchronisation): fp32 [3, K, B] - logprob, entropy,
        pmax - of the codes the frame call returned."""
        if self.stats is None:
            raise RuntimeError("no statistics: call enable_stats before the first frame")
        return self.stats.clone()

    def fill_noise(self, noise=None):
        """``noise``: K tensors [B, V] of Exp(1) draws (pins the sampler), or None for fresh draws from torch's generator."""
        if noise is None:
            self.noise_buf.exponential_(1)
        else:
            for i, q in enumerate(noise):
                self.noise_buf[i].copy_(q.reshape(self.noise_buf[i].shape), non_blocking=True)
        # rows with a generator of their own (set_row_seed) get ONE [K, V] Exp(1) draw from it, in codebook order - so a seeded
        # request's frames do not depend on its row, its neighbours or when it joined.  ``draw_rows`` limits the draws to the rows
        # that sample this frame (an idle row's generator must not move).
        for b, g in self.row_gen.items():
            if self.draw_rows is None or b in self.draw_rows:
                if self.noise_stage is None:
                    K, _, V = self.noise_buf.shape
                    self.noise_stage = torch.empty(K, V, dtype=F32, device=self.noise_buf.device)
                self.noise_buf[:, b].copy_(self.noise_stage.exponential_(1, generator=g))     # two launches per seeded row

    @property
    def cur(self):
        """The last position the caches hold, over all rows (-1: nothing prefilled)."""
        return max(self.row_pos)

    def _advance(self):
        """The rows of a decode frame (``active_rows``: all of them unless ``set_active`` chose) move one position on, on the host;
        the device positions move inside the frame (``backbone_step``).  The decode kernels index LDS and the KV caches with the
        position, so a row at the length limit refuses the frame and nothing moves."""
        if any(self.row_pos[b] + 1 >= self.e.m.bb.max_seq_len for b in self.active_rows):
            raise ValueError("sequence exceeds max_seq_len")
        for b in self.active_rows:
            self.row_pos[b] += 1

    def _embed(self, tokens, masks, out=None):
        """The embedded rows [M, d] of [..., K+1] tokens and masks, into ``out`` or a new tensor."""
        m = self.e.m
        K1 = tokens.shape[-1]
        tk = tokens.reshape(-1, K1).to(device=m.device, dtype=torch.int64).contiguous()
        mk = masks.reshape(-1, K1).to(device=m.device, dtype=torch.uint8).contiguous()
        h0 = out if out is not None else torch.empty(tk.shape[0], m.bb.embed_dim, dtype=BF16, device=m.device)
        ops.embed_fwd(tk, mk, m.block("text_embeddings.weight"), m.block("audio_embeddings.weight"), h0, m.args.audio_vocab_size)
        return h0

    def _prompt_forward(self, b, tokens, masks, B, S, save, **kw):
        """The training forward of the backbone over prompt-side positions, with the adapters generation applies to row ``b``:
        its own bank adapter, or the model's live ones."""
        m = self.e.m
        h0 = self._embed(tokens, masks)
        with (row_lora(m, self.adapters[b]) if self.adapters is not None else generation_lora(m)):
            return self.e.backbone.forward(h0, B, S, save, **kw)

    def prefill(self, tokens, masks):
        e, m = self.e, self.e.m
        if self.adapters is not None:                        # (per-row adapters: every row's prefill with its own adapter)
            return self.prefill_ragged(list(tokens), list(masks))
        B, S, K1 = tokens.shape
        if S > m.bb.max_seq_len:
            raise ValueError("prompt longer than max_seq_len")
        hidden = self._prompt_forward(0, tokens, masks, B, S, True)
        self.bb.fill_from(e.backbone.acts, B, S)
        e.backbone.acts = []
        self.bb.pos.fill_(S - 1)
        self.row_pos[:] = [S - 1] * B
        return hidden.view(B, S, -1)[:, -1, :].contiguous()

    def append(self, tokens, masks):
        """Feed n more positions ([n, K+1] or [1, n, K+1] frames) after the ``cur + 1`` the caches hold - the next turn of a
        conversation: the training forward's kernels for the n rows, with every layer's attention running against the state's own
        caches (``ops.attn_append``: the rows' K / V are appended, nothing is prefilled again).  Returns the last position's hidden
        row [1, d] for ``Engine._frame_tail``, as ``prefill`` does.  Adapters apply as in ``prefill`` (live ``model.lora``, or
        the state's own bank adapter).  The captured frame graph reads the position from device memory and stays valid."""
        m = self.e.m
        if self.B != 1:
            raise ValueError(f"append takes a one-sequence state (this one has {self.B} rows)")
        if self.cur < 0:
            raise RuntimeError("append needs a prefilled state (prefill the first turn)")
        n, pos0 = tokens.numel() // tokens.shape[-1], self.cur + 1
        if n < 1:
            raise ValueError("append needs at least one position")
        if pos0 + n > m.bb.max_seq_len:
            raise ValueError("sequence exceeds max_seq_len")
        pos = torch.arange(pos0, pos0 + n, dtype=torch.int32, device=m.device)
        hidden = self._prompt_forward(0, tokens, masks, 1, n, False, pos=pos, append=(self.bb, 0, pos0))
        self.bb.pos.fill_(pos0 + n - 1)
        self.row_pos[0] = pos0 + n - 1
        return hidden[-1:].contiguous()

    def append_rows(self, rows, tokens_list, masks_list):
        """``append`` for rows of a multi-row state: feed each listed row b its new positions ([n_b, K+1] frames) after the
        ``row_pos[b] + 1`` it holds - the next turns of conversations that share a running batch (csm/serving.py).  Segments whose
        rows share a bank adapter (or have none) are stacked into ONE backbone forward (``_Stack.forward``, ragged ``append``:
        the weights are walked once for all of them); rows with different adapters take one forward per adapter (``row_lora``
        is one adapter per forward).  A row that holds nothing (``row_pos[b] == -1``) is refused: first turns go through
        ``prefill_row``.  Returns the segments' last hidden rows [R, d] in the order of ``rows``.  A segment's bits do not depend
        on what is stacked with it; one segment on a one-row state equals ``append``."""
        m = self.e.m
        rows = list(rows)
        R = len(rows)
        if not (1 <= R <= 16 and len(tokens_list) == R and len(masks_list) == R):
            raise ValueError(f"append_rows takes 1..16 rows with one token and one mask tensor each (got {R} rows)")
        rows = self._distinct_rows(rows, "append_rows")
        K1 = tokens_list[0].shape[-1]
        tks = [t.reshape(-1, K1).to(device=m.device, dtype=torch.int64) for t in tokens_list]
        mks = [k.reshape(-1, K1).to(device=m.device, dtype=torch.uint8) for k in masks_list]
        held = [self.row_pos[b] for b in rows]
        ns, pos0s = [t.shape[0] for t in tks], [h + 1 for h in held]
        for b, h, n in zip(rows, held, ns):
            if h < 0:
                raise RuntimeError(f"append_rows: row {b} holds nothing (a first turn goes through prefill_row)")
            if n < 1:
                raise ValueError("append_rows needs at least one position per row")
            if h + 1 + n > m.bb.max_seq_len:
                raise ValueError("sequence exceeds max_seq_len")
        groups = {}                                              # adapter identity -> segment indices, in order
        for j, b in enumerate(rows):
            groups.setdefault(id(self.adapters[b]) if self.adapters is not None else None, []).append(j)
        last = [None] * R
        for idx in groups.values():
            # (host integers only: one arange per segment)
            pos = torch.cat([torch.arange(pos0s[j], pos0s[j] + ns[j], dtype=torch.int32, device=m.device) for j in idx])
            seg = (self.bb, [rows[j] for j in idx], [pos0s[j] for j in idx], [ns[j] for j in idx])
            hidden = self._prompt_forward(rows[idx[0]], torch.cat([tks[j] for j in idx]), torch.cat([mks[j] for j in idx]), 1,
                                          pos.shape[0], False, pos=pos, append=seg)
            end = 0
            for j in idx:
                end += ns[j]
                last[j] = hidden[end - 1]
        for b, p0, n in zip(rows, pos0s, ns):
            self.bb.pos[b] = p0 + n - 1
            self.row_pos[b] = p0 + n - 1
        return torch.stack(last).contiguous()

    # ---- the checks of the methods that move histories between rows ------------------------------------------------------------
    def _row(self, b) -> int:
        b = int(b)
        if not 0 <= b < self.B:
            raise ValueError(f"row {b} out of range (the state has {self.B})")
        return b

    def _distinct_rows(self, rows, what: str):
        rows = [int(b) for b in rows]
        if len(set(rows)) != len(rows) or any(not 0 <= b < self.B for b in rows):
            raise ValueError(f"{what}: rows must be distinct rows of 0..{self.B - 1}, got {rows}")
        return rows

    def _check_parked(self, parked, what: str, fits: bool = True) -> int:
        """The length of ``parked``, a parked history of this backbone (``park_row``'s format; ``fits``: one a row can hold)."""
        kv = self.bb.kv
        if parked.dim() != 5 or parked.shape[:3] != (kv.shape[0], 2, kv.shape[3]) or parked.shape[4] != kv.shape[5] or \
                parked.dtype != kv.dtype or (fits and not 1 <= parked.shape[3] <= kv.shape[4]):
            raise ValueError(f"{what}: {tuple(parked.shape)} {parked.dtype} is not a parked history of this model's backbone")
        return parked.shape[3]

    def park_row(self, b, length: int):
        """The K / V of positions 0 .. length-1 of row ``b`` in every backbone layer, as one contiguous tensor
        [layers, 2, KV, length, hd] (one strided copy of the stack's cache allocation) - what a conversation keeps while it holds
        no slot.  The depth decoder's cache is per frame and needs nothing."""
        b, length = self._row(b), int(length)
        if not 1 <= length <= self.row_pos[b] + 1:
            raise ValueError(f"park_row: {length} positions of row {b}, which holds {self.row_pos[b] + 1}")
        return self.bb.kv[:, :, b, :, :length].contiguous()

    def resume_row(self, b, parked):
        """Copy a parked history (``park_row``, of this or another row, or of another state of the same model) into row ``b`` from
        position 0 (one strided copy) and set the row's device position and host mirror to its last position."""
        b, length = self._row(b), self._check_parked(parked, "resume_row")
        self.bb.kv[:, :, b, :, :length].copy_(parked)
        self.bb.pos[b] = length - 1
        self.row_pos[b] = length - 1

    def fork_rows(self, rows, parkeds):
        """``resume_row`` for several rows at once: each ``parkeds[r]`` into row ``rows[r]`` from position 0, the rows' device
        positions and host mirrors to their last positions - ONE launch (``ops.kv_fork_rows``) instead of a strided copy and a
        position write per row.  The same parked history may be given for several rows - one voice forked into many requests
        (csm/serving.py) - and none is written.  Leaves the caches, ``bb.pos`` and ``row_pos`` in the state the R ``resume_row``
        calls leave, bit for bit."""
        rows, parkeds = list(rows), list(parkeds)
        R = len(rows)
        if not (1 <= R <= 16 and len(parkeds) == R):
            raise ValueError(f"fork_rows takes 1..16 rows with one parked history each (got {R} rows, {len(parkeds)} histories)")
        rows = self._distinct_rows(rows, "fork_rows")
        for parked in parkeds:
            self._check_parked(parked, "fork_rows")
        ops.kv_fork_rows([p.contiguous() for p in parkeds], self.bb.kv, self.bb.pos, rows)
        for b, parked in zip(rows, parkeds):
            self.row_pos[b] = parked.shape[3] - 1

    def park_rows(self, rows):
        """Take up to 16 distinct prefilled rows out of the batch in the middle of their utterances: one ``ParkedRow`` each - the
        K / V of all ``row_pos[b] + 1`` positions the row holds (ONE ``ops.kv_park_rows`` launch for all rows, ``park_row``'s
        format), at the levels that keep rings the row's ring of sampled codes and its frame counter (ONE
        ``ops.sample_hist_move_rows`` launch, a slice of one packed buffer), and the row's noise generator, which leaves
        ``row_gen``.  The caches, positions and rings are only read: the rows stay as they are until something else is written
        there.  Adapter, sampling parameters and the last sampled frame are the caller's to keep."""
        rows = list(rows)
        if not 1 <= len(rows) <= 16:
            raise ValueError(f"park_rows takes 1..16 rows, got {len(rows)}")
        rows = self._distinct_rows(rows, "park_rows")
        if any(self.row_pos[b] < 0 for b in rows):
            raise ValueError(f"park_rows: row {next(b for b in rows if self.row_pos[b] < 0)} holds nothing")
        kvs = ops.kv_park_rows(self.bb.kv, rows, [self.row_pos[b] + 1 for b in rows])
        packed = self.sampler.park_history(rows)
        return [ParkedRow(kv, None if packed is None else packed[r], self.row_gen.pop(b, None)) for r, (b, kv) in enumerate(zip(rows, kvs))]

    def resume_rows(self, rows, parked):
        """``park_rows``' results into the rows ``rows`` (any rows, of this or another state of the same model at the same
        level): ONE ``fork_rows`` for the K / V, the device positions and the host mirrors; at the levels that keep rings ONE
        ring move towards the state, which restores the rows' frame counters; the generators through ``set_row_seed(generator=)``
        (a row parked without one returns to the whole-buffer draw).  No buffer a captured frame reads changes address and the
        level does not move: nothing recaptures."""
        rows, parked = [int(b) for b in rows], list(parked)
        if len(parked) != len(rows):
            raise ValueError(f"resume_rows: {len(parked)} parked rows for {len(rows)} rows")
        if self.sampler.keeps_history and any(p.hist is None for p in parked):
            raise ValueError("resume_rows: a row parked without its ring of sampled codes (a state below the processed level) "
                             "into a state that keeps rings")
        self.fork_rows(rows, [p.kv for p in parked])
        if self.sampler.keeps_history:
            self.sampler.resume_history(rows, torch.stack([p.hist for p in parked]))
        for b, p in zip(rows, parked):
            self.set_row_seed(b, None, generator=p.gen)

    def shift_parked(self, parked, keep: int, drop: int):
        """A parked history (``park_row``) without its positions ``keep .. keep+drop-1``: a new tensor of ``length - drop``
        positions whose keys behind the gap are rotated back by ``drop`` positions (``ops.kv_shift``, one launch) - the context
        shift that lets a conversation forget turns without prefilling the kept ones again.  Touches nothing of the state."""
        keep, drop, length = int(keep), int(drop), self._check_parked(parked, "shift_parked", fits=False)
        if not (drop >= 1 and keep >= 0 and keep + drop <= length and length - drop >= 1):
            raise ValueError(f"shift_parked: keep {keep} + drop {drop} of {length} positions (at least one is dropped and one is left)")
        return ops.kv_shift(parked.contiguous(), self.e.m.rope_table("backbone"), keep, drop)

    def shift_row(self, b, keep: int, drop: int):
        """Row ``b`` forgets its positions ``keep .. keep+drop-1``: ``park_row`` of all it holds, ``shift_parked``, ``resume_row``
        (which sets the device position and the host mirror to the new last position).  The other rows, the depth decoder's
        caches and the captured frame graph are not touched."""
        b = self._row(b)
        self.resume_row(b, self.shift_parked(self.park_row(b, self.row_pos[b] + 1), keep, drop))

    def truncate(self, length: int):
        """Forget every position from ``length`` on (1 <= length <= cur + 1): every row's device position and host mirror move
        back to ``length - 1``.  Nothing is cleared - cache rows past the position are never read and the next step overwrites them."""
        length = int(length)
        if not 1 <= length <= self.cur + 1:
            raise ValueError(f"truncate to {length} positions: the caches hold {self.cur + 1}")
        self.bb.pos.fill_(length - 1)
        self.row_pos[:] = [length - 1] * self.B

    def prefill_ragged(self, tokens_list, masks_list):
        """Prompts of different lengths, one per batch row: each is prefilled on its own ([1, S_b] through the training
        forward) into its row of the caches; positions are per row from then on (``pos`` is a device vector)."""
        last = [self.prefill_row(b, tk, mk) for b, (tk, mk) in enumerate(zip(tokens_list, masks_list))]
        return torch.stack(last).contiguous()

    def prefill_row(self, b, tk, mk):
        """Prefill ONE row of a live state with a prompt ([S, K+1] tokens and mask) while the other rows keep what they hold:
        the training forward for [1, S] (with the row's own adapter), its K / V rows into row ``b`` of the caches from position
        0, the row's device position and host mirror to S - 1.  Returns the last position's hidden row [d]."""
        e, m = self.e, self.e.m
        b = self._row(b)
        S = tk.shape[0]
        if S > m.bb.max_seq_len:
            raise ValueError("prompt longer than max_seq_len")
        hidden = self._prompt_forward(b, tk, mk, 1, S, True)
        self.bb.fill_row(e.backbone.acts, b, S)
        e.backbone.acts = []
        self.bb.pos[b] = S - 1
        self.row_pos[b] = S - 1
        return hidden[-1]

    # ---- slot lifecycle: rows that join, idle and leave independently (csm/serving.py) ---------------------------------------
    def set_row_adapter(self, b, state):
        """Give row ``b`` the bank adapter ``state`` (None = no adapter) from its next prefill / frame on: one int written to
        ``row_adapter[b]`` on the device, which the per-row adapter kernels read.  ``state`` must be one of the adapters bound at
        creation (``bank``): the pointer tables and the adapter count are part of the captured graph."""
        if state is None:
            idx = -1
        else:
            idx = next((j for j, s in enumerate(self.bank or []) if s is state), None)
            if idx is None:
                raise ValueError("set_row_adapter: this adapter was not bound when the state was created (adapters added to the "
                                 "bank later need a new state)")
        if self.adapters is None:
            return                                   # (no bank: only None gets here)
        self.adapters[b] = state
        for stack in (self.bb, self.dc):
            if stack.lora_rows is not None:
                stack.lora_rows[0][b:b + 1].fill_(idx)

    # ---- per-row sampling: thin names over ``self.sampler`` (csm/sampling.py: the levels, the buffers, the one writer) ----------
    def set_row_sampling(self, b, temperature, topk):
        """Row ``b`` samples with ``temperature`` / ``topk`` from its next frame on, in every frame body called with
        ``temperature=None, topk=None`` (level 1: the rows sampler).  The first call gives its pair to every row."""
        self.sampler.write(b, 1, temperature, topk)

    def set_row_filters(self, b, top_p, min_p):
        """... and with the nucleus ``top_p`` and the min-p threshold ``min_p`` (level 2: the filtered rows sampler; after
        ``set_row_sampling``).  The call that raises the level gives its two to every row: make it before the first capture."""
        self.sampler.write(b, 2, top_p, min_p)

    def set_row_processors(self, b, temperature, topk, top_p, min_p, repetition_penalty, repetition_window):
        """... with these six, each a number (every codebook) or K numbers (one per codebook) (level 3: the processed rows
        sampler, which keeps the rows' rings of sampled codes).  The call that raises the level gives its six to every row."""
        self.sampler.write(b, 3, temperature, topk, top_p, min_p, repetition_penalty, repetition_window)

    def set_row_typical(self, b, temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p):
        """... with these seven, each a number or K numbers: the six of ``set_row_processors`` and ``typical_p`` in (0, 1], locally
        typical sampling as the last filter (level 4: the typical rows sampler; 1.0 is the processed sampler's draw).  The call
        that raises the level gives its seven to every row."""
        self.sampler.write(b, 4, temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p)

    def reset_row_history(self, b):
        """Row ``b`` starts an utterance: its frame counter returns to 0.  The ring is left as it is - the sampler looks at
        min(window, frame) entries, so what an earlier utterance left there is never read."""
        self.sampler.reset_history(b)

    def set_live(self, rows):
        """The rows whose draws count in the next frame tail (the processed sampler writes their ring and advances their frame);
        the others' rings and counters stay as they are, whatever their rows of the batch hold.  Nothing below level 3."""
        self.sampler.set_live(rows)

    def sampling_args(self, temperature, topk, top_p=None, min_p=None, repetition_penalty=None, repetition_window=None,
                      typical_p=None):
        """What ``Engine.generate_frame`` / ``generate_first_frames`` hand to the frame bodies: two numbers (or None, None) with
        nothing else named pass through; anything else (``sampling.normalise``: a value per row, ``top_p`` / ``min_p``, a penalty,
        a window, values per codebook, ``typical_p``) is written to the rows at the level it needs and (None, None) comes back."""
        return self.sampler.args(temperature, topk, top_p, min_p, repetition_penalty, repetition_window, typical_p)

    row_sampling = property(lambda self: self.sampler.row_sampling, doc="[(temperature, topk)] * B at levels 1 and 2, else None")
    row_filters = property(lambda self: self.sampler.row_filters, doc="[(top_p, min_p)] * B at level 2, else None")
    row_processors = property(lambda self: self.sampler.row_processors, doc="six K-tuples per row at level 3, else None")
    row_typical = property(lambda self: self.sampler.row_typical, doc="seven K-tuples per row at level 4, else None")

    def set_row_seed(self, b, seed, generator=None):
        """Row ``b``'s sampler noise comes from its own ``torch.Generator`` seeded with ``seed`` (``fill_noise``); None returns
        the row to the whole-buffer draw from torch's global generator.  ``generator``: an existing generator to draw from
        instead of a fresh one - a conversation's, which travels with it from slot to slot (``new_row_generator``)."""
        if generator is not None:
            self.row_gen[b] = generator
        elif seed is None:
            self.row_gen.pop(b, None)
        else:
            self.row_gen[b] = self.new_row_generator(seed)

    def new_row_generator(self, seed):
        """A generator of the kind ``set_row_seed`` makes, for a caller that keeps it across rows (``set_row_seed(generator=)``)."""
        g = torch.Generator(device=self.noise_buf.device)
        g.manual_seed(int(seed))
        return g

    def set_active(self, rows):
        """The rows that advance in the following ``serve_frame`` calls; the others idle: their position is pinned (to 0, then the
        frame's increment: they attend to two positions of their own row) and their output is meaningless."""
        rows = sorted(int(b) for b in rows)
        if any(not 0 <= b < self.B or self.row_pos[b] < 0 for b in rows):
            raise ValueError(f"set_active: rows must be prefilled rows of 0..{self.B - 1}, got {rows}")
        if self.active is None:
            self.active = torch.ones(self.B, dtype=torch.int32, device=self.bb.pos.device)
        if rows != self.active_rows:
            # (a blocking copy: the host list is a temporary, and the set changes at chunk boundaries and length limits only)
            self.active.copy_(torch.tensor([1 if b in rows else 0 for b in range(self.B)], dtype=torch.int32))
        self.active_rows = rows

    def serve_first(self, last_h, rows, temperature, topk):
        """The first frame of the rows just prefilled (``last_h`` [B, d]: their ``prefill_row`` results in their rows, anything in
        the others) - ``Engine._frame_tail`` over the whole batch, with per-row noise drawn for ``rows`` only.  [B, K]; the other
        rows' output is meaningless.  ``temperature`` / ``topk``, here and in ``serve_frame``: two numbers, or None, None for each
        row's own pair (``set_row_sampling``)."""
        self.draw_rows = set(rows)
        self.set_live(rows)                              # (the other rows are mid-utterance: this tail must not count for them)
        try:
            return self.e._frame_tail(self, last_h, temperature, topk, None)
        finally:
            self.draw_rows = None

    def serve_frame(self, tokens, masks, temperature, topk):
        """One decode frame in which only the active rows (``set_active``) advance.  The position increment sits inside the captured
        frame graph, so the idle rows are pinned outside it, before the replay: ``pos *= active`` (one small launch).  The caller
        feeds idle rows zero tokens.  Returns [B, K]; idle rows' output is meaningless."""
        m = self.e.m
        if self.active is None:
            self.set_active(self.active_rows)
        self.bb.pos.mul_(self.active)
        self.set_live(self.active_rows)
        self.draw_rows = set(self.active_rows)
        try:
            if getattr(m, "use_hip_graph", True):
                return self.graph_frame(tokens, masks, temperature, topk)
            self._advance()
            return self.e._decode_frame(self, tokens, masks, temperature, topk, None)
        finally:
            self.draw_rows = None

    def backbone_step(self, tokens, masks):
        self._embed(tokens, masks, out=self.h0)                 # (the persistent buffer: a captured graph reads it)
        self.bb.pos.add_(1)
        return self.bb.step(self.h0)

    def graph_frame(self, tokens, masks, temperature, topk, noise=None):
        """Replay one decode frame (~1.8 k kernel launches) as a single HIP graph.  The first decode frame runs eagerly
        (warm-up: lazy function attributes, allocator), the second is captured, later ones are replays; positions, input
        tokens and the frame's noise live in persistent device buffers, so the same graph serves every frame.  Re-captured
        when temperature / top-k change; with ``None, None`` the key is (None, None) and the sampler reads each row's pair from
        the row buffers (``set_row_sampling``), so a change of any row's parameters replays the same graph; once the state has
        row filters (``set_row_filters``) it is (None, None, "filters") - the frame holds the filtered rows sampler, and a change
        of any row's top-p / min-p replays it too; with row processors (``set_row_processors``) it is (None, None, "processors"), with
        typical sampling (``set_row_typical``) (None, None, "typical"); in statistics mode (``enable_stats``) every key ends with
        "stats"."""
        m = self.e.m
        self._advance()
        key = self.sampler.graph_key(temperature, topk)
        if self.graph is None or self.graph_key != key:
            if self.warm < 1 or self.graph_key not in (None, key):
                self.warm, self.graph, self.graph_key = 1, None, None
                return self.e._decode_frame(self, tokens, masks, temperature, topk, noise)
            self.in_tok = tokens.to(torch.int64).clone()
            self.in_msk = masks.to(torch.uint8).clone()
            self.fill_noise(noise)
            torch.cuda.synchronize()
            _prime_graph_rng(m.device)
            g = torch.cuda.CUDAGraph()
            # No cyclic garbage collection while the stream is capturing: a collection that happens to run inside the ~700
            # launches may finalise objects whose destructors call the runtime (an older model's captured graph, events) - not
            # allowed during capture, the process aborts (seen once a test run's allocation pattern moved a collection in
            # there).  torch.cuda.graph() collects before it starts capturing; reference-counted frees are unaffected.
            import gc
            gc_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    self.out_static = self.e._decode_frame_body(self, self.in_tok, self.in_msk, temperature, topk)
            finally:
                if gc_on:
                    gc.enable()
            self.graph, self.graph_key = g, key
            g.replay()
            return self.out_static.clone()
        self.in_tok.copy_(tokens)
        self.in_msk.copy_(masks)
        self.fill_noise(noise)
        self.graph.replay()
        return self.out_static.clone()

    def decoder_reset(self):
        pass   # positions restart at 0 every frame; stale cache rows beyond the current position are never read

    def decoder_step(self, x_in, i, code=None, final_norm=True):
        """Decoder position i.  Input = ``x_in`` [B, d] (the backbone state, i = 0) or, with ``code`` (int32 [B] on the
        device), the audio embedding of code i-1 gathered inside the projection product (model.py:189-191)."""
        m = self.e.m
        if code is None:
            ops.gemv(x_in.contiguous(), m.block("projection.weight"), self.proj)
        else:
            ops.gemv_ex(m.block("audio_embeddings.weight"), m.block("projection.weight"), self.proj, row_index=code,
                        row_offset=(i - 1) * m.args.audio_vocab_size)
        self.dc.pos = self.dpos[i]
        self.dc.pos_host = i if DECODE_POS_HOST else None
        return self.dc.step(self.proj, final_norm=final_norm)
