"""A float64 reference of a WHOLE generated frame (``DecodeState.prefill_ragged`` / ``backbone_step`` -> ``Engine._frame_tail_body``
-> ``DecodeState.decoder_step``: the wiring of the decode kernels, not the kernels - those have pins of their own), an emulation of
the frame's bf16 stores, a per-vector judge, the cases of every decode mode and a catalogue of seeded wiring faults.
test_gen_frame_ref_cpu.py proves this module (against the oracle, against itself, and that every fault is caught);
test_gen_frame_logits_gpu.py judges the engine by it.

Plain torch on the CPU, seeded, the same on every machine.  ``_run`` restates a prefill of ragged prompts followed by F
teacher-forced decode frames in its own text, in whatever dtype the weights have (float64 everywhere but the oracle comparison,
which runs it in fp32).  Weights are what the device holds: the bf16 values widened; in FP8 mode ``scale[n] * decoded code`` for
exactly the weights ``_DecodeStack.attach_fp8`` quantises (q / k / v / w1 / w3 / w2 of both stacks, and the output projection
except the depth decoder's at B = 1, whose fused attention product keeps bf16) - the prompt forward stays on the bf16 weights.
Adapters: live ones (``attach_lora``: one scale) or one per row (``attach_lora_rows``: an adapter or none per row, each with its
own scale and bias), on both stacks, restated per module (the fused row orders q | k | v and interleaved w1 / w3 are the engine's
layout; faults 15 and 16 below build them on purpose).

Teacher forcing.  ``inputs(case)["forced"]`` [F, K, B] are the codes fed forward: codebook i's embedding in the depth decoder and
the next frame's backbone input come from them, not from a sample, so every logits vector is a pure function of the case.  The
values are distinct across rows and codebooks of a frame where K B <= V; at B = 16 (128 codes, V = 67) they are distinct across the
rows of a codebook and across the codebooks of a row.

Evaluations of a ``Case`` (each a ``Result``: logits [F, K, B, V]; kv [F, layers, 2, B, KV, S_KEEP, hd], the backbone cache after
every frame; pos [F, B], the backbone position of every row after every frame):
  frame64(case)               exact arithmetic, float64.
  frame_emulated(case, seed)  the same with a rounding wherever the engine stores or rounds to bf16.  seed None: nearest even; an
                              integer: stochastic rounding (train_step_ref.Rounder).
  judge(got, x64, emu, case)  every logits vector and every K or V row a frame wrote (the prefill's rows with frame 0):
                                ratio = |got - x64|_2 / max(|emu - x64|_2, 2^-10 |x64|_2)
                              and the exact conditions: positions equal the reference's; cache slots past a row's position are
                              the zeros they were created as; slots below the written one are bit-unchanged by the frame; an idle
                              row (below); the SET of decode-step weights held as e4m3 codes is the reference's (FP8 mode).  Prints ``RATIO <case> <frame> <codebook> <worst over rows>``.

Idle rows (``serve_idle_b4``).  ``DecodeState.serve_frame`` pins an idle row's DEVICE position to 0 before the frame's increment
and the frame writes a zero token's K / V at slot 1 of that row (engine.py ``set_active`` / ``serve_frame``, csm/serving.py module
docstring: "harmless for a row that is free, fatal for a history").  The condition judged is therefore the engine's contract,
stated exactly: an idle row's device position is IDLE_PIN = 1, its host mirror ``row_pos`` is unchanged (the GPU test), every
cache slot of it but slot 1 is bit-unchanged, and its logits are not judged (the contract calls them meaningless).

Hooks (``R``), with the line of csm/engine.py (E), the contract line of decode_gemv_ref.py (G) / decode_attn_ref.py (A), or the
hook of train_step_ref.py (T) each mirrors.  The fp32 logits (E919, E929, E970, E993) are never rounded.
  prompt side (``_prompt_stack``: forward values of T's hooks; E204-291)
    h0            E1355 embed_fwd (T h0)
    xn, hn        E232, E259 (T xn, hn)
    q, k          prefill has pos None: RoPE in the projection's epilogue, ONE rounding after the rotation (E234-237, E164-165, T "q, k
                  fused") - also with a fused adapter group.  A group with a bias takes the per-adapter path and the stand-alone
                  RoPE kernel: rounded before AND after the rotation (E167-178, E238).  v: one rounding.
    adapters      fused (no bias): tx = bf16(s x At), then one product (E164-165, T "LoRA tx").  With a bias (lora.py forward):
                  y = bf16(base), t = bf16(x A^T), y = bf16(y + s t B^T), y = bf16(y + bias); on w1 / w3 through a zeroed tmp
                  that is then added into the stored gate | up (E167-178), and SwiGLU reads the ROUNDED gate | up.
    P, o          P rounded before the PV product (T ``_Attn``), o E239-245
    h, out        one rounding of product + residual E255-256, E280-281
    act           from the unrounded gate / up in the fused epilogue (T act)
    xf            E286-288: the row ``_frame_tail_body`` reads as last_h
  decode side (``_decode_step``: E1069-1096)
    h0            E1668 embed_fwd into the persistent buffer
    x^            G "RMSNorm prologue": bf16(x rstd w) of every product with a norm prologue (E1080, E1089), the head product on
                  the un-normed decoder residual included (E929)
    qkv           G plain: one rounding (E1080)
    q, k          rounded before the rotation (they are read from the stored qkv) and once after it (the comment at E989,
                  A ``rotate``); the cache holds the rotated bf16 k, the stored v (A ``ref_decode_attention``)
    o             A ``ref_product``: the attention result rounded to bf16 (fused or not: E1084, E1087)
    h, layer out  G residual: one rounding of product + residual (E1084 / E1088, E1091)
    g, u, act     G SwiGLU: g, u rounded before SiLU, then act (E1089)
    t             G lora_project: t = bf16(scale x^ At) (E1115, E1121); the extension and the bias join the sum BEFORE the
                  epilogue's one rounding (G K-extension; FP8: the scaled base sum, E1117)
    xf            the backbone's final norm is a stored tensor (E1095); the decoder's is folded into the head product (x^ above)
    proj          E1723 / E1725: bf16 (the gathered embedding row is a bf16 value already)
  recompute path (``use_kv_cache = False``, E952-997): the whole history through the prompt-side forward every frame, proj
  E988, the decoder through the training forward with the rotation UN-fused (E991: before and after), xf stored (E286-288).

Record (measured on this module alone; ``measure`` recomputes it and test_gen_frame_ref_cpu.py holds it to these):
  W = worst ratio over every case of CASES, eight stochastic draws, every vector, each draw judged against frame64 with the
      nearest-even draw as x_emu.  L = 2 W: the factor is for what the emulation leaves out - summation orders, fp32
      accumulation, approximated exp / rsqrt.  L is never raised to fit the GPU.
  See W_RECORDED / L below and RECORD at the end of this docstring.

RECORD
%(record)s
"""
import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import train_step_ref as T
from oracle import csm_oracle as O

F64 = torch.float64
CFG = replace(O.tiny_cfg(), n_codebooks=8)
K, V = CFG.n_codebooks, CFG.audio_vocab
PARAM_SEED = 11
PARAM_STD = 0.06
FRAMES = 5                     # the tail after the prefill, the eager warm-up, the captured frame and two replays
S_KEEP = 32                    # cache slots a Result keeps (prompts are 5..19 long, five frames); the GPU test holds the rest to zero
IDLE_PIN = 1
TEMP, TOPK = 0.8, 12           # the engine tests' sampling parameters (the old criteria)
SEEDS = tuple(range(8))
ALL7 = ("q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3")

W_RECORDED = 3.63              # measured 3.6215 on 2026-10-20 (its worst case: rows_b16), written rounded up
L = 2 * W_RECORDED             # 7.26


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Adapter:
    modules: Tuple[str, ...] = ALL7
    r: int = 8
    alpha: float = 16.0
    bias: bool = False
    seed: int = 1

    @property
    def scaling(self):
        return self.alpha / self.r


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    seed: int
    frames: int = FRAMES
    fp8: bool = False
    live: Optional[Adapter] = None                    # model.lora, un-merged
    bank: Tuple[Adapter, ...] = ()                    # per-row adapters ...
    rows: Optional[Tuple[int, ...]] = None            # ... row b's index into ``bank`` (-1: none)
    kv_cache: bool = True                             # False: the recompute path (rectangular prompts, eager only)
    idle: Tuple[int, ...] = ()                        # rows that idle from frame 1 on (serve_frame)
    sampling: Optional[Tuple[Tuple[float, int], ...]] = None     # (temperature, topk) per row: the rows sampler

    def active(self, f: int) -> List[int]:
        return [b for b in range(self.B) if f == 0 or b not in self.idle]


_A0 = Adapter(seed=1, alpha=16.0)
_A1 = Adapter(seed=2, alpha=4.0, bias=True)
_ROWS16 = (0, -1, 1, 0, 1, 1, -1, 0, -1, 0, 0, 1, 1, -1, 0, 1)
CASES: Dict[str, Case] = {c.name: c for c in (
    Case("plain_b1", 1, 31),
    Case("plain_b3", 3, 32),
    Case("plain_b16", 16, 33),
    Case("recompute_b2", 2, 34, frames=2, kv_cache=False),
    Case("fp8_b1", 1, 35, fp8=True),
    Case("fp8_b4", 4, 36, fp8=True),
    Case("live_qv_b1", 1, 37, live=Adapter(("q_proj", "v_proj"), seed=3)),
    Case("live_all7_bias_b2", 2, 38, live=Adapter(ALL7, r=8, bias=True, seed=4)),
    Case("live_mlp_r4_b4", 4, 39, live=Adapter(("w1", "w2", "w3"), r=4, alpha=8.0, seed=5)),
    Case("rows_b4", 4, 40, bank=(_A0, _A1), rows=(0, -1, 1, 0)),
    Case("rows_b16", 16, 41, bank=(_A0, _A1), rows=_ROWS16),
    Case("fp8_rows_b4", 4, 42, fp8=True, bank=(_A0, _A1), rows=(0, -1, 1, 0)),
    Case("serve_idle_b4", 4, 43, idle=(1, 3), sampling=((0.8, 12), (1.0, 5), (0.6, 30), (0.9, 1))),
)}


def params(dtype=F64, seed: int = PARAM_SEED) -> Dict[str, torch.Tensor]:
    """The tiny 8-codebook model's weights as the GPU holds them: bf16 values, widened.  Matrices N(0, PARAM_STD) - about
    1 / sqrt(d), so that a layer's products weigh as much as the residual they join - and norm scales 1 + 0.25 N(0, 1) instead of
    the initialiser's ones: with ones a norm applied twice is the norm applied once, and fault 6 would be invisible."""
    g = torch.Generator().manual_seed(seed + 1)
    out = {}
    for k, v in O.init_params(CFG, seed=seed, std=PARAM_STD).items():
        if k.endswith(".scale"):
            v = 1.0 + 0.25 * torch.randn(v.shape, generator=g)
        out[k] = v.to(torch.bfloat16).to(dtype)
    return out


def make_adapter(ad: Adapter, dtype=F64) -> Dict[str, torch.Tensor]:
    """{name.lora_A [r, in], name.lora_B [out, r], name.lora_bias [out]} of both stacks under LoRAState.named_tensors' names,
    bf16 values widened, B (and the bias) non-zero.  The GPU test copies these very values into the model's adapters."""
    shapes = O.param_shapes(CFG)
    g = torch.Generator().manual_seed(7000 + ad.seed)
    out = {}
    for prefix, c in (("backbone", CFG.backbone), ("decoder", CFG.decoder)):
        for i in range(c.n_layers):
            for mod in ad.modules:
                name = f"{prefix}.layers.{i}.{'attn' if mod.endswith('proj') else 'mlp'}.{mod}"
                out_f, in_f = shapes[f"{name}.weight"]
                out[f"{name}.lora_A"] = (torch.randn(ad.r, in_f, generator=g) / math.sqrt(in_f)).to(torch.bfloat16).to(dtype)
                out[f"{name}.lora_B"] = (torch.randn(out_f, ad.r, generator=g) * 0.05).to(torch.bfloat16).to(dtype)
                if ad.bias:
                    out[f"{name}.lora_bias"] = (torch.randn(out_f, generator=g) * 0.05).to(torch.bfloat16).to(dtype)
    return out


def inputs(case: Case) -> dict:
    """tokens / masks: B prompts [S_b, K+1] (ragged, 5..19 long; one length for the recompute path, whose history is one
    rectangular tensor); forced [F, K, B] int64; noise [F, K, B, V] fp32 Exp(1) (the sampler check and the old criteria)."""
    g = torch.Generator().manual_seed(900 + case.seed)
    tokens, mask, _ = O.synthetic_batch(CFG, case.B, 20, seed=case.seed)
    lens = torch.randint(5, 20, (case.B,), generator=g).tolist()
    if not case.kv_cache:
        lens = [lens[0]] * case.B
    forced = torch.empty(case.frames, K, case.B, dtype=torch.int64)
    for f in range(case.frames):
        if K * case.B <= V:
            forced[f] = torch.randperm(V, generator=g)[:K * case.B].view(K, case.B)
        else:                                      # 17 i mod 67 is distinct for i < 8: distinct down every column and along every row
            p = torch.randperm(V, generator=g)[:case.B]
            forced[f] = (p[None, :] + 17 * torch.arange(K)[:, None]) % V
    noise = torch.empty(case.frames, K, case.B, V).exponential_(1, generator=g)
    return dict(tokens=[tokens[b, :lens[b]] for b in range(case.B)], masks=[mask[b, :lens[b]] for b in range(case.B)], lens=lens,
                forced=forced, noise=noise)


# ------------------------------------------------------------------------------------------------------------ weights
def quantise_rows(W: torch.Tensor):
    """include/csm_hip.h csm_quantize_rows_fp8 restated: per row scale = amax / 448 in fp32 (1 for a zero row), code =
    e4m3fn(clamp(w / scale)) to nearest even.  -> (decoded codes fp32 [N, K], scale fp32 [N])."""
    w = W.float()
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (w / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float(), scale


def decode_weights(P, case: Case, fault: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The layer products' weights of the one-position steps: P's, or in FP8 mode scale[n] * code for what attach_fp8 quantises.
    -> (weights, the names quantised)."""
    Wd = {k: v for k, v in P.items() if ".layers." in k and k.endswith(".weight")}
    if not case.fp8:
        return Wd, frozenset()
    done = set()
    dt = P["projection.weight"].dtype
    for name in list(Wd):
        if name.endswith("output_proj.weight") and name.startswith("decoder.") and case.B == 1 and fault != "fp8_b1_out_proj_quantised":
            continue                                                   # the fused attention + output projection keeps bf16
        q, s = quantise_rows(Wd[name])
        Wd[name] = s.to(dt)[:, None] * q.to(dt)
        done.add(name)
    if fault == "fp8_w13_scales_stacked":
        for name in [n for n in Wd if n.endswith("mlp.w1.weight")]:
            n3 = name.replace("w1", "w3")
            (q1, s1), (q3, s3) = quantise_rows(P[name]), quantise_rows(P[n3])
            st = torch.cat([s1, s3]).to(dt)                            # the scales of w1 | w3 read in the interleaved row order
            Wd[name], Wd[n3] = st[0::2, None] * q1.to(dt), st[1::2, None] * q3.to(dt)
    return Wd, frozenset(done)


def _group_mods(mod: str):
    return {"q_proj": ("q_proj", "k_proj", "v_proj"), "k_proj": ("q_proj", "k_proj", "v_proj"), "v_proj": ("q_proj", "k_proj", "v_proj"),
            "output_proj": ("output_proj",), "w1": ("w1", "w3"), "w3": ("w1", "w3"), "w2": ("w2",)}[mod]


class _Lo:
    """One adapter as a stack sees it: its tensors, its scale, whether its groups take the per-adapter (bias) path."""

    def __init__(self, spec: Adapter, tensors, scale=None):
        self.spec, self.t, self.s = spec, tensors, spec.scaling if scale is None else scale

    def has(self, name):
        return f"{name}.lora_A" in self.t

    def unfused(self, mod):
        return self.spec.bias and any(m in self.spec.modules for m in _group_mods(mod))


def _row_adapters(case: Case, ads, side: str, prefix: str, fault: Optional[str]) -> List[Optional[_Lo]]:
    """Row b's adapter on ``side`` ('prompt' | 'decode') of stack ``prefix``.  ``ads`` = {'live': tensors} or {'bank': [tensors]}."""
    if case.live is not None:
        lo = _Lo(case.live, ads["live"], 1.0 if (fault == "decoder_lora_scale_one" and side == "decode" and prefix == "decoder") else None)
        if fault == "bias_rows_stacked" and side == "decode" and case.live.bias:
            t = dict(lo.t)
            for n1 in [n for n in t if n.endswith("w1.lora_bias")]:
                n3 = n1.replace("w1", "w3")
                st = torch.cat([t[n1], t[n3]])                         # w1 | w3 stacked, read in the interleaved row order
                t[n1], t[n3] = st[0::2], st[1::2]
            lo = _Lo(case.live, t)
        return [lo] * case.B
    if case.rows is None:
        return [None] * case.B
    rows = list(case.rows)
    if side == "decode":
        if fault == "decoder_adapter_next_row" and prefix == "decoder":
            rows = rows[1:] + rows[:1]
        if fault == "none_row_gets_adapter0":
            rows = [max(a, 0) for a in rows]
    return [None if a < 0 else _Lo(case.bank[a], ads["bank"][a]) for a in rows]


# ------------------------------------------------------------------------------------------------------------ the prompt side
def _attn_prompt(q, k, v, R):
    """q [S, H, hd], k / v [S, KV, hd], causal.  The training kernels' scheme (train_step_ref._Attn.forward)."""
    S, H, hd = q.shape
    rep = H // k.shape[1]
    qh, kh, vh = q.transpose(0, 1), k.repeat_interleave(rep, 1).transpose(0, 1), v.repeat_interleave(rep, 1).transpose(0, 1)
    s = (qh @ kh.transpose(-1, -2) / math.sqrt(hd)).masked_fill(~torch.tril(torch.ones(S, S, dtype=torch.bool)), float("-inf"))
    if not R.on:
        o = torch.softmax(s, dim=-1) @ vh
    else:
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = (R(e) @ vh) / e.sum(-1, keepdim=True)
    return o.transpose(0, 1).reshape(S, H * hd)


def _prompt_stack(P, prefix, c, x, R, lo: Optional[_Lo], fused_rope=True):
    """The training forward of one stack on ONE sequence x [S, d] at positions 0..S-1 -> (xf [S, d], the un-normed residual
    [S, d], per layer the rotated k [S, KV, hd] and v [S, KV, hd])."""
    S = x.shape[0]
    H, KV, hd = c.n_heads, c.n_kv_heads, c.head_dim
    table, pos = T._table(c, x.dtype), torch.arange(S)[None]
    ks, vs = [], []

    def lin(name, inp, res=None):
        y = inp @ P[f"{name}.weight"].t()
        if res is not None:
            y = y + res
        if lo is None or not lo.has(name):
            return y
        A, Bm = lo.t[f"{name}.lora_A"], lo.t[f"{name}.lora_B"]
        if not lo.spec.bias:
            return y + R(lo.s * (inp @ A.t())) @ Bm.t()
        y = R(R(y) + lo.s * (R(inp @ A.t()) @ Bm.t()))
        return R(y + lo.t[f"{name}.lora_bias"])

    def lin13(name, inp):
        """w1 / w3 on the per-adapter path: the adapter's output goes through a zeroed tmp and is added into the stored value."""
        y = R(inp @ P[f"{name}.weight"].t())
        if not lo.has(name):
            return y
        tmp = R(lo.s * (R(inp @ lo.t[f"{name}.lora_A"].t()) @ lo.t[f"{name}.lora_B"].t()))
        return R(y + R(tmp + lo.t[f"{name}.lora_bias"]))

    def rot(y, heads, fused):
        return R(T._rope((y if fused else R(y)).view(1, S, heads, hd), table, pos))[0]

    for i in range(c.n_layers):
        p = f"{prefix}.layers.{i}"
        xn = R(T._rms(x, P[f"{p}.sa_norm.scale"], c.norm_eps))
        fr = fused_rope and not (lo is not None and lo.unfused("q_proj"))
        q = rot(lin(f"{p}.attn.q_proj", xn), H, fr)
        k = rot(lin(f"{p}.attn.k_proj", xn), KV, fr)
        v = R(lin(f"{p}.attn.v_proj", xn)).view(S, KV, hd)
        ks.append(k)
        vs.append(v)
        o = R(_attn_prompt(q, k, v, R))
        h = R(lin(f"{p}.attn.output_proj", o, res=x))
        hn = R(T._rms(h, P[f"{p}.mlp_norm.scale"], c.norm_eps))
        if lo is not None and lo.unfused("w1"):
            g, u = lin13(f"{p}.mlp.w1", hn), lin13(f"{p}.mlp.w3", hn)
        else:
            g, u = lin(f"{p}.mlp.w1", hn), lin(f"{p}.mlp.w3", hn)
        act = R(g * torch.sigmoid(g) * u)
        x = R(lin(f"{p}.mlp.w2", act, res=h))
    return R(T._rms(x, P[f"{prefix}.norm.scale"], c.norm_eps)), x, ks, vs


# ------------------------------------------------------------------------------------------------------------ the decode side
def _decode_step(P, Wd, prefix, c, x, pos, cache, rows, R, los, slot_off=0):
    """One position per row: x [n, d] for the batch rows ``rows`` at positions pos [n] (int64) against cache
    [layers, 2, B, KV, S, hd], which gets the new K / V rows -> the un-normed residual stream [n, d]."""
    n = x.shape[0]
    H, KV, hd = c.n_heads, c.n_kv_heads, c.head_dim
    rep, table = H // KV, T._table(c, x.dtype)

    def lin(name, xh):
        acc = xh @ Wd[f"{name}.weight"].t()
        done = set()
        for j, lo in enumerate(los):
            if lo is None or not lo.has(name) or id(lo) in done:
                continue
            done.add(id(lo))
            idx = [m for m, other in enumerate(los) if other is lo]
            ext = R(lo.s * (xh[idx] @ lo.t[f"{name}.lora_A"].t())) @ lo.t[f"{name}.lora_B"].t()
            if f"{name}.lora_bias" in lo.t:
                ext = ext + lo.t[f"{name}.lora_bias"]
            acc = acc.index_add(0, torch.tensor(idx), ext)
        return acc

    for i in range(c.n_layers):
        p = f"{prefix}.layers.{i}"
        xh = R(T._rms(x, P[f"{p}.sa_norm.scale"], c.norm_eps))
        q, k, v = (R(lin(f"{p}.attn.{m}", xh)) for m in ("q_proj", "k_proj", "v_proj"))
        q = R(T._rope(q.view(n, 1, H, hd), table, pos[:, None]))[:, 0]
        k = R(T._rope(k.view(n, 1, KV, hd), table, pos[:, None]))[:, 0]
        v = v.view(n, KV, hd)
        o = torch.empty(n, H * hd, dtype=x.dtype)
        for j, b in enumerate(rows):
            pj = int(pos[j])
            Kc = torch.cat([cache[i, 0, b, :, :pj], k[j][:, None]], dim=1)            # [KV, pj + 1, hd]
            Vc = torch.cat([cache[i, 1, b, :, :pj], v[j][:, None]], dim=1)
            pr = torch.softmax(q[j].view(KV, rep, hd) @ Kc.transpose(-1, -2) / math.sqrt(hd), dim=-1)
            o[j] = (pr @ Vc).reshape(-1)
            cache[i, 0, b, :, pj + slot_off], cache[i, 1, b, :, pj + slot_off] = k[j], v[j]
        o = R(o)
        h = R(lin(f"{p}.attn.output_proj", o) + x)
        hn = R(T._rms(h, P[f"{p}.mlp_norm.scale"], c.norm_eps))
        g, u = R(lin(f"{p}.mlp.w1", hn)), R(lin(f"{p}.mlp.w3", hn))
        act = R(g * torch.sigmoid(g) * u)
        x = R(lin(f"{p}.mlp.w2", act) + h)
    return x


@dataclass
class Result:
    logits: torch.Tensor                       # [F, K, B, V]
    kv: Optional[torch.Tensor]                 # [F, layers, 2, B, KV, S_KEEP, hd] (None: the recompute path has no cache)
    pos: Optional[torch.Tensor]                # [F, B] int64
    quantised: frozenset = frozenset()         # the decode-step weights held as e4m3 codes (names of the un-fused modules)


def _embed(P, tok, msk, fault=None):
    """tok / msk [S, K+1] -> the masked embedding sum [S, d] (unrounded)."""
    dt = P["projection.weight"].dtype
    e = torch.cat([P["audio_embeddings.weight"][tok[:, :K] + V * torch.arange(K)], P["text_embeddings.weight"][tok[:, K]][:, None]], dim=1)
    m = msk.clone()
    if fault == "text_column_added":
        m[~m[:, K], K] = True                  # (an audio frame's masked-off text column: text token 0)
    return (e * m[:, :, None].to(dt)).sum(1)


def _frame_tokens(codes):
    """codes [n, K] -> the audio frame fed back: tokens [n, K+1] (text column 0), mask [n, K+1] (text column off)."""
    n = codes.shape[0]
    return (torch.cat([codes, torch.zeros(n, 1, dtype=torch.int64)], 1),
            torch.cat([torch.ones(n, K, dtype=torch.bool), torch.zeros(n, 1, dtype=torch.bool)], 1))


def _run(case: Case, R, P=None, ads=None, fault: Optional[str] = None, inp=None) -> Result:
    P = P if P is not None else params()
    dt = P["projection.weight"].dtype
    inp = inp if inp is not None else inputs(case)
    if ads is None:
        ads = adapters(case, dt)
    if not case.kv_cache:
        return _run_recompute(case, R, P, ads, fault, inp)
    Wd, quantised = decode_weights(P, case, fault)
    B, Fn, bb, dc = case.B, case.frames, CFG.backbone, CFG.decoder
    forced = inp["forced"]
    cache = torch.zeros(bb.n_layers, 2, B, bb.n_kv_heads, bb.max_seq_len, bb.head_dim, dtype=dt)
    pos = torch.zeros(B, dtype=torch.int64)
    lo_p = _row_adapters(case, ads, "prompt", "backbone", fault)
    lo_b = _row_adapters(case, ads, "decode", "backbone", fault)
    lo_d = _row_adapters(case, ads, "decode", "decoder", fault)
    logits = torch.zeros(Fn, K, B, V, dtype=dt)
    kv = torch.zeros(Fn, bb.n_layers, 2, B, bb.n_kv_heads, S_KEEP, bb.head_dim, dtype=dt)
    poss = torch.zeros(Fn, B, dtype=torch.int64)
    # ---- prefill: every row on its own, the training forward, K / V copied into the cache
    last_h, last_x = torch.zeros(B, bb.dim, dtype=dt), torch.zeros(B, bb.dim, dtype=dt)
    for b in range(B):
        S = inp["lens"][b]
        xf, xres, ks, vs = _prompt_stack(P, "backbone", bb, R(_embed(P, inp["tokens"][b], inp["masks"][b])), R, lo_p[b])
        for i in range(bb.n_layers):
            cache[i, 0, b, :, :S], cache[i, 1, b, :, :S] = ks[i].transpose(0, 1), vs[i].transpose(0, 1)
        pos[b] = S - 1 + (1 if fault == "backbone_pos_plus_one" else 0)
        last_h[b], last_x[b] = xf[-1], xres[-1]
    for f in range(Fn):
        rows = case.active(f) if fault != "idle_row_advanced" else list(range(B))
        if f > 0:
            # ---- backbone step: the embedding of the fed-back frame at the next position
            tok, msk = _frame_tokens(forced[f - 1].t()[rows])
            for j, b in enumerate(rows):
                if b in case.idle:                               # (fault idle_row_advanced only: an idle row is fed zeros)
                    tok[j], msk[j] = 0, False
            pos[rows] += 1
            xres = _decode_step(P, Wd, "backbone", bb, R(_embed(P, tok, msk, fault)), pos[rows], cache, rows, R, [lo_b[b] for b in rows],
                                slot_off=1 if fault == "kv_slot_plus_one" else 0)
            last_x[rows] = xres
            last_h[rows] = R(T._rms(xres, P["backbone.norm.scale"], bb.norm_eps))
            for b in range(B):
                if b not in rows:
                    pos[b] = IDLE_PIN                            # serve_frame pins an idle row's device position: 0, then + 1
        rows_t = torch.tensor(rows)
        head_in = last_x if fault == "no_backbone_norm_c0" else last_h
        logits[f, 0, rows_t] = head_in[rows] @ P["codebook0_head.weight"].t()
        # ---- depth decoder: position 0 is the backbone state, position i the embedding of code i - 1
        dcache = torch.zeros(dc.n_layers, 2, B, dc.n_kv_heads, K + 1, dc.head_dim, dtype=dt)
        los = [lo_d[b] for b in rows]
        for i in range(K):
            if i == 0:
                x = last_h[rows] if fault == "no_projection_pos0" else R(last_h[rows] @ P["projection.weight"].t())
            else:
                off = (i - 1) * V
                if fault == "gather_offset_dropped" or (fault == "gather_offset_plus_one" and i == 3):
                    off = 0 if fault == "gather_offset_dropped" else i * V
                x = R(P["audio_embeddings.weight"][forced[f, i - 1, rows_t] + off] @ P["projection.weight"].t())
            di = max(i - 1, 0) if fault == "decoder_pos_minus_one" else i
            hres = _decode_step(P, Wd, "decoder", dc, x, torch.full((len(rows),), di, dtype=torch.int64), dcache, rows, R, los)
            if i >= 1:
                dn = P["decoder.norm.scale"]
                xh = hres if fault == "no_decoder_norm" else R(T._rms(hres, dn, dc.norm_eps))
                if fault == "decoder_norm_twice":
                    xh = R(T._rms(xh, dn, dc.norm_eps))
                hi = i - 2 if (fault == "head_last_shifted" and i == K - 1) else i - 1
                logits[f, i, rows_t] = xh @ P["audio_head"][hi]
        kv[f], poss[f] = cache[..., :S_KEEP, :], pos
    return Result(logits, kv, poss, quantised)


def _run_recompute(case: Case, R, P, ads, fault, inp) -> Result:
    """use_kv_cache = False: every frame recomputes the whole history with the prompt-side forward (adapters: model.lora)."""
    dt = P["projection.weight"].dtype
    B, Fn, bb, dc = case.B, case.frames, CFG.backbone, CFG.decoder
    forced = inp["forced"]
    lo_p = _row_adapters(case, ads, "prompt", "backbone", fault)
    logits = torch.zeros(Fn, K, B, V, dtype=dt)
    for b in range(B):
        tok, msk = inp["tokens"][b], inp["masks"][b]
        for f in range(Fn):
            if f > 0:
                t1, m1 = _frame_tokens(forced[f - 1, :, b][None])
                tok, msk = torch.cat([tok, t1]), torch.cat([msk, m1])
            xf, _, _, _ = _prompt_stack(P, "backbone", bb, R(_embed(P, tok, msk)), R, lo_p[b])
            last_h = xf[-1]
            logits[f, 0, b] = last_h @ P["codebook0_head.weight"].t()
            emb = P["audio_embeddings.weight"][forced[f, :K - 1, b] + V * torch.arange(K - 1)]
            x0 = R(torch.cat([last_h[None], emb]) @ P["projection.weight"].t())
            dxf, _, _, _ = _prompt_stack(P, "decoder", dc, x0, R, lo_p[b], fused_rope=False)
            for i in range(1, K):
                logits[f, i, b] = dxf[i] @ P["audio_head"][i - 1]
    return Result(logits, None, None)


def adapters(case: Case, dtype=F64):
    if case.live is not None:
        return {"live": make_adapter(case.live, dtype)}
    if case.rows is not None:
        return {"bank": [make_adapter(a, dtype) for a in case.bank]}
    return {}


def frame64(case: Case, P=None, ads=None) -> Result:
    return _run(case, T.Rounder(False), P, ads)


def frame_emulated(case: Case, seed: Optional[int] = None, P=None, ads=None, fault: Optional[str] = None, hooks: bool = True) -> Result:
    return _run(case, T.Rounder(hooks, seed), P, ads, fault)


# ------------------------------------------------------------------------------------------------------------ the judge
@dataclass
class Verdict:
    ratios: Dict[Tuple[int, int], float]       # (frame, codebook) -> the worst logits ratio over the judged rows
    kv_ratios: Dict[int, float]                # frame -> the worst ratio of the K / V rows it wrote
    broken: List[str]                          # every exact condition that does not hold
    n_logits: int
    n_kv: int

    @property
    def worst(self) -> float:
        return float("inf") if self.broken else max(list(self.ratios.values()) + list(self.kv_ratios.values()))


def _ratio(a, b, c):
    """Per vector over the last dimension."""
    num = (a - b).norm(dim=-1)
    den = torch.maximum((c - b).norm(dim=-1), 2.0 ** -10 * b.norm(dim=-1))
    r = torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))
    return torch.nan_to_num(r, nan=float("inf"))


def judge(got: Result, x64: Result, emu: Result, case: Case, quiet: bool = False) -> Verdict:
    ratios, kvr, broken, n_lg, n_kv = {}, {}, [], 0, 0
    if got.quantised != x64.quantised:
        broken.append(f"the decode steps hold other weights as e4m3 codes than the reference: {sorted(got.quantised ^ x64.quantised)}")
    g, r, e = (t.logits.detach().to("cpu", F64) for t in (got, x64, emu))
    assert g.shape == r.shape == e.shape == (case.frames, K, case.B, V), (g.shape, r.shape)
    for f in range(case.frames):
        rows = torch.tensor(case.active(f))
        for i in range(K):
            ratios[(f, i)] = float(_ratio(g[f, i, rows], r[f, i, rows], e[f, i, rows]).max())
            n_lg += len(rows)
            if not quiet:
                print(f"RATIO {case.name} {f} {i} {ratios[(f, i)]:.3f}")
    if x64.kv is None:
        return Verdict(ratios, kvr, broken, n_lg, n_kv)
    gk, rk, ek = (t.kv.detach().to("cpu", F64) for t in (got, x64, emu))
    assert gk.shape == rk.shape == ek.shape, (gk.shape, rk.shape)
    for f in range(case.frames):
        worst = 0.0
        for b in range(case.B):
            p, pg = int(x64.pos[f, b]), int(got.pos[f, b])
            if pg != p:
                broken.append(f"frame {f} row {b}: position {pg}, the reference's is {p}")
            if b not in case.active(f):
                keep = [s for s in range(S_KEEP) if s != IDLE_PIN]
                if not torch.equal(gk[f][:, :, b][:, :, :, keep], gk[f - 1][:, :, b][:, :, :, keep]):
                    broken.append(f"frame {f} idle row {b}: a cache slot other than {IDLE_PIN} changed")
                continue
            if bool((gk[f][:, :, b, :, p + 1:] != 0).any()):
                broken.append(f"frame {f} row {b}: a cache slot past position {p} is not zero")
            lo = 0
            if f > 0:
                lo = p
                if not torch.equal(gk[f][:, :, b, :, :p], gk[f - 1][:, :, b, :, :p]):
                    broken.append(f"frame {f} row {b}: a cache slot below position {p} changed")
            rt = _ratio(gk[f][:, :, b, :, lo:p + 1], rk[f][:, :, b, :, lo:p + 1], ek[f][:, :, b, :, lo:p + 1])
            n_kv += rt.numel()
            worst = max(worst, float(rt.max()))
        kvr[f] = worst
        if not quiet:
            print(f"RATIO {case.name} {f} kv {worst:.3f}")
    return Verdict(ratios, kvr, broken, n_lg, n_kv)


def expected_counts(case: Case, inp=None) -> Tuple[int, int]:
    """How many logits vectors and K / V rows ``judge`` must have judged: none may be skipped."""
    inp = inp if inp is not None else inputs(case)
    n_lg = sum(K * len(case.active(f)) for f in range(case.frames))
    if not case.kv_cache:
        return n_lg, 0
    per_slot = CFG.backbone.n_layers * 2 * CFG.backbone.n_kv_heads
    return n_lg, per_slot * (sum(inp["lens"]) + sum(len(case.active(f)) for f in range(1, case.frames)))


def measure(cases=None, seeds=SEEDS, quiet=True):
    """-> (W, {case: its worst ratio}): every stochastic draw judged against frame64 with the nearest-even draw as x_emu."""
    per, P = {}, params()
    for c in (cases if cases is not None else CASES.values()):
        ads = adapters(c)
        x64, rne = frame64(c, P, ads), frame_emulated(c, None, P, ads)
        per[c.name] = max(judge(frame_emulated(c, s, P, ads), x64, rne, c, quiet=True).worst for s in seeds)
        if not quiet:
            print(f"W {c.name} {per[c.name]:.3f}")
    return max(per.values()), per


# ------------------------------------------------------------------------------------------------------------ the old criteria
def sampled_codes(logits: torch.Tensor, noise: torch.Tensor, case: Case) -> torch.Tensor:
    """The oracle sampler on logits [F, K, B, V] with noise [F, K, B, V]: T 0.8 / top-k 12, or each row's own pair."""
    out = torch.empty(logits.shape[:3], dtype=torch.int64)
    lg = logits.float()
    for b in range(case.B):
        t, k = case.sampling[b] if case.sampling is not None else (TEMP, TOPK)
        out[:, :, b] = O.sample_topk(lg[:, :, b], k, t, noise[:, :, b])[..., 0]
    return out


def old_criteria(mut: Result, x64: Result, emu: Result, case: Case, inp=None):
    """What the engine tests assert, on a mutant's logits: (the share of sampled codes that agree with the reference's - the tests
    ask >= 0.9; the codebook-0 max|err| over what the nearest-even emulation errs - the served tests ask <= 2)."""
    inp = inp if inp is not None else inputs(case)
    a, b = sampled_codes(mut.logits, inp["noise"], case), sampled_codes(x64.logits, inp["noise"], case)
    keep = torch.zeros(a.shape, dtype=torch.bool)
    for f in range(case.frames):
        keep[f][:, case.active(f)] = True
    agree = float((a == b)[keep].float().mean())
    k0 = keep[:, 0]
    c0 = float((mut.logits[:, 0] - x64.logits[:, 0]).abs().amax(-1)[k0].max()) / float((emu.logits[:, 0] - x64.logits[:, 0]).abs().amax(-1)[k0].max())
    return agree, c0


# ------------------------------------------------------------------------------------------------------------ faults
# name -> (what is wired wrongly, the cases of CASES it can show in), in the order of the issue's catalogue
FAULTS: Dict[str, Tuple[str, Tuple[str, ...]]] = {
    "head_last_shifted": ("the last codebook's logits taken with the head of the codebook before it", ("plain_b3",)),
    "gather_offset_plus_one": ("gather offset i V instead of (i - 1) V for codebook 3's input", ("plain_b3",)),
    "gather_offset_dropped": ("gather offset dropped: every code embedded as codebook 0's", ("plain_b3",)),
    "decoder_pos_minus_one": ("decoder position i - 1 for i >= 1", ("plain_b1", "plain_b3")),
    "no_decoder_norm": ("decoder final norm missing before the head", ("plain_b3",)),
    "decoder_norm_twice": ("decoder final norm applied twice", ("plain_b3",)),
    "no_backbone_norm_c0": ("backbone final norm missing before the codebook-0 head", ("plain_b3",)),
    "no_projection_pos0": ("projection skipped at decoder position 0", ("plain_b3",)),
    "backbone_pos_plus_one": ("backbone position one too far after the prefill", ("plain_b3",)),
    "kv_slot_plus_one": ("new backbone K / V written one slot too far", ("plain_b3",)),
    "text_column_added": ("the masked-off text column added into an audio frame's embedding", ("plain_b3",)),
    "decoder_lora_scale_one": ("LoRA scale 1 in the decoder stack only", ("live_qv_b1", "live_all7_bias_b2")),
    "decoder_adapter_next_row": ("row b takes row b + 1's adapter in the decoder only", ("rows_b4",)),
    "none_row_gets_adapter0": ("a row without an adapter gets adapter 0", ("rows_b4",)),
    "bias_rows_stacked": ("group bias rows stacked w1 | w3 instead of interleaved", ("live_all7_bias_b2",)),
    "fp8_w13_scales_stacked": ("FP8 row scales of w13 not interleaved with their rows", ("fp8_b4",)),
    "fp8_b1_out_proj_quantised": ("the B = 1 decoder output projection quantised although the fused path keeps it bf16", ("fp8_b1",)),
    "idle_row_advanced": ("an idle row advanced", ("serve_idle_b4",)),
}

# the faults the old criteria let through (test_gen_frame_ref_cpu.py recomputes this set)
OLD_CRITERIA_BLIND = ("no_backbone_norm_c0", "fp8_b1_out_proj_quantised", "idle_row_advanced")

RECORD = """  W = 3.6215, recorded as 3.63; L = 7.26; 2 L = 14.52 (measured 2026-10-20).  Per case: the worst ratio of the eight draws (reference
  alone), then the worst ratio of the engine on an MI355X (measured 2026-10-20; eager and graph alike - their logits and caches
  are equal bit for bit; every exact condition held, every picked code equal to the oracle sampler's):
    plain_b1 2.48 / 1.29        plain_b3 2.80 / 1.48          plain_b16 3.43 / 1.71         recompute_b2 3.10 / 1.59
    fp8_b1 2.91 / 1.65          fp8_b4 2.94 / 1.51            live_qv_b1 2.76 / 1.57        live_all7_bias_b2 3.29 / 1.60
    live_mlp_r4_b4 2.97 / 1.49  rows_b4 2.89 / 1.44           rows_b16 3.62 / 1.95          fp8_rows_b4 2.90 / 1.56
    serve_idle_b4 2.72 / 1.44
  No case failed and the engine was not changed.
  Fault table: worst ratio of the faulty emulation (caught at >= 2 L, or by a broken exact condition) and the older criteria on
  the same logits against the TRUE reference - the share of codes sampled alike (T 0.8, top-k 12, the engine tests' noise; they ask
  >= 0.9) and, for the served rows, codebook-0 max|err| over the emulation's (they ask <= 2).  Where both compared paths share a
  fault the older criteria see nothing at all, whatever this table says.
    fault                        case                ratio   broken   codes agree   c0 err / emulation's   old criteria
    head_last_shifted            plain_b3            158.7   0        0.875         1.00                   fail
    gather_offset_plus_one       plain_b3            132.7   0        0.542         1.00                   fail
    gather_offset_dropped        plain_b3            160.7   0        0.417         1.00                   fail
    decoder_pos_minus_one        plain_b1            105.9   0        0.300         1.00                   fail
                                 plain_b3            123.9   0        0.400         1.00                   fail
    no_decoder_norm              plain_b3            88.6    0        0.758         1.00                   fail
    decoder_norm_twice           plain_b3            26.9    0        0.875         1.00                   fail
    no_backbone_norm_c0          plain_b3            82.3    0        0.975         45.66                  PASS (c0 is asked of served rows only)
    no_projection_pos0           plain_b3            173.8   0        0.308         1.00                   fail
    backbone_pos_plus_one        plain_b3            638.0   27       0.817         32.65                  fail
    kv_slot_plus_one             plain_b3            638.0   12       0.817         51.13                  fail
    text_column_added            plain_b3            176.1   0        0.675         64.03                  fail
    decoder_lora_scale_one       live_qv_b1          41.6    0        0.800         1.00                   fail
                                 live_all7_bias_b2   55.2    0        0.600         1.00                   fail
    decoder_adapter_next_row     rows_b4             114.3   0        0.644         1.00                   fail
    none_row_gets_adapter0       rows_b4             172.2   0        0.844         69.13                  fail
    bias_rows_stacked            live_all7_bias_b2   28.1    0        0.850         9.56                   fail
    fp8_w13_scales_stacked       fp8_b4              57.6    0        0.644         34.67                  fail
    fp8_b1_out_proj_quantised    fp8_b1              5.9     1        0.975         1.00                   PASS
    idle_row_advanced            serve_idle_b4       1.0     16       0.969         1.00                   PASS
  fp8_b1_out_proj_quantised does NOT reach 2 L as a ratio: one 256 x 256 e4m3 matrix among the eight of the depth decoder moves no
  logits vector by more than 5.9 x its bf16 noise (11 with weights placed on e4m3 midpoints, measured).  It is caught by an exact
  condition instead: the set of weights held as e4m3 codes equals the reference's (the GPU test reads it off the state's tables).
  Two of the faults planted in the real engine (a wrapper of ops.gemv_ex that moves codebook 3's row_offset, or drops the norm
  prologue of the head product; plain_b3, MI355X, 2026-10-20) give the catalogue's figures: 132.7 and 88.9; unplanted 1.5.
  The model: matrices N(0, 0.06) and norm scales 1 + 0.25 N(0, 1) (``params``); with the initialiser's N(0, 0.02) and unit norm
  scales decoder_norm_twice shows ratio 1.0 (a norm of a normed row is that row) and the logits are nearly flat."""
__doc__ = __doc__.replace("%(record)s", RECORD)
