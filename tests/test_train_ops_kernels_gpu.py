"""The training step's bandwidth kernels of csrc/ops.hip - RMSNorm, the column sums, dropout, bias, RoPE, SwiGLU, the embedding
forward and backward, the row moves, cross-entropy, the gradient norm / clip and AdamW - against the float64 reference of
tests/train_ops_ref.py (proved by tests/test_train_ops_ref_cpu.py).  Kernel level only: no model is built.

Every output buffer starts as NaN (or a sentinel) and every element of every case is judged by ``train_ops_ref.judge``: the bounds
are derived there from u = 2^-24, the length of the kernel's serial chain and the allowances of the device functions - never
from what the kernels give.  Each judgement prints ``RATIO <kernel> <worst |err| / bound>``; a ratio above 1 fails."""
import ctypes

import pytest
import torch

import train_ops_ref as T

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _cu(t):
    return None if t is None else t.cuda()


def _nan(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _lib():
    from csm.hip import check, lib
    return check, lib


def _ids(cases):
    return [(c.name + (f"_R{c.R}" if hasattr(c, "R") else "")) if hasattr(c, "name") else "-".join(str(int(v) if isinstance(v, bool) else v) for v in c)
            for c in cases]


def _cases(op):
    return pytest.mark.parametrize("c", T.OPS[op].cases, ids=_ids(T.OPS[op].cases))


def _judge(op, c, got, inp=None):
    inp = T.OPS[op].inputs(c) if inp is None else inp
    T.judge_all(op, got, T.OPS[op].ref(inp), str(c))


# ------------------------------------------------------------------------------------------------------------- RMSNorm
@_cases("rmsnorm_fwd")
def test_rmsnorm_fwd(dev, c):
    check, lib = _lib()
    i = T.rms_inputs(c)
    y, rstd = _nan(c.M, c.D), _nan(c.M, dtype=torch.float32) if c.rstd else None
    x, w = _cu(i["x"]), _cu(i["w"])
    check(lib.csm_rmsnorm_fwd(_p(x), _p(w), _p(y), _p(rstd), c.M, c.D, T.EPS, _s()), "csm_rmsnorm_fwd")
    _judge("rmsnorm_fwd", c, {"y": y, "rstd": rstd}, i)


@_cases("rmsnorm_bwd")
def test_rmsnorm_bwd(dev, c):
    check, lib = _lib()
    from csm.hip import ops
    i = T.rms_inputs(c)
    x, w, r, dy, dres = (_cu(i[k]) for k in ("x", "w", "rstd", "dy", "dres"))
    dx = _nan(c.M, c.D)
    part = _nan(lib.csm_rmsnorm_bwd_blocks(), c.D, dtype=torch.float32) if c.dsc else None
    check(lib.csm_rmsnorm_bwd(_p(x), _p(w), _p(r), _p(dy), _p(dres), _p(dx), _p(part), c.M, c.D, _s()), "csm_rmsnorm_bwd")
    got = {"dx": dx}
    if c.dsc:
        assert not bool(torch.isnan(part).any()), "a partial row of dscale was not written"
        got["dscale"] = _nan(c.D)
        ops.colsum_bf16(part, got["dscale"], accumulate=False)
    _judge("rmsnorm_bwd", c, got, i)


# ------------------------------------------------------------------------------------------------------------- column sums
@_cases("colsum")
def test_colsum(dev, c):
    """n = 1: csm_colsum_bf16.  n > 1: csm_colsum_bf16_multi, judged pair by pair and bit-equal to the single launches."""
    from csm.hip import ops
    i = T.colsum_inputs(c)
    parts = [_cu(p) for p in i["partials"]]
    single = [_cu(d) if c.acc else _nan(c.D) for d in i["dst"]]
    for p, d in zip(parts, single):
        ops.colsum_bf16(p, d, accumulate=c.acc)
    _judge("colsum", c, {f"dst{k}": d for k, d in enumerate(single)}, i)
    multi = [_cu(d) if c.acc else _nan(c.D) for d in i["dst"]]
    ops.colsum_bf16_multi(list(zip(parts, multi)), accumulate=c.acc)
    for a, b in zip(single, multi):
        T.judge("colsum_multi", b, a.cpu(), None)


@_cases("colsum_rows")
def test_colsum_rows(dev, c):
    check, lib = _lib()
    i = T.colsum_rows_inputs(c)
    x, part = _cu(i["x"]), _nan(c.S, c.D, dtype=torch.float32)
    check(lib.csm_colsum_rows_bf16(_p(x), c.ld, c.M, c.D, _p(part), c.S, _s()), "csm_colsum_rows_bf16")
    _judge("colsum_rows", c, {"partials": part}, i)


# ------------------------------------------------------------------------------------------------------------- dropout, bias
def _dropout(lib, check, x, out, c, M=None):
    check(lib.csm_dropout_bf16(_p(x), x.stride(0), _p(out), out.stride(0), c.M if M is None else M, c.D, c.p, c.seed, int(c.acc), _s()),
          "csm_dropout_bf16")


@_cases("dropout")
def test_dropout(dev, c):
    """Mask and kept values bit for bit; columns >= D of a strided output untouched; the mask is a function of (seed, row D + col)
    alone: another pair of strides and a launch on the first rows reproduce it; p = 0 is the identity."""
    check, lib = _lib()
    i = T.drop_inputs(c)
    x, out = _cu(i["x"]), _cu(i["out0"])
    _dropout(lib, check, x, out, c)
    _judge("dropout", c, {"out": out}, i)
    want = T.drop_f32(i)["out"][:, :c.D]
    if c.M * c.D <= 1 << 16:
        x2, out2 = torch.zeros(c.M, c.ld_in + 16, dtype=BF16, device="cuda"), torch.zeros(c.M, c.ld_out + 8, dtype=BF16, device="cuda")
        x2[:, :c.D], out2[:, :c.D] = x[:, :c.D], _cu(i["out0"])[:, :c.D]
        _dropout(lib, check, x2, out2, c)
        T.judge("dropout.other_strides", out2[:, :c.D].contiguous(), want.contiguous(), None)
        Ms = (c.M + 1) // 2
        out3 = _cu(i["out0"])
        _dropout(lib, check, x, out3, c, M=Ms)
        T.judge("dropout.row_slice", out3[:Ms, :c.D].contiguous(), want[:Ms].contiguous(), None)
        T.judge("dropout.row_slice_rest", out3[Ms:].contiguous(), i["out0"][Ms:].contiguous(), None)
    if c.p == 0.0 and not c.acc:
        T.judge("dropout.identity", out[:, :c.D].contiguous(), i["x"][:, :c.D].contiguous(), None)


@_cases("bias_add")
def test_bias_add(dev, c):
    check, lib = _lib()
    i = T.bias_inputs(c)
    y, b = _cu(i["y"]), _cu(i["bias"])
    check(lib.csm_bias_add_bf16(_p(y), c.ld, _p(b), c.M, c.D, _s()), "csm_bias_add_bf16")
    _judge("bias_add", c, {"y": y}, i)


# ------------------------------------------------------------------------------------------------------------- RoPE, SwiGLU
@_cases("rope")
def test_rope(dev, c):
    check, lib = _lib()
    i = T.rope_inputs(c)
    qkv, table, pos = _cu(i["qkv"]), _cu(i["table"]), _cu(i["pos"]) if c.use_pos else None
    check(lib.csm_rope(_p(qkv), _p(table), _p(pos), c.M, c.S, c.nh, c.hd, qkv.stride(0), int(c.inverse), _s()), "csm_rope")
    W = c.nh * c.hd
    _judge("rope", c, {"rot": qkv[:, :W].contiguous(), "rest": qkv[:, W:].contiguous()}, i)


@_cases("swiglu_fwd")
def test_swiglu_fwd(dev, c):
    check, lib = _lib()
    i = T.swiglu_inputs(c)
    gu, out = _cu(i["gu"]), _nan(c.M, c.F)
    check(lib.csm_swiglu_fwd(_p(gu), _p(out), c.M, c.F, _s()), "csm_swiglu_fwd")
    _judge("swiglu_fwd", c, {"out": out}, i)


@_cases("swiglu_bwd")
def test_swiglu_bwd(dev, c):
    check, lib = _lib()
    i = T.swiglu_inputs(c)
    gu, dout, dgu = _cu(i["gu"]), _cu(i["dout"]), _nan(c.M, 2 * c.F)
    check(lib.csm_swiglu_bwd(_p(gu), _p(dout), _p(dgu), c.M, c.F, _s()), "csm_swiglu_bwd")
    _judge("swiglu_bwd", c, {"dgu": dgu}, i)


# ------------------------------------------------------------------------------------------------------------- embedding, rows
@_cases("embed_fwd")
def test_embed_fwd(dev, c):
    from csm.hip import ops
    i = T.embed_inputs(c)
    out = _nan(i["tokens"].shape[0], c.D)
    ops.embed_fwd(_cu(i["tokens"]), _cu(i["mask"]), _cu(i["text"]), _cu(i["audio"]), out, T.VA)
    _judge("embed_fwd", c, {"out": out}, i)


@_cases("embed_bwd_sorted")
def test_embed_bwd_sorted(dev, c):
    from csm.hip import ops
    i = T.embed_bwd_inputs(c)
    gt, ga = _cu(i["g_text"]), _cu(i["g_audio"])
    ops.embed_bwd_sorted(_cu(i["rows"]), _cu(i["src"]), _cu(i["dh"]), _cu(i["dseq"]), gt, ga)
    _judge("embed_bwd_sorted", c, {"g_text": gt, "g_audio": ga}, i)


@_cases("rows_add")
def test_rows_add(dev, c):
    from csm.hip import ops
    i = T.rows_inputs(c)
    dst = _cu(i["table"])
    ops.rows_add_bf16(dst, _cu(i["rows"]), _cu(i["src"]), c.stride)
    _judge("rows_add", c, {"dst": dst}, i)


@_cases("rows_take")
def test_rows_take(dev, c):
    from csm.hip import ops
    i = T.rows_inputs(c)
    table, out = _cu(i["table"]), _nan(c.N, c.D)
    ops.rows_take_bf16(table, _cu(i["rows"]), out)
    _judge("rows_take", c, {"out": out, "table": table}, i)


@_cases("decoder_input_fwd")
def test_decoder_input_fwd(dev, c):
    from csm.hip import ops
    i = T.decin_inputs(c)
    out = _nan(c.N, c.K, c.D)
    ops.decoder_input_fwd(_cu(i["hidden"]), _cu(i["rows"]), _cu(i["codes"]), _cu(i["audio"]), out, T.VA)
    _judge("decoder_input_fwd", c, {"out": out}, i)


# ------------------------------------------------------------------------------------------------------------- cross-entropy
@_cases("ce_fwd_bwd")
def test_ce_fwd_bwd(dev, c):
    """Every dispatch of csm_ce_fwd_bwd; loss_rows per row, and csm_reduce_sum_f32 on top of the device's own rows."""
    check, lib = _lib()
    i = T.ce_inputs(c)
    flat = torch.full((c.R * c.ldl + 4,), T.CE_GARBAGE, device="cuda")
    logits = flat[c.offset:c.offset + c.R * c.ldl].view(c.R, c.ldl)           # offset 1: one float off the 16-byte alignment
    logits.copy_(i["logits"])
    assert T.ce_kernel_chain(c, aligned=logits.data_ptr() % 16 == 0)[0] == T.ce_kernel_chain(c)[0]
    tg, loss = _cu(i["targets"]), _nan(c.R, dtype=torch.float32)
    dl = _nan(c.R, c.ldd) if c.has_d else None
    check(lib.csm_ce_fwd_bwd(_p(logits), _p(tg), _p(loss), _p(dl), c.R, c.V, c.ldl, c.ldd, T.CE_GSCALE, _s()), "csm_ce_fwd_bwd")
    got = {"loss_rows": loss}
    if c.has_d:
        got["dlogits"] = dl
    _judge("ce_fwd_bwd", c, got, i)
    total = _nan(1, dtype=torch.float32)
    check(lib.csm_reduce_sum_f32(_p(loss), c.R, T.REDUCE_SCALE, _p(total), _s()), "csm_reduce_sum_f32")
    T.judge_all("reduce_sum", {"out": total}, T.reduce_ref(dict(x=loss.cpu())), f"loss rows of {c.name}")


@pytest.mark.parametrize("n", T.REDUCE_N)
def test_reduce_sum(dev, n):
    check, lib = _lib()
    i = T.reduce_inputs(n)
    x, out = _cu(i["x"]), _nan(1, dtype=torch.float32)
    check(lib.csm_reduce_sum_f32(_p(x), n, T.REDUCE_SCALE, _p(out), _s()), "csm_reduce_sum_f32")
    _judge("reduce_sum", n, {"out": out}, i)


# ------------------------------------------------------------------------------------------------------------- norm and clip
@_cases("sumsq")
def test_sumsq_and_clip(dev, c):
    """The per-block partial sums, then csm_clip_coef on the device's own partials for every kind of max_norm."""
    check, lib = _lib()
    i = T.sumsq_inputs(c)
    assert lib.csm_sumsq_blocks() == T.SUMSQ_BLOCKS
    buf = _cu(i["buf"])
    g = buf[c.offset:]
    part = _nan(T.SUMSQ_BLOCKS, dtype=torch.float32)
    check(lib.csm_sumsq_bf16(_p(g), c.n, _p(part), _s()), "csm_sumsq_bf16")
    _judge("sumsq", c, {"partials": part}, i)
    norm = float(part.double().sum().sqrt())
    for max_norm in (0.0, -1.0, 0.5 * norm, 2.0 * norm + 1.0):
        out = _nan(2, dtype=torch.float32)
        check(lib.csm_clip_coef(_p(part), T.SUMSQ_BLOCKS, max_norm, _p(out), _s()), "csm_clip_coef")
        T.judge_all("clip_coef", {"norm_and_coef": out}, T.clip_ref(dict(partials=part.cpu(), max_norm=float(torch.tensor(max_norm).float()))),
                    f"n={c.n} max_norm={max_norm:.3g}")


@_cases("clip_coef")
def test_clip_coef(dev, c):
    check, lib = _lib()
    i = T.clip_inputs(c)
    part, out = _cu(i["partials"]), _nan(2, dtype=torch.float32)
    check(lib.csm_clip_coef(_p(part), T.SUMSQ_BLOCKS, i["max_norm"], _p(out), _s()), "csm_clip_coef")
    _judge("clip_coef", c, {"norm_and_coef": out}, i)


# ------------------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("c", T.ADAM_CASES, ids=_ids(T.ADAM_CASES))
def test_adamw_step_and_split(dev, c):
    """master / m / v after EACH step against the float64 step from the device's own previous state; param = master.to(bf16);
    zero_grad; the split-master kernel equal to the plain one bit for bit in master, m and v."""
    from csm.hip import lib, ops
    i = T.adam_inputs(c)
    coef = torch.tensor([123.0, c.coef], device="cuda") if c.coef is not None else None
    master, m, v = _cu(i["master"]), _cu(i["m"]), _cu(i["v"])
    param = _nan(c.n)
    sp, slo = (t.cuda() for t in T.split_master(i["master"]))
    sm, sv = m.clone(), v.clone()
    if c.one_block:
        lib.csm_set_adamw_blocks(1)                           # one block: the grid-stride loop does all the work
    try:
        for step, g in zip(T.ADAM_STEPS, i["grads"]):
            state = {"master": master.cpu(), "m": m.cpu(), "v": v.cpu()}
            grad, sgrad = _cu(g), _cu(g)
            kw = dict(norm_and_coef=coef, grad_mul=c.gmul, zero_grad=c.zero_grad)
            ops.adamw_step(master, m, v, param, grad, T.ADAM_LR, T.ADAM_B1, T.ADAM_B2, T.ADAM_EPS, c.wd, step, **kw)
            ops.adamw_step_split(slo, sm, sv, sp, sgrad, T.ADAM_LR, T.ADAM_B1, T.ADAM_B2, T.ADAM_EPS, c.wd, step, **kw)
            T.judge_all("adamw", {"master": master, "m": m, "v": v}, T.adam_ref(state, g, c, step), f"{c} step {step}")
            T.judge("adamw.param", param, master.cpu().to(BF16), None)
            want_grad = torch.zeros_like(g) if c.zero_grad else g
            T.judge("adamw.grad", grad, want_grad, None)
            T.judge("adamw_split.grad", sgrad, want_grad, None)
            T.judge("adamw_split.master", T.join_master(sp.cpu(), slo.cpu()).view(torch.int32), master.cpu().view(torch.int32), None)
            T.judge("adamw_split.m", sm.view(torch.int32), m.cpu().view(torch.int32), None)
            T.judge("adamw_split.v", sv.view(torch.int32), v.cpu().view(torch.int32), None)
            T.judge("adamw_split.param", sp, T.split_master(master.cpu())[0], None)
    finally:
        lib.csm_set_adamw_blocks(1 << 20)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_documented_bad_arguments_are_refused(dev):
    """Every CSM_REQUIRE of the entries above that a caller can trip without a bad address: the call returns 1 before any launch
    and the outputs keep their sentinel."""
    from csm.hip import lib
    s = _s()
    a = torch.full((64, 4104), 3.0, dtype=BF16, device="cuda")                # any bf16 operand
    f = torch.full((256 * 4104,), 3.0, dtype=torch.float32, device="cuda")    # any fp32 operand
    idx = torch.zeros(64, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    u8 = torch.ones(64, dtype=torch.uint8, device="cuda")
    out = torch.full((64, 4104), 7.0, dtype=BF16, device="cuda")
    fo = torch.full((256 * 4104,), 7.0, dtype=torch.float32, device="cuda")
    A, Fp, O, FO, I, I32, M8 = (_p(t) for t in (a, f, out, fo, idx, i32, u8))
    beta = (1e-3, 0.9, 0.999, 1e-8, 0.01)
    calls = {
        "rmsnorm_fwd D%8": lambda: lib.csm_rmsnorm_fwd(A, A, O, FO, 4, 12, 1e-5, s),
        "rmsnorm_fwd D>4096": lambda: lib.csm_rmsnorm_fwd(A, A, O, FO, 4, 4104, 1e-5, s),
        "rmsnorm_fwd null x": lambda: lib.csm_rmsnorm_fwd(None, A, O, FO, 4, 8, 1e-5, s),
        "rmsnorm_fwd null y": lambda: lib.csm_rmsnorm_fwd(A, A, None, FO, 4, 8, 1e-5, s),
        "rmsnorm_fwd M=0": lambda: lib.csm_rmsnorm_fwd(A, A, O, FO, 0, 8, 1e-5, s),
        "rmsnorm_bwd D%8": lambda: lib.csm_rmsnorm_bwd(A, A, Fp, A, None, O, FO, 4, 12, s),
        "rmsnorm_bwd D>4096": lambda: lib.csm_rmsnorm_bwd(A, A, Fp, A, None, O, FO, 4, 4104, s),
        "rmsnorm_bwd null rstd": lambda: lib.csm_rmsnorm_bwd(A, A, None, A, None, O, FO, 4, 8, s),
        "colsum null": lambda: lib.csm_colsum_bf16(None, 4, 8, O, 0, s),
        "colsum rows=0": lambda: lib.csm_colsum_bf16(Fp, 0, 8, O, 0, s),
        "colsum_multi n=9": lambda: lib.csm_colsum_bf16_multi(9, (ctypes.c_void_p * 9)(*[Fp] * 9), (ctypes.c_void_p * 9)(*[O] * 9), 4, 8, 0, s),
        "colsum_multi null pair": lambda: lib.csm_colsum_bf16_multi(2, (ctypes.c_void_p * 2)(Fp, None), (ctypes.c_void_p * 2)(O, O), 4, 8, 0, s),
        "dropout p=1": lambda: lib.csm_dropout_bf16(A, 4104, O, 4104, 4, 8, 1.0, 1, 0, s),
        "dropout p<0": lambda: lib.csm_dropout_bf16(A, 4104, O, 4104, 4, 8, -0.1, 1, 0, s),
        "dropout D%8": lambda: lib.csm_dropout_bf16(A, 4104, O, 4104, 4, 12, 0.1, 1, 0, s),
        "dropout ld_in<D": lambda: lib.csm_dropout_bf16(A, 8, O, 4104, 4, 16, 0.1, 1, 0, s),
        "dropout ld_out<D": lambda: lib.csm_dropout_bf16(A, 4104, O, 8, 4, 16, 0.1, 1, 0, s),
        "dropout ld%8": lambda: lib.csm_dropout_bf16(A, 4100, O, 4104, 4, 16, 0.1, 1, 0, s),
        "bias_add ld<D": lambda: lib.csm_bias_add_bf16(O, 8, A, 4, 16, s),
        "bias_add D%8": lambda: lib.csm_bias_add_bf16(O, 4104, A, 4, 12, s),
        "bias_add null": lambda: lib.csm_bias_add_bf16(O, 4104, None, 4, 16, s),
        "colsum_rows ld<D": lambda: lib.csm_colsum_rows_bf16(A, 8, 4, 16, FO, 1, s),
        "colsum_rows slices=0": lambda: lib.csm_colsum_rows_bf16(A, 4104, 4, 16, FO, 0, s),
        "colsum_rows slices>65535": lambda: lib.csm_colsum_rows_bf16(A, 4104, 4, 16, FO, 65536, s),
        "rope null table": lambda: lib.csm_rope(O, None, None, 4, 4, 2, 64, 4104, 0, s),
        "rope hd%8": lambda: lib.csm_rope(O, Fp, None, 4, 4, 2, 60, 4104, 0, s),
        "rope ld%8": lambda: lib.csm_rope(O, Fp, None, 4, 4, 2, 64, 4100, 0, s),
        "rope S=0": lambda: lib.csm_rope(O, Fp, None, 4, 0, 2, 64, 4104, 0, s),
        "swiglu_fwd F%8": lambda: lib.csm_swiglu_fwd(A, O, 4, 12, s),
        "swiglu_fwd null": lambda: lib.csm_swiglu_fwd(None, O, 4, 8, s),
        "swiglu_bwd F%8": lambda: lib.csm_swiglu_bwd(A, A, O, 4, 12, s),
        "swiglu_bwd null dout": lambda: lib.csm_swiglu_bwd(A, None, O, 4, 8, s),
        "embed_fwd D%8": lambda: lib.csm_embed_fwd(I, M8, A, A, O, 4, 1, 12, 7, s),
        "embed_fwd K=0": lambda: lib.csm_embed_fwd(I, M8, A, A, O, 4, 0, 8, 7, s),
        "embed_fwd null mask": lambda: lib.csm_embed_fwd(I, None, A, A, O, 4, 1, 8, 7, s),
        "embed_bwd D%8": lambda: lib.csm_embed_bwd_sorted(I, I, 4, A, A, 4, O, O, 4, 8, 12, s),
        "embed_bwd D>4096": lambda: lib.csm_embed_bwd_sorted(I, I, 4, A, A, 4, O, O, 4, 8, 4104, s),
        "embed_bwd n_occ=0": lambda: lib.csm_embed_bwd_sorted(I, I, 0, A, A, 4, O, O, 4, 8, 8, s),
        "rows_add D%8": lambda: lib.csm_rows_add_bf16(O, I32, A, 4, 1, 12, s),
        "rows_add stride=0": lambda: lib.csm_rows_add_bf16(O, I32, A, 4, 0, 8, s),
        "rows_take D%8": lambda: lib.csm_rows_take_bf16(O, I32, O, 4, 12, s),
        "rows_take null rows": lambda: lib.csm_rows_take_bf16(O, None, O, 4, 8, s),
        "decoder_input D%8": lambda: lib.csm_decoder_input_fwd(A, I32, I, A, O, 4, 2, 12, 7, s),
        "decoder_input null codes": lambda: lib.csm_decoder_input_fwd(A, I32, None, A, O, 4, 2, 8, 7, s),
        "ce ldl<V": lambda: lib.csm_ce_fwd_bwd(Fp, I, FO, O, 4, 100, 96, 104, 1.0, s),
        "ce ldd<V": lambda: lib.csm_ce_fwd_bwd(Fp, I, FO, O, 4, 100, 104, 96, 1.0, s),
        "ce null loss": lambda: lib.csm_ce_fwd_bwd(Fp, I, None, O, 4, 100, 104, 104, 1.0, s),
        "ce R=0": lambda: lib.csm_ce_fwd_bwd(Fp, I, FO, O, 0, 100, 104, 104, 1.0, s),
        "reduce_sum n=0": lambda: lib.csm_reduce_sum_f32(Fp, 0, 1.0, FO, s),
        "sumsq misaligned": lambda: lib.csm_sumsq_bf16(A + 2, 64, FO, s),
        "sumsq n=0": lambda: lib.csm_sumsq_bf16(A, 0, FO, s),
        "clip_coef n=0": lambda: lib.csm_clip_coef(Fp, 0, 1.0, FO, s),
        "clip_coef null": lambda: lib.csm_clip_coef(None, 4, 1.0, FO, s),
        "adamw n%8": lambda: lib.csm_adamw_step(FO, FO, FO, O, O, 12, *beta, 1, None, 1.0, 0, s),
        "adamw step=0": lambda: lib.csm_adamw_step(FO, FO, FO, O, O, 8, *beta, 0, None, 1.0, 0, s),
        "adamw null m": lambda: lib.csm_adamw_step(FO, None, FO, O, O, 8, *beta, 1, None, 1.0, 0, s),
        "adamw_split n%8": lambda: lib.csm_adamw_step_split(O, FO, FO, O, O, 12, *beta, 1, None, 1.0, 0, s),
        "adamw_split step=0": lambda: lib.csm_adamw_step_split(O, FO, FO, O, O, 8, *beta, 0, None, 1.0, 0, s),
    }
    wrong = {name: rc for name, rc in ((name, call()) for name, call in calls.items()) if rc != 1}
    torch.cuda.synchronize()
    assert not wrong, f"not refused with code 1: {wrong}"
    assert bool((out == 7.0).all()) and bool((fo == 7.0).all()), "a refused call wrote to its output"
    assert bool((a == 3.0).all()) and bool((f == 3.0).all())


def test_records(dev):
    """Prints the worst bound utilisation per kernel output seen in this run and the measured function errors."""
    for name in sorted(T.utilisation):
        print(f"UTIL {name} {T.utilisation[name]:.4f}")
    print(f"measured function errors (ulp): {dict(T.measured)}")
