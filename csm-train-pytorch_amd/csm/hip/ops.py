"""Torch-tensor front end of the C ABI: shape/dtype checks on the host, raw pointers + the current stream below.

PyTorch is plumbing here (device memory, streams); every arithmetic op is a hand-written gfx950 kernel.
"""
import ctypes
import math
from typing import Optional

import torch

from . import CsmHipError, check, lib
from ..sampling import FULL_LEVEL, LEVELS, PARAMS

BF16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _mat(t: torch.Tensor, dtype=BF16):
    """2-D row-major view with unit inner stride -> (ptr, rows, cols, ld)."""
    assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1, (t.dtype, t.shape, t.stride())
    return t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)


def _pin(pin):
    """The keyword for a pinned call, nothing otherwise: ``gemm`` / ``linear_swiglu_fwd`` may be wrapped by a timer that knows
    their positional arguments only (bench.py), and an un-pinned call must look the way it always did."""
    return {"pin": True} if pin else {}


def gemm(A, B, C, R=None, transA=False, transB=False, alpha=1.0, batch=1, sA=0, sB=0, sC=0, sR=0, pin=False):
    """C[M,N] = alpha * opA(A) . opB(B)^T (+ R).  A: [M,K] (or [K,M] if transA); B: [N,K] (or [K,N] if transB).
    ``pin`` (this call only; bf16 output, one batch): the 128x128 kernel whatever M is, so that a row's bits do not depend on the
    other rows of the launch (``csm_gemm_bf16_pinned``)."""
    pa, a0, a1, lda = _mat(A)
    pb, b0, b1, ldb = _mat(B)
    M, K = (a1, a0) if transA else (a0, a1)
    N, Kb = (b1, b0) if transB else (b0, b1)
    assert K == Kb, (A.shape, B.shape, transA, transB)
    out_f32 = C.dtype == torch.float32
    pc, c0, c1, ldc = _mat(C, C.dtype)
    assert (c0, c1) == (M, N), (C.shape, M, N)
    pr, ldr = None, 0
    if R is not None:
        pr, r0, r1, ldr = _mat(R)
        assert (r0, r1) == (M, N)
    if pin:
        assert not out_f32 and batch == 1
        check(lib.csm_gemm_bf16_pinned(pa, pb, pc, pr, M, N, K, lda, ldb, ldc, ldr, int(transA), int(transB), float(alpha), None, None,
                                       0, 0, None, None, 0, 0, 0, _stream()), "csm_gemm_bf16_pinned")
        return C
    check(lib.csm_gemm_bf16(pa, pb, pc, pr, M, N, K, lda, ldb, ldc, ldr, int(transA), int(transB), int(out_f32),
                            float(alpha), batch, sA, sB, sC, sR, _stream()), "csm_gemm_bf16")
    return C


def linear_swiglu_fwd(x, w13, gu, act, residual=None, pin=False):
    """gu[M,2F] = x w13^T (+ residual) with gate/up interleaved, act[M,F] = silu(gate)*up, one GEMM launch.
    ``residual`` [M,2F] (may be ``gu`` itself) is how LoRA adapters on w1 / w3 join: their product is written first."""
    pa, M, K, lda = _mat(x)
    pb, N, Kb, ldb = _mat(w13)
    assert K == Kb and gu.shape == (M, N) and act.shape == (M, N // 2) and gu.is_contiguous() and act.is_contiguous()
    pr, ldr = (None, 0) if residual is None else (residual.data_ptr(), residual.stride(0))
    assert residual is None or (residual.shape == (M, N) and residual.stride(1) == 1 and residual.dtype == BF16)
    if pin:                                                   # (see gemm)
        check(lib.csm_gemm_bf16_pinned(pa, pb, gu.data_ptr(), pr, M, N, K, lda, ldb, N, ldr, 0, 0, 1.0, None, None, 0, 1, None,
                                       act.data_ptr(), N // 2, 0, 0, _stream()), "csm_gemm_bf16_pinned(swiglu fwd)")
        return
    check(lib.csm_gemm_bf16_ex(pa, pb, gu.data_ptr(), pr, M, N, K, lda, ldb, N, ldr, 0, 0, 0, 1.0, 1, 0, 0, 0, 0, 1, None,
                               act.data_ptr(), N // 2, _stream()), "csm_gemm_bf16_ex(swiglu fwd)")


def linear_dx_swiglu_bwd(dy, w2, gu, dgu):
    """dgu[M,2F] = SwiGLU'(gu) applied to (dy[M,d] w2[d,F]); the intermediate d(act) is never stored."""
    pa, M, K, lda = _mat(dy)
    pb, Kb, F, ldb = _mat(w2)
    assert K == Kb and gu.shape == (M, 2 * F) and dgu.shape == (M, 2 * F) and gu.is_contiguous() and dgu.is_contiguous()
    check(lib.csm_gemm_bf16_ex(pa, pb, dgu.data_ptr(), None, M, F, K, lda, ldb, 2 * F, 0, 0, 1, 0, 1.0, 1, 0, 0, 0, 0, 2,
                               gu.data_ptr(), None, 2 * F, _stream()), "csm_gemm_bf16_ex(swiglu bwd)")


def linear_rope_fwd(x, w, out, table, S, n_rope_cols, head_dim):
    """out[M,N] = x[M,K] w[N,K]^T with RoPE (positions = row % S) applied to columns [0, n_rope_cols) in the GEMM epilogue."""
    pa, M, K, lda = _mat(x)
    pb, N, Kb, ldb = _mat(w)
    assert K == Kb and out.shape == (M, N) and out.dtype == BF16 and out.stride(1) == 1
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] >= S and table.shape[1] * 2 == head_dim
    check(lib.csm_gemm_bf16_rope(pa, pb, out.data_ptr(), M, N, K, lda, ldb, out.stride(0), table.data_ptr(), S, n_rope_cols, head_dim,
                                 _stream()), "csm_gemm_bf16_rope")
    return out


def gemm_kext(A, B, C, xA, xB, R=None, transB=False, rope=None, swiglu_act=None, swiglu_bwd_gu=None, pin=False):
    """C[M,N] = A . opB(B)^T + xA[M,kx] . xB[N,kx]^T (+ R): a frozen projection with its LoRA adapters as extra k-steps of the
    same product.  ``rope`` = (table, S, n_rope_cols, head_dim), ``swiglu_act`` = act[M,N/2] or ``swiglu_bwd_gu`` = gate/up [M,2N]
    (then C = d(gate/up) [M,2N]) select the fused epilogues, which see the sum."""
    pa, M, K, lda = _mat(A)
    pb, b0, b1, ldb = _mat(B)
    N, Kb = (b1, b0) if transB else (b0, b1)
    assert K == Kb, (A.shape, B.shape, transB)
    kx = xA.shape[1]
    assert xA.shape == (M, kx) and xB.shape == (N, kx) and xA.is_contiguous() and xB.is_contiguous() and xA.dtype == BF16 and xB.dtype == BF16
    assert C.shape == (M, 2 * N if swiglu_bwd_gu is not None else N) and C.dtype == BF16 and C.stride(1) == 1
    pr, ldr = (None, 0) if R is None else (R.data_ptr(), R.stride(0))
    assert R is None or (R.shape == (M, N) and R.stride(1) == 1 and R.dtype == BF16)
    epi, aux_in, aux_out, ld_aux, rc, hd = 0, None, None, 0, 0, 0
    if rope is not None:
        table, S, rc, hd = rope
        assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] >= S and table.shape[1] * 2 == hd
        epi, aux_in, ld_aux = 3, table.data_ptr(), S
    elif swiglu_act is not None:
        assert swiglu_act.shape == (M, N // 2) and swiglu_act.is_contiguous() and C.is_contiguous()
        epi, aux_out, ld_aux = 1, swiglu_act.data_ptr(), N // 2
    elif swiglu_bwd_gu is not None:      # the product is d(act) [M,N]; C = d(gate/up) [M,2N] from gate/up [M,2N]
        assert swiglu_bwd_gu.shape == (M, 2 * N) and swiglu_bwd_gu.is_contiguous() and C.is_contiguous() and R is None
        epi, aux_in, ld_aux = 2, swiglu_bwd_gu.data_ptr(), 2 * N
    if pin:                                                   # (see gemm)
        check(lib.csm_gemm_bf16_pinned(pa, pb, C.data_ptr(), pr, M, N, K, lda, ldb, C.stride(0), ldr, 0, int(transB), 1.0, xA.data_ptr(),
                                       xB.data_ptr(), kx, epi, aux_in, aux_out, ld_aux, rc, hd, _stream()), "csm_gemm_bf16_pinned(kext)")
        return C
    check(lib.csm_gemm_bf16_kext(pa, pb, C.data_ptr(), pr, M, N, K, lda, ldb, C.stride(0), ldr, 0, int(transB), xA.data_ptr(),
                                 xB.data_ptr(), kx, epi, aux_in, aux_out, ld_aux, rc, hd, _stream()), "csm_gemm_bf16_kext")
    return C


def skinny_nt(x, wt, out, alpha=1.0, pin=False):
    """out[M,N] = alpha * x[M,K] wt[N,K]^T for N in (32, 64): the bandwidth-shaped product of a LoRA group (falls back to the
    GEMM for other widths)."""
    pa, M, K, lda = _mat(x)
    pb, N, Kb, ldb = _mat(wt)
    assert K == Kb and out.shape == (M, N) and out.dtype == BF16 and out.stride(1) == 1
    if N not in (32, 64) or K % 128:
        return gemm(x, wt, out, None, False, False, alpha, **_pin(pin))
    check(lib.csm_skinny_nt_bf16(pa, pb, out.data_ptr(), M, N, K, lda, ldb, out.stride(0), float(alpha), _stream()), "csm_skinny_nt_bf16")
    return out


def skinny_nt_sel(x, wt, out, sel, blk, alpha=1.0):
    """out[m, n] = alpha * x[m] . wt[n] where sel[m] >= 0 and n // blk == sel[m], +0 elsewhere: ``skinny_nt`` for a stack of LoRA
    adapters whose blocks of ``blk`` columns lie side by side in ``wt`` [N, K] (``sel``: int32 [M] on the device, -1 = no
    adapter).  There is no other route: shapes the kernel does not take are an error."""
    pa, M, K, lda = _mat(x)
    pb, N, Kb, ldb = _mat(wt)
    assert K == Kb and out.shape == (M, N) and out.dtype == BF16 and out.stride(1) == 1 and out.is_cuda
    assert sel.is_cuda and sel.dtype == torch.int32 and sel.shape == (M,) and sel.is_contiguous(), (sel.dtype, sel.shape)
    check(lib.csm_skinny_nt_sel_bf16(pa, pb, out.data_ptr(), sel.data_ptr(), M, N, K, int(blk), lda, ldb, out.stride(0), float(alpha),
                                     _stream()), "csm_skinny_nt_sel_bf16")
    return out


def linear_fwd(x, w, out, residual=None, alpha=1.0, pin=False):
    """out[M,N] = x[M,K] w[N,K]^T (+ residual)."""
    return gemm(x, w, out, residual, False, False, alpha, **_pin(pin))


def linear_dx(dy, w, out, residual=None, alpha=1.0):
    """out[M,K] = dy[M,N] w[N,K] (+ residual)."""
    return gemm(dy, w, out, residual, False, True, alpha)


def linear_dx_dw(dy, w, dx, x, dw, accumulate=False, alpha=1.0, swiglu_gu=None):
    """dx[M,Kin] = dy[M,Nout] w[Nout,Kin] and dw[Nout,Kin] (+)= alpha * dy^T x[M,Kin] in ONE launch (tiles of the two
    products interleaved).  With ``swiglu_gu`` [M, 2 Kin] the first product carries the SwiGLU-backward epilogue and dx is
    d(gate/up) [M, 2 Kin] (w = w2).  Returns False when the shapes do not suit the paired kernel (caller falls back)."""
    M, Nout = dy.shape
    Kin = w.shape[1]
    if M % 64 or Nout % 64 or Kin % 8 or not (dy.stride(1) == w.stride(1) == x.stride(1) == dw.stride(1) == dx.stride(1) == 1):
        return False
    assert w.shape == (Nout, Kin) and x.shape == (M, Kin) and dw.shape == (Nout, Kin), (dy.shape, w.shape, x.shape, dw.shape)
    assert dx.shape == (M, 2 * Kin if swiglu_gu is not None else Kin)
    epi, aux, ld_aux = (0, None, 0) if swiglu_gu is None else (2, swiglu_gu.data_ptr(), swiglu_gu.stride(0))
    check(lib.csm_gemm_bf16_dgrad_wgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), x.data_ptr(), dw.data_ptr(), M, Nout, Kin,
                                        dy.stride(0), w.stride(0), dx.stride(0), x.stride(0), dw.stride(0), epi, aux, ld_aux,
                                        int(accumulate), float(alpha), _stream()), "csm_gemm_bf16_dgrad_wgrad")
    return True


def two_linear_dw(dy1, x1, dw1, dy2, x2, dw2, accumulate=False, alpha=1.0):
    """dw1[N1,K1] (+)= alpha dy1^T x1 and dw2[N2,K2] (+)= alpha dy2^T x2 (same row count M) in ONE launch of 256x256 tiles.
    Returns False when the shapes do not suit it (caller falls back to two linear_dw calls)."""
    M = dy1.shape[0]
    ts = (dy1, x1, dw1, dy2, x2, dw2)
    if M % 64 or dy2.shape[0] != M or any(t.stride(1) != 1 for t in ts) or any(d % 8 for t in ts for d in t.shape[1:]):
        return False
    assert x1.shape[0] == M and x2.shape[0] == M and dw1.shape == (dy1.shape[1], x1.shape[1]) and dw2.shape == (dy2.shape[1], x2.shape[1])
    check(lib.csm_gemm_bf16_two_wgrad(dy1.data_ptr(), x1.data_ptr(), dw1.data_ptr(), dy1.shape[1], x1.shape[1], dy1.stride(0), x1.stride(0),
                                      dw1.stride(0), dy2.data_ptr(), x2.data_ptr(), dw2.data_ptr(), dy2.shape[1], x2.shape[1], dy2.stride(0),
                                      x2.stride(0), dw2.stride(0), M, int(accumulate), float(alpha), _stream()), "csm_gemm_bf16_two_wgrad")
    return True


def multi_linear_dw(problems, accumulate=False, alpha=1.0):
    """dw_i[N_i,K_i] (+)= alpha dy_i^T x_i for a list of (dy_i, x_i, dw_i) sharing the row count M, in ONE launch of 256x256 tiles
    (csm_gemm_bf16_multi_wgrad).  Returns False when the shapes do not suit it (caller falls back to its per-layer launches)."""
    import ctypes as C
    n = len(problems)
    if n < 1 or n > 12:
        return False
    M = problems[0][0].shape[0]
    for dy, x, dw in problems:
        ts = (dy, x, dw)
        if M % 64 or dy.shape[0] != M or x.shape[0] != M or any(t.stride(1) != 1 for t in ts) or any(d % 8 for t in ts for d in t.shape[1:]):
            return False
        assert dw.shape == (dy.shape[1], x.shape[1])
    vp, ip = C.c_void_p * n, C.c_int * n
    check(lib.csm_gemm_bf16_multi_wgrad(n, vp(*[p[0].data_ptr() for p in problems]), vp(*[p[1].data_ptr() for p in problems]),
                                        vp(*[p[2].data_ptr() for p in problems]), ip(*[p[0].shape[1] for p in problems]),
                                        ip(*[p[1].shape[1] for p in problems]), ip(*[p[0].stride(0) for p in problems]),
                                        ip(*[p[1].stride(0) for p in problems]), ip(*[p[2].stride(0) for p in problems]),
                                        M, int(accumulate), float(alpha), _stream()), "csm_gemm_bf16_multi_wgrad")
    return True


_splitk_ws = {}


def linear_dw(dy, x, out, accumulate=False, alpha=1.0):
    """out[N,K] (+)= dy[M,N]^T x[M,K].

    Weight gradients with a small output and a long contraction (attention output projection, every decoder matrix)
    would put a handful of 256x256 tiles on 256 CUs; those are split along the contraction over the GEMM's batch
    dimension into fp32 partial slabs (so that tiles x splits fills the chip) and summed into the bf16 gradient by the
    column-sum kernel."""
    Mrows, N = dy.shape
    Kout = x.shape[1]
    tiles = ((N + 255) // 256) * ((Kout + 255) // 256)
    tiles128 = ((N + 127) // 128) * ((Kout + 127) // 128)
    # measured (tools/probes/wgrad_probe.py): once the 128x128 kernel has >= ~320 tiles for its 512 workgroup slots the
    # direct GEMM beats slabs + column sum (fused-qkv dW: 126 vs 160 us); below that the split wins (o_proj dW: 108 vs 132)
    # (round 3, four-wave kernel: half a round of 256x256 tiles - the depth decoder's w2 gradient, 128 tiles - is better split in
    # two than given to the 128x128 kernel: 261 vs 295 us)
    if (tiles <= 96 and tiles128 < 320 or 96 < tiles <= 128) and Mrows >= 4096 and out.is_contiguous() and Mrows % 64 == 0:
        splits = 1
        while tiles * splits * 2 <= 256 and (Mrows // (splits * 2)) % 64 == 0 and Mrows // (splits * 2) >= 512:
            splits *= 2
        if splits > 1:
            chunk = Mrows // splits
            key = (splits, N, Kout, dy.device)
            ws = _splitk_ws.get(key)
            if ws is None:
                ws = _splitk_ws[key] = torch.empty(splits, N * Kout, dtype=torch.float32, device=dy.device)
            gemm(dy[:chunk], x[:chunk], ws[0].view(N, Kout), None, True, True, alpha, batch=splits,
                 sA=chunk * dy.stride(0), sB=chunk * x.stride(0), sC=N * Kout)
            colsum_bf16(ws, out.view(-1), accumulate=accumulate)
            return out
    return gemm(dy, x, out, out if accumulate else None, True, True, alpha)


def rmsnorm_fwd(x, scale, y, rstd, eps=1e-5):
    M, D = x.shape
    check(lib.csm_rmsnorm_fwd(x.data_ptr(), scale.data_ptr(), y.data_ptr(), _ptr(rstd), M, D, eps, _stream()), "csm_rmsnorm_fwd")
    return y


def rmsnorm_bwd(x, scale, rstd, dy, dx, dres=None, dscale_partials=None):
    M, D = x.shape
    check(lib.csm_rmsnorm_bwd(x.data_ptr(), scale.data_ptr(), rstd.data_ptr(), dy.data_ptr(), _ptr(dres), dx.data_ptr(),
                              _ptr(dscale_partials), M, D, _stream()), "csm_rmsnorm_bwd")
    return dx


def colsum_bf16(partials, dst, accumulate=False):
    rows, D = partials.shape
    check(lib.csm_colsum_bf16(partials.data_ptr(), rows, D, dst.data_ptr(), int(accumulate), _stream()), "csm_colsum_bf16")


def colsum_bf16_multi(pairs, accumulate=False):
    """dst_i (+)= column sums of partials_i for a list of (partials_i [rows, D] fp32, dst_i [D] bf16) of one shape: one launch per
    8 pairs, the arithmetic of colsum_bf16 per pair."""
    import ctypes as C
    rows, D = pairs[0][0].shape
    assert all(p.shape == (rows, D) and p.is_contiguous() and d.numel() == D for p, d in pairs)
    for i in range(0, len(pairs), 8):
        chunk = pairs[i:i + 8]
        n = len(chunk)
        vp = C.c_void_p * n
        check(lib.csm_colsum_bf16_multi(n, vp(*[p.data_ptr() for p, _ in chunk]), vp(*[d.data_ptr() for _, d in chunk]), rows, D,
                                        int(accumulate), _stream()), "csm_colsum_bf16_multi")


def dropout_bf16(x, out, p, seed, accumulate=False):
    """out (+)= dropout(x, p) on [M, D] bf16 row-strided matrices; the mask depends only on (seed, row*D + col)."""
    M, D = x.shape
    assert out.shape == x.shape and x.stride(1) == 1 and out.stride(1) == 1
    check(lib.csm_dropout_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, D, float(p), int(seed) & (2 ** 64 - 1),
                               int(accumulate), _stream()), "csm_dropout_bf16")
    return out


def bias_add_bf16(y, bias):
    M, D = y.shape
    assert y.stride(1) == 1 and bias.numel() == D and bias.is_contiguous()
    check(lib.csm_bias_add_bf16(y.data_ptr(), y.stride(0), bias.data_ptr(), M, D, _stream()), "csm_bias_add_bf16")


def bias_grad_bf16(dy, gbias, accumulate=True, slices=64):
    """gbias (+)= sum over rows of dy [M, D] (bf16, row-strided), fp32 accumulation in two stages."""
    M, D = dy.shape
    assert dy.stride(1) == 1
    slices = max(1, min(slices, (M + 3) // 4))
    part = torch.empty(slices, D, dtype=torch.float32, device=dy.device)
    check(lib.csm_colsum_rows_bf16(dy.data_ptr(), dy.stride(0), M, D, part.data_ptr(), slices, _stream()), "csm_colsum_rows_bf16")
    colsum_bf16(part, gbias, accumulate=accumulate)


def rope(qkv, table, S, n_heads_qk, head_dim, pos=None, inverse=False):
    M, ld = qkv.shape
    assert table.dtype == torch.float32 and table.is_contiguous()
    check(lib.csm_rope(qkv.data_ptr(), table.data_ptr(), _ptr(pos), M, S, n_heads_qk, head_dim, qkv.stride(0), int(inverse),
                       _stream()), "csm_rope")
    return qkv


def attn_fwd(qkv, out, lse, B, S, H, KV, HD):
    assert qkv.is_contiguous() and out.is_contiguous() and qkv.shape == (B * S, (H + 2 * KV) * HD)
    check(lib.csm_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, S, H, KV, HD, _stream()), "csm_attn_fwd")
    return out


def attn_bwd(qkv, out, dout, lse, dqkv, delta_ws, B, S, H, KV, HD, rope_table=None):
    """dqkv = gradient of the (rotated) q | k | v rows; with ``rope_table`` the RoPE backward is applied in the dQ / dK
    epilogues and dqkv is the gradient of the un-rotated projection output (positions = row index in the sequence)."""
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    need = lib.csm_attn_bwd_workspace_bytes(B, S, H)
    assert delta_ws.dtype == torch.float32 and delta_ws.is_contiguous() and delta_ws.numel() * 4 >= need, f"delta_ws: {need} bytes of scratch"
    if rope_table is None:
        check(lib.csm_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                               delta_ws.data_ptr(), B, S, H, KV, HD, _stream()), "csm_attn_bwd")
    else:
        assert rope_table.dtype == torch.float32 and rope_table.is_contiguous() and rope_table.shape[0] >= S
        check(lib.csm_attn_bwd_rope(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                    delta_ws.data_ptr(), rope_table.data_ptr(), B, S, H, KV, HD, _stream()), "csm_attn_bwd_rope")
    return dqkv


def _seg_array(t, B, S):
    assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B * S, "segment array: int32 [B*S] on the device"
    return t.data_ptr()


def attn_fwd_seg(qkv, out, lse, seg_start, B, S, H, KV, HD):
    """attn_fwd on packed rows: key j is visible to query i iff seg_start[i] <= j <= i (int32 [B*S], row-local).  head_dim 64."""
    assert qkv.is_contiguous() and out.is_contiguous() and qkv.shape == (B * S, (H + 2 * KV) * HD)
    check(lib.csm_attn_fwd_seg(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), _seg_array(seg_start, B, S), B, S, H, KV, HD, _stream()),
          "csm_attn_fwd_seg")
    return out


def attn_bwd_seg(qkv, out, dout, lse, dqkv, delta_ws, seg_start, seg_end, B, S, H, KV, HD):
    """attn_bwd on packed rows (seg_end [B*S]: the last position of the position's segment); dqkv is the gradient of the rotated
    rows - there is no fused RoPE form."""
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    need = lib.csm_attn_bwd_workspace_bytes(B, S, H)
    assert delta_ws.dtype == torch.float32 and delta_ws.is_contiguous() and delta_ws.numel() * 4 >= need, f"delta_ws: {need} bytes of scratch"
    check(lib.csm_attn_bwd_seg(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), delta_ws.data_ptr(),
                               _seg_array(seg_start, B, S), _seg_array(seg_end, B, S), B, S, H, KV, HD, _stream()), "csm_attn_bwd_seg")
    return dqkv


def swiglu_fwd(gu, out):
    M, F2 = gu.shape
    check(lib.csm_swiglu_fwd(gu.data_ptr(), out.data_ptr(), M, F2 // 2, _stream()), "csm_swiglu_fwd")
    return out


def swiglu_bwd(gu, dout, dgu):
    M, F2 = gu.shape
    check(lib.csm_swiglu_bwd(gu.data_ptr(), dout.data_ptr(), dgu.data_ptr(), M, F2 // 2, _stream()), "csm_swiglu_bwd")
    return dgu


def embed_fwd(tokens, mask_u8, text_emb, audio_emb, out, audio_vocab):
    M, K1 = tokens.shape
    assert tokens.dtype == torch.int64 and mask_u8.dtype == torch.uint8 and tokens.is_contiguous() and mask_u8.is_contiguous()
    check(lib.csm_embed_fwd(tokens.data_ptr(), mask_u8.data_ptr(), text_emb.data_ptr(), audio_emb.data_ptr(), out.data_ptr(),
                            M, K1 - 1, out.shape[1], audio_vocab, _stream()), "csm_embed_fwd")
    return out


def embed_bwd_sorted(sorted_rows, src_index, dh, dseq, g_text, g_audio):
    assert sorted_rows.dtype == torch.int64 and src_index.dtype == torch.int64 and sorted_rows.is_contiguous() and src_index.is_contiguous()
    check(lib.csm_embed_bwd_sorted(sorted_rows.data_ptr(), src_index.data_ptr(), sorted_rows.numel(), dh.data_ptr(), _ptr(dseq),
                                   dh.shape[0], g_text.data_ptr(), g_audio.data_ptr(), g_text.shape[0],
                                   g_text.shape[0] + g_audio.shape[0], dh.shape[1], _stream()), "csm_embed_bwd_sorted")


def rows_add_bf16(dst, rows_i32, src, src_stride_rows):
    check(lib.csm_rows_add_bf16(dst.data_ptr(), rows_i32.data_ptr(), src.data_ptr(), rows_i32.numel(), int(src_stride_rows),
                                dst.shape[1], _stream()), "csm_rows_add_bf16")


def rows_take_bf16(table, rows_i32, out):
    """out[n] = table[rows[n]]; table[rows[n]] = 0 (unique rows; negative = padding -> zero row)."""
    assert rows_i32.dtype == torch.int32 and rows_i32.is_contiguous() and out.is_contiguous() and out.shape == (rows_i32.numel(), table.shape[1])
    check(lib.csm_rows_take_bf16(table.data_ptr(), rows_i32.data_ptr(), out.data_ptr(), rows_i32.numel(), table.shape[1], _stream()),
          "csm_rows_take_bf16")
    return out


def decoder_input_fwd(hidden, rows_i32, codes, audio_emb, out, audio_vocab):
    N, K = codes.shape
    assert rows_i32.dtype == torch.int32 and codes.dtype == torch.int64 and codes.is_contiguous()
    check(lib.csm_decoder_input_fwd(hidden.data_ptr(), rows_i32.data_ptr(), codes.data_ptr(), audio_emb.data_ptr(),
                                    out.data_ptr(), N, K, hidden.shape[1], audio_vocab, _stream()), "csm_decoder_input_fwd")
    return out


def ce_fwd_bwd(logits_f32, targets, loss_rows, dlogits, V, grad_scale):
    R, ldl = logits_f32.shape[0], logits_f32.stride(0)
    assert logits_f32.dtype == torch.float32 and targets.dtype == torch.int64 and targets.is_contiguous()
    ldd = dlogits.stride(0) if dlogits is not None else 0
    check(lib.csm_ce_fwd_bwd(logits_f32.data_ptr(), targets.data_ptr(), loss_rows.data_ptr(), _ptr(dlogits), R, V, ldl, ldd,
                             float(grad_scale), _stream()), "csm_ce_fwd_bwd")


def reduce_sum(x_f32, out_f32, scale=1.0):
    check(lib.csm_reduce_sum_f32(x_f32.data_ptr(), x_f32.numel(), float(scale), out_f32.data_ptr(), _stream()), "csm_reduce_sum_f32")


def sumsq_blocks() -> int:
    return lib.csm_sumsq_blocks()


def sumsq_bf16(g, partials):
    check(lib.csm_sumsq_bf16(g.data_ptr(), g.numel(), partials.data_ptr(), _stream()), "csm_sumsq_bf16")


def clip_coef(partials, max_norm, norm_and_coef):
    check(lib.csm_clip_coef(partials.data_ptr(), partials.numel(), float(max_norm), norm_and_coef.data_ptr(), _stream()), "csm_clip_coef")


ADAMW_BLOCK = 2048                     # elements per ``block_live`` flag of the flagged AdamW entries


def _live_ptr(block_live, n):
    assert block_live.dtype == torch.uint8 and block_live.is_contiguous() and block_live.numel() == -(-n // ADAMW_BLOCK)
    return block_live.data_ptr()


def adamw_step(master, m, v, param, grad, lr, beta1, beta2, eps, wd, step, norm_and_coef=None, grad_mul=1.0, zero_grad=False, *,
               block_live=None):
    """``block_live`` (uint8, one per 2048 elements, 0 = "m and v of this block are all-zero bits"): blocks that are not live and
    get an all-zero gradient only have their weights decayed; same bits out as without it (csm_adamw_step_live)."""
    n = master.numel()
    assert master.dtype == torch.float32 and param.dtype == BF16 and grad.dtype == BF16 and param.numel() == n == grad.numel()
    args = (master.data_ptr(), m.data_ptr(), v.data_ptr(), param.data_ptr(), grad.data_ptr(), n, lr, beta1, beta2, eps, wd, int(step),
            _ptr(norm_and_coef), float(grad_mul), int(zero_grad))
    if block_live is None:
        check(lib.csm_adamw_step(*args, _stream()), "csm_adamw_step")
    else:
        check(lib.csm_adamw_step_live(*args, _live_ptr(block_live, n), _stream()), "csm_adamw_step_live")


def adamw_step_split(master_lo, m, v, param, grad, lr, beta1, beta2, eps, wd, step, norm_and_coef=None, grad_mul=1.0, zero_grad=False, *,
                     block_live=None):
    n = master_lo.numel()
    assert master_lo.dtype == torch.int16 and param.dtype == BF16 and grad.dtype == BF16 and param.numel() == n == grad.numel()
    args = (master_lo.data_ptr(), m.data_ptr(), v.data_ptr(), param.data_ptr(), grad.data_ptr(), n, lr, beta1, beta2, eps, wd, int(step),
            _ptr(norm_and_coef), float(grad_mul), int(zero_grad))
    if block_live is None:
        check(lib.csm_adamw_step_split(*args, _stream()), "csm_adamw_step_split")
    else:
        check(lib.csm_adamw_step_split_live(*args, _live_ptr(block_live, n), _stream()), "csm_adamw_step_split_live")


def gemv(x, W, y, residual=None):
    """y[B,N] = x[B,K] W[N,K]^T (+ residual), B <= 16.  B <= 4: the VALU kernels, each row bit-equal to a one-row launch;
    B = 5..16 (K % 32 == 0): the MFMA kernel, each row bit-equal across every B in 5..16, position and batch-mate."""
    B, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K and y.shape == (B, N) and x.stride(1) == 1 and W.stride(1) == 1 and y.stride(1) == 1
    check(lib.csm_gemv_bf16(x.data_ptr(), W.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K, W.stride(0), x.stride(0),
                            y.stride(0), int(y.dtype == torch.float32), _stream()), "csm_gemv_bf16")
    return y


def _gemv_dims(x, W, y, swiglu, row_index):
    """(B, N, K) of an extended or fused decode product, after the asserts its wrappers share: the shapes (y is [B, N/2] under
    SwiGLU), unit inner strides and the ``row_index`` gather."""
    B = y.shape[0]
    K = x.shape[1]
    N = W.shape[0]
    assert W.shape[1] == K and y.shape == (B, N // 2 if swiglu else N) and x.stride(1) == 1 and W.stride(1) == 1 and y.stride(1) == 1
    assert row_index is not None or x.shape[0] == B
    assert row_index is None or (row_index.dtype == torch.int32 and row_index.numel() == B and row_index.is_contiguous())
    return B, N, K


def _ext_rows_args(B, ext_t, Bx_tab, bias_tab, row_adapter, kx, ldb):
    """The trailing arguments of the ``*_kext_rows`` entry points (extension operand, adapter tables, stream), after the
    asserts on them."""
    A = Bx_tab.numel()
    assert ext_t.shape[0] == B and ext_t.shape[1] >= kx and ext_t.stride(1) == 1 and ext_t.dtype == BF16
    assert Bx_tab.dtype == torch.int64 and Bx_tab.is_contiguous() and Bx_tab.is_cuda
    assert bias_tab is None or (bias_tab.dtype == torch.int64 and bias_tab.numel() == A and bias_tab.is_contiguous() and bias_tab.is_cuda)
    assert row_adapter.dtype == torch.int32 and row_adapter.numel() == B and row_adapter.is_contiguous() and row_adapter.is_cuda
    return (ext_t.data_ptr(), Bx_tab.data_ptr(), _ptr(bias_tab), row_adapter.data_ptr(), A, int(kx), ext_t.stride(0), int(ldb),
            _stream())


def gemv_ex(x, W, y, residual=None, norm_scale=None, eps=1e-5, swiglu=False, row_index=None, row_offset=0):
    """gemv with an RMSNorm prologue on x (norm_scale), the SwiGLU pairing of interleaved gate/up rows (y is [B, N/2]) and /
    or x gathered from a table: batch row b = x[row_index[b] + row_offset] (row_index int32 [B] on the device).  B <= 16 as
    for ``gemv`` (every fusion on both kernel families)."""
    B, N, K = _gemv_dims(x, W, y, swiglu, row_index)
    check(lib.csm_gemv_bf16_ex(x.data_ptr(), W.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K, W.stride(0), x.stride(0),
                               y.stride(0), int(y.dtype == torch.float32), _ptr(norm_scale), float(eps), int(swiglu),
                               _ptr(row_index), int(row_offset), _stream()), "csm_gemv_bf16_ex")
    return y


def quantize_rows_fp8(W, W8=None, scale=None):
    """W bf16 [N, K] -> (W8 uint8 [N, K] of OCP e4m3fn codes, scale fp32 [N]): per row scale = max|w| / 448 (1.0 for an all-zero
    row), code = e4m3fn(w / scale), round to nearest even, saturating (csm_quantize_rows_fp8; csm/quant.py restates the rule in
    torch and agrees bit for bit).  Rows keep W's order."""
    assert W.is_cuda and W.dtype == BF16 and W.dim() == 2 and W.stride(1) == 1, (W.dtype, W.shape, W.stride())
    N, K = W.shape
    if W8 is None:
        W8 = torch.empty(N, (K + 15) // 16 * 16, dtype=torch.uint8, device=W.device)[:, :K]     # (16-byte aligned rows)
    if scale is None:
        scale = torch.empty(N, dtype=torch.float32, device=W.device)
    assert W8.dtype == torch.uint8 and W8.shape == (N, K) and W8.stride(1) == 1 and scale.dtype == torch.float32 and scale.numel() == N
    check(lib.csm_quantize_rows_fp8(W.data_ptr(), W8.data_ptr(), scale.data_ptr(), N, K, W.stride(0), W8.stride(0), _stream()),
          "csm_quantize_rows_fp8")
    return W8, scale


def gemv_fp8w(x, W8, scale, y, residual=None, norm_scale=None, eps=1e-5, swiglu=False, row_index=None, row_offset=0):
    """``gemv_ex`` with e4m3 weights and one fp32 scale per output row (``quantize_rows_fp8``): y[b][n] = epilogue(scale[n] *
    sum_k x^[b][k] q[n][k]), bf16 activations, fp32 products and sum, the scale applied once after the reduction.  Same fusions,
    same B <= 16 and the same bit-level invariants as the bf16 products; K % 16 == 0, 16-byte aligned weight rows."""
    B, N, K = _gemv_dims(x, W8, y, swiglu, row_index)
    assert W8.dtype == torch.uint8 and scale.dtype == torch.float32 and scale.numel() == N and scale.is_contiguous() and x.dtype == BF16
    check(lib.csm_gemv_fp8w(x.data_ptr(), W8.data_ptr(), scale.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K, W8.stride(0),
                            x.stride(0), y.stride(0), int(y.dtype == torch.float32), _ptr(norm_scale), float(eps), int(swiglu),
                            _ptr(row_index), int(row_offset), _stream()), "csm_gemv_fp8w")
    return y


def gemv_fp8w_kext_rows(x, W8, scale, y, ext_t, Bx_tab, row_adapter, kx, ldb, residual=None, norm_scale=None, eps=1e-5, swiglu=False,
                        row_index=None, row_offset=0, bias_tab=None):
    """``gemv_fp8w`` with row b extended by its own adapter a = row_adapter[b] (the bank of ``gemv_kext_rows`` on the quantised
    base): y = epilogue(scale[n] * x^ q^T + ext_t[b] Bx[a]^T + bias[a]) - the scale on the base sum only, the extension added in
    fp32 after it.  Tables as for ``gemv_kext_rows``.  B = 1..16: B <= 4 row b is the bits of the one-row launch with adapter a;
    5..16 a row's bits depend on its own operands only; a row without adapter is the plain ``gemv_fp8w`` at the same B."""
    B, N, K = _gemv_dims(x, W8, y, swiglu, row_index)
    assert W8.dtype == torch.uint8 and scale.dtype == torch.float32 and scale.numel() == N and scale.is_contiguous() and x.dtype == BF16
    check(lib.csm_gemv_fp8w_kext_rows(x.data_ptr(), W8.data_ptr(), scale.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K,
                                      W8.stride(0), x.stride(0), y.stride(0), int(y.dtype == torch.float32), _ptr(norm_scale),
                                      float(eps), int(swiglu), _ptr(row_index), int(row_offset),
                                      *_ext_rows_args(B, ext_t, Bx_tab, bias_tab, row_adapter, kx, ldb)), "csm_gemv_fp8w_kext_rows")
    return y

def lora_project(x, At, t, scale, norm_scale=None, eps=1e-5):
    """t[B, kx] = scale * x^ At (bf16), x^ = x or its RMSNorm (norm_scale): the extension operand of ``gemv_kext`` for a LoRA
    group whose At [K, kx] is read in place (training/lora.py)."""
    B, K = x.shape
    kx = At.shape[1]
    assert At.shape[0] == K and t.shape == (B, kx) and x.stride(1) == 1 and At.stride(1) == 1 and t.stride(1) == 1
    assert x.dtype == At.dtype == t.dtype == BF16
    check(lib.csm_lora_project_bf16(x.data_ptr(), At.data_ptr(), t.data_ptr(), B, K, kx, x.stride(0), At.stride(0), t.stride(0),
                                    float(scale), _ptr(norm_scale), float(eps), _stream()), "csm_lora_project_bf16")
    return t


def gemv_kext(x, W, y, ext_t, ext_B, residual=None, norm_scale=None, eps=1e-5, swiglu=False, row_index=None, row_offset=0,
              bias=None):
    """``gemv_ex`` with a LoRA group as K-extension: y = epilogue(x^ W^T + ext_t ext_B^T + bias).  ext_t [B, kx] from
    ``lora_project``; ext_B [N, kx] and bias [N] in W's row order."""
    B, N, K = _gemv_dims(x, W, y, swiglu, row_index)
    kx = ext_B.shape[1]
    assert ext_t.shape == (B, kx) and ext_B.shape[0] == N and ext_t.stride(1) == 1 and ext_B.stride(1) == 1
    assert bias is None or (bias.shape == (N,) and bias.is_contiguous() and bias.dtype == BF16)
    check(lib.csm_gemv_bf16_kext(x.data_ptr(), W.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K, W.stride(0), x.stride(0),
                                 y.stride(0), int(y.dtype == torch.float32), _ptr(norm_scale), float(eps), int(swiglu),
                                 _ptr(row_index), int(row_offset), ext_t.data_ptr(), ext_B.data_ptr(), kx, ext_t.stride(0),
                                 ext_B.stride(0), _ptr(bias), _stream()), "csm_gemv_bf16_kext")
    return y


def lora_project_rows(x, At_tab, t, row_adapter, scale, kx, lda, norm_scale=None, eps=1e-5):
    """``lora_project`` with one adapter per batch row (a bank of adapters, csm/lora_bank.py): t[b] = scale[a] * x^[b] At[a],
    a = row_adapter[b] (int32 [B] on the device, -1 = none: a zero row).  ``At_tab`` int64 [A] holds the device addresses of the
    adapters' At [K, lda] (16-byte aligned), ``scale`` fp32 [A]; B = 1..16.  Each row is the bits of a one-row ``lora_project``
    with its own At and scale."""
    B, K = x.shape
    A = At_tab.numel()
    assert t.shape[0] == B and t.shape[1] >= kx and x.stride(1) == 1 and t.stride(1) == 1 and x.dtype == t.dtype == BF16
    assert At_tab.dtype == torch.int64 and At_tab.is_contiguous() and At_tab.is_cuda
    assert scale.dtype == torch.float32 and scale.numel() == A and scale.is_contiguous() and scale.is_cuda
    assert row_adapter.dtype == torch.int32 and row_adapter.numel() == B and row_adapter.is_contiguous() and row_adapter.is_cuda
    check(lib.csm_lora_project_rows_bf16(x.data_ptr(), At_tab.data_ptr(), t.data_ptr(), row_adapter.data_ptr(), scale.data_ptr(), A,
                                         B, K, int(kx), x.stride(0), int(lda), t.stride(0), _ptr(norm_scale), float(eps), _stream()),
          "csm_lora_project_rows_bf16")
    return t


def gemv_kext_rows(x, W, y, ext_t, Bx_tab, row_adapter, kx, ldb, residual=None, norm_scale=None, eps=1e-5, swiglu=False,
                   row_index=None, row_offset=0, bias_tab=None):
    """``gemv_ex`` with row b extended by its own adapter a = row_adapter[b]: y = epilogue(x^ W^T + ext_t[b] Bx[a]^T + bias[a]).
    ``Bx_tab`` / ``bias_tab`` int64 [A]: device addresses of each adapter's Bx [N, ldb] (W's row order) and bias [N] (0 = none;
    ``bias_tab`` None = no adapter has one).  B = 1..16: B <= 4 row b is the bits of a one-row ``gemv_kext`` with adapter a; 5..16
    a row's bits depend on its own operands only; a row without adapter is the plain ``gemv_ex`` at the same B."""
    B, N, K = _gemv_dims(x, W, y, swiglu, row_index)
    check(lib.csm_gemv_bf16_kext_rows(x.data_ptr(), W.data_ptr(), y.data_ptr(), _ptr(residual), B, N, K, W.stride(0), x.stride(0),
                                      y.stride(0), int(y.dtype == torch.float32), _ptr(norm_scale), float(eps), int(swiglu),
                                      _ptr(row_index), int(row_offset),
                                      *_ext_rows_args(B, ext_t, Bx_tab, bias_tab, row_adapter, kx, ldb)), "csm_gemv_bf16_kext_rows")
    return y


def attn_decode_rope(qkv, kcache, vcache, out, pos_i32, table, H, KV, HD, pos_host=None):
    """rope(q, new k) + append(new k, v) + one-position attention against the caches, one launch.  ``pos_host``: the position all
    rows share, as a host integer (the depth decoder's step; HD = 128, H = 4 KV, S_max <= 32): the launch that issues every load
    of its prologue at once."""
    B, _, S_max, _ = kcache.shape
    assert table.dtype == torch.float32 and table.is_contiguous()
    if pos_host is not None and HD == 128 and H == 4 * KV and S_max <= 32 and out.is_contiguous():
        check(lib.csm_attn_decode_rope_at(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), int(pos_host),
                                          table.data_ptr(), B, H, KV, HD, S_max, qkv.stride(0), _stream()), "csm_attn_decode_rope_at")
        return out
    check(lib.csm_attn_decode_rope(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), pos_i32.data_ptr(),
                                   table.data_ptr(), B, H, KV, HD, S_max, qkv.stride(0), _stream()), "csm_attn_decode_rope")
    return out


def gemv_attn(qkv, kcache, vcache, pos_i32, table, W, y, residual, H, KV, HD, pos_host=None):
    """A depth-decoder layer's rope + append + attention + output projection (+ residual) in one launch (S_max <= 64,
    HD = 128); bit-identical to ``attn_decode_rope`` followed by ``gemv``.  ``pos_host``: the position as a host integer (B = 1,
    S_max <= 32): the launch that issues every load of its prologue at once."""
    B, _, S_max, _ = kcache.shape
    N = W.shape[0]
    assert table.dtype == torch.float32 and table.is_contiguous() and W.shape[1] == H * HD and W.stride(1) == 1 and y.shape == (B, N)
    if (pos_host is not None and B == 1 and S_max <= 32 and HD == 128 and H * HD == 1024 and H <= 8 and KV <= 2
            and H % 2 == 0 and (H // KV) % 2 == 0):
        assert qkv.is_contiguous() and y.is_contiguous() and (residual is None or residual.is_contiguous())
        check(lib.csm_gemv_attn_at_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), int(pos_host), table.data_ptr(), W.data_ptr(),
                                        y.data_ptr(), _ptr(residual), N, H, KV, HD, S_max, W.stride(0), _stream()), "csm_gemv_attn_at_bf16")
        return y
    check(lib.csm_gemv_attn_bf16(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), pos_i32.data_ptr(), table.data_ptr(),
                                 W.data_ptr(), y.data_ptr(), _ptr(residual), B, N, H, KV, HD, S_max, qkv.stride(0), W.stride(0),
                                 y.stride(0), _stream()), "csm_gemv_attn_bf16")
    return y


def gemv_t(x, W, y):
    """y[B,N] = x[B,K] W[K,N], B <= 4."""
    B, K = x.shape
    N = W.shape[1]
    assert W.shape[0] == K and y.shape == (B, N) and W.stride(1) == 1
    check(lib.csm_gemv_t_bf16(x.data_ptr(), W.data_ptr(), y.data_ptr(), B, N, K, W.stride(0), x.stride(0), y.stride(0),
                              int(y.dtype == torch.float32), _stream()), "csm_gemv_t_bf16")
    return y


def attn_append(qkv, kcache, vcache, out, row, pos0, H, KV, HD):
    """The n = ``qkv.shape[0]`` new positions ``pos0 .. pos0+n-1`` of the sequence in batch row ``row`` of the caches
    ([B, KV, S_max, HD]): appends their K / V rows (q and k already rotated for those positions) and attends every new query to
    cache positions ``0 .. its own``.  A row's bits do not depend on how the new positions are split into launches."""
    B, _, S_max, _ = kcache.shape
    n = qkv.shape[0]
    assert qkv.is_contiguous() and out.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()
    assert qkv.shape == (n, (H + 2 * KV) * HD) and out.shape == (n, H * HD) and vcache.shape == kcache.shape == (B, KV, S_max, HD)
    if not 0 <= int(row) < B:
        raise CsmHipError(f"csm_attn_append failed (code 1): batch row {row} outside the caches ({B} rows)")
    check(lib.csm_attn_append(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), int(row), int(pos0), n, H, KV, HD,
                              S_max, 1.0 / math.sqrt(HD), _stream()), "csm_attn_append")
    return out


def attn_append_rows(qkv, kcache, vcache, out, rows, pos0s, ns, H, KV, HD):
    """``attn_append`` for R <= 16 segments in one launch: segment r is ``ns[r]`` new positions from ``pos0s[r]`` of the sequence
    in batch row ``rows[r]`` of the caches, its q / k / v the next ``ns[r]`` rows of the stacked ``qkv`` [sum ns, ...].  ``rows``,
    ``pos0s`` and ``ns`` are host integers: they travel in the kernel arguments.  Every row has the bits of a one-segment
    ``attn_append`` of its segment."""
    B, _, S_max, _ = kcache.shape
    rows, pos0s, ns = [int(x) for x in rows], [int(x) for x in pos0s], [int(x) for x in ns]
    R, M = len(rows), qkv.shape[0]
    assert qkv.is_contiguous() and out.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()
    assert qkv.shape == (M, (H + 2 * KV) * HD) and out.shape == (M, H * HD) and vcache.shape == kcache.shape == (B, KV, S_max, HD)
    if not (len(pos0s) == len(ns) == R):
        raise CsmHipError(f"csm_attn_append_rows failed (code 1): {R} rows, {len(pos0s)} positions and {len(ns)} lengths")
    for r in rows:
        if not 0 <= r < B:
            raise CsmHipError(f"csm_attn_append_rows failed (code 1): batch row {r} outside the caches ({B} rows)")
    if 1 <= R <= 16 and all(n >= 1 for n in ns) and sum(ns) != M:
        raise CsmHipError(f"csm_attn_append_rows failed (code 1): the segments hold {sum(ns)} positions, qkv has {M} rows")
    arr = ctypes.c_int * max(R, 1)
    check(lib.csm_attn_append_rows(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), arr(*rows), arr(*pos0s),
                                   arr(*ns), R, H, KV, HD, S_max, 1.0 / math.sqrt(HD), _stream()), "csm_attn_append_rows")
    return out


def kv_append(qkv, kcache, vcache, pos_i32, H, KV, HD):
    B, _, S_max, _ = kcache.shape
    check(lib.csm_kv_append(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), pos_i32.data_ptr(), B, H, KV, HD, S_max,
                            qkv.stride(0), _stream()), "csm_kv_append")


def kv_shift(parked, table, keep, drop):
    """The context shift of a parked history ([layers, 2, KV, len, HD] bf16, ``DecodeState.park_row``): a NEW tensor
    [layers, 2, KV, len - drop, HD] without positions ``keep .. keep+drop-1`` - the head and every V copied, the keys behind the
    gap rotated back by ``drop`` positions (csm_kv_shift; row ``drop`` of ``table``, sine negated).  ``parked`` is not touched."""
    assert parked.dim() == 5 and parked.shape[1] == 2 and parked.dtype == BF16 and parked.is_contiguous()
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[1] * 2 == parked.shape[4]
    layers, _, KV, length, HD = parked.shape
    keep, drop = int(keep), int(drop)
    out = torch.empty(layers, 2, KV, max(length - drop, 0), HD, dtype=BF16, device=parked.device)
    check(lib.csm_kv_shift(parked.data_ptr(), out.data_ptr(), table.data_ptr(), table.shape[0], layers, KV, HD, length, keep, drop,
                           _stream()), "csm_kv_shift")
    return out


def kv_fork_rows(parkeds, kv, pos, rows):
    """R <= 16 parked histories (``DecodeState.park_row``: [layers, 2, KV, len_r, HD] bf16, contiguous) into positions
    ``0 .. len_r - 1`` of batch rows ``rows[r]`` of the cache allocation ``kv`` [layers, 2, B, KV, S_max, HD], and ``pos[rows[r]] =
    len_r - 1`` (int32 [B]) - ONE launch (csm_kv_fork_rows), the table in the kernel arguments.  The same tensor may be given for
    several rows; no parked tensor is touched, nor anything of ``kv`` / ``pos`` outside the named rows' leading positions."""
    parkeds, rows = list(parkeds), [int(b) for b in rows]
    R = len(rows)
    if len(parkeds) != R:
        raise CsmHipError(f"csm_kv_fork_rows failed (code 1): {len(parkeds)} parked histories for {R} rows")
    assert kv.dim() == 6 and kv.shape[1] == 2 and kv.dtype == BF16 and kv.is_contiguous()
    layers, _, B, KV, S_max, HD = kv.shape
    assert pos.dtype == torch.int32 and pos.shape == (B,) and pos.is_contiguous() and pos.device == kv.device
    for p in parkeds:
        assert p.dim() == 5 and p.shape[:3] == (layers, 2, KV) and p.shape[4] == HD, f"kv_fork_rows: {tuple(p.shape)} against {tuple(kv.shape)}"
        assert p.dtype == BF16 and p.is_contiguous() and p.device == kv.device
    ptr, arr = ctypes.c_void_p * max(R, 1), ctypes.c_int * max(R, 1)
    check(lib.csm_kv_fork_rows(ptr(*[p.data_ptr() for p in parkeds]), kv.data_ptr(), pos.data_ptr(), arr(*rows),
                               arr(*[p.shape[3] for p in parkeds]), R, layers, B, KV, HD, S_max, _stream()), "csm_kv_fork_rows")


def kv_park_rows(kv, rows, lens):
    """The mirror of ``kv_fork_rows``: positions ``0 .. lens[r] - 1`` of batch rows ``rows[r]`` (R <= 16, distinct) of the cache
    allocation ``kv`` [layers, 2, B, KV, S_max, HD] as R new contiguous tensors [layers, 2, KV, lens[r], HD] - ``DecodeState.
    park_row``'s format - by ONE launch (csm_kv_park_rows), the table in the kernel arguments.  ``kv`` is only read."""
    rows, lens = [int(b) for b in rows], [int(n) for n in lens]
    R = len(rows)
    if len(lens) != R:
        raise CsmHipError(f"csm_kv_park_rows failed (code 1): {len(lens)} lengths for {R} rows")
    assert kv.dim() == 6 and kv.shape[1] == 2 and kv.dtype == BF16 and kv.is_contiguous()
    layers, _, B, KV, S_max, HD = kv.shape
    outs = [torch.empty(layers, 2, KV, max(n, 0), HD, dtype=BF16, device=kv.device) for n in lens]
    ptr, arr = ctypes.c_void_p * max(R, 1), ctypes.c_int * max(R, 1)
    check(lib.csm_kv_park_rows(ptr(*[o.data_ptr() for o in outs]), kv.data_ptr(), arr(*rows), arr(*lens), R, layers, B, KV, HD,
                               S_max, _stream()), "csm_kv_park_rows")
    return outs


def sample_hist_move_rows(code_hist, hist_frame, packed, rows, to_state):
    """The rings ``code_hist[rows[r]]`` (int32 [K, 64] of [B, K, 64]) and counters ``hist_frame[rows[r]]`` of R <= 16 distinct
    rows against row r of ``packed`` int32 [R, K * 64 + 1], by ONE launch (csm_sample_hist_move_rows): ``to_state`` False reads
    the state and writes ``packed``, True reads ``packed`` and writes only the named rows.  Returns ``packed``."""
    rows = [int(b) for b in rows]
    R = len(rows)
    assert code_hist.dim() == 3 and code_hist.dtype == torch.int32 and code_hist.is_contiguous()
    B, K, H = code_hist.shape
    assert hist_frame.dtype == torch.int32 and hist_frame.shape == (B,) and hist_frame.is_contiguous()
    assert packed.dtype == torch.int32 and packed.shape == (R, K * H + 1) and packed.is_contiguous() and packed.device == code_hist.device
    arr = ctypes.c_int * max(R, 1)
    check(lib.csm_sample_hist_move_rows(code_hist.data_ptr(), hist_frame.data_ptr(), packed.data_ptr(), arr(*rows), R, B, K,
                                        int(bool(to_state)), _stream()), "csm_sample_hist_move_rows")
    return packed


def attn_decode(qkv, kcache, vcache, out, pos_i32, H, KV, HD):
    B, _, S_max, _ = kcache.shape
    check(lib.csm_attn_decode(qkv.data_ptr(), kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), pos_i32.data_ptr(), B, H, KV,
                              HD, S_max, qkv.stride(0), _stream()), "csm_attn_decode")
    return out


def sample_topk(logits_f32, q_f32, out_i32, topk, temperature, V=None):
    rows = logits_f32.shape[0]
    V = V or logits_f32.shape[1]
    assert q_f32.is_contiguous() and q_f32.shape == (rows, V)
    check(lib.csm_sample_topk(logits_f32.data_ptr(), q_f32.data_ptr(), out_i32.data_ptr(), rows, V, logits_f32.stride(0),
                              int(topk), float(temperature), _stream()), "csm_sample_topk")
    return out_i32


# per level, as plain tuples (the launch is a hot path): the entry point's name, the dtypes of what it reads, whether it keeps rings
_ROWS = tuple((lv.fn and "csm_" + lv.fn, tuple(p.dtype for p in PARAMS[:lv.reads]), lv.rings) for lv in LEVELS)
_RING_AT = LEVELS[FULL_LEVEL].reads                      # (the entry points take the ring after what the first level with one reads)


def _sample_rows(level, logits_f32, q_f32, out_i32, params, ring=(), advance=False, V=None):
    """The launch of the rows sampler of ``level`` (``sampling.LEVELS``): ``params`` - the parameters its kernel reads, in
    ``sampling.PARAMS``' order, one entry per row each; ``ring`` - (hist, frame, live) where the level keeps the rows' rings."""
    name, dtypes, rings = _ROWS[level]
    rows = logits_f32.shape[0]
    V = V or logits_f32.shape[1]
    assert q_f32.is_contiguous() and q_f32.shape == (rows, V) and len(params) == len(dtypes)
    args = []
    for a, dtype in zip(params, dtypes):
        assert a.dtype == dtype and a.is_contiguous() and a.numel() == rows
        args.append(a.data_ptr())
    args[0], args[1] = args[1], args[0]                  # (the entry points take top-k before the temperature)
    if rings:
        hist_i32, frame, live = ring
        assert frame.dtype == torch.int32 and frame.is_contiguous() and frame.numel() == rows
        assert live.dtype == torch.int32 and live.is_contiguous() and live.numel() == rows
        assert hist_i32.dtype == torch.int32 and hist_i32.dim() == 2 and hist_i32.shape == (rows, 64) and hist_i32.stride(1) == 1
        assert rows == 1 or hist_i32.stride(0) >= 64
        ldh = hist_i32.stride(0) if rows > 1 else 64
        args[_RING_AT:_RING_AT] = (hist_i32.data_ptr(), ldh, frame.data_ptr(), live.data_ptr(), 1 if advance else 0)
    check(getattr(lib, name)(logits_f32.data_ptr(), q_f32.data_ptr(), out_i32.data_ptr(), rows, V, logits_f32.stride(0), *args,
                             _stream()), name)
    return out_i32


def sample_topk_rows(logits_f32, q_f32, out_i32, topk_i32, temperature_f32, V=None):
    """``sample_topk`` with row r's parameters read from ``topk_i32[r]`` / ``temperature_f32[r]`` on the device."""
    return _sample_rows(1, logits_f32, q_f32, out_i32, (temperature_f32, topk_i32), V=V)


def sample_filtered_rows(logits_f32, q_f32, out_i32, topk_i32, temperature_f32, top_p_f32, min_p_f32, V=None):
    """``sample_topk_rows`` with row r's nucleus and min-p thresholds read from ``top_p_f32[r]`` / ``min_p_f32[r]`` on the device
    (``csm_sample_filtered_rows``; a row with 1.0 / 0.0 is ``sample_topk_rows``' row)."""
    return _sample_rows(2, logits_f32, q_f32, out_i32, (temperature_f32, topk_i32, top_p_f32, min_p_f32), V=V)


def sample_processed_rows(logits_f32, q_f32, out_i32, topk_i32, temperature_f32, top_p_f32, min_p_f32, penalty_f32, window_i32,
                          hist_i32, frame_i32, live_i32, advance=False, V=None):
    """``sample_filtered_rows`` with a windowed repetition penalty per row and the row's memory of what it drew
    (``csm_sample_processed_rows``).  ``hist_i32`` [rows, 64] (any row stride >= 64): row r's ring, slot f % 64 the code of frame
    f; ``frame_i32[r]``: f; the ids of the last min(window_i32[r], f, 64) frames are penalised by ``penalty_f32[r]`` before the
    draw.  A row with ``live_i32[r]`` != 0 then stores its winner to slot f % 64 and, with ``advance``, f + 1 to ``frame_i32[r]``.
    A row with penalty 1 or window 0 is ``sample_filtered_rows``' row."""
    return _sample_rows(3, logits_f32, q_f32, out_i32, (temperature_f32, topk_i32, top_p_f32, min_p_f32, penalty_f32, window_i32),
                        (hist_i32, frame_i32, live_i32), advance, V)


def sample_typical_rows(logits_f32, q_f32, out_i32, topk_i32, temperature_f32, top_p_f32, min_p_f32, penalty_f32, window_i32,
                        hist_i32, frame_i32, live_i32, typical_p_f32, advance=False, V=None):
    """``sample_processed_rows`` with locally typical sampling per row (``csm_sample_typical_rows``): after the nucleus, the
    tokens whose surprise -ln P is closest to the entropy of what is left are kept, most typical first, until ``typical_p_f32[r]``
    of the mass is reached (the token that crosses it is kept).  A row with 1.0 is ``sample_processed_rows``' row: out, ring and
    counter."""
    return _sample_rows(4, logits_f32, q_f32, out_i32, (temperature_f32, topk_i32, top_p_f32, min_p_f32, penalty_f32, window_i32,
                                                        typical_p_f32), (hist_i32, frame_i32, live_i32), advance, V)


def sample_stats_rows(logits_f32, codes_i32, logprob=None, entropy=None, pmax=None, V=None):
    """What the model thought of each drawn code (``csm_sample_stats_rows``): row r of ``logits_f32`` [rows, >= V] (any row stride)
    with ``codes_i32[r]`` -> ``logprob[r]`` (log_softmax at the code; -inf for a code outside [0, V)), ``entropy[r]`` (nats) and
    ``pmax[r]`` of softmax(row) - temperature 1, no filter, no penalty.  Each output is an fp32 tensor of ``rows`` elements or
    None (not computed); at least one must be given.  Returns (logprob, entropy, pmax)."""
    assert logits_f32.dim() == 2 and logits_f32.dtype == torch.float32 and logits_f32.stride(1) == 1
    rows = logits_f32.shape[0]
    V = V or logits_f32.shape[1]
    assert codes_i32.dtype == torch.int32 and codes_i32.is_contiguous() and codes_i32.numel() == rows
    ptrs = []
    for o in (logprob, entropy, pmax):
        assert o is None or (o.dtype == torch.float32 and o.is_contiguous() and o.numel() == rows and o.device == logits_f32.device)
        ptrs.append(None if o is None else o.data_ptr())
    ldl = logits_f32.stride(0) if rows > 1 else max(logits_f32.stride(0), V)
    check(lib.csm_sample_stats_rows(logits_f32.data_ptr(), codes_i32.data_ptr(), *ptrs, rows, V, ldl, _stream()),
          "csm_sample_stats_rows")
    return logprob, entropy, pmax


def rvq_encode(x_f32, codebooks_f32, codes_i64, n_semantic=1):
    T, D = x_f32.shape
    K, Cn, D2 = codebooks_f32.shape
    assert D == D2 and codes_i64.shape == (K, T) and x_f32.is_contiguous() and codebooks_f32.is_contiguous()
    check(lib.csm_rvq_encode(x_f32.data_ptr(), codebooks_f32.data_ptr(), codes_i64.data_ptr(), T, K, Cn, D, n_semantic,
                             _stream()), "csm_rvq_encode")
    return codes_i64


def rvq_decode(codes_i64, codebooks_f32, out_f32):
    K, T = codes_i64.shape
    _, Cn, D = codebooks_f32.shape
    check(lib.csm_rvq_decode(codes_i64.data_ptr(), codebooks_f32.data_ptr(), out_f32.data_ptr(), T, K, Cn, D, _stream()),
          "csm_rvq_decode")
    return out_f32


def _f32(t, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (name, t.dtype, t.shape, t.stride())
    return t.data_ptr()


def conv1d_stream_f32(hist, x, w, bias, y, hist_out, dilation=1, elu_in=False, residual=None):
    """One chunk of a causal stride-1 conv (csm_conv1d_stream_f32): x [C_in, n] new columns after ``hist`` [C_in, (k-1)*dil]
    -> y [C_out, n] (+ residual [C_out, n]); the next history goes to ``hist_out`` (same shape as hist, a different buffer).
    hist / hist_out may be None when k == 1.  w: [C_out, C_in/groups, k]."""
    C_in, n = x.shape
    C_out, cin_g, k = w.shape
    H = (k - 1) * dilation
    assert y.shape == (C_out, n) and C_in % cin_g == 0
    if H:
        assert hist.shape == (C_in, H) and hist_out.shape == (C_in, H) and hist.data_ptr() != hist_out.data_ptr()
    check(lib.csm_conv1d_stream_f32(_f32(hist, "hist") if H else None, _f32(x, "x"), _f32(w, "w"),
                                    None if bias is None else _f32(bias, "bias"), None if residual is None else _f32(residual, "res"),
                                    _f32(y, "y"), _f32(hist_out, "hist_out") if H else None, C_in, C_out, n, k, dilation,
                                    C_in // cin_g, int(elu_in), _stream()), "csm_conv1d_stream_f32")
    return y


def conv1d_stream_strided_f32(hist, x, w, bias, y, hist_out, stride, dilation=1, elu_in=False, residual=None, edge_first=False):
    """One chunk of a causal conv with stride >= 1 (csm_conv1d_stream_strided_f32): x [C_in, n_in] new columns (n_in a multiple
    of stride) after ``hist`` [C_in, H], H = (k-1)*dil + 1 - stride -> y [C_out, n_in // stride] (+ residual); the next history
    goes to ``hist_out`` (a different buffer).  ``edge_first``: ``hist`` is not read, every history column is column 0 of x (the
    first chunk of an edge-replicated conv).  hist / hist_out may be None when H == 0.  w: [C_out, C_in/groups, k]."""
    C_in, n_in = x.shape
    C_out, cin_g, k = w.shape
    H = (k - 1) * dilation + 1 - stride
    assert y.shape == (C_out, n_in // stride) and C_in % cin_g == 0
    if H > 0:
        assert hist.shape == (C_in, H) and hist_out.shape == (C_in, H)
    check(lib.csm_conv1d_stream_strided_f32(_f32(hist, "hist") if H > 0 else None, _f32(x, "x"), _f32(w, "w"),
                                            None if bias is None else _f32(bias, "bias"),
                                            None if residual is None else _f32(residual, "res"), _f32(y, "y"),
                                            _f32(hist_out, "hist_out") if H > 0 else None, C_in, C_out, n_in, k, stride, dilation,
                                            C_in // cin_g, int(elu_in), int(edge_first), _stream()), "csm_conv1d_stream_strided_f32")
    return y


def conv_transpose1d_stream_f32(hist, x, w, bias, y, hist_out, pos0, stride, groups=1, elu_in=False):
    """One chunk of a causal transposed conv (csm_conv_transpose1d_stream_f32): x [C_in, n] new columns at input position
    ``pos0`` after ``hist`` [C_in, ceil(k/stride)-1] -> y [C_out, n*stride]; next history to ``hist_out``.
    w: [C_in, C_out/groups, k] (torch layout)."""
    C_in, n = x.shape
    C_in_w, cout_g, k = w.shape
    H = (k - 1) // stride
    C_out = cout_g * groups
    assert C_in_w == C_in and y.shape == (C_out, n * stride)
    if H:
        assert hist.shape == (C_in, H) and hist_out.shape == (C_in, H) and hist.data_ptr() != hist_out.data_ptr()
    check(lib.csm_conv_transpose1d_stream_f32(_f32(hist, "hist") if H else None, _f32(x, "x"), _f32(w, "w"),
                                              None if bias is None else _f32(bias, "bias"), _f32(y, "y"),
                                              _f32(hist_out, "hist_out") if H else None, C_in, C_out, n, int(pos0), k, stride,
                                              groups, int(elu_in), _stream()), "csm_conv_transpose1d_stream_f32")
    return y


def attn_window_stream_f32(qkv, kcache, vcache, out, pos0, heads, window):
    """Sliding-window attention of the n rows of qkv [n, 3*D] (post-RoPE) at positions pos0..pos0+n-1 against the ring caches
    kcache / vcache [ring, D] (position p in slot p % ring), appending the new k / v rows (csm_attn_window_stream_f32).
    out: [n, D].  Needs ring >= window + n - 1."""
    n, D3 = qkv.shape
    ring, D = kcache.shape
    assert D3 == 3 * D and vcache.shape == (ring, D) and out.shape == (n, D)
    check(lib.csm_attn_window_stream_f32(_f32(qkv, "qkv"), _f32(kcache, "kcache"), _f32(vcache, "vcache"), _f32(out, "out"), n,
                                         int(pos0), heads, D // heads, window, ring, _stream()), "csm_attn_window_stream_f32")
    return out


def _ints(values):
    """A host int array for the rows ops (they hand it to the kernel by value: nothing is copied to the device)."""
    import ctypes
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def conv1d_stream_rows_f32(arena, x, w, bias, y, slots, parity, dilation=1, elu_in=False, residual=None):
    """``conv1d_stream_f32`` for R rows in one launch (csm_conv1d_stream_rows_f32): x [R, C_in, n] -> y [R, C_out, n]
    (+ residual [R, C_out, n]).  ``arena`` [n_slots, 2, C_in, H] holds both history buffers of every slot (None when k == 1):
    row r reads buffer ``parity[r]`` of slot ``slots[r]`` and writes the next history to the other one."""
    R, C_in, n = x.shape
    C_out, cin_g, k = w.shape
    H = (k - 1) * dilation
    assert y.shape == (R, C_out, n) and C_in % cin_g == 0 and len(slots) == len(parity) == R
    n_slots = arena.shape[0] if H else max(slots) + 1
    if H:
        assert arena.shape[1:] == (2, C_in, H)
    check(lib.csm_conv1d_stream_rows_f32(_f32(arena, "arena") if H else None, _f32(x, "x"), _f32(w, "w"),
                                         None if bias is None else _f32(bias, "bias"), None if residual is None else _f32(residual, "res"),
                                         _f32(y, "y"), R, _ints(slots), _ints(parity), n_slots, C_in, C_out, n, k, dilation, C_in // cin_g,
                                         int(elu_in), _stream()), "csm_conv1d_stream_rows_f32")
    return y


def conv1d_stream_strided_rows_f32(arena, x, w, bias, y, slots, parity, stride, dilation=1, elu_in=False, residual=None,
                                   edge_first=()):
    """``conv1d_stream_strided_f32`` for R rows in one launch (csm_conv1d_stream_strided_rows_f32): x [R, C_in, n_in] ->
    y [R, C_out, n_in // stride] (+ residual of that shape).  ``arena`` [n_slots, 2, C_in, H], H = (k-1)*dil + 1 - stride (None
    when H == 0), read and written as by ``conv1d_stream_rows_f32``.  ``edge_first``: one flag per row (or empty = none); a
    flagged row does not read its history, every history column is column 0 of its x."""
    R, C_in, n_in = x.shape
    C_out, cin_g, k = w.shape
    H = (k - 1) * dilation + 1 - stride
    assert y.shape == (R, C_out, n_in // stride) and C_in % cin_g == 0 and len(slots) == len(parity) == R
    assert len(edge_first) in (0, R)
    n_slots = arena.shape[0] if H > 0 else max(slots) + 1
    if H > 0:
        assert arena.shape[1:] == (2, C_in, H)
    mask = sum(1 << r for r, e in enumerate(edge_first) if e)
    check(lib.csm_conv1d_stream_strided_rows_f32(_f32(arena, "arena") if H > 0 else None, _f32(x, "x"), _f32(w, "w"),
                                                 None if bias is None else _f32(bias, "bias"),
                                                 None if residual is None else _f32(residual, "res"), _f32(y, "y"), R, _ints(slots),
                                                 _ints(parity), mask, n_slots, C_in, C_out, n_in, k, stride, dilation, C_in // cin_g,
                                                 int(elu_in), _stream()), "csm_conv1d_stream_strided_rows_f32")
    return y


def conv_transpose1d_stream_rows_f32(arena, x, w, bias, y, slots, parity, pos0, stride, groups=1, elu_in=False):
    """``conv_transpose1d_stream_f32`` for R rows in one launch: x [R, C_in, n] at input positions ``pos0[r]`` ->
    y [R, C_out, n*stride]; ``arena`` [n_slots, 2, C_in, ceil(k/stride)-1] as for ``conv1d_stream_rows_f32``."""
    R, C_in, n = x.shape
    C_in_w, cout_g, k = w.shape
    H = (k - 1) // stride
    C_out = cout_g * groups
    assert C_in_w == C_in and y.shape == (R, C_out, n * stride) and len(slots) == len(parity) == len(pos0) == R
    n_slots = arena.shape[0] if H else max(slots) + 1
    if H:
        assert arena.shape[1:] == (2, C_in, H)
    check(lib.csm_conv_transpose1d_stream_rows_f32(_f32(arena, "arena") if H else None, _f32(x, "x"), _f32(w, "w"),
                                                   None if bias is None else _f32(bias, "bias"), _f32(y, "y"), R, _ints(slots),
                                                   _ints(parity), _ints(pos0), n_slots, C_in, C_out, n, k, stride, groups, int(elu_in),
                                                   _stream()), "csm_conv_transpose1d_stream_rows_f32")
    return y


def rope_half_rows_f32(qkv, pos0, n, heads, base):
    """Rotate-half RoPE in place on qkv [R*n, 3*D]: row r's n positions start at ``pos0[r]`` (csm_rope_half_rows_f32)."""
    R = len(pos0)
    T, D3 = qkv.shape
    assert T == R * n
    check(lib.csm_rope_half_rows_f32(_f32(qkv, "qkv"), R, _ints(pos0), n, heads, D3 // 3 // heads, float(base), _stream()),
          "csm_rope_half_rows_f32")
    return qkv


def attn_window_stream_rows_f32(qkv, kcache, vcache, out, slots, pos0, n, heads, window):
    """``attn_window_stream_f32`` for R rows in one launch: qkv [R*n, 3*D], out [R*n, D], ring caches [n_slots, ring, D]; row r
    sits at positions pos0[r] .. pos0[r]+n-1 of slot slots[r].  Needs ring >= window + n - 1."""
    R = len(slots)
    T, D3 = qkv.shape
    n_slots, ring, D = kcache.shape
    assert T == R * n and D3 == 3 * D and vcache.shape == kcache.shape and out.shape == (T, D) and len(pos0) == R
    check(lib.csm_attn_window_stream_rows_f32(_f32(qkv, "qkv"), _f32(kcache, "kcache"), _f32(vcache, "vcache"), _f32(out, "out"), R,
                                              _ints(slots), _ints(pos0), n_slots, n, heads, D // heads, window, ring, _stream()),
          "csm_attn_window_stream_rows_f32")
    return out


def transpose_rows_f32(x, y):
    """y[b] = x[b]^T for x [batch, R, C] (csm_transpose_rows_f32)."""
    b, R, Cn = x.shape
    assert y.shape == (b, Cn, R)
    check(lib.csm_transpose_rows_f32(_f32(x, "x"), _f32(y, "y"), b, R, Cn, _stream()), "csm_transpose_rows_f32")
    return y


def resample_f32(x, taps, y, o, n, width):
    """One-shot band-limited resampling (csm_resample_f32): x [R, N] -> y [R, ceil(n*N/o)] with the polyphase table ``taps``
    [n, 2*width + o] of the reduced rate pair o / n (``csm.codec.resample.design``)."""
    R, N = x.shape
    assert taps.shape == (n, 2 * width + o) and y.shape == (R, -(-n * N // o))
    check(lib.csm_resample_f32(_f32(x, "x") if N else None, _f32(taps, "taps"), _f32(y, "y") if N else None, R, N, o, n, width,
                               _stream()), "csm_resample_f32")
    return y


def resample_stream_rows_f32(arena, xs, taps, y, slots, parity, pos, final, max_in, o, n, width):
    """R streams in one launch (csm_resample_stream_rows_f32): row r feeds the 1-D fp32 tensor ``xs[r]`` (None or empty: nothing
    new - only with its ``final`` flag) to the stream of slot ``slots[r]`` that has seen ``pos[r]`` samples; ``arena``
    [n_slots, 2, T - 1] holds the carries, ``y`` [R, ldy] receives each row's new outputs from column 0.  Slots, parities,
    lengths, positions and the rows' device pointers travel by value."""
    R = len(slots)
    T = 2 * width + o
    assert len(xs) == len(parity) == len(pos) == R and arena.shape[1:] == (2, T - 1) and taps.shape == (n, T)
    assert len(final) in (0, R) and y.dim() == 2 and y.shape[0] == R
    n_in = [0 if x is None else x.numel() for x in xs]
    ptrs = (ctypes.c_void_p * R)(*[_f32(x, "x") if k else None for x, k in zip(xs, n_in)])
    mask = sum(1 << r for r, f in enumerate(final) if f)
    check(lib.csm_resample_stream_rows_f32(_f32(arena, "arena"), ptrs, _f32(taps, "taps"), _f32(y, "y") if y.numel() else None,
                                           y.shape[1], R, _ints(slots), _ints(parity), _ints(n_in),
                                           (ctypes.c_longlong * R)(*[int(p) for p in pos]), mask, arena.shape[0], int(max_in), o, n,
                                           width, _stream()), "csm_resample_stream_rows_f32")
    return y


def resample_stream_f32(carry, parity, x, pos, final, taps, y, max_in, o, n, width):
    """One stream (csm_resample_stream_f32): ``carry`` [2, T - 1], ``x`` the next samples (None: a flush), ``y`` [>= outputs]."""
    T = 2 * width + o
    assert carry.shape == (2, T - 1) and taps.shape == (n, T) and y.dim() == 1
    k = 0 if x is None else x.numel()
    check(lib.csm_resample_stream_f32(_f32(carry, "carry"), int(parity), _f32(x, "x") if k else None, k, int(pos), int(bool(final)),
                                      _f32(taps, "taps"), _f32(y, "y") if y.numel() else None, y.numel(), int(max_in), o, n, width,
                                      _stream()), "csm_resample_stream_f32")
    return y


def resample(x, orig_sr, new_sr):
    """``csm.data.resample`` on the device: x [..., N] fp32 -> [..., ceil(N * new_sr / orig_sr)] (``csm.codec.resample``)."""
    from ..codec.resample import get_resampler
    return get_resampler(orig_sr, new_sr, x.device)(x)
