"""Weight-only FP8 (OCP e4m3fn) quantisation, one fp32 scale per output row: the rule of ``csm_quantize_rows_fp8``
(include/csm_hip.h) restated in plain torch.  It runs anywhere (CPU included), agrees bit for bit with the HIP quantiser and is
what the tests compare it to; use it to prepare or inspect decode weights offline.

Per row of W [N, K]:  amax = max |w|,  scale = amax / 448 (fp32 division; 1.0 for an all-zero row),
code = e4m3fn(clamp(w / scale, -448, 448)), round to nearest even.  The clamp makes the conversion saturating (a plain torch
cast of 500.0 to float8_e4m3fn is NaN), so finite weights never give a NaN code.  Dequantised weight: ``code.float() * scale``.
"""
import torch

E4M3_MAX = 448.0
F8 = torch.float8_e4m3fn


def quantize_rows_fp8(W: torch.Tensor):
    """W [N, K] (bf16 or fp32, finite) -> (codes uint8 [N, K] holding e4m3fn bit patterns, scale fp32 [N])."""
    if W.dim() != 2:
        raise ValueError(f"quantize_rows_fp8: a 2-D matrix is needed (got {tuple(W.shape)})")
    w = W.detach().float()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_rows_fp8: the weights must be finite")
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    q = (w / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(F8)
    return q.view(torch.uint8), scale


def dequantize_rows_fp8(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """(codes uint8 [N, K], scale fp32 [N]) -> fp32 [N, K], exactly the numbers the FP8 decode products multiply with."""
    return codes.view(F8).float() * scale.float()[:, None]


def snap_rows_to_fp8_grid(W: torch.Tensor) -> torch.Tensor:
    """Weights that FP8 mode represents EXACTLY (test helper): per row s = 2^ceil(log2(amax / 448)), w' = e4m3(w / s) * s, then
    w'[0] = 448 s.  Every w' is exact in bf16, the quantiser's scale for the row is exactly s and quantising w' returns it."""
    w = W.detach().float()
    amax = w.abs().amax(dim=1).clamp_min(2.0 ** -100)
    s = torch.exp2(torch.ceil(torch.log2(amax / E4M3_MAX)))
    s = torch.where(s * E4M3_MAX < amax, s * 2, s)                 # (log2's rounding must not leave amax above 448 s)
    q = (w / s[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(F8).float() * s[:, None]
    q[:, 0] = E4M3_MAX * s
    return q.to(W.dtype)
