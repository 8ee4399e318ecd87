"""float64 reference of the row-selected skinny product ``csm_skinny_nt_sel_bf16`` (csrc/gemm.hip) and of the stacked-adapter
LoRA form it serves (csm/training/lora.py, ``LoRAState(n_adapters > 1)``).

  out[m][n] = alpha * sum_k X[m][k] Wt[n][k]   if sel[m] >= 0 and n // blk == sel[m]
            = +0 (bits 0x0000)                 otherwise - chosen, never multiplied: Inf / NaN of X does not reach it

The cases are data (``CASES``).  A case fixes M, K, (N, blk), the number of adapters A (A * blk <= N; the columns past A * blk are
padding that no row may select), a ``sel`` pattern, alpha, the guard columns of X and of the output, and whether the rows that
select nothing hold Inf / NaN.

Bounds.  A selected element is the skinny product of ``train_gemm_ref``: a chain of K / 4 products per wave plus the three joining
additions (``acc_slack(sabs, K // 4 + 3)``), alpha, half a bf16 ulp - imported from there, not restated.  Every other element of
the window has slack -1: it must equal the reference (0) exactly, and ``judge_bits`` also wants its bits to be 0x0000.  The output
lives in a NaN-filled buffer with GR guard rows above and below and ldo - N guard columns, judged whole: guards keep their bits.
"""
from collections import namedtuple

import torch

from train_gemm_ref import GR, acc32, acc_slack, product, scaled
from train_ops_ref import judge, trunc_bf16  # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GUARD_BITS = 0x7FC1                                               # a quiet NaN with a payload: what the buffer holds before the launch

MS = (1, 15, 16, 17, 33, 1000)
KS = (128, 256, 640, 2048)                                        # 640: a short round; 2048: two rounds per K quarter
SHAPES = ((32, 8, 4), (32, 16, 2), (64, 16, 4), (96, 24, 3), (256, 16, 16), (256, 32, 8))   # (N, blk, A); (96, 24, 3): 24 padding columns
PATTERNS = ("const", "runs_mid", "each_diff", "all_none", "mixed_none", "dead_tile", "last_partial", "poison")

Case = namedtuple("Case", "name M K N blk A pattern alpha ldx_pad ldo_pad")


def _cases():
    out, mk = [], [(M, K) for M in MS for K in KS]
    j = 0
    for N, blk, A in SHAPES:
        for pat in PATTERNS:
            # every (shape, pattern) pair, the (M, K) pairs in rotation (each twice over the table); the patterns that need more
            # than one 16-row tile take the next M that has one
            M, K = mk[j % len(mk)]
            if pat in ("dead_tile", "runs_mid", "last_partial") and M < 33:
                M = (33, 1000)[j % 2]
            if pat in ("mixed_none", "poison") and M < 15:          # (rows that select nothing must exist)
                M = 15
            out.append(Case(f"{pat}_{M}x{N}x{K}_b{blk}", M, K, N, blk, A, pat, (1.0, 0.25, 2.0)[j % 3], 8 * (j % 3), 4 * (1 + j % 3)))
            j += 5                                                # (5 and 24 are coprime: the rotation reaches every pair)
    # the big shape with every pattern that changes inside tiles, at both round structures
    out.append(Case("each_diff_1000x256x2048_b16", 1000, 2048, 256, 16, 16, "each_diff", 2.0, 0, 4))
    out.append(Case("runs_mid_1000x256x640_b32", 1000, 640, 256, 32, 8, "runs_mid", 0.5, 8, 8))
    return tuple(out)


CASES = _cases()
CASE = {c.name: c for c in CASES}


def sel_of(c) -> torch.Tensor:
    """The case's ``sel`` [M] int32."""
    m = torch.arange(c.M)
    A = c.A
    if c.pattern == "const":
        s = torch.full((c.M,), A - 1)
    elif c.pattern == "runs_mid":                                  # runs of 24 rows that change at rows 8, 32, 56, ...: inside tiles
        s = ((m + 16) // 24) % A
    elif c.pattern == "each_diff":
        s = m % A
    elif c.pattern == "all_none":
        s = torch.full((c.M,), -1)
    elif c.pattern == "mixed_none":
        s = torch.where(m % 3 == 1, torch.full_like(m, -1), (m // 2) % A)
    elif c.pattern == "dead_tile":                                 # rows 16..31 select nothing: a 16-row tile without work
        s = torch.where((m >= 16) & (m < 32), torch.full_like(m, -1), torch.zeros_like(m))
    elif c.pattern == "last_partial":                              # the ragged last tile alone uses the last adapter
        s = torch.where(m >= (c.M // 16) * 16, torch.full_like(m, A - 1), torch.zeros_like(m))
    elif c.pattern == "poison":
        s = torch.where(m % 4 == 2, torch.full_like(m, -1), m % A)
    else:
        raise ValueError(c.pattern)
    return s.to(torch.int32)


def inputs(c):
    """-> dict X [M, K + ldx_pad] (view [M, K] = ``X``), Wt [N, K], sel; all bf16 / int32 on the CPU.  ``poison``: the rows with
    sel = -1 hold Inf, -Inf and NaN."""
    g = torch.Generator().manual_seed(1000003 * c.M + 7919 * c.K + 31 * c.N + c.blk + len(c.pattern))
    Xbuf = (torch.randn(c.M, c.K + c.ldx_pad, generator=g)).to(BF16)
    Wt = (torch.randn(c.N, c.K, generator=g) * 0.5).to(BF16)
    sel = sel_of(c)
    if c.pattern == "poison":
        rows = (sel < 0).nonzero().reshape(-1)
        for j, r in enumerate(rows.tolist()):
            Xbuf[r, :] = (float("inf"), float("-inf"), float("nan"))[j % 3]
            if j % 2:
                Xbuf[r, ::2] = 1.0                                  # Inf / NaN mixed with ordinary values
    return {"c": c, "Xbuf": Xbuf, "X": Xbuf[:, :c.K], "Wt": Wt, "sel": sel}


def selected(c, sel) -> torch.Tensor:
    """[M, N] bool: the elements row m keeps."""
    n = torch.arange(c.N)
    return (sel[:, None] >= 0) & ((n[None, :] // c.blk) == sel[:, None].long())


def reference(i):
    """-> (value [M, N] float64, slack): slack -1 (exact) where nothing is selected."""
    c = i["c"]
    keep = selected(c, i["sel"])
    X = torch.where((i["sel"] >= 0)[:, None], i["X"].double(), torch.zeros((), dtype=F64))   # rows that select nothing never count
    val, sabs, _ = product(X, i["Wt"], 0, 0)
    v, s = scaled(val, acc_slack(sabs, c.K // 4 + 3), c.alpha)
    s = torch.as_tensor(s, dtype=F64).expand(v.shape)
    return torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, s, torch.full_like(s, -1.0))


# ------------------------------------------------------------------------------------------------------------- guard buffers
def out_buffer(c) -> torch.Tensor:
    """The flat output buffer before the launch: (GR + M + GR) rows of ldo = N + ldo_pad, every element the guard NaN."""
    return torch.full(((2 * GR + c.M) * (c.N + c.ldo_pad),), GUARD_BITS, dtype=torch.int32).to(torch.int16).view(BF16)


def window(c, buf) -> torch.Tensor:
    """The [M, N] output window of a buffer (a view)."""
    ldo = c.N + c.ldo_pad
    return buf.view(2 * GR + c.M, ldo)[GR:GR + c.M, :c.N]


def judge_bits(tag, c, i, buf):
    """The whole buffer: guards keep GUARD_BITS, unselected window elements are 0x0000 bit for bit, selected ones lie within the
    skinny product's bound.  -> worst |err| / bound over the selected elements."""
    buf = buf.detach().cpu()
    ldo = c.N + c.ldo_pad
    bits = buf.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).view(2 * GR + c.M, ldo)
    inside = torch.zeros(2 * GR + c.M, ldo, dtype=torch.bool)
    inside[GR:GR + c.M, :c.N] = True
    bad = (bits != GUARD_BITS) & ~inside
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} guard elements overwritten, first at {tuple(bad.nonzero()[0].tolist())}"
    keep = selected(c, i["sel"])
    wbits = bits[GR:GR + c.M, :c.N]
    nz = (wbits != 0) & ~keep
    assert not bool(nz.any()), (f"{tag}: {int(nz.sum())} unselected elements are not +0, first at {tuple(nz.nonzero()[0].tolist())}: "
                                f"bits {int(wbits[tuple(nz.nonzero()[0].tolist())]):#06x}")
    ref, slack = reference(i)
    return judge(tag, window(c, buf).contiguous(), ref, slack)


# ------------------------------------------------------------------------------------------------------------- restatement
MUTANTS = ("mask_by_multiply", "block_plus1", "mod_for_div", "none_as_zero", "padding_written")
# the cases on which each wrong restatement must fail (test_lora_rows_cpu checks that there is at least one, and all of them fail)
MUTANT_CASES = {
    "mask_by_multiply": lambda c: c.pattern == "poison",
    "block_plus1": lambda c: c.pattern not in ("all_none",),
    "mod_for_div": lambda c: c.pattern not in ("all_none",),
    "none_as_zero": lambda c: c.pattern in ("all_none", "mixed_none", "poison"),
    "padding_written": lambda c: c.A * c.blk < c.N and c.pattern != "all_none",
}


def restate(i, mut=None):
    """fp32 in the kernel's order -> the flat output buffer: per K quarter the k-steps of 32 ascending (``acc32``), the quarters
    joined ((q0 + q1) + q2) + q3, alpha, one bf16 rounding, then the selection."""
    c = i["c"]
    s = i["sel"].long()
    if mut == "none_as_zero":
        s = s.clamp(min=0)
    a, b = i["X"].float(), i["Wt"].float().t()
    if mut != "mask_by_multiply":
        a = torch.where((s >= 0)[:, None], a, torch.zeros((), dtype=F32))     # (the kernel never lets such a row's sums out)
    q = c.K // 4
    parts = [acc32(a[:, j * q:(j + 1) * q], b[j * q:(j + 1) * q]) for j in range(4)]
    full = ((((parts[0] + parts[1]) + parts[2]) + parts[3]) * c.alpha).to(BF16)
    n = torch.arange(c.N)
    if mut == "block_plus1":
        keep = (s[:, None] >= 0) & ((n[None, :] // c.blk) == s[:, None] + 1)
    elif mut == "mod_for_div":
        keep = (s[:, None] >= 0) & ((n[None, :] % c.blk) == s[:, None])
    else:
        keep = (s[:, None] >= 0) & ((n[None, :] // c.blk) == s[:, None])
    if mut == "mask_by_multiply":
        win = full * keep.to(BF16)                                # NaN * 0 = NaN: the zeros must be chosen
    else:
        win = torch.where(keep, full, torch.zeros((), dtype=BF16))
    if mut == "padding_written":
        pad = n >= c.A * c.blk
        win = torch.where(pad[None, :] & (s[:, None] >= 0), full, win)
    buf = out_buffer(c)
    window(c, buf).copy_(win)
    return buf


# ------------------------------------------------------------------------------------------------------------- the LoRA form
def stacked_operands(A_list, B_list, rows_of, N_out, blk, kx):
    """At [in, kx] and Bx [N_out, kx] (float64, requires_grad) of a stack: adapter a = (A_list[a] [members][r, in], B_list[a]
    [members][out_j, r]) owns columns [a blk, (a + 1) blk), member j the columns j r .. inside it and the rows ``rows_of[j]`` of
    the fused projection.  -> (At, Bx, mask [N_out, kx] of the entries that belong to an adapter)."""
    in_f = A_list[0][0].shape[1]
    At, Bx, mask = torch.zeros(in_f, kx, dtype=F64), torch.zeros(N_out, kx, dtype=F64), torch.zeros(N_out, kx, dtype=F64)
    for a, (As, Bs) in enumerate(zip(A_list, B_list)):
        for j, (Aj, Bj) in enumerate(zip(As, Bs)):
            r = Aj.shape[0]
            c0 = a * blk + j * r
            At[:, c0:c0 + r] = Aj.t()
            Bx[rows_of[j], c0:c0 + r] = Bj
            mask[rows_of[j], c0:c0 + r] = 1
    return At.requires_grad_(), Bx.requires_grad_(), mask


def stacked_forward(x, W0, At, Bx, sel, blk, s):
    """y = x W0^T + tx Bx^T with tx = s x At zero outside row m's block (the K-extension form)."""
    n = torch.arange(At.shape[1])
    keep = (sel[:, None] >= 0) & ((n[None, :] // blk) == sel[:, None].long())
    tx = torch.where(keep, s * (x @ At), torch.zeros((), dtype=F64))
    return x @ W0.t() + tx @ Bx.t()


def dense_forward(x, W0, A_list, B_list, rows_of, sel, s):
    """Row by row: y[m] = x[m] W0^T + s (x[m] A_a^T) B_a^T with a = sel[m], member j writing its rows of the fused projection."""
    rows = []
    for m in range(x.shape[0]):
        y = x[m] @ W0.t()
        a = int(sel[m])
        if a >= 0:
            for j, (Aj, Bj) in enumerate(zip(A_list[a], B_list[a])):
                add = torch.zeros_like(y)
                add[rows_of[j]] = s * ((x[m] @ Aj.t()) @ Bj.t())
                y = y + add
        rows.append(y)
    return torch.stack(rows)
