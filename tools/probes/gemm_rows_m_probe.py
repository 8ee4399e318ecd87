"""Do the bits of an output row of the backbone's linear products depend on M, the number of rows in the launch?

DecodeState.append_rows stacks the next turns of several conversations into one forward, so M = sum of their lengths, and
gemm_dispatch picks its kernel from (M, N, K).  For the CSM-1B backbone's four products a fixed block of 24 rows is multiplied
alone (M = 24: what a one-row append of that turn runs) and then as the first / last rows of launches of growing M, through
the automatic dispatch and through the per-call pin (ops.gemm(pin=True), csm_gemm_bf16_pinned); each line says which kernel ran
and whether the block's rows kept the bits of the M = 24 launch.

    python tools/probes/gemm_rows_m_probe.py > profiles/r09_gemm_rows_m_probe.txt
"""
import torch

from csm.hip import lib, ops

BF = torch.bfloat16
SHAPES = [("attn.qkv", 3072, 2048), ("attn.output_proj", 2048, 2048), ("mlp.w13", 16384, 2048), ("mlp.w2", 2048, 8192)]
MS = [6, 8, 24, 25, 64, 129, 256, 512, 768, 1024, 1536, 2048, 4096]
NB = 24


def main():
    g = torch.Generator().manual_seed(0)
    verdict = {"auto": True, "pin": True}
    for name, N, K in SHAPES:
        W = (torch.randn(N, K, generator=g) * 0.02).to(BF).cuda()
        block = torch.randn(NB, K, generator=g).to(BF).cuda()
        ref = torch.empty(NB, N, dtype=BF, device="cuda")
        ops.gemm(block, W, ref)
        print(f"{name}: N = {N}, K = {K}; reference M = {NB} ran {lib.csm_gemm_last_kernel().decode()}")
        for M in MS:
            nb = min(NB, M)
            for where in ("first", "last"):
                A = torch.randn(M, K, generator=g).to(BF).cuda()
                lo = 0 if where == "first" else M - nb
                A[lo:lo + nb] = block[:nb]
                line = f"  M = {M:5d}, block {where:5s}:"
                for mode in ("auto", "pin"):
                    C = torch.empty(M, N, dtype=BF, device="cuda")
                    ops.gemm(A, W, C, pin=mode == "pin")
                    same = torch.equal(C[lo:lo + nb].view(torch.int16), ref[:nb].view(torch.int16))
                    verdict[mode] &= same
                    line += f"  {mode} {'same bits' if same else 'DIFFERENT'} ({lib.csm_gemm_last_kernel().decode().split('<')[0]})"
                print(line)
    torch.cuda.synchronize()
    for mode, ok in verdict.items():
        print(f"{mode}: a row's bits {'do not depend' if ok else 'DEPEND'} on M over these shapes")


if __name__ == "__main__":
    main()
