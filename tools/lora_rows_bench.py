#!/usr/bin/env python3
"""What training several speakers' LoRA adapters in one batch costs and buys: CSM-1B (random init), LoRA r = 8 on q_proj / v_proj,
B = 8 examples of S = 2048 positions, loss mode C (semantic CE + depth decoder on 1/16 of the frames), one GPU, ONE job.

Legs, alternating over --rounds so that drift hits all of them (a host clock around --steps units that end in a device synchronise,
after --warmup untimed units of every leg).  For every A = 1 / 4 / 16 the legs cover the SAME n = max(B, A) examples, so that every
adapter set of a stack has an example in the step:
  single    one single-adapter LoRA step over the n examples (one set for the whole batch): what the project had before stacks
  stack A   one step with a stack of A adapter sets, example i running with set i mod A
  seq A     the same examples speaker by speaker, measured: A single-adapter steps of the n / A examples of one speaker each -
            what training the A speakers one after the other costs, every step walking the frozen base model again
Reported: ms per unit, positions per second, stack against seq, stack against single.  A stack pays KX / 32 extra k-steps per
row in the K-extension of the frozen GEMMs (KX = 32 A here); that cost is in these figures.

Then ``csm_skinny_nt_sel_bf16`` alone at M = 16384, K = 2048: N = 32 / 64 / 256 (blk = 16: 2 / 4 / 16 adapters, 2048 contiguous
rows per adapter as in a batch of 8 examples; and, for N = 256, every row another adapter - the worst case, all 16 tiles walked)
against ``csm_skinny_nt_bf16`` at N = 32.  Device events around 50 calls after a warm-up call, two passes.

No GPU, no number: the script fails without a device."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "csm-train-pytorch_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=4, help="timed steps per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps per leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--adapters", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", type=str, default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_rows_bench: no GPU - nothing is measured without one")
    from csm.data import SyntheticCSMDataset
    from csm.hip import ops
    from csm.models.model import Model
    from csm.training.lora import LoRAState
    from csm.training.optim import FusedAdamW
    from csm.training.trainer import csm_1b_args
    from csm.training.utils import compute_loss

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    args = csm_1b_args()
    B, S = a.batch, a.seq
    model = Model(args, device="cuda:0", seed=0)
    model.acoustic_mode = "amortized"
    for k in model.trainable:
        model.trainable[k] = False
    nmax = max([B] + a.adapters)
    b = SyntheticCSMDataset(nmax, S, args.text_vocab_size, args.audio_vocab_size, args.audio_num_codebooks, seed=1234).get_batch(0, nmax)
    tk, mk, tg = (b[k].cuda() for k in ("input_tokens", "input_masks", "target_audio_tokens"))
    say(f"# lora_rows_bench: CSM-1B random init, LoRA r=8 q_proj/v_proj, B={B} S={S}, loss mode C; {torch.cuda.get_device_name(0)}")

    def state(A):
        model.lora = st = LoRAState(model, 8, 16.0, 0.0, ["q_proj", "v_proj"], None, False, seed=0, n_adapters=A)
        return st, FusedAdamW(model, {}, lora_lr=1e-4)

    def step(st, opt, rows, ids):
        model.lora = st
        loss, _ = compute_loss(model, *rows, 100.0, 1.0, adapter_ids=ids)
        model.engine.backward(1.0)
        opt.clip_grad_norm(1.0)
        opt.step(zero_grad=True)
        return loss

    # a leg is (examples it covers, what one unit of it runs); every unit of the legs of one A covers the SAME examples
    single = state(1)
    legs = {}
    for A in a.adapters:
        n = max(B, A)                                           # every set has at least one example in the step
        take = lambda idx: (tk[idx].contiguous(), mk[idx].contiguous(), tg[idx].contiguous())   # noqa: E731  (resident before the timed region)
        rows = take(torch.arange(n, device="cuda"))
        if f"single B={n}" not in legs:                          # one adapter set for the whole batch: what the project had before stacks
            legs[f"single B={n}"] = (n, 1, 32, lambda rows=rows: step(*single, rows, None))
        st = state(A)
        ids = [i % A for i in range(n)] if A > 1 else None      # (n_adapters = 1 IS the single-adapter state: the default costs what it did)
        legs[f"stack A={A} B={n}"] = (n, A, next(iter(st[0].groups.values())).kx, lambda st=st, rows=rows, ids=ids: step(*st, rows, ids))
        if A > 1:
            # the same n examples speaker by speaker, measured: A single-adapter steps of the n / A examples of one speaker each
            parts = [take(torch.arange(sp, n, A, device="cuda")) for sp in range(A)]
            legs[f"seq   A={A} B={n // A}x{A}"] = (n, A, 32, lambda parts=parts: [step(*single, r, None) for r in parts][-1])

    def units(name, k):
        fn = legs[name][3]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            loss = fn()
        torch.cuda.synchronize()
        assert float(loss.detach()) == float(loss.detach()), f"{name}: loss is NaN"
        return (time.perf_counter() - t0) / k

    for name in legs:
        units(name, a.warmup)
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name in legs:
            times[name].append(units(name, a.steps))
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    say()
    say(f"{'leg':20s} {'examples':>8s} {'KX':>4s} {'ms':>9s} {'positions/s':>12s}   ms of each round (one unit = all the leg's examples once)")
    for name, (n, A, kx, _) in legs.items():
        say(f"{name:20s} {n:8d} {kx:4d} {med[name] * 1e3:9.2f} {n * S / med[name]:12.0f}   {' '.join(f'{t * 1e3:.2f}' for t in times[name])}")
    say()
    for name, (n, A, kx, _) in legs.items():
        if name.startswith("stack") and A > 1:
            seq, one = med[f"seq   A={A} B={n // A}x{A}"], med[f"single B={n}"]
            say(f"A={A}: the stack step is x{seq / med[name]:.2f} the positions/s of the {A} measured single-adapter steps over the same {n} "
                f"examples, and costs {100 * (med[name] / one - 1):+.1f} % against one adapter set on the same batch")

    # ---- the product alone
    M, K = 16384, 2048
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)

    def timeit(fn, n=50):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    rows = []
    W32 = torch.randn(32, K, device="cuda", generator=g).to(torch.bfloat16)
    o32 = torch.empty(M, 32, dtype=torch.bfloat16, device="cuda")
    rows.append(("csm_skinny_nt_bf16      N=32", lambda: ops.skinny_nt(X, W32, o32)))
    keep = []
    for N in (32, 64, 256):
        A = N // 16
        W = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
        o = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        runs = ((torch.arange(M) // 2048) % A).to(torch.int32).cuda()
        keep.append((W, o, runs))
        rows.append((f"csm_skinny_nt_sel_bf16  N={N:<3d} blk=16, 2048-row runs", lambda W=W, o=o, s=runs: ops.skinny_nt_sel(X, W, o, s, 16)))
        if N == 256:
            each = (torch.arange(M) % A).to(torch.int32).cuda()
            none = torch.full((M,), -1, dtype=torch.int32).cuda()
            keep.append((each, none))
            rows.append((f"csm_skinny_nt_sel_bf16  N={N:<3d} blk=16, every row another", lambda W=W, o=o, s=each: ops.skinny_nt_sel(X, W, o, s, 16)))
            rows.append((f"csm_skinny_nt_sel_bf16  N={N:<3d} blk=16, all rows -1", lambda W=W, o=o, s=none: ops.skinny_nt_sel(X, W, o, s, 16)))
    res = {n: [] for n, _ in rows}
    for _ in range(2):
        for n, fn in rows:
            res[n].append(timeit(fn))
    say()
    say(f"the product alone, M={M} K={K} (X: {M * K * 2 / 1e6:.0f} MB read once), us per call (50 calls after a warm-up call, two passes):")
    for n, _ in rows:
        t = min(res[n])
        say(f"  {n:58s} {' '.join(f'{x:8.1f}' for x in res[n])}   {M * K * 2 / t / 1e6:6.2f} TB/s of X")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
