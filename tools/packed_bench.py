#!/usr/bin/env python3
"""What sequence packing buys on fine-tuning-sized examples: CSM-1B (random init), full-parameter train step, loss mode C
(semantic CE + depth decoder on 1/16 of the labelled frames), one GPU.

The example lengths are seeded and drawn uniformly from 150..700 positions (a target's text frames plus at most two context turns
of at most 10 s each); the list is written out.  Three legs in ONE job, on the same examples, every one an "epoch" over all of
them in steps of --batch examples:
  padded    collate_variable_length in the drawn order (every example padded to its batch's maximum)
  bucketed  the same after sorting by length (what LengthBucketSampler's windows converge to: its best case)
  packed    collate_packed into rows of 2048 positions (segment-masked attention, RoPE restarting per example)
All three pad the targets with IGNORE_INDEX, so they train on the same labelled frames.  Per leg: ms per step, real (unpadded)
positions per second, fill ratio = real positions / positions computed.  Timing: a host clock around whole epochs that end in a
device synchronise, after warm-up epochs over the same shapes; the legs alternate (--rounds) so that drift hits all of them.

Then the attention kernels alone at B = 4, S = 2048, 32 / 8 heads: one segment per row through the segment-masked kernels against
the unsegmented ones (forward: default; backward: second-generation dK/dV - variant bit 10 - and the default asm dK/dV), and a
packed layout of 8 x 256 per row.  Device events around 20 calls after a warm-up call.

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
    ap.add_argument("--examples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16, help="examples drawn per step")
    ap.add_argument("--warmup", type=int, default=1, help="untimed epochs per leg")
    ap.add_argument("--rounds", type=int, default=3, help="timed epochs per leg, the legs alternating")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", type=str, default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_bench: no GPU - nothing is measured without one")
    from csm.data import SyntheticCSMDataset, collate_packed, collate_variable_length
    from csm.data.training_data import IGNORE_INDEX
    from csm.hip import ops
    from csm.models.model import Model
    from csm.training.trainer import CSMTrainer, csm_1b_args
    import tempfile

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator().manual_seed(a.seed)
    lengths = torch.randint(150, 701, (a.examples,), generator=g).tolist()
    args = csm_1b_args()
    items = []
    for i, S in enumerate(lengths):
        it = SyntheticCSMDataset(1, S, args.text_vocab_size, args.audio_vocab_size, args.audio_num_codebooks, seed=5000 + i)[0]
        it["target_audio_tokens"] = it["target_audio_tokens"][:S - 1]
        items.append(it)
    real = sum(lengths)
    say(f"# packed_bench: {a.examples} examples, seed {a.seed}, {a.batch} examples per step, lengths (positions):")
    say("# " + " ".join(map(str, lengths)))
    say(f"# real positions per epoch: {real}; {torch.cuda.get_device_name(0)}")

    def on_device(b):
        return {k: (v if k == "segment_lengths" else v.cuda()) for k, v in b.items()}      # the descriptor is built from host integers

    chunks = lambda order: [[items[i] for i in order[j:j + a.batch]] for j in range(0, len(order), a.batch)]   # noqa: E731
    drawn, by_len = list(range(a.examples)), sorted(range(a.examples), key=lambda i: lengths[i])
    legs = {"padded": [on_device(collate_variable_length(c, target_pad=IGNORE_INDEX)) for c in chunks(drawn)],
            "bucketed": [on_device(collate_variable_length(c, target_pad=IGNORE_INDEX)) for c in chunks(by_len)],
            "packed": [on_device(collate_packed(c, max_seq_len=2048)) for c in chunks(drawn)]}

    model = Model(args, device="cuda:0", seed=0)
    model.acoustic_mode = "amortized"
    model.target_ignore_index = IGNORE_INDEX
    tr = CSMTrainer("", tempfile.mkdtemp(prefix="csm_packed_bench_"), device="cuda:0")
    tr.logger.setLevel(30)
    tr.model = model
    tr.prepare_optimizer()

    def epoch(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            loss, _ = tr.train_step(b, 1, True, 1.0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, float(loss)

    for name, batches in legs.items():
        for _ in range(a.warmup):
            epoch(batches)
    times = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, batches in legs.items():
            dt, loss = epoch(batches)
            assert loss == loss, f"{name}: loss is NaN"
            times[name].append(dt)
    say()
    say(f"{'leg':9s} {'steps':>5s} {'rows x S per step':>30s} {'fill':>6s} {'ms/step':>9s} {'real pos/s':>11s} {'epoch s (each round)':>24s}")
    base = None
    for name, batches in legs.items():
        shapes = [tuple(b["input_tokens"].shape[:2]) for b in batches]
        computed = sum(r * s for r, s in shapes)
        best = sorted(times[name])[len(times[name]) // 2]                      # the median round
        rate = real / best
        base = base or rate
        say(f"{name:9s} {len(batches):5d} {' '.join(f'{r}x{s}' for r, s in shapes):>30s} {real / computed:6.3f} {best / len(batches) * 1e3:9.2f} "
            f"{rate:11.0f} {' '.join(f'{t:.3f}' for t in times[name]):>24s}   x{rate / base:.2f} vs padded")

    # ---- the attention kernels alone
    B, S, H, KV, hd = 4, 2048, 32, 8, 64
    gd = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B * S, (H + 2 * KV) * hd, device="cuda", generator=gd).to(torch.bfloat16)
    dout = torch.randn(B * S, H * hd, device="cuda", generator=gd).to(torch.bfloat16)
    out = torch.empty(B * S, H * hd, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    lse8 = torch.empty_like(lse)                                               # the 8 x 256 layout has statistics of its own
    dqkv, delta = torch.empty_like(qkv), torch.empty(2, B, H, S, dtype=torch.float32, device="cuda")

    def arrays(n):
        p = torch.arange(S, dtype=torch.int32)
        ss = (p // n * n).repeat(B)
        return ss.cuda(), (ss + n - 1).cuda()

    def timeit(fn, n=20):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    say()
    say(f"attention kernels alone, B={B} S={S} {H}/{KV} heads x {hd}, us per call (20 calls after a warm-up call, two passes):")
    one, eight = arrays(S), arrays(256)
    D = 2 | (1 << 2) | (3 << 4) | (1 << 6) | (1 << 7)
    ops.attn_fwd(qkv, out, lse, B, S, H, KV, hd)
    rows = [("fwd  unsegmented (default)", 0, lambda: ops.attn_fwd(qkv, out, lse, B, S, H, KV, hd)),
            ("fwd  seg, 1 x 2048", 0, lambda: ops.attn_fwd_seg(qkv, out, lse, one[0], B, S, H, KV, hd)),
            ("fwd  seg, 8 x 256", 0, lambda: ops.attn_fwd_seg(qkv, out, lse8, eight[0], B, S, H, KV, hd)),
            ("bwd  unsegmented, default (asm dK/dV)", 0, lambda: ops.attn_bwd(qkv, out, dout, lse, dqkv, delta, B, S, H, KV, hd)),
            ("bwd  unsegmented, variant bit 10", D | 1 << 10, lambda: ops.attn_bwd(qkv, out, dout, lse, dqkv, delta, B, S, H, KV, hd)),
            ("bwd  seg, 1 x 2048", 0, lambda: ops.attn_bwd_seg(qkv, out, dout, lse, dqkv, delta, one[0], one[1], B, S, H, KV, hd)),
            ("bwd  seg, 8 x 256", 0, lambda: ops.attn_bwd_seg(qkv, out, dout, lse8, dqkv, delta, eight[0], eight[1], B, S, H, KV, hd))]
    res = {n: [] for n, _, _ in rows}
    try:
        for _ in range(2):
            for n, word, fn in rows:
                ops.lib.csm_set_attn_variant(word)
                res[n].append(timeit(fn))
    finally:
        ops.lib.csm_set_attn_variant(0)
    for n, _, _ in rows:
        say(f"  {n:40s} {' '.join(f'{t:8.1f}' for t in res[n])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
