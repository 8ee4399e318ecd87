#!/usr/bin/env python3
"""Mimi codec on the GPU: encode / decode time for 10 s of 24 kHz audio (seeded random weights with the HF key names), then
the streaming decoder: microseconds per ``MimiDecodeStream.step`` of n = 1, 2, 4 frames and the kernel launches per step, then
the streaming encoder: ``encode`` of 5 s next to microseconds per ``MimiEncodeStream.step`` of n = 1, 2, 4 frames, then the rows
encoder: one ``MimiEncodeStreamRows.step`` of R = 1 / 4 / 16 rows at n = 4 against R consecutive ``MimiEncodeStream.step`` calls,
then the device resampler: one ``ResampleStreamRows.step`` of R = 1 / 4 / 16 rows for a 320 ms chunk against R one-row launches.
MIMI_BENCH=rows runs the rows leg alone, MIMI_BENCH=resample the resampler leg alone (no codec is built)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "csm-train-pytorch_amd"))
import torch


def resample_leg():
    """One rows launch at R = 1 / 4 / 16 for a 320 ms chunk against R one-row launches (``ResampleStream.feed``), alternated
    three times in this job: 200 back-to-back steps between two synchronisations, median and spread of the repeats."""
    from csm.codec.resample import Resampler
    for (a, b), n_in in (((24000, 48000), 7680), ((16000, 24000), 5120), ((44100, 24000), 14112)):
        rs = Resampler(a, b, device="cuda")
        for R in (1, 4, 16):
            g = torch.Generator().manual_seed(R)
            xs = [(torch.randn(n_in, generator=g) * 0.1).cuda() for _ in range(R)]
            rows, singles = rs.stream_rows(16, n_in), [rs.stream(n_in) for _ in range(R)]
            slots = list(range(R))
            for s_ in slots:
                rows.open(s_)
            legs = {"rows": lambda: rows.step(slots, xs), "single": lambda: [singles[r].feed(xs[r]) for r in range(R)]}
            res = {"rows": [], "single": []}
            for _ in range(3):
                for name, fn in legs.items():
                    for _ in range(20):
                        out = fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(200):
                        out = fn()
                    torch.cuda.synchronize()
                    res[name].append((time.perf_counter() - t0) / 200 * 1e6)
                    if name == "rows": got = out
            same = all(torch.equal(got[r], out[r]) for r in range(R))        # both ran 660 steps from position 0 on the same audio
            med = {k: sorted(v)[1] for k, v in res.items()}
            print(f"resample {a} -> {b} rows step R={R:2d} n_in={n_in}: {med['rows']:.1f} us per step (repeats "
                  f"{[round(v, 1) for v in res['rows']]}), 1 launch; {R} one-row launches {med['single']:.1f} us (repeats "
                  f"{[round(v, 1) for v in res['single']]}) -> {med['single'] / med['rows']:.2f}x; outputs "
                  f"{'equal' if same else 'DIFFER'}", flush=True)


if os.environ.get("MIMI_BENCH") == "resample":
    resample_leg()
    sys.exit(0)
from transformers import MimiConfig, MimiModel
from csm.codec import MimiCodec

torch.manual_seed(0)
hf = MimiModel(MimiConfig()).eval()
with torch.no_grad():
    for n, b in hf.named_buffers():
        if n.endswith("embed_sum"):
            b.copy_(torch.randn(b.shape))
codec = MimiCodec(hf.state_dict(), device="cuda")
wav = torch.randn(1, 1, 240000) * 0.1
def t(fn, n=3):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, r
ROWS_ONLY = os.environ.get("MIMI_BENCH") == "rows"
te, codes = t(lambda: codec.encode(wav)) if not ROWS_ONLY else (0.0, None)
td, out = t(lambda: codec.decode(codes)) if not ROWS_ONLY else (0.0, None)
if not ROWS_ONLY: print(f"encode 10 s: {te*1e3:.1f} ms ({10/te:.0f}x real time) -> codes {tuple(codes.shape)};  decode: {td*1e3:.1f} ms ({10/td:.0f}x real time) -> {tuple(out.shape)}")


class _Counting:
    """Counts the C-ABI calls made through a module's ``lib`` (each is one kernel launch for these ops)."""
    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        def call(*a):
            self.n += 1
            return fn(*a)
        return call


import csm.codec.mimi as mimi_mod
from csm.hip import ops as ops_mod
stream = codec.decode_stream()
for n in (() if ROWS_ONLY else (1, 2, 4)):
    steps = 48 // n
    chunk = codes[:, :, :n]
    stream.reset()
    for _ in range(4):
        stream.step(chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stream.step(chunk)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / steps * 1e6
    counters = [_Counting(mimi_mod.lib), _Counting(ops_mod.lib)]
    mimi_mod.lib, ops_mod.lib = counters
    stream.step(chunk)
    mimi_mod.lib, ops_mod.lib = counters[0]._lib, counters[1]._lib
    launches = counters[0].n + counters[1].n + 1          # + the latent's zero fill
    print(f"stream step n={n}: {us:.0f} us per step ({us / n:.0f} us per 80-ms frame, {n * 80e3 / us:.0f}x real time), "
          f"{launches} launches per step")

wav5 = wav[:, :, :120000].cuda()
t5, _ = t(lambda: codec.encode(wav5))
print(f"encode 5 s: {t5*1e3:.1f} ms ({5/t5:.0f}x real time)")
enc = codec.encode_stream()
for n in (() if ROWS_ONLY else (1, 2, 4)):
    steps = 48 // n
    chunk = wav5[:, :, :n * 1920]
    enc.reset()
    for _ in range(4):
        enc.step(chunk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        enc.step(chunk)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / steps * 1e6
    counters = [_Counting(mimi_mod.lib), _Counting(ops_mod.lib)]
    mimi_mod.lib, ops_mod.lib = counters
    enc.step(chunk)
    mimi_mod.lib, ops_mod.lib = counters[0]._lib, counters[1]._lib
    print(f"encode stream step n={n}: {us:.0f} us per step ({us / n:.0f} us per 80-ms frame, {n * 80e3 / us:.0f}x real time), "
          f"{counters[0].n + counters[1].n} launches per step; 5 s in {62.5 / n * us / 1e3:.1f} ms of steps")


# rows encoder: R utterances per step against R single steps, alternated twice in this job (the better of each is kept)
n, steps = 4, 12
encs = [codec.encode_stream() for _ in range(16)]
rows = codec.encode_stream_rows(slots=16)
for R in (1, 4, 16):
    g = torch.Generator().manual_seed(R)
    chunk = (torch.randn(R, n * 1920, generator=g) * 0.1).cuda()
    slots = list(range(R))
    best = {"rows": float("inf"), "single": float("inf")}
    for _ in range(2):
        for s_ in slots:
            rows.open(s_)
            encs[s_].reset()
        def rows_step(): return rows.step(slots, chunk)
        def single_steps(): return [encs[r].step(chunk[r].view(1, 1, -1)) for r in range(R)]
        for name, fn in (("rows", rows_step), ("single", single_steps)):
            for _ in range(4):
                out = fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = fn()
            torch.cuda.synchronize()
            best[name] = min(best[name], (time.perf_counter() - t0) / steps * 1e6)
            if name == "rows": got = out
        same = all(torch.equal(got[r], out[r][0]) for r in range(R))       # both ran 16 steps from position 0 on the same audio
    counters = [_Counting(mimi_mod.lib), _Counting(ops_mod.lib)]
    mimi_mod.lib, ops_mod.lib = counters
    rows.step(slots, chunk)
    mimi_mod.lib, ops_mod.lib = counters[0]._lib, counters[1]._lib
    print(f"encode rows step R={R:2d} n={n}: {best['rows']:.0f} us per step, {counters[0].n + counters[1].n} launches; {R} single "
          f"steps {best['single']:.0f} us -> {best['single'] / best['rows']:.2f}x ({best['rows'] / best['single'] * R:.2f} single steps "
          f"for {R} rows); codes {'equal' if same else 'DIFFER'}", flush=True)

resample_leg()
