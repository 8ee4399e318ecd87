#!/usr/bin/env python3
"""BASELINE config 5: generate() - Mimi encode of the context + AR multi-codebook decode of 10 s of audio (125 frames) +
Mimi decode, on one MI355X, CSM-1B random init.  Neither tokenizer can be fetched offline: the text side is a byte-level
stand-in, the audio side is the real GPU codec (csm.codec.MimiCodec) with seeded random weights in the Hugging Face
layout (GEN_CODEC=rvq swaps in the quantiser-only stand-in when transformers is unavailable).  GEN_LORA=q_proj,v_proj (or
all): decode frames/s with live LoRA adapters against the same adapters merged, alternated in one process.  GEN_STREAM=1:
generate_stream() with chunk_frames 1, 2 and 4 against generate() on the same setting, alternated in one process: time from
the call to the first chunk on the host, total wall time and frames/s.  GEN_BATCH_SWEEP=1: generate_batch() at 1, 4, 8 and 16
utterances from one process, one line each (aggregate frames/s, seconds per frame).  GEN_LORA_BANK=q_proj,v_proj (or all): decode
frames/s with a different LoRA adapter per utterance (16 adapters, some rows without) against the same batch without adapters
and against the same utterances one at a time with their adapter live as model.lora, alternated in one process.
GEN_FP8=1 together with GEN_LORA_BANK=...: bf16 + bank, FP8 + bank (model.fp8_adapters), FP8 and bf16 without adapters, alternated
on one model at B = 4 / 8 / 16 (decode loop only).  GEN_FP8=1: decode frames/s with bf16 and with FP8 (weight-only e4m3) decode weights,
alternated on one model at B = 1 / 4 / 16, and the bytes of decode weights in each mode.  GEN_SERVE=1: the running batch (Generator.serve): rows-codec step against single steps, the server step at
16 rows, the join stall (serve_main).  GEN_SERVE_SAMPLING=1: the rows sampler against the scalar one and the 16-row
server step with row_sampling off / on (serve_sampling_main); GEN_SERVE_SAMPLING=processors: the processed rows sampler (repetition penalty, per-codebook
parameters; serve_processors_main); GEN_SERVE_SAMPLING=typical: the typical rows sampler (typical_p) at identity, one-wave and
block-wide, and the server step with row_processors / row_typical (serve_typical_main); GEN_SERVE_SAMPLING=filters: the filtered rows sampler (top-p / min-p)
in four forms and the server step with row_filters off / on (serve_filters_main).  GEN_SERVE_STATS=1: csm_sample_stats_rows alone at
512 rows and the 16-row server step with stats off / on (serve_stats_main).  GEN_SERVE_CONV=1: 16 six-turn conversations on the running batch (BatchServer.conversation):
time to the first chunk of turns 1 / 3 / 5 against stateless submits, one append_rows against one-row calls, park / resume, aggregate
frames/s (serve_conv_main).  GEN_HEAR=1: a 5 s heard turn's last sample to the first chunk of the reply, with
``add(Segment)`` against ``hear`` fed during the turn, served (16 slots) and at B = 1 (hear_main), then the batched hearing of
``serve(hear_slots=16)`` against ``hear_slots=0``: the hearing cost per 4-frame chunk of 16 listeners and the last sample to
the first chunk when all 16 end together, ``end_heard`` against 16 ``end`` calls (hear_rows_main; GEN_HEAR=rows: that leg alone).  GEN_CONVERSATION=1: a scripted dialogue of 8 turns (odd turns spoken with 63 frames, even turns the other party's 5 s of audio)
through a Conversation (KV cache kept between turns) and statelessly (generate_stream with the accumulated Segment list - every
turn encodes and prefills the whole history again), alternated in one process after a warm-up dialogue of each: per spoken turn the
host time from the call to the first chunk (chunk_frames=2) and the turn's total; plus csm_attn_append alone next to the
csm_attn_fwd launch that would recompute the whole sequence.  GEN_RESAMPLE=1: the 16-slot server step with output_sample_rate=48000 and the 16-listener hear_step at 16 kHz input, each
against the same step without the resampler (resample_main).  GEN_OVERFLOW=1: a conversation past the length limit
(max_audio_length_ms = 90 000: 923 positions) - time to the first chunk of the overflowing turn under on_overflow="drop_oldest"
(the kept history is prefilled again) and "shift" (the KV cache slides: csm_kv_shift) next to an in-limit turn, at B = 1 and for
16 conversations that overflow at one boundary of the 16-slot server, plus csm_kv_shift alone (overflow_main).  GEN_VOICE=1: a voice
prompt prefilled once (Generator.voice) against the same 5 s given as context: fork_rows against resume_row calls, the staggered
served load, submit -> first chunk, and the steps that admit 1 and 16 joins (voice_main).  GEN_SERVE_STREAMS=1: more listeners than
slots (Generator.serve(streams=N)): the server step with 16 rows rotated out and in at every chunk boundary against the step
without rotation, park_rows / resume_rows against the one-row calls, and the streams one GPU keeps fed under the wall clock
without an underrun (serve_streams_main)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "csm-train-pytorch_amd"))
import torch
from csm.generator import Generator, Segment
from csm.models.model import Model
from csm.training.trainer import csm_1b_args
from csm.hip import ops


class ByteTokenizer:
    def encode(self, text):
        return [128000] + [b + 1000 for b in text.encode()] + [128001]


class RvqOnlyCodec:
    """Mimi's quantiser stage only: 1920-sample frames are folded into 256-d latents by a fixed random projection."""
    sample_rate = 24000

    def __init__(self, device, K=32):
        g = torch.Generator(device=device).manual_seed(0)
        self.cb = torch.randn(K, 2048, 256, device=device, generator=g)
        self.proj = torch.randn(1920, 256, device=device, generator=g) / 44.0
        self.K = K

    def encode(self, wav):                      # [1,1,N] -> [1,K,T]
        T = wav.shape[-1] // 1920
        lat = (wav[0, 0, :T * 1920].view(T, 1920) @ self.proj).contiguous()
        codes = torch.empty(self.K, T, dtype=torch.int64, device=wav.device)
        ops.rvq_encode(lat, self.cb, codes, 1)
        return codes.unsqueeze(0)

    def decode(self, codes):                    # [1,K,T] -> [1,1,N]
        c = codes[0].clamp(0, 2047).contiguous()
        out = torch.empty(c.shape[1], 256, dtype=torch.float32, device=codes.device)
        ops.rvq_decode(c, self.cb, out)
        return (out @ self.proj.t()).reshape(1, 1, -1)


def make_codec(dev):
    if os.environ.get("GEN_CODEC", "mimi") == "mimi":
        from transformers import MimiConfig, MimiModel
        from csm.codec import MimiCodec
        torch.manual_seed(0)
        hf = MimiModel(MimiConfig()).eval()
        with torch.no_grad():
            for name, buf in hf.named_buffers():
                if name.endswith("embed_sum"):
                    buf.copy_(torch.randn(buf.shape))
        return MimiCodec(hf.state_dict(), device=dev)
    return RvqOnlyCodec(dev)


def run(model, frames=125, repeats=2):
    """BASELINE config 5 on an existing model (bench.py's extra leg): 5 s of context audio tokenised by Mimi, ``frames`` AR
    frames, Mimi decode.  Returns the best of ``repeats`` timed runs after one short warm-up."""
    dev = model.device
    if not model.caches_are_enabled():
        model.setup_caches(1)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    gen.generate(text, 1, ctx, max_audio_length_ms=80 * 5)                  # warm-up: lazy attributes, allocator, graph capture
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.time()
        audio = gen.generate(text, 1, ctx, max_audio_length_ms=80 * frames)
        torch.cuda.synchronize()
        dt = time.time() - t0
        nfr = audio.numel() / 1920
        if best is None or dt / max(nfr, 1) < best[0] / max(best[1], 1):
            best = (dt, nfr)
    dt, nfr = best
    return {"frames": nfr, "seconds": round(dt, 4), "frames_per_s": round(nfr / dt, 1), "ms_per_frame": round(dt / max(nfr, 1) * 1e3, 3),
            "x_real_time": round(nfr * 0.08 / dt, 2), "includes": "Mimi encode of the context + prefill + decode frames + Mimi decode"}


def run_batch(model, nb=4, frames=125):
    """generate_batch(): ``nb`` utterances decoded together (ragged prompts, shared weight loads); aggregate frames/s of the second
    of two runs (the first captures the batch's frame graph)."""
    dev = model.device
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    texts = [f"utterance number {i}: the quick brown fox jumps over the lazy dog" for i in range(nb)]
    ctxs = [ctx if i % 2 == 0 else [] for i in range(nb)]
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.time()
        outs = gen.generate_batch(texts, list(range(nb)), ctxs, max_audio_length_ms=80 * frames)
        torch.cuda.synchronize()
        dt = time.time() - t0
    tot = sum(o.numel() for o in outs) / 1920
    return {"utterances": nb, "frames": tot, "seconds": round(dt, 4), "frames_per_s_aggregate": round(tot / dt, 1),
            "x_real_time_aggregate": round(tot * 0.08 / dt, 2)}


def decode_fps(model, frames=100, prompt=40):
    """Decode frames/s of ``model`` on its own: a ``prompt``-position text prompt is prefilled, then ``frames`` frames are
    generated (frame graph replays) and timed, without codec or prefill."""
    dev = model.device
    K = model.args.audio_num_codebooks
    model.setup_caches(1)
    model.reset_caches()
    g = torch.Generator().manual_seed(0)
    tok = torch.zeros(1, prompt, K + 1, dtype=torch.long)
    tok[0, :, K] = torch.randint(0, model.args.text_vocab_size, (prompt,), generator=g)
    msk = torch.zeros(1, prompt, K + 1, dtype=torch.bool)
    msk[0, :, K] = True
    amask = torch.cat([torch.ones(1, K, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool)], 1).unsqueeze(1).to(dev)
    pad = torch.zeros(1, 1, dtype=torch.long, device=dev)
    pos = torch.arange(prompt).unsqueeze(0).to(dev)
    f = model.generate_frame(tok.to(dev), msk.to(dev), pos, 0.9, 50)
    for _ in range(3):                                                       # eager frame, capture, first replay
        pos = pos[:, -1:] + 1
        f = model.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), amask, pos, 0.9, 50)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(frames):
        pos = pos[:, -1:] + 1
        f = model.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), amask, pos, 0.9, 50)
    torch.cuda.synchronize()
    return frames / (time.time() - t0)


def lora_main(mods):
    """GEN_LORA=q_proj,v_proj (config 3) or GEN_LORA=all: decode frames/s with live adapters (K-extension kernels) against the
    same adapters merged into a second model's weights, alternated in one process (GEN_ROUNDS rounds)."""
    from csm.training.lora import apply_lora_to_model, merge_lora_weights
    dev = "cuda:0"
    mods = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"] if mods == "all" else mods.split(",")
    models = {}
    for name in ("live", "merged"):
        m = Model(csm_1b_args(), device=dev, seed=0)
        apply_lora_to_model(m, r=8, alpha=16.0, target_modules=mods)
        with torch.no_grad():
            gb = torch.Generator(device=dev).manual_seed(1)
            for ad in m.lora.adapters.values():
                ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=gb, device=dev) * 0.02).to(torch.bfloat16))
        if name == "merged":
            merge_lora_weights(m)
            m.lora = None
        models[name] = m
    res = {"live": [], "merged": []}
    for _ in range(int(os.environ.get("GEN_ROUNDS", 3))):
        for name in ("merged", "live"):
            res[name].append(decode_fps(models[name], int(os.environ.get("GEN_FRAMES", 100))))
    best = {k: max(v) for k, v in res.items()}
    print(f"LoRA {','.join(mods)} r=8: decode frames/s live {[round(x, 1) for x in res['live']]} merged "
          f"{[round(x, 1) for x in res['merged']]} -> best live {best['live']:.1f} / merged {best['merged']:.1f} = "
          f"{best['live'] / best['merged']:.3f}x")


def decode_fps_batch(model, B, adapters=None, frames=50, prompt=40):
    """``decode_fps`` for B utterances decoded together (aggregate frames/s); ``adapters``: a LoRAState or None per row."""
    dev = model.device
    K = model.args.audio_num_codebooks
    model.setup_caches(B)
    model.reset_caches()
    g = torch.Generator().manual_seed(0)
    tok = torch.zeros(B, prompt, K + 1, dtype=torch.long)
    tok[:, :, K] = torch.randint(0, model.args.text_vocab_size, (B, prompt), generator=g)
    msk = torch.zeros(B, prompt, K + 1, dtype=torch.bool)
    msk[:, :, K] = True
    amask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1).to(dev)
    pad = torch.zeros(B, 1, dtype=torch.long, device=dev)
    pos = torch.arange(prompt).unsqueeze(0).repeat(B, 1).to(dev)
    f = model.generate_frame(tok.to(dev), msk.to(dev), pos, 0.9, 50, adapters=adapters)
    for _ in range(3):                                                       # eager frame, capture, first replay
        pos = pos[:, -1:] + 1
        f = model.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), amask, pos, 0.9, 50)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(frames):
        pos = pos[:, -1:] + 1
        f = model.generate_frame(torch.cat([f.long(), pad], 1).unsqueeze(1), amask, pos, 0.9, 50)
    torch.cuda.synchronize()
    return B * frames / (time.time() - t0)


def _random_bank(model, mods, dev, n=16):
    """``n`` random r = 8 adapters of ``model`` with non-zero B (lora_bank_main's)."""
    from csm.training.lora import LoRAState
    bank = []
    for s in range(n):
        st = LoRAState(model, 8, 16.0, 0.0, mods, None, False, seed=s, grad=False)
        with torch.no_grad():
            gb = torch.Generator(device=dev).manual_seed(100 + s)
            for ad in st.adapters.values():
                ad.B[:, :8].copy_((torch.randn(ad.B.shape[0], 8, generator=gb, device=dev) * 0.02).to(torch.bfloat16))
        bank.append(st)
    return bank


def lora_bank_main(mods):
    """GEN_LORA_BANK=q_proj,v_proj (or all): CSM-1B random init, 16 random r = 8 adapters with non-zero B.  For B = 4, 8, 16
    (GEN_BANK_SIZES): (a) one adapter per utterance - distinct adapters, every fourth row without; (b) the same batch without
    adapters; (c) the utterances one at a time, each with its adapter live as model.lora (today's only option; its aggregate
    frames/s is the one-utterance rate whatever B).  Alternated in one process, GEN_ROUNDS rounds, best of each."""
    dev = "cuda:0"
    mods = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"] if mods == "all" else mods.split(",")
    model = Model(csm_1b_args(), device=dev, seed=0)
    bank = _random_bank(model, mods, dev)
    frames = int(os.environ.get("GEN_FRAMES", 50))
    sizes = [int(v) for v in os.environ.get("GEN_BANK_SIZES", "4,8,16").split(",")]
    rounds = int(os.environ.get("GEN_ROUNDS", 2))
    res = {}
    for _ in range(rounds):
        for B in sizes:
            rows = [None if b % 4 == 3 else bank[b] for b in range(B)]
            res.setdefault(("none", B), []).append(decode_fps_batch(model, B, None, frames))
            res.setdefault(("bank", B), []).append(decode_fps_batch(model, B, rows, frames))
        one = []
        for s in (0, 1):                                                     # (c): live adapter, one utterance
            model.lora = bank[s]
            try:
                one.append(decode_fps(model, frames))
            finally:
                model.lora = None
        res.setdefault(("live1", 1), []).append(max(one))
    live1 = max(res[("live1", 1)])
    print(f"LoRA bank {','.join(mods)} r=8, 16 adapters: one utterance at a time with its adapter live (c): "
          f"{[round(x, 1) for x in res[('live1', 1)]]} -> best {live1:.1f} frames/s", flush=True)
    for B in sizes:
        a, b = max(res[("bank", B)]), max(res[("none", B)])
        print(f"GEN_LORA_BANK B={B:2d}: (a) per-row adapters {[round(x, 1) for x in res[('bank', B)]]} (b) no adapters "
              f"{[round(x, 1) for x in res[('none', B)]]} frames/s aggregate -> best (a) {a:.1f} / (b) {b:.1f} = {a / b:.3f}x; "
              f"(a) / (c) = {a / live1:.2f}x", flush=True)


def fp8_bank_main(mods):
    """GEN_FP8=1 GEN_LORA_BANK=q_proj,v_proj (or all): CSM-1B random init, 16 random r = 8 adapters (GEN_LORA_BANK's bank and
    rows: distinct adapters, every fourth row without).  Decode-loop frames/s (captured graph) of four legs on ONE model,
    alternated in one process - bf16 + bank, FP8 + bank (model.fp8_adapters), FP8 without adapters, bf16 without adapters - at
    B = GEN_BANK_SIZES (default 4,8,16), GEN_ROUNDS alternated repeats (default 3), best of each."""
    dev = "cuda:0"
    mods = ["q_proj", "k_proj", "v_proj", "output_proj", "w1", "w2", "w3"] if mods == "all" else mods.split(",")
    model = Model(csm_1b_args(), device=dev, seed=0)
    bank = _random_bank(model, mods, dev)
    model.fp8_adapters = True
    frames = int(os.environ.get("GEN_FRAMES", 50))
    sizes = [int(v) for v in os.environ.get("GEN_BANK_SIZES", "4,8,16").split(",")]
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    legs = (("bf16+bank", "bf16", True), ("fp8+bank", "fp8", True), ("fp8", "fp8", False), ("bf16", "bf16", False))
    res = {}
    for _ in range(rounds):
        for B in sizes:
            rows = [None if b % 4 == 3 else bank[b] for b in range(B)]
            for name, mode, banked in legs:
                model.decode_weights = mode
                res.setdefault((name, B), []).append(decode_fps_batch(model, B, rows if banked else None, frames))
                st = model._decode_state
                assert (st.bb.w8 is not None) == (mode == "fp8") and (st.bb.lora_rows is not None) == banked
    model.decode_weights = "bf16"
    print(f"GEN_FP8 + GEN_LORA_BANK {','.join(mods)} r=8, 16 adapters, {frames} frames, {rounds} alternated repeats (best of each)", flush=True)
    for B in sizes:
        best = {name: max(res[(name, B)]) for name, _, _ in legs}
        print(f"GEN_FP8_BANK B={B:2d}: " + " ".join(f"{name} {[round(x, 1) for x in res[(name, B)]]}" for name, _, _ in legs) +
              f" frames/s aggregate -> best fp8+bank {best['fp8+bank']:.1f} / bf16+bank {best['bf16+bank']:.1f} = "
              f"{best['fp8+bank'] / best['bf16+bank']:.3f}x; fp8+bank / fp8 = {best['fp8+bank'] / best['fp8']:.3f}x; "
              f"bf16+bank / bf16 = {best['bf16+bank'] / best['bf16']:.3f}x; fp8 / bf16 = {best['fp8'] / best['bf16']:.3f}x", flush=True)


def fp8_main():
    """GEN_FP8=1: CSM-1B random init, decode-loop frames/s (captured graph) with bf16 and with FP8 (weight-only e4m3) decode
    weights on ONE model, alternated in one process (GEN_ROUNDS rounds, best of each) at B = GEN_BATCH_SIZES (default 1,4,16),
    plus the bytes of layer-product weights a decode frame's steps stream in each mode.  GEN_FP8_TEACHER=1 adds the quantisation
    loss on these RANDOM weights (teacher-forced, shared noise): relative error of codebook-0 logits, share of agreeing codes."""
    dev = "cuda:0"
    model = Model(csm_1b_args(), device=dev, seed=0)
    frames = int(os.environ.get("GEN_FRAMES", 100))
    sizes = [int(v) for v in os.environ.get("GEN_BATCH_SIZES", "1,4,16").split(",")]
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    modes = os.environ.get("GEN_FP8_MODES", "bf16,fp8").split(",")     # (one mode alone: a profiler run of that mode)
    res, nbytes = {}, {}
    for _ in range(rounds):
        for B in sizes:
            for mode in modes:
                model.decode_weights = mode
                res.setdefault((mode, B), []).append(decode_fps_batch(model, B, None, frames))
                st = model._decode_state
                nbytes[mode] = (st.bb.weight_bytes(), st.dc.weight_bytes())
    model.decode_weights = "bf16"
    for mode in modes:
        bb, dc = nbytes[mode]
        print(f"GEN_FP8 decode weights {mode}: backbone {bb / 2**20:.1f} MiB + depth decoder {dc / 2**20:.1f} MiB per step "
              f"(layer products; heads, embeddings and projection stay bf16 in both modes)", flush=True)
    if len(modes) < 2:
        for B in sizes:
            print(f"GEN_FP8 B={B:2d}: {modes[0]} {[round(x, 1) for x in res[(modes[0], B)]]} frames/s aggregate", flush=True)
        return
    for B in sizes:
        a, b = max(res[("fp8", B)]), max(res[("bf16", B)])
        print(f"GEN_FP8 B={B:2d}: fp8 {[round(x, 1) for x in res[('fp8', B)]]} bf16 {[round(x, 1) for x in res[('bf16', B)]]} "
              f"frames/s aggregate -> best fp8 {a:.1f} / bf16 {b:.1f} = {a / b:.3f}x", flush=True)
    if os.environ.get("GEN_FP8_TEACHER") == "1":
        fp8_loss(model)


def fp8_loss(model, B=4, frames=8, prompt=40):
    """Teacher-forced FP8 vs bf16 on the same (random) weights with shared noise: share of agreeing codes and the relative
    error of the codebook-0 logits of every decode frame (max |diff| / max |bf16 logits|)."""
    from csm.hip import ops
    dev = model.device
    K, V = model.args.audio_num_codebooks, model.args.audio_vocab_size
    g = torch.Generator().manual_seed(0)
    tok = torch.zeros(B, prompt, K + 1, dtype=torch.long)
    tok[:, :, K] = torch.randint(0, model.args.text_vocab_size, (B, prompt), generator=g)
    msk = torch.zeros(B, prompt, K + 1, dtype=torch.bool)
    msk[:, :, K] = True
    amask = torch.cat([torch.ones(B, K, dtype=torch.bool), torch.zeros(B, 1, dtype=torch.bool)], 1).unsqueeze(1)
    eng = model.engine
    body = eng._frame_tail_body
    out = {}
    for mode in ("bf16", "fp8"):
        model.decode_weights = mode
        model.setup_caches(B)
        hs, fr = [], []
        eng._frame_tail_body = lambda st, h, t, k: (hs.append(h.clone()), body(st, h, t, k))[1]
        model.use_hip_graph = False
        try:
            t, mk, pos = tok, msk, torch.arange(prompt).unsqueeze(0).repeat(B, 1)
            for step in range(frames):
                gn = torch.Generator().manual_seed(100 + step)
                noise = [torch.empty(B, V).exponential_(1, generator=gn) for _ in range(K)]
                f = model.generate_frame(t.to(dev), mk.to(dev), pos.to(dev), 0.9, 50, noise=noise).cpu()
                fr.append(f)
                nxt = out["bf16"][0][step] if mode == "fp8" else f
                t = torch.cat([nxt.long(), torch.zeros(B, 1, dtype=torch.long)], 1).unsqueeze(1)
                mk, pos = amask, pos[:, -1:] + 1
        finally:
            model.use_hip_graph = True
            del eng._frame_tail_body
        out[mode] = (torch.stack(fr), hs)
    model.decode_weights = "bf16"
    agree = (out["bf16"][0] == out["fp8"][0]).float().mean().item()
    agree0 = (out["bf16"][0][:, :, 0] == out["fp8"][0][:, :, 0]).float().mean().item()
    rel = []
    for hb, hf in zip(out["bf16"][1][1:], out["fp8"][1][1:]):
        lg = [torch.empty(B, model.vocab_pad, dtype=torch.float32, device=dev) for _ in range(2)]
        ops.gemv(hb, model.block("codebook0_head.padded"), lg[0])
        ops.gemv(hf, model.block("codebook0_head.padded"), lg[1])
        rel.append(((lg[0] - lg[1])[:, :V].abs().max() / lg[0][:, :V].abs().max()).item())
    print(f"GEN_FP8 quantisation loss on RANDOM CSM-1B weights (B={B}, {frames} teacher-forced frames, shared noise): codes agree "
          f"{agree:.1%} (codebook 0: {agree0:.1%}); codebook-0 logits of the decode frames: relative error max {max(rel):.3g}, "
          f"mean {sum(rel) / len(rel):.3g}", flush=True)


def stream_main():
    """GEN_STREAM=1: for each chunk size, generate() and generate_stream() alternate (GEN_ROUNDS rounds, same seed, so the
    same frames); the first chunk counts as arrived when its samples are on the host."""
    dev = "cuda:0"
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    frames = int(os.environ.get("GEN_FRAMES", 125))
    ms = 80 * frames
    gen.generate(text, 1, ctx, max_audio_length_ms=80 * 5)                           # warm-up: allocator, graph capture
    for _ in gen.generate_stream(text, 1, ctx, max_audio_length_ms=80 * 5, chunk_frames=2):
        pass

    def plain():
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        audio = gen.generate(text, 1, ctx, max_audio_length_ms=ms)
        audio.cpu()
        dt = time.perf_counter() - t0
        return dt, dt, audio.numel() / 1920

    def streamed(c):
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first, n = None, 0
        for chunk in gen.generate_stream(text, 1, ctx, max_audio_length_ms=ms, chunk_frames=c):
            chunk.cpu()
            if first is None:
                first = time.perf_counter() - t0
            n += chunk.numel()
        return first, time.perf_counter() - t0, n / 1920

    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    for c in (1, 2, 4):
        res = {"generate": [], "stream": []}
        for _ in range(rounds):
            res["generate"].append(plain())
            res["stream"].append(streamed(c))
        for name, runs in res.items():
            first, total, nfr = min(runs, key=lambda r: r[1])
            print(f"chunk_frames={c} {name:8s}: first audio {first * 1e3:7.1f} ms, total {total * 1e3:7.1f} ms, {nfr:.0f} frames, "
                  f"{nfr / total:.1f} frames/s (best of {rounds}; totals {[round(r[1] * 1e3, 1) for r in runs]} ms)")
        ratio = min(r[1] for r in res["stream"]) / min(r[1] for r in res["generate"])
        print(f"chunk_frames={c}: stream / generate total wall time = {ratio:.3f}")


def sweep_main():
    """GEN_BATCH_SWEEP=1: ``run_batch``'s setting (5 s of context on alternate rows, GEN_FRAMES frames) for every batch size of
    GEN_BATCH_SIZES (default 1,4,8,16) on one model; one line per size."""
    dev = "cuda:0"
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    frames = int(os.environ.get("GEN_FRAMES", 125))
    for nb in [int(v) for v in os.environ.get("GEN_BATCH_SIZES", "1,4,8,16").split(",")]:
        texts = [f"utterance number {i}: the quick brown fox jumps over the lazy dog" for i in range(nb)]
        ctxs = [ctx if i % 2 == 0 else [] for i in range(nb)]
        for _ in range(2):                                                   # the first run captures the batch's frame graph
            torch.cuda.synchronize()
            t0 = time.time()
            outs = gen.generate_batch(texts, list(range(nb)), ctxs, max_audio_length_ms=80 * frames)
            torch.cuda.synchronize()
            dt = time.time() - t0
        tot = sum(o.numel() for o in outs) / 1920
        print(f"GEN_BATCH_SWEEP B={nb:2d}: {tot:.0f} frames in {dt:.3f} s -> {tot / dt:.1f} frames/s aggregate, "
              f"{dt / max(tot / nb, 1) * 1e3:.2f} ms per batch frame ({tot * 0.08 / dt:.2f}x real time aggregate)", flush=True)


def attn_append_micro(dev, H=32, KV=8, HD=64, S_max=2048, iters=200):
    """csm_attn_append at (n, pos0) against csm_attn_fwd at S = pos0 + n (CSM-1B backbone heads): device time per launch."""
    for n, pos0 in ((64, 1024), (200, 1800)):
        S = pos0 + n
        qkv = torch.randn(S, (H + 2 * KV) * HD, device=dev).to(torch.bfloat16)
        kc = torch.randn(1, KV, S_max, HD, device=dev).to(torch.bfloat16)
        vc = torch.randn(1, KV, S_max, HD, device=dev).to(torch.bfloat16)
        new = qkv[pos0:].contiguous()
        o_app = torch.empty(n, H * HD, dtype=torch.bfloat16, device=dev)
        o_fwd = torch.empty(S, H * HD, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(1, H, S, dtype=torch.float32, device=dev)
        calls = {"csm_attn_append": lambda: ops.attn_append(new, kc, vc, o_app, 0, pos0, H, KV, HD),
                 "csm_attn_fwd": lambda: ops.attn_fwd(qkv, o_fwd, lse, 1, S, H, KV, HD)}
        us = {k: [] for k in calls}
        for _ in range(5):                                       # alternated repeats; the first one also warms up
            for name, f in calls.items():
                for _ in range(20):
                    f()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    f()
                b.record()
                torch.cuda.synchronize()
                us[name].append(a.elapsed_time(b) * 1e3 / iters)
        fl = 4.0 * n * (pos0 + (n + 1) / 2) * HD * H
        print(f"attn micro n={n:3d} pos0={pos0:4d}: csm_attn_append {min(us['csm_attn_append']):6.1f} us "
              f"({[round(x, 1) for x in us['csm_attn_append']]}; {fl / min(us['csm_attn_append']) / 1e6:.1f} TFLOP/s) vs csm_attn_fwd S={S} "
              f"{min(us['csm_attn_fwd']):6.1f} us ({[round(x, 1) for x in us['csm_attn_fwd']]})")


def conversation_main():
    """GEN_CONVERSATION=1 (see the module docstring).  GEN_ROUNDS timed dialogues of each kind (default 5), alternated; the
    first chunk counts as arrived when its samples are on the host."""
    dev = "cuda:0"
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    frames = int(os.environ.get("GEN_FRAMES", 63))
    turns = int(os.environ.get("GEN_TURNS", 8))
    rounds = int(os.environ.get("GEN_ROUNDS", 5))
    ms = 80 * frames
    g = torch.Generator(device=dev).manual_seed(1)
    script = []
    for t in range(turns):
        if t % 2 == 0:
            script.append(("say", t % 4 // 2, f"turn {t + 1}: the quick brown fox jumps over the lazy dog"))
        else:
            script.append(("hear", 1 - (t - 1) % 4 // 2, f"turn {t + 1}: and what did the dog do",
                           torch.randn(5 * 24000, device=dev, generator=g) * 0.1))

    def timed(stream):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first, parts = None, []
        for chunk in stream():
            chunk.cpu()
            if first is None:
                first = time.perf_counter() - t0
            parts.append(chunk)
        return first, time.perf_counter() - t0, torch.cat(parts)

    def dialogue(kind):
        """One pass over the script; per turn (first chunk s or None, total s)."""
        torch.manual_seed(0)
        conv, segs, out = (gen.conversation() if kind == "conversation" else None), [], []
        for item in script:
            if item[0] == "say":
                _, spk, text = item
                if conv is not None:
                    first, total, audio = timed(lambda: conv.generate_stream(text, spk, max_audio_length_ms=ms, chunk_frames=2))
                else:
                    first, total, audio = timed(lambda: gen.generate_stream(text, spk, segs, max_audio_length_ms=ms, chunk_frames=2))
                    segs.append(Segment(spk, text, audio))
                assert audio.numel() == frames * 1920, "a random-init model should not emit EOS"
                out.append((first, total))
            else:
                _, spk, text, audio = item
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if conv is not None:
                    conv.add(Segment(spk, text, audio))
                    torch.cuda.synchronize()
                else:
                    segs.append(Segment(spk, text, audio))
                out.append((None, time.perf_counter() - t0))
        return out, (conv.tokens.shape[0] if conv is not None else None)

    for kind in ("conversation", "stateless"):                      # warm-up dialogue of each: allocator, graph capture, every shape
        dialogue(kind)
    res = {"conversation": [], "stateless": []}
    hist = None
    for _ in range(rounds):
        for kind in res:
            out, n = dialogue(kind)
            res[kind].append(out)
            hist = n or hist
    med = lambda xs: sorted(xs)[len(xs) // 2]                        # noqa: E731
    print(f"GEN_CONVERSATION: {turns} turns, {frames} frames per spoken turn, chunk_frames=2, {rounds} alternated rounds; history at "
          f"the end {hist} positions.  ms as median [min..max]")
    for t, item in enumerate(script):
        line = f"turn {t + 1} ({item[0]:4s})"
        for kind in res:
            tot = [r[t][1] * 1e3 for r in res[kind]]
            if item[0] == "say":
                fc = [r[t][0] * 1e3 for r in res[kind]]
                line += f" | {kind}: first chunk {med(fc):7.1f} [{min(fc):6.1f}..{max(fc):6.1f}], total {med(tot):7.1f} [{min(tot):6.1f}..{max(tot):6.1f}]"
            else:
                line += f" | {kind}: add {med(tot):6.1f} [{min(tot):5.1f}..{max(tot):5.1f}]"
        print(line)
    attn_append_micro(dev)


def _timed(fn, iters):
    """Mean seconds per call of ``fn`` over ``iters`` calls between two device synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def serve_main():
    """GEN_SERVE=1: the running batch (Generator.serve) on CSM-1B random init, 16 slots, chunk_frames 4, 5 s of context each.
    (a) the rows-codec step at R = 1, 4, 16 against R consecutive MimiDecodeStream.step calls, alternated, best of GEN_ROUNDS;
    (b) the whole server step at 16 active rows (4 frames + codec) against the 320 ms of audio it makes per stream, aggregate
    frames/s next to generate_batch at B = 16, and a staggered-arrival, mixed-length workload; (c) the stall a join with 5 s of
    context imposes on 15 running rows (a step with one join minus the median step without).  GEN_SERVE_PARTS=a: (a) alone."""
    dev = "cuda:0"
    n = 4
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    # ---- (a) codec
    singles = [codec.decode_stream(max_chunk_frames=n) for _ in range(16)]
    rows = codec.decode_stream_rows(slots=16, max_chunk_frames=n)
    for s in range(16):
        rows.open(s)
    for R in (1, 4, 16):
        codes = torch.randint(0, 2048, (R, 32, n), device=dev, generator=g)

        def one_by_one():
            for r in range(R):
                singles[r].step(codes[r:r + 1])

        def together():
            rows.step(list(range(R)), codes)

        for f in (one_by_one, together):
            _timed(f, 3)
        best = {"single": 1e9, "rows": 1e9}
        for _ in range(rounds):
            best["single"] = min(best["single"], _timed(one_by_one, 20))
            best["rows"] = min(best["rows"], _timed(together, 20))
        print(f"GEN_SERVE (a) codec step, {n} frames, R={R:2d}: rows {best['rows'] * 1e3:.2f} ms, {R} single steps "
              f"{best['single'] * 1e3:.2f} ms -> {best['single'] / best['rows']:.2f}x", flush=True)
    del singles, rows
    if os.environ.get("GEN_SERVE_PARTS", "abc") == "a":                       # the codec comparison alone
        return
    # ---- (b) server step at 16 active rows
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    frames = int(os.environ.get("GEN_FRAMES", 125))
    for seeded in (True, False):                                             # per-row generators against the whole-buffer draw
        srv = gen.serve(slots=16, chunk_frames=n)
        for i in range(16):
            srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i if seeded else None, max_audio_length_ms=80 * 400)
        t_first = _timed(srv.step, 1)                                        # 16 prefills + the first chunk
        _timed(srv.step, 2)                                                  # eager warm-up frame, graph capture
        steps = sorted(_timed(srv.step, 1) for _ in range(20))
        med = steps[len(steps) // 2]
        print(f"GEN_SERVE (b) server step, 16 rows x {n} frames ({'per-row seeds' if seeded else 'no seeds'}): median {med * 1e3:.1f} ms "
              f"(min {steps[0] * 1e3:.1f}, max {steps[-1] * 1e3:.1f}) for {n * 80} ms of audio per stream -> {n * 0.08 / med:.2f}x real "
              f"time per stream, {16 * n / med:.1f} frames/s aggregate; first step with 16 joins {t_first * 1e3:.0f} ms", flush=True)
    # ---- (c) join stall: 15 rows running, one request with 5 s of context joins
    srv = gen.serve(slots=16, chunk_frames=n)
    for i in range(15):
        srv.submit(f"utterance number {i}: {text}", i, ctx, max_audio_length_ms=80 * 400)
    _timed(srv.step, 3)
    plain = sorted(_timed(srv.step, 1) for _ in range(9))[4]
    joins, subs = [], []
    for j in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        srv.submit(f"late comer {j}: {text}", 3, ctx, max_audio_length_ms=80 * n)      # leaves after one chunk
        torch.cuda.synchronize()
        subs.append(time.perf_counter() - t0)
        joins.append(_timed(srv.step, 1))
        assert srv.last_join_rows == 1
        _timed(srv.step, 1)
    joins, subs = sorted(joins[1:]), sorted(subs[1:])                       # (the first join warms the 16-row frame tail up)
    print(f"GEN_SERVE (c) join with 5 s of context into 15 running rows: step {joins[len(joins) // 2] * 1e3:.1f} ms against "
          f"{plain * 1e3:.1f} ms without -> stall {(joins[len(joins) // 2] - plain) * 1e3:.1f} ms; submit (tokenise + Mimi encode) "
          f"{subs[len(subs) // 2] * 1e3:.1f} ms", flush=True)
    # ---- generate_batch at B = 16 and a staggered, mixed-length served workload, same job
    texts = [f"utterance number {i}: {text}" for i in range(16)]
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = gen.generate_batch(texts, list(range(16)), [ctx] * 16, max_audio_length_ms=80 * frames)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    tot = sum(o.numel() for o in outs) / 1920
    print(f"GEN_SERVE generate_batch B=16, {frames} frames, 5 s of context each: {tot:.0f} frames in {dt:.3f} s -> {tot / dt:.1f} "
          f"frames/s aggregate (prefills and the 16 decodes included)", flush=True)
    for _ in range(2):
        srv = gen.serve(slots=16, chunk_frames=n)
        lens = [frames // 4 + (i * 37) % (frames - frames // 4 + 1) for i in range(32)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reqs, first = [], {}
        for i in range(8):
            reqs.append(srv.submit(texts[i % 16], i, ctx, max_audio_length_ms=80 * lens[i]))
        while srv.queued or srv.active or len(reqs) < 32:
            for k in range(2):                                              # two arrivals per chunk until all 32 are in
                if len(reqs) < 32:
                    reqs.append(srv.submit(texts[len(reqs) % 16], len(reqs), ctx, max_audio_length_ms=80 * lens[len(reqs)]))
            srv.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    tot = sum(r.audio().numel() for r in reqs) / 1920
    print(f"GEN_SERVE served 32 staggered requests of {min(lens)}..{max(lens)} frames, 5 s of context each, 16 slots: {tot:.0f} frames "
          f"in {dt:.3f} s -> {tot / dt:.1f} frames/s aggregate (Mimi encode, prefills, streaming decode included)", flush=True)


def _spread(v):
    v = sorted(v)
    return f"median {v[len(v) // 2] * 1e3:.3f} ms ({v[0] * 1e3:.3f} .. {v[-1] * 1e3:.3f})"


def serve_streams_main():
    """GEN_SERVE_STREAMS=1: more listeners than slots (Generator.serve(streams=N)) on CSM-1B random init, 16 slots, chunk_frames 4,
    5 s of context each - GEN_SERVE's setting.  (a) Rotation cost: the steady server step with 32 streams in fair share (16 rows
    parked and 16 resumed at every chunk boundary) against the same step with 16 streams (no rotation), GEN_ROUNDS (default 3)
    alternated repeats, medians of 20 steps, the difference next to the repeats' own spread; and DecodeState.park_rows /
    resume_rows at R = 1 / 4 / 16 (rings included: a row_processors state) against R park_row / resume_row calls plus the ring
    and token copies they stand for.  (b) Capacity under the wall clock: max_lead_ms 2000, streams in GEN_STREAMS (default
    16,32,64,96,128), two arrivals per server step, every request GEN_FRAMES (default 100) frames; per value the underruns (a
    chunk delivered after its listener's buffer ran dry), submit -> first chunk (median, worst) and aggregate frames/s.
    GEN_SERVE_PARTS=a / b: one part alone."""
    dev = "cuda:0"
    n = 4
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    parts = os.environ.get("GEN_SERVE_PARTS", "ab")
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"

    def steady(streams, **kw):
        srv = gen.serve(slots=16, chunk_frames=n, streams=streams, **kw)
        for i in range(streams):
            srv.submit(f"utterance number {i}: {text}", i % 16, ctx, seed=i, max_audio_length_ms=80 * 400)
        _timed(srv.step, 6)                                                  # admissions, eager warm-up frame, graph capture
        before = dict(srv.stats)
        steps = sorted(_timed(srv.step, 1) for _ in range(20))
        moved = (srv.stats["parks"] - before["parks"], srv.stats["resumes"] - before["resumes"])
        return steps[len(steps) // 2], moved

    if "a" in parts:
        for streams in (16, 32):
            steady(streams)
        res = {16: [], 32: []}
        for _ in range(rounds):
            for streams in (16, 32):
                med, moved = steady(streams)
                res[streams].append(med)
        assert moved == (16 * 20, 16 * 20), moved                            # (the last one ran with 32: 16 out and 16 in per step)
        for streams in (16, 32):
            print(f"GEN_SERVE_STREAMS (a) server step, 16 rows x {n} frames, {streams} streams "
                  f"({'16 rows parked + 16 resumed per step' if streams == 32 else 'no rotation'}): medians of 20 steps "
                  f"{_spread(res[streams])}", flush=True)
        d = sorted(b - a for a, b in zip(res[16], res[32]))
        own = max(max(v) - min(v) for v in res.values())
        print(f"GEN_SERVE_STREAMS (a) rotation - none: {d[len(d) // 2] * 1e3:+.2f} ms per step ({d[0] * 1e3:+.2f} .. {d[-1] * 1e3:+.2f}); "
              f"the repeats' own spread {own * 1e3:.2f} ms", flush=True)
        # park_rows / resume_rows against the one-row calls and the copies they stand for, on a state that keeps rings
        srv = gen.serve(slots=16, chunk_frames=n, row_sampling=True, row_processors=True)
        for i in range(16):
            srv.submit(f"utterance number {i}: {text}", i, ctx, max_audio_length_ms=80 * 400)
        _timed(srv.step, 3)
        st, samp, tok = srv._state, srv._state.sampler, srv._tok
        with torch.inference_mode():
            for R in (1, 4, 16):
                rows = list(range(R))
                held = {}

                def park_all():
                    held["rows"], held["tok"] = st.park_rows(rows), tok[rows]

                def resume_all():
                    st.resume_rows(rows, held["rows"])
                    tok[rows] = held["tok"]

                def park_each():
                    held["each"] = [(st.park_row(b, st.row_pos[b] + 1), samp.code_hist[b].clone(), samp.hist_frame[b:b + 1].clone(),
                                     tok[b].clone()) for b in rows]

                def resume_each():
                    for b, (kv, ring, frame, t) in zip(rows, held["each"]):
                        st.resume_row(b, kv)
                        samp.code_hist[b].copy_(ring)
                        samp.hist_frame[b:b + 1].copy_(frame)
                        tok[b].copy_(t)

                for f in (park_all, resume_all, park_each, resume_each):
                    _timed(f, 5)
                t = {f.__name__: [] for f in (park_all, resume_all, park_each, resume_each)}
                for _ in range(rounds):
                    for f in (park_all, resume_all, park_each, resume_each):
                        t[f.__name__].append(_timed(f, 30))
                print(f"GEN_SERVE_STREAMS (a) {st.row_pos[0] + 1} positions, R={R:2d}: park_rows {_spread(t['park_all'])} against {R} "
                      f"park_row + copies {_spread(t['park_each'])}; resume_rows {_spread(t['resume_all'])} against {R} resume_row + "
                      f"copies {_spread(t['resume_each'])}", flush=True)
        del srv, st, samp, tok
    if "b" not in parts:
        return
    frames = int(os.environ.get("GEN_FRAMES", 100))
    lead = 2000.0

    def capacity(streams):
        srv = gen.serve(slots=16, chunk_frames=n, streams=streams, max_lead_ms=lead)
        reqs, t_sub, t_first, heard, under = [], {}, {}, {}, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while True:
            for _ in range(2):                                              # two arrivals per server step until all are in
                if len(reqs) < streams:
                    t_sub[len(reqs)] = time.perf_counter()
                    reqs.append(srv.submit(f"utterance number {len(reqs)}: {text}", len(reqs) % 16, ctx, seed=len(reqs),
                                           max_audio_length_ms=80 * frames))
            due = srv.next_due()
            if due is None:
                if len(reqs) == streams:
                    break
                continue
            if due > 0:
                time.sleep(due)
                continue
            out = srv.step()
            torch.cuda.synchronize()                                        # (the chunk is heard: its samples are there)
            t = time.perf_counter()
            for r, a, _ in out:
                if r.id in t_first:                                         # what the listener had left when this chunk came
                    if heard[r.id] - (t - t_first[r.id]) * 1000.0 < 0:
                        under += 1
                elif a.numel():
                    t_first[r.id] = t
                heard[r.id] = heard.get(r.id, 0.0) + a.numel() / 24.0
        dt = time.perf_counter() - t0
        lat = sorted(t_first[i] - t_sub[i] for i in range(streams))
        return under, lat[len(lat) // 2], lat[-1], sum(r._emitted for r in reqs) / dt, srv.stats

    capacity(16)                                                             # warm-up: graph capture, allocator
    for streams in [int(v) for v in os.environ.get("GEN_STREAMS", "16,32,64,96,128").split(",")]:
        under, med, worst, fps, stats = capacity(streams)
        print(f"GEN_SERVE_STREAMS (b) {streams:3d} streams x {frames} frames, max_lead_ms {lead:.0f}, two arrivals per step: {under} underruns; "
              f"submit -> first chunk median {med * 1e3:.0f} ms, worst {worst * 1e3:.0f} ms; {fps:.1f} frames/s aggregate "
              f"({streams * 12.5:.1f} frames/s is real time for all); {stats['steps']} steps, {stats['parks']} parks in "
              f"{stats['park_launches']} launches, {stats['resumes']} resumes in {stats['resume_launches']}", flush=True)


def voice_main():
    """GEN_VOICE=1: a voice prompt prefilled once (Generator.voice) against the same segments given as context, on CSM-1B random
    init, 16 slots, chunk_frames 4, 5 s of context - the two sides alternated, GEN_ROUNDS (default 3) repeats, each side's median
    (min .. max).  (a) DecodeState.fork_rows (csm_kv_fork_rows, one launch) against R resume_row calls at R = 1 / 4 / 16, 80 and
    441 positions; (b) aggregate frames/s of GEN_SERVE's staggered-arrival load with submit(context=) and submit(voice=);
    (c) in that load, the time from the submit call to the request's first chunk; (d) the step that admits 1 join next to 15
    running rows and the step that admits 16 joins (what a running row waits for its next chunk)."""
    from csm.engine import DecodeState
    dev = "cuda:0"
    n = 4
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    # ---- (a) the kernel against the strided copies
    with torch.inference_mode():
        st = DecodeState(model.engine, 16)
        kv = st.bb.kv
        for length in (80, 441):
            parked = torch.randn(kv.shape[0], 2, kv.shape[3], length, kv.shape[5], device=dev).to(kv.dtype)
            for R in (1, 4, 16):
                rows = list(range(R))

                def resumes():
                    for b in rows:
                        st.resume_row(b, parked)

                def fork():
                    st.fork_rows(rows, [parked] * R)

                for f in (resumes, fork):
                    _timed(f, 5)
                res = {"resume": [], "fork": []}
                for _ in range(rounds):
                    res["resume"].append(_timed(resumes, 50))
                    res["fork"].append(_timed(fork, 50))
                print(f"GEN_VOICE (a) {length} positions, R={R:2d}: fork_rows {_spread(res['fork'])}; {R} resume_row {_spread(res['resume'])}",
                      flush=True)
        del st, kv
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    texts = [f"utterance number {i}: {text}" for i in range(16)]
    frames = int(os.environ.get("GEN_FRAMES", 125))
    voice = gen.voice(ctx)
    print(f"GEN_VOICE voice of 5 s: {voice.positions} positions, {voice.nbytes / 1e6:.1f} MB", flush=True)
    kinds = {"context": lambda: {"context": ctx}, "voice": lambda: {"context": [], "voice": voice}}

    # ---- (b) + (c) the staggered load of GEN_SERVE: 8 requests at the start, two arrivals per chunk until all 32 are in
    def load(kind):
        srv = gen.serve(slots=16, chunk_frames=n)
        lens = [frames // 4 + (i * 37) % (frames - frames // 4 + 1) for i in range(32)]
        reqs, t_sub, t_first = [], {}, {}

        def submit():
            i = len(reqs)
            t = time.perf_counter()
            reqs.append(srv.submit(texts[i % 16], i, max_audio_length_ms=80 * lens[i], **kinds[kind]()))
            t_sub[reqs[-1]] = t
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(8):
            submit()
        while srv.queued or srv.active or len(reqs) < 32:
            for _ in range(2):
                if len(reqs) < 32:
                    submit()
            out = srv.step()
            torch.cuda.synchronize()                                    # (the chunk is heard: its samples are there)
            t = time.perf_counter()
            for r, _, _ in out:
                t_first.setdefault(r, t)
        dt = time.perf_counter() - t0
        tot = sum(r.audio().numel() for r in reqs) / 1920
        return tot / dt, sorted(t_first[r] - t_sub[r] for r in reqs)

    for kind in kinds:
        load(kind)                                                     # warm-up: graph capture, allocator
    res = {k: [] for k in kinds}
    for _ in range(rounds):
        for kind in kinds:
            res[kind].append(load(kind))
    for kind in kinds:
        fps = sorted(f for f, _ in res[kind])
        lat = sorted(l[len(l) // 2] for _, l in res[kind])
        worst = sorted(l[-1] for _, l in res[kind])
        print(f"GEN_VOICE (b) 32 staggered requests, 5 s of context as {kind}: {fps[len(fps) // 2]:.1f} frames/s aggregate "
              f"({fps[0]:.1f} .. {fps[-1]:.1f})", flush=True)
        print(f"GEN_VOICE (c) submit call -> first chunk, as {kind}: median request {_spread(lat)}; slowest request {_spread(worst)}",
              flush=True)

    # ---- (d) the admitting step: 1 join next to 15 running rows, 16 joins at once
    def one_join(kind):
        srv = gen.serve(slots=16, chunk_frames=n)
        for i in range(15):
            srv.submit(texts[i], i, max_audio_length_ms=80 * 400, **kinds[kind]())
        _timed(srv.step, 3)
        plain = sorted(_timed(srv.step, 1) for _ in range(5))[2]
        joins = []
        for j in range(3):
            srv.submit(f"late comer {j}: {text}", 3, max_audio_length_ms=80 * n, **kinds[kind]())      # leaves after one chunk
            torch.cuda.synchronize()
            joins.append(_timed(srv.step, 1))
            assert srv.last_join_rows == 1
            _timed(srv.step, 1)
        return sorted(joins[1:])[0], plain                             # (the first join warms the 16-row frame tail up)

    def sixteen_joins(kind):
        srv = gen.serve(slots=16, chunk_frames=n)
        for i in range(16):
            srv.submit(texts[i], i, max_audio_length_ms=80 * 400, **kinds[kind]())
        torch.cuda.synchronize()
        t = _timed(srv.step, 1)
        assert srv.last_join_rows == 16
        return t

    for kind in kinds:
        one_join(kind), sixteen_joins(kind)
    res = {k: {"one": [], "plain": [], "sixteen": []} for k in kinds}
    for _ in range(rounds):
        for kind in kinds:
            j, p = one_join(kind)
            res[kind]["one"].append(j)
            res[kind]["plain"].append(p)
            res[kind]["sixteen"].append(sixteen_joins(kind))
    for kind in kinds:
        r = res[kind]
        print(f"GEN_VOICE (d) as {kind}: step with 1 join into 15 running rows {_spread(r['one'])} against {_spread(r['plain'])} "
              f"without; step with 16 joins {_spread(r['sixteen'])}", flush=True)


def serve_sampling_main():
    """GEN_SERVE_SAMPLING=1: per-request sampling parameters (Generator.serve(row_sampling=True)).  (a) the sampler alone, 16 rows,
    V = 2051 in the model's padded logits buffer: csm_sample_topk at (50, 0.9) against csm_sample_topk_rows with that pair in every
    row and with a mixed list (five rows in the block-wide form) - 200 back-to-back launches between two synchronisations,
    alternated, median (min .. max) of GEN_ROUNDS repeats (default 5).  (b) the steady 16-row server step of GEN_SERVE's setting
    (CSM-1B random init, 16 slots, chunk_frames 4, 5 s of context each, per-row seeds): row_sampling off (the one-pair path - the
    yardstick), on with the server's pair in every row, on with a mixed list (four rows above topk 64); each leg is a fresh
    server, the three alternated GEN_ROUNDS times (default 3), per leg the median of 20 steps and the spread of the repeats'
    medians."""
    dev = "cuda:0"
    n = 4
    topk = [1, 2, 12, 50, 64, 65, 200, 2051, 50, 50, 64, 65, 1, 7, 300, 33]
    temp = [0.9, 0.5, 0.8, 0.9, 1.0, 1.3, 0.7, 1.0, 0.25, 2.0, 0.9, 0.9, 1.5, 0.6, 1.1, 0.95]
    # ---- (a) the sampler alone
    V, ld = 2051, 2112
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(16, ld, device=dev, generator=g) * 2
    q = torch.empty(16, V, device=dev).exponential_(1, generator=g)
    out = torch.empty(16, dtype=torch.int32, device=dev)
    k_eq, t_eq = torch.full((16,), 50, dtype=torch.int32, device=dev), torch.full((16,), 0.9, dtype=torch.float32, device=dev)
    k_mix, t_mix = torch.tensor(topk, dtype=torch.int32, device=dev), torch.tensor(temp, dtype=torch.float32, device=dev)
    legs = {"scalar (50, 0.9)": lambda: ops.sample_topk(lg, q, out, 50, 0.9, V=V),
            "rows, (50, 0.9) in every row": lambda: ops.sample_topk_rows(lg, q, out, k_eq, t_eq, V=V),
            "rows, mixed": lambda: ops.sample_topk_rows(lg, q, out, k_mix, t_mix, V=V)}
    rounds = int(os.environ.get("GEN_ROUNDS", 5))
    res = {name: [] for name in legs}
    for f in legs.values():
        _timed(f, 20)
    for _ in range(rounds):
        for name, f in legs.items():
            res[name].append(_timed(f, 200))
    for name, v in res.items():
        v.sort()
        print(f"GEN_SERVE_SAMPLING (a) sampler, 16 rows, V={V}: {name}: median {v[len(v) // 2] * 1e6:.2f} us per launch "
              f"(min {v[0] * 1e6:.2f}, max {v[-1] * 1e6:.2f}; {rounds} x 200 back-to-back launches)", flush=True)
    # ---- (b) the server step
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    topk_b = list(topk)
    topk_b[11] = 50                                                          # four rows above 64: 65, 200, 2051, 300
    modes = {"off": None, "on, equal": [(0.9, 50)] * 16, "on, mixed": list(zip(temp, topk_b))}
    meds = {name: [] for name in modes}
    for _ in range(rounds):
        for name, pairs in modes.items():
            srv = gen.serve(slots=16, chunk_frames=n, row_sampling=pairs is not None)
            for i in range(16):
                kw = {} if pairs is None else dict(temperature=pairs[i][0], topk=pairs[i][1])
                srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400, **kw)
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            meds[name].append(steps[len(steps) // 2])
    for name, v in meds.items():
        print(f"GEN_SERVE_SAMPLING (b) server step, 16 rows x {n} frames, row_sampling {name}: medians of 20 steps "
              f"{[round(x * 1e3, 2) for x in v]} ms -> median {sorted(v)[len(v) // 2] * 1e3:.2f} ms, spread of the repeats "
              f"{(max(v) - min(v)) * 1e3:.2f} ms", flush=True)
    off = sorted(meds["off"])[rounds // 2]
    for name in ("on, equal", "on, mixed"):
        on = sorted(meds[name])[rounds // 2]
        print(f"GEN_SERVE_SAMPLING (b) row_sampling {name} - off: {(on - off) * 1e3:+.2f} ms per step = {(on - off) * 1e6 / n:+.1f} us per "
              f"frame (off's own repeats span {(max(meds['off']) - min(meds['off'])) * 1e3:.2f} ms)", flush=True)


def serve_stats_main():
    """GEN_SERVE_STATS=1: per-request sampling statistics (Generator.serve(stats=True)), in the shape of GEN_SERVE_SAMPLING=1.
    (a) csm_sample_stats_rows alone at the frame's shape, 512 rows (32 codebooks x 16 slots), V = 2051 in the padded buffer -
    200 back-to-back launches between two synchronisations, median (min .. max) of GEN_ROUNDS repeats (default 5).  (b) the
    steady 16-row server step of GEN_SERVE's setting (CSM-1B random init, 16 slots, chunk_frames 4, 5 s of context each,
    per-row seeds): stats off (the yardstick) against on; each leg is a fresh server, the two alternated GEN_ROUNDS times
    (default 3), per leg the median of 20 steps and the spread of the repeats' medians."""
    dev = "cuda:0"
    n = 4
    V, ld, rows = 2051, 2112, 512
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(rows, ld, device=dev, generator=g) * 2
    codes = torch.randint(0, V, (rows,), device=dev, generator=g, dtype=torch.int32)
    out = torch.empty(3, rows, dtype=torch.float32, device=dev)
    f = lambda: ops.sample_stats_rows(lg, codes, out[0], out[1], out[2], V=V)      # noqa: E731
    rounds = int(os.environ.get("GEN_ROUNDS", 5))
    _timed(f, 20)
    v = sorted(_timed(f, 200) for _ in range(rounds))
    kernel = v[len(v) // 2]
    print(f"GEN_SERVE_STATS (a) csm_sample_stats_rows, {rows} rows, V={V}: median {kernel * 1e6:.2f} us per launch "
          f"(min {v[0] * 1e6:.2f}, max {v[-1] * 1e6:.2f}; {rounds} x 200 back-to-back launches)", flush=True)
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    meds = {"off": [], "on": []}
    for _ in range(rounds):
        for name in meds:
            srv = gen.serve(slots=16, chunk_frames=n, stats=name == "on")
            for i in range(16):
                srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400)
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            meds[name].append(steps[len(steps) // 2])
    for name, v in meds.items():
        print(f"GEN_SERVE_STATS (b) server step, 16 rows x {n} frames, stats {name}: medians of 20 steps "
              f"{[round(x * 1e3, 2) for x in v]} ms -> median {sorted(v)[len(v) // 2] * 1e3:.2f} ms, spread of the repeats "
              f"{(max(v) - min(v)) * 1e3:.2f} ms", flush=True)
    off, on = sorted(meds["off"])[rounds // 2], sorted(meds["on"])[rounds // 2]
    print(f"GEN_SERVE_STATS (b) stats on - off: {(on - off) * 1e3:+.3f} ms per step = {(on - off) * 1e6 / n:+.1f} us per frame = "
          f"{(on - off) / n / kernel:+.1f} stand-alone kernel times (off's own repeats span "
          f"{(max(meds['off']) - min(meds['off'])) * 1e3:.2f} ms)", flush=True)


def serve_filters_main():
    """GEN_SERVE_SAMPLING=filters: per-request top-p / min-p (Generator.serve(row_sampling=True, row_filters=True)), in the shape of
    GEN_SERVE_SAMPLING=1.  (a) the sampler alone, 16 rows, V = 2051 in the model's padded logits buffer, four forms: csm_sample_topk
    at (50, 0.9); csm_sample_topk_rows with that pair in every row; csm_sample_filtered_rows with that pair and (1, 0) in every row
    (filters off: the block-uniform skip); csm_sample_filtered_rows with mixed values - (50, 0.9) rows with top-p 0.9 / min-p 0.05
    (the one-wave filter) next to pure-nucleus rows, topk = V with top-p 0.9 (the block-wide filter: a second radix select) - and,
    shown separately, 16 pure-nucleus rows and 16 one-wave-filter rows.  200 back-to-back launches between two synchronisations,
    alternated, median (min .. max) of GEN_ROUNDS repeats (default 5).  (b) the steady 16-row server step of GEN_SERVE's setting:
    row_sampling on without row_filters (the yardstick), row_filters on with (1, 0) everywhere, on with mixed values (four
    pure-nucleus rows); each leg a fresh server, alternated GEN_ROUNDS times (default 3), per leg the median of 20 steps."""
    dev = "cuda:0"
    n = 4
    V, ld = 2051, 2112
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(16, ld, device=dev, generator=g) * 2
    q = torch.empty(16, V, device=dev).exponential_(1, generator=g)
    out = torch.empty(16, dtype=torch.int32, device=dev)

    def f32(v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    k_eq, t_eq = i32([50] * 16), f32([0.9] * 16)
    p_off, m_off = f32([1.0] * 16), f32([0.0] * 16)
    nucleus = [b % 4 == 3 for b in range(16)]                                # four pure-nucleus rows among twelve top-k 50 rows
    k_mix = i32([V if x else 50 for x in nucleus])
    p_mix, m_mix = f32([0.9] * 16), f32([0.0 if x else 0.05 for x in nucleus])
    k_all, m_all = i32([V] * 16), f32([0.05] * 16)
    legs = {"scalar (50, 0.9)": lambda: ops.sample_topk(lg, q, out, 50, 0.9, V=V),
            "rows, (50, 0.9) in every row": lambda: ops.sample_topk_rows(lg, q, out, k_eq, t_eq, V=V),
            "filtered, (50, 0.9) and filters off (1, 0) in every row": lambda: ops.sample_filtered_rows(lg, q, out, k_eq, t_eq, p_off, m_off, V=V),
            "filtered, mixed (12 rows top-k 50 + top-p 0.9 + min-p 0.05, 4 rows pure nucleus 0.9)":
                lambda: ops.sample_filtered_rows(lg, q, out, k_mix, t_eq, p_mix, m_mix, V=V),
            "filtered, one-wave filter in every row (top-k 50, top-p 0.9, min-p 0.05)":
                lambda: ops.sample_filtered_rows(lg, q, out, k_eq, t_eq, p_mix, m_all, V=V),
            "filtered, pure nucleus in every row (topk = V, top-p 0.9)":
                lambda: ops.sample_filtered_rows(lg, q, out, k_all, t_eq, p_mix, m_off, V=V)}
    rounds = int(os.environ.get("GEN_ROUNDS", 5))
    res = {name: [] for name in legs}
    for f in legs.values():
        _timed(f, 20)
    for _ in range(rounds):
        for name, f in legs.items():
            res[name].append(_timed(f, 200))
    for name, v in res.items():
        v.sort()
        print(f"GEN_SERVE_SAMPLING=filters (a) sampler, 16 rows, V={V}: {name}: median {v[len(v) // 2] * 1e6:.2f} us per launch "
              f"(min {v[0] * 1e6:.2f}, max {v[-1] * 1e6:.2f}; {rounds} x 200 back-to-back launches)", flush=True)
    if os.environ.get("GEN_SERVE_PARTS", "ab") == "a":
        return
    # ---- (b) the server step
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    mixed = [dict(topk=V, top_p=0.9) if x else dict(top_p=0.9, min_p=0.05) for x in nucleus]
    modes = {"off (row_sampling only)": None, "on, (1, 0) everywhere": [{}] * 16, "on, mixed": mixed}
    meds = {name: [] for name in modes}
    for _ in range(rounds):
        for name, kws in modes.items():
            srv = gen.serve(slots=16, chunk_frames=n, row_sampling=True, row_filters=kws is not None)
            for i in range(16):
                srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400, **(kws[i] if kws else {}))
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            meds[name].append(steps[len(steps) // 2])
    for name, v in meds.items():
        print(f"GEN_SERVE_SAMPLING=filters (b) server step, 16 rows x {n} frames, row_filters {name}: medians of 20 steps "
              f"{[round(x * 1e3, 2) for x in v]} ms -> median {sorted(v)[len(v) // 2] * 1e3:.2f} ms, spread of the repeats "
              f"{(max(v) - min(v)) * 1e3:.2f} ms", flush=True)
    off = sorted(meds["off (row_sampling only)"])[rounds // 2]
    for name in ("on, (1, 0) everywhere", "on, mixed"):
        on = sorted(meds[name])[rounds // 2]
        print(f"GEN_SERVE_SAMPLING=filters (b) row_filters {name} - off: {(on - off) * 1e3:+.2f} ms per step = {(on - off) * 1e6 / n:+.1f} "
              f"us per frame (off's own repeats span {(max(meds['off (row_sampling only)']) - min(meds['off (row_sampling only)'])) * 1e3:.2f} ms)",
              flush=True)


def serve_processors_main():
    """GEN_SERVE_SAMPLING=processors: a windowed repetition penalty and per-codebook parameters per request
    (Generator.serve(row_sampling=True, row_processors=True)), in the shape of GEN_SERVE_SAMPLING=filters.  (a) the sampler alone, 16
    rows, V = 2051 in the model's padded logits buffer, (50, 0.9) with top-p 0.9 / min-p 0.05 in every row (the one-wave filter):
    csm_sample_filtered_rows; csm_sample_processed_rows with penalty 1 (the block-uniform skip), with penalty 1.3 at window 16 and
    at window 64 (rings of random ids, frame 200, every row live).  200 back-to-back launches between two synchronisations,
    alternated, median (min .. max) of GEN_ROUNDS repeats (default 5).  (b) the steady 16-row server step of GEN_SERVE's setting:
    row_filters on (the yardstick: the code before the processors), row_processors on at identity (penalty 1 everywhere), on with a
    mixed load (penalties 1.0 .. 2.0 at windows 0 .. 64, an acoustic temperature / top-k of their own in half of the rows); each
    leg a fresh server, alternated GEN_ROUNDS times (default 3), per leg the median of 20 steps."""
    dev = "cuda:0"
    n = 4
    V, ld = 2051, 2112
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(16, ld, device=dev, generator=g) * 2
    q = torch.empty(16, V, device=dev).exponential_(1, generator=g)
    out = torch.empty(16, dtype=torch.int32, device=dev)

    def f32(v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    k, t, p, m = i32([50] * 16), f32([0.9] * 16), f32([0.9] * 16), f32([0.05] * 16)
    hist = torch.randint(0, V, (16, 64), device=dev, generator=g).to(torch.int32)
    frame, live = i32([200] * 16), i32([1] * 16)
    r_off, r_on, w16, w64 = f32([1.0] * 16), f32([1.3] * 16), i32([16] * 16), i32([64] * 16)

    def processed(r, w):
        return lambda: ops.sample_processed_rows(lg, q, out, k, t, p, m, r, w, hist, frame, live, advance=False, V=V)
    legs = {"filtered (csm_sample_filtered_rows)": lambda: ops.sample_filtered_rows(lg, q, out, k, t, p, m, V=V),
            "processed, penalty 1": processed(r_off, w64),
            "processed, penalty 1.3 at window 16": processed(r_on, w16),
            "processed, penalty 1.3 at window 64": processed(r_on, w64)}
    rounds = int(os.environ.get("GEN_ROUNDS", 5))
    res = {name: [] for name in legs}
    for f in legs.values():
        _timed(f, 20)
    for _ in range(rounds):
        for name, f in legs.items():
            res[name].append(_timed(f, 200))
    for name, v in res.items():
        v.sort()
        print(f"GEN_SERVE_SAMPLING=processors (a) sampler, 16 rows, V={V}: {name}: median {v[len(v) // 2] * 1e6:.2f} us per launch "
              f"(min {v[0] * 1e6:.2f}, max {v[-1] * 1e6:.2f}; {rounds} x 200 back-to-back launches)", flush=True)
    if os.environ.get("GEN_SERVE_PARTS", "ab") == "a":
        return
    # ---- (b) the server step
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    K = model.args.audio_num_codebooks
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    pens = [(1.0, 64), (1.3, 16), (2.0, 64), (1.1, 0), (1.5, 33), (1.3, 64), (1.2, 8), (1.7, 64)]
    mixed = []
    for b in range(16):
        kw = dict(top_p=0.9, min_p=0.05, repetition_penalty=pens[b % 8][0], repetition_window=pens[b % 8][1])
        if b % 2:
            kw.update(temperature=[0.9] + [0.7] * (K - 1), topk=[50] + [30] * (K - 1))
        mixed.append(kw)
    base = "row_filters (the yardstick)"
    modes = {base: (dict(row_filters=True), [{}] * 16), "row_processors, identity": (dict(row_processors=True), [{}] * 16),
             "row_processors, mixed": (dict(row_processors=True), mixed)}
    meds = {name: [] for name in modes}
    for _ in range(rounds):
        for name, (flags, kws) in modes.items():
            srv = gen.serve(slots=16, chunk_frames=n, row_sampling=True, **flags)
            for i in range(16):
                srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400, **kws[i])
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            meds[name].append(steps[len(steps) // 2])
    for name, v in meds.items():
        print(f"GEN_SERVE_SAMPLING=processors (b) server step, 16 rows x {n} frames, {name}: medians of 20 steps "
              f"{[round(x * 1e3, 2) for x in v]} ms -> median {sorted(v)[len(v) // 2] * 1e3:.2f} ms, spread of the repeats "
              f"{(max(v) - min(v)) * 1e3:.2f} ms", flush=True)
    off = sorted(meds[base])[rounds // 2]
    for name in ("row_processors, identity", "row_processors, mixed"):
        on = sorted(meds[name])[rounds // 2]
        print(f"GEN_SERVE_SAMPLING=processors (b) {name} - row_filters: {(on - off) * 1e3:+.2f} ms per step = "
              f"{(on - off) * 1e6 / n:+.1f} us per frame (row_filters' own repeats span {(max(meds[base]) - min(meds[base])) * 1e3:.2f} ms)",
              flush=True)


def serve_typical_main():
    """GEN_SERVE_SAMPLING=typical: locally typical sampling per request (Generator.serve(row_sampling=True, row_typical=True)), in the
    shape of GEN_SERVE_SAMPLING=processors.  (a) the sampler alone, 16 rows, V = 2051 in the model's padded logits buffer, temperature
    0.9, penalty 1.3 at window 16 (rings of random ids, frame 200, every row live), no top-p / min-p: csm_sample_processed_rows at
    top-k 50; csm_sample_typical_rows at typical_p 1 (the block-uniform skip); at 0.9 with top-k 50 in every row (the one-wave form);
    at 0.9 with top-k V in every row (the block-wide form: a second mass select), beside the processed sampler at top-k V.  200
    back-to-back launches between two synchronisations, alternated, median (min .. max) of GEN_ROUNDS repeats (default 3).  (b) the
    steady 16-row server step of GEN_SERVE's setting: row_processors on (the yardstick), row_typical on at identity (typical_p 1
    everywhere), on with a mixed load (typical_p 0.2 .. 1.0, per codebook in a quarter of the rows, over the processors leg's
    mixed penalties); each leg a fresh server, alternated GEN_ROUNDS times (default 3), per leg the median of 20 steps."""
    dev = "cuda:0"
    n = 4
    V, ld = 2051, 2112
    g = torch.Generator(device=dev).manual_seed(0)
    lg = torch.randn(16, ld, device=dev, generator=g) * 2
    q = torch.empty(16, V, device=dev).exponential_(1, generator=g)
    out = torch.empty(16, dtype=torch.int32, device=dev)

    def f32(v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)
    k50, kV, t, p, m = i32([50] * 16), i32([V] * 16), f32([0.9] * 16), f32([1.0] * 16), f32([0.0] * 16)
    hist = torch.randint(0, V, (16, 64), device=dev, generator=g).to(torch.int32)
    frame, live = i32([200] * 16), i32([1] * 16)
    r, w = f32([1.3] * 16), i32([16] * 16)
    y1, y9 = f32([1.0] * 16), f32([0.9] * 16)

    def typical(k, y):
        return lambda: ops.sample_typical_rows(lg, q, out, k, t, p, m, r, w, hist, frame, live, y, advance=False, V=V)

    def processed(k):
        return lambda: ops.sample_processed_rows(lg, q, out, k, t, p, m, r, w, hist, frame, live, advance=False, V=V)
    legs = {"processed, top-k 50 (csm_sample_processed_rows)": processed(k50),
            "typical at identity (typical_p 1), top-k 50": typical(k50, y1),
            "typical 0.9, top-k 50 (one-wave)": typical(k50, y9),
            "processed, top-k V": processed(kV),
            "typical 0.9, top-k V (block-wide)": typical(kV, y9)}
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    res = {name: [] for name in legs}
    for f in legs.values():
        _timed(f, 20)
    for _ in range(rounds):
        for name, f in legs.items():
            res[name].append(_timed(f, 200))
    for name, v in res.items():
        v.sort()
        print(f"GEN_SERVE_SAMPLING=typical (a) sampler, 16 rows, V={V}: {name}: median {v[len(v) // 2] * 1e6:.2f} us per launch "
              f"(min {v[0] * 1e6:.2f}, max {v[-1] * 1e6:.2f}; {rounds} x 200 back-to-back launches)", flush=True)
    if os.environ.get("GEN_SERVE_PARTS", "ab") == "a":
        return
    # ---- (b) the server step
    codec = make_codec(dev)
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    K = model.args.audio_num_codebooks
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    pens = [(1.0, 64), (1.3, 16), (2.0, 64), (1.1, 0), (1.5, 33), (1.3, 64), (1.2, 8), (1.7, 64)]
    typs = [0.9, 0.2, 1.0, 0.5, 0.95, 0.7, 0.3, 0.99]
    mixed = []
    for b in range(16):
        kw = dict(top_p=0.9, min_p=0.05, repetition_penalty=pens[b % 8][0], repetition_window=pens[b % 8][1], typical_p=typs[b % 8])
        if b % 4 == 1:
            kw.update(typical_p=[typs[b % 8]] + [0.8] * (K - 1), topk=[50] + [2051] * (K - 1))     # (the block-wide form too)
        mixed.append(kw)
    base = "row_processors (the yardstick)"
    modes = {base: (dict(row_processors=True), [{}] * 16), "row_typical, identity": (dict(row_typical=True), [{}] * 16),
             "row_typical, mixed": (dict(row_typical=True), mixed)}
    meds = {name: [] for name in modes}
    for _ in range(rounds):
        for name, (flags, kws) in modes.items():
            srv = gen.serve(slots=16, chunk_frames=n, row_sampling=True, **flags)
            for i in range(16):
                srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400, **kws[i])
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            meds[name].append(steps[len(steps) // 2])
    for name, v in meds.items():
        print(f"GEN_SERVE_SAMPLING=typical (b) server step, 16 rows x {n} frames, {name}: medians of 20 steps "
              f"{[round(x * 1e3, 2) for x in v]} ms -> median {sorted(v)[len(v) // 2] * 1e3:.2f} ms, spread of the repeats "
              f"{(max(v) - min(v)) * 1e3:.2f} ms", flush=True)
    off = sorted(meds[base])[rounds // 2]
    for name in ("row_typical, identity", "row_typical, mixed"):
        on = sorted(meds[name])[rounds // 2]
        print(f"GEN_SERVE_SAMPLING=typical (b) {name} - row_processors: {(on - off) * 1e3:+.2f} ms per step = "
              f"{(on - off) * 1e6 / n:+.1f} us per frame = {(on - off) * 1e6 / n / K:+.2f} us per draw ({K} launches a frame; "
              f"row_processors' own repeats span {(max(meds[base]) - min(meds[base])) * 1e3:.2f} ms)", flush=True)


def serve_conv_main():
    """GEN_SERVE_CONV=1: conversations on the running batch (BatchServer.conversation) on CSM-1B random init - 16 slots,
    chunk_frames 4, 16 conversations of 6 turns: odd turns spoken (GEN_FRAMES frames, default 24), even turns 5 s of the other
    party's audio (Mimi-encoded at ``add``, outside the timed steps).  All 16 turns of a round are admitted at one chunk boundary.
    (a) host time from the step() that admits turn 1 / 3 / 5 of all 16 conversations to their first chunk on the host, next to
        the same turns submitted statelessly (``submit`` with the accumulated segments as context, Mimi-encoded at submit) on the
        same server in the same job; GEN_ROUNDS dialogues (default 3) after one warm-up dialogue, min / median / max;
    (b) one append_rows over J = 1, 2, 4, 8, 16 segments of turn 5's feed length against J one-row append_rows calls;
    (c) park_row / resume_row at the history lengths reached after turns 1, 3, 5;
    (d) aggregate frames/s of the whole dialogue (all steps and the adds' Mimi encodes)."""
    dev = "cuda:0"
    NC, n = 16, 4
    frames = int(os.environ.get("GEN_FRAMES", 24))
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    ms = 80 * frames
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    srv = gen.serve(slots=NC, chunk_frames=n)
    g = torch.Generator(device=dev).manual_seed(1)
    heard = [torch.randn(5 * 24000, device=dev, generator=g) * 0.1 for _ in range(3)]
    say = lambda t: (t % 4 // 2, f"turn {t + 1}: the quick brown fox jumps over the lazy dog")          # noqa: E731
    med = lambda xs: sorted(xs)[len(xs) // 2]                                                           # noqa: E731
    fmt = lambda xs: f"{med(xs):7.1f} [{min(xs):6.1f}..{max(xs):6.1f}]"                                 # noqa: E731

    def admit_and_finish(reqs):
        """The step that admits ``reqs`` timed to their first chunk on the host, then the rest of the turn."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = srv.step()
        torch.cat([a for _, a, _ in out]).cpu()
        first = time.perf_counter() - t0
        assert srv.last_join_rows == len(reqs) and len(out) == len(reqs)
        while srv.active:
            srv.step()
        assert all(r.done and r.codes().shape[1] == frames for r in reqs), "a random-init model should not emit EOS"
        return first * 1e3

    def dialogue():
        convs = [srv.conversation(seed=i) for i in range(NC)]
        segs = [[] for _ in range(NC)]
        first, cached, fed, feed = {}, {}, {}, None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(6):
            if t % 2 == 0:
                spk, text = say(t)
                reqs = [c.say(text, spk, max_audio_length_ms=ms) for c in convs]
                feed = [(r._tokens, r._mask) for r in reqs]
                fed[t] = feed[0][0].shape[0]
                first[t] = admit_and_finish(reqs)
                cached[t] = convs[0].cached
                for i, r in enumerate(reqs):
                    segs[i].append(Segment(spk, text, r.audio()))
            else:
                for i, c in enumerate(convs):
                    seg = Segment(1 - (t - 1) % 4 // 2, f"turn {t + 1}: and what did the dog do", heard[t // 2])
                    c.add(seg)
                    segs[i].append(seg)
        torch.cuda.synchronize()
        return dict(first=first, cached=cached, fed=fed, feed=feed, total=time.perf_counter() - t0, convs=convs, segs=segs)

    def stateless(segs, t):
        spk, text = say(t)
        reqs = [srv.submit(text, spk, segs[i][:t], seed=i, max_audio_length_ms=ms) for i in range(NC)]
        return admit_and_finish(reqs), reqs[0]._tokens.shape[0]

    d = dialogue()                                                    # warm-up: allocator, graph capture, every shape
    for t in (0, 2, 4):
        stateless(d["segs"], t)
    runs, less, plen = [], {0: [], 2: [], 4: []}, {}
    for _ in range(rounds):
        for c in d["convs"]:
            c.close()
        d = dialogue()
        runs.append(d)
        for t in (0, 2, 4):
            f, plen[t] = stateless(d["segs"], t)
            less[t].append(f)
    hist = d["convs"][0].tokens.shape[0]
    print(f"GEN_SERVE_CONV: {NC} conversations x 6 turns on {NC} slots, chunk_frames {n}, {frames} frames per spoken turn, 5 s heard "
          f"per even turn; {rounds} dialogues after one warm-up; history at the end {hist} positions.  ms as median [min..max]")
    for t in (0, 2, 4):
        fc = [r["first"][t] for r in runs]
        print(f"(a) turn {t + 1}: step that admits all {NC} turns -> first chunk: conversation {fmt(fc)} (fed {d['fed'][t]} "
              f"positions; {d['cached'][t]} cached after the turn) | stateless submit {fmt(less[t])} (prompt {plen[t]} positions)")
    spread = max(max(r["first"][t] for r in runs) - min(r["first"][t] for r in runs) for t in (2, 4))
    print(f"(a) run-to-run spread of the conversation figure (max - min over the {rounds} dialogues, worst of turns 3 and 5): {spread:.1f} ms; "
          f"turn 5 - turn 3 (medians): {med([r['first'][4] for r in runs]) - med([r['first'][2] for r in runs]):+.1f} ms")
    tot = [NC * 3 * frames / r["total"] for r in runs]
    print(f"(d) aggregate over the whole dialogue ({NC * 3 * frames} frames kept; steps + adds' Mimi encodes): {med(tot):.0f} frames/s "
          f"[{min(tot):.0f}..{max(tot):.0f}]")
    # ---- (c) park / resume
    st = srv._state
    with torch.inference_mode():
        for c in d["convs"]:
            c.close()
        d = dialogue()
        parked = [c._parked for c in d["convs"]]
        for t in (0, 2, 4):
            L = d["cached"][t]
            part = parked[0][:, :, :, :L].contiguous()
            st.resume_row(0, part)
            tp = [_timed(lambda: st.park_row(0, L), 20) * 1e3 for _ in range(rounds)]
            tr = [_timed(lambda: st.resume_row(0, part), 20) * 1e3 for _ in range(rounds)]
            print(f"(c) history {L:4d} positions ({part.numel() * 2 / 1e6:5.1f} MB): park_row {min(tp):.3f} ms, resume_row {min(tr):.3f} ms "
                  f"(best of {rounds} x 20)")
        # ---- (b) one append_rows over J segments against J one-row calls, at the end-of-dialogue history
        base = []
        for b in range(NC):
            st.resume_row(b, parked[b])
            base.append(st.row_pos[b])
        feed = d["feed"]

        def reset(J):
            for b in range(J):
                st.row_pos[b] = base[b]

        for J in (1, 2, 4, 8, 16):
            def together():
                reset(J)
                st.append_rows(list(range(J)), [feed[b][0] for b in range(J)], [feed[b][1] for b in range(J)])

            def one_by_one():
                reset(J)
                for b in range(J):
                    st.append_rows([b], [feed[b][0]], [feed[b][1]])

            for f in (together, one_by_one):
                _timed(f, 2)
            best = {"rows": 1e9, "single": 1e9}
            for _ in range(rounds):
                best["rows"] = min(best["rows"], _timed(together, 5))
                best["single"] = min(best["single"], _timed(one_by_one, 5))
            print(f"(b) append_rows, {feed[0][0].shape[0]} positions per segment after {base[0] + 1} cached, J={J:2d}: one call "
                  f"{best['rows'] * 1e3:7.2f} ms, {J} one-row calls {best['single'] * 1e3:7.2f} ms -> {best['single'] / best['rows']:.2f}x", flush=True)


def hear_main():
    """GEN_HEAR=1: the time from the last sample of a 5 s heard turn to the first audio chunk of the reply, on CSM-1B random init,
    with the heard turn entered (a) by ``add(Segment)`` after its last sample - tokenise + whole-segment Mimi encode on the path -
    and (b) by ``hear`` fed in 4-frame pieces while the turn is spoken (untimed: that happens during the turn), so that the last
    piece (2.5 frames), ``end`` (its flush) and the reply are what is left.  Served: GEN_SERVE_CONV's setting (16 slots,
    chunk_frames 4, all 16 conversations' heard turns end at once, reply = ``say`` + the step that admits all 16 to the chunk on
    the host).  B = 1: GEN_CONVERSATION's setting (``generate_stream``, chunk_frames 2).  Each dialogue: a spoken turn of
    GEN_FRAMES frames (default 24), the heard turn, the reply.  GEN_ROUNDS rounds (default 3) of (a) and (b) alternated after one
    warm-up round of each; ms as median [min..max].  Also the per-piece ``feed`` time during the turn."""
    dev = "cuda:0"
    NC, n = 16, 4
    frames = int(os.environ.get("GEN_FRAMES", 24))
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    ms = 80 * frames
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    g = torch.Generator(device=dev).manual_seed(1)
    heard = torch.randn(5 * 24000, device=dev, generator=g) * 0.1
    piece = 4 * 1920
    cut = heard.numel() // piece * piece                              # 60 frames arrive during the turn, 2.5 at its end
    line, heard_text, reply = "turn 1: the quick brown fox jumps over the lazy dog", "turn 2: and what did the dog do", "turn 3: it slept"
    med = lambda xs: sorted(xs)[len(xs) // 2]                                                           # noqa: E731
    fmt = lambda xs: f"{med(xs):7.1f} [{min(xs):6.1f}..{max(xs):6.1f}]"                                 # noqa: E731
    feeds = []

    def during(turns):
        """What happens while the turn is spoken: every whole 4-frame piece is fed (timed per piece, all conversations)."""
        for lo in range(0, cut, piece):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in turns:
                t.feed(heard[lo:lo + piece])
            torch.cuda.synchronize()
            feeds.append((time.perf_counter() - t0) * 1e3 / len(turns))

    def served(form):
        srv = gen.serve(slots=NC, chunk_frames=n)
        convs = [srv.conversation(seed=i) for i in range(NC)]
        for c in convs:
            c.say(line, 0, max_audio_length_ms=ms)
        for _ in srv.run():
            pass
        turns = [c.hear(1) for c in convs] if form == "hear" else None
        if turns:
            during(turns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()                                      # the turn's last sample
        for i, c in enumerate(convs):
            if turns:
                turns[i].feed(heard[cut:])
                turns[i].end(heard_text)
            else:
                c.add(Segment(1, heard_text, heard))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        snap = convs[0].tokens                                         # (the history with the heard turn; later pushes make new tensors)
        for c in convs:
            c.say(reply, 0, max_audio_length_ms=ms)
        out = srv.step()
        torch.cat([a for _, a, _ in out]).cpu()
        t2 = time.perf_counter()
        assert srv.last_join_rows == NC
        for _ in srv.run():
            pass
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, snap

    def single(form):
        conv = gen.conversation()
        for _ in conv.generate_stream(line, 0, max_audio_length_ms=ms, chunk_frames=2):
            pass
        turn = conv.hear(1) if form == "hear" else None
        if turn:
            during([turn])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if turn:
            turn.feed(heard[cut:])
            turn.end(heard_text)
        else:
            conv.add(Segment(1, heard_text, heard))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        snap = conv.tokens
        s = conv.generate_stream(reply, 0, max_audio_length_ms=ms, chunk_frames=2)
        next(s).cpu()
        t2 = time.perf_counter()
        for _ in s:
            pass
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, snap

    print(f"GEN_HEAR: 5 s heard turn ({heard.numel() // 1920} whole frames + {heard.numel() % 1920} samples), {frames} frames per spoken "
          f"turn, {rounds} alternated rounds after one warm-up of each form; ms as median [min..max]")
    for name, fn in (("served, 16 conversations at once, chunk_frames 4", served), ("B = 1 generate_stream, chunk_frames 2", single)):
        res = {"add": [], "hear": []}
        toks = {}
        for r in range(rounds + 1):
            for form in ("add", "hear"):
                torch.manual_seed(7)
                enter, first, toks[form] = fn(form)
                if r:
                    res[form].append((enter, first))
        # (whole frames equal bit for bit; the last, partial frame is the documented deviation: layers padded against waveform padded)
        same = bool((toks["add"][:-2] == toks["hear"][:-2]).all()) if toks["add"].shape == toks["hear"].shape else False
        for form, what in (("add", "(a) add(Segment) + reply"), ("hear", "(b) last piece + end + reply")):
            print(f"{name}: {what}: last sample -> first chunk on the host {fmt([f for _, f in res[form]])} ms, of which entering the "
                  f"turn {fmt([e for e, _ in res[form]])} ms", flush=True)
        print(f"{name}: (b) - (a) = {med([f for _, f in res['hear']]) - med([f for _, f in res['add']]):+.1f} ms (medians); histories "
              f"{'equal up to the last partial frame' if same else 'DIFFER'}")
    print(f"feed of one 4-frame piece during the turn (one encoder step, per conversation): {fmt(feeds)} ms; a 5 s turn makes "
          f"{cut // piece} of them, one per 320 ms of audio")


def hear_rows_main():
    """GEN_HEAR=1 (after hear_main) or GEN_HEAR=rows (alone): 16 conversations on the 16-slot server (CSM-1B random init,
    chunk_frames 4) each hear a 5 s turn in 4-frame pieces, with (a) ``hear_slots=0`` - one MimiEncodeStream per conversation, one
    encoder step per ``feed`` - and (b) ``hear_slots=16`` - ``feed`` buffers, one ``hear_step`` per chunk encodes all 16.
    Reported: the hearing cost of one chunk (16 feeds, plus ``hear_step`` for (b); nobody speaks meanwhile), and the time from
    the last sample (a 2.5-frame piece) to the first chunk of the 16 replies on the host when all 16 turns end together: (a) 16
    ``end`` calls, (b1) 16 ``end`` calls on the rows encoder (16 one-row drains), (b2) one ``end_heard``.  GEN_ROUNDS rounds
    (default 3) alternated after one warm-up round of each form; ms as median [min..max]."""
    dev = "cuda:0"
    NC, n = 16, 4
    frames = int(os.environ.get("GEN_FRAMES", 24))
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    ms = 80 * frames
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    g = torch.Generator(device=dev).manual_seed(1)
    heard = [torch.randn(5 * 24000, device=dev, generator=g) * 0.1 for _ in range(NC)]
    piece = n * 1920
    cut = heard[0].numel() // piece * piece
    line, heard_text, reply = "turn 1: the quick brown fox jumps over the lazy dog", "turn 2: and what did the dog do", "turn 3: it slept"
    med = lambda xs: sorted(xs)[len(xs) // 2]                                                           # noqa: E731
    fmt = lambda xs: f"{med(xs):7.1f} [{min(xs):6.1f}..{max(xs):6.1f}]"                                 # noqa: E731

    def dialogue(form):
        hs = 0 if form == "a" else NC
        srv = gen.serve(slots=NC, chunk_frames=n, hear_slots=hs)
        convs = [srv.conversation(seed=i) for i in range(NC)]
        for c in convs:
            c.say(line, 0, max_audio_length_ms=ms)
        for _ in srv.run():
            pass
        turns = [c.hear(1) for c in convs]
        chunks = []
        for lo in range(0, cut, piece):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, t in enumerate(turns):
                t.feed(heard[i][lo:lo + piece])
            srv.hear_step()
            torch.cuda.synchronize()
            chunks.append((time.perf_counter() - t0) * 1e3)
        assert all(t.frames == cut // 1920 for t in turns)
        torch.cuda.synchronize()
        t0 = time.perf_counter()                                      # the turns' last sample
        for i, t in enumerate(turns):
            t.feed(heard[i][cut:])
        if form == "b2":
            srv.end_heard([(t, heard_text) for t in turns])
        else:
            for t in turns:
                t.end(heard_text)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        snap = [c.tokens for c in convs]
        for c in convs:
            c.say(reply, 0, max_audio_length_ms=ms)
        out = srv.step()
        torch.cat([a for _, a, _ in out]).cpu()
        t2 = time.perf_counter()
        assert srv.last_join_rows == NC
        for _ in srv.run():
            pass
        return chunks, (t1 - t0) * 1e3, (t2 - t0) * 1e3, snap

    forms = (("a", "(a) hear_slots=0, 16 end calls"), ("b1", "(b1) hear_slots=16, 16 end calls"), ("b2", "(b2) hear_slots=16, one end_heard"))
    res = {f: {"chunk": [], "enter": [], "first": []} for f, _ in forms}
    toks = {}
    print(f"GEN_HEAR rows: {NC} conversations hear 5 s ({cut // piece} pieces of {n} frames + 2.5 frames at the end) on {NC} slots, "
          f"chunk_frames {n}, {rounds} alternated rounds after one warm-up of each form; ms as median [min..max]")
    for r in range(rounds + 1):
        for f, _ in forms:
            torch.manual_seed(7)
            chunks, enter, first, toks[f] = dialogue(f)
            if r:
                res[f]["chunk"] += chunks[1:]                         # (the first piece of a turn warms the encoder's buffers)
                res[f]["enter"].append(enter)
                res[f]["first"].append(first)
    same = all(torch.equal(x, y) for f in ("b1", "b2") for x, y in zip(toks["a"], toks[f]))
    for f, what in forms:
        print(f"{what}: hearing cost per chunk ({NC} listeners) {fmt(res[f]['chunk'])} ms; last sample -> first chunk on the host "
              f"{fmt(res[f]['first'])} ms, of which entering the 16 turns {fmt(res[f]['enter'])} ms", flush=True)
    a, b = med(res["a"]["chunk"]), med(res["b2"]["chunk"])
    print(f"per chunk: {a:.1f} -> {b:.1f} ms ({a / b:.2f}x); last sample -> first chunk: {med(res['a']['first']):.1f} -> "
          f"{med(res['b2']['first']):.1f} ms with end_heard ({med(res['b1']['first']):.1f} ms with 16 end calls on the rows encoder); "
          f"histories {'equal' if same else 'DIFFER'}")


def overflow_main():
    """GEN_OVERFLOW=1: CSM-1B random init.  Every conversation: a 5 s voice prompt (kept: keep_turns=1) and six 5 s turns of the
    other party, spoken turn 1 (GEN_FRAMES frames, default 24; prefills everything), a 5 s turn, spoken turn 2 (in the limit: the
    baseline, fed by append), a 5 s turn, spoken turn 3 with max_audio_length_ms = 90 000 - the length rule (923 positions, 920
    served) drops the two oldest turns after the voice prompt.  The 5 s turns are tokenised and Mimi-encoded once, outside the
    timed part.  GEN_ROUNDS rounds (default 3) of drop_oldest and shift alternated after one warm-up round of each; ms as median
    [min..max]; a first chunk counts as arrived when its samples are on the host.
    (a) B = 1 (Generator.conversation, generate_stream, chunk_frames 2): the call -> first chunk of turns 2 and 3;
    (b) GEN_SERVE_CONV's setting (16 slots, chunk_frames 4): the step that admits all 16 turns -> first chunk, turns 2 and 3;
    (c) csm_kv_shift alone at len 900 / drop 200 / keep 100 in CSM-1B geometry, and shift_row (park + shift + resume)."""
    dev = "cuda:0"
    NC, n = 16, 4
    frames = int(os.environ.get("GEN_FRAMES", 24))
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    ms, long_ms = 80 * frames, 90_000
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    g = torch.Generator(device=dev).manual_seed(1)
    with torch.inference_mode():
        heard = [gen._tokenize_segment(Segment(t % 2, f"turn {t}: and what did the dog do", torch.randn(5 * 24000, device=dev, generator=g) * 0.1))
                 for t in range(9)]
    text = "the quick brown fox jumps over the lazy dog"
    med = lambda xs: sorted(xs)[len(xs) // 2]                                                           # noqa: E731
    fmt = lambda xs: f"{med(xs):7.1f} [{min(xs):6.1f}..{max(xs):6.1f}]"                                 # noqa: E731
    MODES = ("drop_oldest", "shift")

    def push(conv, segs):
        for t, m in segs:
            conv._push(t.long(), m.bool())                           # (what add() does after its tokenise + Mimi encode)

    def first_chunk(stream, whole):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = stream()
        next(it).cpu()
        first = time.perf_counter() - t0
        if whole:
            for _ in it:
                pass
        else:
            it.close()                                               # abandoned after the first chunk: the turn is settled
        return first * 1e3

    def solo(mode):
        torch.manual_seed(0)
        conv = gen.conversation(on_overflow=mode, keep_turns=1)
        push(conv, heard[:7])
        say = lambda ms_, whole: first_chunk(lambda: conv.generate_stream(text, 0, max_audio_length_ms=ms_, chunk_frames=2), whole)  # noqa: E731
        say(ms, True)
        push(conv, heard[7:8])
        fed2 = conv.tokens.shape[0] - conv.cached
        t2 = say(ms, True)
        push(conv, heard[8:9])
        before, cached = conv.tokens.shape[0], conv.cached
        t3 = say(long_ms, False)
        return dict(t2=t2, t3=t3, fed2=fed2, before=before, cached=cached, after=conv.tokens.shape[0], turns=len(conv._turns))

    def served(mode):
        srv = gen.serve(slots=NC, chunk_frames=n)

        def admit(reqs, finish):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = srv.step()
            torch.cat([a for _, a, _ in out]).cpu()
            first = time.perf_counter() - t0
            assert srv.last_join_rows == NC and len(out) == NC
            while finish and srv.active:
                srv.step()
            return first * 1e3
        convs = [srv.conversation(seed=i, on_overflow=mode, keep_turns=1) for i in range(NC)]
        for c in convs:
            push(c, heard[:7])
        admit([c.say(text, 0, max_audio_length_ms=ms) for c in convs], True)
        for c in convs:
            push(c, heard[7:8])
        t2 = admit([c.say(text, 0, max_audio_length_ms=ms) for c in convs], True)
        for c in convs:
            push(c, heard[8:9])
        before, cached = convs[0].tokens.shape[0], convs[0].cached
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reqs = [c.say(text, 0, max_audio_length_ms=long_ms) for c in convs]       # _fit runs here: 16 shift_parked under "shift"
        torch.cuda.synchronize()
        t_say = (time.perf_counter() - t0) * 1e3
        fed3 = reqs[0]._tokens.shape[0]
        t3 = admit(reqs, False)                                                    # (the 90 s turns are not played out)
        return dict(t2=t2, t3=t3, say=t_say, fed3=fed3, before=before, cached=cached, kept=convs[0].cached)

    for name, leg in (("(a) B = 1, chunk_frames 2", solo), ("(b) 16 conversations on 16 slots, chunk_frames 4", served)):
        for mode in MODES:
            leg(mode)                                                # warm-up round of each: allocator, graph capture, shapes
        res = {m: [] for m in MODES}
        for _ in range(rounds):
            for mode in MODES:
                res[mode].append(leg(mode))
        r = res["shift"][0]
        print(f"GEN_OVERFLOW {name}: history {r['before']} positions ({r['cached']} cached) before turn 3, {frames} frames per in-limit turn; "
              f"{rounds} alternated rounds after one warm-up of each; ms as median [min..max]")
        for mode in MODES:
            v = res[mode]
            line = f"  {mode:11s}: in-limit turn 2 -> first chunk {fmt([x['t2'] for x in v])} | overflowing turn 3 -> first chunk {fmt([x['t3'] for x in v])}"
            if "say" in v[0]:
                line += f" (fed {v[0]['fed3']} positions per row, history {v[0]['kept']} positions once fed; the 16 say() calls before it {fmt([x['say'] for x in v])})"
            else:
                line += f" (turn 2 fed {v[0]['fed2']} + text; history {v[0]['after']} positions in {v[0]['turns']} turns after turn 3's first chunk)"
            print(line, flush=True)
    # ---- (c) the kernel alone, CSM-1B geometry
    with torch.inference_mode():
        L, keep, drop = 900, 100, 200
        c = model.bb
        parked = torch.randn(c.num_layers, 2, c.num_kv_heads, L, c.head_dim, device=dev).to(torch.bfloat16)
        table = model.rope_table("backbone")
        _timed(lambda: ops.kv_shift(parked, table, keep, drop), 20)
        tk = sorted(_timed(lambda: ops.kv_shift(parked, table, keep, drop), 100) * 1e3 for _ in range(max(rounds, 5)))
        moved = parked.numel() * 2 * (2 * L - drop) / L
        print(f"GEN_OVERFLOW (c) csm_kv_shift len {L} keep {keep} drop {drop}, {c.num_layers} layers x {c.num_kv_heads} kv heads x {c.head_dim}: "
              f"median {med(tk) * 1e3:.1f} us [{tk[0] * 1e3:.1f}..{tk[-1] * 1e3:.1f}] per call (output allocation included), "
              f"{moved / 1e6:.1f} MB read + written -> {moved / med(tk) / 1e6:.0f} GB/s")
        from csm.engine import DecodeState
        st = DecodeState(model.engine, 1)
        st.resume_row(0, parked)

        def row():
            st.resume_row(0, parked)
            st.shift_row(0, keep, drop)
        _timed(row, 5)
        both = sorted(_timed(row, 20) * 1e3 for _ in range(max(rounds, 5)))
        res_only = sorted(_timed(lambda: st.resume_row(0, parked), 20) * 1e3 for _ in range(max(rounds, 5)))
        print(f"GEN_OVERFLOW (c) shift_row (park_row + csm_kv_shift + resume_row) at the same sizes: median {med(both) - med(res_only):.3f} ms "
              f"(resume_row of {L} positions alone {med(res_only):.3f} ms, taken off)")


def resample_main():
    """GEN_RESAMPLE=1: the device resampler on the serving paths, CSM-1B random init, 16 slots, chunk_frames 4.  (a) the steady
    16-row server step of GEN_SERVE's setting with ``output_sample_rate=48000`` (one rows resampler launch per step) against the
    same step without it; (b) the 16-listener ``hear_step`` (16 feeds of one 320 ms chunk + the step; nobody speaks) with
    ``hear(sample_rate=16000)`` against 24 kHz input.  Each leg is a fresh server, the two alternated GEN_ROUNDS times (default 3),
    per repeat the median of 20 steps / 12 chunks; the difference is reported next to the base's own repeat-to-repeat spread."""
    dev = "cuda:0"
    n, NC = 4, 16
    rounds = int(os.environ.get("GEN_ROUNDS", 3))
    model = Model(csm_1b_args(), device=dev, seed=0)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=make_codec(dev))
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]
    text = "the quick brown fox jumps over the lazy dog"
    med = lambda xs: sorted(xs)[len(xs) // 2]                                                           # noqa: E731

    def report(what, unit, res, base, other):
        for name, v in res.items():
            print(f"GEN_RESAMPLE {what}, {name}: medians {[round(x * 1e3, 3) for x in v]} ms -> median {med(v) * 1e3:.3f} ms, spread of "
                  f"the repeats {(max(v) - min(v)) * 1e3:.3f} ms", flush=True)
        d = med(res[other]) - med(res[base])
        print(f"GEN_RESAMPLE {what}: {other} - {base}: {d * 1e3:+.3f} ms per {unit} ({base}'s own repeats span "
              f"{(max(res[base]) - min(res[base])) * 1e3:.3f} ms)", flush=True)

    # ---- (a) speaking: the server step
    res = {"24 kHz out (off)": [], "48 kHz out": []}
    for _ in range(rounds):
        for name, rate in (("24 kHz out (off)", None), ("48 kHz out", 48000)):
            srv = gen.serve(slots=NC, chunk_frames=n, output_sample_rate=rate)
            reqs = [srv.submit(f"utterance number {i}: {text}", i, ctx, seed=i, max_audio_length_ms=80 * 400) for i in range(NC)]
            _timed(srv.step, 1)                                              # 16 prefills + the first chunk
            _timed(srv.step, 2)                                              # eager warm-up frame, graph capture
            steps = sorted(_timed(srv.step, 1) for _ in range(20))
            res[name].append(steps[len(steps) // 2])
            assert reqs[0].sample_rate == (rate or 24000) and reqs[0].chunks[-1].numel() in (n * 1920, 2 * n * 1920)
    report(f"(a) server step, {NC} rows x {n} frames", "step", res, "24 kHz out (off)", "48 kHz out")
    # ---- (b) hearing: 16 listeners, one 320 ms chunk each per hear_step
    res = {"24 kHz in (off)": [], "16 kHz in": []}
    g = torch.Generator(device=dev).manual_seed(1)
    for _ in range(rounds):
        for name, rate in (("24 kHz in (off)", None), ("16 kHz in", 16000)):
            piece = n * 1920 * (rate or 24000) // 24000
            heard = [torch.randn(14 * piece, device=dev, generator=g) * 0.1 for _ in range(NC)]
            srv = gen.serve(slots=NC, chunk_frames=n, hear_slots=NC)
            turns = [srv.conversation().hear(1, sample_rate=rate) for _ in range(NC)]
            chunks = []
            for c in range(14):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i, t in enumerate(turns):
                    t.feed(heard[i][c * piece:(c + 1) * piece])
                srv.hear_step()
                torch.cuda.synchronize()
                chunks.append(time.perf_counter() - t0)
            assert all(t.frames >= 13 * n for t in turns)
            res[name].append(med(chunks[2:]))                                # (the first pieces warm the encoder's buffers)
            for t in turns:
                t.cancel()
    report(f"(b) hear_step, {NC} listeners x {n} frames", "chunk", res, "24 kHz in (off)", "16 kHz in")


def main():
    if os.environ.get("GEN_SERVE_STREAMS") == "1":
        return serve_streams_main()
    if os.environ.get("GEN_VOICE") == "1":
        return voice_main()
    if os.environ.get("GEN_RESAMPLE") == "1":
        return resample_main()
    if os.environ.get("GEN_OVERFLOW") == "1":
        return overflow_main()
    if os.environ.get("GEN_HEAR") == "rows":
        return hear_rows_main()
    if os.environ.get("GEN_HEAR") == "1":
        hear_main()
        return hear_rows_main()
    if os.environ.get("GEN_SERVE_STATS") == "1":
        return serve_stats_main()
    if os.environ.get("GEN_SERVE_SAMPLING") == "1":
        return serve_sampling_main()
    if os.environ.get("GEN_SERVE_SAMPLING") == "filters":
        return serve_filters_main()
    if os.environ.get("GEN_SERVE_SAMPLING") == "processors":
        return serve_processors_main()
    if os.environ.get("GEN_SERVE_SAMPLING") == "typical":
        return serve_typical_main()
    if os.environ.get("GEN_SERVE_CONV") == "1":
        return serve_conv_main()
    if os.environ.get("GEN_SERVE") == "1":
        return serve_main()
    if os.environ.get("GEN_CONVERSATION") == "1":
        return conversation_main()
    if os.environ.get("GEN_BATCH_SWEEP") == "1":
        return sweep_main()
    if os.environ.get("GEN_FP8") == "1" and os.environ.get("GEN_LORA_BANK"):
        return fp8_bank_main(os.environ["GEN_LORA_BANK"])
    if os.environ.get("GEN_FP8") == "1":
        return fp8_main()
    if os.environ.get("GEN_LORA_BANK"):
        return lora_bank_main(os.environ["GEN_LORA_BANK"])
    if os.environ.get("GEN_LORA"):
        return lora_main(os.environ["GEN_LORA"])
    if os.environ.get("GEN_STREAM") == "1":
        return stream_main()
    dev = "cuda:0"
    model = Model(csm_1b_args(), device=dev, seed=0)
    codec = make_codec(dev)
    gen = Generator(model, text_tokenizer=ByteTokenizer(), audio_tokenizer=codec)
    ctx = [Segment(0, "hello there", torch.randn(5 * 24000, device=dev) * 0.1)]        # 5 s of context audio to tokenise
    frames = int(os.environ.get("GEN_FRAMES", 125))
    for n in (5, frames):
        torch.cuda.synchronize()
        t0 = time.time()
        audio = gen.generate("the quick brown fox jumps over the lazy dog", 1, ctx, max_audio_length_ms=80 * n)
        torch.cuda.synchronize()
        dt = time.time() - t0
        print(f"{n} frames requested: {audio.numel() / 24000:.2f} s of audio in {dt:.2f} s -> {audio.numel() / 1920 / dt:.1f} frames/s "
              f"({audio.numel() / 24000 / dt:.2f}x real time)")
    nb = int(os.environ.get("GEN_BATCH", 4))
    if nb > 1:
        texts = [f"utterance number {i}: the quick brown fox jumps over the lazy dog" for i in range(nb)]
        ctxs = [ctx if i % 2 == 0 else [] for i in range(nb)]
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.time()
            outs = gen.generate_batch(texts, list(range(nb)), ctxs, max_audio_length_ms=80 * frames)
            torch.cuda.synchronize()
            dt = time.time() - t0
        tot = sum(o.numel() for o in outs)
        print(f"batch of {nb}: {tot / 24000:.2f} s of audio in {dt:.2f} s -> {tot / 1920 / dt:.1f} frames/s aggregate ({tot / 24000 / dt:.2f}x real time)")


if __name__ == "__main__":
    main()
