"""Mimi audio codec on MI355X - the audio tokenizer ``Generator`` uses (reference src/csm/generator.py:67-70,117,209).

The reference obtains Mimi from ``moshi==0.2.2`` (``loaders.get_mimi`` + ``set_num_codebooks(32)``), a third-party package
that is neither vendored nor installed here, and whose weights come from the hub.  This module re-implements the
*architecture* (SEANet causal conv encoder / decoder with ratios 8-6-5-4, two 8-layer causal transformers with layer
scale and a 250-frame window, stride-2 down / up-sampling to 12.5 Hz, split residual VQ with 1 semantic + 31 acoustic
codebooks of 2048 x 256) on hand-written fp32 HIP kernels, taking the weights as a state dict with the key names of the
Hugging Face port (``transformers.MimiModel.state_dict()``; the moshi checkpoint maps onto it 1:1).  It exposes exactly
what ``Generator`` touches: ``encode([1,1,N]) -> [1,K,T]`` int64, ``decode([1,K,T]) -> [1,1,N]``, ``sample_rate``, and
``decode_stream()``: a stateful decoder that turns successive chunks of frames into their audio, bit-identical to ``decode``,
and ``encode_stream()``: its counterpart for the audio that is heard, bit-identical to ``encode`` on whole frames.
``decode_stream_rows()`` / ``encode_stream_rows()`` are the two for up to 16 utterances at once, one launch per op.
"""
import math
from typing import Dict, Optional

import torch

from ..hip import check, lib, ops

F32 = torch.float32


def _s():
    return torch.cuda.current_stream().cuda_stream


def decoder_conv_layers(ratios=(8, 6, 5, 4)):
    """The causal convolutions ``MimiCodec.decode`` runs, in order, as (weight prefix, kind, k, stride, input ELU): kind
    "convt" = transposed conv (the 2x upsample, then one per SEANet ratio), "conv" = stride-1 conv."""
    layers = [("upsample", "convt", 4, 2, False), ("decoder.layers.0", "conv", 7, 1, False)]
    idx = 1
    for r in ratios:
        layers += [(f"decoder.layers.{idx + 1}", "convt", 2 * r, r, True),
                   (f"decoder.layers.{idx + 2}.block.1", "conv", 3, 1, True),
                   (f"decoder.layers.{idx + 2}.block.3", "conv", 1, 1, True)]
        idx += 3
    layers.append((f"decoder.layers.{idx + 1}", "conv", 3, 1, True))
    return layers


def encoder_conv_layers(ratios=(8, 6, 5, 4)):
    """The causal convolutions ``MimiCodec.encode_latent`` runs, in order, as (weight prefix, k, stride, input ELU, replicate):
    the SEANet encoder (per ratio, taken in reverse, a residual block and a stride-r conv), then - after the transformer - the
    stride-2 ``downsample``, the only one whose left padding replicates the edge (replicate True) instead of being zero."""
    layers = [("encoder.layers.0", 7, 1, False, False)]
    idx = 1
    for r in reversed(tuple(ratios)):
        layers += [(f"encoder.layers.{idx}.block.1", 3, 1, True, False),
                   (f"encoder.layers.{idx}.block.3", 1, 1, True, False),
                   (f"encoder.layers.{idx + 2}", 2 * r, r, True, False)]
        idx += 3
    layers += [(f"encoder.layers.{idx + 1}", 3, 1, True, False), ("downsample", 4, 2, False, True)]
    return layers


def history_len(kind: str, k: int, stride: int = 1, dilation: int = 1) -> int:
    """Input columns a streaming layer carries between chunks: k_eff - stride = (k-1)*dil + 1 - stride for a causal conv (its
    left padding; (k-1)*dil at stride 1), ceil(k/stride)-1 for a transposed conv whose overhang is cropped on the right."""
    return (k - 1) * dilation + 1 - stride if kind == "conv" else (k - 1) // stride


def ring_slot(pos: int, ring: int) -> int:
    """Slot of absolute transformer position ``pos`` in a K/V ring of ``ring`` rows (csm_attn_window_stream_f32)."""
    return pos % ring


def _transformer_rows(cd: "MimiCodec", tr: str, kv, x, rows, pos0, n2):
    """``MimiCodec._transformer`` on the stacked rows x [R*n2, hidden] of transformer ``tr``: the row-wise ops (LayerNorm, linear)
    run over all of them, RoPE and the ring attention take row r's own first position ``pos0[r]`` and the K/V rings
    ``kv[layer]`` ([slots, ring, hidden] each) of its slot ``rows[r]``.  Shared by the rows decoder and the rows encoder."""
    T, D = x.shape
    H, w = cd.heads, cd.w
    for i in range(cd.n_layers):
        p = f"{tr}.layers.{i}"
        xn = torch.empty_like(x)
        check(lib.csm_layernorm_f32(x.data_ptr(), w[f"{p}.input_layernorm.weight"].data_ptr(), w[f"{p}.input_layernorm.bias"].data_ptr(),
                                    xn.data_ptr(), T, D, cd.eps, _s()), "csm_layernorm_f32")
        qkv = cd._linear(xn, w[f"{p}.self_attn.qkv"])
        ops.rope_half_rows_f32(qkv, pos0, n2, H, cd.theta)
        o = torch.empty(T, D, dtype=F32, device=cd.dev)
        kc, vc = kv[i]
        ops.attn_window_stream_rows_f32(qkv, kc, vc, o, rows, pos0, n2, H, cd.window)
        x = cd._linear(o, w[f"{p}.self_attn.o_proj.weight"], scale=w[f"{p}.self_attn_layer_scale.scale"], res=x)
        check(lib.csm_layernorm_f32(x.data_ptr(), w[f"{p}.post_attention_layernorm.weight"].data_ptr(),
                                    w[f"{p}.post_attention_layernorm.bias"].data_ptr(), xn.data_ptr(), T, D, cd.eps, _s()),
              "csm_layernorm_f32")
        h1 = cd._linear(xn, w[f"{p}.mlp.fc1.weight"], act=1)
        x = cd._linear(h1, w[f"{p}.mlp.fc2.weight"], scale=w[f"{p}.mlp_layer_scale.scale"], res=x)
    return x


def peel_schedule(pending, max_chunk_frames: int):
    """The launches that encode ``pending`` = {slot: whole frames waiting} with rows kernels that take ONE chunk size per launch:
    a list of (n, [slots]).  While any slot has frames left, every such slot steps by n = the least of min(left,
    max_chunk_frames) over them - so each launch carries every slot that still has work (the fullest rows), and there is one
    launch per distinct pending count plus one per ``max_chunk_frames`` split (the fewest).  Any split gives the same bits."""
    if max_chunk_frames < 1:
        raise ValueError("max_chunk_frames must be >= 1")
    left = {int(s): int(p) for s, p in dict(pending).items() if int(p) > 0}
    out = []
    while left:
        n = min(min(p, max_chunk_frames) for p in left.values())
        out.append((n, sorted(left)))
        left = {s: p - n for s, p in left.items() if p > n}
    return out


class MimiCodec:
    sample_rate = 24000
    frame_rate = 12.5

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", num_codebooks: int = 32, ratios=(8, 6, 5, 4),
                 num_filters: int = 64, hidden: int = 512, heads: int = 8, window: int = 250, n_layers: int = 8,
                 codebook_dim: int = 256, n_semantic: int = 1, rope_theta: float = 10000.0, norm_eps: float = 1e-5):
        self.dev = torch.device(device)
        self.K, self.ratios, self.nf, self.hidden, self.heads = num_codebooks, tuple(ratios), num_filters, hidden, heads
        self.window, self.n_layers, self.cdim, self.n_sem = window, n_layers, codebook_dim, n_semantic
        self.theta, self.eps = rope_theta, norm_eps
        self.w = {k: v.detach().to(self.dev, F32).contiguous() for k, v in state_dict.items() if v.dtype.is_floating_point}
        w = self.w
        for tr in ("encoder_transformer", "decoder_transformer"):          # fuse q|k|v rows once
            for i in range(n_layers):
                p = f"{tr}.layers.{i}.self_attn"
                w[f"{p}.qkv"] = torch.cat([w[f"{p}.q_proj.weight"], w[f"{p}.k_proj.weight"], w[f"{p}.v_proj.weight"]], 0).contiguous()
        self.cb = {}
        for name, n in (("semantic", n_semantic), ("acoustic", num_codebooks - n_semantic)):
            q = f"quantizer.{name}_residual_vector_quantizer"
            books = [w[f"{q}.layers.{i}.codebook.embed_sum"] / w[f"{q}.layers.{i}.codebook.cluster_usage"].clamp(min=1e-5)[:, None]
                     for i in range(n)]
            self.cb[name] = torch.stack(books).contiguous()
            w[f"{q}.in"] = w[f"{q}.input_proj.weight"].squeeze(-1).contiguous()      # [256, 512]
            w[f"{q}.out"] = w[f"{q}.output_proj.weight"].squeeze(-1).contiguous()    # [512, 256]

    def set_num_codebooks(self, n: int):
        self.K = n

    # ------------------------------------------------------------------ kernels
    def _conv(self, x, name, k, stride=1, dil=1, elu=False, res=None, pad_mode=0):
        wt, b = self.w[f"{name}.conv.weight"], self.w.get(f"{name}.conv.bias")
        C_out, cin_g, kk = wt.shape
        assert kk == k
        C_in, T_in = x.shape
        groups = C_in // cin_g
        k_eff = (k - 1) * dil + 1
        pad_total = k_eff - stride
        n_frames = math.ceil((T_in - k_eff + pad_total) / stride + 1) - 1
        extra = n_frames * stride + k_eff - pad_total - T_in
        T_out = (T_in + pad_total + extra - k_eff) // stride + 1
        y = torch.empty(C_out, T_out, dtype=F32, device=self.dev)
        check(lib.csm_conv1d_f32(x.data_ptr(), wt.data_ptr(), b.data_ptr() if b is not None else None,
                                 res.data_ptr() if res is not None else None, y.data_ptr(), C_in, C_out, T_in, T_out, k, stride,
                                 dil, pad_total, pad_mode, groups, int(elu), _s()), "csm_conv1d_f32")
        return y

    def _convt(self, x, name, k, stride, elu=False):
        wt, b = self.w[f"{name}.conv.weight"], self.w.get(f"{name}.conv.bias")
        C_in, cout_g, kk = wt.shape
        assert kk == k and x.shape[0] == C_in
        groups = 1 if cout_g != 1 or C_in == 1 else C_in
        C_out = cout_g * groups
        T_in = x.shape[1]
        T_out = T_in * stride                              # causal: the k - stride overhang is trimmed on the right
        y = torch.empty(C_out, T_out, dtype=F32, device=self.dev)
        check(lib.csm_conv_transpose1d_f32(x.data_ptr(), wt.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(),
                                           C_in, C_out, T_in, T_out, k, stride, 0, groups, int(elu), _s()), "csm_conv_transpose1d_f32")
        return y

    def _resblock(self, x, name):
        h = self._conv(x, f"{name}.block.1", 3, elu=True)
        return self._conv(h, f"{name}.block.3", 1, elu=True, res=x)

    def _linear(self, x, W, scale=None, res=None, act=0):
        T, K = x.shape
        N = W.shape[0]
        y = torch.empty(T, N, dtype=F32, device=self.dev)
        check(lib.csm_linear_f32(x.data_ptr(), W.data_ptr(), scale.data_ptr() if scale is not None else None,
                                 res.data_ptr() if res is not None else None, y.data_ptr(), T, N, K, x.stride(0), act, _s()),
              "csm_linear_f32")
        return y

    def _transpose(self, x):
        R, Cn = x.shape
        y = torch.empty(Cn, R, dtype=F32, device=self.dev)
        check(lib.csm_transpose_f32(x.data_ptr(), y.data_ptr(), R, Cn, _s()), "csm_transpose_f32")
        return y

    def _transformer(self, x, tr, pos0=0, kv=None):
        """x [T, hidden] -> [T, hidden]: pre-LN, rotate-half RoPE, causal window attention, GELU MLP, layer scale.
        Streaming (``kv`` = one (k, v) ring cache pair [ring, hidden] per layer): the T rows sit at positions pos0.. and
        attend to the cached keys before them; each attention launch covers at most ring - window + 1 rows."""
        T, D = x.shape
        H, hd, w = self.heads, D // self.heads, self.w
        for i in range(self.n_layers):
            p = f"{tr}.layers.{i}"
            xn = torch.empty_like(x)
            check(lib.csm_layernorm_f32(x.data_ptr(), w[f"{p}.input_layernorm.weight"].data_ptr(), w[f"{p}.input_layernorm.bias"].data_ptr(),
                                        xn.data_ptr(), T, D, self.eps, _s()), "csm_layernorm_f32")
            qkv = self._linear(xn, w[f"{p}.self_attn.qkv"])
            check(lib.csm_rope_half_f32(qkv.data_ptr(), T, H, hd, self.theta, pos0, _s()), "csm_rope_half_f32")
            o = torch.empty(T, D, dtype=F32, device=self.dev)
            if kv is None:
                check(lib.csm_attn_window_f32(qkv.data_ptr(), o.data_ptr(), T, H, hd, self.window, _s()), "csm_attn_window_f32")
            else:
                kc, vc = kv[i]
                rows = kc.shape[0] - self.window + 1
                for r0 in range(0, T, rows):
                    ops.attn_window_stream_f32(qkv[r0:r0 + rows], kc, vc, o[r0:r0 + rows], pos0 + r0, H, self.window)
            x = self._linear(o, w[f"{p}.self_attn.o_proj.weight"], scale=w[f"{p}.self_attn_layer_scale.scale"], res=x)
            check(lib.csm_layernorm_f32(x.data_ptr(), w[f"{p}.post_attention_layernorm.weight"].data_ptr(),
                                        w[f"{p}.post_attention_layernorm.bias"].data_ptr(), xn.data_ptr(), T, D, self.eps, _s()),
                  "csm_layernorm_f32")
            h1 = self._linear(xn, w[f"{p}.mlp.fc1.weight"], act=1)
            x = self._linear(h1, w[f"{p}.mlp.fc2.weight"], scale=w[f"{p}.mlp_layer_scale.scale"], res=x)
        return x

    # ------------------------------------------------------------------ public protocol (Mimi's)
    @torch.no_grad()
    def encode_latent(self, wav: torch.Tensor) -> torch.Tensor:
        """[1,1,N] waveform -> pre-quantiser latent [T, hidden] at 12.5 Hz."""
        x = wav.reshape(1, -1).to(self.dev, F32).contiguous()
        x = self._conv(x, "encoder.layers.0", 7)
        idx = 1
        for r in reversed(self.ratios):
            x = self._resblock(x, f"encoder.layers.{idx}")
            x = self._conv(x, f"encoder.layers.{idx + 2}", 2 * r, stride=r, elu=True)
            idx += 3
        x = self._conv(x, f"encoder.layers.{idx + 1}", 3, elu=True)                  # [hidden, T25]
        x = self._transformer(self._transpose(x), "encoder_transformer")
        x = self._conv(self._transpose(x), "downsample", 4, stride=2, pad_mode=1)     # [hidden, T]
        return self._transpose(x)

    @torch.no_grad()
    def encode(self, wav: torch.Tensor) -> torch.Tensor:
        return self._quantize(self.encode_latent(wav)).unsqueeze(0)

    def _quantize(self, lat):
        """latent [T, hidden] -> codes [K, T] int64 (both residual VQs; every row on its own)."""
        T = lat.shape[0]
        codes = torch.empty(self.K, T, dtype=torch.int64, device=self.dev)
        q = "quantizer.semantic_residual_vector_quantizer"
        ops.rvq_encode(self._linear(lat, self.w[f"{q}.in"]), self.cb["semantic"], codes[:self.n_sem], self.n_sem)
        if self.K > self.n_sem:
            q = "quantizer.acoustic_residual_vector_quantizer"
            na = self.K - self.n_sem
            ops.rvq_encode(self._linear(lat, self.w[f"{q}.in"]), self.cb["acoustic"][:na].contiguous(), codes[self.n_sem:], 0)
        return codes

    def encode_stream(self, max_chunk_frames: int = 32) -> "MimiEncodeStream":
        """A stateful encoder: ``step(wav [1,1,n*1920])`` returns the codes [1,K,n] of the next n frames, and the concatenated
        steps equal ``encode`` of all the samples, bit for bit."""
        return MimiEncodeStream(self, max_chunk_frames)

    def encode_stream_rows(self, slots: int = 16, max_chunk_frames: int = 32) -> "MimiEncodeStreamRows":
        """``encode_stream`` for up to ``slots`` (<= 16) utterances heard at once: ``open(slot)`` starts one, ``step(slots, wav
        [R, n*1920])`` returns the next n frames' codes of R of them ([R, K, n]) from one launch per op; ``feed`` / ``drain`` buffer
        and batch.  Every slot's concatenated codes equal ``encode`` of its whole frames, bit for bit."""
        return MimiEncodeStreamRows(self, slots, max_chunk_frames)

    def _dequantize(self, c):
        """codes [K, T] int64 -> latent [T, hidden] (both residual VQs + their output projections)."""
        K, T = c.shape
        lat = torch.zeros(T, self.hidden, dtype=F32, device=self.dev)
        for name, lo, hi in (("semantic", 0, min(K, self.n_sem)), ("acoustic", self.n_sem, K)):
            if hi <= lo:
                continue
            q = f"quantizer.{name}_residual_vector_quantizer"
            zq = torch.empty(T, self.cdim, dtype=F32, device=self.dev)
            ops.rvq_decode(c[lo:hi].contiguous(), self.cb[name][:hi - lo].contiguous(), zq)
            lat = self._linear(zq, self.w[f"{q}.out"], res=lat)
        return lat

    @torch.no_grad()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        c = codes[0].to(self.dev, torch.int64).contiguous()
        lat = self._dequantize(c)
        x = self._convt(self._transpose(lat), "upsample", 4, 2)                       # [hidden, 2T]
        x = self._transformer(self._transpose(x), "decoder_transformer")
        x = self._conv(self._transpose(x), "decoder.layers.0", 7)
        idx = 1
        for r in self.ratios:
            x = self._convt(x, f"decoder.layers.{idx + 1}", 2 * r, r, elu=True)
            x = self._resblock(x, f"decoder.layers.{idx + 2}")
            idx += 3
        x = self._conv(x, f"decoder.layers.{idx + 1}", 3, elu=True)                  # [1, N]
        return x.reshape(1, 1, -1)

    def decode_stream(self, max_chunk_frames: int = 32) -> "MimiDecodeStream":
        """A stateful decoder: ``step(codes [1,K,n])`` returns the n * 1920 samples of the next n frames, and the concatenated
        steps equal ``decode`` of all the frames, bit for bit."""
        return MimiDecodeStream(self, max_chunk_frames)

    def decode_stream_rows(self, slots: int = 16, max_chunk_frames: int = 32, state_slots=None) -> "MimiDecodeStreamRows":
        """``decode_stream`` for up to ``slots`` (<= 16) utterances that join and leave independently: ``open(slot)`` starts one,
        ``step(slots, codes [R,K,n])`` returns the next n frames' audio of R of them ([R, n * 1920]) from one launch per op.  Every
        slot's concatenated chunks equal ``decode`` of its frames, bit for bit.  ``state_slots`` (>= slots; None: ``slots``): how
        many streams keep a state - slot indices then run over 0 .. state_slots - 1 and a ``step`` still takes at most ``slots``."""
        return MimiDecodeStreamRows(self, slots, max_chunk_frames, state_slots)


class MimiEncodeStream:
    """Streaming state of ``MimiCodec.encode``: audio goes in as it arrives, 80 ms frame by 80 ms frame, and its codes come out.
    Every encoder op is causal - SEANet convs padded on the left by k_eff - stride, a causal windowed transformer, the stride-2
    downsample edge-replicated on the left - and every kernel computes an output with a reduction order that does not depend on
    the sequence length, so the concatenated codes of all ``step`` / ``feed`` calls equal ``encode(wav)[..., :whole_frames]`` bit
    for bit, for any split.  The state is:
      * per conv layer (``encoder_conv_layers``), the last ``history_len`` input columns in two buffers that alternate each
        step; the stride-1 layers run csm_conv1d_stream_f32, the strided ones csm_conv1d_stream_strided_f32, and the first
        chunk of ``downsample`` takes its history from its own first column (``edge_first``);
      * per encoder-transformer layer, a K/V ring of ``window + 2 * max_chunk_frames - 1`` post-RoPE rows;
      * the number of frames encoded so far, and the samples of a frame not yet complete (``feed``), on the device.
    ``step`` makes no host synchronisation.
    The one deviation: ``encode`` of a waveform that is not a whole number of frames pads every LAYER on the right, ``flush``
    pads the WAVEFORM with zeros - so the codes of that last partial frame may differ from ``encode(wav)``'s; they equal
    ``encode(zero-padded wav)``'s."""

    def __init__(self, codec: MimiCodec, max_chunk_frames: int = 32):
        if max_chunk_frames < 1:
            raise ValueError("max_chunk_frames must be >= 1")
        self.codec = codec
        dev, w = codec.dev, codec.w
        self.layers = {name: (k, stride, elu, rep) for name, k, stride, elu, rep in encoder_conv_layers(codec.ratios)}
        self.frame = math.prod(stride for _, stride, _, _ in self.layers.values())        # samples per frame (1920)
        self.hist = {}
        for name, (k, stride, _, _) in self.layers.items():
            H = history_len("conv", k, stride)
            C_in = w[f"{name}.conv.weight"].shape[1]                                       # (every encoder conv has groups = 1)
            self.hist[name] = [torch.zeros(C_in, H, dtype=F32, device=dev) for _ in range(2)] if H else None
        self.ring = codec.window + 2 * max_chunk_frames - 1
        self.kv = [tuple(torch.zeros(self.ring, codec.hidden, dtype=F32, device=dev) for _ in range(2)) for _ in range(codec.n_layers)]
        self.reset()

    def reset(self):
        """Start a new utterance."""
        for bufs in self.hist.values():
            if bufs is not None:
                bufs[0].zero_()
        self._par = 0                      # hist[name][_par] holds the current history
        self.pos = 0                       # frames encoded so far
        self._rem = torch.zeros(0, dtype=F32, device=self.codec.dev)       # feed(): samples of the frame in progress

    def _conv(self, x, name, res=None, edge_first=False):
        k, stride, elu, _ = self.layers[name]
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        bufs = self.hist[name]
        h, h_next = (None, None) if bufs is None else (bufs[self._par], bufs[self._par ^ 1])
        y = torch.empty(wt.shape[0], x.shape[1] // stride, dtype=F32, device=self.codec.dev)
        if stride == 1:
            return ops.conv1d_stream_f32(h, x, wt, b, y, h_next, 1, elu, res)
        return ops.conv1d_stream_strided_f32(h, x, wt, b, y, h_next, stride, 1, elu, res, edge_first)

    @torch.no_grad()
    def step(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [1, 1, n * 1920], n >= 1 -> the codes of the next n frames [1, K, n] int64."""
        cd = self.codec
        if wav.numel() == 0 or wav.numel() % self.frame:
            raise ValueError(f"step takes a whole number (>= 1) of {self.frame}-sample frames, got {wav.numel()} samples "
                             "(feed() takes any length)")
        n = wav.numel() // self.frame
        x = wav.reshape(1, -1).to(cd.dev, F32).contiguous()
        x = self._conv(x, "encoder.layers.0")
        idx = 1
        for _ in cd.ratios:
            h = self._conv(x, f"encoder.layers.{idx}.block.1")
            x = self._conv(h, f"encoder.layers.{idx}.block.3", res=x)
            x = self._conv(x, f"encoder.layers.{idx + 2}")
            idx += 3
        x = self._conv(x, f"encoder.layers.{idx + 1}")                                           # [hidden, 2n]
        x = cd._transformer(cd._transpose(x), "encoder_transformer", pos0=2 * self.pos, kv=self.kv)
        x = self._conv(cd._transpose(x), "downsample", edge_first=self.pos == 0)                 # [hidden, n]
        codes = cd._quantize(cd._transpose(x))
        self._par ^= 1
        self.pos += n
        return codes.unsqueeze(0)

    def _none(self):
        return torch.zeros(1, self.codec.K, 0, dtype=torch.int64, device=self.codec.dev)

    @torch.no_grad()
    def feed(self, wav: torch.Tensor) -> torch.Tensor:
        """Any number of samples (none included): the codes of the whole frames now available ([1, K, 0] when there is none); the
        samples of the frame in progress wait on the device for the next call."""
        buf = torch.cat([self._rem, wav.reshape(-1).to(self.codec.dev, F32)])
        whole = buf.numel() // self.frame * self.frame
        self._rem = buf[whole:].clone()
        return self.step(buf[:whole]) if whole else self._none()

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """The codes of the held partial frame, zero-padded to a whole one ([1, K, 0] when nothing is held)."""
        if not self._rem.numel():
            return self._none()
        pad = torch.zeros(self.frame - self._rem.numel(), dtype=F32, device=self.codec.dev)
        buf, self._rem = torch.cat([self._rem, pad]), self._rem[:0]
        return self.step(buf)


class MimiEncodeStreamRows:
    """``MimiEncodeStream`` for up to 16 utterances heard at once: the same state with a leading slot dimension, and a ``step``
    that encodes one chunk of R of them with ONE launch per op - csm_conv1d_stream_rows_f32 for the stride-1 convs,
    csm_conv1d_stream_strided_rows_f32 for the strided ones, the rows transformer of ``MimiDecodeStreamRows``; LayerNorm, the
    linears and the RVQ search are row-wise and run on the stacked rows.  An encoder step is latency-bound (a chain of dependent
    FMAs per output), so the rows ride along.  Every row is computed with the arithmetic of the one-row kernels, so a slot's
    concatenated codes equal ``MimiEncodeStream``'s and ``MimiCodec.encode``'s on its whole frames, bit for bit, whatever its
    neighbours do.
    State per slot: both history buffers of every conv layer ([slots, 2, C_in, H]), a K/V ring of
    ``window + 2 * max_chunk_frames - 1`` rows per transformer layer, the frames encoded so far and the history parity (host),
    and the samples not yet encoded: the remainder of the last ``drain`` on the device plus the pieces ``feed`` was given since.
    ``step`` makes no host synchronisation: slots, parities, positions and the edge-first flags reach the kernels by value.
    The rows kernels take one chunk size per launch; ``drain`` brings ragged slots to it with ``peel_schedule``.
    ``flush`` pads the WAVEFORM of a partial frame with zeros, as ``MimiEncodeStream.flush`` does."""

    def __init__(self, codec: MimiCodec, slots: int = 16, max_chunk_frames: int = 32):
        if not 1 <= slots <= 16:
            raise ValueError(f"slots must be 1..16 (the rows kernels take at most 16 rows a launch), got {slots}")
        if max_chunk_frames < 1:
            raise ValueError("max_chunk_frames must be >= 1")
        self.codec, self.slots, self.max_chunk_frames = codec, slots, max_chunk_frames
        dev, w = codec.dev, codec.w
        self.layers = {name: (k, stride, elu, rep) for name, k, stride, elu, rep in encoder_conv_layers(codec.ratios)}
        self.frame = math.prod(stride for _, stride, _, _ in self.layers.values())        # samples per frame (1920)
        self.hist = {}
        for name, (k, stride, _, _) in self.layers.items():
            H = history_len("conv", k, stride)
            C_in = w[f"{name}.conv.weight"].shape[1]                                       # (every encoder conv has groups = 1)
            self.hist[name] = torch.zeros(slots, 2, C_in, H, dtype=F32, device=dev) if H else None
        self.ring = codec.window + 2 * max_chunk_frames - 1
        self.kv = [tuple(torch.zeros(slots, self.ring, codec.hidden, dtype=F32, device=dev) for _ in range(2))
                   for _ in range(codec.n_layers)]
        self.pos = [0] * slots             # frames encoded so far, per slot
        self._par = [0] * slots            # hist[name][slot, _par[slot]] holds the slot's current history
        self._live = [False] * slots       # open(slot) .. close(slot)
        self._rem = [None] * slots         # device: the samples the last drain left over (less than a frame), or None
        self._fed = [[] for _ in range(slots)]     # the pieces fed since, as given
        self._count = [0] * slots          # samples waiting: remainder + pieces

    def _slot(self, slot):
        if not 0 <= slot < self.slots:
            raise ValueError(f"slot {slot} out of range (0..{self.slots - 1})")
        return int(slot)

    def open(self, slot: int):
        """Start a new utterance in ``slot`` (also after an earlier one ended there): zero histories, position 0, nothing waiting."""
        slot = self._slot(slot)
        for arena in self.hist.values():
            if arena is not None:
                arena[slot].zero_()
        self._par[slot] = 0
        self.pos[slot] = 0
        self._live[slot] = True
        self._rem[slot], self._fed[slot], self._count[slot] = None, [], 0

    def close(self, slot: int):
        """The utterance in ``slot`` is over: what still waits there is dropped and ``drain()`` no longer visits it."""
        slot = self._slot(slot)
        self._live[slot] = False
        self._rem[slot], self._fed[slot], self._count[slot] = None, [], 0

    @property
    def open_slots(self):
        return [s for s in range(self.slots) if self._live[s]]

    def _conv(self, x, name, rows, res=None, edge_first=()):
        k, stride, elu, _ = self.layers[name]
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        y = torch.empty(x.shape[0], wt.shape[0], x.shape[2] // stride, dtype=F32, device=self.codec.dev)
        par = [self._par[s] for s in rows]
        if stride == 1:
            return ops.conv1d_stream_rows_f32(self.hist[name], x, wt, b, y, rows, par, 1, elu, res)
        return ops.conv1d_stream_strided_rows_f32(self.hist[name], x, wt, b, y, rows, par, stride, 1, elu, res, edge_first)

    def _transpose(self, x):
        y = torch.empty(x.shape[0], x.shape[2], x.shape[1], dtype=F32, device=self.codec.dev)
        return ops.transpose_rows_f32(x, y)

    @torch.no_grad()
    def step(self, slots, wav: torch.Tensor) -> torch.Tensor:
        """wav [R, n * 1920] - the next n frames of the utterances in ``slots`` (R distinct slot indices, in the rows' order) ->
        their codes [R, K, n] int64."""
        cd = self.codec
        rows = [int(s) for s in slots]
        R = len(rows)
        if not 1 <= R <= self.slots or len(set(rows)) != R or any(not 0 <= s < self.slots for s in rows):
            raise ValueError(f"step takes 1..{self.slots} distinct slots in 0..{self.slots - 1}, got {rows}")
        if wav.dim() != 2 or wav.shape[0] != R or wav.shape[1] == 0 or wav.shape[1] % self.frame:
            raise ValueError(f"wav must be [R = {R}, n * {self.frame}] with n >= 1, got {tuple(wav.shape)}")
        n = wav.shape[1] // self.frame
        if n > self.max_chunk_frames:
            raise ValueError(f"a step takes 1..max_chunk_frames = {self.max_chunk_frames} frames per row, got {n}")
        x = wav.reshape(R, 1, -1).to(cd.dev, F32).contiguous()
        x = self._conv(x, "encoder.layers.0", rows)
        idx = 1
        for _ in cd.ratios:
            h = self._conv(x, f"encoder.layers.{idx}.block.1", rows)
            x = self._conv(h, f"encoder.layers.{idx}.block.3", rows, res=x)
            x = self._conv(x, f"encoder.layers.{idx + 2}", rows)
            idx += 3
        x = self._conv(x, f"encoder.layers.{idx + 1}", rows)                                       # [R, hidden, 2n]
        x = _transformer_rows(cd, "encoder_transformer", self.kv, self._transpose(x).view(R * 2 * n, cd.hidden), rows,
                              [2 * self.pos[s] for s in rows], 2 * n)
        x = self._conv(self._transpose(x.view(R, 2 * n, cd.hidden)), "downsample", rows,
                       edge_first=[self.pos[s] == 0 for s in rows])                                # [R, hidden, n]
        codes = cd._quantize(self._transpose(x).view(R * n, cd.hidden))                            # [K, R * n], row after row
        for s in rows:
            self._par[s] ^= 1
            self.pos[s] += n
        return codes.view(cd.K, R, n).permute(1, 0, 2).contiguous()

    def feed(self, slot: int, wav: torch.Tensor) -> int:
        """Any number of samples for ``slot``: they wait for the next ``drain``.  Nothing is launched, copied or synchronised -
        the piece is held as given, so the caller must not overwrite it before that drain.  Returns ``pending(slot)``."""
        slot = self._slot(slot)
        if not self._live[slot]:
            raise ValueError(f"feed: slot {slot} is not open")
        if wav.numel():
            self._fed[slot].append(wav.detach().reshape(-1))
            self._count[slot] += wav.numel()
        return self._count[slot] // self.frame

    def pending(self, slot: int) -> int:
        """Whole frames waiting in ``slot``."""
        return self._count[self._slot(slot)] // self.frame

    @torch.no_grad()
    def drain(self, slots=None, flush=()):
        """Encode every whole frame waiting in ``slots`` (default: all open slots) -> {slot: codes [K, m] int64}, m >= 0.
        Slots named in ``flush`` (a subset of ``slots``) first have their partial frame zero-padded to a whole one.  The launches
        follow ``peel_schedule``."""
        cd = self.codec
        todo = self.open_slots if slots is None else [self._slot(s) for s in slots]
        flush = {self._slot(s) for s in flush}
        if len(set(todo)) != len(todo) or any(not self._live[s] for s in todo) or not flush <= set(todo):
            raise ValueError(f"drain takes distinct open slots and flushes only slots it drains, got {todo} / flush {sorted(flush)}")
        bufs = {}
        for s in todo:
            parts = ([self._rem[s]] if self._rem[s] is not None else []) + [p.to(cd.dev, F32) for p in self._fed[s]]
            tail = self._count[s] % self.frame
            if s in flush and tail:
                parts.append(torch.zeros(self.frame - tail, dtype=F32, device=cd.dev))
                self._count[s] += self.frame - tail
            if parts:
                bufs[s] = parts[0] if len(parts) == 1 else torch.cat(parts)
            self._fed[s] = []
        out = {s: [] for s in todo}
        at = dict.fromkeys(todo, 0)
        for n, group in peel_schedule({s: self._count[s] // self.frame for s in todo}, self.max_chunk_frames):
            m = n * self.frame
            codes = self.step(group, torch.stack([bufs[s][at[s]:at[s] + m] for s in group]))
            for r, s in enumerate(group):
                out[s].append(codes[r])
                at[s] += m
        for s in todo:
            self._count[s] -= at[s]
            self._rem[s] = bufs[s][at[s]:].clone() if self._count[s] else None
        none = torch.zeros(cd.K, 0, dtype=torch.int64, device=cd.dev)
        return {s: torch.cat(c, 1) if c else none for s, c in out.items()}


class MimiDecodeStream:
    """Streaming state of ``MimiCodec.decode``. Every decoder op is causal (stride-1 convs with left zero padding, transposed
    convs cropped on the right, a causal windowed transformer), so frame t's samples depend on codes 0..t only, and every
    kernel computes an output with a reduction order that does not depend on the sequence length.  The state is:
      * per conv / transposed conv layer, the last ``history_len`` input columns ([C_in, H] fp32), in two buffers that
        alternate each step (the kernel reads one and writes the next history into the other);
      * per decoder-transformer layer, a K/V ring of ``window + 2 * max_chunk_frames - 1`` post-RoPE rows (position p in slot
        p % ring): larger than the window so that one launch can append a chunk's keys while its earlier queries still read
        the keys those slots held;
      * the number of frames decoded so far.
    ``step`` makes no host synchronisation; chunks may be any size >= 1 (more than ``max_chunk_frames`` costs extra attention
    launches)."""

    def __init__(self, codec: MimiCodec, max_chunk_frames: int = 32):
        if max_chunk_frames < 1:
            raise ValueError("max_chunk_frames must be >= 1")
        self.codec = codec
        dev, w = codec.dev, codec.w
        self.hist = {}
        for name, kind, k, stride, _ in decoder_conv_layers(codec.ratios):
            wt = w[f"{name}.conv.weight"]
            H = history_len(kind, k, stride)
            C_in = wt.shape[0] if kind == "convt" else wt.shape[1]
            self.hist[name] = [torch.zeros(C_in, H, dtype=F32, device=dev) for _ in range(2)] if H else None
        self.ring = codec.window + 2 * max_chunk_frames - 1
        self.kv = [tuple(torch.zeros(self.ring, codec.hidden, dtype=F32, device=dev) for _ in range(2)) for _ in range(codec.n_layers)]
        self.reset()

    def reset(self):
        """Start a new utterance."""
        for bufs in self.hist.values():
            if bufs is not None:
                bufs[0].zero_()
        self._par = 0                      # hist[name][_par] holds the current history
        self.cols = {name: 0 for name in self.hist}
        self.pos = 0                       # frames decoded so far

    def _hist(self, name):
        bufs = self.hist[name]
        return (None, None) if bufs is None else (bufs[self._par], bufs[self._par ^ 1])

    def _conv(self, x, name, elu=False, res=None):
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        h, h_next = self._hist(name)
        y = torch.empty(wt.shape[0], x.shape[1], dtype=F32, device=self.codec.dev)
        return ops.conv1d_stream_f32(h, x, wt, b, y, h_next, 1, elu, res)

    def _convt(self, x, name, stride, elu=False):
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        C_in, cout_g, _ = wt.shape
        groups = 1 if cout_g != 1 or C_in == 1 else C_in          # as MimiCodec._convt
        h, h_next = self._hist(name)
        y = torch.empty(cout_g * groups, x.shape[1] * stride, dtype=F32, device=self.codec.dev)
        ops.conv_transpose1d_stream_f32(h, x, wt, b, y, h_next, self.cols[name], stride, groups, elu)
        self.cols[name] += x.shape[1]
        return y

    @torch.no_grad()
    def step(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [1, K, n] -> the next n frames of audio [1, 1, n * 1920]."""
        cd = self.codec
        c = codes[0].to(cd.dev, torch.int64).contiguous()
        n = c.shape[1]
        if n < 1:
            raise ValueError("step needs at least one frame")
        x = self._convt(cd._transpose(cd._dequantize(c)), "upsample", 2)                         # [hidden, 2n]
        x = cd._transformer(cd._transpose(x), "decoder_transformer", pos0=2 * self.pos, kv=self.kv)
        x = self._conv(cd._transpose(x), "decoder.layers.0")
        idx = 1
        for r in cd.ratios:
            x = self._convt(x, f"decoder.layers.{idx + 1}", r, elu=True)
            h = self._conv(x, f"decoder.layers.{idx + 2}.block.1", elu=True)
            x = self._conv(h, f"decoder.layers.{idx + 2}.block.3", elu=True, res=x)
            idx += 3
        x = self._conv(x, f"decoder.layers.{idx + 1}", elu=True)                                 # [1, n * 1920]
        self._par ^= 1
        self.pos += n
        return x.reshape(1, 1, -1)


class MimiDecodeStreamRows:
    """``MimiDecodeStream`` for up to 16 utterances at once: the same state with a leading slot dimension, and a ``step`` that
    decodes one chunk of every active utterance with ONE launch per op (the rows forms of the streaming kernels,
    csm_*_stream_rows_f32) instead of one decoder step per utterance.  A streaming step is latency-bound - a chain of dependent
    FMAs per output - so the rows ride along at little extra cost.  Utterances join and leave independently: each slot has its
    own frame count (from which the transposed convolutions', RoPE's and the K/V ring's absolute positions follow) and its own
    history parity.  Every row is computed with the arithmetic of the one-row kernels, so the concatenated chunks of a slot
    equal ``MimiDecodeStream.step``'s and ``MimiCodec.decode``'s, bit for bit, whatever its neighbours do.
    State per slot: both history buffers of every conv layer ([slots, 2, C_in, H]), a K/V ring of
    ``window + 2 * max_chunk_frames - 1`` rows per transformer layer, the frames decoded so far and the parity.
    ``step`` makes no host synchronisation: slots, parities and positions reach the kernels by value.
    ``state_slots`` >= slots sizes the arenas for more streams than a launch has rows (the kernels take the arena's slot count
    apart from the rows of a launch): slot indices run over 0 .. state_slots - 1, a ``step`` takes at most ``slots`` of them."""

    def __init__(self, codec: MimiCodec, slots: int = 16, max_chunk_frames: int = 32, state_slots: Optional[int] = None):
        if not 1 <= slots <= 16:
            raise ValueError(f"slots must be 1..16 (the rows kernels take at most 16 rows a launch), got {slots}")
        if max_chunk_frames < 1:
            raise ValueError("max_chunk_frames must be >= 1")
        if state_slots is not None and (isinstance(state_slots, bool) or int(state_slots) != state_slots or state_slots < slots):
            raise ValueError(f"state_slots must be an integer >= slots = {slots} (None: one state per row of a launch), got {state_slots!r}")
        self.codec, self.slots, self.max_chunk_frames = codec, slots, max_chunk_frames
        # the streams that keep a state here: ``slots`` of them, or - more streams than rows of a launch - ``state_slots``; a
        # stream then keeps its slot for its whole life, whichever rows it is stepped with, and nothing is ever copied
        self.state_slots = slots if state_slots is None else int(state_slots)
        slots = self.state_slots
        dev, w = codec.dev, codec.w
        self.hist = {}
        for name, kind, k, stride, _ in decoder_conv_layers(codec.ratios):
            wt = w[f"{name}.conv.weight"]
            H = history_len(kind, k, stride)
            C_in = wt.shape[0] if kind == "convt" else wt.shape[1]
            self.hist[name] = torch.zeros(slots, 2, C_in, H, dtype=F32, device=dev) if H else None
        self.ring = codec.window + 2 * max_chunk_frames - 1
        self.kv = [tuple(torch.zeros(slots, self.ring, codec.hidden, dtype=F32, device=dev) for _ in range(2))
                   for _ in range(codec.n_layers)]
        self.pos = [0] * slots             # frames decoded so far, per slot
        self._par = [0] * slots            # hist[name][slot, _par[slot]] holds the slot's current history

    def open(self, slot: int):
        """Start a new utterance in ``slot`` (also after an earlier one ended there)."""
        if not 0 <= slot < self.state_slots:
            raise ValueError(f"slot {slot} out of range (0..{self.state_slots - 1})")
        for arena in self.hist.values():
            if arena is not None:
                arena[slot].zero_()
        self._par[slot] = 0
        self.pos[slot] = 0

    def _conv(self, x, name, rows, elu=False, res=None):
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        y = torch.empty(x.shape[0], wt.shape[0], x.shape[2], dtype=F32, device=self.codec.dev)
        return ops.conv1d_stream_rows_f32(self.hist[name], x, wt, b, y, rows, [self._par[s] for s in rows], 1, elu, res)

    def _convt(self, x, name, stride, rows, n, elu=False):
        wt, b = self.codec.w[f"{name}.conv.weight"], self.codec.w.get(f"{name}.conv.bias")
        C_in, cout_g, _ = wt.shape
        groups = 1 if cout_g != 1 or C_in == 1 else C_in          # as MimiCodec._convt
        cols = x.shape[2] // n                                    # input columns of this layer per frame
        y = torch.empty(x.shape[0], cout_g * groups, x.shape[2] * stride, dtype=F32, device=self.codec.dev)
        return ops.conv_transpose1d_stream_rows_f32(self.hist[name], x, wt, b, y, rows, [self._par[s] for s in rows],
                                                    [self.pos[s] * cols for s in rows], stride, groups, elu)

    def _transpose(self, x):
        y = torch.empty(x.shape[0], x.shape[2], x.shape[1], dtype=F32, device=self.codec.dev)
        return ops.transpose_rows_f32(x, y)

    def _transformer(self, x, rows, n2):
        """The decoder transformer on the stacked rows x [R*n2, hidden], each row at position 2 * frames-so-far."""
        return _transformer_rows(self.codec, "decoder_transformer", self.kv, x, rows, [2 * self.pos[s] for s in rows], n2)

    @torch.no_grad()
    def step(self, slots, codes: torch.Tensor) -> torch.Tensor:
        """codes [R, K, n] - the next n frames of the utterances in ``slots`` (R distinct slot indices, in the rows' order) ->
        their audio [R, n * 1920]."""
        cd = self.codec
        rows = [int(s) for s in slots]
        R = len(rows)
        if not 1 <= R <= self.slots or len(set(rows)) != R or any(not 0 <= s < self.state_slots for s in rows):
            raise ValueError(f"step takes 1..{self.slots} distinct slots in 0..{self.state_slots - 1}, got {rows}")
        if codes.dim() != 3 or codes.shape[0] != R:
            raise ValueError(f"codes must be [R = {R}, K, n], got {tuple(codes.shape)}")
        K, n = codes.shape[1], codes.shape[2]
        if not 1 <= n <= self.max_chunk_frames:
            raise ValueError(f"a step takes 1..max_chunk_frames = {self.max_chunk_frames} frames per row, got {n}")
        c = codes.to(cd.dev, torch.int64).permute(1, 0, 2).reshape(K, R * n).contiguous()        # frames stacked row after row
        lat = cd._dequantize(c).view(R, n, cd.hidden)
        x = self._convt(self._transpose(lat), "upsample", 2, rows, n)                              # [R, hidden, 2n]
        x = self._transformer(self._transpose(x).view(R * 2 * n, cd.hidden), rows, 2 * n)
        x = self._conv(self._transpose(x.view(R, 2 * n, cd.hidden)), "decoder.layers.0", rows)
        idx = 1
        for r in cd.ratios:
            x = self._convt(x, f"decoder.layers.{idx + 1}", r, rows, n, elu=True)
            h = self._conv(x, f"decoder.layers.{idx + 2}.block.1", rows, elu=True)
            x = self._conv(h, f"decoder.layers.{idx + 2}.block.3", rows, elu=True, res=x)
            idx += 3
        x = self._conv(x, f"decoder.layers.{idx + 1}", rows, elu=True)                            # [R, 1, n * 1920]
        for s in rows:
            self._par[s] ^= 1
            self.pos[s] += n
        return x.reshape(R, -1)
