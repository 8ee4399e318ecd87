"""Streaming Mimi decode, host side: the csm-generate flags and the per-layer state plan, checked against the decoder's own
layer list (the Hugging Face port of the architecture, built on the CPU)."""
import torch


def test_generate_cli_stream_flags():
    from csm.cli.generate import parse_args
    base = ["--model-path", "c.pt", "--text", "hi", "--mimi-weights", "m", "--text-tokenizer", "t"]
    a = parse_args(base)
    assert a.stream is False and a.chunk_frames == 4
    a = parse_args(base + ["--stream", "--chunk-frames", "2"])
    assert a.stream is True and a.chunk_frames == 2


def test_decoder_conv_layers_match_hf_decoder():
    from transformers import MimiConfig, MimiModel
    from csm.codec.mimi import decoder_conv_layers, history_len
    torch.manual_seed(0)
    hf = MimiModel(MimiConfig()).eval()
    layers = decoder_conv_layers(tuple(MimiConfig().upsampling_ratios))
    for name, kind, k, stride, elu in layers:
        conv = hf.get_submodule(name).conv
        assert isinstance(conv, torch.nn.ConvTranspose1d if kind == "convt" else torch.nn.Conv1d), name
        assert conv.kernel_size[0] == k and conv.stride[0] == stride and conv.dilation[0] == 1, name
        if kind == "convt":
            assert conv.padding[0] == 0, name                      # the overhang is cropped afterwards, on the right
        if name.startswith("decoder.layers.") and ".block." not in name:
            idx = int(name.split(".")[2])
            assert isinstance(hf.decoder.layers[idx - 1], torch.nn.ELU) == elu, name
    # every convolution of the decoder side is in the plan, exactly once
    convs = {n[:-len(".conv")] for n, mod in hf.named_modules()
             if isinstance(mod, (torch.nn.Conv1d, torch.nn.ConvTranspose1d)) and (n.startswith("decoder.") or n.startswith("upsample."))}
    assert convs == {name for name, *_ in layers} and len(layers) == len(convs)
    # the carried input columns: 1 for every transposed conv (k = 4 s = 2, k = 2r s = r), (k-1) for the stride-1 convs
    hist = [history_len(kind, k, stride) for _, kind, k, stride, _ in layers]
    assert hist == [1, 6] + [1, 2, 0] * 4 + [2]


def test_history_len_and_ring_slots():
    from csm.codec.mimi import history_len, ring_slot
    assert history_len("conv", 7) == 6 and history_len("conv", 3, dilation=2) == 4 and history_len("conv", 1) == 0
    assert history_len("convt", 4, 2) == 1 and history_len("convt", 16, 8) == 1 and history_len("convt", 2, 2) == 0
    assert history_len("convt", 7, 2) == 3 and history_len("convt", 5, 2) == 2
    # ring of window + m - 1 slots: a launch of up to m new positions writes slots that no query of that launch reads
    window, m = 250, 8
    ring = window + m - 1
    for pos0 in (0, 5, 249, 250, 251, 1000, 12345):
        for n in range(1, m + 1):
            read = range(max(0, pos0 - window + 1), pos0)
            written = range(pos0, pos0 + n)
            slots_r = {ring_slot(p, ring) for p in read}
            slots_w = {ring_slot(p, ring) for p in written}
            assert len(slots_w) == n and not (slots_r & slots_w)
    # a ring of exactly `window` slots would not do: the chunk's second position lands on a key its first query reads
    assert ring_slot(1001, window) == ring_slot(1001 - window, window) and 1001 - window > 1000 - window
