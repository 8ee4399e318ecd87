"""Sequence packing on the host: ``csm.data.collate_packed`` (first-fit packing, the per-segment target rule) and the presence of
the two segment-masked attention entry points in the header, the bindings and the library.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from csm.data import collate_packed, create_dataloader
from csm.data.training_data import IGNORE_INDEX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4


def _example(i, S, T):
    """Tokens that name their example and position, so a copy can be recognised anywhere."""
    tok = (1000 * (i + 1) + torch.arange(S))[:, None].repeat(1, K + 1)
    mask = torch.zeros(S, K + 1, dtype=torch.bool)
    mask[:, i % (K + 1)] = True
    tg = (100 * (i + 1) + torch.arange(T))[:, None].repeat(1, K) % 60
    return {"input_tokens": tok, "input_masks": mask, "target_audio_tokens": tg}


# (S_i, T_i): T_i = S_i - 1, shorter, longer (T_i = S_i as CSMDataset may give), a length-1 example, two equal lengths (a tie)
SHAPES = [(40, 39), (31, 20), (33, 33), (17, 16), (50, 60), (1, 1), (33, 32), (128, 127), (90, 10)]


def _check(batch, out, max_seq_len):
    tok, mk, tg, seg = out["input_tokens"], out["input_masks"], out["target_audio_tokens"], out["segment_lengths"]
    R, S, _ = tok.shape
    assert mk.shape == tok.shape and tg.shape == (R, S, K) and seg.shape[0] == R and seg.dtype == torch.long
    assert S <= max_seq_len and (S % 128 == 0 or S == max_seq_len)
    assert S == min(max_seq_len, -(-int(seg.sum(1).max()) // 128) * 128)
    want_tg = torch.full_like(tg, IGNORE_INDEX)
    seen = []
    for r in range(R):
        lens = seg[r][seg[r] > 0].tolist()
        assert seg[r].tolist() == lens + [0] * (seg.shape[1] - len(lens)) and sum(lens) <= S
        o = 0
        for n in lens:
            i = int(tok[r, o, 0]) // 1000 - 1                       # which example starts here
            b = batch[i]
            seen.append(i)
            assert n == b["input_tokens"].shape[0]
            assert torch.equal(tok[r, o:o + n], b["input_tokens"]) and torch.equal(mk[r, o:o + n], b["input_masks"])
            t = min(n - 1, b["target_audio_tokens"].shape[0])
            want_tg[r, o:o + t] = b["target_audio_tokens"][:t]
            o += n
        assert not bool(mk[r, o:].any()) and not bool(tok[r, o:].any())     # the row's padding
    assert sorted(seen) == list(range(len(batch))), "every example exactly once"
    assert torch.equal(tg, want_tg), "targets: the per-segment position rule, IGNORE_INDEX everywhere else"
    return seg


def test_collate_packed_layout_and_target_rule():
    batch = [_example(i, S, T) for i, (S, T) in enumerate(SHAPES)]
    out = collate_packed(batch, max_seq_len=128)
    seg = _check(batch, out, 128)
    # first fit over decreasing lengths, ties in batch order: 128 | 90 33(2) 1 | 50 40 33(6) | 31 17
    assert [[x for x in r if x] for r in seg.tolist()] == [[128], [90, 33, 1], [50, 40, 33], [31, 17]]
    assert int(out["input_tokens"][1, 90, 0]) // 1000 - 1 == 2 and int(out["input_tokens"][2, 90, 0]) // 1000 - 1 == 6   # the tie
    again = collate_packed(batch, max_seq_len=128)
    assert all(torch.equal(out[k], again[k]) for k in out), "the same input gives the same output"


def test_collate_packed_rounds_the_row_length_up_to_128_and_caps_it():
    batch = [_example(i, S, T) for i, (S, T) in enumerate([(40, 39), (31, 30), (33, 32), (17, 16), (50, 49)])]
    out = collate_packed(batch, max_seq_len=2048)
    assert out["input_tokens"].shape[:2] == (1, 256) and out["segment_lengths"].tolist() == [[50, 40, 33, 31, 17]]
    _check(batch, out, 2048)
    out = collate_packed(batch, max_seq_len=100)
    assert out["input_tokens"].shape[:2] == (2, 100) and out["segment_lengths"].tolist() == [[50, 40, 0], [33, 31, 17]]
    _check(batch, out, 100)
    out = collate_packed(batch, max_seq_len=128)                 # what tests/test_packed_train_gpu.py trains on: 2 rows of 128
    assert out["input_tokens"].shape[:2] == (2, 128) and out["segment_lengths"].tolist() == [[50, 40, 33], [31, 17, 0]]


def test_collate_packed_refuses_an_over_long_example():
    batch = [_example(0, 40, 39), _example(1, 129, 128)]
    with pytest.raises(ValueError, match="max_seq_len"):
        collate_packed(batch, max_seq_len=128)


def test_dataloader_selects_the_packed_collate():
    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(SHAPES)

        def __getitem__(self, i):
            return _example(i, *SHAPES[i])

    for b in create_dataloader(DS(), batch_size=4, shuffle=False, num_workers=0, pin_memory=False, pack_sequences=True, max_seq_len=128):
        assert "segment_lengths" in b and b["input_tokens"].shape[1] == 128
    plain = next(iter(create_dataloader(DS(), batch_size=4, shuffle=False, num_workers=0, pin_memory=False)))
    assert "segment_lengths" not in plain


def test_cli_flag():
    import argparse
    from csm.cli.common import add_data_args
    p = argparse.ArgumentParser()
    add_data_args(p)
    assert p.parse_args(["--pack-sequences"]).pack_sequences and not p.parse_args([]).pack_sequences


def test_segment_exports_in_header_bindings_and_library():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csm_hip.h")).read(), flags=re.S)
    from csm import hip
    from csm.hip import ops
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name, nargs in (("csm_attn_fwd_seg", 10), ("csm_attn_bwd_seg", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in hip.EXPORTS and len(hip._SIGS[name][0]) == nargs and hasattr(lib, name)
    assert callable(ops.attn_fwd_seg) and callable(ops.attn_bwd_seg)
    assert hip.lib.csm_abi_version() == 3
