"""Weight-only FP8 decode, the parts that need no GPU: the torch restatement of the quantiser (csm/quant.py) against the e4m3
format's own error bound, the grid-snap helper of the GPU tests, and the public surface (header, CLI flag, Model attribute)."""
import os

import pytest
import torch

from csm.quant import dequantize_rows_fp8, quantize_rows_fp8, snap_rows_to_fp8_grid

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the (N, K) of tests/test_generate_wide_batch_gpu.py::SHAPES (that module is GPU-marked as a whole; the list is restated here)
SHAPES = [(3072, 2048), (2048, 2048), (16384, 2048), (2048, 8192), (2112, 2048), (1024, 2048), (1536, 1024), (1024, 1024),
          (16384, 1024), (1024, 8192), (2112, 1024), (1024, 256), (300, 512), (66, 96)]


def _weights(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    return (torch.randn(N, K, generator=g) * 0.02).to(BF)


def test_shapes_are_the_wide_batch_decode_shapes():
    src = open(os.path.join(ROOT, "tests", "test_generate_wide_batch_gpu.py")).read()
    for n, k in SHAPES:
        assert f"({n}, {k}, " in src, (n, k)


@pytest.mark.parametrize("N,K", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_restatement_meets_the_format_bound(N, K):
    """|q s - w| <= max(2^-4 |w|, 2^-10 s) (1 + 2^-10): half a unit of a 3-bit mantissa, half the smallest subnormal (2^-9),
    slack for the fp32 quotient.  No exception allowed."""
    W = _weights(N, K)
    q, s = quantize_rows_fp8(W)
    assert q.dtype == torch.uint8 and q.shape == (N, K) and s.dtype == torch.float32 and s.shape == (N,)
    w, d = W.float(), dequantize_rows_fp8(q, s)
    bound = torch.maximum(2.0 ** -4 * w.abs(), 2.0 ** -10 * s[:, None]) * (1 + 2.0 ** -10)
    err = (d - w).abs()
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements above the e4m3 bound, worst ratio {(err / bound).max():.4f}"
    assert int((q & 0x7F).max()) <= 0x7E, "a NaN code (0x7f / 0xff)"
    amax = w.abs().amax(1)
    assert bool((d.abs().amax(1) <= amax * (1 + 2.0 ** -10)).all()), "a dequantised value above its row's maximum"
    assert torch.equal(s, amax / 448.0)


def test_restatement_edges():
    q, s = quantize_rows_fp8(torch.zeros(3, 16, dtype=BF))
    assert torch.equal(s, torch.ones(3)) and int(q.max()) == 0
    # saturation: the row maximum maps to +-448 (0x7e / 0xfe), never to a NaN code; a plain cast would not saturate
    W = torch.tensor([[1.0, -1.0, 0.5, 2.0 ** -12, 2.0 ** -9 * 1.5 / 448, 0.0, 0.9999, -0.97] + [0.0] * 8]).to(BF)
    q, s = quantize_rows_fp8(W)
    assert q[0, 0] == 0x7E and q[0, 1] == 0xFE and float(s[0]) == float(torch.tensor(1.0) / 448)
    assert torch.isnan(torch.tensor(500.0).to(torch.float8_e4m3fn).float())
    d = dequantize_rows_fp8(q, s)
    assert float(d[0, 0]) == pytest.approx(1.0, rel=1e-6) and float(d[0, 2]) == pytest.approx(0.5, rel=1e-6)
    # subnormal codes: spacing 2^-9 in code units
    W = torch.zeros(1, 16, dtype=BF)
    W[0, 0] = 448.0
    W[0, 1:8] = torch.tensor([2.0 ** -9, 2.0 ** -10, 2.0 ** -9 * 1.5, 2.0 ** -11, 3 * 2.0 ** -9, 2.0 ** -6, 2.0 ** -7 * 1.25]).to(BF)
    q, s = quantize_rows_fp8(W)
    assert float(s[0]) == 1.0
    assert q[0, :8].tolist() == [0x7E, 0x01, 0x00, 0x02, 0x00, 0x03, 0x08, 0x05]      # ties to even: 2^-10 -> 0, 1.5 * 2^-9 -> 2
    with pytest.raises(ValueError, match="finite"):
        quantize_rows_fp8(torch.tensor([[float("inf")] * 16]))


@pytest.mark.parametrize("N,K", [(1536, 1024), (1024, 256), (300, 512), (66, 96)])
def test_grid_snap_is_lossless(N, K):
    W = _weights(N, K)
    Ws = snap_rows_to_fp8_grid(W)
    assert Ws.dtype == BF and torch.equal(Ws.float().to(BF).float(), Ws.float())
    q, s = quantize_rows_fp8(Ws)
    assert torch.equal(dequantize_rows_fp8(q, s).to(BF), Ws), "quantising snapped weights must return them exactly"
    assert torch.equal(dequantize_rows_fp8(q, s), Ws.float())
    assert bool((torch.log2(s) == torch.log2(s).round()).all()), "snapped rows have power-of-two scales"


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "csm_hip.h")).read()
    assert "int csm_quantize_rows_fp8(const void* W, void* W8, void* scale, int N, int K, int ldw, int ldw8, csm_stream_t stream);" in h
    assert "int csm_gemv_fp8w(const void* x, const void* W8, const void* scale, void* y, const void* residual, int B, int N, int K, int ldw8," in h
    assert "e4m3fn" in h and "fnuz" in h


def test_cli_lists_decode_weights(capsys):
    from csm.cli.generate import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    assert "--decode-weights" in capsys.readouterr().out
    base = ["--model-path", "m.pt", "--text", "hi", "--mimi-weights", "w", "--text-tokenizer", "t"]
    assert parse_args(base).decode_weights == "bf16"
    assert parse_args(base + ["--decode-weights", "fp8"]).decode_weights == "fp8"
    with pytest.raises(SystemExit):
        parse_args(base + ["--decode-weights", "int8"])


def test_model_decode_weights_attribute():
    from csm.models.model import Model, ModelArgs
    m = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 2051, 4))
    assert m.decode_weights == "bf16"
    m._decode_state = object()
    m.decode_weights = "bf16"
    assert m._decode_state is not None, "setting the same value keeps the state"
    m.decode_weights = "fp8"
    assert m.decode_weights == "fp8" and m._decode_state is None, "changing the mode drops the decode state (and its graph)"
    for bad in ("fp4", "FP8", None, 8):
        with pytest.raises(ValueError, match="decode_weights"):
            m.decode_weights = bad
    assert m.decode_weights == "fp8"
    import inspect
    from csm.generator import load_csm_1b
    assert inspect.signature(load_csm_1b).parameters["decode_weights"].default == "bf16"
