"""``csm_skinny_nt_sel_bf16`` on the device against tests/lora_rows_ref.py: every case of its table in a NaN-filled buffer with
guard rows and guard columns judged whole (guards keep their bits, every unselected element is 0x0000, every selected element
lies within the skinny product's bound AND has the bits ``csm_skinny_nt_bf16`` gives it on the 32-row window of Wt that holds its
column), wild ``sel`` values, and the refusals of the entry point."""
import pytest
import torch

import lora_rows_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _s():
    return torch.cuda.current_stream().cuda_stream


def _launch(lib, c, X, Wt, buf, sel, ldx=None):
    ldo = c.N + c.ldo_pad
    out = buf[R.GR * ldo:]
    return lib.csm_skinny_nt_sel_bf16(X.data_ptr(), Wt.data_ptr(), out.data_ptr(), sel.data_ptr(), c.M, c.N, c.K, c.blk,
                                      ldx if ldx is not None else X.stride(0), c.K, ldo, float(c.alpha), _s())


def _plain_windows(lib, c, X, Wt):
    """[M, N]: csm_skinny_nt_bf16 (N = 32) on every 32-row window of Wt, side by side."""
    full = torch.empty(c.M, c.N, dtype=BF16, device=X.device)
    for w in range(c.N // 32):
        o = torch.empty(c.M, 32, dtype=BF16, device=X.device)
        assert lib.csm_skinny_nt_bf16(X.data_ptr(), Wt[32 * w:32 * w + 32].data_ptr(), o.data_ptr(), c.M, 32, c.K, X.stride(0), c.K, 32,
                                      float(c.alpha), _s()) == 0
        full[:, 32 * w:32 * w + 32] = o
    return full


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_selected_product_against_float64(dev, name):
    from csm.hip import lib
    c = R.CASE[name]
    i = R.inputs(c)
    Xbuf, Wt, sel = i["Xbuf"].to(dev), i["Wt"].to(dev), i["sel"].to(dev)
    X = Xbuf[:, :c.K]
    buf = R.out_buffer(c).to(dev)
    assert _launch(lib, c, X, Wt, buf, sel) == 0, lib.csm_last_error()
    plain = _plain_windows(lib, c, X, Wt)
    torch.cuda.synchronize()
    worst = R.judge_bits(f"gpu.{name}", c, i, buf)
    print(f"RATIO skinny_nt_sel {name} {worst:.4f}")
    assert worst <= 1.0
    keep = R.selected(c, i["sel"])
    got = R.window(c, buf.cpu()).contiguous().view(torch.int16)
    want = plain.cpu().view(torch.int16)
    diff = (got != want) & keep
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} selected elements differ in bits from csm_skinny_nt_bf16"


def test_wild_sel_values_select_nothing(dev):
    """sel is compared, never an index: huge, negative and just-past-the-end values give rows of +0."""
    from csm.hip import lib
    c = R.CASE[next(n for n in R.CASE if n.startswith("each_diff") and R.CASE[n].N == 96)]
    i = R.inputs(c)
    wild = torch.tensor([2 ** 31 - 1, -2 ** 31, 4, 5, 1 << 20, -2, -7, 89478486], dtype=torch.int64)   # (89478486 * 24 wraps to ~48)
    sel = i["sel"].clone()
    rows = torch.arange(0, c.M, max(1, c.M // len(wild)))[:len(wild)]
    sel[rows] = wild[:len(rows)].to(torch.int32)
    buf = R.out_buffer(c).to(dev)
    assert _launch(lib, c, i["Xbuf"].to(dev)[:, :c.K], i["Wt"].to(dev), buf, sel.to(dev)) == 0, lib.csm_last_error()
    torch.cuda.synchronize()
    expect = dict(i, sel=torch.where((sel < 0) | (sel >= c.N // c.blk), torch.full_like(sel, -1), sel))
    assert R.judge_bits("gpu.wild", c, expect, buf) <= 1.0
    assert not bool(R.window(c, buf.cpu())[rows].view(torch.int16).any())


def test_refusals_write_nothing(dev):
    from csm.hip import lib
    c = R.Case("refuse", 33, 256, 64, 16, 4, "const", 1.0, 0, 4)
    i = R.inputs(c)
    X, Wt, sel = i["Xbuf"].to(dev), i["Wt"].to(dev), i["sel"].to(dev)
    buf = R.out_buffer(c).to(dev)
    before = buf.clone()
    ldo = c.N + c.ldo_pad
    o = buf[R.GR * ldo:].data_ptr()
    base = dict(X=X.data_ptr(), Wt=Wt.data_ptr(), out=o, sel=sel.data_ptr(), M=c.M, N=c.N, K=c.K, blk=c.blk, ldx=c.K, ldw=c.K, ldo=ldo)
    broken = [("null X", dict(X=None)), ("null Wt", dict(Wt=None)), ("null out", dict(out=None)), ("null sel", dict(sel=None)),
              ("M=0", dict(M=0)), ("N=16", dict(N=16)), ("N=48", dict(N=48)), ("N=288", dict(N=288, ldo=288)), ("N=0", dict(N=0)),
              ("K=64", dict(K=64)), ("K=192", dict(K=192)), ("K=0", dict(K=0)), ("blk=0", dict(blk=0)), ("blk=12", dict(blk=12)),
              ("blk=-8", dict(blk=-8)), ("ldx&7", dict(ldx=c.K + 4)), ("ldx small", dict(ldx=c.K - 8)), ("ldw&7", dict(ldw=c.K + 4)),
              ("ldw small", dict(ldw=c.K - 8)), ("ldo&3", dict(ldo=ldo + 2)), ("ldo small", dict(ldo=c.N - 4)),
              ("X misaligned", dict(X=X.data_ptr() + 2)), ("Wt misaligned", dict(Wt=Wt.data_ptr() + 8)), ("out misaligned", dict(out=o + 2)),
              ("sel misaligned", dict(sel=sel.data_ptr() + 2))]
    for label, change in broken:
        k = dict(base, **change)
        rc = lib.csm_skinny_nt_sel_bf16(k["X"], k["Wt"], k["out"], k["sel"], k["M"], k["N"], k["K"], k["blk"], k["ldx"], k["ldw"], k["ldo"],
                                        1.0, _s())
        assert rc != 0, f"{label}: accepted"
        assert lib.csm_last_error(), label
    torch.cuda.synchronize()
    assert buf.view(torch.int16).equal(before.view(torch.int16)), "a refused call wrote to the output buffer"
    k = base
    assert lib.csm_skinny_nt_sel_bf16(k["X"], k["Wt"], k["out"], k["sel"], k["M"], k["N"], k["K"], k["blk"], k["ldx"], k["ldw"], k["ldo"], 1.0,
                                      _s()) == 0
    torch.cuda.synchronize()
    assert not buf.view(torch.int16).equal(before.view(torch.int16))


def test_ops_front_end(dev):
    """``ops.skinny_nt_sel`` passes strides and refuses what the kernel does not take - there is no other route."""
    from csm.hip import CsmHipError, ops
    c = R.CASE[next(n for n in R.CASE if n.startswith("runs_mid") and R.CASE[n].N == 64)]
    i = R.inputs(c)
    X, Wt, sel = i["Xbuf"].to(dev)[:, :c.K], i["Wt"].to(dev), i["sel"].to(dev)
    buf = R.out_buffer(c).to(dev)
    ops.skinny_nt_sel(X, Wt, R.window(c, buf), sel, c.blk, alpha=c.alpha)
    torch.cuda.synchronize()
    assert R.judge_bits("gpu.ops", c, i, buf) <= 1.0
    with pytest.raises(CsmHipError, match="blk"):
        ops.skinny_nt_sel(X, Wt, R.window(c, buf), sel, 12)
    with pytest.raises(AssertionError):
        ops.skinny_nt_sel(X, Wt, R.window(c, buf), sel.long(), c.blk)
    with pytest.raises(CsmHipError):
        ops.skinny_nt_sel(X[:, :64].contiguous(), Wt[:, :64].contiguous(), R.window(c, buf), sel, c.blk)      # K = 64: no fall-back
