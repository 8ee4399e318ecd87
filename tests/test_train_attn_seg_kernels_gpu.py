"""The segment-masked training attention kernels - csm_attn_fwd_seg and csm_attn_bwd_seg (csrc/attention64.hip, the SEG instantiations
of the three second-generation head_dim-64 kernels) - against the float64 reference of tests/train_attn_seg_ref.py (proved by
tests/test_train_attn_seg_ref_cpu.py).  Kernel level only: no model is built.

Every output buffer starts as NaN and EVERY element is judged by ``train_ops_ref.judge`` against the bounds derived there - the
same judge and the same bar (|err| / bound <= 1) as tests/test_train_attn_kernels_gpu.py.  Each judgement prints
``RATIO <kernel> <worst |err| / bound> <case>``."""
import pytest
import torch

import train_attn_ref as A
import train_attn_seg_ref as G

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
_memo = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _lib():
    from csm.hip import check, lib
    return check, lib


def _ref(c):
    """Inputs, descriptor arrays and references of a case, computed once, shared by the tests and left unchanged."""
    if c.name not in _memo:
        i = G.inputs(c)
        f = G.ref_forward(i["qkv"], c)
        out, lse = f.out.to(BF16), f.lse.float()
        ss, se, _ = G.arrays(c)
        _memo[c.name] = dict(i=i, f=f, out=out, lse=lse, ss=ss.cuda(), se=se.cuda(), b=G.ref_backward(i["qkv"], out, lse, i["dout"], c))
    return _memo[c.name]


def _fwd_seg(c, qkv, ss):
    check, lib = _lib()
    out, lse = _nan(c.B * c.S, c.H * c.HD), _nan(c.B, c.H, c.S, dtype=F32)
    check(lib.csm_attn_fwd_seg(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), ss.data_ptr(), c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_fwd_seg")
    return out, lse


def _bwd_seg(c, qkv, out, lse, dout, ss, se):
    check, lib = _lib()
    dqkv, ws = _nan(*qkv.shape), _nan(2, c.B, c.H, c.S, dtype=F32)
    assert ws.numel() * 4 == lib.csm_attn_bwd_workspace_bytes(c.B, c.S, c.H)
    check(lib.csm_attn_bwd_seg(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), ss.data_ptr(),
                               se.data_ptr(), c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_bwd_seg")
    took = lib.csm_attn_last_dkv_kernel()
    return dqkv, ws, took


def _run(c, qkv=None, dout=None):
    """Forward, then the backward of the reference's own out and lse.  -> out, lse, dqkv, ws (on the device)."""
    r = _ref(c)
    qkv = r["i"]["qkv"].cuda() if qkv is None else qkv
    dout = r["i"]["dout"].cuda() if dout is None else dout
    out, lse = _fwd_seg(c, qkv, r["ss"])
    dqkv, ws, took = _bwd_seg(c, qkv, r["out"].cuda(), r["lse"].cuda(), dout, r["ss"], r["se"])
    assert took == 0, "the segment backward always takes the compiler-scheduled dQ and dK/dV kernels"
    return out, lse, dqkv, ws


@pytest.mark.parametrize("c", G.CASES, ids=[c.name for c in G.CASES])
def test_bounds(dev, c):
    """Forward (out, lse) and backward (dQ, dK, dV, -delta and -lse log2(e) as published for the dK/dV pass), isolated and chained."""
    r = _ref(c)
    out, lse, dqkv, ws = _run(c)
    ws = ws.cpu()
    A.judge_forward("attn.seg_fwd", out, lse, r["f"], c.name)
    A.judge_backward("attn.seg_bwd", dqkv, -ws[0], r["b"], c, f"{c.name} isolated")
    ref = -r["lse"].double() * float(torch.tensor(A.LOG2E32, dtype=F32))
    A.judge("attn.seg_bwd.nlse2", ws[1], ref, 2 * A.U * ref.abs())
    # in a chain: the kernel's own out and lse, against the reference backward of those
    dq2, ws2, _ = _bwd_seg(c, r["i"]["qkv"].cuda(), out, lse, r["i"]["dout"].cuda(), r["ss"], r["se"])
    A.judge_backward("attn.seg_bwd.chain", dq2, -ws2.cpu()[0], G.ref_backward(r["i"]["qkv"], out.cpu(), lse.cpu(), r["i"]["dout"], c), c, f"{c.name} chained")


@pytest.mark.parametrize("c", G.SINGLE, ids=[c.name for c in G.SINGLE])
def test_one_segment_gives_the_bits_of_the_unsegmented_kernels(dev, c):
    check, lib = _lib()
    r = _ref(c)
    qkv, dout = r["i"]["qkv"].cuda(), r["i"]["dout"].cuda()
    out, lse, dqkv, ws = _run(c)
    o0, l0 = _nan(c.B * c.S, c.H * c.HD), _nan(c.B, c.H, c.S, dtype=F32)
    check(lib.csm_attn_fwd(qkv.data_ptr(), o0.data_ptr(), l0.data_ptr(), c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_fwd")
    assert torch.equal(out.view(torch.int16), o0.view(torch.int16)) and torch.equal(lse.view(torch.int32), l0.view(torch.int32))
    d0, w0 = _nan(*qkv.shape), _nan(2, c.B, c.H, c.S, dtype=F32)
    try:
        lib.csm_set_attn_variant(A.DEFAULT_WORD | 1 << 10)
        check(lib.csm_attn_bwd(qkv.data_ptr(), r["out"].cuda().data_ptr(), dout.data_ptr(), r["lse"].cuda().data_ptr(), d0.data_ptr(), w0.data_ptr(),
                               c.B, c.S, c.H, c.KV, c.HD, _s()), "csm_attn_bwd")
        assert lib.csm_attn_last_dkv_kernel() == 0
    finally:
        lib.csm_set_attn_variant(0)
    assert torch.equal(dqkv.view(torch.int16), d0.view(torch.int16)) and torch.equal(ws.view(torch.int32), w0.view(torch.int32))


def test_segments_do_not_see_each_other(dev):
    """[63, 65, 127, 129]: other finite data in the qkv and dout rows of the second segment leaves every bit of the other
    segments' out, lse, dQ, dK and dV as it was."""
    c = next(c for c in G.CASES if c.layouts == ((63, 65, 127, 129),))
    r = _ref(c)
    base = _run(c)
    qkv, dout = r["i"]["qkv"].clone(), r["i"]["dout"].clone()
    g = A.seeded(63, 65)
    qkv[63:128] = (torch.randn(65, qkv.shape[1], generator=g) * 3).to(BF16)
    dout[63:128] = (torch.randn(65, dout.shape[1], generator=g) * 3).to(BF16)
    # (the backward takes the reference's out and lse: those of the other segments do not depend on the second one either)
    other = _run(c, qkv.cuda(), dout.cuda())
    keep = torch.ones(c.S, dtype=torch.bool, device="cuda")
    keep[63:128] = False
    assert not torch.equal(base[0][~keep].view(torch.int16), other[0][~keep].view(torch.int16)), "the second segment itself did change"
    assert torch.equal(base[0][keep].view(torch.int16), other[0][keep].view(torch.int16)), "out"
    assert torch.equal(base[1][:, :, keep].view(torch.int32), other[1][:, :, keep].view(torch.int32)), "lse"
    assert torch.equal(base[2][keep].view(torch.int16), other[2][keep].view(torch.int16)), "dQ | dK | dV"


@pytest.mark.parametrize("c", [G.CASES[5], G.CASES[9], G.CASES[-2]], ids=[G.CASES[5].name, G.CASES[9].name, G.CASES[-2].name])
def test_two_runs_give_the_same_bits(dev, c):
    a, b = _run(c), _run(c)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int16), b[2].view(torch.int16)) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


def test_dispatch_and_refusals(dev):
    """After a segment backward csm_attn_last_dkv_kernel() answers 0 - also for a shape the asm dK/dV kernel takes unsegmented
    (S % 64 == 0, 4 query heads per kv head).  head_dim 128, a bad shape and a null descriptor are refused and launch nothing."""
    _, lib = _lib()
    c = next(c for c in G.CASES if c.layouts == ((128, 128, 128),))._replace(H=4, KV=1)
    qkv, dout = torch.randn(c.S, 6 * 64, device="cuda").to(BF16), torch.randn(c.S, 4 * 64, device="cuda").to(BF16)
    ss, se, _ = G.arrays(c)
    ss, se = ss.cuda(), se.cuda()
    out, lse = _fwd_seg(c, qkv, ss)
    d0, w0 = _nan(*qkv.shape), _nan(2, c.B, c.H, c.S, dtype=F32)
    assert lib.csm_attn_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), d0.data_ptr(), w0.data_ptr(), c.B, c.S, c.H, c.KV, 64, _s()) == 0
    assert lib.csm_attn_last_dkv_kernel() == 1                     # the unsegmented backward of this shape does take the asm loop
    assert _bwd_seg(c, qkv, out, lse, dout, ss, se)[2] == 0
    o, l, d, w = _nan(c.S, 4 * 64), _nan(1, 4, c.S, dtype=F32), _nan(*qkv.shape), _nan(2, 1, 4, c.S, dtype=F32)

    def fwd(S=c.S, HD=64, seg=ss.data_ptr()):
        return lib.csm_attn_fwd_seg(qkv.data_ptr(), o.data_ptr(), l.data_ptr(), seg, 1, S, 4, 1, HD, _s())

    def bwd(S=c.S, HD=64, seg=ss.data_ptr(), end=se.data_ptr()):
        return lib.csm_attn_bwd_seg(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), d.data_ptr(), w.data_ptr(), seg, end, 1, S, 4, 1, HD, _s())

    for call, kw, text in ((fwd, dict(HD=128), b"csm_attn_fwd_seg: head_dim 128 unsupported (64)"), (bwd, dict(HD=128), b"csm_attn_bwd_seg: head_dim 128 unsupported (64)"),
                           (fwd, dict(S=0), b"csm_attn_fwd_seg: bad shape"), (bwd, dict(S=0), b"csm_attn_bwd_seg: bad shape"),
                           (fwd, dict(seg=None), b"csm_attn_fwd_seg: null pointer"), (bwd, dict(end=None), b"csm_attn_bwd_seg: null pointer")):
        rc = call(**kw)
        assert rc == 1 and text in lib.csm_last_error(), (rc, lib.csm_last_error())
    torch.cuda.synchronize()
    for t in (o, l, d, w):
        assert bool(torch.isnan(t).all()), "a refused call launched something"
