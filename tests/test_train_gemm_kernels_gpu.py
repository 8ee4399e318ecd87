"""The training GEMM kernels - csm_gemm_bf16, _ex, _rope, _kext, _pinned on the 128 x 128 (register staging and LDS-DMA), the
eight-wave 256 x 256, the four-wave 256 x 256 and the 256 x 192 tile kernels, csm_gemm_bf16_dgrad_wgrad, _two_wgrad,
_multi_wgrad, the split-K route of ops.linear_dw and csm_skinny_nt_bf16 - against the float64 reference of
tests/train_gemm_ref.py (proved by tests/test_train_gemm_ref_cpu.py).  Kernel level only: no model is built.

Every output lives in a buffer of sentinels (guard rows, guard columns, a moved base) and EVERY element of EVERY buffer, the
guards included, is judged by ``train_ops_ref.judge`` against a bound derived in the reference module from the roundings the
kernels perform - never from what the kernels give.  Each judgement prints ``RATIO <kernel> <worst |err| / bound> <case>``; a
ratio above 1 fails.  Each case asserts through csm_gemm_last_kernel() that the intended kernel took it.  The bit-equality
relations between the kernels are asserted next to the judged values, on the same launches."""
import ctypes

import pytest
import torch

import train_gemm_ref as G

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
_refs, _runs = {}, {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from csm.hip import check, lib
    return check, lib


def _ref(c):
    """Inputs and embedded reference of a case: once per data key, shared by the cases and tests that need it, left unchanged."""
    k = c.data_key()
    if k not in _refs:
        i = G.inputs(c)
        _refs[k] = (i, G.embedded_reference(i))
    return _refs[k]


def _strided(t, ld, off=0, gap_rows=1):
    """A device copy of [batch, rows, cols] (or [rows, cols]) with leading dimension ld, its base ``off`` elements into the
    allocation and a row of padding between the batches.  -> (view, batch stride)."""
    t3 = t if t.dim() == 3 else t[None]
    b, r, cdim = t3.shape
    stride = (r + gap_rows) * ld
    buf = torch.zeros(off + b * stride + 16, dtype=t.dtype, device="cuda")
    v = buf.as_strided((b, r, cdim), (stride, ld, 1), off)
    v.copy_(t3)
    return v, stride


class _Switches:
    """The kernel-selecting switches of a case, restored whatever happens."""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        check, lib = _lib()
        check(lib.csm_set_gemm_variant(self.c.variant))
        lib.csm_set_gemm256_persistent(self.c.persistent)
        for k, v in self.c.tuning:
            check(lib.csm_set_gemm_tuning(k, v))

    def __exit__(self, *exc):
        _, lib = _lib()
        lib.csm_set_gemm_variant(2)
        lib.csm_set_gemm256_persistent(1)
        for k, _ in self.c.tuning:
            lib.csm_set_gemm_tuning(k, 1)


def _outputs(c, i):
    """name -> (flat sentinel buffer on the device, its [batch, rows, cols] window), the window preloaded where the launch reads it."""
    out, init = {}, G.initial(i)
    for name, l in G.layouts(c).items():
        buf = G.sentinel_buffer(l).cuda()
        w = G.view(buf, l)
        if name in init:
            w.copy_(init[name].reshape(l.batch, l.rows, l.cols).cuda())
        out[name] = (buf, w)
    return out


def _launch_gemm(c, i, out, lib):
    L = G.layouts(c)["C"]
    A, B = i["A"].cuda(), i["B"].cuda()
    C = out["C"][1]
    lda, ldb = A.shape[-1], B.shape[-1]
    sA, sB = (A[0].numel(), B[0].numel()) if c.batch > 1 else (0, 0)
    pr, ldr, sR, keep = None, 0, 0, []
    if c.R == "alias":
        pr, ldr, sR = C.data_ptr(), L.ld, L.stride
    elif c.R == "sep":
        R, sR = _strided(i["R"].cuda(), c.N + c.ldr_pad, c.off_r)
        pr, ldr = R.data_ptr(), c.N + c.ldr_pad
        keep.append(R)
    sC = L.stride if c.batch > 1 else 0
    sR = sR if c.batch > 1 else 0
    epi, aux_in, aux_out, ld_aux, rc, hd = c.epi, None, None, 0, 0, 0
    if c.epi == 1:
        aux_out, ld_aux = out["act"][1].data_ptr(), G.layouts(c)["act"].ld
    elif c.epi == 2:
        gu, _ = _strided(i["gu"].cuda(), 2 * c.N + c.aux_pad)
        keep.append(gu)
        aux_in, ld_aux = gu.data_ptr(), 2 * c.N + c.aux_pad
    elif c.epi == 3:
        tab = i["table"].cuda()
        keep.append(tab)
        aux_in, ld_aux, rc, hd = tab.data_ptr(), c.S, c.p0, c.hd
    xA, xB = (i["xA"].cuda(), i["xB"].cuda()) if c.kx else (None, None)
    pxa, pxb = (xA.data_ptr(), xB.data_ptr()) if c.kx else (None, None)
    a, b, cp = A.data_ptr(), B.data_ptr(), C.data_ptr()
    if c.route == "plain":
        assert c.epi == 0 and not c.kx
        rc_ = lib.csm_gemm_bf16(a, b, cp, pr, c.M, c.N, c.K, lda, ldb, L.ld, ldr, c.ta, c.tb, c.f32, c.alpha, c.batch, sA, sB, sC, sR, _s())
    elif c.route == "ex":
        assert not c.kx and c.epi in (0, 1, 2)
        rc_ = lib.csm_gemm_bf16_ex(a, b, cp, pr, c.M, c.N, c.K, lda, ldb, L.ld, ldr, c.ta, c.tb, c.f32, c.alpha, c.batch, sA, sB, sC, sR, epi, aux_in,
                                   aux_out, ld_aux, _s())
    elif c.route == "rope":
        assert c.epi == 3 and not c.kx and c.R is None and not c.ta and not c.tb and c.alpha == 1.0
        rc_ = lib.csm_gemm_bf16_rope(a, b, cp, c.M, c.N, c.K, lda, ldb, L.ld, aux_in, c.S, c.p0, c.hd, _s())
    elif c.route == "kext":
        assert c.kx and c.alpha == 1.0 and c.batch == 1 and not c.f32
        rc_ = lib.csm_gemm_bf16_kext(a, b, cp, pr, c.M, c.N, c.K, lda, ldb, L.ld, ldr, c.ta, c.tb, pxa, pxb, c.kx, epi, aux_in, aux_out, ld_aux,
                                     rc, hd, _s())
    else:
        assert c.route == "pinned" and c.batch == 1 and not c.f32
        rc_ = lib.csm_gemm_bf16_pinned(a, b, cp, pr, c.M, c.N, c.K, lda, ldb, L.ld, ldr, c.ta, c.tb, c.alpha, pxa, pxb, c.kx, epi, aux_in, aux_out,
                                       ld_aux, rc, hd, _s())
    torch.cuda.synchronize()
    del keep, xA, xB
    return rc_


def _launch(c, i, out):
    """The case's launch through the C ABI (ops.linear_dw for the split-K route).  -> the kernel name recorded."""
    from csm.hip import ops
    check, lib = _lib()
    d = {k: (v.cuda() if torch.is_tensor(v) else [t.cuda() for t in v]) for k, v in i.items() if k != "c" and k != "table"}
    with _Switches(c):
        if c.kind == "gemm":
            check(_launch_gemm(c, i, out, lib), c.name)
        elif c.kind == "pair":
            Ls = G.layouts(c)
            aux, ld_aux = (d["gu"].data_ptr(), 2 * c.K) if c.epi == 2 else (None, 0)
            check(lib.csm_gemm_bf16_dgrad_wgrad(d["dY"].data_ptr(), d["W"].data_ptr(), out["dX"][1].data_ptr(), d["X"].data_ptr(), out["dW"][1].data_ptr(),
                                                c.M, c.N, c.K, c.N, c.K, Ls["dX"].ld, c.K, Ls["dW"].ld, c.epi, aux, ld_aux, c.acc, c.alpha, _s()), c.name)
        elif c.kind == "wgrads":
            Ls = G.layouts(c)
            n = len(c.probs)
            if c.route == "two":
                a = []
                for k in range(2):
                    a += [d["dY"][k].data_ptr(), d["X"][k].data_ptr(), out[f"dW{k}"][1].data_ptr(), c.probs[k][0], c.probs[k][1], c.probs[k][0],
                          c.probs[k][1], Ls[f"dW{k}"].ld]
                check(lib.csm_gemm_bf16_two_wgrad(*a, c.M, c.acc, c.alpha, _s()), c.name)
            else:
                vp, ip = ctypes.c_void_p * n, ctypes.c_int * n
                check(lib.csm_gemm_bf16_multi_wgrad(n, vp(*[t.data_ptr() for t in d["dY"]]), vp(*[t.data_ptr() for t in d["X"]]),
                                                    vp(*[out[f"dW{k}"][1].data_ptr() for k in range(n)]), ip(*[p[0] for p in c.probs]),
                                                    ip(*[p[1] for p in c.probs]), ip(*[p[0] for p in c.probs]), ip(*[p[1] for p in c.probs]),
                                                    ip(*[Ls[f"dW{k}"].ld for k in range(n)]), c.M, c.acc, c.alpha, _s()), c.name)
        elif c.kind == "splitk":
            w = out["dW"][1][0]
            assert w.is_contiguous()
            ops.linear_dw(d["dY"], d["X"], w, accumulate=bool(c.acc), alpha=c.alpha)
        else:
            X, _ = _strided(d["X"], c.K + c.ldx_pad)
            check(lib.csm_skinny_nt_bf16(X.data_ptr(), d["Wt"].data_ptr(), out["out"][1].data_ptr(), c.M, c.N, c.K, c.K + c.ldx_pad, c.K,
                                         G.layouts(c)["out"].ld, c.alpha, _s()), c.name)
        torch.cuda.synchronize()
        return lib.csm_gemm_last_kernel().decode()


def _run(c):
    """One launch per case: -> (name -> whole buffer on the CPU, kernel name)."""
    if c.name not in _runs:
        i = _ref(c)[0]
        out = _outputs(c, i)
        kernel = _launch(c, i, out)
        _runs[c.name] = ({k: v[0].cpu() for k, v in out.items()}, kernel)
    return _runs[c.name]


def _tag(c):
    k = G.expected_kernel(c)
    return {"skinny": "skinny_nt_kernel", "splitk": "splitk+colsum"}.get(c.kind) or k.split("<")[0] + ("(glds)" if k.endswith("true>") else "")


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case(dev, c):
    if c.branch == "n6":
        assert G.n6_rule(c, 1), "the shape must select the 256 x 192 tile"
    if c.branch == "rounds":
        assert G.tiles256(c.M, c.N) > 256, "the shape must give a persistent workgroup a second tile"
    got, kernel = _run(c)
    want = G.expected_kernel(c)
    if want is not None:
        assert kernel == want, f"{c.name}: ran {kernel}, meant {want}"
    G.judge_case(f"gemm.{c.branch}.{_tag(c)}", c, got, _ref(c)[1])


def _same(a, b, what):
    ga, gb = _run(a)[0], _run(b)[0]
    for name in ga:
        assert torch.equal(ga[name].view(torch.int16 if ga[name].dtype == BF16 else torch.int32),
                           gb[name].view(torch.int16 if gb[name].dtype == BF16 else torch.int32)), f"{what}: {a.name} vs {b.name}: {name} differs"


def _groups(pred):
    """Cases that compute the same thing (one data key, one route) on different kernels."""
    g = {}
    for c in G.CASES:
        if pred(c):
            g.setdefault((c.data_key(), c.route), []).append(c)
    return [v for v in g.values() if len(v) > 1]


def test_four_wave_equals_eight_wave(dev):
    """The same products in the same order on the eight-wave (variant 3) and the four-wave kernel (variant 4): the same bits,
    through every epilogue, with the K-extension, batched, ragged, with a moved base."""
    groups = _groups(lambda c: c.kind == "gemm" and c.variant in (3, 4) and c.persistent == 1 and not c.tuning and c.route != "pinned" and not c.big)
    assert len(groups) >= 50
    for grp in groups:
        assert {c.variant for c in grp} == {3, 4}
        _same(grp[0], grp[1], "four-wave vs eight-wave")


def test_persistent_equals_one_tile_per_workgroup(dev):
    groups = _groups(lambda c: c.branch == "rounds")
    assert groups
    for grp in groups:
        for c in grp[1:]:
            _same(grp[0], c, "persistent / one tile per workgroup / eight- and four-wave")


def test_256x192_tiles_equal_256x256(dev):
    groups = _groups(lambda c: c.branch == "n6")
    assert len(groups) == 8
    for grp in groups:
        assert {_run(c)[1].split("<")[0] for c in grp} == {"gemm256w4n6_kernel", "gemm256w4_kernel"}
        _same(grp[0], grp[1], "256 x 192 vs 256 x 256")


def test_k_extension_routes_agree(dev):
    """tuning(7, 0) sends a K-extension product to the eight-wave kernel: the bits of variant 3."""
    for c in (c for c in G.CASES if c.branch == "kext" and c.tuning):
        _same(c, G.CASE[c.name.replace("v4_t7", "v3")], "K-extension on the eight-wave kernel")


@pytest.mark.parametrize("variant", [1, 3, 4])
def test_zero_extension_equals_plain_product(dev, variant):
    """An all-zero K-extension adds exact zeros: the plain product's bits (csm_gemm_bf16_kext against csm_gemm_bf16)."""
    base = G.Case(f"zero_ext_v{variant}", M=264, N=328, K=128, tb=1, R="sep", ldc_pad=8, variant=variant)
    ext = base.with_(f"zero_ext_v{variant}_kx", kx=64, rank=0, route="kext")
    assert not bool(_ref(ext)[0]["xA"].any()) and not bool(_ref(ext)[0]["xB"].any())
    i = _ref(ext)[0]
    outs = []
    for c in (ext, base):                                         # the plain product on the extension case's operands
        inp = dict(i, c=c)
        out = _outputs(c, inp)
        _launch(c, inp, out)
        outs.append(out["C"][0].cpu())
    G.judge_case(f"gemm.kext.zero_v{variant}", ext, {"C": outs[0]}, _ref(ext)[1])
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("c", [c for c in G.CASES if c.kind == "pair"], ids=lambda c: c.name)
def test_paired_launch_equals_separate_launches(dev, c):
    """dX and dW of the paired launch against the same two products launched alone on the eight-wave kernel."""
    check, lib = _lib()
    i = _ref(c)[0]
    Ls = G.layouts(c)
    out = _outputs(c, i)
    d = {k: i[k].cuda() for k in ("dY", "W", "X")}
    sep = c.with_(c.name + "_sep", variant=3)
    with _Switches(sep):
        gu = i["gu"].cuda() if c.epi == 2 else None
        check(lib.csm_gemm_bf16_ex(d["dY"].data_ptr(), d["W"].data_ptr(), out["dX"][1].data_ptr(), None, c.M, c.K, c.N, c.N, c.K, Ls["dX"].ld, 0, 0, 1,
                                   0, 1.0, 1, 0, 0, 0, 0, c.epi, gu.data_ptr() if c.epi == 2 else None, None, 2 * c.K if c.epi == 2 else 0, _s()), "dX alone")
        assert lib.csm_gemm_last_kernel().decode() == "gemm256p_kernel<0, 1, unsigned short>"
        dw = out["dW"][1]
        check(lib.csm_gemm_bf16(d["dY"].data_ptr(), d["X"].data_ptr(), dw.data_ptr(), dw.data_ptr() if c.acc else None, c.N, c.K, c.M, c.N, c.K,
                                Ls["dW"].ld, Ls["dW"].ld, 1, 1, 0, c.alpha, 1, 0, 0, 0, 0, _s()), "dW alone")
        assert lib.csm_gemm_last_kernel().decode() == "gemm256p_kernel<1, 1, unsigned short>"
        torch.cuda.synchronize()
    got = _run(c)[0]
    for name in ("dX", "dW"):
        assert torch.equal(out[name][0].cpu().view(torch.int16), got[name].view(torch.int16)), f"{c.name}: {name} of the pair differs from the product alone"


def test_multi_launch_equals_two_launch(dev):
    """The tile arithmetic of csm_gemm_bf16_multi_wgrad is csm_gemm_bf16_two_wgrad's: the same two products, the same bits."""
    assert G.CASE["two_w4_a0"].data_key() == G.CASE["multi2"].data_key()
    _same(G.CASE["two_w4_a0"], G.CASE["multi2"], "two against multi")


# ------------------------------------------------------------------------------------------------------------- refusals
class _Arena:
    """Operands of a small valid call of every entry point, and output buffers of sentinels to look at afterwards."""

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        mk = lambda: torch.randn(1 << 16, generator=g).to(BF16).cuda()            # noqa: E731
        self.a, self.b, self.r, self.x, self.aux = mk(), mk(), mk(), mk(), mk()
        self.table = torch.randn(1 << 14, generator=g).cuda()
        self.lay = G.Layout(256, 256, 256, 0, 1, 0, BF16)
        self.outs = [G.sentinel_buffer(self.lay).cuda() for _ in range(3)]
        self.o = [b.data_ptr() + 2 * 256 * G.GR for b in self.outs]               # 16-byte aligned windows inside the guards

    def intact(self):
        torch.cuda.synchronize()
        want = G.sentinel_buffer(self.lay).view(torch.int16)
        return all(torch.equal(b.cpu().view(torch.int16), want) for b in self.outs)


def _refusals(t):
    """(label, entry point, arguments) of calls that must return an error: one broken requirement each, from the CSM_REQUIREs of
    gemm.hip.  The valid base calls are 64 x 64 x 64 (skinny 64 x 32 x 128)."""
    a, b, r, x, aux, tab = (v.data_ptr() for v in (t.a, t.b, t.r, t.x, t.aux, t.table))
    c0, c1, c2 = t.o
    out = []

    def ex(label, **o):
        k = dict(A=a, B=b, C=c0, R=None, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ldr=0, ta=0, tb=0, f32=0, alpha=1.0, batch=1, sA=0, sB=0, sC=0,
                 sR=0, epi=0, aux_in=None, aux_out=None, ld_aux=0)
        k.update(o)
        out.append((f"ex:{label}", "csm_gemm_bf16_ex", [k[n] for n in ("A", "B", "C", "R", "M", "N", "K", "lda", "ldb", "ldc", "ldr", "ta", "tb", "f32", "alpha",
                                                                      "batch", "sA", "sB", "sC", "sR", "epi", "aux_in", "aux_out", "ld_aux")] + [_s()]))

    for lab, o in (("null A", dict(A=None)), ("null B", dict(B=None)), ("null C", dict(C=None)), ("M=0", dict(M=0)), ("N=0", dict(N=0)), ("K=0", dict(K=0)),
                   ("batch=0", dict(batch=0)), ("lda&7", dict(lda=68)), ("ldb&7", dict(ldb=68)), ("A misaligned", dict(A=a + 2)), ("B misaligned", dict(B=b + 8)),
                   ("sA&7", dict(batch=2, sA=4100, sB=4096, sC=8192)), ("sB&7", dict(batch=2, sA=4096, sB=4100, sC=8192)), ("K&7 (A)", dict(K=60)),
                   ("M&7 (transA)", dict(ta=1, M=60)), ("N&7 (transB)", dict(tb=1, N=60)), ("lda<K", dict(lda=56)), ("ldb<K", dict(ldb=56)),
                   ("lda<M (transA)", dict(ta=1, M=72)), ("ldb<N (transB)", dict(tb=1, N=72, ldc=72)), ("ldc<N", dict(ldc=56)),
                   ("epilogue 3 through _ex", dict(epi=3, aux_in=tab, ld_aux=8)), ("epilogue -1", dict(epi=-1)),
                   ("swiglu fwd fp32", dict(epi=1, aux_out=c1, ld_aux=32, f32=1)), ("swiglu fwd null act", dict(epi=1, ld_aux=32)),
                   ("swiglu fwd N&3", dict(epi=1, aux_out=c1, ld_aux=32, N=62)), ("swiglu fwd ldc&3", dict(epi=1, aux_out=c1, ld_aux=32, ldc=66)),
                   ("swiglu fwd ld_aux<N/2", dict(epi=1, aux_out=c1, ld_aux=30)), ("swiglu fwd ld_aux odd", dict(epi=1, aux_out=c1, ld_aux=33)),
                   ("swiglu fwd ldr&3", dict(epi=1, aux_out=c1, ld_aux=32, R=r, ldr=65)), ("swiglu fwd ldr&3 (2)", dict(epi=1, aux_out=c1, ld_aux=32, R=r, ldr=66)),
                   ("swiglu bwd ldc<2N", dict(epi=2, aux_in=aux, ld_aux=128, ldc=120)), ("swiglu bwd null gu", dict(epi=2, ld_aux=128, ldc=128)),
                   ("swiglu bwd ldc&7", dict(epi=2, aux_in=aux, ld_aux=128, ldc=132)), ("swiglu bwd ld_aux&7", dict(epi=2, aux_in=aux, ld_aux=132, ldc=128)),
                   ("swiglu bwd ld_aux<2N", dict(epi=2, aux_in=aux, ld_aux=120, ldc=128)), ("swiglu bwd with R", dict(epi=2, aux_in=aux, ld_aux=128, ldc=128, R=r, ldr=64)),
                   ("swiglu bwd gu misaligned", dict(epi=2, aux_in=aux + 8, ld_aux=128, ldc=128)), ("swiglu bwd C misaligned", dict(epi=2, aux_in=aux, ld_aux=128, ldc=128, C=c0 + 8)),
                   ("swiglu bwd fp32", dict(epi=2, aux_in=aux, ld_aux=128, ldc=128, f32=1)), ("swiglu bwd N&3", dict(epi=2, aux_in=aux, ld_aux=128, ldc=128, tb=0, N=62))):
        ex(lab, **o)

    def rope(label, **o):
        k = dict(A=a, W=b, C=c0, M=64, N=64, K=64, lda=64, ldw=64, ldc=64, table=tab, S=16, p0=32, hd=16)
        k.update(o)
        out.append((f"rope:{label}", "csm_gemm_bf16_rope", [k[n] for n in ("A", "W", "C", "M", "N", "K", "lda", "ldw", "ldc", "table", "S", "p0", "hd")] + [_s()]))

    for lab, o in (("null table", dict(table=None)), ("S=0", dict(S=0)), ("hd<8", dict(hd=4, p0=32)), ("hd&7", dict(hd=12, p0=36)), ("p0<0", dict(p0=-16)),
                   ("p0>N", dict(p0=80)), ("p0%hd", dict(p0=24)), ("N&7", dict(N=60, p0=32)), ("ldc&7", dict(ldc=68)), ("C misaligned", dict(C=c0 + 8)),
                   ("null A", dict(A=None))):
        rope(lab, **o)

    def kext(label, pinned=False, **o):
        k = dict(A=a, B=b, C=c0, R=None, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, ldr=0, ta=0, tb=0, alpha=1.0, xA=x, xB=aux, kx=32, epi=0, aux_in=None,
                 aux_out=None, ld_aux=0, rc=0, hd=0)
        k.update(o)
        if pinned:
            names = ("A", "B", "C", "R", "M", "N", "K", "lda", "ldb", "ldc", "ldr", "ta", "tb", "alpha", "xA", "xB", "kx", "epi", "aux_in", "aux_out", "ld_aux", "rc", "hd")
        else:
            names = ("A", "B", "C", "R", "M", "N", "K", "lda", "ldb", "ldc", "ldr", "ta", "tb", "xA", "xB", "kx", "epi", "aux_in", "aux_out", "ld_aux", "rc", "hd")
        out.append((f"{'pinned' if pinned else 'kext'}:{label}", "csm_gemm_bf16_pinned" if pinned else "csm_gemm_bf16_kext", [k[n] for n in names] + [_s()]))

    ropeargs = dict(epi=3, aux_in=tab, ld_aux=16, rc=32, hd=16)
    for pinned in (False, True):
        for lab, o in (("kx=48", dict(kx=48)), ("kx=288", dict(kx=288)), ("null xA", dict(xA=None)), ("null xB", dict(xB=None)), ("xA misaligned", dict(xA=x + 8)),
                       ("xB misaligned", dict(xB=aux + 2)), ("epilogue 4", dict(epi=4)), ("epilogue -1", dict(epi=-1)), ("rope null table", dict(ropeargs, aux_in=None)),
                       ("rope S=0", dict(ropeargs, ld_aux=0)), ("rope hd&7", dict(ropeargs, hd=12, rc=36)), ("rope p0>N", dict(ropeargs, rc=80)),
                       ("rope p0%hd", dict(ropeargs, rc=24)), ("rope ldc&7", dict(ropeargs, ldc=68)), ("rope C misaligned", dict(ropeargs, C=c0 + 8)),
                       ("rope transB", dict(ropeargs, tb=1)), ("rope ldr&3", dict(ropeargs, R=r, ldr=65)), ("rope transA", dict(ropeargs, ta=1)), ("null A", dict(A=None)), ("K&7", dict(K=60))):
            kext(lab, pinned, **o)
    kext("kx=0", False, kx=0)
    kext("kx=-32", True, kx=-32)

    def skinny(label, **o):
        k = dict(X=a, Wt=b, out=c0, M=64, N=32, K=128, ldx=128, ldw=128, ldo=32, alpha=1.0)
        k.update(o)
        out.append((f"skinny:{label}", "csm_skinny_nt_bf16", [k[n] for n in ("X", "Wt", "out", "M", "N", "K", "ldx", "ldw", "ldo", "alpha")] + [_s()]))

    for lab, o in (("null X", dict(X=None)), ("null Wt", dict(Wt=None)), ("null out", dict(out=None)), ("M=0", dict(M=0)), ("N=48", dict(N=48, ldo=48)),
                   ("K=64", dict(K=64)), ("K=192", dict(K=192, ldx=192, ldw=192)), ("ldx&7", dict(ldx=132)), ("ldw&7", dict(ldw=132)), ("ldo&3", dict(ldo=34)),
                   ("ldx<K", dict(ldx=120)), ("ldw<K", dict(ldw=120)), ("ldo<N", dict(ldo=28)), ("X misaligned", dict(X=a + 8)), ("Wt misaligned", dict(Wt=b + 2)),
                   ("out misaligned", dict(out=c0 + 4))):
        skinny(lab, **o)

    def pair(label, **o):
        k = dict(dY=a, W=b, dX=c0, X=x, dW=c1, M=64, Nout=64, Kin=64, ld_dy=64, ldw=64, ld_dx=64, ldx=64, ld_dw=64, epi=0, aux=None, ld_aux=0, acc=0, alpha=1.0)
        k.update(o)
        out.append((f"pair:{label}", "csm_gemm_bf16_dgrad_wgrad", [k[n] for n in ("dY", "W", "dX", "X", "dW", "M", "Nout", "Kin", "ld_dy", "ldw", "ld_dx", "ldx", "ld_dw",
                                                                                  "epi", "aux", "ld_aux", "acc", "alpha")] + [_s()]))

    sw = dict(epi=2, aux=aux, ld_aux=128, ld_dx=128)
    for lab, o in [(f"null {n}", {n: None}) for n in ("dY", "W", "dX", "X", "dW")] + \
                  [("M=0", dict(M=0)), ("M%64", dict(M=32)), ("Nout%64", dict(Nout=32)), ("Kin&7", dict(Kin=60))] + \
                  [(f"{n}&7", {n: 68}) for n in ("ld_dy", "ldw", "ld_dx", "ldx", "ld_dw")] + \
                  [(f"{n} too small", {n: 56}) for n in ("ld_dy", "ldw", "ld_dx", "ldx", "ld_dw")] + \
                  [(f"{n} misaligned", {n: p + 8}) for n, p in (("dY", a), ("W", b), ("dX", c0), ("X", x), ("dW", c1))] + \
                  [("dx_epilogue 1", dict(epi=1)), ("dx_epilogue 3", dict(epi=3)), ("swiglu null gu", dict(sw, aux=None)), ("swiglu ld_dx<2Kin", dict(sw, ld_dx=120)),
                   ("swiglu ld_aux&7", dict(sw, ld_aux=132)), ("swiglu ld_aux<2Kin", dict(sw, ld_aux=120)), ("swiglu gu misaligned", dict(sw, aux=aux + 8))]:
        pair(lab, **o)

    def two(label, **o):
        k = dict(dY1=a, X1=x, dW1=c0, N1=64, K1=64, ld_dy1=64, ldx1=64, ld_dw1=64, dY2=b, X2=aux, dW2=c1, N2=64, K2=64, ld_dy2=64, ldx2=64, ld_dw2=64, M=64,
                 acc=0, alpha=1.0)
        k.update(o)
        out.append((f"two:{label}", "csm_gemm_bf16_two_wgrad", [k[n] for n in ("dY1", "X1", "dW1", "N1", "K1", "ld_dy1", "ldx1", "ld_dw1", "dY2", "X2", "dW2", "N2", "K2",
                                                                               "ld_dy2", "ldx2", "ld_dw2", "M", "acc", "alpha")] + [_s()]))

    for lab, o in [(f"null {n}", {n: None}) for n in ("dY1", "X1", "dW1", "dY2", "X2", "dW2")] + \
                  [("M=0", dict(M=0)), ("M%64", dict(M=32)), ("N1=0", dict(N1=0)), ("K2=0", dict(K2=0)), ("N2&7", dict(N2=60)), ("K1&7", dict(K1=60))] + \
                  [(f"{n}&7", {n: 68}) for n in ("ld_dy1", "ldx1", "ld_dw1", "ld_dy2", "ldx2", "ld_dw2")] + \
                  [(f"{n} too small", {n: 56}) for n in ("ld_dy1", "ldx1", "ld_dw1", "ld_dy2", "ldx2", "ld_dw2")] + \
                  [(f"{n} misaligned", {n: p + 8}) for n, p in (("dY1", a), ("X1", x), ("dW1", c0), ("dY2", b), ("X2", aux), ("dW2", c1))]:
        two(lab, **o)

    def multi(label, n=2, M=64, arrays=True, **o):
        k = dict(dY=[a, b], X=[x, aux], dW=[c0, c1], N=[64, 64], K=[64, 64], ld_dy=[64, 64], ldx=[64, 64], ld_dw=[64, 64])
        for key, (idx, val) in o.items():
            k[key] = list(k[key])
            k[key][idx] = val
        m = max(n, 2)
        pad = lambda v: (list(v) + [v[-1]] * m)[:m]               # noqa: E731
        vp, ip = ctypes.c_void_p * m, ctypes.c_int * m
        args = [n, vp(*pad(k["dY"])), vp(*pad(k["X"])), vp(*pad(k["dW"])), ip(*pad(k["N"])), ip(*pad(k["K"])), ip(*pad(k["ld_dy"])), ip(*pad(k["ldx"])),
                ip(*pad(k["ld_dw"])), M, 0, 1.0, _s()]
        if not arrays:
            args[3] = None
        out.append((f"multi:{label}", "csm_gemm_bf16_multi_wgrad", args))

    multi("n=0", n=0)
    multi("n=13", n=13)
    multi("null array", arrays=False)
    multi("M=0", M=0)
    multi("M%64", M=32)
    for lab, o in (("null dY", dict(dY=(1, None))), ("null X", dict(X=(0, None))), ("null dW", dict(dW=(1, None))), ("N=0", dict(N=(1, 0))), ("K=0", dict(K=(0, 0))),
                   ("N&7", dict(N=(1, 60))), ("K&7", dict(K=(0, 60))), ("ld_dy&7", dict(ld_dy=(1, 68))), ("ldx&7", dict(ldx=(1, 68))), ("ld_dw&7", dict(ld_dw=(0, 68))),
                   ("ld_dy small", dict(ld_dy=(0, 56))), ("ldx small", dict(ldx=(1, 56))), ("ld_dw small", dict(ld_dw=(1, 56))), ("dY misaligned", dict(dY=(1, b + 8))),
                   ("X misaligned", dict(X=(0, x + 2))), ("dW misaligned", dict(dW=(1, c1 + 8)))):
        multi(lab, **o)
    return out


def test_refused_calls_write_nothing(dev):
    """Every requirement of the GEMM entry points that a caller can break from Python: the call returns its error, the error has a
    text, and no output buffer changes."""
    _, lib = _lib()
    t = _Arena()
    calls = _refusals(t)
    assert len(calls) > 180
    for label, fn, args in calls:
        rc = getattr(lib, fn)(*args)
        assert rc != 0, f"{label}: accepted"
        assert lib.csm_last_error(), label
    assert t.intact(), "a refused call wrote to an output buffer"
    for fn, args in (("csm_set_gemm_variant", (5,)), ("csm_set_gemm_variant", (-1,)), ("csm_set_gemm_tuning", (9, 0)), ("csm_set_gemm_tuning", (-1, 0)),
                     ("csm_set_gemm_tuning", (2, 33)), ("csm_set_gemm_tuning", (3, 20001)), ("csm_set_gemm_tuning", (4, -1))):
        assert getattr(lib, fn)(*args) != 0, (fn, args)
    # the valid base calls themselves are accepted (the refusals above are refused for the one thing each breaks)
    a, b, x, aux = (v.data_ptr() for v in (t.a, t.b, t.x, t.aux))
    assert lib.csm_gemm_bf16_ex(a, b, t.o[0], None, 64, 64, 64, 64, 64, 64, 0, 0, 0, 0, 1.0, 1, 0, 0, 0, 0, 0, None, None, 0, _s()) == 0
    assert lib.csm_gemm_bf16_dgrad_wgrad(a, b, t.o[0], x, t.o[1], 64, 64, 64, 64, 64, 64, 64, 64, 0, None, 0, 0, 1.0, _s()) == 0
    assert lib.csm_skinny_nt_bf16(a, b, t.o[2], 64, 32, 128, 128, 128, 32, 1.0, _s()) == 0
    torch.cuda.synchronize()
    assert not t.intact()


def test_records(dev):
    """The worst utilisation per branch and kernel seen by this file's judgements, for DESIGN.md (runs last)."""
    rows = {}
    for name, u in G.utilisation.items():
        if name.startswith("gemm."):
            key = name.rsplit(".", 1)[0]
            rows[key] = max(rows.get(key, 0.0), u)
    for key in sorted(rows):
        print(f"UTILISATION {key} {rows[key]:.4f}")
    assert rows and max(rows.values()) <= 1.0
