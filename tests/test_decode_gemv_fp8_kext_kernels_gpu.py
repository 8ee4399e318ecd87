"""csm_gemv_fp8w_kext_rows - gemv_fp8_kernel and gemv_fp8_mfma_kernel with the per-row K-extension pack - against the float64
reference of tests/decode_gemv_fp8_kext_ref.py (proved by tests/test_decode_gemv_fp8_kext_ref_cpu.py).  Kernel level only: every
launch goes through the C ABI with the case's own strides and offsets, every output lives in a sentinel buffer and EVERY element
of it, the guards included, is judged (``RATIO <route> <worst |err| / bound> <case>``).  Normalised cases are judged wide and
tight, SwiGLU cases also against the float64 SwiGLU of the bf16 (g, u) the same product leaves without that epilogue, as in
test_decode_gemv_kernels_gpu.py.  The header's three bit-level contracts and the host refusals are asserted on top."""
import pytest
import torch

import decode_gemv_fp8_kext_ref as X
import decode_gemv_ref as D
import train_gemm_ref as G

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
_refs, _devs, _runs, _xhats = {}, {}, {}, {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from csm.hip import check, lib
    return check, lib


def _ref(c):
    """Inputs and the embedded wide reference: once per case, shared, left unchanged."""
    if c.name not in _refs:
        i = X.inputs(c)
        _refs[c.name] = (i, X.embedded(c, *X.reference(i)))
    return _refs[c.name]


def _nan_like(n, dtype):
    if dtype == torch.uint8:
        return torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda")                   # e4m3fn NaN
    return torch.full((n,), 0x7FC0, dtype=torch.int16, device="cuda").view(BF16)


def _strided(t, ld):
    """A device copy of [rows, cols] with leading dimension ld; the padding holds NaN (whatever reads it shows)."""
    r, cdim = t.shape
    assert ld >= cdim
    buf = _nan_like(r * ld + 16, t.dtype)
    v = buf.as_strided((r, cdim), (ld, 1), 0)
    v.copy_(t)
    return v


def _dev(c):
    """The case's operands on the device with the case's strides: once per case."""
    if c.name in _devs:
        return _devs[c.name]
    i = _ref(c)[0]
    st = D.strides(c)
    d = dict(st)
    d["x"] = _strided(i["x"].cuda(), st["ldx"])
    d["W"] = _strided(i["W8"].cuda(), st["ldw"])
    d["scale"] = i["scale"].cuda()
    if c.norm:
        d["nw"] = i["nw"].cuda()
    if c.res:
        d["R"] = i["R"].cuda().contiguous()
    if c.gather:
        d["row_index"] = i["row_index"].cuda()
    d["t"] = _strided(i["t"].cuda(), st["ldt"])
    d["Bx"] = [_strided(b.cuda(), st["ldb"]) for b in i["Bx"]]
    d["bias"] = [None if (not c.bias or i["bias_null"][a]) else i["bias"][a].cuda() for a in range(len(d["Bx"]))]
    d["Bx_tab"] = torch.tensor([b.data_ptr() for b in d["Bx"]], dtype=torch.int64).cuda()
    d["bias_tab"] = torch.tensor([0 if b is None else b.data_ptr() for b in d["bias"]], dtype=torch.int64).cuda() if c.bias else None
    d["row_adapter"] = torch.tensor(D.adapters(c), dtype=torch.int32).cuda()
    _devs[c.name] = d
    return d


def _p(t, off_elems=0):
    return None if t is None else t.data_ptr() + off_elems * t.element_size()


def _call(c, d, y, b0=0, nb=None, ext=True, swiglu=None, res=None, row_adapter=None, ldy=None):
    """Launch rows b0 .. b0 + nb of the case into the window ``y``; ``ext`` False: csm_gemv_fp8w on the same operands."""
    _, lib = _lib()
    nb = c.B - b0 if nb is None else nb
    swiglu = c.swiglu if swiglu is None else swiglu
    res = c.res if res is None else res
    ldy = d["ldy"] if ldy is None else ldy                       # (the (g, u) launch of a SwiGLU case: N columns)
    yp = y.data_ptr() + b0 * ldy * y.element_size()
    if c.gather:
        xp, ri, ro = _p(d["x"]), _p(d["row_index"], b0), D.ROW_OFFSET
    else:
        xp, ri, ro = _p(d["x"], b0 * d["ldx"]), None, 0
    rp = _p(d["R"], b0 * ldy) if res else None
    head = (xp, _p(d["W"]), _p(d["scale"]), yp, rp, nb, c.N, c.K, d["ldw"], d["ldx"], ldy, int(y.dtype == F32), _p(d.get("nw")), D.EPS,
            int(swiglu), ri, ro)
    if not ext:
        return lib.csm_gemv_fp8w(*head, _s())
    ra = d["row_adapter"] if row_adapter is None else row_adapter
    return lib.csm_gemv_fp8w_kext_rows(*head, _p(d["t"], b0 * d["ldt"]), _p(d["Bx_tab"]), _p(d["bias_tab"]), _p(ra, b0), D.N_ADAPTERS, c.kx,
                                       d["ldt"], d["ldb"], _s())


def _launch(c, lay=None, **kw):
    """A fresh sentinel buffer, one launch.  -> (whole buffer on the CPU, kernel name)."""
    check, lib = _lib()
    if lay is not None:
        kw["ldy"] = lay.ld
    lay = lay or D.layout(c)
    buf = G.sentinel_buffer(lay).cuda()
    check(_call(c, _dev(c), G.view(buf, lay)[0], **kw), c.name)
    torch.cuda.synchronize()
    return buf.cpu(), lib.csm_gemv_last_kernel().decode()


def _run(c):
    if c.name not in _runs:
        _runs[c.name] = _launch(c)
    return _runs[c.name]


def _window(c, buf):
    return G.view(buf, D.layout(c))[0]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _xhat(c):
    """ops.rmsnorm_fwd of the case's batch rows: the tight reference's x^ (K above its 4096: the fp32 restatement's, with flips)."""
    if c.name not in _xhats:
        i = _ref(c)[0]
        if c.K > D.RMS_TIGHT_MAX_K:
            _xhats[c.name] = D.xhat32(i)
        else:
            from csm.hip import ops
            x = i["x"][D.x_rows(c, i)].contiguous().cuda()
            y = torch.empty_like(x)
            ops.rmsnorm_fwd(x, i["nw"].cuda(), y, None, eps=D.EPS)
            torch.cuda.synchronize()
            _xhats[c.name] = y.cpu()
    return _xhats[c.name]


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_case(dev, c):
    got, kernel = _run(c)
    want = X.expected_kernel(c)
    assert kernel == want, f"{c.name}: ran {kernel}, meant {want}"
    i, wide = _ref(c)
    route = X.route_of(c)
    D.judge_case(f"dgemv8x.{route}.wide" if c.norm else f"dgemv8x.{route}", c, got, wide)
    if c.fam == "integer":
        assert torch.equal(_window(c, got).double(), X.reference(i)[0]), f"{c.name}: not bit for bit"
    flips = c.K > D.RMS_TIGHT_MAX_K
    if c.norm:
        D.judge_case(f"dgemv8x.{route}.tight", c, got, X.embedded(c, *X.reference(i, xhat=_xhat(c), flips=flips)))
    if c.swiglu:
        # the same launch without the SwiGLU epilogue (and without R): its bf16 (g, u), judged itself, then their float64 SwiGLU
        plain = c.with_(c.name + "_gu", swiglu=0, res=0, tag=c.name)
        pi = dict(i, c=plain)
        lay = D.layout(plain)
        gbuf, gk = _launch(c, lay=lay, swiglu=0, res=0)
        assert gk == X.expected_kernel(plain)
        D.judge_case(f"dgemv8x.{route}.gu", plain, gbuf, X.embedded(plain, *X.reference(pi)))
        if c.norm:
            D.judge_case(f"dgemv8x.{route}.gu.tight", plain, gbuf, X.embedded(plain, *X.reference(pi, xhat=_xhat(c), flips=flips)))
        v, s = D.swiglu_tight(G.view(gbuf, lay)[0], i["R"][:, :c.no] if c.res else None)
        D.judge_case(f"dgemv8x.{route}.swiglu_tight", c, got, X.embedded(c, v, s))


# ------------------------------------------------------------------------------------------------------------- contracts
def test_rows_without_adapter_equal_the_plain_fp8_product(dev):
    """A row with a = -1 or a >= n_adapters is csm_gemv_fp8w's row at the same B, bit for bit; csm_gemv_fp8w keeps its kernel
    names (no ext suffix)."""
    cases = [c for c in X.CASES if any(a < 0 for a in X.live_rows(c))]
    assert len(cases) >= 30 and {X.route_of(c) for c in cases} == set(X.ROUTES)
    n = 0
    for c in cases:
        full = _window(c, _run(c)[0])
        plain, kernel = _launch(c, ext=False)
        assert kernel == D.expected_kernel(c) and "ext" not in kernel
        for b, a in enumerate(X.live_rows(c)):
            if a < 0:
                n += 1
                assert torch.equal(_bits(full[b]), _bits(_window(c, plain)[b])), f"{c.name}: row {b} (adapter {D.adapters(c)[b]})"
    assert n >= 60


def test_all_rows_without_adapter_is_the_plain_launch(dev):
    """Every row at -1: the whole buffer of csm_gemv_fp8w."""
    for c in [c for c in X.CASES if c.fam == "random" and c.K in (1024, 2048)][:8]:
        none = torch.full((c.B,), -1, dtype=torch.int32, device="cuda")
        a, _ = _launch(c, row_adapter=none)
        b, _ = _launch(c, ext=False)
        assert torch.equal(_bits(a), _bits(b)), c.name


def test_rows_equal_the_one_row_launch(dev):
    """B <= 4: row b of a B-row launch is the bits of the one-row launch on that row with its adapter; the one-row launch
    writes nothing else."""
    cases = [c for c in X.CASES if 2 <= c.B <= 4]
    assert len(cases) >= 20
    for c in cases:
        full = _window(c, _run(c)[0])
        for b in range(c.B):
            one, kernel = _launch(c, b0=b, nb=1)
            assert kernel == X.expected_kernel(c.with_("one", B=1)), (c.name, kernel)
            assert torch.equal(_bits(_window(c, one)[b]), _bits(full[b])), f"{c.name}: row {b} differs from its one-row launch"
            _window(c, one)[b] = G.sentinel(one.dtype)
            assert torch.equal(_bits(one), _bits(G.sentinel_buffer(D.layout(c)))), f"{c.name}: the one-row launch wrote outside row {b}"


def test_wide_rows_do_not_depend_on_the_batch(dev):
    """B = 5..16: the last five rows of a 16-row launch launched alone as a batch of five (another B, other positions, other
    batch-mates), and a row of a 5-row launch with its batch-mates' adapters changed, keep their bits."""
    wide = [c for c in X.CASES if c.B == 16]
    assert len(wide) >= 10
    for c in wide:
        full = _window(c, _run(c)[0])
        part, kernel = _launch(c, b0=c.B - 5, nb=5)
        assert kernel == X.expected_kernel(c)
        assert torch.equal(_bits(_window(c, part)[c.B - 5:]), _bits(full[c.B - 5:])), f"{c.name}: rows change with the batch"
    five = [c for c in X.CASES if c.B == 5]
    assert len(five) >= 10
    for c in five:
        full = _window(c, _run(c)[0])
        ad = D.adapters(c)
        for keep in (0, 2, 4):                                   # rows with and without an adapter
            other = [ad[b] if b == keep else ((ad[b] + 1) % D.N_ADAPTERS if ad[b] >= 0 else 0) for b in range(5)]
            got, _ = _launch(c, row_adapter=torch.tensor(other, dtype=torch.int32).cuda())
            assert torch.equal(_bits(_window(c, got)[keep]), _bits(full[keep])), f"{c.name}: row {keep} changes with its batch-mates' adapters"
            assert not torch.equal(_bits(_window(c, got)), _bits(full)), f"{c.name}: the other rows ignore their adapters"


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(dev):
    """Each call is a valid one with exactly one requirement broken: it returns 1 with an error text and no buffer changes; the
    valid call itself is accepted at the end."""
    _, lib = _lib()
    g = torch.Generator().manual_seed(11)
    mk = lambda n: torch.randn(n, generator=g).to(BF16).cuda()    # noqa: E731
    x, nw, t, Bx = mk(17 * 1024), mk(1024), mk(17 * 528), mk(64 * 528)
    W8 = torch.randint(0, 120, (64 * 1024 + 16,), generator=g).to(torch.uint8).cuda()
    scale = torch.rand(64, generator=g).cuda() + 0.5
    lay = G.Layout(17, 64, 64, 0, 1, 0, BF16)
    out = G.sentinel_buffer(lay).cuda()
    y = G.view(out, lay)[0].data_ptr()
    y32buf = G.sentinel_buffer(G.Layout(17, 64, 64, 0, 1, 0, F32)).cuda()
    y32 = G.view(y32buf, G.Layout(17, 64, 64, 0, 1, 0, F32))[0].data_ptr()
    ra = torch.tensor([0, 1, -1, 0] * 5, dtype=torch.int32).cuda()
    Bx_tab = torch.tensor([Bx.data_ptr(), Bx.data_ptr()], dtype=torch.int64).cuda()
    order = ("x", "W", "s", "y", "R", "B", "N", "K", "ldw", "ldx", "ldy", "f32", "nw", "eps", "sw", "ri", "ro", "t", "Bxt", "bt", "ra", "na", "kx", "ldt", "ldb")

    def args(**o):
        k = dict(x=x.data_ptr(), W=W8.data_ptr(), s=scale.data_ptr(), y=y, R=None, B=2, N=64, K=1024, ldw=1024, ldx=1024, ldy=64, f32=0, nw=None,
                 eps=1e-5, sw=0, ri=None, ro=0, t=t.data_ptr(), Bxt=Bx_tab.data_ptr(), bt=None, ra=ra.data_ptr(), na=2, kx=40, ldt=40, ldb=40)
        k.update(o)
        return [k[n] for n in order] + [_s()]

    bad = (("kx=520", dict(kx=520, ldt=520, ldb=520)), ("kx=12", dict(kx=12, ldt=16, ldb=16)), ("kx=0", dict(kx=0)), ("ld_t<kx", dict(ldt=32)),
           ("ld_B<kx", dict(ldb=32)), ("ld_t%8", dict(ldt=44)), ("ld_B%8", dict(ldb=44)), ("t misaligned", dict(t=t.data_ptr() + 2)),
           ("x misaligned", dict(x=x.data_ptr() + 2)), ("W8 misaligned", dict(W=W8.data_ptr() + 8)), ("norm_scale misaligned", dict(nw=nw.data_ptr() + 2)),
           ("B=17", dict(B=17)), ("B=0", dict(B=0)), ("B=17 wide", dict(B=17, K=512)), ("null t", dict(t=None)), ("null Bx table", dict(Bxt=None)),
           ("null row_adapter", dict(ra=None)), ("no adapters", dict(na=0)), ("null scale", dict(s=None)), ("null x", dict(x=None)), ("null y", dict(y=None)),
           ("K%16", dict(K=1016)), ("K>8192", dict(K=8208, ldw=8208, ldx=8208)), ("ldw8%16", dict(ldw=1032)), ("ldw8<K", dict(ldw=1008)),
           ("ldx%8", dict(ldx=1028)), ("swiglu odd N", dict(sw=1, N=63)), ("swiglu fp32", dict(sw=1, f32=1, y=y32)), ("B=5 kx=520", dict(B=5, kx=520, ldt=520, ldb=520)),
           ("B=9 kx=12", dict(B=9, kx=12, ldt=16, ldb=16)), ("B=9 null table", dict(B=9, Bxt=None)))
    want, want32 = out.clone(), y32buf.clone()
    for label, o in bad:
        rc = lib.csm_gemv_fp8w_kext_rows(*args(**o))
        assert rc == 1, f"{label}: returned {rc}"
        assert lib.csm_last_error(), label
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(want.cpu())) and torch.equal(_bits(y32buf.cpu()), _bits(want32.cpu())), "a refused call wrote"
    for B in (2, 9):
        assert lib.csm_gemv_fp8w_kext_rows(*args(B=B)) == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(out.cpu()), _bits(want.cpu()))
    del nw


def test_records(dev):
    """The worst utilisation per route and judgement seen by this file (runs last): the record for DESIGN.md."""
    rows = {k: v for k, v in D.utilisation.items() if k.startswith("dgemv8x.")}
    for key in sorted(rows):
        print(f"UTIL {key} {rows[key]:.4f}")
    assert rows and max(rows.values()) <= 1.0
