"""The decode-step product kernels - csm_gemv_bf16, _ex, _kext, _kext_rows on gemv_reg_kernel, gemv_regn_kernel, gemv_kernel and
gemv_mfma_kernel, csm_gemv_fp8w on gemv_fp8_kernel and gemv_fp8_mfma_kernel, csm_gemv_t_bf16, csm_lora_project_bf16 and
_rows_bf16 - against the float64 reference of tests/decode_gemv_ref.py (proved by tests/test_decode_gemv_ref_cpu.py).  Kernel
level only: no model is built, every launch goes through the C ABI with the case's own strides and offsets.

Every output lives in a buffer of sentinels (guard rows, guard columns, a moved base) and EVERY element of the buffer, the guards
included, is judged by ``train_ops_ref.judge`` against a bound derived in the reference module from the roundings the kernels
perform - never from what the kernels give.  Each judgement prints ``RATIO <route> <worst |err| / bound> <case>``; a ratio above
1 fails.  Normalised cases are judged twice: wide (x^ from float64) and tight (x^ = ops.rmsnorm_fwd's bf16 output of the same
rows); SwiGLU cases also against the float64 SwiGLU of the bf16 (g, u) the same product leaves without that epilogue.  Each
case asserts through csm_gemv_last_kernel() that the intended kernel took it.  The bit-equalities the header promises are
asserted on the same launches."""
import pytest
import torch

import decode_gemv_ref as D
import train_gemm_ref as G

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
TUNING_DEFAULT = {0: 1, 1: 1, 2: 1, 3: 1, 4: 0}
_refs, _devs, _runs, _xhats = {}, {}, {}, {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from csm.hip import check, lib
    return check, lib


class _Tuning:
    """The csm_set_decode_tuning keys of a case, restored whatever happens."""

    def __init__(self, tuning):
        self.tuning = tuning

    def __enter__(self):
        check, lib = _lib()
        for k, v in self.tuning:
            check(lib.csm_set_decode_tuning(k, v))

    def __exit__(self, *exc):
        _, lib = _lib()
        for k, _ in self.tuning:
            lib.csm_set_decode_tuning(k, TUNING_DEFAULT[k])


def _ref(c):
    """Inputs and the embedded wide reference: once per data key, shared, left unchanged."""
    k = c.data_key()
    if k not in _refs:
        i = D.inputs(c)
        _refs[k] = (i, D.embedded(c, *D.reference(i)))
    return _refs[k]


def _nan_like(n, dtype):
    if dtype == torch.uint8:
        return torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda")                   # e4m3fn NaN
    if dtype == BF16:
        return torch.full((n,), 0x7FC0, dtype=torch.int16, device="cuda").view(BF16)
    return torch.zeros(n, dtype=dtype, device="cuda")


def _strided(t, ld):
    """A device copy of [rows, cols] with leading dimension ld; the padding holds NaN (whatever reads it shows)."""
    r, cdim = t.shape
    assert ld >= cdim
    buf = _nan_like(r * ld + 16, t.dtype)
    v = buf.as_strided((r, cdim), (ld, 1), 0)
    v.copy_(t)
    return v


def _dev(c):
    """The case's operands on the device, laid out with the case's strides: once per data key."""
    k = c.data_key()
    if k in _devs:
        return _devs[k]
    i = _ref(c)[0]
    st = D.strides(c)
    d = dict(st)
    d["x"] = _strided(i["x"].cuda(), st["ldx"])
    if c.kind == "fp8":
        d["W"] = _strided(i["W8"].cuda(), st["ldw"])
        d["scale"] = i["scale"].cuda()
    elif c.kind in ("proj", "proj_rows"):
        d["At"] = [_strided(a.cuda(), st["lda"]) for a in i["W"]]
        d["At_tab"] = torch.tensor([a.data_ptr() for a in d["At"]], dtype=torch.int64).cuda()
        if c.kind == "proj_rows":
            d["pscale"] = i["pscale"].cuda()
    else:
        d["W"] = _strided(i["W"].cuda(), st["ldw"])
    if c.norm:
        d["nw"] = i["nw"].cuda()
    if c.res:
        d["R"] = i["R"].cuda().contiguous()                       # [B][ldy], the padding columns random: R shares ldy with y
    if c.gather:
        d["row_index"] = i["row_index"].cuda()
    if c.ext:
        d["t"] = _strided(i["t"].cuda(), st["ldt"])
        d["Bx"] = [_strided(b.cuda(), st["ldb"]) for b in i["Bx"]]
        d["bias"] = [None if (not c.bias or i["bias_null"][a]) else i["bias"][a].cuda() for a in range(len(d["Bx"]))]
        if c.ext == 2:
            d["Bx_tab"] = torch.tensor([b.data_ptr() for b in d["Bx"]], dtype=torch.int64).cuda()
            d["bias_tab"] = torch.tensor([0 if b is None else b.data_ptr() for b in d["bias"]], dtype=torch.int64).cuda() if c.bias else None
    if c.ext == 2 or c.kind == "proj_rows":
        d["row_adapter"] = torch.tensor(D.adapters(c), dtype=torch.int32).cuda()
    _devs[k] = d
    return d


def _p(t, off_elems=0):
    return None if t is None else t.data_ptr() + off_elems * t.element_size()


def _call(c, d, y, b0=0, nb=None, ext=None, adapter=None):
    """Launch rows b0 .. b0 + nb of the case into the window ``y`` ([B, cols] view of a sentinel buffer; the rows keep their
    places).  ``ext``: the extension kind to launch with (default: the case's); ``adapter``: with ext = 1 on a per-row case, or
    csm_lora_project_bf16 on a rows case, the one adapter to use.  -> the return code."""
    _, lib = _lib()
    nb = c.B - b0 if nb is None else nb
    ext = c.ext if ext is None else ext
    ldy = d["ldy"]
    yp = y.data_ptr() + b0 * ldy * y.element_size()
    f32 = int(y.dtype == F32)
    if c.kind in ("proj", "proj_rows"):
        xp = _p(d["x"], b0 * d["ldx"])
        nw = _p(d.get("nw"))
        if c.kind == "proj" or adapter is not None:
            a = 0 if adapter is None else adapter
            sc = D.PROJ_SCALE if c.kind == "proj" else float(_ref(c)[0]["pscale"][a])
            return lib.csm_lora_project_bf16(xp, _p(d["At"][a]), yp, nb, c.K, c.kx, d["ldx"], d["lda"], ldy, sc, nw, D.EPS, _s())
        return lib.csm_lora_project_rows_bf16(xp, _p(d["At_tab"]), yp, _p(d["row_adapter"], b0), _p(d["pscale"]), D.N_ADAPTERS, nb, c.K, c.kx,
                                              d["ldx"], d["lda"], ldy, nw, D.EPS, _s())
    if c.kind == "gemv_t":
        return lib.csm_gemv_t_bf16(_p(d["x"], b0 * d["ldx"]), _p(d["W"]), yp, nb, c.N, c.K, d["ldw"], d["ldx"], ldy, f32, _s())
    if c.gather:
        xp, ri, ro = _p(d["x"]), _p(d["row_index"], b0), D.ROW_OFFSET
    else:
        xp, ri, ro = _p(d["x"], b0 * d["ldx"]), None, 0
    rp = _p(d["R"], b0 * ldy) if c.res else None
    nw = _p(d.get("nw"))
    base = (xp, _p(d["W"]))
    tail = (rp, nb, c.N, c.K, d["ldw"], d["ldx"], ldy, f32)
    fus = (nw, D.EPS, int(c.swiglu), ri, ro)
    if c.kind == "fp8":
        return lib.csm_gemv_fp8w(xp, _p(d["W"]), _p(d["scale"]), yp, *tail, *fus, _s())
    if ext == 0:
        if not (c.norm or c.swiglu or c.gather):
            return lib.csm_gemv_bf16(*base, yp, *tail, _s())
        return lib.csm_gemv_bf16_ex(*base, yp, *tail, *fus, _s())
    tp = _p(d["t"], b0 * d["ldt"])
    if ext == 1:
        a = 0 if adapter is None else adapter
        return lib.csm_gemv_bf16_kext(*base, yp, *tail, *fus, tp, _p(d["Bx"][a]), c.kx, d["ldt"], d["ldb"], _p(d["bias"][a]), _s())
    return lib.csm_gemv_bf16_kext_rows(*base, yp, *tail, *fus, tp, _p(d["Bx_tab"]), _p(d["bias_tab"]), _p(d["row_adapter"], b0), D.N_ADAPTERS,
                                       c.kx, d["ldt"], d["ldb"], _s())


def _launch(c, **kw):
    """A fresh sentinel buffer, one launch under the case's tuning keys.  -> (whole buffer on the CPU, kernel name)."""
    check, lib = _lib()
    l = D.layout(c)
    buf = G.sentinel_buffer(l).cuda()
    with _Tuning(c.tuning):
        check(_call(c, _dev(c), G.view(buf, l)[0], **kw), c.name)
        torch.cuda.synchronize()
        kernel = lib.csm_gemv_last_kernel().decode()
    return buf.cpu(), kernel


def _run(c):
    """The case's own launch: once."""
    if c.name not in _runs:
        _runs[c.name] = _launch(c)
    return _runs[c.name]


def _window(c, buf):
    return G.view(buf, D.layout(c))[0]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _xhat(c):
    """ops.rmsnorm_fwd of the case's batch rows (bf16 [B, K] on the CPU): the tight reference's x^.  K above rmsnorm_fwd's 4096:
    the fp32 restatement's on the CPU (judged with ``flips``)."""
    k = c.data_key()
    if k not in _xhats and c.K > D.RMS_TIGHT_MAX_K:
        _xhats[k] = D.xhat32(_ref(c)[0])
    if k not in _xhats:
        from csm.hip import ops
        i = _ref(c)[0]
        x = i["x"][D.x_rows(c, i)].contiguous().cuda()
        y = torch.empty_like(x)
        ops.rmsnorm_fwd(x, i["nw"].cuda(), y, None, eps=D.EPS)
        torch.cuda.synchronize()
        _xhats[k] = y.cpu()
    return _xhats[k]


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_case(dev, c):
    got, kernel = _run(c)
    want = D.expected_kernel(c)
    assert kernel == want, f"{c.name}: ran {kernel}, meant {want}"
    i, wide = _ref(c)
    route = D.route_of(c)
    D.judge_case(f"dgemv.{route}.wide" if c.norm else f"dgemv.{route}", c, got, wide)
    if c.norm:
        xh = _xhat(c)
        D.judge_case(f"dgemv.{route}.tight", c, got, D.embedded(c, *D.reference(i, xhat=xh, flips=c.K > D.RMS_TIGHT_MAX_K)))
    if c.swiglu:
        # the same product without the SwiGLU epilogue (and without R): its bf16 (g, u), judged itself, then their float64 SwiGLU
        plain = c.with_(c.name + "_gu", swiglu=0, res=0, tag=c.name)
        pi = dict(i, c=plain)
        _refs.setdefault(plain.data_key(), (pi, D.embedded(plain, *D.reference(pi))))
        gbuf, _ = _run(plain)
        D.judge_case(f"dgemv.{D.route_of(plain)}.gu", plain, gbuf, _refs[plain.data_key()][1])
        if c.norm:
            D.judge_case(f"dgemv.{D.route_of(plain)}.gu.tight", plain, gbuf, D.embedded(plain, *D.reference(pi, xhat=_xhat(c), flips=c.K > D.RMS_TIGHT_MAX_K)))
        v, s = D.swiglu_tight(_window(plain, gbuf), i["R"][:, :c.no] if c.res else None)
        D.judge_case(f"dgemv.{route}.swiglu_tight", c, got, D.embedded(c, v, s))


# ------------------------------------------------------------------------------------------------------------- bit-equalities
def _small(pred):
    return [c for c in D.CASES if not c.big and pred(c)]


def test_rows_equal_the_one_row_launch(dev):
    """B <= 4 (VALU kernels, FP8 included, the K-extensions, lora_project): row b is the bits of a one-row launch on that row."""
    cases = _small(lambda c: 2 <= c.B <= 4 and not c.mfma and c.kind in ("gemv", "fp8", "proj"))
    assert len(cases) > 150
    for c in cases:
        full = _window(c, _run(c)[0])
        for b in range(c.B):
            one, kernel = _launch(c, b0=b, nb=1)
            assert kernel.split("<")[0] == D.route_of(c.with_("one", B=1)), (c.name, kernel)
            assert torch.equal(_bits(_window(c, one)[b]), _bits(full[b])), f"{c.name}: row {b} differs from its one-row launch ({kernel})"
            _window(c, one)[b] = G.sentinel(one.dtype)
            assert torch.equal(_bits(one), _bits(G.sentinel_buffer(D.layout(c)))), f"{c.name}: the one-row launch wrote outside row {b}"


def test_wide_rows_do_not_depend_on_the_batch(dev):
    """B = 5..16 (MFMA kernels, bf16 / FP8 / per-row extension): the last five rows launched alone as a batch of five - another
    B, other positions, other batch-mates - keep their bits."""
    cases = _small(lambda c: c.B >= 9 and c.kind in ("gemv", "fp8"))
    assert len(cases) > 60
    for c in cases:
        full = _window(c, _run(c)[0])
        part, kernel = _launch(c, b0=c.B - 5, nb=5)
        assert kernel.split("<")[0] == D.route_of(c)
        assert torch.equal(_bits(_window(c, part)[c.B - 5:]), _bits(full[c.B - 5:])), f"{c.name}: rows change with the batch"


def test_zero_extension_equals_plain_product(dev):
    """ext_B all zeros, no bias: csm_gemv_bf16_kext leaves csm_gemv_bf16_ex's bits."""
    cases = _small(lambda c: c.ext == 1 and c.fam == "random")
    assert len(cases) >= 20
    for c in cases:
        d = dict(_dev(c))
        d["Bx"] = [torch.zeros_like(d["Bx"][0].as_strided((c.N * d["ldb"],), (1,)))]
        d["bias"] = [None]
        check, lib = _lib()
        outs = []
        for ext in (1, 0):
            buf = G.sentinel_buffer(D.layout(c)).cuda()
            with _Tuning(c.tuning):
                check(_call(c, d, _window(c, buf), ext=ext), c.name)
            torch.cuda.synchronize()
            assert lib.csm_gemv_last_kernel().decode().endswith(f"ext{ext}>")
            outs.append(buf.cpu())
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), c.name


def test_rows_without_adapter_equal_plain_product(dev):
    """csm_gemv_bf16_kext_rows: a row whose adapter is -1 or out of range is csm_gemv_bf16_ex's row at the same B."""
    cases = _small(lambda c: c.ext == 2 and any(D.live_adapter(a) < 0 for a in D.adapters(c)))
    assert len(cases) >= 30
    for c in cases:
        full = _window(c, _run(c)[0])
        plain, kernel = _launch(c, ext=0)
        assert kernel == D.expected_kernel(c).replace("ext2", "ext0")
        for b, a in enumerate(D.adapters(c)):
            if D.live_adapter(a) < 0:
                assert torch.equal(_bits(full[b]), _bits(_window(c, plain)[b])), f"{c.name}: row {b} (adapter {a})"


def test_kext_rows_equal_one_row_kext(dev):
    """B <= 4: row b of csm_gemv_bf16_kext_rows is a one-row csm_gemv_bf16_kext with that row's adapter (and its bias or none)."""
    cases = _small(lambda c: c.ext == 2 and c.B <= 4)
    assert len(cases) >= 30
    n = 0
    for c in cases:
        full = _window(c, _run(c)[0])
        for b, a in enumerate(D.adapters(c)):
            if D.live_adapter(a) >= 0:
                one, kernel = _launch(c, b0=b, nb=1, ext=1, adapter=a)
                assert kernel.endswith("ext1>")
                assert torch.equal(_bits(_window(c, one)[b]), _bits(full[b])), f"{c.name}: row {b} (adapter {a})"
                n += 1
    assert n >= 30


def test_project_rows_equal_one_row_project(dev):
    cases = _small(lambda c: c.kind == "proj_rows")
    n = 0
    for c in cases:
        full = _window(c, _run(c)[0])
        for b, a in enumerate(D.adapters(c)):
            if D.live_adapter(a) >= 0:
                one, kernel = _launch(c, b0=b, nb=1, adapter=a)
                assert kernel == "lora_project_kernel<1>"
                assert torch.equal(_bits(_window(c, one)[b]), _bits(full[b])), f"{c.name}: row {b} (adapter {a})"
                n += 1
            else:
                assert not bool(_bits(full[b]).any()), f"{c.name}: row {b} without adapter is not +0"
    assert n >= 40


def _twins(suffix):
    return [(D.CASE[c.name[:-len(suffix)]], c) for c in D.CASES if c.name.endswith(suffix)]


def test_register_kernels_equal_the_lds_kernel(dev):
    """Keys 0 / 3 off send the K = 1024 / 2048 products to gemv_kernel: the bits of gemv_reg_kernel / gemv_regn_kernel."""
    pairs = _twins("_lds")
    assert len(pairs) >= 40
    for a, b in pairs:
        assert _run(a)[1].startswith(("gemv_reg_kernel", "gemv_regn_kernel")) and _run(b)[1].startswith("gemv_kernel<")
        assert torch.equal(_bits(_run(a)[0]), _bits(_run(b)[0])), a.name


def test_nontemporal_loads_change_nothing(dev):
    """Key 1 off on every K = 2048 case (reg, regn, MFMA): the other instantiation, the same bits."""
    pairs = _twins("_nt0")
    assert len(pairs) >= 20
    for a, b in pairs:
        ka, kb = _run(a)[1], _run(b)[1]
        assert ka != kb and ka.split("<")[0] == kb.split("<")[0], (ka, kb)
        assert torch.equal(_bits(_run(a)[0]), _bits(_run(b)[0])), a.name


def test_pairs_per_wave_change_nothing(dev):
    """Key 2: one, two and four gate / up pairs per wave give the same bits (2050 outputs: a tail in the last wave of either)."""
    one = _run(D.CASE["reg_rpw1"])
    for r in (2, 4):
        got = _run(D.CASE[f"reg_rpw{r}"])
        assert got[1] == f"gemv_reg_kernel<2, bf16, 1, 0, {r}, ext0>" and one[1] == "gemv_reg_kernel<2, bf16, 1, 0, 1, ext0>"
        assert torch.equal(_bits(got[0]), _bits(one[0])), r


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refused_calls_write_nothing(dev):
    """Arguments the entry points refuse: the call returns 1, the error has a text, no output buffer changes.  Every call below
    is a valid call with exactly one requirement broken (the valid calls themselves are accepted at the end)."""
    _, lib = _lib()
    g = torch.Generator().manual_seed(7)
    mk = lambda n: torch.randn(n, generator=g).to(BF16).cuda()    # noqa: E731
    x, W, R, nw, t, Bx, bias = mk(16 * 1024), mk(64 * 1024), mk(16 * 64), mk(1024), mk(16 * 512), mk(64 * 512), mk(64)
    W8 = torch.randint(0, 120, (64 * 1024,), generator=g).to(torch.uint8).cuda()
    scale = torch.rand(64, generator=g).cuda() + 0.5
    lay = G.Layout(16, 64, 64, 0, 1, 0, BF16)
    outs = [G.sentinel_buffer(lay).cuda() for _ in range(2)]
    y = outs[0].data_ptr() + 2 * 64 * G.GR
    y32buf = G.sentinel_buffer(G.Layout(16, 64, 64, 0, 1, 0, F32)).cuda()
    outs.append(y32buf)
    y32 = y32buf.data_ptr() + 4 * 64 * G.GR
    ra = torch.tensor([0, 1, -1, 0] * 4, dtype=torch.int32).cuda()
    Bx_tab = torch.tensor([Bx.data_ptr(), Bx.data_ptr()], dtype=torch.int64).cuda()
    At_tab = torch.tensor([W.data_ptr(), W.data_ptr()], dtype=torch.int64).cuda()             # At [K][lda]: 1024 x 40 elements of W
    pscale = torch.ones(2).cuda()
    xp, Wp, tp, Bp = x.data_ptr(), W.data_ptr(), t.data_ptr(), Bx.data_ptr()
    calls = []

    def ex(label, **o):
        k = dict(x=xp, W=Wp, y=y, R=None, B=2, N=64, K=1024, ldw=1024, ldx=1024, ldy=64, f32=0, nw=None, eps=1e-5, sw=0, ri=None, ro=0)
        k.update(o)
        calls.append((f"ex:{label}", "csm_gemv_bf16_ex", [k[n] for n in ("x", "W", "y", "R", "B", "N", "K", "ldw", "ldx", "ldy", "f32", "nw", "eps", "sw", "ri", "ro")] + [_s()]))

    for lab, o in (("B=0", dict(B=0)), ("B=17", dict(B=17)), ("K%8", dict(K=1020)), ("K%32 at B=5", dict(B=5, K=1000, ldw=1000, ldx=1000)),
                   ("K%32 at B=16", dict(B=16, K=1016)), ("swiglu odd N", dict(sw=1, N=63)), ("swiglu fp32", dict(sw=1, f32=1, y=y32)),
                   ("swiglu odd N, B=9", dict(sw=1, N=63, B=9)), ("ldw%8", dict(ldw=1028)), ("ldx%8", dict(ldx=1028)), ("null x", dict(x=None)),
                   ("null W", dict(W=None)), ("null y", dict(y=None)), ("N=0", dict(N=0)), ("K=0", dict(K=0)), ("B*K beyond the LDS copy", dict(B=4, K=8200, ldw=8200, ldx=8200))):
        ex(lab, **o)
    calls.append(("gemv:B=17", "csm_gemv_bf16", [xp, Wp, y, None, 17, 64, 1024, 1024, 1024, 64, 0, _s()]))
    calls.append(("gemv:K%8", "csm_gemv_bf16", [xp, Wp, y, None, 1, 64, 1021, 1024, 1024, 64, 0, _s()]))

    def kext(label, rows=False, **o):
        k = dict(x=xp, W=Wp, y=y, R=None, B=2, N=64, K=1024, ldw=1024, ldx=1024, ldy=64, f32=0, nw=None, eps=1e-5, sw=0, ri=None, ro=0, t=tp, Bx=Bp, kx=40,
                 ldt=40, ldb=40, bias=None, Bxt=Bx_tab.data_ptr(), bt=None, ra=ra.data_ptr(), na=2)
        k.update(o)
        head = [k[n] for n in ("x", "W", "y", "R", "B", "N", "K", "ldw", "ldx", "ldy", "f32", "nw", "eps", "sw", "ri", "ro")]
        if rows:
            calls.append((f"kext_rows:{label}", "csm_gemv_bf16_kext_rows", head + [k["t"], k["Bxt"], k["bt"], k["ra"], k["na"], k["kx"], k["ldt"], k["ldb"], _s()]))
        else:
            calls.append((f"kext:{label}", "csm_gemv_bf16_kext", head + [k["t"], k["Bx"], k["kx"], k["ldt"], k["ldb"], k["bias"], _s()]))

    for rows in (False, True):
        for lab, o in (("kx=520", dict(kx=520, ldt=520, ldb=520)), ("kx=0", dict(kx=0)), ("kx%8", dict(kx=36)), ("ld_t<kx", dict(ldt=32)), ("ld_B<kx", dict(ldb=32)),
                       ("ld_t%8", dict(ldt=44)), ("ld_B%8", dict(ldb=44)), ("t misaligned", dict(t=tp + 2)), ("null t", dict(t=None)), ("B=0", dict(B=0)),
                       ("B=17", dict(B=17)), ("K%8", dict(K=1020)), ("swiglu odd N", dict(sw=1, N=63)), ("swiglu fp32", dict(sw=1, f32=1, y=y32))):
            kext(lab, rows, **o)
    kext("B=5", False, B=5)
    kext("Bx misaligned", False, Bx=Bp + 2)
    kext("null Bx", False, Bx=None)
    kext("K%32 at B=5", True, B=5, K=1000, ldw=1000, ldx=1000)
    kext("no adapters", True, na=0)
    kext("null row_adapter", True, ra=None)
    kext("null table", True, Bxt=None)

    def fp8(label, **o):
        k = dict(x=xp, W=W8.data_ptr(), s=scale.data_ptr(), y=y, R=None, B=2, N=64, K=1024, ldw=1024, ldx=1024, ldy=64, f32=0, nw=None, eps=1e-5, sw=0, ri=None, ro=0)
        k.update(o)
        calls.append((f"fp8:{label}", "csm_gemv_fp8w", [k[n] for n in ("x", "W", "s", "y", "R", "B", "N", "K", "ldw", "ldx", "ldy", "f32", "nw", "eps", "sw", "ri", "ro")] + [_s()]))

    for lab, o in (("B=0", dict(B=0)), ("B=17", dict(B=17)), ("K%16", dict(K=1016)), ("K>8192", dict(K=8208, ldw=8208, ldx=8208)), ("ldw8%16", dict(ldw=1032)),
                   ("ldw8<K", dict(ldw=1008)), ("W8 misaligned", dict(W=W8.data_ptr() + 8)), ("x misaligned", dict(x=xp + 2)), ("ldx%8", dict(ldx=1028)),
                   ("norm_scale misaligned", dict(nw=nw.data_ptr() + 2)), ("swiglu odd N", dict(sw=1, N=63)), ("swiglu fp32", dict(sw=1, f32=1, y=y32)),
                   ("null scale", dict(s=None))):
        fp8(lab, **o)

    def proj(label, rows=False, **o):
        k = dict(x=xp, At=Wp, t=y, B=2, K=1024, kx=40, ldx=1024, lda=40, ldt=64, scale=1.0, nw=None, eps=1e-5, tab=At_tab.data_ptr(), ra=ra.data_ptr(),
                 ps=pscale.data_ptr(), na=2)
        k.update(o)
        if rows:
            calls.append((f"proj_rows:{label}", "csm_lora_project_rows_bf16", [k["x"], k["tab"], k["t"], k["ra"], k["ps"], k["na"], k["B"], k["K"], k["kx"], k["ldx"],
                                                                             k["lda"], k["ldt"], k["nw"], k["eps"], _s()]))
        else:
            calls.append((f"proj:{label}", "csm_lora_project_bf16", [k["x"], k["At"], k["t"], k["B"], k["K"], k["kx"], k["ldx"], k["lda"], k["ldt"], k["scale"], k["nw"],
                                                                   k["eps"], _s()]))

    for rows in (False, True):
        for lab, o in (("B=0", dict(B=0)), ("K%8", dict(K=1020)), ("kx%8", dict(kx=36)), ("kx=0", dict(kx=0)), ("lda<kx", dict(lda=32)), ("ldt<kx", dict(ldt=32)),
                       ("lda%8", dict(lda=44)), ("norm with ldx%8", dict(nw=nw.data_ptr(), ldx=1028)), ("norm with x misaligned", dict(nw=nw.data_ptr(), x=xp + 2)),
                       ("null x", dict(x=None))):
            proj(lab, rows, **o)
    proj("B=5", False, B=5)
    proj("At misaligned", False, At=Wp + 2)
    proj("B=17", True, B=17)
    proj("no adapters", True, na=0)
    for lab, a in (("B=0", [xp, Wp, y, 0, 64, 16, 64, 16, 64, 0]), ("B=5", [xp, Wp, y, 5, 64, 16, 64, 16, 64, 0]), ("ldw%8", [xp, Wp, y, 2, 64, 16, 68, 16, 64, 0]),
                   ("N=0", [xp, Wp, y, 2, 0, 16, 64, 16, 64, 0]), ("null W", [xp, None, y, 2, 64, 16, 64, 16, 64, 0])):
        calls.append((f"gemv_t:{lab}", "csm_gemv_t_bf16", a + [_s()]))
    assert len(calls) >= 90
    want = [b.clone() for b in outs]
    for label, fn, args in calls:
        rc = getattr(lib, fn)(*args)
        assert rc == 1, f"{label}: returned {rc}"
        assert lib.csm_last_error(), label
    torch.cuda.synchronize()
    for b, w in zip(outs, want):
        assert torch.equal(_bits(b.cpu()), _bits(w.cpu())), "a refused call wrote to an output buffer"
    for key, val in ((5, 0), (-1, 1)):
        assert lib.csm_set_decode_tuning(key, val) != 0
    # the valid base calls are accepted (each refusal above is refused for the one thing it breaks)
    assert lib.csm_gemv_bf16_ex(xp, Wp, y, None, 2, 64, 1024, 1024, 1024, 64, 0, None, 1e-5, 0, None, 0, _s()) == 0
    assert lib.csm_gemv_bf16_kext(xp, Wp, y, None, 2, 64, 1024, 1024, 1024, 64, 0, None, 1e-5, 0, None, 0, tp, Bp, 40, 40, 40, None, _s()) == 0
    assert lib.csm_gemv_bf16_kext_rows(xp, Wp, y, None, 2, 64, 1024, 1024, 1024, 64, 0, None, 1e-5, 0, None, 0, tp, Bx_tab.data_ptr(), None, ra.data_ptr(), 2, 40,
                                       40, 40, _s()) == 0
    assert lib.csm_gemv_fp8w(xp, W8.data_ptr(), scale.data_ptr(), y, None, 2, 64, 1024, 1024, 1024, 64, 0, None, 1e-5, 0, None, 0, _s()) == 0
    assert lib.csm_lora_project_bf16(xp, Wp, y, 2, 1024, 40, 1024, 40, 64, 1.0, None, 1e-5, _s()) == 0
    assert lib.csm_lora_project_rows_bf16(xp, At_tab.data_ptr(), y, ra.data_ptr(), pscale.data_ptr(), 2, 2, 1024, 40, 1024, 40, 64, None, 1e-5, _s()) == 0
    assert lib.csm_gemv_t_bf16(xp, Wp, y, 2, 64, 16, 64, 16, 64, 0, _s()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(outs[0].cpu()), _bits(want[0].cpu()))
    del R, bias


def test_records(dev):
    """The worst utilisation per route and judgement seen by this file (runs last): the record for decode_gemv_ref's docstring."""
    rows = {k: v for k, v in D.utilisation.items() if k.startswith("dgemv.")}
    for key in sorted(rows):
        print(f"UTILISATION {key} {rows[key]:.4f}")
    assert rows and max(rows.values()) <= 1.0
