"""Proof of tests/decode_gemv_ref.py on the CPU: the reference agrees with torch's own float64 machinery, correct fp32
restatements of the decode product kernels' arithmetic (summed in two orders that are not torch.matmul's) fit every bound, the
integer cases' expectations are exact, and every wrong restatement is caught on every case it applies to."""
import pytest
import torch

import decode_gemv_ref as D
import train_gemm_ref as G

F64, BF16 = torch.float64, torch.bfloat16
SMALL = [c for c in D.CASES if not c.big]
_DATA = {}


def _data(c):
    """(inputs, wide embedded reference, tight embedded reference or None) once per data key."""
    k = c.data_key()
    if k not in _DATA:
        i = D.inputs(c)
        wide = D.embedded(c, *D.reference(i))
        tight = D.embedded(c, *D.reference(i, xhat=D.xhat32(i), flips=c.K > D.RMS_TIGHT_MAX_K)) if c.norm else None
        _DATA[k] = (i, wide, tight)
    return _DATA[k]


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.data_key() not in seen:
            seen.add(c.data_key())
            out.append(c)
    return out


UNIQUE = _unique(SMALL)


def _fails(c, buf, refs):
    """The judgement of a wrong restatement: the GPU test asserts every reference the case has (wide, and tight where x^ is
    normalised), so a mutant is caught when one of them fails.  -> the number that fail."""
    bad = 0
    for emb in refs:
        try:
            D.judge("mutant", buf, *emb)
        except AssertionError:
            bad += 1
    return bad


def test_case_table_covers_the_routes():
    want = {"gemv_reg_kernel", "gemv_regn_kernel", "gemv_kernel", "gemv_mfma_kernel", "gemv_fp8_kernel", "gemv_fp8_mfma_kernel",
            "lora_project_kernel", "lora_project_rows_kernel", "gemv_t_kernel"}
    assert set(D.ROUTES) == want
    ks = {D.expected_kernel(c) for c in D.CASES}
    for kch in (2, 4, 16):
        assert any(k.startswith(f"gemv_reg_kernel<{kch},") for k in ks) and any(k.startswith(f"gemv_regn_kernel<{kch},") for k in ks)
    for seg in (1, 2, 4, 8):
        assert any(k.startswith(f"gemv_mfma_kernel<{seg},") for k in ks) and any(k.startswith(f"gemv_fp8_mfma_kernel<{seg},") for k in ks)
    for kc in (1, 2, 8):
        assert any(k.startswith(f"gemv_fp8_kernel<{kc},") for k in ks)
    assert {"gemv_reg_kernel<2, bf16, 1, 0, 2, ext0>", "gemv_reg_kernel<2, bf16, 1, 0, 4, ext0>", "gemv_reg_kernel<16, bf16, 0, 1, 1, ext0>",
            "gemv_regn_kernel<16, 3, bf16, 0, 1, 4, ext0>", "gemv_mfma_kernel<8, bf16, 0, 1, ext0>"} <= ks
    for ext in (1, 2):
        for r in ("gemv_reg_kernel", "gemv_regn_kernel", "gemv_kernel"):
            assert any(k.startswith(r) and k.endswith(f"ext{ext}>") for k in ks), (r, ext)
    assert any(k.startswith("gemv_mfma_kernel") and k.endswith("ext2>") for k in ks)
    assert sum(c.big for c in D.CASES) == 3
    assert any(D.dynamic_lds_bytes(c) > 65536 for c in D.CASES if D.route_of(c) == "gemv_regn_kernel")
    assert any(D.dynamic_lds_bytes(c) > 65536 for c in D.CASES if D.route_of(c) == "gemv_fp8_kernel")
    for c in D.CASES:                                             # nothing the library would refuse, nothing outside the LDS copy of x
        assert 1 <= c.B <= 16 and (c.kind in ("gemv_t",) or c.K % 8 == 0)
        if c.kind == "fp8":
            assert c.K % 16 == 0 and c.K <= 8192
        if c.mfma:
            assert c.K % 32 == 0
        if D.route_of(c) == "gemv_kernel":
            assert c.B * c.K * 2 <= 65536
    # every route has a strided and a contiguous case
    for r in D.ROUTES:
        assert {c.pad for c in D.CASES if D.route_of(c) == r} == {0, 1}, r


@pytest.mark.parametrize("c", UNIQUE, ids=lambda c: c.name)
def test_reference_agrees_with_torch(c):
    """The value against torch's own float64 matmul / rms_norm / silu, written independently of the module's helpers."""
    i = _data(c)[0]
    if c.fam == "integer":
        return                                                    # (test_integer_cases_are_exact)
    val = D.reference(i)[0]
    x = i["x"].double()[D.x_rows(c, i)]
    if c.norm:
        x = torch.nn.functional.rms_norm(x, (c.K,), i["nw"].double(), D.EPS)
    ad = [D.live_adapter(a) for a in D.adapters(c)]
    if c.kind == "proj":
        want = D.PROJ_SCALE * torch.matmul(x, i["W"][0].double())
    elif c.kind == "proj_rows":
        want = torch.stack([float(i["pscale"][a]) * torch.matmul(x[b], i["W"][a].double()) if a >= 0 else torch.zeros(c.kx, dtype=F64)
                            for b, a in enumerate(ad)])
    elif c.kind == "gemv_t":
        want = torch.matmul(x, i["W"].double())
    else:
        if c.kind == "fp8":
            from csm.quant import dequantize_rows_fp8
            W = dequantize_rows_fp8(i["W8"], torch.ones(c.N)).double() * i["scale"].double()[:, None]
        else:
            W = i["W"].double()
        want = torch.matmul(x, W.t())
        if c.ext:
            for b in range(c.B):
                a = ad[b] if c.ext == 2 else 0
                if a >= 0:
                    want[b] += torch.matmul(i["Bx"][a].double(), i["t"][b].double())
                    if c.bias and not i["bias_null"][a]:
                        want[b] += i["bias"][a].double()
        if c.swiglu:
            want = torch.nn.functional.silu(want[:, 0::2]) * want[:, 1::2]
    if c.res:
        want = want + i["R"].double()[:, :c.no]
    if c.swiglu:
        # the reference does not round g and u (its slack carries that rounding): the same formula, loosely compared too
        assert torch.allclose(val, want, rtol=1e-9, atol=1e-12)
    else:
        assert torch.allclose(val, want, rtol=1e-11, atol=1e-13), float((val - want).abs().max())


@pytest.mark.parametrize("c", UNIQUE, ids=lambda c: c.name)
def test_fp32_restatements_fit_the_bounds(c):
    i, wide, tight = _data(c)
    for order in D.ORDERS:
        buf = D.restate(i, order)
        D.judge_case(f"cpu.{D.route_of(c)}.{order}", c, buf, wide)
        if tight is not None:
            D.judge_case(f"cpu.{D.route_of(c)}.{order}.tight", c, buf, tight)


def test_wide_slack_is_mostly_the_normalisation(capsys):
    """What the tight judgement is for: in the wide slack of the normalised cases the x^ term dominates."""
    shares = []
    for c in UNIQUE:
        if c.norm and c.kind == "gemv" and not c.swiglu and not c.ext:
            i = _data(c)[0]
            w, t = D.reference(i)[1], D.reference(i, xhat=D.xhat32(i))[1]
            shares.append(float(1 - (t.sum() / w.sum())))
    assert shares and min(shares) > 0.5, min(shares)


def test_integer_cases_are_exact():
    """Integer operands: the expectation is RNE-bf16 of an integer-arithmetic value, every fp32 order gives it bit for bit, and
    every element carries slack -1."""
    n = 0
    for c in UNIQUE:
        if c.fam != "integer":
            continue
        n += 1
        i = _data(c)[0]
        val, sl = D.reference(i)
        assert bool((sl < 0).all())
        assert bool((val * 4 == (val * 4).round()).all())            # integers (quarters under an FP8 scale of 1/2 or lora_project's 1.75)
        for order in D.ORDERS:
            got = G.view(D.restate(i, order), D.layout(c))[0]
            assert torch.equal(got.double(), val), c.name
        # in int64 arithmetic, for the forms that have one
        if c.kind == "gemv" and not c.ext:
            x = i["x"].double()[D.x_rows(c, i)].long()
            exact = x @ i["W"].double().long().t()
            if c.res:
                exact = exact + i["R"].double().long()[:, :c.no]
            assert bool((exact.abs() < 2 ** 24).all())
            assert torch.equal(exact.double() if c.f32 else exact.double().to(BF16).double(), val)
    assert n >= 40


def _mutant_cases(mut):
    return [c for c in UNIQUE if D.applies(mut, c)]


@pytest.mark.parametrize("mut", [m for m in D.MUTANTS if m != "chunk"])
def test_wrong_restatements_are_caught(mut):
    cases = _mutant_cases(mut)
    assert len(cases) >= 3, (mut, len(cases))
    missed = []
    for c in cases:
        i, wide, tight = _data(c)
        refs = [wide] if tight is None else [wide, tight]
        if not _fails(c, D.restate(i, "lanes", mut), refs):
            missed.append(c.name)
    assert not missed, f"{mut}: not caught on {len(missed)} of {len(cases)}: {missed[:12]}"


def test_every_planted_chunk_is_seen():
    """Each single aligned 8-chunk of k zeroed, at every planted position of every planted case: caught by the tight
    judgement where there is one, by the only one otherwise."""
    cases = _mutant_cases("chunk")
    assert len(cases) >= 40
    missed, n = [], 0
    for c in cases:
        i, wide, tight = _data(c)
        refs = [wide] if tight is None else [tight]               # (a dropped chunk must be seen where the x^ rounding does not hide it)
        chunks = D.planted_chunks(c.K)
        assert chunks and chunks[0] == 0 and chunks[-1] == c.K // 8 - 1
        if c.K >= 1024:
            assert {63, 64, c.K // 8 - 4} <= set(chunks)
        for ch in chunks:
            n += 1
            if not _fails(c, D.restate(i, "lanes", "chunk", ch), refs):
                missed.append((c.name, ch))
    assert not missed, f"{len(missed)} of {n} dropped chunks not caught: {missed[:12]}"


def test_swiglu_tight_reference():
    """swiglu_tight of the bf16 (g, u) an fp32 restatement of the plain product leaves: the fused restatement fits it."""
    n = 0
    for c in UNIQUE:
        if not c.swiglu or c.fam == "integer":
            continue
        n += 1
        i = _data(c)[0]
        plain = c.with_(c.name + "_gu", swiglu=0, res=0, tag=c.name)
        gu = G.view(D.restate(dict(i, c=plain), "lanes"), D.layout(plain))[0]
        v, s = D.swiglu_tight(gu, i["R"][:, :c.no] if c.res else None)
        D.judge_case(f"cpu.{D.route_of(c)}.swiglu_tight", c, D.restate(i, "lanes"), D.embedded(c, v, s))
        if D.applies("gate_up_swapped", c):
            with pytest.raises(AssertionError):
                D.judge("mutant", D.restate(i, "lanes", "gate_up_swapped"), *D.embedded(c, v, s))
    assert n >= 20


def test_guard_elements_are_judged():
    c = D.CASE["regn_K1024_B2_plain_random"]
    i, wide, _ = _data(c)
    l = D.layout(c)
    for j in (l.off + G.GR * l.ld - 1, l.off + G.GR * l.ld + c.no, l.off + (G.GR + c.B) * l.ld, 0, G.flat_len(l) - 1):
        buf = D.restate(i)
        buf[j] = 0.5
        with pytest.raises(AssertionError):
            D.judge("guard", buf, *wide)


def test_dispatch_restatement_matches_the_source():
    """expected_kernel restates gemv_launch / csm_gemv_fp8w: the thresholds it relies on are still in the sources."""
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csm-train-pytorch_amd", "csrc")
    gen, q = open(os.path.join(root, "generate.hip")).read(), open(os.path.join(root, "quant.hip")).read()
    mfma = open(os.path.join(root, "gemv_mfma.h")).read()          # the B = 5..16 launcher both files call
    for text in ("if (B == 1 && g_gemv_reg && (K == 1024 || K == 2048 || K == 8192))",
                 "if (B >= 2 && g_gemv_reg && g_gemv_regn && (K == 1024 || K == 2048 || (K == 8192 && !swiglu && !out_f32)))",
                 "if (B > 4 || (B >= 2 && g_gemv_mfma_small && (K & 31) == 0))",
                 "const bool nt = g_gemv_nt && (K == 2048 || (K == 8192 && N == 2048));",
                 "if (swiglu && K == 1024 && !nt && g_gemv_rpw > 1 && no >= 2048)"):
        assert text in gen, text
    for text in ("const int spw = ((K + 63) / 64 + 7) / 8;", "const int seg = spw <= 1 ? 1 : (spw <= 2 ? 2 : (spw <= 4 ? 4 : 8));"):
        assert text in mfma, text
    for text in ("const int kc = K <= 1024 ? 1 : (K <= 2048 ? 2 : 8);", "const bool nt = K == 2048 || (K == 8192 && N == 2048);",
                 "if (B > 4)"):
        assert text in q, text
    from csm import hip
    assert hip._SIGS["csm_gemv_last_kernel"] == ([], hip.C.c_char_p) and hasattr(hip.lib, "csm_gemv_last_kernel")
