"""Proof of tests/decode_gemv_fp8_kext_ref.py on the CPU: the reference agrees with a plain torch float64 computation, fp32
restatements of the arithmetic quant.hip documents for csm_gemv_fp8w_kext_rows (two summation orders) fit every bound, the
integer cases are exact, and every wrong restatement is caught on every case it applies to.  Header, ctypes table and the built
library agree on the new symbol."""
import os
import re

import pytest
import torch

import decode_gemv_fp8_kext_ref as X
import decode_gemv_ref as D
import train_gemm_ref as G

F64, BF16 = torch.float64, torch.bfloat16
_DATA = {}


def _data(c):
    """(inputs, wide embedded reference, tight embedded reference or None) once per case."""
    if c.name not in _DATA:
        i = X.inputs(c)
        wide = X.embedded(c, *X.reference(i))
        tight = X.embedded(c, *X.reference(i, xhat=D.xhat32(i), flips=c.K > D.RMS_TIGHT_MAX_K)) if c.norm else None
        _DATA[c.name] = (i, wide, tight)
    return _DATA[c.name]


def _fails(buf, refs):
    bad = 0
    for emb in refs:
        try:
            D.judge("mutant", buf, *emb)
        except AssertionError:
            bad += 1
    return bad


def test_case_table_covers_the_paths():
    assert set(X.ROUTES) == {"gemv_fp8_kernel", "gemv_fp8_mfma_kernel"}
    ks = {X.expected_kernel(c) for c in X.CASES}
    assert all(k.endswith(", ext2>") for k in ks)
    for kc in (1, 2, 8):
        for nb in (1, 2, 3, 4):
            assert any(k.startswith(f"gemv_fp8_kernel<{kc}, {nb},") for k in ks), (kc, nb)
    for seg in (1, 2, 4, 8):
        assert any(k.startswith(f"gemv_fp8_mfma_kernel<{seg},") for k in ks)
    assert {c.K for c in X.CASES} == set(X.KS) and {c.B for c in X.CASES} == set(X.BS) and {c.kx for c in X.CASES} == set(X.KXS)
    assert {c.no for c in X.CASES} == {X.N_OUT}
    for r in X.ROUTES:
        mine = [c for c in X.CASES if X.route_of(c) == r]
        assert {c.pad for c in mine} == {0, 1} and {c.bias for c in mine} == {0, 1, 2} and {c.fam for c in mine} == {"random", "planted", "integer"}
        for f in ("res", "f32", "norm", "swiglu", "gather"):
            assert any(getattr(c, f) for c in mine), (r, f)
        assert any(k.split(", ")[-2] == "1" for k in {X.expected_kernel(c) for c in mine})      # a non-temporal instantiation
    assert any(D.dynamic_lds_bytes(c) > 65536 for c in X.CASES)
    rows = {a for c in X.CASES for a in D.adapters(c)}
    assert rows == {0, 1, 2, -1, D.N_ADAPTERS}
    one = {D.adapters(c)[0] for c in X.CASES if c.B == 1}
    assert {0, 1, -1, D.N_ADAPTERS} <= one
    for c in X.CASES:                                             # nothing the entry point would refuse
        assert c.K % 16 == 0 and c.K <= 8192 and c.kx % 8 == 0 and 0 < c.kx <= 512 and 1 <= c.B <= 16
    # planted: every chunk of the extension, the first and chunk kx / 8 - 1 among them
    for c in X.CASES:
        if c.fam == "planted":
            ch = X.ext_chunks(c)
            assert ch[0] == 0 and ch[-1] == c.kx // 8 - 1 and len(ch) == c.kx // 8


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_reference_agrees_with_torch(c):
    """Against torch's float64 matmul / rms_norm / silu on the DEQUANTISED weights (scale folded into W: another association)."""
    i = _data(c)[0]
    val = X.reference(i)[0]
    from csm.quant import dequantize_rows_fp8
    x = i["x"].double()[D.x_rows(c, i)]
    if c.norm:
        x = torch.nn.functional.rms_norm(x, (c.K,), i["nw"].double(), D.EPS)
    W = dequantize_rows_fp8(i["W8"], torch.ones(c.N)).double() * i["scale"].double()[:, None]
    want = torch.matmul(x, W.t())
    for b, a in enumerate(D.adapters(c)):
        if 0 <= a < D.N_ADAPTERS:
            want[b] += torch.matmul(i["Bx"][a].double(), i["t"][b].double())
            if c.bias and not (c.bias == X.BIAS_ONE_NULL and a == 1):
                want[b] += i["bias"][a].double()
    if c.swiglu:
        want = torch.nn.functional.silu(want[:, 0::2]) * want[:, 1::2]
    if c.res:
        want = want + i["R"].double()[:, :c.no]
    if c.fam == "integer":
        want = want if c.f32 else want.to(BF16).double()
        assert torch.equal(val, want)
    else:
        assert torch.allclose(val, want, rtol=1e-9 if c.swiglu else 1e-11, atol=1e-12), float((val - want).abs().max())


@pytest.mark.parametrize("c", X.CASES, ids=lambda c: c.name)
def test_fp32_restatements_fit_the_bounds(c):
    i, wide, tight = _data(c)
    for order in D.ORDERS:
        buf = X.restate(i, order)
        D.judge_case(f"cpu.{X.route_of(c)}.{order}", c, buf, wide)
        if tight is not None:
            D.judge_case(f"cpu.{X.route_of(c)}.{order}.tight", c, buf, tight)
        if c.fam == "integer":
            assert torch.equal(G.view(buf, D.layout(c))[0].double(), X.reference(i)[0]), c.name


def test_integer_cases_are_exact():
    n = 0
    for c in X.CASES:
        if c.fam != "integer":
            continue
        n += 1
        val, sl = X.reference(_data(c)[0])
        assert bool((sl < 0).all()) and bool((val * 2 == (val * 2).round()).all())        # halves under a scale of 1/2
        assert float(val.abs().max()) < 2 ** 20
    assert n >= 8


@pytest.mark.parametrize("mut", [m for m in X.MUTANTS if m != "ext_chunk"])
def test_wrong_restatements_are_caught(mut):
    cases = [c for c in X.CASES if X.applies(mut, c)]
    assert len(cases) >= 3, (mut, len(cases))
    missed = []
    for c in cases:
        i, wide, tight = _data(c)
        refs = [wide] if tight is None else [wide, tight]
        if not _fails(X.restate(i, "lanes", mut), refs):
            missed.append(c.name)
    assert not missed, f"{mut}: not caught on {len(missed)} of {len(cases)}: {missed[:12]}"


def test_every_dropped_extension_chunk_is_seen():
    """Each aligned 8-chunk of the extension dropped, one at a time, on every planted case: caught (by the tight judgement where
    there is one)."""
    cases = [c for c in X.CASES if X.applies("ext_chunk", c)]
    assert len(cases) >= 8 and any(c.kx == 512 for c in cases) and {X.route_of(c) for c in cases} == set(X.ROUTES)
    missed, n = [], 0
    for c in cases:
        i, wide, tight = _data(c)
        refs = [wide] if tight is None else [tight]
        for ch in X.ext_chunks(c):
            n += 1
            if not _fails(X.restate(i, "lanes", "ext_chunk", ch), refs):
                missed.append((c.name, ch))
    assert n >= 200 and not missed, f"{len(missed)} of {n} dropped chunks not caught: {missed[:12]}"


def test_rows_without_adapter_are_the_plain_fp8_product():
    """The reference and the restatement of a row with a = -1 or a >= n_adapters are decode_gemv_ref's plain FP8 ones."""
    n = 0
    for c in X.CASES:
        live = X.live_rows(c)
        if all(a >= 0 for a in live) or c.fam == "integer":
            continue
        i = _data(c)[0]
        plain = c.with_(c.name + "_plain", ext=0, kx=0, bias=0)
        pi = dict(i, c=plain)
        (v, s), (pv, ps) = X.reference(i), D.reference(pi)
        got, pgot = G.view(X.restate(i), D.layout(c))[0], G.view(D.restate(pi), D.layout(plain))[0]
        for b, a in enumerate(live):
            if a < 0:
                n += 1
                # (the slack is the same expression associated another way: float64 rounding apart)
                assert torch.equal(v[b], pv[b]) and torch.allclose(s[b], ps[b], rtol=1e-12, atol=0) and torch.equal(got[b], pgot[b]), (c.name, b)
    assert n >= 20


def test_header_sigs_and_library_agree():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "csm_hip.h")).read()
    m = re.search(r"\bint csm_gemv_fp8w_kext_rows\((.*?)\);", text, re.S)
    assert m, "csm_gemv_fp8w_kext_rows is not declared in include/csm_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    base = re.search(r"\bint csm_gemv_fp8w\((.*?)\);", text, re.S).group(1).replace("\n", " ").split(",")
    rows = re.search(r"\bint csm_gemv_bf16_kext_rows\((.*?)\);", text, re.S).group(1).replace("\n", " ").split(",")
    names = lambda ps: [re.split(r"[\s*]+", p.strip())[-1] for p in ps]      # noqa: E731
    # csm_gemv_fp8w's list, then csm_gemv_bf16_kext_rows's extension arguments in its order, then the stream
    assert names(params) == names(base)[:-1] + names(rows)[names(rows).index("ext_t"):]
    from csm import hip
    C = hip.C

    def ctype(p):
        if "*" in p or p.startswith("csm_stream_t"):
            return C.c_void_p
        return {"int": C.c_int, "float": C.c_float}[p.split()[0]]

    args, res = hip._SIGS["csm_gemv_fp8w_kext_rows"]
    assert res is C.c_int and list(args) == [ctype(p) for p in params]
    assert hasattr(hip.lib, "csm_gemv_fp8w_kext_rows")
    assert hip.lib.csm_abi_version() == 3
    from csm.hip import ops
    assert callable(ops.gemv_fp8w_kext_rows)
