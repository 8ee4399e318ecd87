"""The fp32 Mimi codec kernels of csrc/codec.hip - csm_conv1d_f32, csm_conv_transpose1d_f32, csm_layernorm_f32, csm_linear_f32
(tiled and few-rows), csm_rope_half_f32, csm_attn_window_f32 (+ its stream form), csm_transpose_f32 and the rows forms - against
the float64 reference of tests/codec_ref.py (proved against torch's float64 kernels by tests/test_codec_ref_cpu.py).  Kernel
level only: no model is built.

Every output buffer starts as NaN and every element is judged: |got - ref| <= bound, the bound derived in codec_ref from
u = 2^-24, the length of the kernel's serial chain and the measured allowances of the device elementary functions - never from
what the kernels give.  One-hot attention cases, transposes and the rows forms (against the one-row stream kernels) are exact,
bit for bit.  Each judgement prints ``RATIO <kernel> <worst |err| / bound>``; a ratio above 1 fails."""
import pytest
import torch

import codec_ref as R
from test_stream_gpu import CONV_CASES, CONVT_CASES

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _judge(kernel, got, ref_out, bound, what=""):
    ratio = R.worst_ratio(got, ref_out, bound)
    print(f"RATIO {kernel} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{kernel} {what}: worst |err| / bound = {ratio:.3f}"


# ------------------------------------------------------------------------------------------------------------- conv1d
def _conv_gpu(c, inp):
    from csm.hip import check, lib
    x, w, b, res = _cu(*inp)
    y = _nan(c.C_out, c.T_out)
    check(lib.csm_conv1d_f32(_p(x), _p(w), _p(b), _p(res), _p(y), c.C_in, c.C_out, c.T_in, c.T_out, c.k, c.stride, c.dil, c.pad_left,
                             c.pad_mode, c.groups, int(c.elu), _s()), "csm_conv1d_f32")
    return y


@pytest.mark.parametrize("c", R.conv_cases(), ids=lambda c: c.name)
def test_conv1d(dev, c):
    inp = R.conv_inputs(c)
    ref = R.conv_ref(c, inp)
    _judge("csm_conv1d_f32", _conv_gpu(c, inp), ref.out, R.conv_bound(ref), c.name)


def test_conv1d_grid_stride_loop(dev):
    """T_out = 4096 * 256 + 257: the last 257 outputs belong to the second pass of the loop."""
    c = R.CONV_LOOP
    inp = R.conv_inputs(c)
    y = _conv_gpu(c, inp)
    assert not bool(torch.isnan(y).any()), f"{int(torch.isnan(y).sum())} outputs never written, first at {int(torch.isnan(y).flatten().nonzero()[0])}"
    cols = R.loop_columns(c.T_out)
    ref = R.conv_ref(c, inp, t_idx=cols)
    _judge("csm_conv1d_f32", y[:, cols.cuda()], ref.out, R.conv_bound(ref), "loop")


# ------------------------------------------------------------------------------------------------------------- conv_transpose1d
def _convt_gpu(c, inp):
    from csm.hip import check, lib
    x, w, b = _cu(*inp)
    y = _nan(c.C_out, c.T_out)
    check(lib.csm_conv_transpose1d_f32(_p(x), _p(w), _p(b), _p(y), c.C_in, c.C_out, c.T_in, c.T_out, c.k, c.stride, c.crop, c.groups,
                                       int(c.elu), _s()), "csm_conv_transpose1d_f32")
    return y


@pytest.mark.parametrize("c", R.convt_cases(), ids=lambda c: c.name)
def test_conv_transpose1d(dev, c):
    inp = R.convt_inputs(c)
    ref = R.convt_ref(c, inp)
    y = _convt_gpu(c, inp)
    _judge("csm_conv_transpose1d_f32", y, ref.out, R.convt_bound(ref), c.name)
    if not bool(ref.reached.all()):                     # outputs no tap reaches: the bias, or 0, exactly
        want = (inp[2] if inp[2] is not None else torch.zeros(c.C_out))[:, None].expand(c.C_out, c.T_out)
        assert _same(y.cpu()[~ref.reached], want[~ref.reached].contiguous())


def test_conv_transpose1d_grid_stride_loop(dev):
    c = R.CONVT_LOOP
    inp = R.convt_inputs(c)
    y = _convt_gpu(c, inp)
    assert not bool(torch.isnan(y).any()), f"{int(torch.isnan(y).sum())} outputs never written"
    cols = R.loop_columns(c.T_out)
    ref = R.convt_ref(c, inp, t_idx=cols)
    _judge("csm_conv_transpose1d_f32", y[:, cols.cuda()], ref.out, R.convt_bound(ref), "loop")


# ------------------------------------------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layernorm(dev, case):
    from csm.hip import check, lib
    inp = R.ln_inputs(case)
    x, w, b = _cu(*inp)
    y = _nan(*x.shape)
    check(lib.csm_layernorm_f32(_p(x), _p(w), _p(b), _p(y), x.shape[0], x.shape[1], R.LN_EPS, _s()), "csm_layernorm_f32")
    ref = R.layernorm(*inp, R.LN_EPS)
    _judge("csm_layernorm_f32", y, ref.out, R.layernorm_bound(ref), str(case))


# ------------------------------------------------------------------------------------------------------------- linear
def _linear_gpu(x, W, scale, res, act, K):
    from csm.hip import check, lib
    T, N = x.shape[0], W.shape[0]
    y = _nan(T, N)
    check(lib.csm_linear_f32(_p(x), _p(W), _p(scale), _p(res), _p(y), T, N, K, x.shape[1], act, _s()), "csm_linear_f32")
    return y


@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("shape", R.LIN_TILED, ids=str)
def test_linear_tiled(dev, shape, epi):
    T, N, K, pad = shape
    inp = R.linear_inputs(T, N, K, pad, epi)
    x, W, scale, res = _cu(*inp[:4])
    ref = R.linear(*inp, K)
    _judge("csm_linear_f32(tiled)", _linear_gpu(x, W, scale, res, inp[4], K), ref.out, R.linear_bound(ref), f"{shape} {epi}")


@pytest.mark.parametrize("epi", R.EPILOGUES)
@pytest.mark.parametrize("shape", R.LIN_ROWS, ids=str)
def test_linear_few_rows(dev, shape, epi):
    """T <= 16, K % 32 == 0, an aligned W: the one-thread-per-output kernel.  The same weights one float off a 16-byte boundary
    take the tiled kernel, which must meet the bound too and give the same bits."""
    T, N, K, pad = shape
    inp = R.linear_inputs(T, N, K, pad, epi)
    x, W, scale, res = _cu(*inp[:4])
    assert W.data_ptr() % 16 == 0
    ref = R.linear(*inp, K)
    bound = R.linear_bound(ref)
    y = _linear_gpu(x, W, scale, res, inp[4], K)
    _judge("csm_linear_f32(rows)", y, ref.out, bound, f"{shape} {epi}")
    buf = torch.empty(N * K + 1, device="cuda")
    W1 = buf[1:].view(N, K)
    W1.copy_(W)
    assert W1.data_ptr() % 16 == 4
    y1 = _linear_gpu(x, W1, scale, res, inp[4], K)
    _judge("csm_linear_f32(tiled)", y1, ref.out, bound, f"{shape} {epi} W + 1 float")
    assert _same(y1, y), (shape, epi)


# ------------------------------------------------------------------------------------------------------------- rope_half
def _rope_gpu(qkv, H, hd, pos0):
    from csm.hip import check, lib
    g = qkv.cuda()
    check(lib.csm_rope_half_f32(_p(g), g.shape[0], H, hd, R.ROPE_BASE, pos0, _s()), "csm_rope_half_f32")
    return g


@pytest.mark.parametrize("pos0", R.ROPE_POS)
@pytest.mark.parametrize("geom", R.ROPE_GEOMS, ids=str)
def test_rope_half(dev, geom, pos0):
    H, hd = geom
    qkv = R.rope_inputs(5, H, hd, pos0)
    ref = R.rope_half(qkv, H, hd, R.ROPE_BASE, pos0)
    got = _rope_gpu(qkv, H, hd, pos0)
    _judge("csm_rope_half_f32", got, ref.out, R.rope_bound(ref), f"{geom} pos0 {pos0}")
    assert _same(got[:, 2 * H * hd:], qkv[:, 2 * H * hd:])                       # the v third: untouched


@pytest.mark.parametrize("geom", R.ROPE_GEOMS, ids=str)
def test_rope_half_position_is_absolute(dev, geom):
    """pos0 = p, T = 1 gives row p of pos0 = 0, T = p + 1, bit for bit (p = 4095 at H = 8 also runs the grid-stride loop)."""
    H, hd = geom
    P = max(R.ROPE_POS)
    qkv = R.rope_inputs(P + 1, H, hd, 0)
    whole = _rope_gpu(qkv, H, hd, 0)
    for p in R.ROPE_POS:
        assert _same(_rope_gpu(qkv[p:p + 1], H, hd, p), whole[p:p + 1]), p


def test_rope_half_grid_stride_loop(dev):
    T, H, hd, pos0 = R.ROPE_LOOP
    qkv = R.rope_inputs(T, H, hd, pos0)
    ref = R.rope_half(qkv, H, hd, R.ROPE_BASE, pos0)
    got = _rope_gpu(qkv, H, hd, pos0)
    _judge("csm_rope_half_f32", got, ref.out, R.rope_bound(ref), "loop")
    assert _same(got[:, 2 * H * hd:], qkv[:, 2 * H * hd:])


# ------------------------------------------------------------------------------------------------------------- attn_window
def _attn_forms(qkv, H, window):
    """The full-sequence kernel, the stream kernel in one chunk and in chunks of 3 (ring exactly window + n - 1, NaN before)."""
    from csm.hip import check, lib, ops
    g = qkv.cuda()
    T, D = g.shape[0], H * R.ATTN_HD
    out = _nan(T, D)
    check(lib.csm_attn_window_f32(_p(g), _p(out), T, H, R.ATTN_HD, window, _s()), "csm_attn_window_f32")
    yield "csm_attn_window_f32", out
    for n in (T, 3):
        kc, vc = _nan(window + n - 1, D), _nan(window + n - 1, D)
        outs = []
        for t0 in range(0, T, n):
            o = _nan(min(n, T - t0), D)
            ops.attn_window_stream_f32(g[t0:t0 + n], kc, vc, o, t0, H, window)
            outs.append(o)
        yield f"csm_attn_window_stream_f32(n={'T' if n == T else n})", torch.cat(outs)


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attn_window_random(dev, case):
    H, window = case
    qkv = R.attn_random(H, window)
    ref = R.attn_window(qkv, H, R.ATTN_HD, window)
    bound = R.attn_bound(ref)
    for name, out in _attn_forms(qkv, H, window):
        _judge(name, out, ref.out, bound, str(case))


@pytest.mark.parametrize("case", R.ATTN_CASES, ids=str)
def test_attn_window_onehot(dev, case):
    """The oldest key of the window carries the whole softmax: row q is its value row bit for bit.  The same key one position
    older is outside the window: the reference ignores it, and a kernel that admitted it would return its value row."""
    H, window = case
    D = H * R.ATTN_HD
    for q in R.onehot_queries(window):
        qkv, pos = R.onehot_case(H, window, q)
        ref = R.attn_window(qkv, H, R.ATTN_HD, window)
        bound = R.attn_bound(ref)
        for name, out in _attn_forms(qkv, H, window):
            _judge(name, out, ref.out, bound, f"{case} one-hot q {q}")
            assert _same(out[q], qkv[pos, 2 * D:]), (name, case, q)
        qkv, pos = R.onehot_case(H, window, q, outside=True)
        if qkv is None:
            continue
        ref = R.attn_window(qkv, H, R.ATTN_HD, window)
        bound = R.attn_bound(ref)
        for name, out in _attn_forms(qkv, H, window):
            _judge(name, out, ref.out, bound, f"{case} key outside q {q}")


# ------------------------------------------------------------------------------------------------------------- transpose
def test_transpose_exact(dev):
    from csm.hip import check, lib, ops
    for Rr in R.TRANSPOSE_SIZES:
        for Cn in R.TRANSPOSE_SIZES:
            x = torch.randn(3, Rr, Cn, generator=torch.Generator().manual_seed(Rr * 100 + Cn))
            want = R.transpose(x)
            g = x.cuda()
            y = _nan(Cn, Rr)
            check(lib.csm_transpose_f32(_p(g[0]), _p(y), Rr, Cn, _s()), "csm_transpose_f32")
            assert _same(y, want[0]), (Rr, Cn)
            for batch in (1, 3):
                yb = _nan(batch, Cn, Rr)
                ops.transpose_rows_f32(g[:batch].contiguous(), yb)
                assert _same(yb, want[:batch]), (Rr, Cn, batch)


# ------------------------------------------------------------------------------------------------------------- rows forms
ROWS_R = (1, 3, 16)
ROWS_N = (1, 5, 22, 90)             # R * n below 64, between 64 and 256, above 256: every branch of rows_block


def _rows_layout(Rn, salt):
    """Scrambled distinct slots in an arena of Rn + 3 slots, mixed parities, a different position per row."""
    n_slots = Rn + 3
    slots = [(5 * r + 2 + salt) % n_slots for r in range(Rn)] if n_slots % 5 else [(7 * r + 2 + salt) % n_slots for r in range(Rn)]
    assert len(set(slots)) == Rn
    parity = [(r * r + r // 2 + salt) % 2 for r in range(Rn)]
    pos = [(37 * r + 11 * salt) % 101 for r in range(Rn)]
    return n_slots, slots, parity, pos


def _guard(*shape):
    """A finite pattern with no two neighbours equal: an untouched element is recognised bit for bit."""
    n = 1
    for s in shape:
        n *= s
    return (1000.0 + torch.arange(n, dtype=torch.float32) * 0.25).reshape(shape).cuda()


@pytest.mark.parametrize("Rn", ROWS_R)
@pytest.mark.parametrize("case", CONV_CASES, ids=str)
def test_conv1d_stream_rows_bitwise(dev, case, Rn):
    from csm.hip import ops
    C_in, C_out, k, dil, groups, elu, use_res, use_bias = case
    H = (k - 1) * dil
    g = torch.Generator().manual_seed(1000 + Rn)
    w = torch.randn(C_out, C_in // groups, k, generator=g).cuda()
    b = torch.randn(C_out, generator=g).cuda() if use_bias else None
    for n in ROWS_N:
        n_slots, slots, parity, _ = _rows_layout(Rn, n)
        arena = _guard(n_slots, 2, C_in, H) if H else None
        for r in range(Rn):
            if H:
                arena[slots[r], parity[r]] = torch.randn(C_in, H, generator=g).cuda()
        for step in range(2):                           # the history the first step writes is what the second reads
            par = [p ^ step for p in parity]
            x = torch.randn(Rn, C_in, n, generator=g).cuda()
            res = torch.randn(Rn, C_out, n, generator=g).cuda() if use_res else None
            expect = arena.clone() if H else None
            y = _nan(Rn, C_out, n)
            ops.conv1d_stream_rows_f32(arena, x, w, b, y, slots, par, dil, elu, res)
            for r in range(Rn):
                y1 = _nan(C_out, n)
                h_in = expect[slots[r], par[r]].clone() if H else None
                h_out = _nan(C_in, H) if H else None
                ops.conv1d_stream_f32(h_in, x[r].contiguous(), w, b, y1, h_out, dil, elu, None if res is None else res[r].contiguous())
                assert _same(y[r], y1), (case, Rn, n, step, r)
                if H:
                    expect[slots[r], par[r] ^ 1] = h_out
            if H:                                       # next histories; unnamed slots and the read halves keep their bits
                assert _same(arena, expect), (case, Rn, n, step)


@pytest.mark.parametrize("Rn", ROWS_R)
@pytest.mark.parametrize("case", CONVT_CASES, ids=str)
def test_conv_transpose1d_stream_rows_bitwise(dev, case, Rn):
    from csm.hip import ops
    C_in, C_out, k, s, groups, elu, use_bias = case
    H = (k - 1) // s
    g = torch.Generator().manual_seed(2000 + Rn)
    w = torch.randn(C_in, C_out // groups, k, generator=g).cuda()
    b = torch.randn(C_out, generator=g).cuda() if use_bias else None
    for n in ROWS_N:
        n_slots, slots, parity, pos = _rows_layout(Rn, n)
        pos[0] = 0                                      # one row at the start of its stream: the taps before position 0 are skipped
        arena = _guard(n_slots, 2, C_in, H) if H else None
        for r in range(Rn):
            if H:
                arena[slots[r], parity[r]] = torch.randn(C_in, H, generator=g).cuda()
        for step in range(2):
            par = [p ^ step for p in parity]
            p0 = [p + step * n for p in pos]
            x = torch.randn(Rn, C_in, n, generator=g).cuda()
            expect = arena.clone() if H else None
            y = _nan(Rn, C_out, n * s)
            ops.conv_transpose1d_stream_rows_f32(arena, x, w, b, y, slots, par, p0, s, groups, elu)
            for r in range(Rn):
                y1 = _nan(C_out, n * s)
                h_in = expect[slots[r], par[r]].clone() if H else None
                h_out = _nan(C_in, H) if H else None
                ops.conv_transpose1d_stream_f32(h_in, x[r].contiguous(), w, b, y1, h_out, p0[r], s, groups, elu)
                assert _same(y[r], y1), (case, Rn, n, step, r)
                if H:
                    expect[slots[r], par[r] ^ 1] = h_out
            if H:
                assert _same(arena, expect), (case, Rn, n, step)


@pytest.mark.parametrize("Rn", ROWS_R)
def test_attn_window_stream_rows_bitwise(dev, Rn):
    from csm.hip import ops
    H, window = 2, 37
    D = H * R.ATTN_HD
    g = torch.Generator().manual_seed(3000 + Rn)
    for n in ROWS_N:
        n_slots, slots, _, pos = _rows_layout(Rn, n)
        pos[0] = 0
        ring = window + n - 1
        kc = torch.randn(n_slots, ring, D, generator=g).cuda()
        vc = torch.randn(n_slots, ring, D, generator=g).cuda()
        for step in range(2):
            p0 = [p + step * n for p in pos]
            qkv = torch.randn(Rn * n, 3 * D, generator=g).cuda()
            ek, ev = kc.clone(), vc.clone()
            out = _nan(Rn * n, D)
            ops.attn_window_stream_rows_f32(qkv, kc, vc, out, slots, p0, n, H, window)
            for r in range(Rn):
                o1 = _nan(n, D)
                k1, v1 = ek[slots[r]].clone(), ev[slots[r]].clone()
                ops.attn_window_stream_f32(qkv[r * n:(r + 1) * n].contiguous(), k1, v1, o1, p0[r], H, window)
                assert _same(out[r * n:(r + 1) * n], o1), (Rn, n, step, r)
                ek[slots[r]], ev[slots[r]] = k1, v1
            assert _same(kc, ek) and _same(vc, ev), (Rn, n, step)


@pytest.mark.parametrize("Rn", ROWS_R)
@pytest.mark.parametrize("geom", R.ROPE_GEOMS, ids=str)
def test_rope_half_rows_bitwise(dev, geom, Rn):
    from csm.hip import ops
    H, hd = geom
    for n in ROWS_N:
        _, _, _, pos = _rows_layout(Rn, n)
        pos[-1] = 4095
        qkv = R.rope_inputs(Rn * n, H, hd, n)
        got = ops.rope_half_rows_f32(qkv.cuda(), pos, n, H, R.ROPE_BASE)
        for r in range(Rn):
            assert _same(got[r * n:(r + 1) * n], _rope_gpu(qkv[r * n:(r + 1) * n], H, hd, pos[r])), (geom, Rn, n, r)


# ------------------------------------------------------------------------------------------------------------- refusals
def _refused(rc, *untouched):
    """An argument check turned the call down (1 - not a failed launch, 2) and nothing was written."""
    torch.cuda.synchronize()
    assert rc == 1, rc
    for t, before in untouched:
        assert _same(t, before)


def _ints(v):
    import ctypes
    return (ctypes.c_int * len(v))(*v)


def test_refusals_conv(dev):
    """Every probe has valid buffers behind it, sized for the call as if it were accepted."""
    from csm.hip import lib
    x, w, b = torch.randn(6, 8).cuda(), torch.randn(6, 6, 3).cuda(), torch.randn(6).cuda()
    y = _nan(6, 16)
    y0 = y.clone()
    h, h2 = torch.zeros(6, 2, device="cuda"), _nan(6, 2)
    arena = _guard(3, 2, 6, 2)
    a0 = arena.clone()
    one, zero = _ints([0]), _ints([0])
    s = _s()
    # a null output
    _refused(lib.csm_conv1d_f32(_p(x), _p(w), _p(b), None, None, 6, 6, 8, 8, 3, 1, 1, 2, 0, 1, 0, s))
    _refused(lib.csm_conv_transpose1d_f32(_p(x), _p(w), _p(b), None, 6, 6, 8, 16, 3, 2, 0, 1, 0, s))
    _refused(lib.csm_conv1d_stream_f32(_p(h), _p(x), _p(w), _p(b), None, None, _p(h2), 6, 6, 8, 3, 1, 1, 0, s), (h2, _nan(6, 2)))
    _refused(lib.csm_conv_transpose1d_stream_f32(_p(h), _p(x), _p(w), _p(b), None, _p(h2), 6, 6, 8, 0, 3, 1, 1, 0, s), (h2, _nan(6, 2)))
    # groups that do not divide the channels (4 does not divide 6; w holds enough for any reading of it)
    _refused(lib.csm_conv1d_f32(_p(x), _p(w), _p(b), None, _p(y), 6, 6, 8, 8, 3, 1, 1, 2, 0, 4, 0, s), (y, y0))
    _refused(lib.csm_conv_transpose1d_f32(_p(x), _p(w), _p(b), _p(y), 6, 6, 8, 16, 3, 2, 0, 4, 0, s), (y, y0))
    _refused(lib.csm_conv1d_stream_f32(_p(h), _p(x), _p(w), _p(b), None, _p(y), _p(h2), 6, 6, 8, 3, 1, 4, 0, s), (y, y0), (h2, _nan(6, 2)))
    _refused(lib.csm_conv_transpose1d_stream_f32(_p(h), _p(x), _p(w), _p(b), _p(y), _p(h2), 6, 6, 8, 0, 3, 1, 4, 0, s), (y, y0), (h2, _nan(6, 2)))
    _refused(lib.csm_conv1d_stream_strided_f32(_p(h), _p(x), _p(w), _p(b), None, _p(y), _p(h2), 6, 6, 8, 3, 1, 1, 4, 0, 0, s), (y, y0))
    _refused(lib.csm_conv1d_stream_rows_f32(_p(arena), _p(x), _p(w), _p(b), None, _p(y), 1, one, zero, 3, 6, 6, 8, 3, 1, 4, 0, s), (y, y0), (arena, a0))
    _refused(lib.csm_conv_transpose1d_stream_rows_f32(_p(arena), _p(x), _p(w), _p(b), _p(y), 1, one, zero, zero, 3, 6, 6, 8, 3, 1, 4, 0, s),
             (y, y0), (arena, a0))
    # the rows forms: a slot named twice, parity 2 (slot 0 of 3: even a kernel that took parity 2 would stay inside the arena)
    x2 = torch.randn(2, 6, 4).cuda()
    _refused(lib.csm_conv1d_stream_rows_f32(_p(arena), _p(x2), _p(w), _p(b), None, _p(y), 2, _ints([1, 1]), _ints([0, 1]), 3, 6, 6, 4, 3, 1, 1, 0, s),
             (y, y0), (arena, a0))
    _refused(lib.csm_conv1d_stream_rows_f32(_p(arena), _p(x2), _p(w), _p(b), None, _p(y), 1, _ints([0]), _ints([2]), 3, 6, 6, 4, 3, 1, 1, 0, s),
             (y, y0), (arena, a0))
    _refused(lib.csm_conv_transpose1d_stream_rows_f32(_p(arena), _p(x2), _p(w), _p(b), _p(y), 2, _ints([1, 1]), _ints([0, 1]), _ints([0, 0]), 3, 6, 6, 4,
                                                      3, 1, 1, 0, s), (y, y0), (arena, a0))
    _refused(lib.csm_conv_transpose1d_stream_rows_f32(_p(arena), _p(x2), _p(w), _p(b), _p(y), 1, _ints([0]), _ints([2]), _ints([0]), 3, 6, 6, 4, 3, 1,
                                                      1, 0, s), (y, y0), (arena, a0))


def test_refusals_dense(dev):
    from csm.hip import lib
    s = _s()
    x, w, b = torch.randn(4, 32).cuda(), torch.randn(32).cuda(), torch.randn(32).cuda()
    W = torch.randn(8, 32).cuda()
    _refused(lib.csm_layernorm_f32(_p(x), _p(w), _p(b), None, 4, 32, 1e-5, s))
    _refused(lib.csm_linear_f32(_p(x), _p(W), None, None, None, 4, 8, 32, 32, 0, s))
    y = _nan(4, 8)
    _refused(lib.csm_linear_f32(_p(x), _p(W), None, None, _p(y), 4, 8, 32, 31, 0, s), (y, _nan(4, 8)))          # ldx < K
    _refused(lib.csm_linear_f32(_p(x), _p(W), _p(w), None, _p(y), 4, 8, 32, 32, 0, s), (y, _nan(4, 8)))         # a scale without a residual
    _refused(lib.csm_transpose_f32(_p(x), None, 4, 32, s))
    _refused(lib.csm_transpose_rows_f32(_p(x), None, 1, 4, 32, s))
    _refused(lib.csm_rope_half_f32(None, 2, 1, 64, R.ROPE_BASE, 0, s))
    # an odd head_dim: qkv sized for it (T 2, H 2, hd 7)
    q = torch.randn(2, 3 * 2 * 7).cuda()
    q0 = q.clone()
    _refused(lib.csm_rope_half_f32(_p(q), 2, 2, 7, R.ROPE_BASE, 0, s), (q, q0))
    _refused(lib.csm_rope_half_rows_f32(_p(q), 2, _ints([0, 5]), 1, 2, 7, R.ROPE_BASE, s), (q, q0))
    # grid rows beyond 65535 blocks: R = 65535 * 32 + 1
    Rr = 65535 * 32 + 1
    big = torch.zeros(Rr, device="cuda")
    out = _nan(Rr)
    _refused(lib.csm_transpose_f32(_p(big), _p(out), Rr, 1, s))
    _refused(lib.csm_transpose_rows_f32(_p(big), _p(out), 1, Rr, 1, s))
    assert bool(torch.isnan(out).all())
    _refused(lib.csm_transpose_rows_f32(_p(big), _p(out), 65536, 4, 4, s))                                        # batch beyond the grid's depth
    assert bool(torch.isnan(out).all())


def test_refusals_attention(dev):
    from csm.hip import lib
    s = _s()
    one = _ints([0])

    def bufs(T, H, hd, ring, slots=1):
        D = H * hd
        return torch.randn(T, 3 * D).cuda(), _nan(slots, ring, D), _nan(slots, ring, D), _nan(T, D)

    def all_forms(T, H, hd, window, ring, full=True):
        qkv, kc, vc, out = bufs(T, H, hd, max(ring, 1))
        if full:
            _refused(lib.csm_attn_window_f32(_p(qkv), _p(out), T, H, hd, window, s))
        _refused(lib.csm_attn_window_stream_f32(_p(qkv), _p(kc), _p(vc), _p(out), T, 0, H, hd, window, ring, s))
        _refused(lib.csm_attn_window_stream_rows_f32(_p(qkv), _p(kc), _p(vc), _p(out), 1, one, one, 1, T, H, hd, window, ring, s))
        for t in (kc, vc, out):
            assert bool(torch.isnan(t).all())

    all_forms(2, 1, 128, 4, 5)                          # head_dim 128
    all_forms(2, 1, 64, 0, 1)                           # window 0
    all_forms(2, 1, 64, 8193, 8194)                     # window 8193
    all_forms(4, 1, 64, 5, 5 + 4 - 2, full=False)       # ring = window + n - 2
    qkv, kc, vc, out = bufs(2, 1, 64, 6)
    _refused(lib.csm_attn_window_f32(_p(qkv), None, 2, 1, 64, 4, s))
    _refused(lib.csm_attn_window_stream_f32(_p(qkv), _p(kc), _p(vc), None, 2, 0, 1, 64, 4, 6, s))
    assert bool(torch.isnan(kc).all())
    qkv2, kc2, vc2, out2 = bufs(4, 1, 64, 6, slots=3)   # two rows of n = 2 naming one slot
    _refused(lib.csm_attn_window_stream_rows_f32(_p(qkv2), _p(kc2), _p(vc2), _p(out2), 2, _ints([1, 1]), _ints([0, 3]), 3, 2, 1, 64, 4, 6, s))
    assert bool(torch.isnan(kc2).all()) and bool(torch.isnan(out2).all())
    # H = 65536: a grid dimension beyond 65535
    qkv, kc, vc, out = bufs(1, 65536, 64, 1)
    _refused(lib.csm_attn_window_f32(_p(qkv), _p(out), 1, 65536, 64, 1, s))
    _refused(lib.csm_attn_window_stream_f32(_p(qkv), _p(kc), _p(vc), _p(out), 1, 0, 65536, 64, 1, 1, s))
    _refused(lib.csm_attn_window_stream_rows_f32(_p(qkv), _p(kc), _p(vc), _p(out), 1, one, one, 1, 1, 65536, 64, 1, 1, s))
    for t in (kc, vc, out):
        assert bool(torch.isnan(t).all())
