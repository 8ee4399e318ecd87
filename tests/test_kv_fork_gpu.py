"""csm_kv_fork_rows (the rows form of DecodeState.resume_row) against plain strided copies: the destination's bits are the
sources', nothing outside positions [0, len) of the named rows is written, ``pos`` is ``len - 1`` on the named rows only, and
every refusal launches nothing."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LAYERS, B, S_MAX = 2, 17, 2048
GUARD = 0.1005859375
POS_GUARD = -7
SHAPES = [(8, 64), (2, 128), (1, 64)]                                # (KV, HD)
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 130, 2047, 2048]


def _bits(t):
    return t.view(torch.int16)


def _rows(R):
    return [(7 * r + 5) % 17 for r in range(R)]                      # 5, 12, 2, 9, 16, 6, ... : distinct mod 17, not sorted


def _lens(R):
    """R lengths out of LENS in which 1 and S_max both occur from R = 3 on (R = 1: S_max)."""
    order = [2048, 1, 65, 16, 2047, 2, 15, 17, 63, 64, 130, 1, 2048, 130, 17, 64]
    return order[:R]


def _parked(KV, HD, length, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(LAYERS, 2, KV, length, HD, generator=g, device="cuda").to(BF)


def _caches(KV, HD):
    kv = torch.full((LAYERS, 2, B, KV, S_MAX, HD), GUARD, dtype=BF, device="cuda")
    pos = torch.full((B,), POS_GUARD, dtype=torch.int32, device="cuda")
    return kv, pos


def _check(kv, pos, rows, parkeds):
    want = torch.full_like(kv, GUARD)
    want_pos = torch.full_like(pos, POS_GUARD)
    for b, p in zip(rows, parkeds):                                  # what R resume_row calls do: one strided copy each
        want[:, :, b, :, :p.shape[3]].copy_(p)
        want_pos[b] = p.shape[3] - 1
    assert torch.equal(pos, want_pos)
    assert torch.equal(_bits(kv), _bits(want))                       # named rows' [0, len) = the source; everything else the guard


@pytest.mark.parametrize("KV,HD", SHAPES)
@pytest.mark.parametrize("R", [1, 3, 16])
def test_fork_rows_equals_strided_copies(dev, KV, HD, R):
    """Distinct sources (R = 16: sixteen of them), mixed lengths, cache rows in non-ascending order."""
    from csm.hip import ops
    rows, lens = _rows(R), _lens(R)
    assert len(set(rows)) == R and (R == 1 or {1, S_MAX} <= set(lens))
    parkeds = [_parked(KV, HD, n, seed=100 * R + r) for r, n in enumerate(lens)]
    before = [p.clone() for p in parkeds]
    kv, pos = _caches(KV, HD)
    ops.kv_fork_rows(parkeds, kv, pos, rows)
    _check(kv, pos, rows, parkeds)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(parkeds, before))


@pytest.mark.parametrize("KV,HD", SHAPES)
@pytest.mark.parametrize("length", [1, 130, S_MAX])
def test_fork_rows_sixteen_rows_from_one_source(dev, KV, HD, length):
    from csm.hip import ops
    rows = _rows(16)
    src = _parked(KV, HD, length, seed=length)
    kv, pos = _caches(KV, HD)
    ops.kv_fork_rows([src] * 16, kv, pos, rows)
    _check(kv, pos, rows, [src] * 16)


def test_fork_rows_mixes_shared_and_own_sources(dev):
    from csm.hip import ops
    KV, HD = 8, 64
    a, b = _parked(KV, HD, 65, seed=1), _parked(KV, HD, 17, seed=2)
    parkeds = [a, b, a, a, b]
    kv, pos = _caches(KV, HD)
    ops.kv_fork_rows(parkeds, kv, pos, _rows(5))
    _check(kv, pos, _rows(5), parkeds)


def test_fork_rows_bad_arguments(dev):
    from csm.hip import CsmHipError, check, lib, ops
    KV, HD, s_max, nb = 2, 64, 64, 3
    kv = torch.full((LAYERS, 2, nb, KV, s_max, HD), GUARD, dtype=BF, device="cuda")
    pos = torch.full((nb,), POS_GUARD, dtype=torch.int32, device="cuda")
    kv0, pos0 = kv.clone(), pos.clone()
    big = torch.zeros(LAYERS * 2 * KV * s_max * HD + 64, dtype=BF, device="cuda")
    src = big[:LAYERS * 2 * KV * 8 * HD]
    stream = torch.cuda.current_stream().cuda_stream

    def raw(srcs=(src.data_ptr(), src.data_ptr()), rows=(1, 0), lens=(8, 8), R=None, hd=HD, cache=kv.data_ptr(),
            p=pos.data_ptr(), tab=True, srctab=True):
        ptr, arr = ctypes.c_void_p * 17, ctypes.c_int * 17
        return lib.csm_kv_fork_rows(ptr(*srcs) if srctab else None, cache, p, arr(*rows) if tab else None, arr(*lens),
                                    len(rows) if R is None else R, LAYERS, nb, KV, hd, s_max, stream)

    def refused(rc, *words):
        msg = lib.csm_last_error()
        assert rc == 1 and msg.startswith(b"csm_kv_fork_rows") and all(w in msg for w in words), (rc, msg)

    refused(raw(srctab=False), b"null pointer")
    refused(raw(cache=None), b"null pointer")
    refused(raw(p=None), b"null pointer")
    refused(raw(tab=False), b"null pointer")
    refused(raw(srcs=(src.data_ptr(), None)), b"segment 1", b"null pointer")
    refused(raw(srcs=(), rows=(), lens=()), b"0 segments")
    refused(raw(R=17), b"17 segments")
    refused(raw(lens=(8, 0)), b"0 positions outside 1 .. S_max = 64")
    refused(raw(lens=(-1, 8)), b"positions outside")
    refused(raw(lens=(8, s_max + 1)), b"65 positions outside 1 .. S_max = 64")
    refused(raw(rows=(0, nb)), b"batch row 3 outside the caches (3 rows)")
    refused(raw(rows=(-1, 0)), b"batch row -1 outside the caches")
    refused(raw(rows=(1, 1)), b"batch row 1 appears in two segments")
    refused(raw(hd=32), b"head_dim 32 unsupported")
    refused(raw(srcs=(src.data_ptr(), src.data_ptr() + 2)), b"segment 1", b"16-byte aligned")
    row1 = kv[0, 0, 1]                                                  # a source inside the destination cache
    refused(raw(srcs=(src.data_ptr(), row1.data_ptr())), b"segment 1", b"overlaps the cache")
    refused(raw(srcs=(kv.data_ptr() + kv.numel() * 2 - 16, src.data_ptr())), b"segment 0", b"overlaps the cache")
    with pytest.raises(CsmHipError, match="2 parked histories for 1 rows"):
        ops.kv_fork_rows([src.view(LAYERS, 2, KV, 8, HD)] * 2, kv, pos, [0])
    with pytest.raises(AssertionError):
        ops.kv_fork_rows([src.view(LAYERS, 2, KV, 8, HD).float()], kv, pos, [0])
    with pytest.raises(AssertionError):
        ops.kv_fork_rows([src.view(LAYERS, 2, KV, 8, HD)[:, :, :, :4]], kv, pos, [0])            # not contiguous
    with pytest.raises(AssertionError):
        ops.kv_fork_rows([src.view(LAYERS, 2, KV, 8, HD).cpu()], kv, pos, [0])
    with pytest.raises(AssertionError):
        ops.kv_fork_rows([src.view(LAYERS, 2, 1, 16, HD)], kv, pos, [0])                         # another model's shape
    torch.cuda.synchronize()
    assert torch.equal(_bits(kv), _bits(kv0)) and torch.equal(pos, pos0)                         # nothing was launched
    full = big[:LAYERS * 2 * KV * s_max * HD].view(LAYERS, 2, KV, s_max, HD)
    check(raw(srcs=(src.data_ptr(), full.data_ptr()), lens=(8, s_max)), "csm_kv_fork_rows")      # the longest legal length is fine
    torch.cuda.synchronize()
    assert pos.tolist() == [s_max - 1, 7, POS_GUARD] and torch.equal(_bits(kv[:, :, 2]), _bits(kv0[:, :, 2]))
