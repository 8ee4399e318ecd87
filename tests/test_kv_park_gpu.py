"""csm_kv_park_rows (the rows form of DecodeState.park_row, the mirror of csm_kv_fork_rows) against plain strided copies: each
destination's bits are ``kv[:, :, b, :, :len]``, nothing around the destinations is written, the cache and ``pos`` are untouched,
``fork(park(x))`` restores a row, and every refusal launches nothing.  And csm_sample_hist_move_rows: the samplers' rings and
frame counters to a packed buffer and back into other rows."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LAYERS, B, S_MAX = 2, 17, 2048
GUARD = 0.1005859375
POS_GUARD = -7
SHAPES = [(8, 64), (2, 128), (1, 64)]                                # (KV, HD)
PAD = 24                                                             # guard elements (48 bytes) before, between and after


def _bits(t):
    return t.view(torch.int16)


def _rows(R):
    return [(7 * r + 5) % 17 for r in range(R)]                      # 5, 12, 2, 9, 16, 6, ... : distinct mod 17, not sorted


def _lens(R):
    """R lengths out of 1, 2, 15, 16, 17, 63, 64, 65, 130, 2047, 2048 in which 1 and S_max both occur from R = 3 on."""
    order = [2048, 1, 65, 16, 2047, 2, 15, 17, 63, 64, 130, 1, 2048, 130, 17, 64]
    return order[:R]


def _cache(KV, HD, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(LAYERS, 2, B, KV, S_MAX, HD, generator=g, device="cuda").to(BF)


def _park_into_guard(kv, rows, lens):
    """The raw call with the destinations laid out inside ONE guard-filled buffer, PAD guard elements around each.  Returns
    (the buffer, [(offset, elements)] per destination)."""
    from csm.hip import check, lib
    layers, _, _, KV, s_max, HD = kv.shape
    sizes = [layers * 2 * KV * n * HD for n in lens]
    offs, at = [], PAD
    for n in sizes:
        offs.append(at)
        at += n + PAD                                               # (PAD * 2 bytes = 48: every destination stays 16-byte aligned)
    buf = torch.full((at,), GUARD, dtype=BF, device="cuda")
    R = len(rows)
    ptr, arr = ctypes.c_void_p * R, ctypes.c_int * R
    check(lib.csm_kv_park_rows(ptr(*[buf.data_ptr() + 2 * o for o in offs]), kv.data_ptr(), arr(*rows), arr(*lens), R, layers,
                               kv.shape[2], KV, HD, s_max, torch.cuda.current_stream().cuda_stream), "csm_kv_park_rows")
    return buf, list(zip(offs, sizes))


@pytest.mark.parametrize("KV,HD", SHAPES)
@pytest.mark.parametrize("R", [1, 3, 16])
def test_park_rows_equals_strided_copies(dev, KV, HD, R):
    rows, lens = _rows(R), _lens(R)
    assert len(set(rows)) == R and (R == 1 or {1, S_MAX} <= set(lens))
    kv = _cache(KV, HD, seed=10 * R + KV)
    kv0 = kv.clone()
    buf, where = _park_into_guard(kv, rows, lens)
    want = torch.full_like(buf, GUARD)
    for b, n, (o, size) in zip(rows, lens, where):
        want[o:o + size] = kv0[:, :, b, :, :n].contiguous().reshape(-1)          # what park_row does: one strided copy
    assert torch.equal(_bits(buf), _bits(want))                                   # the destinations' bits, the guard intact
    assert torch.equal(_bits(kv), _bits(kv0))                                     # the cache is only read


@pytest.mark.parametrize("KV,HD", SHAPES)
def test_fork_of_park_restores_a_scrambled_row(dev, KV, HD):
    from csm.hip import ops
    rows, lens = _rows(3), [130, 2048, 1]
    kv = _cache(KV, HD, seed=KV)
    kv0 = kv.clone()
    pos = torch.full((B,), POS_GUARD, dtype=torch.int32, device="cuda")
    parked = ops.kv_park_rows(kv, rows, lens)
    assert torch.equal(pos, torch.full_like(pos, POS_GUARD))                       # (pos is no argument of the park)
    assert [tuple(p.shape) for p in parked] == [(LAYERS, 2, KV, n, HD) for n in lens]
    for b, n, p in zip(rows, lens, parked):
        assert torch.equal(_bits(p), _bits(kv0[:, :, b, :, :n]))
        kv[:, :, b, :, :n] = 3.0                                                   # scramble what was parked
    ops.kv_fork_rows(parked, kv, pos, rows)
    assert torch.equal(_bits(kv), _bits(kv0))
    assert [pos[b].item() for b in rows] == [n - 1 for n in lens]
    # into OTHER rows: what a resumed request finds in its new slot
    other = [0, 1, 3]
    ops.kv_fork_rows(parked, kv, pos, other)
    for b, o, n in zip(rows, other, lens):
        assert torch.equal(_bits(kv[:, :, o, :, :n]), _bits(kv0[:, :, b, :, :n]))


def test_park_rows_bad_arguments(dev):
    from csm.hip import CsmHipError, check, lib, ops
    KV, HD, s_max, nb = 2, 64, 64, 3
    kv = torch.randn(LAYERS, 2, nb, KV, s_max, HD, device="cuda").to(BF)
    per = LAYERS * 2 * KV * HD                                          # elements per position
    big = torch.full((2 * per * s_max + 64,), GUARD, dtype=BF, device="cuda")
    big0 = big.clone()
    d0, d1 = big.data_ptr(), big.data_ptr() + 2 * per * s_max           # two destinations that can hold s_max positions each
    stream = torch.cuda.current_stream().cuda_stream

    def raw(dsts=(d0, d1), rows=(1, 0), lens=(8, 8), R=None, hd=HD, cache=kv.data_ptr(), tab=True, dsttab=True, lentab=True,
            layers=LAYERS, B=nb, kv_heads=KV, S=s_max):
        ptr, arr = ctypes.c_void_p * 17, ctypes.c_int * 17
        return lib.csm_kv_park_rows(ptr(*dsts) if dsttab else None, cache, arr(*rows) if tab else None, arr(*lens) if lentab else None,
                                    len(rows) if R is None else R, layers, B, kv_heads, hd, S, stream)

    def refused(rc, *words):
        msg = lib.csm_last_error()
        assert rc == 1 and msg.startswith(b"csm_kv_park_rows") and all(w in msg for w in words), (rc, msg)

    refused(raw(dsttab=False), b"null pointer")
    refused(raw(cache=None), b"null pointer")
    refused(raw(tab=False), b"null pointer")
    refused(raw(lentab=False), b"null pointer")
    refused(raw(dsts=(d0, None)), b"segment 1", b"null pointer")
    refused(raw(dsts=(), rows=(), lens=()), b"0 segments")
    refused(raw(R=17), b"17 segments")
    refused(raw(lens=(8, 0)), b"0 positions outside 1 .. S_max = 64")
    refused(raw(lens=(-1, 8)), b"positions outside")
    refused(raw(lens=(8, s_max + 1)), b"65 positions outside 1 .. S_max = 64")
    refused(raw(rows=(0, nb)), b"batch row 3 outside the caches (3 rows)")
    refused(raw(rows=(-1, 0)), b"batch row -1 outside the caches")
    refused(raw(rows=(1, 1)), b"batch row 1 appears in two segments")
    refused(raw(hd=32), b"head_dim 32 unsupported")
    refused(raw(layers=0), b"bad shape layers=0 B=3 KV=2 S_max=64")
    refused(raw(layers=-1), b"bad shape layers=-1")
    refused(raw(B=0), b"bad shape layers=2 B=0")
    refused(raw(kv_heads=0), b"bad shape", b"KV=0")
    refused(raw(S=0), b"bad shape", b"S_max=0")
    refused(raw(S=(1 << 24) + 1), b"bad shape", b"S_max=16777217")
    refused(raw(layers=1 << 30, kv_heads=2), b"bad shape layers=1073741824")                       # layers * 2 * KV past an int
    refused(raw(dsts=(d0, d1 + 2)), b"segment 1", b"16-byte aligned")
    refused(raw(cache=kv.data_ptr() + 2), b"the cache must be 16-byte aligned")
    refused(raw(dsts=(d0, kv[0, 0, 1].data_ptr())), b"segment 1", b"overlaps the cache")           # a destination inside the cache
    refused(raw(dsts=(kv.data_ptr() + kv.numel() * 2 - 16, d1)), b"segment 0", b"overlaps the cache")
    refused(raw(dsts=(d0, d0 + 2 * per * 8 - 16)), b"segments 0 and 1 overlap")                   # the last 16 bytes of the first
    refused(raw(dsts=(d0, d0)), b"segments 0 and 1 overlap")
    with pytest.raises(CsmHipError, match="1 lengths for 2 rows"):
        ops.kv_park_rows(kv, [0, 1], [8])
    with pytest.raises(AssertionError):
        ops.kv_park_rows(kv.float(), [0], [8])
    with pytest.raises(AssertionError):
        ops.kv_park_rows(kv[:, :, :, :, :32], [0], [8])                                             # not contiguous
    with pytest.raises(CsmHipError, match="positions outside"):
        ops.kv_park_rows(kv, [0], [s_max + 1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(big), _bits(big0))                                                    # nothing was launched
    check(raw(dsts=(d0, d0 + 2 * per * 8), lens=(8, s_max)), "csm_kv_park_rows")                  # adjacent, the longest legal length
    torch.cuda.synchronize()
    assert torch.equal(_bits(big[:per * 8]), _bits(kv[:, :, 1, :, :8].contiguous().reshape(-1)))
    assert torch.equal(_bits(big[per * 8:per * (8 + s_max)]), _bits(kv[:, :, 0].contiguous().reshape(-1)))
    assert torch.equal(_bits(big[per * (8 + s_max):]), _bits(big0[per * (8 + s_max):]))


# ---- the samplers' rings ----------------------------------------------------------------------------------------------------
HIST = 64


def _rings(K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hist = torch.randint(0, 2051, (B, K, HIST), generator=g, device="cuda", dtype=torch.int32)
    frame = torch.randint(0, 100000, (B,), generator=g, device="cuda", dtype=torch.int32)
    live = torch.randint(0, 2, (B,), generator=g, device="cuda", dtype=torch.int32)
    return hist, frame, live


@pytest.mark.parametrize("K", [32, 4])
@pytest.mark.parametrize("R", [1, 3, 16])
def test_hist_move_rows_out_and_back_into_other_rows(dev, K, R):
    from csm.hip import ops
    hist, frame, live = _rings(K, seed=K + R)
    hist0, frame0, live0 = hist.clone(), frame.clone(), live.clone()
    rows = _rows(R)
    packed = torch.full((R, K * HIST + 1), -5, dtype=torch.int32, device="cuda")
    assert ops.sample_hist_move_rows(hist, frame, packed, rows, False) is packed
    for r, b in enumerate(rows):
        assert torch.equal(packed[r, :-1], hist0[b].reshape(-1)) and packed[r, -1] == frame0[b]
    assert torch.equal(hist, hist0) and torch.equal(frame, frame0)                  # towards the packed buffer the state is only read
    other = [(b + 3) % B for b in rows]                                             # distinct again, mostly rows that were not named
    packed0 = packed.clone()
    ops.sample_hist_move_rows(hist, frame, packed, other, True)
    want_h, want_f = hist0.clone(), frame0.clone()
    for b, o in zip(rows, other):
        want_h[o], want_f[o] = hist0[b], frame0[b]
    assert torch.equal(hist, want_h) and torch.equal(frame, want_f)                 # the named rows, and only they
    assert torch.equal(packed, packed0) and torch.equal(live, live0)                # (hist_live is no argument: nothing can reach it)


def test_hist_move_rows_bad_arguments(dev):
    from csm.hip import lib, ops
    K, R = 4, 2
    hist, frame, _ = _rings(K, seed=1)
    hist0, frame0 = hist.clone(), frame.clone()
    packed = torch.full((R, K * HIST + 1), -5, dtype=torch.int32, device="cuda")
    packed0 = packed.clone()
    stream = torch.cuda.current_stream().cuda_stream

    def raw(h=hist.data_ptr(), f=frame.data_ptr(), p=packed.data_ptr(), rows=(1, 0), R=None, nb=B, k=K, to_state=1, tab=True):
        arr = ctypes.c_int * 17
        return lib.csm_sample_hist_move_rows(h, f, p, arr(*rows) if tab else None, len(rows) if R is None else R, nb, k, to_state, stream)

    def refused(rc, *words):
        msg = lib.csm_last_error()
        assert rc == 1 and msg.startswith(b"csm_sample_hist_move_rows") and all(w in msg for w in words), (rc, msg)

    for kw in ({"h": None}, {"f": None}, {"p": None}, {"tab": False}):
        refused(raw(**kw), b"null pointer")
    refused(raw(rows=()), b"0 rows (1 to 16)")
    refused(raw(R=17), b"17 rows")
    refused(raw(nb=0), b"bad shape")
    refused(raw(k=0), b"bad shape")
    refused(raw(k=4097), b"bad shape B=17 K=4097")
    refused(raw(to_state=2), b"direction 2")
    refused(raw(rows=(0, B)), b"batch row 17 outside the state (17 rows)")
    refused(raw(rows=(-1, 0)), b"batch row -1 outside")
    refused(raw(rows=(3, 3)), b"batch row 3 appears in two entries")
    refused(raw(p=packed.data_ptr() + 2), b"4-byte aligned")
    refused(raw(p=hist[5].data_ptr()), b"overlaps the state")
    refused(raw(p=frame.data_ptr()), b"overlaps the state")
    for to_state in (0, 1):
        refused(raw(rows=(0, B), to_state=to_state), b"outside the state")
    with pytest.raises(AssertionError):
        ops.sample_hist_move_rows(hist, frame, packed[:1], [0, 1], True)                           # one packed row for two rows
    with pytest.raises(AssertionError):
        ops.sample_hist_move_rows(hist.long(), frame, packed, [0, 1], True)
    torch.cuda.synchronize()
    assert torch.equal(hist, hist0) and torch.equal(frame, frame0) and torch.equal(packed, packed0)   # nothing was launched
