"""The device resampler's host side (csm/codec/resample.py), without a GPU: the table ``design`` builds is the kernel of
``csm.data.resample``, the geometry is the documented one, the streaming schedule emits every output exactly once and never one
whose taps reach past what was fed, the C ABI carries the three new symbols, and the public surfaces refuse bad rates at the call."""
import ctypes
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from csm.codec import resample as R
from csm.data.training_data import resample as host_resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 24000), (16000, 24000), (8000, 24000), (44100, 24000), (24000, 48000), (24000, 16000), (24000, 8000),
         (24000, 44100)]
GEOMETRY = {(48000, 24000): (2, 1, 13, 28), (16000, 24000): (2, 3, 7, 16), (8000, 24000): (1, 3, 7, 15),
            (44100, 24000): (147, 80, 12, 171), (24000, 48000): (1, 2, 7, 15), (24000, 16000): (3, 2, 10, 23),
            (24000, 8000): (3, 1, 19, 41), (24000, 44100): (80, 147, 7, 94)}


def apply64(x, o, n, width, taps):
    """The documented sum in float64 numpy: y[j] = sum_t taps[j mod n][t] * xbar[(j div n) * o - width + t]."""
    N = x.shape[0]
    T = 2 * width + o
    M = -(-n * N // o)
    blocks = -(-M // n)
    xb = np.zeros(width + blocks * o + T, dtype=np.float64)
    xb[width:width + N] = x
    y = np.empty(blocks * n, dtype=np.float64)
    for q in range(blocks):
        y[q * n:(q + 1) * n] = taps @ xb[q * o:q * o + T]
    return y[:M]


@pytest.mark.parametrize("pair", PAIRS + [(22050, 24000)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_design_reproduces_host_resample(pair):
    o, n, width, taps = R.design(*pair)
    assert taps.dtype == np.float64 and taps.shape == (n, 2 * width + o)
    g = torch.Generator().manual_seed(pair[0] + pair[1])
    for N in (1, 37, 5003):
        x = torch.randn(N, generator=g, dtype=torch.float64)
        ref = host_resample(x, *pair).numpy()
        got = apply64(x.numpy(), o, n, width, taps)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12, (pair, N, np.abs(got - ref).max())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_geometry_table(pair):
    assert R.geometry(*pair) == GEOMETRY[pair]
    o, n, width, taps = R.design(*pair)
    assert (o, n, width, taps.shape[1]) == GEOMETRY[pair]
    assert n * taps.shape[1] * 4 <= 55 * 1024 + 512          # "the largest table is 55 KB"


@pytest.mark.parametrize("pair", PAIRS + [(22050, 24000)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_schedule_emits_every_output_once_and_never_early(pair):
    o, n, width, T = R.geometry(*pair)
    rng = random.Random(pair[0] * 7 + pair[1])
    for N in (1, width, width + o - 1, width + o, 2 * T + 3, 1920, 5003):
        for cut in ("random", "ones", "whole"):
            pos, emitted, left = 0, 0, N
            while left:
                k = {"random": rng.randint(1, 400), "ones": 1, "whole": left}[cut]
                k = min(k, left)
                m = R.step_outputs(pos, k, False, o, n, width)
                assert m >= 0 and m % n == 0 and m <= R.max_step_outputs(k, o, n, width)
                pos, left, emitted = pos + k, left - k, emitted + m
                assert emitted == n * R.ready_blocks(pos, o, width)
                if emitted:                                   # the last input sample the newest output's taps touch was fed
                    q = emitted // n - 1
                    assert q * o - width + T - 1 <= pos - 1
                # ... and the next block is NOT computable yet: nothing is held back beyond the lag
                assert (emitted // n) * o - width + T - 1 > pos - 1
                # the carry of T - 1 samples reaches back to the first sample of the next block
                assert pos - (T - 1) <= (emitted // n) * o - width
            tail = R.step_outputs(pos, 0, True, o, n, width)
            assert tail >= 0 and tail <= R.max_step_outputs(1, o, n, width)
            assert emitted + tail == math.ceil(n * N / o) == R.out_len(N, o, n)
    assert R.step_outputs(0, 0, True, o, n, width) == 0       # a flush on an empty stream


def test_abi_has_the_three_symbols_and_is_still_3():
    from csm import hip
    names = ("csm_resample_f32", "csm_resample_stream_f32", "csm_resample_stream_rows_f32")
    header = open(os.path.join(ROOT, "include", "csm_hip.h")).read()
    so = ctypes.CDLL(hip.LIB_PATH)
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hip.EXPORTS
        assert getattr(so, name) is not None
    assert hip.lib.csm_abi_version() == 3


def test_kernel_entry_points_refuse_without_a_device():
    """The argument checks come before any launch, so they can be exercised with null pointers and no GPU."""
    from csm import hip
    lib = hip.lib
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    L = lambda *v: (ctypes.c_longlong * len(v))(*v)
    P = lambda *v: (ctypes.c_void_p * len(v))(*v)

    def rows(R_=2, slots=(0, 1), parity=(0, 0), n_in=(4, 4), pos=(0, 0), mask=0, n_slots=4, max_in=8, o=2, n=3, width=7, ldy=64):
        return lib.csm_resample_stream_rows_f32(None, P(*([1] * len(slots))), None, None, ldy, R_, I(*slots), I(*parity), I(*n_in),
                                                L(*pos), mask, n_slots, max_in, o, n, width, None)

    assert rows(R_=0) == 1 and rows(R_=17, slots=tuple(range(17)), parity=(0,) * 17, n_in=(4,) * 17, pos=(0,) * 17, n_slots=32) == 1
    assert rows(slots=(0, 4)) == 1 and rows(slots=(-1, 0)) == 1            # out of range
    assert rows(slots=(1, 1)) == 1                                         # named twice
    assert b"twice" in lib.csm_last_error()
    assert rows(parity=(0, 2)) == 1
    assert rows(mask=0b100) == 1                                           # a bit at R
    assert rows(n_in=(4, 9)) == 1                                          # above max_in
    assert rows(n_in=(4, 0)) == 1                                          # nothing new without the final bit
    assert rows(pos=(0, -1)) == 1
    assert rows(ldy=2) == 1                                                # would emit more than y holds
    assert rows(o=3, n=3) == 1 and b"equal rates" in lib.csm_last_error()
    assert rows(o=4, n=6) == 1                                             # not in lowest terms
    assert rows(o=44101, n=24000, width=12) == 1                           # T over the limit
    assert rows(o=1999, n=4001, width=12) == 1                             # table over the limit
    assert lib.csm_resample_f32(None, None, None, 1, 16, 3, 3, 7, None) == 1
    assert lib.csm_resample_f32(None, None, None, 0, 16, 2, 3, 7, None) == 1
    assert lib.csm_resample_f32(None, None, None, 1, 16, 2, 3, 7, None) == 1   # null pointers with work to do
    assert lib.csm_resample_f32(None, None, None, 1, 0, 2, 3, 7, None) == 0    # N = 0: nothing to launch
    assert lib.csm_resample_stream_f32(None, 2, None, 4, 0, 0, None, None, 64, 8, 2, 3, 7, None) == 1


@pytest.mark.parametrize("bad", [(0, 24000), (24000, 0), (-8000, 24000), (24000.0, 16000), (True, 24000), (None, 24000)])
def test_bad_rates_raise(bad):
    with pytest.raises(ValueError):
        R.geometry(*bad)
    with pytest.raises(ValueError):
        R.design(*bad)


def test_equal_rates_and_oversized_tables_raise():
    with pytest.raises(ValueError, match="equal rates"):
        R.geometry(24000, 24000)
    with pytest.raises(ValueError, match="at most"):
        R.geometry(44101, 24000)                               # coprime rates: 44125 taps per phase
    with pytest.raises(ValueError, match="at most"):
        R.geometry(1999, 4001)                                 # 2011 taps x 4001 phases: over the entry limit
    with pytest.raises(ValueError):
        R.Resampler(24000, 24000, device="cpu")
    with pytest.raises(ValueError):
        R.Resampler(44101, 24000, device="cpu")
    assert R.rate_resampler("sample_rate", None, 24000, "cpu", True) is None
    assert R.rate_resampler("sample_rate", 24000, 24000, "cpu", True) is None


class _Codec:
    sample_rate = 24000

    def encode_stream(self):
        raise AssertionError("hear(sample_rate=0) must raise before it makes a stream")

    def decode_stream_rows(self, *a, **k):
        raise AssertionError("serve(output_sample_rate=-1) must raise before it makes a decoder")


class _Gen:
    """As much of a Generator as the rate checks touch: they come first, before any model, cache or codec is used."""
    sample_rate, device = 24000, "cpu"
    _audio_tokenizer = _Codec()
    _run = 0

    def _out_resampler(self, rate):
        from csm.generator import Generator
        return Generator._out_resampler(self, rate)


def test_host_surfaces_refuse_bad_rates_at_the_call():
    from csm.conversation import Conversation, open_heard_turn
    from csm.generator import Generator
    from csm.serving import BatchServer, ServedConversation
    gen = _Gen()
    conv = Conversation.__new__(Conversation)
    conv._gen, conv._heard, conv._enc = gen, None, None
    for bad in (0, -16000, 16000.0, True):
        with pytest.raises(ValueError, match="sample_rate"):
            conv.hear(0, sample_rate=bad)
        with pytest.raises(ValueError, match="sample_rate"):
            open_heard_turn(conv, 0, bad)
    assert conv._heard is None
    for bad in (-1, 0, 48000.0):
        with pytest.raises(ValueError, match="output_sample_rate"):
            BatchServer(gen, output_sample_rate=bad)
        for call in (Generator.generate, Generator.generate_stream):
            with pytest.raises(ValueError, match="output_sample_rate"):
                call(gen, "hi", 0, [], output_sample_rate=bad)
        with pytest.raises(ValueError, match="output_sample_rate"):
            Generator.generate_batch(gen, ["hi"], [0], [[]], output_sample_rate=bad)
    with pytest.raises(ValueError, match="at most"):
        BatchServer(gen, output_sample_rate=44101)
    with pytest.raises(ValueError, match="at most"):
        conv.hear(0, sample_rate=44101)
    srv = BatchServer.__new__(BatchServer)
    srv._gen, srv._run, srv.hear_slots = gen, 0, 0
    sc = ServedConversation.__new__(ServedConversation)
    sc._srv, sc._gen, sc.closed, sc._heard, sc._enc = srv, gen, False, None, None
    with pytest.raises(ValueError, match="sample_rate"):
        sc.hear(0, sample_rate=0)
