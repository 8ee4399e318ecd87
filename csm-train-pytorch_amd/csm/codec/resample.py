"""Band-limited sample-rate conversion on the device: what ``csm.data.resample`` computes on the host in float64 (the
windowed-sinc interpolation of ``torchaudio.functional.resample``: ``sinc_interp_hann``, ``lowpass_filter_width=6``,
``rolloff=0.99``), as HIP kernels (csrc/resample.hip) in three forms that agree bit for bit:

  * ``Resampler(orig_sr, new_sr)(wav)``: one shot;
  * ``Resampler.stream()`` -> ``ResampleStream``: ``feed`` pieces of any length, ``flush`` at the end - the concatenated
    outputs equal the one-shot result however the input was cut;
  * ``Resampler.stream_rows()`` -> ``ResampleStreamRows``: up to 16 such streams advanced by ONE launch, each in its own slot.

For ``orig_sr -> new_sr`` with g = gcd, o = orig_sr / g, n = new_sr / g: ``width = ceil(6 * o / (min(o, n) * 0.99))``, T = 2 * width
+ o taps per phase, a table ``taps[n][T]`` built here in float64 and rounded once to fp32, and
    y[j] = sum_t taps[j mod n][t] * xbar[(j div n) * o - width + t],    j < M = ceil(n * N / o),
xbar = x inside [0, N) and 0 outside.  Output block q = j div n needs input up to q * o + width + o - 1, so after N' samples the
blocks q < ``ready_blocks(N')`` = max(0, floor((N' - width - o) / o) + 1) can be emitted: a stream lags its input by width + o
samples and ``flush`` emits the rest against zeros.  The schedule is integer arithmetic on the host (the kernels read nothing
back); ``design`` and the schedule import and run without a GPU.
"""
import math
from typing import List, Sequence

import torch

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
MAX_TAPS = 2048              # taps per phase the kernels take (T = 2 * width + o)
MAX_TABLE = 1 << 22          # table entries n * T the kernels take (16 MB of fp32)
F32 = torch.float32


def check_rate(name: str, rate) -> int:
    """A sample rate: an integer number of Hz >= 1 (bool refused: it is not a rate)."""
    if isinstance(rate, bool) or not isinstance(rate, int) or rate < 1:
        raise ValueError(f"{name} must be an integer number of Hz >= 1, got {rate!r}")
    return rate


def geometry(orig_sr: int, new_sr: int):
    """(o, n, width, T) of a rate pair.  Refused: rates that are no positive integers, equal rates, and a pair whose table
    exceeds what the kernels take (``MAX_TAPS`` taps per phase, ``MAX_TABLE`` entries)."""
    orig_sr, new_sr = check_rate("orig_sr", orig_sr), check_rate("new_sr", new_sr)
    if orig_sr == new_sr:
        raise ValueError(f"equal rates ({orig_sr} Hz): there is nothing to resample - pass the audio on as it is")
    g = math.gcd(orig_sr, new_sr)
    o, n = orig_sr // g, new_sr // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    T = 2 * width + o
    if T > MAX_TAPS or n * T > MAX_TABLE:
        raise ValueError(f"{orig_sr} -> {new_sr} Hz needs a table of {n} phases x {T} taps: the resampler takes at most {MAX_TAPS} "
                         f"taps per phase and {MAX_TABLE} entries (rates with a larger common divisor have smaller tables)")
    return o, n, width, T


def design(orig_sr: int, new_sr: int):
    """(o, n, width, taps): the polyphase table ``taps`` [n, 2 * width + o] as a float64 numpy array, built as
    ``csm.data.resample`` builds its kernel."""
    o, n, width, _ = geometry(orig_sr, new_sr)
    base = min(o, n) * ROLLOFF
    idx = torch.arange(-width, width + o, dtype=torch.float64) / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx[None, :]) * base
    t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    taps = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / o)
    return o, n, width, taps.numpy()


# ---- the schedule: host integers only -----------------------------------------------------------------------------------------
def out_len(n_samples: int, o: int, n: int) -> int:
    """M: outputs of a signal of ``n_samples``."""
    return -(-n * n_samples // o)


def ready_blocks(fed: int, o: int, width: int) -> int:
    """Output blocks (n outputs each) computable once ``fed`` samples of a stream are in."""
    return max(0, (fed - width - o) // o + 1)


def step_outputs(pos: int, n_in: int, final: bool, o: int, n: int, width: int) -> int:
    """Outputs a stream at ``pos`` samples emits when it is fed ``n_in`` more; ``final``: the stream ends there."""
    first = n * ready_blocks(pos, o, width)
    return (out_len(pos + n_in, o, n) if final else n * ready_blocks(pos + n_in, o, width)) - first


def max_step_outputs(max_in: int, o: int, n: int, width: int) -> int:
    """The most outputs one step of up to ``max_in`` samples can emit (a final one: the lag comes out with it)."""
    return -(-n * (max_in + width + o - 1) // o)


# ---- the device forms ---------------------------------------------------------------------------------------------------------
class Resampler:
    """The table of one rate pair on ``device`` and the one-shot form: ``resampler(wav[..., N]) -> [..., ceil(N * new / orig)]``."""

    def __init__(self, orig_sr: int, new_sr: int, device="cuda"):
        self.orig_sr, self.new_sr = int(orig_sr), int(new_sr)
        self.o, self.n, self.width, taps = design(orig_sr, new_sr)
        self.T = 2 * self.width + self.o
        self.device = torch.device(device)
        self.taps = torch.from_numpy(taps).to(F32).to(self.device).contiguous()       # rounded once, uploaded once

    @property
    def lag(self) -> int:
        """Input samples a stream of this pair holds back: width + o."""
        return self.width + self.o

    @torch.no_grad()
    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        from ..hip import ops
        shape = wav.shape
        x = wav.reshape(-1, shape[-1]).to(self.device, F32).contiguous()
        y = torch.empty(x.shape[0], out_len(shape[-1], self.o, self.n), dtype=F32, device=self.device)
        if x.shape[0]:
            ops.resample_f32(x, self.taps, y, self.o, self.n, self.width)
        return y.reshape(shape[:-1] + (y.shape[1],))

    def stream(self, max_in: int = None) -> "ResampleStream":
        """A stateful stream; ``max_in``: the most samples one launch takes (longer pieces are fed in several; default 1 s)."""
        return ResampleStream(self, self.orig_sr if max_in is None else max_in)

    def stream_rows(self, slots: int = 16, max_in: int = None, state_slots: int = None) -> "ResampleStreamRows":
        """Up to 16 streams advanced by one launch per step, each in its own slot.  ``state_slots`` (>= slots): that many streams
        keep a carry, slot indices run over all of them, and a step still takes at most ``slots``."""
        return ResampleStreamRows(self, slots, self.orig_sr if max_in is None else max_in, state_slots)


def _check_max_in(max_in):
    if isinstance(max_in, bool) or not isinstance(max_in, int) or max_in < 1:
        raise ValueError(f"max_in must be an integer >= 1, got {max_in!r}")
    return max_in


class ResampleStream:
    """One stream of a ``Resampler``.  State: the last T - 1 input samples in two device buffers that alternate each launch, and on
    the host the number of samples seen.  ``feed`` makes no host synchronisation."""

    def __init__(self, rs: Resampler, max_in: int):
        self.rs, self.max_in = rs, _check_max_in(max_in)
        self._carry = torch.zeros(2, rs.T - 1, dtype=F32, device=rs.device)
        self.reset()

    def reset(self):
        """Start a new stream."""
        self._carry.zero_()
        self._par, self.pos, self.ended = 0, 0, False

    def _launch(self, x, final):
        from ..hip import ops
        rs = self.rs
        k = 0 if x is None else x.numel()
        y = torch.empty(step_outputs(self.pos, k, final, rs.o, rs.n, rs.width), dtype=F32, device=rs.device)
        ops.resample_stream_f32(self._carry, self._par, x, self.pos, final, rs.taps, y, self.max_in, rs.o, rs.n, rs.width)
        self._par ^= 1
        self.pos += k
        return y

    @torch.no_grad()
    def feed(self, x: torch.Tensor) -> torch.Tensor:
        """The next samples of the stream, any number (none included) -> the outputs now computable (1-D, maybe empty)."""
        if self.ended:
            raise RuntimeError("feed: this stream was flushed - reset() starts the next one")
        x = x.reshape(-1).to(self.rs.device, F32).contiguous()
        out = [self._launch(x[i:i + self.max_in], False) for i in range(0, x.numel(), self.max_in)]
        return out[0] if len(out) == 1 else torch.cat(out) if out else torch.zeros(0, dtype=F32, device=self.rs.device)

    @torch.no_grad()
    def flush(self) -> torch.Tensor:
        """The stream ends: the outputs still owed, computed against zeros past its end (empty for an empty stream)."""
        if self.ended:
            raise RuntimeError("flush: this stream was flushed already - reset() starts the next one")
        self.ended = True
        if self.pos == 0:
            return torch.zeros(0, dtype=F32, device=self.rs.device)
        return self._launch(None, True)


class ResampleStreamRows:
    """``ResampleStream`` for up to 16 streams at once: a carry arena [slots, 2, T - 1] and per slot, on the host, the parity and
    the samples seen.  ``step`` advances R of them with ONE launch (csm_resample_stream_rows_f32) - each row with its own piece,
    of its own length - and a row's outputs are those of a ``ResampleStream`` fed the same pieces, whatever its neighbours do."""

    def __init__(self, rs: Resampler, slots: int = 16, max_in: int = 24000, state_slots: int = None):
        if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= 16:
            raise ValueError(f"slots must be 1..16 (the rows kernel takes at most 16 rows a launch), got {slots!r}")
        if state_slots is not None and (isinstance(state_slots, bool) or not isinstance(state_slots, int) or state_slots < slots):
            raise ValueError(f"state_slots must be an integer >= slots = {slots} (None: one carry per row of a launch), got {state_slots!r}")
        self.rs, self.slots, self.max_in = rs, slots, _check_max_in(max_in)
        # more streams than rows of a launch: the arena holds ``state_slots`` carries, slot indices run over all of them and a
        # step still takes at most ``slots``; a stream keeps its slot for its whole life, so no carry is ever copied
        self.state_slots = slots if state_slots is None else state_slots
        slots = self.state_slots
        self._arena = torch.zeros(slots, 2, rs.T - 1, dtype=F32, device=rs.device)
        self.pos = [0] * slots
        self._par = [0] * slots
        self._live = [False] * slots

    def _slot(self, slot):
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.state_slots:
            raise ValueError(f"slot {slot!r} out of range (0..{self.state_slots - 1})")
        return slot

    def open(self, slot: int):
        """Start a new stream in ``slot`` (also after an earlier one ended there)."""
        slot = self._slot(slot)
        self._arena[slot].zero_()
        self.pos[slot], self._par[slot], self._live[slot] = 0, 0, True

    def close(self, slot: int):
        """The stream in ``slot`` is dropped."""
        self._live[self._slot(slot)] = False

    @property
    def open_slots(self) -> List[int]:
        return [s for s in range(self.state_slots) if self._live[s]]

    @torch.no_grad()
    def step(self, slots: Sequence[int], xs: Sequence[torch.Tensor], final: Sequence[int] = ()) -> List[torch.Tensor]:
        """``xs[r]``: the next samples (1..max_in; none only for a slot named in ``final``) of the stream in ``slots[r]``;
        ``final``: the slots whose stream ends with this step (they emit what they still owe and close).  Returns each row's
        outputs (1-D views of one buffer, maybe empty)."""
        from ..hip import ops
        rs = self.rs
        rows = [self._slot(s) for s in slots]
        fin = {self._slot(s) for s in final}
        R = len(rows)
        if not 1 <= R <= self.slots or len(set(rows)) != R or len(xs) != R or not fin <= set(rows):
            raise ValueError(f"step takes 1..{self.slots} distinct slots with one piece each and ends only slots it steps, got "
                             f"{rows} / {len(xs)} pieces / final {sorted(fin)}")
        if any(not self._live[s] for s in rows):
            raise ValueError(f"step: slot {next(s for s in rows if not self._live[s])} is not open")
        xs = [None if x is None else x.reshape(-1).to(rs.device, F32).contiguous() for x in xs]
        ks = [0 if x is None else x.numel() for x in xs]
        for s, k in zip(rows, ks):
            if k > self.max_in or (k == 0 and s not in fin):
                raise ValueError(f"step: slot {s} brings {k} samples - a row takes 1..max_in = {self.max_in} (none only when it ends)")
        ms = [step_outputs(self.pos[s], k, s in fin, rs.o, rs.n, rs.width) for s, k in zip(rows, ks)]
        y = torch.empty(R, max(ms), dtype=F32, device=rs.device)
        ops.resample_stream_rows_f32(self._arena, xs, rs.taps, y, rows, [self._par[s] for s in rows], [self.pos[s] for s in rows],
                                     [s in fin for s in rows], self.max_in, rs.o, rs.n, rs.width)
        for s, k in zip(rows, ks):
            self._par[s] ^= 1
            self.pos[s] += k
            if s in fin:
                self._live[s] = False
        return [y[r, :m] for r, m in enumerate(ms)]


_CACHE = {}


def get_resampler(orig_sr: int, new_sr: int, device) -> Resampler:
    """The ``Resampler`` of a rate pair on ``device``: its table is built and uploaded once per process."""
    key = (orig_sr, new_sr, str(torch.device(device)))
    if key not in _CACHE:
        _CACHE[key] = Resampler(orig_sr, new_sr, device)
    return _CACHE[key]


def rate_resampler(name: str, rate, native_sr: int, device, to_native: bool):
    """What ``hear(sample_rate=)`` / ``output_sample_rate=`` resolve to: None for None or the codec's own rate (today's path),
    else the ``Resampler`` into (``to_native``) or out of the codec's rate.  A bad rate raises here, at the call."""
    if rate is None:
        return None
    rate = check_rate(name, rate)
    if rate == int(native_sr):
        return None
    return get_resampler(rate, int(native_sr), device) if to_native else get_resampler(int(native_sr), rate, device)
