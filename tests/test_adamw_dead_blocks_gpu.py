"""The flagged AdamW kernels (csm_adamw_step_live / csm_adamw_step_split_live: one ``block_live`` byte per 2048 elements, a block
that never had a gradient only has its weights decayed) against the un-flagged kernels, bit for bit as integer views; one case
is also judged by the float64 reference of tests/train_ops_ref.py; then ``FusedAdamW`` with the flags on against a twin with
``CSM_ADAMW_DEAD_BLOCKS=0``."""
import itertools

import pytest
import torch

import train_ops_ref as T

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BLOCK = 2048
N = 5 * BLOCK + 1032                                          # five whole blocks and a partial tail block
NBLK = 6
LR, B1, B2, EPS = T.ADAM_LR, T.ADAM_B1, T.ADAM_B2, T.ADAM_EPS


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(what, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ, first at {int((g != w).nonzero()[0])}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grads():
    """Step k = 1..4.  block 0: never; 1: step 1 only; 2: step 3 only; 3: every step; 4: one element of its last 8-element vector
    at step 2; the tail: never.  -> the four gradients and, per step, which blocks have had a gradient so far."""
    g = _gen(31)
    grads, live, seen = [], [], torch.zeros(NBLK, dtype=torch.uint8)
    for k in (1, 2, 3, 4):
        gr = torch.zeros(N, dtype=BF16)
        for b in ([1] if k == 1 else []) + ([2] if k == 3 else []) + [3]:
            gr[b * BLOCK:(b + 1) * BLOCK] = (torch.randn(BLOCK, generator=g) + 3.0).to(BF16)        # (+3: hardly an element is 0, never a whole block)
            seen[b] = 1
        if k == 2:
            gr[5 * BLOCK - 3] = 0.5
            seen[4] = 1
        grads.append(gr)
        live.append(seen.clone())
    return grads, live


class Pair:
    """The same state twice on the device: ``ref`` goes through the un-flagged kernel, ``got`` through the flagged one."""

    def __init__(self, split, n, seed=7, edge=True):
        from csm.hip import ops
        master = torch.randn(n, generator=_gen(seed))
        if edge:                                              # signed zeros and subnormals among the weights of a dead block
            master[:8] = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 65504.0, -3.0, 2.0 ** -126, 1.0])
        self.split, self.n = split, n
        self.fn = ops.adamw_step_split if split else ops.adamw_step
        self.state = []
        for _ in range(2):
            if split:
                p, lo = (t.cuda() for t in T.split_master(master))
                st = dict(w=lo, param=p)
            else:
                st = dict(w=master.cuda(), param=torch.full((n,), float("nan"), dtype=BF16, device="cuda"))
            st.update(m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
            self.state.append(st)
        self.ref, self.got = self.state
        self.live = torch.zeros(-(-n // BLOCK), dtype=torch.uint8, device="cuda")

    def master(self, st):
        return T.join_master(st["param"].cpu(), st["w"].cpu()) if self.split else st["w"].cpu()

    def step(self, grad, step, wd, coef, zero_grad):
        for st in self.state:
            st["grad"] = grad.cuda()
            if not self.split:
                st["param"].fill_(float("nan"))
            kw = dict(block_live=self.live) if st is self.got else {}
            self.fn(st["w"], st["m"], st["v"], st["param"], st["grad"], LR, B1, B2, EPS, wd, step, norm_and_coef=coef, zero_grad=zero_grad, **kw)

    def check(self, what):
        for k in ("w", "param", "m", "v", "grad"):
            _same(f"{what}: {k}", self.got[k], self.ref[k])


VARIANTS = list(itertools.product((False, True), (0.0, 0.01), (False, True), (False, True), (False, True)))


@pytest.mark.parametrize("split,wd,with_coef,zero_grad,one_block", VARIANTS,
                         ids=["-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in zip(("split", "wd", "coef", "zg", "one"), c)) for c in VARIANTS])
def test_flagged_equals_unflagged(dev, split, wd, with_coef, zero_grad, one_block):
    """Four steps from zero moments: after each, param, lo / master, m, v and grad equal the un-flagged kernel's bits and
    block_live equals "this block has had a non-zero gradient so far"."""
    from csm.hip import lib
    grads, live = _grads()
    coef = torch.tensor([123.0, 0.37], device="cuda") if with_coef else None
    pr = Pair(split, N)
    if one_block:
        lib.csm_set_adamw_blocks(1)                           # one workgroup walks all six blocks
    try:
        for k, (g, want) in enumerate(zip(grads, live), start=1):
            pr.step(g, k, wd, coef, zero_grad)
            pr.check(f"step {k}")
            _same(f"step {k}: block_live", pr.live, want)
            dead = [b for b in range(NBLK) if not want[b]]
            assert all(not _bits(pr.got[key][b * BLOCK:(b + 1) * BLOCK]).any() for b in dead for key in ("m", "v"))
    finally:
        lib.csm_set_adamw_blocks(1 << 20)


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
@pytest.mark.parametrize("zero_grad", (False, True), ids=("keep", "zero"))
def test_minus_zero_gradient_takes_the_full_path(dev, split, zero_grad):
    """-0.0 as the only set bit of block 0's gradient; block 1 all +0."""
    pr = Pair(split, 2 * BLOCK)
    g = torch.zeros(2 * BLOCK, dtype=BF16)
    g[1234] = -0.0
    assert int(_bits(g)[1234]) == -32768 and int((_bits(g) != 0).sum()) == 1
    pr.step(g, 1, 0.01, None, zero_grad)
    pr.check("-0")
    assert pr.live.tolist() == [1, 0]
    assert int(_bits(pr.got["grad"])[1234]) == (0 if zero_grad else -32768)


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
@pytest.mark.parametrize("zero_grad", (False, True), ids=("keep", "zero"))
def test_dropped_step_leaves_state_and_flags(dev, split, zero_grad):
    """coef[1] < 0: weights, moments and flags stay, gradients are cleared as zero_grad says - also in a block that is not
    live and whose gradient is not zero."""
    grads, live = _grads()
    pr = Pair(split, N)
    pr.step(grads[0], 1, 0.01, None, True)
    _same("flags after the first step", pr.live, live[0])
    before = {k: v.clone() for k, v in pr.got.items() if k != "grad"}
    g = (torch.randn(N, generator=_gen(5)) + 3.0).to(BF16)
    pr.step(g, 2, 0.01, torch.tensor([123.0, -1.0], device="cuda"), zero_grad)
    pr.check("dropped")
    _same("flags after the dropped step", pr.live, live[0])
    for k, v in before.items():
        if k != "param" or split:                             # (the plain form's param is an output only: the test refills it)
            _same(f"dropped: {k} unchanged", pr.got[k], v)
    _same("dropped: grad", pr.got["grad"], torch.zeros_like(g) if zero_grad else g)


@pytest.mark.parametrize("split", (False, True), ids=("plain", "split"))
def test_flagged_against_float64_reference(dev, split):
    """The four steps of test_flagged_equals_unflagged (wd = 0.01, clip coefficient 0.37, zero_grad) judged after EACH step
    against the float64 step from the device's own previous state, as test_adamw_step_and_split judges the un-flagged kernels."""
    grads, _ = _grads()
    c = T.AdamCase(N, 0.01, 1.0, 0.37, True, False)
    coef = torch.tensor([123.0, c.coef], device="cuda")
    pr = Pair(split, N, edge=False)                           # (the reference's bounds are relative: no subnormal weights)
    for k, g in enumerate(grads, start=1):
        st = pr.got
        state = {"master": pr.master(st), "m": st["m"].cpu(), "v": st["v"].cpu()}
        pr.step(g, k, c.wd, coef, c.zero_grad)
        master = pr.master(st)
        T.judge_all("adamw_live", {"master": master, "m": st["m"], "v": st["v"]}, T.adam_ref(state, g, c, k), f"split={split} step {k}")
        T.judge("adamw_live.param", st["param"], T.split_master(master)[0] if split else master.to(BF16), None)
        T.judge("adamw_live.grad", st["grad"], torch.zeros_like(g), None)


# ------------------------------------------------------------------------------------------------------------- optimiser
def _trainer(tmp_path, tag):
    from csm.models.model import Model, ModelArgs
    from csm.training.trainer import CSMTrainer
    tr = CSMTrainer("", str(tmp_path / tag), device="cuda")
    tr.logger.setLevel(40)
    tr.model = Model(ModelArgs("llama-tiny-backbone", "llama-tiny-decoder", 300, 67, 4), device="cuda", seed=3)
    tr.prepare_optimizer()
    return tr


def _batch(seed, B=2, S=24, K=4):
    """Text tokens from three ids, audio codes from the lower half of the codebooks: most embedding rows never get a gradient."""
    g = _gen(seed)
    tokens, mask = torch.zeros(B, S, K + 1, dtype=torch.long), torch.zeros(B, S, K + 1, dtype=torch.bool)
    tokens[:, :6, K] = torch.tensor([3, 7, 250])[torch.randint(0, 3, (B, 6), generator=g)]
    mask[:, :6, K] = True
    tokens[:, 6:, :K] = torch.randint(0, 32, (B, S - 6, K), generator=g)
    mask[:, 6:, :K] = True
    return {"input_tokens": tokens.cuda(), "input_masks": mask.cuda(), "target_audio_tokens": torch.randint(0, 64, (B, S, K), generator=g).cuda()}


def _opt_state(opt):
    return {f"{n}.{k}": t for n in opt.state for k, t in (("master", opt.master(n)), ("m", opt.state[n]["m"]), ("v", opt.state[n]["v"]))}


def test_optimizer_flags_equal_unflagged_twin(dev, tmp_path, monkeypatch):
    """Three train steps with the flags on and a twin with CSM_ADAMW_DEAD_BLOCKS=0: masters, m, v and losses bit-equal; flags of
    both kinds afterwards; a reloaded optimiser derives its flags from the moments and steps on bit-equal to the twin."""
    from csm.training.optim import FusedAdamW, live_blocks
    monkeypatch.setenv("CSM_ADAMW_DEAD_BLOCKS", "1")
    on = _trainer(tmp_path, "on")
    monkeypatch.setenv("CSM_ADAMW_DEAD_BLOCKS", "0")
    off = _trainer(tmp_path, "off")
    assert "live" in on.optimizer.state["embeddings"] and all("live" not in st for n, st in on.optimizer.state.items() if n != "embeddings")
    assert all("live" not in st for st in off.optimizer.state.values())
    assert not on.optimizer.state["embeddings"]["live"].any()
    for s in range(3):
        b = _batch(40 + s)
        l_on, _ = on.train_step(b, 1, True, 1.0)
        l_off, _ = off.train_step(b, 1, True, 1.0)
        _same(f"step {s}: loss", l_on, l_off)
    want = _opt_state(off.optimizer)
    for k, t in _opt_state(on.optimizer).items():
        _same(k, t, want[k])
    emb = on.optimizer.state["embeddings"]
    live = emb["live"].cpu()
    assert int(live.min()) == 0 and int(live.max()) == 1, live.tolist()
    _same("flags == any bit of the moments", live, live_blocks(emb["m"], emb["v"]))
    # state_dict -> a fresh optimiser -> load_state_dict: the flags are not saved, they are derived from the loaded moments
    sd = on.optimizer.state_dict()
    assert all(set(st) == {"master", "m", "v"} for st in sd["state"].values())
    monkeypatch.setenv("CSM_ADAMW_DEAD_BLOCKS", "1")
    fresh = FusedAdamW(on.model, {g["name"]: g["lr"] for g in on.optimizer.param_groups}, weight_decay=on.weight_decay)
    assert not fresh.state["embeddings"]["live"].any()
    fresh.load_state_dict(sd)
    _same("reloaded flags", fresh.state["embeddings"]["live"], live)
    on.optimizer = fresh
    b = _batch(50)
    l_on, _ = on.train_step(b, 1, True, 1.0)
    l_off, _ = off.train_step(b, 1, True, 1.0)
    _same("after reload: loss", l_on, l_off)
    want = _opt_state(off.optimizer)
    for k, t in _opt_state(fresh).items():
        _same(f"after reload: {k}", t, want[k])
