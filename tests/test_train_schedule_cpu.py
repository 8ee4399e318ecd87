"""The launch schedule of the train step, without a GPU: every mode of ``_Stack.forward`` / ``_Stack.backward`` (csm/engine.py) must
issue exactly the events of ``tests/golden/train_schedule.json`` - the same launches, hooks and LoRA calls, in the same order, on
the same operands (train_schedule_ref.py: how a trace is taken and what an event says).  The golden traces were recorded from the
schedule as it was spelled out projection by projection, before ``_Stack`` got one body per projection; they are not to be
recorded again to make a change pass: a difference means a launch moved."""
import json

import pytest

import train_schedule_ref as R


@pytest.fixture(scope="module")
def golden():
    with open(R.GOLDEN) as f:
        return json.load(f)


def test_every_mode_has_a_golden_trace(golden):
    assert list(golden) == list(R.MODES)


@pytest.mark.parametrize("mode", list(R.MODES))
def test_schedule(golden, mode):
    got, want = R.trace(mode), golden[mode]
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"mode {mode}, event {n}: the schedule issues\n  {g}\nand the golden trace has\n  {w}"
    assert len(got) == len(want), (f"mode {mode}: {len(got)} events, the golden trace has {len(want)}; the first one over: "
                                   f"{(got + want)[min(len(got), len(want))]}")


def test_the_recorder_reaches_every_branch(golden):
    """What the modes are there for, read off the golden traces themselves."""
    ops = {mode: [e.split("(")[0] for e in ev] for mode, ev in golden.items()}
    # five layers: 4-2 share one launch, 1 and 0 go alone (what is launched last is what an all-reduce cannot hide)
    assert [ops["wide"].count(o) for o in ("multi_linear_dw", "two_linear_dw", "colsum_bf16_multi")] == [1, 2, 3]
    assert "two_linear_dw" in ops["wide_defer_attn_1"] and "multi_linear_dw" not in ops["wide_defer_attn_1"]
    assert ops["wide_norms_undeferred"].count("colsum_bf16") == 11 and "colsum_bf16_multi" not in ops["wide_norms_undeferred"]
    assert ops["narrow"].count("multi_linear_dw") == 2 and ops["narrow"].count("linear_dw") == 3 + 1      # w13 x 3, the odd w2
    assert ops["narrow_ungrouped_kernels"].count("two_linear_dw") == 3
    assert "linear_dw" not in ops["wide_frozen"] and "colsum_bf16" not in ops["wide_frozen"]
    assert "linear_rope_fwd" in ops["tiny"] and "linear_rope_fwd" not in ops["fwd_pos_unfused_rope"]
    assert "swiglu_fwd" in ops["lora_bias"] and "swiglu_bwd" in ops["lora_bias"] and "swiglu_fwd" not in ops["lora_dropout"]
    assert ops["lora_all7"].count("gemm_kext") == 2 * 8 and "linear_fwd" not in ops["lora_all7"]
    assert any(e.startswith("linear_swiglu_fwd(") and ";residual=" in e for e in golden["lora_dropout"])
    assert "attn_fwd_seg" in ops["packed"] and "attn_bwd_seg" in ops["packed"]
    assert "attn_append" in ops["append"] and "attn_append_rows" in ops["append_ragged"]
    # the ops a benchmark's timers wrap see no ``pin`` keyword unless a call is pinned
    swiglu = {mode: [e for e in golden[mode] if e.startswith("linear_swiglu_fwd(")] for mode in ("tiny", "append_ragged")}
    assert swiglu["tiny"] and not any("pin" in e for e in swiglu["tiny"]) and all(e.endswith(";pin=True)") for e in swiglu["append_ragged"])
    assert any(";sel=sel" in e or ",sel=sel" in e for e in golden["lora_stack"])
