"""What tests/test_gpu_value_head.py stands on, checked on the CPU: the float64 forward of tests/_forward_ref.py agrees
with the fp32 C oracle; every case's value head is alive; every named defect moves the float64 value output by at least
three times the bound the GPU test applies (a kernel with that defect is then off by at least twice the bound); and
the four committed parity cases whose head is dead stay recorded as such.  No case is skipped or excluded: the seeds in
_forward_ref.CASES were picked so that the reference alone meets these conditions."""
import numpy as np
import pytest

from kami_amd import weights as W
from oracle import pyoracle as ko

import _forward_ref as FR

NAMES = list(FR.CASES)


@pytest.mark.parametrize("name", [n for n in NAMES if FR.CASES[n]["B"] <= 64])
def test_forward64_agrees_with_the_fp32_oracle(name):
    """fp32 oracle against float64: 1e-5 on logits, 5e-6 on values (observed 6e-6 / 3e-7 at 119, 64, 6, 64).  Through
    the public forward64, not the cached pieces of case()."""
    c = FR.case(name)
    p, v, lg = FR.forward64(c["blob"], c["F"], c["C"], c["R"], c["x"])
    assert np.array_equal(v, c["value"]) and np.array_equal(lg, c["logits"])      # case() shares the trunk: same numbers
    op, ov, ol = ko.forward(c["blob"], c["F"], c["C"], c["R"], c["x"])
    dl, dv = float(np.abs(ol - lg).max()), float(np.abs(ov - v).max())
    print(f"{name}: oracle vs float64: logits {dl:.2e} values {dv:.2e}")
    assert dl <= 1e-5 and dv <= 5e-6, (name, dl, dv)
    assert float(np.abs(op - p).max()) <= 1e-5
    assert abs(c["model"]["f32"]["value"] - dv) < 1e-12 and abs(c["model"]["f32"]["logit"] - dl) < 1e-12


def test_forward64_agrees_with_the_oracle_at_depth():
    """the residual loop more than once: the headline shape of the parity tests (119, 64, 6), plain random_weights"""
    F, C, R, B = 119, 64, 6, 8
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=20.0)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    _, v, lg = FR.forward64(blob, F, C, R, x)
    _, ov, ol = ko.forward(blob, F, C, R, x)
    assert float(np.abs(ol - lg).max()) <= 1e-5 and float(np.abs(ov - v).max()) <= 5e-6


def test_live_value_blob_changes_two_tensors_only():
    c = FR.case("t8_c24_b17")
    F, C, R = c["F"], c["C"], c["R"]
    raw = W.random_weights(F, C, R, seed=c["seed"], peaky=FR.PEAKY)
    live = FR.live_value_blob(raw, F, C, R, c["x"])
    assert np.array_equal(live, c["blob"])
    a, b = W.split(raw, F, C, R), W.split(live, F, C, R)
    changed = {n for n in a if not np.array_equal(a[n], b[n])}
    assert changed == {"vbatchnorm.bias", "valuefc.weight"}
    assert abs(float(np.median(c["z"]))) < 1e-6                                    # the shift sits at the plane's median
    contrib = c["pre"] - b["valuefc.bias"][None, :].astype(np.float64)
    assert abs(float(contrib.std()) - 0.5) < 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_value_head_is_alive(name):
    c = FR.case(name)
    z, v, B = c["z"], c["value"], c["B"]
    frac = (z > 0).mean(1)
    small = float((np.abs(v) < 0.95).mean())
    std = float(v.std(0).min()) if B > 1 else float("nan")
    print(f"{name}: squares > 0 per board {frac.min():.2f}..{frac.max():.2f}, |v| < 0.95 on {small:.3f}, |v| max {np.abs(v).max():.3f}, "
          f"smallest column std across boards {std:.3f}")
    assert frac.min() >= 0.25 and frac.max() <= 0.75, (name, frac.min(), frac.max())
    assert small >= 0.90, (name, small)
    if B >= 16:
        assert (z > 0).any(0).all(), (name, "a square that is positive on no board")
        assert (z <= 0).any(0).all(), (name, "a square that the ReLU cuts on no board")
        assert std >= 0.1, (name, std)


@pytest.mark.parametrize("name", NAMES)
def test_mutations_have_teeth(name):
    """every defect of MUTATIONS moves the float64 value output by >= 3 x the case's value bound, for every dtype that
    has to see it (bf16: all but the single-element ones, which f16 — the same templates — and f32 carry)"""
    c = FR.case(name)
    for dtype in ("bf16", "f16", "f32"):
        bound = c["bound"][dtype]["value"]
        ratios = {m: c["effect"][m] / bound for m in FR.mutations_for(dtype, c["B"])}
        worst = min(ratios, key=ratios.get)
        print(f"{name} {dtype}: value bound {bound:.2e} (model {c['model'][dtype]['value']:.2e}), logit bound {c['bound'][dtype]['logit']:.2e}, "
              f"smallest mutation effect / bound {ratios[worst]:.1f} ({worst})")
        assert ratios[worst] >= FR.TEETH, (name, dtype, worst, ratios[worst])
    assert len(FR.mutations_for("f16", 17)) == len(FR.MUTATIONS) == 14 and len(FR.mutations_for("bf16", 17)) == 8
    assert "h:board_xor1" not in FR.mutations_for("f32", 1)


def test_bounds_have_the_stated_form():
    c = FR.case("t8_f30_b17")
    for dtype in ("bf16", "f16"):
        for q in ("value", "logit"):
            assert c["bound"][dtype][q] == 2.0 * c["model"][dtype][q] > 0
    _, v, lg = FR.forward_rounded(c["blob"], c["F"], c["C"], c["R"], c["x"], "bf16")
    assert abs(float(np.abs(v - c["value"]).max()) - c["model"]["bf16"]["value"]) < 1e-15
    assert abs(float(np.abs(lg - c["logits"]).max()) - c["model"]["bf16"]["logit"]) < 1e-15
    for q in ("value", "logit"):
        assert c["bound"]["f32"][q] == max(8.0 * c["model"]["f32"][q], 1e-6)
    # bf16 carries 8 significant bits, f16 11: the model's errors are apart by about that factor
    assert 3.0 < c["model"]["bf16"]["value"] / c["model"]["f16"]["value"] < 24.0


@pytest.mark.parametrize("F,C,R,B", FR.DEAD_CASES)
def test_committed_parity_cases_have_a_dead_value_head(F, C, R, B):
    """The gap the live cases close, pinned: on these committed cases of tests/test_gpu_parity.py the value plane is
    negative on every square of every board, and no mutation but (e) and (f), which can revive the plane, changes
    forward64's value output at all.  Fails if random_weights ever generates something else for these seeds."""
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=20.0)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    taps = {}
    _, v, _ = FR.forward64(blob, F, C, R, x, taps=taps)
    assert (taps["z"] < 0).all()
    fcb = W.split(blob, F, C, R)["valuefc.bias"].astype(np.float64)
    assert np.abs(v - np.tanh(fcb)[None, :]).max() < 1e-15          # every row is tanh(valuefc.bias), whatever the input
    for m in FR.MUTATIONS:
        tm = {}
        _, vm, _ = FR.forward64(blob, F, C, R, x, taps=tm, mutation=m)
        d = float(np.abs(vm - v).max())
        if m == "g:fc_bias0":            # the row IS tanh(bias): this one defect is all such a case can see
            assert d > 0
            continue
        if m == "f:no_relu":
            assert d > 0
            continue
        # (e) and (d) act in front of the ReLU and may lift squares above zero (at 30, 24 zeroing channel 0, whose
        # contribution is negative, lifts one: 1.4e-4); while the plane stays dead nothing shows, and (a), (b), (c), (h)
        # and the last channel of (d), the table's column, never touch its sign
        if m[0] in "abch" or m == "d:vconv_chlast":
            assert (tm["z"] < 0).all(), m
        if (tm["z"] < 0).all():
            assert d == 0.0, (m, d)


@pytest.mark.parametrize("name", ["copy_b5", "copy_b300"])
def test_copyout_cases_tell_the_two_modes_apart(name):
    """what tests/test_gpu_value_head.py's copy-out test relies on: in float64 the flat copy-out and column 0 differ by
    more than 12 bf16 bounds (a kernel within one bound of each is then more than 10 apart)"""
    c = FR.case(name)
    B = c["B"]
    d = float(np.abs(c["value"].reshape(-1)[:B] - c["value"][:, 0]).max())
    print(f"{name}: flat copy-out vs column 0: {d:.3f} = {d / c['bound']['bf16']['value']:.1f} bf16 bounds")
    assert d > 12.0 * c["bound"]["bf16"]["value"] > 12.0 * c["bound"]["f32"]["value"]


@pytest.mark.parametrize("name", ["t2s_c256_b17", "t8_f30_b17"])
def test_reversal_cases_have_distinct_end_rows(name):
    c = FR.case(name)
    assert float(np.abs(c["value"][0] - c["value"][-1]).max()) > 12.0 * c["bound"]["bf16"]["value"]
