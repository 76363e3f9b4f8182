"""What tests/test_gpu_train_large_batch.py stands on, checked without a GPU: the conditions its data must meet (on the
float64 step of tests/_train_ref.py: conditions, not measurements) and which kernels each shape reaches, asked of the
launchers' own functions through kh_train_conv_plan."""
import ctypes as C

import numpy as np
import pytest

from kami_amd import _lib as L

import _train_ref as T


@pytest.mark.parametrize("F,C,R,B", list(T.LARGE) + T.ROBUST_EXTRA)
def test_robust_blob_data_conditions(F, C, R, B):
    """On a ReLU-robust blob no pre-ReLU value comes near zero (min |z| >= 1), so no fp32 implementation flips a mask
    against float64, and plain fp32 PyTorch is within 2.5e-4 of every tensor's gradient scale: with the factor 8 of the
    GPU tests their bound never exceeds 2e-3 of gradient scale."""
    c = T.case(F, C, R, B, True, 0)
    assert c["f64"]["min_z"] >= T.MIN_Z_ROBUST and c["f32"]["min_z"] >= T.MIN_Z_ROBUST
    e = T.e32(c)
    worst = max(e, key=e.get)
    print(f"F{F} C{C} R{R} B{B}: min|z| {c['f64']['min_z']:.3g}, worst fp32-torch gradient error {e[worst]:.3g} ({worst})")
    assert e[worst] <= T.E32_CAP, (worst, e[worst])
    assert 8 * e[worst] <= 2e-3
    # both mask values occur: a dead channel's BatchNorm parameters get no gradient, its neighbours do
    g = c["f64"]["grads"]["batchnorm1.weight"]
    assert (g[3::4] == 0).all() and (g[0::4] != 0).all()


@pytest.mark.parametrize("F,C,R,B", list(T.RANDOM_SMALL))
def test_random_blob_seed_condition(F, C, R, B):
    """Random blobs (data-dependent masks) at the small shapes: the fixed seed keeps every pre-ReLU value of the float64
    step at least 1e-5 (about 170 x 2^-24 at these magnitudes) from zero."""
    c = T.case(F, C, R, B, False, T.RANDOM_SMALL[(F, C, R, B)])
    e = T.e32(c)
    print(f"F{F} C{C} R{R} B{B}: min|z| {c['f64']['min_z']:.3g}, worst fp32-torch gradient error {max(e.values()):.3g}")
    assert c["f64"]["min_z"] >= T.MIN_Z_RANDOM
    assert max(e.values()) <= T.E32_CAP


def test_robust_blob_touches_batchnorm_biases_only():
    from kami_amd import weights as W
    F, Cc, R = 30, 24, 1
    blob = W.random_weights(F, Cc, R, seed=T.WEIGHT_SEED, peaky=T.PEAKY)
    a, b = W.split(blob, F, Cc, R), W.split(T.robust_blob(blob, F, Cc, R), F, Cc, R)
    for name in a:
        if "batchnorm" in name and name.endswith(".bias"):
            want = np.where(np.arange(a[name].size) % 4 == 3, -8.0, 8.0) if a[name].size > 1 else np.array([8.0])
            assert np.array_equal(b[name], want.astype(np.float32)), name
        else:
            assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("F,C,R,B", list(T.LARGE))
def test_dispatch_of_the_large_batch_shapes(F, C, R, B):
    """Every shape reaches the kernels its row of DESIGN.md 5.7's table names."""
    want = T.LARGE[(F, C, R, B)]
    for layer, (ci, co) in T.layer_shapes(F, C).items():
        two, ranges, per, last = T.conv_plan(B, ci, co)
        assert two == (layer in want["two_board"]), (layer, two)
        if layer in want["wgrad"]:
            assert (ranges, per, last) == want["wgrad"][layer], (layer, ranges, per, last)
            assert per > 1 and ranges > 1                    # the board loop makes more than one trip, several ranges are added
    assert any(per > 1 for _, _, per, _ in (T.conv_plan(B, ci, co) for ci, co in T.layer_shapes(F, C).values()))
    # the elementwise kernels' grids are capped at 4096 x 256 threads: the widest layer's activations (the tower's, or
    # the policy conv's 128 channels) need a second grid-stride trip at every shape but the batch of 19
    assert (B * 64 * max(C, T.POLICY_MID) > 4096 * 256) == (B != 19)
    if (F, C, R, B) == (30, 256, 1, 67):                    # the policy conv's data gradient (128 -> 256 channels, added to
        assert T.conv_plan(B, T.POLICY_MID, C)[0]           # the value head's) takes the two-board kernel, its forward the small one
    if (F, C, R, B) == (30, 64, 1, 254):                    # one board short of the tower's boundary
        assert not T.conv_plan(254, 64, 64)[0] and T.conv_plan(255, 64, 64)[0]
        assert T.conv_plan(256, 64, 64)[1:3] == (256, 1) and T.conv_plan(257, 64, 64)[1:3] == (129, 2)


@pytest.mark.parametrize("F,C,R,B", [(30, 64, 2, 8), (30, 128, 1, 12), (119, 64, 1, 64), (30, 256, 1, 6), (30, 24, 1, 5), (30, 64, 1, 64)])
def test_dispatch_of_the_earlier_shapes(F, C, R, B):
    """The shapes tests/test_gpu_train.py steps: the small kernel everywhere, one board per weight-gradient range."""
    for ci, co in T.layer_shapes(F, C).values():
        two, ranges, per, last = T.conv_plan(B, ci, co)
        assert not two and (ranges, per, last) == (B, 1, 1)


def test_conv_plan_boundaries_and_arguments():
    # ceil(B / 2) * ceil(co / 64) >= 128 is the two-board kernel: the first batch on its side, per channel count
    for co, first in ((24, 255), (64, 255), (128, 127), (256, 63)):
        assert not T.conv_plan(first - 1, 64, co)[0] and T.conv_plan(first, 64, co)[0]
    # one board per range until B exceeds ceil(256 / tiles): 256 at 64 x 64, 64 at 128 x 128, 16 at 256 x 256
    for c, most in ((64, 256), (128, 64), (256, 16)):
        assert T.conv_plan(most, c, c)[1:] == (most, 1, 1) and T.conv_plan(most + 1, c, c)[2] == 2
    # the ranges cover the batch, the last one is not empty
    for B in (1, 2, 17, 63, 67, 131, 257, 259, 1000):
        for ci, co in ((30, 64), (119, 24), (64, 64), (128, 128), (256, 256), (256, 128)):
            _, ranges, per, last = T.conv_plan(B, ci, co)
            assert 1 <= last <= per and (ranges - 1) * per + last == B
    lib = L.load()
    assert lib.kh_train_conv_plan(257, 64, 64, None, None, None) == L.KH_OK          # every output is optional
    one = C.c_int(-1)
    assert lib.kh_train_conv_plan(257, 64, 64, C.byref(one), None, None) == L.KH_OK and one.value == 1
    for bad in ((0, 64, 64), (8, 0, 64), (8, 64, -1)):
        assert lib.kh_train_conv_plan(*bad, None, None, None) == L.KH_ERR_INVALID
    assert "kh_train_conv_plan" in L.last_error()
