"""kh_train's large-batch kernels against float64, on the GRADIENT's own scale.

Above the batches tests/test_gpu_train.py steps, a training step changes kernels: the raw-epilogue convolutions move
from conv_f32_small_kernel to conv_f32_kernel<9|1, 3|4> (two boards per workgroup), conv_wgrad_mfma_kernel's workgroups
walk ranges of several boards whose partial sums wgrad_reduce_kernel adds, and the elementwise kernels make more than
one grid-stride trip.  Each shape of _train_ref.LARGE is the smallest batch that reaches one of these paths
(tests/test_train_large_batch_data.py asserts which, through kh_train_conv_plan).

One SGD step at lr = 64 (mlr = 64000; a power of two, so lr * g is exact): the kernel's gradient is (blob - got) / 64
in float64, and the update's own rounding, at most 2^-24 * max(|blob_T|, |got_T|) / 64, is added to the bound.  For every
trainable tensor T, with s_T = max |g64_T| and e32_T = plain fp32 PyTorch's error relative to s_T:

    max |g - g64| <= max(8 * e32_T, 2e-6) * s_T + rounding term

2e-6 is the float64 step tests' bound, here on the gradient's scale; 8 is the margin over an independent fp32
implementation of the same step (both sum some 16 k terms per channel in fp32, in different orders and chunks).  The
same rule holds for the loss and for every BatchNorm running statistic (bn_stats_kernel and its N / (N - 1) at N = 16 k).

The large shapes run ReLU-robust blobs (_train_ref.robust_blob): on random blobs at these sizes the smallest |pre-ReLU|
in float64 is 1e-7 .. 1e-9, every fp32 implementation flips masks against float64 (plain fp32 PyTorch is then 2e-3 ..
3e-2 of gradient scale away), and no honest tolerance holds.  Random blobs, with their data-dependent masks, are
compared the same way at the small shapes, at seeds where float64 keeps min |z| >= 1e-5.

Observed (profiles/train_grad_maxima.json): worst error / bound 0.30 on the matrix cores, 0.76 on the VALU kernels; worst
error / s 3.3e-5 / 2.3e-5; error / (e32 * s) up to 12.9, above 8 only where e32 is under 2.5e-7 (the loss at batch 254:
1e-8, below fp32's own resolution) and the 2e-6 floor decides.  Before conv_wgrad_tiled_kernel summed per board, policyconv2.weight at
batch 257 missed the bound on both paths (9.5e-6 of gradient scale, 8.7 x e32)."""
import numpy as np
import pytest

from kami_amd import NN, weights as W

import _train_ref as T

LR_MLR, LR = 64000, 64.0


def _check(F, C, R, B, robust, seed, monkeypatch):
    from conftest import record_maxima
    c = T.case(F, C, R, B, robust, seed)
    f64, f32, scales = c["f64"], c["f32"], c["scales"]
    assert f64["min_z"] >= (T.MIN_Z_ROBUST if robust else T.MIN_Z_RANDOM)           # the data's conditions
    e32 = T.e32(c)
    assert max(e32.values()) <= T.E32_CAP
    specs = W.tensor_specs(F, C, R)
    failures = []
    for valu, path in (("0", "mfma"), ("1", "valu")):
        monkeypatch.setenv("KAMI_TRAIN_VALU", valu)
        nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
        nn.load_weights(c["blob"], 0)
        first, _ = nn.train(c["x"], c["obs_p"], c["obs_v"], mlr=LR_MLR, epochs=1, batchsize=B)
        assert nn.get_generation() == 1
        got = nn.get_weights().astype(np.float64)
        nn.close()
        worst_ratio, worst_rel, worst_of_bound, off, at = 0.0, 0.0, 0.0, 0, ["", ""]

        def judge(name, err, s, e, rounding=0.0):
            nonlocal worst_ratio, worst_rel, worst_of_bound
            bound = max(8.0 * e, 2e-6) * s + rounding
            worst_of_bound = max(worst_of_bound, err / bound)
            err_net = max(err - rounding, 0.0)                   # what is left for the gradient itself
            if err_net / s > worst_rel:
                worst_rel, at[1] = err_net / s, name
            if e > 0.0 and err_net / (e * s) > worst_ratio:
                worst_ratio, at[0] = err_net / (e * s), name
            if not err <= bound:
                failures.append((path, name, f"err {err:.3g} bound {bound:.3g} s {s:.3g} e32 {e:.3g} err/s {err / s:.3g}"))
        for name, shape in specs:
            k = int(np.prod(shape))
            a, b = got[off:off + k], c["blob"][off:off + k].astype(np.float64)
            off += k
            if "running" in name:
                want = f64["running"][name].ravel()
                s = float(np.abs(want).max())
                judge(name, float(np.abs(a - want).max()), s, float(np.abs(f32["running"][name].ravel() - want).max()) / s)
            else:
                g = (b - a) / LR
                rounding = 2.0 ** -24 * max(float(np.abs(b).max()), float(np.abs(a).max())) / LR
                judge(name, float(np.abs(g - f64["grads"][name].ravel()).max()), scales[name], e32[name], rounding)
        assert off == got.size
        s = abs(f64["loss"])
        judge("first_loss", abs(first - f64["loss"]), s, abs(f32["loss"] - f64["loss"]) / s)
        print(f"F{F} C{C} R{R} B{B} {'robust' if robust else 'random'} {path}: worst err / (e32 s) {worst_ratio:.3g} ({at[0]}), worst err / s {worst_rel:.3g} ({at[1]}), worst err / bound {worst_of_bound:.3g}")
        record_maxima(f"train_grad:F{F}_C{C}_R{R}_B{B}", **{path + "_ratio": worst_ratio, path + "_rel": worst_rel, path + "_of_bound": worst_of_bound})
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("F,C,R,B", list(T.LARGE) + T.ROBUST_EXTRA)
def test_large_batch_step_gradients_vs_float64(F, C, R, B, monkeypatch):
    """ReLU-robust blobs: the six shapes that reach the large-batch kernels, and the two larger shapes of
    test_train_step_on_the_matrix_cores_vs_float64 (where random masks cannot carry this bound)."""
    _check(F, C, R, B, True, 0, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("F,C,R,B", list(T.RANDOM_SMALL))
def test_small_batch_step_gradients_vs_float64_random_masks(F, C, R, B, monkeypatch):
    """Random blobs, so the ReLU masks depend on the data, at the small shapes of the float64 step test."""
    _check(F, C, R, B, False, T.RANDOM_SMALL[(F, C, R, B)], monkeypatch)
