"""One training step of nn.cpp:59-105 restated on PyTorch CPU tensors in a dtype of the caller's choice, returning the
GRADIENTS (test infrastructure; the same network as tests/test_gpu_train.py::_float64_step, which returns the updated
parameters).  float64 is the reference; float32 is the yardstick the gradient-scale tolerances are derived from: an
independent fp32 implementation of the same step, off from float64 by its own summation order alone.

Also here: the data recipe of the float64 step tests, the ReLU-robust blobs the large-batch comparisons are stated on,
the shapes of tests/test_gpu_train_large_batch.py with the kernels each one reaches, and kh_train_conv_plan's binding."""
import ctypes as C_
import functools

import numpy as np

from kami_amd import _lib as L, weights as W

POLICY_MID = 128          # policyconv's output channels (nn.cpp:73)


def step(blob, F, C, R, x, obs_p, obs_v, dtype):
    """-> dict: grads {tensor name: gradient, float64 ndarray} for every trainable tensor, loss (float), running
    {name: the running_mean / running_var buffers after the forward}, min_z = min |z| over every value entering a ReLU."""
    import torch
    import torch.nn.functional as Fn
    ts, off = {}, 0
    for name, shape in W.tensor_specs(F, C, R):
        k = int(np.prod(shape))
        t = torch.tensor(blob[off:off + k].reshape(shape).astype(np.float64)).to(dtype)
        if "running" not in name:
            t.requires_grad_(True)
        ts[name] = t
        off += k
    min_z = [float("inf")]

    def convbn_relu(h, conv, bn, pad):
        h = Fn.conv2d(h, ts[conv + ".weight"], ts[conv + ".bias"], padding=pad)
        z = Fn.batch_norm(h, ts[bn + ".running_mean"], ts[bn + ".running_var"], ts[bn + ".weight"], ts[bn + ".bias"], True, 0.1, 1e-5)
        min_z[0] = min(min_z[0], float(z.detach().abs().min()))
        return torch.relu(z)
    as_t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)
    h = convbn_relu(as_t(x).permute(0, 3, 1, 2), "conv1", "batchnorm1", 1)
    for i in range(R):
        r = f"residual{i}"
        t = convbn_relu(h, r + ".conv1", r + ".batchnorm1", 1)
        h = h + convbn_relu(t, r + ".conv2", r + ".batchnorm2", 1)
    ph = convbn_relu(h, "policyconv", "pbatchnorm", 0)
    ph = Fn.conv2d(ph, ts["policyconv2.weight"], ts["policyconv2.bias"]).permute(0, 2, 3, 1).flatten(1)
    p = torch.exp(torch.log_softmax(ph, 1))
    vh = convbn_relu(h, "valueconv", "vbatchnorm", 0).flatten(1)
    v = torch.tanh(Fn.linear(vh, ts["valuefc.weight"], ts["valuefc.bias"]))
    tv = as_t(obs_v).reshape(-1, 1).expand_as(v)
    loss = -(as_t(obs_p) * torch.log(p + 0.001)).sum() + Fn.mse_loss(v, tv)
    loss.backward()
    grads = {n: t.grad.detach().double().numpy().copy() for n, t in ts.items() if t.requires_grad}
    running = {n: t.detach().double().numpy().copy() for n, t in ts.items() if not t.requires_grad}
    return {"grads": grads, "loss": float(loss.detach().double()), "running": running, "min_z": min_z[0]}


def robust_blob(blob, F, C, R):
    """A copy of `blob` with every BatchNorm bias overwritten: +8 per channel, -8 where channel % 4 == 3 (vbatchnorm's
    single channel: +8).  BatchNorm's output is gamma * xhat + beta with gamma near 1 and |xhat| of a few units, so a
    channel then passes its ReLU untouched or is dead as a whole: no mask depends on rounding, while the elementwise
    kernels still meet both mask values in every stretch of four channels."""
    out, off = blob.copy(), 0
    for name, shape in W.tensor_specs(F, C, R):
        k = int(np.prod(shape))
        if "batchnorm" in name and name.endswith(".bias"):
            b = np.full(k, 8.0, np.float32)
            if k > 1:
                b[3::4] = -8.0
            out[off:off + k] = b
        off += k
    return out


def make_data(B, F, seed=0):
    """The float64 step tests' data: inputs uniform in [0, 1), 30-entry visit rows summing to 1, values in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, 8, 8, F), dtype=np.float32)
    obs_p = np.zeros((B, 4672), np.float32)
    for i in range(B):
        idx = rng.choice(4672, 30, replace=False)
        v = rng.random(30).astype(np.float32)
        obs_p[i, idx] = v / v.sum()
    obs_v = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), B)
    return x, obs_p, obs_v


# (F, C, R, B) -> what kh_train_conv_plan must say: `two_board` = which of the stem / tower / policy-conv FORWARD
# convolutions run conv_f32_kernel (the others run conv_f32_small_kernel); `wgrad` = {layer: (ranges, boards per
# range, boards of the last range)}.  The smallest batches that reach each path; the arithmetic is in DESIGN.md 5.7.
LARGE = {
    (30, 64, 1, 257): dict(two_board={"stem", "tower", "pconv"}, wgrad={"tower": (129, 2, 1), "pconv": (86, 3, 2)}),
    (119, 24, 1, 259): dict(two_board={"stem", "tower", "pconv"}, wgrad={"stem": (87, 3, 1), "tower": (130, 2, 1)}),
    (30, 128, 1, 131): dict(two_board={"stem", "tower", "pconv"}, wgrad={"tower": (44, 3, 2)}),
    (30, 256, 1, 67): dict(two_board={"stem", "tower"}, wgrad={"tower": (14, 5, 2), "pconv": (23, 3, 1)}),
    (30, 256, 1, 19): dict(two_board=set(), wgrad={"tower": (10, 2, 1)}),
    (30, 64, 1, 254): dict(two_board={"pconv"}, wgrad={"pconv": (127, 2, 2)}),
}
# the two larger shapes of test_train_step_on_the_matrix_cores_vs_float64: random masks cannot carry a gradient-scale
# bound there (no seed keeps every pre-ReLU value away from zero), so they get the robust-blob comparison too
ROBUST_EXTRA = [(119, 64, 1, 64), (30, 256, 1, 6)]
# random blobs (data-dependent ReLU masks) at the small shapes: (F, C, R, B) -> data seed, picked on the CPU as the
# first seed whose float64 step keeps min |z| >= MIN_Z_RANDOM (about 170 x 2^-24: no fp32 rounding reaches a mask)
RANDOM_SMALL = {(30, 64, 2, 8): 0, (30, 24, 1, 5): 1, (30, 128, 1, 12): 9}
MIN_Z_ROBUST, MIN_Z_RANDOM, E32_CAP = 1.0, 1e-5, 2.5e-4
WEIGHT_SEED, PEAKY = 4, 3.0


def layer_shapes(F, C):
    """(ci, co) of the three kinds of matrix-core convolution of a training step"""
    return {"stem": (F, C), "tower": (C, C), "pconv": (C, POLICY_MID)}


def conv_plan(B, ci, co):
    """kh_train_conv_plan -> (two-board kernel?, weight-gradient ranges, boards per range, boards of the last range)"""
    two, ranges, per = C_.c_int(-1), C_.c_int(-1), C_.c_int(-1)
    assert L.load().kh_train_conv_plan(B, ci, co, C_.byref(two), C_.byref(ranges), C_.byref(per)) == L.KH_OK
    return bool(two.value), ranges.value, per.value, B - (ranges.value - 1) * per.value


@functools.lru_cache(maxsize=None)
def case(F, C, R, B, robust=True, seed=0):
    """Blob, data, the float64 and the float32 step of one shape: computed once per session, shared, never modified."""
    import torch
    blob = W.random_weights(F, C, R, seed=WEIGHT_SEED, peaky=PEAKY)
    if robust:
        blob = robust_blob(blob, F, C, R)
    x, obs_p, obs_v = make_data(B, F, seed)
    r64 = step(blob, F, C, R, x, obs_p, obs_v, torch.float64)
    r32 = step(blob, F, C, R, x, obs_p, obs_v, torch.float32)
    for a in (blob, x, obs_p, obs_v):
        a.setflags(write=False)
    return {"blob": blob, "x": x, "obs_p": obs_p, "obs_v": obs_v, "f64": r64, "f32": r32, "scales": grad_scales(r64["grads"])}


def grad_scales(g64):
    """s_T = max |g64_T| per trainable tensor.  A gradient that is identically zero in float64 (s_T <= 1e-12 x the
    net-wide maximum: the conv biases in front of a batch-statistics BatchNorm, whose shift the mean removes; in an
    all-pass residual block batchnorm2.bias too) is measured against the net-wide largest BatchNorm-bias gradient."""
    s = {n: float(np.abs(g).max()) for n, g in g64.items()}
    top = max(s.values())
    bn_bias = max(v for n, v in s.items() if "batchnorm" in n and n.endswith(".bias"))
    return {n: (v if v > 1e-12 * top else bn_bias) for n, v in s.items()}


def e32(c):
    """the float32 step's error per trainable tensor, relative to the tensor's gradient scale"""
    return {n: float(np.abs(c["f32"]["grads"][n] - g).max()) / c["scales"][n] for n, g in c["f64"]["grads"].items()}
