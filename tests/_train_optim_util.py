"""Test infrastructure for kh_train_config's optimizer options: the training call restated in float64 on PyTorch CPU
tensors — the network of test_gpu_train._float64_step, updated by a real torch.nn.utils.clip_grad_norm_ and a real
torch.optim.SGD that live across the call's steps (per-call state, like the reference's optim::SGD inside NN::train)."""
import ctypes as C_
import functools

import numpy as np

from kami_amd import weights as W, _lib as L

F, R = 30, 1
LR = 0.005
BOUND = 2e-6                    # the project's bound for 2-6 SGD steps against float64 (test_train_multi_batch_epochs_vs_float64)
# (filters, samples, batch, epochs): 16 filters on the VALU kernels; 64 on the matrix cores with split weight gradients;
# 11 samples in batches of 4 over two epochs: a ragged batch and a velocity carried across an epoch
SHAPES = {"c16": (16, 12, 4, 1), "c64": (64, 24, 8, 1), "c16_ragged": (16, 11, 4, 2)}


@functools.lru_cache(maxsize=None)
def data(shape):
    """The recipe of test_train_multi_batch_epochs_vs_float64: default_rng(1), random_weights(seed=6, peaky=3.0),
    25-entry visit rows, values in {-1, 0, 1}."""
    C, n, batch, epochs = SHAPES[shape]
    rng = np.random.default_rng(1)
    blob = W.random_weights(F, C, R, seed=6, peaky=3.0)
    x = rng.random((n, 8, 8, F), dtype=np.float32)
    obs_p = np.zeros((n, 4672), np.float32)
    for i in range(n):
        idx = rng.choice(4672, 25, replace=False)
        v = rng.random(25).astype(np.float32)
        obs_p[i, idx] = v / v.sum()
    obs_v = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n)
    for a in (blob, x, obs_p, obs_v):
        a.setflags(write=False)
    return blob, x, obs_p, obs_v


def tensors(C):
    """[(name, offset, count, trainable)] in blob order"""
    out, off = [], 0
    for name, shape in W.tensor_specs(F, C, R):
        k = int(np.prod(shape))
        out.append((name, off, k, "running" not in name))
        off += k
    return out


def _run(shape, momentum, nesterov, weight_decay, max_grad_norm):
    import torch
    import torch.nn.functional as Fn
    C, n, batch, epochs = SHAPES[shape]
    blob, x, obs_p, obs_v = data(shape)
    ts, off = {}, 0
    for name, shp in W.tensor_specs(F, C, R):
        k = int(np.prod(shp))
        t = torch.tensor(blob[off:off + k].reshape(shp).astype(np.float64))
        if "running" not in name:
            t.requires_grad_(True)
        ts[name] = t
        off += k
    params = [t for t in ts.values() if t.requires_grad]
    opt = torch.optim.SGD(params, lr=LR, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov)

    def convbn(h, conv, bn, pad):
        h = Fn.conv2d(h, ts[conv + ".weight"], ts[conv + ".bias"], padding=pad)
        return Fn.batch_norm(h, ts[bn + ".running_mean"], ts[bn + ".running_var"], ts[bn + ".weight"], ts[bn + ".bias"], True, 0.1, 1e-5)

    def loss_of(bx, bp, bv):
        h = torch.tensor(bx.astype(np.float64)).permute(0, 3, 1, 2)
        h = torch.relu(convbn(h, "conv1", "batchnorm1", 1))
        for i in range(R):
            r = f"residual{i}"
            t = torch.relu(convbn(h, r + ".conv1", r + ".batchnorm1", 1))
            h = h + torch.relu(convbn(t, r + ".conv2", r + ".batchnorm2", 1))
        ph = torch.relu(convbn(h, "policyconv", "pbatchnorm", 0))
        ph = Fn.conv2d(ph, ts["policyconv2.weight"], ts["policyconv2.bias"]).permute(0, 2, 3, 1).flatten(1)
        p = torch.exp(torch.log_softmax(ph, 1))
        vh = torch.relu(convbn(h, "valueconv", "vbatchnorm", 0)).flatten(1)
        v = torch.tanh(Fn.linear(vh, ts["valuefc.weight"], ts["valuefc.bias"]))
        tv = torch.tensor(bv.astype(np.float64)).reshape(-1, 1).expand_as(v)
        return -(torch.tensor(bp.astype(np.float64)) * torch.log(p + 0.001)).sum() + Fn.mse_loss(v, tv)

    order = np.empty(epochs * n, np.int32)
    assert L.load().kh_train_order(n, epochs, order.ctypes.data_as(C_.c_void_p)) == 0
    # a short last batch keeps the previous batch's rows behind its own (the staging buffers persist)
    sx, sp, sv = np.zeros((batch,) + x.shape[1:], np.float32), np.zeros((batch, 4672), np.float32), np.zeros(batch, np.float32)
    norms = []
    for e in range(epochs):
        o = order[e * n:(e + 1) * n]
        for base in range(0, n, batch):
            idx = o[base:base + batch]
            sx[:len(idx)], sp[:len(idx)], sv[:len(idx)] = x[idx], obs_p[idx], obs_v[idx]
            opt.zero_grad()
            loss_of(sx, sp, sv).backward()
            if max_grad_norm > 0:
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_grad_norm)))
            else:
                norms.append(float(torch.sqrt(sum((p.grad ** 2).sum() for p in params))))
            opt.step()
    out = np.concatenate([ts[name].detach().numpy().ravel() for name, _ in W.tensor_specs(F, C, R)])
    out.setflags(write=False)
    return out, np.array(norms)


@functools.lru_cache(maxsize=None)
def float64_run(shape, momentum=0.0, nesterov=False, weight_decay=0.0, max_grad_norm=0.0):
    """-> (the blob after the call, float64; every step's gradient norm before clipping).  Computed once per argument
    set and shared; both arrays are read-only."""
    return _run(shape, float(momentum), bool(nesterov), float(weight_decay), float(max_grad_norm))


def clip_all(shape, **opts):
    """Half the smallest norm of the unclipped float64 run with these options, and checked in float64: with it every
    step of the run is clipped, every norm at least 1 % away from it."""
    thr = 0.5 * float(float64_run(shape, **opts)[1].min())
    norms = float64_run(shape, max_grad_norm=thr, **opts)[1]
    assert (norms > 1.01 * thr).all(), (thr, norms)
    return thr


def clip_some(shape, **opts):
    """A threshold that clips some steps of the float64 run and not others: the first midpoint between two neighbouring
    norms of the unclipped run (ascending) for which the CLIPPED run — whose later norms differ — has steps on both
    sides, each at least 1 % away from the threshold, so that fp32 cannot flip a branch."""
    base = np.sort(float64_run(shape, **opts)[1])
    for lo, hi in zip(base[:-1], base[1:]):
        thr = float(np.sqrt(lo * hi))
        norms = float64_run(shape, max_grad_norm=thr, **opts)[1]
        if (norms > thr).any() and (norms < thr).any() and (np.abs(norms - thr) >= 0.01 * thr).all():
            return thr
    raise AssertionError(f"no threshold splits the steps of {shape} {opts}: unclipped norms {base}")


def worst_error(got, want, C):
    """max over the trainable tensors of |got - want|.max() / max(1e-3, |want|.max()), and the tensor it occurs in"""
    worst, where = 0.0, None
    for name, off, k, trainable in tensors(C):
        if not trainable:
            continue
        a, b = np.asarray(got[off:off + k], np.float64), want[off:off + k]
        w = float(np.abs(a - b).max()) / max(1e-3, float(np.abs(b).max()))
        if w > worst:
            worst, where = w, name
    return worst, where
