"""kh_train_config's optimizer options on the device (momentum, Nesterov, L2 decay, gradient-norm clipping: csrc/train.hip's
grad_sumsq_kernel / grad_norm_kernel / opt_update_kernel) against the float64 restatement of _train_optim_util — a real
clip_grad_norm_ and torch.optim.SGD living across the call's steps — and the exact contracts of kami_hip.h.

Shapes: F=30, one residual block, 16 filters (12 samples, batch 4: VALU kernels) and 64 filters (24 samples, batch 8:
matrix-core layers, split weight gradients), one epoch = 3 steps; 16 filters with 11 samples, batch 4, two epochs = 6
steps, a ragged batch and a velocity carried across an epoch.  The optimizer kernels see only the blob: wider nets add
nothing, and at 256 filters torch's own fp32 is already 2e-4 from float64 in plain SGD on this data.

Observed on the MI355X (recorded as train_optim:* by conftest.record_maxima, quoted in DESIGN 5.7): every trainable
tensor within 1.4e-7 .. 1.6e-7 of its scale after 3 steps and 2.4e-7 after 6, against the bound of 2e-6; reported norms
within 3.02e-7 (relative) of float64's."""
import ctypes as C_

import numpy as np
import pytest

import _train_optim_util as U
from kami_amd import NN, KamiError, _lib as L

pytestmark = pytest.mark.gpu

MOM = dict(momentum=0.9)
NEST = dict(momentum=0.9, nesterov=True)
WD = dict(weight_decay=1e-2)
ALL = dict(momentum=0.9, nesterov=True, weight_decay=1e-2)
# name -> (options without the threshold, how the threshold is chosen in float64)
OPTIONS = {"momentum": (MOM, None), "nesterov": (NEST, None), "weight_decay": (WD, None), "clip_all": ({}, U.clip_all),
           "clip_some": ({}, U.clip_some), "all_four": (ALL, U.clip_some)}
CASES = [(s, o) for s in ("c16", "c64") for o in OPTIONS] + [("c16_ragged", "all_four")]


# A reported norm against the float64 run's, relative: 2 x the largest error observed on the MI355X over the cases below
# (3.02e-7 at c64_all_four; 1.6e-7 .. 2.7e-7 elsewhere: the norm is one fp32 number, 6e-8 of that is its own rounding, the
# rest the fp32 gradient's).  The project's convention for a tolerance that has no earlier figure.
NORM_TOL = 6.04e-7


def options_of(shape, name):
    opts, pick = OPTIONS[name]
    opts = dict(opts)
    if pick is not None:
        opts["max_grad_norm"] = pick(shape, **opts)
    return opts


def engine(shape, generation=0):
    C = U.SHAPES[shape][0]
    nn = NN(8, 8, U.F, 4672, filters=C, residuals=U.R, dtype="f32")
    nn.load_weights(U.data(shape)[0], generation)
    return nn


def train(nn, shape, **opts):
    _, n, batch, epochs = U.SHAPES[shape]
    _, x, obs_p, obs_v = U.data(shape)
    return nn.train(x, obs_p, obs_v, mlr=5, epochs=epochs, batchsize=batch, **opts)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape,name", CASES)
def test_optimizer_parity_vs_float64(shape, name):
    """Every trainable tensor within 2e-6 of its scale (max(1e-3, |want|.max())) of the float64 run after 3 / 6 steps:
    the project's bound for 2-6 SGD steps.  The expected result differs from the plain-SGD float64 result by at least 50
    times that (1.5e-4 for weight_decay alone, 2.9e-3 .. 3e-1 otherwise), so an engine that ignored the options fails.
    Reported norms: relative error against the float64 norms within NORM_TOL; the number of clipped steps is exact."""
    from conftest import record_maxima
    C = U.SHAPES[shape][0]
    opts = options_of(shape, name)
    want, want_norms = U.float64_run(shape, **opts)
    plain = U.float64_run(shape)[0]
    apart, _ = U.worst_error(want, plain, C)
    assert apart >= 50 * U.BOUND, (apart, opts)                              # the options move the result: float64, on the CPU
    thr = opts.get("max_grad_norm", 0.0)
    if name in ("clip_some", "all_four"):
        assert (want_norms > thr).any() and (want_norms < thr).any(), (thr, want_norms)
    if thr:
        assert (np.abs(want_norms - thr) >= 0.01 * thr).all(), (thr, want_norms)    # fp32 cannot flip a branch
    nn = engine(shape)
    first, last = train(nn, shape, **opts)
    got, norms = nn.get_weights(), nn.last_grad_norms()
    nn.close()
    assert np.isfinite([first, last]).all()
    worst, where = U.worst_error(got, want, C)
    record_maxima(f"train_optim:{shape}_{name}", params=worst)
    print(f"train_optim:{shape}_{name}: worst {worst:.3e} in {where}; float64 apart from plain SGD {apart:.3e}")
    if thr:
        assert norms.shape == want_norms.shape and np.isfinite(norms).all()
        rel = float(np.abs(norms.astype(np.float64) / want_norms - 1.0).max())
        record_maxima(f"train_optim:{shape}_{name}", norm_rel=rel)
        print(f"train_optim:{shape}_{name}: norms {norms}, float64 {want_norms}, worst relative error {rel:.3e}")
        assert int((norms > thr).sum()) == int((want_norms > thr).sum())
        assert rel <= NORM_TOL, (rel, norms, want_norms)
    else:
        assert norms.size == 0
    assert worst <= U.BOUND, (worst, where)


def test_zeroed_options_train_like_a_config_built_the_old_way():
    """blob, losses, generation and kh_bn_batches, bit for bit: keyword defaults against a TrainConfig built
    positionally from the first four fields, as every earlier caller did."""
    shape = "c16_ragged"
    _, n, batch, epochs = U.SHAPES[shape]
    _, x, obs_p, obs_v = U.data(shape)
    a = engine(shape, 3)
    la = train(a, shape)
    b = engine(shape, 3)
    cfg = L.TrainConfig(5 / 1000.0, epochs, batch, 0)
    first, last = C_.c_float(), C_.c_float()
    rc = b._lib.kh_train(b._h, x.ctypes.data_as(C_.c_void_p), obs_p.ctypes.data_as(C_.c_void_p), obs_v.ctypes.data_as(C_.c_void_p),
                         n, C_.byref(cfg), C_.byref(first), C_.byref(last))
    assert rc == L.KH_OK
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert bits(la).tolist() == bits([first.value, last.value]).tolist()
    assert a.get_generation() == b.get_generation() == 4
    assert a.bn_batches() == b.bn_batches() == epochs * -(-n // batch)
    assert a.last_grad_norms().size == 0
    a.close(); b.close()


@pytest.mark.parametrize("shape", ["c16", "c64"])
def test_huge_threshold_is_the_plain_call(shape):
    """max_grad_norm = 1e30 alone: c is exactly 1, the parameters are the plain call's bits; one finite norm per step."""
    a = engine(shape)
    la = train(a, shape)
    b = engine(shape)
    lb = train(b, shape, max_grad_norm=1e30)
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights())) and la == lb
    norms = b.last_grad_norms()
    _, n, batch, epochs = U.SHAPES[shape]
    assert norms.shape == (epochs * -(-n // batch),) and np.isfinite(norms).all() and (norms > 0).all()
    assert a.last_grad_norms().size == 0
    a.close(); b.close()


def _records(n):
    rng = np.random.default_rng(7)
    rec = np.zeros(n, L.RECORD_DTYPE)
    occ = rng.integers(0, 1 << 62, (n, 6), dtype=np.uint64) & rng.integers(0, 1 << 62, (n, 6), dtype=np.uint64)
    rec["board"]["piece_occ"] = occ
    rec["board"]["color_occ"][:, 0] = np.bitwise_or.reduce(occ, axis=1)
    rec["board"]["ply"] = rng.integers(0, 200, n)
    rec["board"]["ctm"] = rng.integers(0, 2, n)
    rec["value"] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n)
    for i in range(n):
        k = int(rng.integers(20, 41))
        rec["nact"][i] = k
        rec["actions"][i, :k] = np.sort(rng.choice(4672, k, replace=False))
        v = rng.random(k).astype(np.float32)
        rec["visits"][i, :k] = v / v.sum()
    return rec


def test_train_records_with_options_equals_train_on_the_expanded_arrays():
    """parameters, statistics, losses and norms, bit for bit; 11 records in batches of 4 over two epochs"""
    shape, opts = "c16_ragged", dict(ALL, max_grad_norm=3.0)
    _, n, batch, epochs = U.SHAPES[shape]
    rec = _records(n)
    a = engine(shape)
    x, p, v = a.expand_records(rec)
    la = a.train(x, p, v, mlr=5, epochs=epochs, batchsize=batch, **opts)
    b = engine(shape)
    lb = b.train_records(rec, mlr=5, epochs=epochs, batchsize=batch, **opts)
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))          # running statistics are part of the blob
    assert la == lb and a.bn_batches() == b.bn_batches() and a.get_generation() == b.get_generation() == 1
    na, nb = a.last_grad_norms(), b.last_grad_norms()
    assert na.size == epochs * -(-n // batch) and np.array_equal(bits(na), bits(nb))
    a.close(); b.close()


def test_same_call_same_bits_also_after_other_options():
    """The same optimizer call twice from the same weights, and once more after a call with different options on the
    same engine (the graph is recorded again, the velocity starts from zero again)."""
    shape, opts = "c64", dict(ALL, max_grad_norm=5.0)
    blob = U.data(shape)[0]
    nn = engine(shape)
    results = []
    for other in (None, None, dict(momentum=0.5, max_grad_norm=100.0)):
        if other is not None:
            train(nn, shape, **other)
        nn.load_weights(blob, 0)
        losses = train(nn, shape, **opts)
        results.append((bits(nn.get_weights()), losses, bits(nn.last_grad_norms())))
    nn.close()
    for w, losses, norms in results[1:]:
        assert np.array_equal(w, results[0][0]) and losses == results[0][1] and np.array_equal(norms, results[0][2])


def test_weight_decay_never_reaches_the_running_statistics():
    """One step (n = batch, one epoch): running_mean / running_var equal the plain one-step call's, bit for bit, while
    the decayed parameters differ."""
    shape = "c16"
    C = U.SHAPES[shape][0]
    _, x, obs_p, obs_v = U.data(shape)
    out = []
    for opts in ({}, dict(weight_decay=0.1)):
        nn = engine(shape)
        nn.train(x[:4], obs_p[:4], obs_v[:4], mlr=5, epochs=1, batchsize=4, **opts)
        out.append(nn.get_weights())
        nn.close()
    seen = 0
    for name, off, k, trainable in U.tensors(C):
        a, b = out[0][off:off + k], out[1][off:off + k]
        if trainable:
            continue
        assert np.array_equal(bits(a), bits(b)), name
        assert not np.array_equal(bits(a), bits(U.data(shape)[0][off:off + k])), name       # the forward did write them
        seen += 1
    assert seen == 2 * (1 + 2 * U.R + 2)
    assert not np.array_equal(bits(out[0]), bits(out[1]))


def test_nesterov_without_momentum_is_rejected_and_changes_nothing():
    shape = "c16"
    nn = engine(shape, 5)
    before = nn.get_weights()
    with pytest.raises(KamiError) as ei:
        train(nn, shape, nesterov=True)
    assert ei.value.status == L.KH_ERR_INVALID and "nesterov" in str(ei.value)
    assert np.array_equal(bits(before), bits(nn.get_weights())) and nn.get_generation() == 5 and nn.bn_batches() == 0
    train(nn, shape, momentum=0.9, nesterov=True)                 # the same engine still trains
    assert nn.get_generation() == 6
    nn.close()
