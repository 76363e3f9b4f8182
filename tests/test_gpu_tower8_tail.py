"""The headline kernel's tail (tower8_kernel: policyconv2 on three row tiles, the softmax's row max reduced from the
accumulators and published with the logits) against the fp32 oracle, at the batch shapes that exercise its board-group bookkeeping.  Run with -m gpu."""
import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from oracle import pyoracle as ko

pytestmark = pytest.mark.gpu

# the 6-block tolerances of tests/test_gpu_parity.py (TOL_BY_DEPTH[6])
TOL = {"f16": dict(logp=1.3e-2, prob_rtol=1.3e-2, value=2.2e-4),
       "bf16": dict(logp=1.3e-1, prob_rtol=1.2e-1, value=2.0e-3)}


def check(dtype, got, want, key):
    p, vf, lg = got
    op, ovf, olg = want
    tol = TOL[dtype]
    dlogp = float(np.abs(np.log(p) - np.log(op)).max())
    big = op > 1e-6
    drel = float((np.abs(p[big] - op[big]) / op[big]).max())
    dval = float(np.abs(vf - ovf).max())
    assert dlogp <= tol["logp"], (key, dlogp)
    assert drel <= tol["prob_rtol"], (key, drel)
    assert dval <= tol["value"], (key, dval)
    if lg is not None:
        assert float(np.abs(lg - olg).max()) <= tol["logp"], key
    assert np.allclose(p.sum(1), 1.0, atol=1e-3), key


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 37, 257, 513, 2048])
def test_tail_vs_oracle_batches(dtype, B):
    """B = 2048: every workgroup walks several board groups, so [BE] and the row-max scratch are reused; 1, 37, 513:
    a dead board in the last group; 257: fewer workgroups than CUs."""
    F, C, R = 119, 64, 6
    blob = W.random_weights(F, C, R, seed=11, peaky=20.0)
    x = np.random.default_rng(B + 5).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    p, vf, lg = nn.infer_full(x)
    check(dtype, (p, vf, lg), ko.forward(blob, F, C, R, x), f"F{F}_B{B}")
    # the plain entry point (no logits copy-out) gives the same rows
    p2, vf2, _ = nn.infer_full(x, want_logits=False)
    assert np.array_equal(p2, p) and np.array_equal(vf2, vf)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_tail_f30_short_stem(dtype):
    """F = 30: the five-chunk stem leaves the stream on odd parity, so the policy steps end with the dummy chunk."""
    F, C, R, B = 30, 64, 6, 97
    blob = W.random_weights(F, C, R, seed=12, peaky=20.0)
    x = np.random.default_rng(7).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    check(dtype, nn.infer_full(x), ko.forward(blob, F, C, R, x), f"F{F}_B{B}")


def _records(n, seed):
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=L.BOARD_DTYPE)
    code = rng.integers(-12, 12, size=(n, 64))
    for t in range(6):
        for col in range(2):
            m = (code == 2 * t + col)
            bits = (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
            b["piece_occ"][:, t] |= bits
            b["color_occ"][:, col] |= bits
    b["ply"] = rng.integers(0, 70000, n)
    b["halfmove_clock"] = rng.integers(0, 200, n)
    b["ctm"] = rng.integers(0, 2, n)
    b["castle_rights"] = rng.integers(0, 16, n)
    nact = rng.integers(0, 40, n)
    offs = np.concatenate([[0], np.cumsum(nact)]).astype(np.int32)
    acts = rng.integers(0, 4672, int(offs[-1])).astype(np.int32)
    return b, offs, acts


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [1, 37, 600])
def test_tail_legal_move_path(dtype, n):
    """kh_encode_infer_legal (F = 30, compact records, the LEGAL instantiation): the priors are the renormalised gather
    of encode_infer's policy rows and the values equal encode_infer's bit for bit."""
    F, C, R = 30, 64, 6
    blob = W.random_weights(F, C, R, seed=13, peaky=20.0)
    boards, offs, acts = _records(n, 100 + n)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    priors, value = nn.infer_legal(boards, offs, acts)
    policy, value2 = nn.encode_infer(boards)
    assert np.array_equal(value, value2)
    for i in range(n):
        a = acts[offs[i]:offs[i + 1]]
        if len(a) == 0:
            continue
        want = policy[i, a] / policy[i, a].sum(dtype=np.float32)
        np.testing.assert_allclose(priors[offs[i]:offs[i + 1]], want, rtol=2e-6, atol=1e-9)


def _poisoned(blob, F, C, R, name, idx, val):
    d = W.split(blob.copy(), F, C, R)
    d[name].reshape(-1)[idx] = val
    return np.concatenate([v.ravel() for v in d.values()])


@pytest.mark.parametrize("F", [119, 30])
def test_tail_nan_contract(F):
    """A NaN plane, a poisoned residual stream and a NaN value output still raise the reference's strings."""
    C, R, B = 64, 6, 5
    blob = W.random_weights(F, C, R, seed=14)
    x = np.random.default_rng(3).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(blob, 1)
    nn.infer(x)
    xb = x.copy()
    xb[B - 1, 4, 2, F - 1] = np.nan
    with pytest.raises(KamiError) as ei:
        nn.infer(xb)
    assert ei.value.status == L.KH_ERR_NAN_POLICY
    assert str(ei.value) == "inference policy output contains NaN"
    # an infinite BatchNorm shift in the last block: the residual stream is poisoned after the ReLUs
    nn.load_weights(_poisoned(blob, F, C, R, f"residual{R - 1}.batchnorm2.bias", 3, np.inf), 2)
    with pytest.raises(KamiError) as ei:
        nn.infer(x)
    assert ei.value.status == L.KH_ERR_NAN_POLICY
    assert str(ei.value) == "inference policy output contains NaN"
    # NaN in the value head only
    nn.load_weights(_poisoned(blob, F, C, R, "valuefc.bias", 200, np.nan), 3)
    with pytest.raises(KamiError) as ei:
        nn.infer(x)
    assert ei.value.status == L.KH_ERR_NAN_VALUE
    assert str(ei.value) == "inference value output contains NaN"
    nn.load_weights(blob, 4)
    nn.infer(x)
