"""Every forward path's value head on nets whose head is ALIVE (tests/_forward_ref.py: about half of each board's value
plane passes the ReLU, rows differ from board to board, tanh works in its curved range), against the float64 forward,
all 256 columns, together with the logits.  Bounds: bf16 / f16 twice the rounding model's own error on the case,
f32 eight times the fp32 C oracle's; tests/test_forward_ref.py shows on the CPU that every defect of
_forward_ref.MUTATIONS moves the float64 output by at least three times these bounds.  Run with -m gpu."""
import numpy as np
import pytest

from kami_amd import NN, _lib as L
from conftest import record_maxima

import _forward_ref as FR

pytestmark = pytest.mark.gpu

PARAMS = [(n, d) for n, c in FR.CASES.items() for d in c["dtypes"]]


def make_nn(c, dtype, **kw):
    nn = NN(8, 8, c["F"], 4672, filters=c["C"], residuals=c["R"], dtype=dtype, **kw)
    nn.load_weights(c["blob"], 1)
    return nn


def within(c, dtype, **errs):
    """print, record (error / bound under the case's key) and assert each quantity's error against the case's bound"""
    ratios = {q: e / c["bound"][dtype][q] for q, e in errs.items()}
    print(FR.key(c, dtype), " ".join(f"{q} {errs[q]:.3e} / {c['bound'][dtype][q]:.3e} = {ratios[q]:.2f}" for q in errs))
    record_maxima(FR.key(c, dtype), **{q + "_over_bound": r for q, r in ratios.items()})
    for q, r in ratios.items():
        assert r <= 1.0, (FR.key(c, dtype), q, errs[q], c["bound"][dtype][q])


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_live_value_head_vs_float64(name, dtype, monkeypatch):
    c = FR.case(name)
    if c["simple"]:
        monkeypatch.setenv("KAMI_F32_SIMPLE", "1")                # read when the engine is created
    nn = make_nn(c, dtype)
    if c["records"]:
        # encode_infer returns the policy and the value copy-out only: the flat mode gives board 0's columns 0 .. B - 1,
        # the per-sample mode column 0 of every board; log-probabilities stand in for the logits, with their own bound
        # of the same form
        B = c["B"]
        p, v = nn.encode_infer(c["boards"])
        _, v0 = make_nn(c, dtype, value_mode=L.KH_VALUE_PER_SAMPLE0).encode_infer(c["boards"])
        ev = max(float(np.abs(v - c["value"].reshape(-1)[:B]).max()), float(np.abs(v0 - c["value"][:, 0]).max()))
        within(c, dtype, value=ev, logp=float(np.abs(np.log(p.astype(np.float64)) - c["logp"]).max()))
    else:
        p, vf, lg = nn.infer_full(c["x"])
        assert vf.shape == c["value"].shape == (c["B"], 256)
        within(c, dtype, value=float(np.abs(vf - c["value"]).max()), logit=float(np.abs(lg - c["logits"]).max()))
    assert np.abs(p.sum(1, dtype=np.float64) - 1.0).max() <= 1e-3


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["copy_b5", "copy_b300"])
def test_value_copyout_modes_on_distinct_rows(name, dtype):
    """KH_VALUE_REFERENCE_FLAT copies the first B entries of the flattened [B, 256] tensor (nn.cpp:186: at B = 300
    entries 256 .. 299 are board 1's columns 0 .. 43), KH_VALUE_PER_SAMPLE0 column 0 of every board: bit for bit the
    entries of value_full, within the bound of the float64 rows, and apart from each other by more than ten bounds,
    which identical rows (a dead head) could not deliver."""
    c = FR.case(name)
    B, bound = c["B"], c["bound"][dtype]["value"]
    flat, per = make_nn(c, dtype), make_nn(c, dtype, value_mode=L.KH_VALUE_PER_SAMPLE0)
    _, vf, _ = flat.infer_full(c["x"], want_logits=False)
    _, vf0, _ = per.infer_full(c["x"], want_logits=False)
    assert np.array_equal(vf, vf0)
    v, v0 = flat.infer(c["x"])[1], per.infer(c["x"])[1]
    assert np.array_equal(v, vf.reshape(-1)[:B])
    assert np.array_equal(v0, vf[:, 0])
    if B > 256:
        assert np.array_equal(v[256:], vf[1, :B - 256])
    assert float(np.abs(v - c["value"].reshape(-1)[:B]).max()) <= bound
    assert float(np.abs(v0 - c["value"][:, 0]).max()) <= bound
    assert float(np.abs(v - v0).max()) > 10.0 * bound


@pytest.mark.parametrize("name", ["t2s_c256_b17", "t8_f30_b17"])
def test_rows_follow_their_boards(name):
    """The boards in reversed order give the rows in reversed order, values (256 distinct columns per board) and
    logits.  Bit for bit: the batch size and with it the plan are the same in both calls (tower2s_kernel +
    policy_head4_kernel<T,2>, and tower8_kernel), a board only changes its group and keeps its slot's parity, and no
    kernel's arithmetic on a board depends on its neighbours."""
    c = FR.case(name)
    nn = make_nn(c, "bf16")
    p, vf, lg = nn.infer_full(c["x"])
    pr, vfr, lgr = nn.infer_full(np.ascontiguousarray(c["x"][::-1]))
    assert float(np.abs(vf[0] - vf[-1]).max()) > 10.0 * c["bound"]["bf16"]["value"]      # the rows ARE distinct
    assert np.array_equal(vfr[::-1], vf) and np.array_equal(lgr[::-1], lg) and np.array_equal(pr[::-1], p)
