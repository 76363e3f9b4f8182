"""Parity tests proper: the HIP path (through the C ABI) against the golden fixtures produced by
the unmodified reference, and against the CPU oracle on seeded inputs.  Run with -m gpu."""
import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from oracle import pyoracle as ko
from conftest import record_maxima

pytestmark = pytest.mark.gpu

# Tolerances per arithmetic type and depth class, vs the fp32 reference / oracle: each entry is <= 2x the maximum
# this suite OBSERVED on the MI355X (profiles/r02_parity_maxima.json, written by conftest.record_maxima; per test
# key there).  logp = log-probabilities and pre-softmax logits, prob_rtol = relative error of probabilities
# > 1e-6, value = the tanh output.  Low-precision error grows with the number of blocks, so the deep BASELINE
# configurations (10 and 20 blocks) carry their own, measured at full depth.
TOL_BY_DEPTH = {
    6: {"f32": dict(logp=1.6e-5, prob_rtol=1.6e-5, value=7.5e-7),      # observed 7.6e-6 / 7.9e-6 / 3.6e-7
        "f16": dict(logp=1.3e-2, prob_rtol=1.3e-2, value=2.2e-4),      # observed 6.5e-3 / 6.5e-3 / 1.1e-4
        "bf16": dict(logp=1.3e-1, prob_rtol=1.2e-1, value=2.0e-3)},    # observed 6.6e-2 / 6.1e-2 / 9.9e-4
    10: {"f32": dict(logp=1.8e-5, prob_rtol=1.7e-5, value=9e-7),       # observed 8.6e-6 / 8.3e-6 / 4.5e-7
         "f16": dict(logp=1.7e-2, prob_rtol=1.6e-2, value=7e-4),       # observed 8.4e-3 / 7.8e-3 / 3.5e-4
         "bf16": dict(logp=1.4e-1, prob_rtol=1.3e-1, value=4.8e-3)},   # observed 7.1e-2 / 6.5e-2 / 2.4e-3
    20: {"f32": dict(logp=3.8e-5, prob_rtol=3.7e-5, value=1.3e-6),     # observed 1.9e-5 / 1.8e-5 / 6.4e-7
         "f16": dict(logp=5.4e-2, prob_rtol=5.3e-2, value=1.8e-3),     # observed 2.7e-2 / 2.7e-2 / 9.1e-4
         "bf16": dict(logp=3.9e-1, prob_rtol=3.6e-1, value=1.4e-2)},   # observed 1.9e-1 / 1.8e-1 / 7.0e-3
}
TOL = TOL_BY_DEPTH[6]


def tol_for(dtype, residuals):
    return TOL_BY_DEPTH[6 if residuals <= 6 else (10 if residuals <= 10 else 20)][dtype]


def compare(key, dtype, got, want, tol=None):
    """got / want = (policy, value_full, logits or None).  Records the observed maxima under `key` (conftest.record_maxima
    -> gpurun_out/parity_maxima.json) and asserts them against the stated tolerance of the arithmetic type."""
    tol = tol or TOL[dtype]
    p, vf, lg = got
    op, ovf, olg = want
    dlogp = float(np.abs(np.log(p) - np.log(op)).max())
    dval = float(np.abs(vf - ovf).max())
    big = op > 1e-6
    drel = float((np.abs(p[big] - op[big]) / op[big]).max()) if big.any() else 0.0
    vals = dict(logp=dlogp, prob_rel=drel, value=dval)
    if lg is not None and olg is not None:
        vals["logit"] = float(np.abs(lg - olg).max())
    record_maxima(f"{dtype}:{key}", **vals)
    assert dlogp <= tol["logp"], (key, dtype, vals)
    assert drel <= tol["prob_rtol"], (key, dtype, vals)
    assert dval <= tol["value"], (key, dtype, vals)
    if "logit" in vals:
        assert vals["logit"] <= tol["logp"], (key, dtype, vals)


def make_nn(d, dtype="f32", **kw):
    nn = NN(8, 8, d["features"], 4672, filters=d["filters"], residuals=d["residuals"], dtype=dtype, **kw)
    nn.load_weights(d["blob"], d["generation"])
    return nn


def random_boards(n, seed):
    """Synthetic records covering every field the encoder reads (not necessarily legal chess)."""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=L.BOARD_DTYPE)
    # each square: empty (p=.5) or one of 12 pieces
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
    return b


# ------------------------------------------------------------------------------ encoding
def test_encode_fixture_bit_exact(observe_fixture):
    f = observe_fixture
    boards = ko.boards_from_fens([s.decode() for s in f["fen"]], f["ply"])
    nn = NN(filters=8, residuals=0)
    got = nn.encode(boards).reshape(len(boards), -1)
    want = f["obs"].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000, 200003])
def test_encode_random_boards_vs_oracle(n):
    boards = random_boards(n, seed=n)
    nn = NN(filters=8, residuals=0)
    got = nn.encode(boards)
    want = ko.observe(boards)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_encode_empty_batch():
    nn = NN(filters=8, residuals=0)
    out = nn.encode(np.zeros(0, dtype=L.BOARD_DTYPE))
    assert out.shape == (0, 8, 8, 30)


# ------------------------------------------------------------------------------ forward
def check_forward(nn, d, dtype):
    policy, vfull, logits = nn.infer_full(d["x"])
    rows = d["policy_rows"]
    assert np.allclose(policy.sum(1), 1.0, atol=1e-3)
    # logits vs the oracle's logits (the reference does not expose them)
    _, _, ologits = ko.forward(d["blob"], d["features"], d["filters"], d["residuals"], d["x"])
    compare("fixture/" + d["name"], dtype, (policy[rows], vfull, logits[rows]), (d["policy"], d["value_full"], ologits[rows]))


def test_forward_f32_vs_reference_fixtures(net_fixture):
    nn = make_nn(net_fixture, "f32")
    check_forward(nn, net_fixture, "f32")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_forward_mfma_vs_reference_fixtures(net_fixture, dtype):
    """The whole-network MFMA kernel (bf16 / f16 operands, fp32 accumulate) vs the reference's
    fp32 outputs, within the stated per-dtype tolerance (TOL)."""
    nn = make_nn(net_fixture, dtype)
    check_forward(nn, net_fixture, dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("F,C,R,B", [(119, 64, 6, 64), (30, 64, 6, 33), (30, 24, 1, 7), (119, 64, 0, 3),
                                     # 33..128 planes take the four-pass stem: ragged rows on both sides of the splits
                                     (33, 64, 1, 5), (61, 48, 1, 3), (64, 64, 1, 4), (67, 64, 1, 3), (100, 64, 2, 7), (128, 64, 1, 2),
                                     # the headline net at a batch with an odd last board group and at a small one
                                     (119, 64, 6, 37), (119, 64, 6, 16)])
def test_forward_mfma_vs_oracle(dtype, F, C, R, B):
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=20.0)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    p, vf, lg = nn.infer_full(x)
    compare(f"oracle/F{F}_{R}x{C}_B{B}", dtype, (p, vf, lg), ko.forward(blob, F, C, R, x))
    assert np.allclose(p.sum(1), 1.0, atol=1e-3)


@pytest.mark.parametrize("dtype", ["bf16"])
def test_mfma_batch_sizes_and_row_independence(dtype):
    F, C, R = 30, 64, 2
    blob = W.random_weights(F, C, R, seed=2, peaky=10.0)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    x = np.random.default_rng(0).random((1027, 8, 8, F), dtype=np.float32)
    p_all, vf_all, _ = nn.infer_full(x, want_logits=False)
    for b in (1, 2, 63, 513):
        p, vf, _ = nn.infer_full(x[:b], want_logits=False)
        assert np.array_equal(p, p_all[:b]) and np.array_equal(vf, vf_all[:b])
    # determinism: same call twice is bit-identical
    p2, vf2, _ = nn.infer_full(x, want_logits=False)
    assert np.array_equal(p2, p_all) and np.array_equal(vf2, vf_all)


def test_mfma_nan_guard():
    F, C, R = 30, 64, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    blob = W.random_weights(F, C, R, seed=3)
    nn.load_weights(blob, 1)
    x = np.random.default_rng(0).random((3, 8, 8, F), dtype=np.float32)
    nn.infer(x)
    xb = x.copy()
    xb[2, 3, 3, 1] = np.nan
    with pytest.raises(KamiError) as ei:
        nn.infer(xb)
    assert ei.value.status == L.KH_ERR_NAN_POLICY


@pytest.mark.parametrize("ch", [0, 63, 64, 118])
def test_mfma_nan_guard_two_pass_stem(ch):
    """F = 119 ingests the planes in four quarters of 32 channels (the first before the stem, the rest under it):
    a non-finite plane in any quarter, in the last board of an odd batch, is still flagged."""
    F, C, R = 119, 64, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, C, R, seed=3), 1)
    x = np.random.default_rng(0).random((3, 8, 8, F), dtype=np.float32)
    nn.infer(x)
    x[2, 7, 7, ch] = np.inf
    with pytest.raises(KamiError) as ei:
        nn.infer(x)
    assert ei.value.status == L.KH_ERR_NAN_POLICY


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("F,C,R,B", [(119, 128, 3, 9), (30, 256, 2, 5), (30, 96, 1, 4), (200, 64, 1, 3)])
def test_forward_wide_nets_vs_oracle(dtype, F, C, R, B):
    """Nets the whole-network kernel does not cover (filters > 64 or features > 128) run the
    per-layer MFMA path (layers_mfma.hip): BASELINE configs 3 and 5 shapes, small batch."""
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=20.0)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    p, vf, lg = nn.infer_full(x)
    compare(f"oracle-wide/F{F}_{R}x{C}_B{B}", dtype, (p, vf, lg), ko.forward(blob, F, C, R, x))
    # NaN guard on this path too
    xb = x.copy(); xb[B - 1, 0, 0, 0] = np.nan
    with pytest.raises(KamiError) as ei:
        nn.infer(xb)
    assert ei.value.status == L.KH_ERR_NAN_POLICY
    # ... and the raised flag does not outlive the call that reported it (the flags are cleared on demand, not per forward)
    p2, _ = nn.infer(x)
    assert np.array_equal(p2, p)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("C,B,step", [(128, 513, 100), (128, 1024, 100), (128, 1021, 255), (256, 200, 50), (256, 131, 50), (256, 600, 300), (256, 515, 103)])
def test_wide_two_workgroups_per_cu_variant_matches(dtype, C, B, step):
    """Wide nets: the launcher picks the 3x3 layer kernel per call — one workgroup per CU with a 4-slot ring (small
    batches), two or three per CU with a 2-slot ring and passes of 128 / 64 input channels, and from 256 workgroups of
    FOUR boards x 128 output channels on conv4_mfma_kernel (128 channels: batch >= 1021; 256 channels: batch >= 509).
    All of them walk the reduction in the same order with the same fp32 epilogue: the same boards evaluated `step`
    at a time (another variant) must give the same bits, ragged last groups included.
    256 filters since round 3: batches up to 256 run tower2s_kernel (two workgroups per board pair, each half the
    output channels; channels >= 128 sum their 64-channel slices in the order 2,3,0,1), larger ones tower2b_kernel
    (0,1,2,3): bit-identical within each range ((200, 50), (131, 50), (600, 300)), equal to rounding across the two
    ((515, 103): observed 1.2e-2 on logits / 7e-4 on probabilities / 7e-4 on values in f16 at TWENTY blocks, 8.9e-2 /
    3.9e-3 / 4.8e-3 in bf16 — profiles/r03_tower2s_ab_stamps.txt; both ranges are pinned against the oracle at full depth by
    test_full_size_properties_wide_configs)."""
    F, R = 119, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(W.random_weights(F, C, R, seed=77, peaky=10.0), 1)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    p, vf, lg = nn.infer_full(x)
    across = C == 256 and B > 256 >= step
    tl, tp, tv = (1e-1, 5e-3, 6e-3) if dtype == "bf16" else (1.5e-2, 1e-3, 1e-3)
    for lo in range(0, B, step):
        pp, pv, pl = nn.infer_full(x[lo:lo + step])
        if across:
            np.testing.assert_allclose(lg[lo:lo + step], pl, atol=tl, rtol=0)
            np.testing.assert_allclose(p[lo:lo + step], pp, atol=tp, rtol=0)
            np.testing.assert_allclose(vf[lo:lo + step], pv, atol=tv, rtol=0)
            continue
        np.testing.assert_array_equal(lg[lo:lo + step], pl)
        np.testing.assert_array_equal(p[lo:lo + step], pp)
        np.testing.assert_array_equal(vf[lo:lo + step], pv)


def test_mfma_unsupported_config_fails_loudly():
    nn = NN(8, 8, 30, 4672, filters=320, residuals=1, dtype="bf16")
    nn.load_weights(W.random_weights(30, 320, 1, seed=1), 1)
    with pytest.raises(KamiError) as ei:
        nn.infer(np.zeros((1, 8, 8, 30), np.float32))
    assert ei.value.status == L.KH_ERR_INVALID


def test_forward_f32_exact_order_kernels(net_fixture, monkeypatch):
    """KAMI_F32_SIMPLE=1: the plain VALU kernels in the oracle's accumulation order (the anchor the
    exact-f32 MFMA path is cross-checked against)."""
    monkeypatch.setenv("KAMI_F32_SIMPLE", "1")
    nn = make_nn(net_fixture, "f32")
    check_forward(nn, net_fixture, "f32")
    monkeypatch.delenv("KAMI_F32_SIMPLE")
    nn2 = make_nn(net_fixture, "f32")
    p1, v1, l1 = nn.infer_full(net_fixture["x"])
    p2, v2, l2 = nn2.infer_full(net_fixture["x"])
    np.testing.assert_allclose(l1, l2, atol=1e-4, rtol=0)     # two fp32 summation orders
    np.testing.assert_allclose(v1, v2, atol=1e-5, rtol=0)


def test_infer_reference_value_copyout(net_fixture):
    """value[i] = flattened [B,256] tensor element i (nn.cpp:186)."""
    d = net_fixture
    nn = make_nn(d, "f32")
    policy, value = nn.infer(d["x"])
    np.testing.assert_allclose(value, d["value"], atol=TOL["f32"]["value"], rtol=0)
    nn2 = make_nn(d, "f32", value_mode=L.KH_VALUE_PER_SAMPLE0)
    _, v0 = nn2.infer(d["x"])
    np.testing.assert_allclose(v0, d["value_full"][:, 0], atol=TOL["f32"]["value"], rtol=0)


@pytest.mark.parametrize("F,C,R,B", [(119, 64, 6, 48), (30, 64, 6, 16), (30, 24, 1, 7), (119, 128, 2, 5)])
def test_forward_f32_vs_oracle_bigger_nets(F, C, R, B):
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=20.0)
    x = np.random.default_rng(B).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(blob, 1)
    p, vf, lg = nn.infer_full(x)
    compare(f"oracle/F{F}_{R}x{C}_B{B}", "f32", (p, vf, lg), ko.forward(blob, F, C, R, x))


def test_batch_sizes_and_row_independence():
    """infer must take any batch >= 1 (evaluate.cpp:136-151) and rows must not interact."""
    F, C, R = 30, 16, 1
    blob = W.random_weights(F, C, R, seed=2, peaky=10.0)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(blob, 1)
    x = np.random.default_rng(0).random((513, 8, 8, F), dtype=np.float32)
    p_all, vf_all, _ = nn.infer_full(x, want_logits=False)
    for b in (1, 2, 63, 257):
        p, vf, _ = nn.infer_full(x[:b], want_logits=False)
        assert np.array_equal(p, p_all[:b]) and np.array_equal(vf, vf_all[:b])


def test_encode_infer_equals_encode_then_infer(observe_fixture):
    f = observe_fixture
    boards = ko.boards_from_fens([s.decode() for s in f["fen"][:40]], f["ply"][:40])
    F, C, R = 30, 16, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(W.random_weights(F, C, R, seed=8, peaky=10.0), 3)
    p1, v1 = nn.encode_infer(boards)
    p2, v2 = nn.infer(nn.encode(boards))
    assert np.array_equal(p1, p2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_ingest_equals_encode_then_infer(observe_fixture, dtype):
    """Compact ingest with the encoder INSIDE the forward kernel (bf16/f16, <= 64 filters) must equal
    encode -> planes -> infer bit for bit: plane values 0/1/2/4/8 are exact in both formats."""
    f = observe_fixture
    sel = np.arange(0, len(f["fen"]), 5)[:201]                   # odd count: last group is half empty
    boards = ko.boards_from_fens([f["fen"][i].decode() for i in sel], f["ply"][sel])
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(W.random_weights(F, C, R, seed=31, peaky=20.0), 3)
    p1, v1 = nn.encode_infer(boards)                             # fused kernel
    p2, v2 = nn.infer(nn.encode(boards))                         # encode kernel, planes through the host
    assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
    op, ovf, _ = ko.forward(nn._blob, F, C, R, ko.observe(boards[:8]))
    np.testing.assert_allclose(np.log(p1[:8]), np.log(op), atol=TOL[dtype]["logp"], rtol=0)


def test_legal_move_gather_matches_expand_renormalisation(observe_fixture):
    """priors = policy[legal] / sum(policy[legal]) (MCTS::expand, mcts.h:273-276,296) with the
    reference's own legal-action lists (Env::actions) from the fixture."""
    f = observe_fixture
    sel = np.arange(0, len(f["fen"]), 9)[:100]
    boards = ko.boards_from_fens([f["fen"][i].decode() for i in sel], f["ply"][sel])
    nact = f["nact"][sel].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(nact)]).astype(np.int32)
    acts = np.concatenate([f["actions"][i, :f["nact"][i]] for i in sel]).astype(np.int32)
    F, C, R = 30, 32, 1
    blob = W.random_weights(F, C, R, seed=21, peaky=20.0)
    for dtype in ("f32", "bf16"):
        nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
        nn.load_weights(blob, 1)
        priors, value = nn.infer_legal(boards, offs, acts)
        policy, value2 = nn.encode_infer(boards)
        assert np.array_equal(value, value2)
        for i in range(len(sel)):
            a = acts[offs[i]:offs[i + 1]]
            if len(a) == 0:
                continue
            want = policy[i, a] / policy[i, a].sum(dtype=np.float32)
            np.testing.assert_allclose(priors[offs[i]:offs[i + 1]], want, rtol=2e-6, atol=1e-9)
            assert abs(priors[offs[i]:offs[i + 1]].sum() - 1.0) < 1e-5
        # planes entry point agrees with the compact one
        pr2, _ = nn.infer_legal(nn.encode(boards), offs, acts)
        assert np.array_equal(pr2, priors)
    # against the oracle end to end (f32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(blob, 1)
    priors, _ = nn.infer_legal(boards, offs, acts)
    op, _, _ = ko.forward(blob, F, C, R, ko.observe(boards))
    i = int(np.argmax(nact))
    a = acts[offs[i]:offs[i + 1]]
    np.testing.assert_allclose(priors[offs[i]:offs[i + 1]], op[i, a] / op[i, a].sum(), rtol=1e-3)


# ------------------------------------------------------------------------------ boundary behaviour
def test_nan_guard_and_errors():
    F, C, R = 30, 8, 0
    nn = NN(8, 8, F, 4672, filters=C, residuals=R)
    x = np.random.default_rng(0).random((2, 8, 8, F), dtype=np.float32)
    with pytest.raises(KamiError) as ei:
        nn.infer(x)
    assert ei.value.status == L.KH_ERR_NO_WEIGHTS
    blob = W.random_weights(F, C, R, seed=3)
    nn.load_weights(blob, 1)
    nn.infer(x)
    xb = x.copy()
    xb[1, 0, 0, 0] = np.nan
    with pytest.raises(KamiError) as ei:
        nn.infer(xb)
    assert ei.value.status == L.KH_ERR_NAN_POLICY
    assert str(ei.value) == "inference policy output contains NaN"       # nn.cpp:177
    # NaN only in the value head: poison valuefc.bias
    d = W.split(blob.copy(), F, C, R)
    d["valuefc.bias"][5] = np.nan
    nn.load_weights(np.concatenate([v.ravel() for v in d.values()]), 2)
    with pytest.raises(KamiError) as ei:
        nn.infer(x)
    assert ei.value.status == L.KH_ERR_NAN_VALUE
    assert str(ei.value) == "inference value output contains NaN"        # nn.cpp:180
    with pytest.raises(KamiError):
        nn.load_weights(blob[:-1], 1)


def test_generation_clone_and_hot_swap(tmp_path):
    F, C, R = 30, 8, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R)
    assert nn.get_generation() == 0
    b1 = W.random_weights(F, C, R, seed=1, peaky=10.0)
    b2 = W.random_weights(F, C, R, seed=2, peaky=10.0)
    x = np.random.default_rng(0).random((4, 8, 8, F), dtype=np.float32)
    nn.load_weights(b1, 5)
    assert nn.get_generation() == 5
    p1, v1 = nn.infer(x)
    twin = nn.clone()                      # NN(NN* other) nn.cpp:130-153
    nn.load_weights(b2, 6)
    p2, _ = nn.infer(x)
    pc, vc = twin.infer(x)
    assert twin.get_generation() == 5 and nn.get_generation() == 6
    assert np.array_equal(pc, p1) and np.array_equal(vc, v1) and not np.array_equal(p2, p1)
    # write -> read -> infer is bit-identical (test/nndisk.cpp:8-29)
    path = str(tmp_path / "m.bin")
    nn.write(path)
    other = NN(8, 8, F, 4672, filters=C, residuals=R)
    other.read(path)
    p3, _ = other.infer(x)
    assert other.get_generation() == 6 and np.array_equal(p3, p2)


def test_concurrent_infer_threads():
    """infer is called concurrently by inference threads on one model (nn.cpp:166)."""
    import threading
    F, C, R = 30, 16, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R)
    nn.load_weights(W.random_weights(F, C, R, seed=4, peaky=10.0), 1)
    xs = [np.random.default_rng(i).random((8 + i, 8, 8, F), dtype=np.float32) for i in range(6)]
    want = [nn.infer(x) for x in xs]
    got = [None] * len(xs)

    def work(i):
        for _ in range(5):
            got[i] = nn.infer(xs[i])

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(xs))]
    [t.start() for t in th]
    [t.join() for t in th]
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])


# ------------------------------------------------------------------------------ submit / wait, coalescing queue
def _legal_case(n, seed):
    rng = np.random.default_rng(seed)
    boards = random_boards(n, seed)
    nact = rng.integers(0, 40, n)
    offs = np.concatenate([[0], np.cumsum(nact)]).astype(np.int32)
    acts = rng.integers(0, 4672, int(offs[-1])).astype(np.int32)
    return boards, offs, acts


@pytest.mark.parametrize("dtype,C", [("bf16", 64), ("f32", 16), ("bf16", 96)])
def test_submit_wait_equals_the_synchronous_calls(dtype, C):
    """kh_submit_* / kh_wait: several small batches queued from one thread and evaluated merged give every caller the
    bits its own synchronous call gives (rows do not interact, nn.cpp:59-91) — for planes -> policy + the reference's
    flat value copy-out (nn.cpp:186, which depends on the CALLER's batch, not the merged one) and for records -> legal
    priors; on the whole-network kernel, the fp32 path and the per-layer path."""
    F, R = 30, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(W.random_weights(F, C, R, seed=3, peaky=10.0), 1)
    xs = [np.random.default_rng(i).random((b, 8, 8, F), dtype=np.float32) for i, b in enumerate((1, 16, 5, 128, 33))]
    want = [nn.infer(x) for x in xs]
    nn.set_coalesce(1024, 20000)                      # hold the launch until all five are queued: one merged launch
    tickets = [nn.submit_infer(x) for x in xs]
    nn.set_coalesce(0, 0)
    got = [t.wait() for t in tickets]
    for (p, v), (wp, wv) in zip(got, want):
        assert np.array_equal(p, wp) and np.array_equal(v, wv)
    launches, rows = nn.coalesce_stats()
    assert rows == sum(len(x) for x in xs) and launches <= 2
    cases = [_legal_case(n, 10 + n) for n in (7, 64, 1, 200)]
    want = [nn.infer_legal(*c) for c in cases]
    for mode in (L.KH_VALUE_REFERENCE_FLAT, L.KH_VALUE_PER_SAMPLE0):
        eng = nn if mode == L.KH_VALUE_REFERENCE_FLAT else NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype, value_mode=mode)
        if eng is not nn:
            eng.load_weights(nn.get_weights(), 1)
            want = [eng.infer_legal(*c) for c in cases]
        eng.set_coalesce(1024, 20000)
        tickets = [eng.submit_infer_legal(*c) for c in cases]
        eng.set_coalesce(0, 0)
        for t, (wp, wv) in zip(tickets, want):
            p, v = t.wait()
            assert np.array_equal(p, wp) and np.array_equal(v, wv)


def test_submit_never_blocks_on_the_callers_own_tickets():
    """Round 1's recorded hang (33 submits from one thread without a wait never returned: every call slot was leased
    to the caller itself, and the 33rd waited for one of them).  Here tickets are a fixed pool: KH_MAX_OUTSTANDING
    un-waited submissions are accepted, one more returns KH_ERR_INVALID at once, and after the waits the queue is
    usable again.  A ticket cannot be waited for twice."""
    F, C, R = 30, 32, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, C, R, seed=3, peaky=10.0), 1)
    x = np.random.default_rng(0).random((4, 8, 8, F), dtype=np.float32)
    want = nn.infer(x)
    tickets = [nn.submit_infer(x) for _ in range(L.KH_MAX_OUTSTANDING)]
    with pytest.raises(KamiError) as ei:
        nn.submit_infer(x)
    assert ei.value.status == L.KH_ERR_INVALID and "outstanding" in str(ei.value)
    for t in tickets:
        p, v = t.wait()
        assert np.array_equal(p, want[0]) and np.array_equal(v, want[1])
    with pytest.raises(KamiError):
        tickets[0].wait()
    p, v = nn.submit_infer(x).wait()
    assert np.array_equal(p, want[0])


def test_try_wait_takes_tickets_in_completion_order():
    """kh_try_wait: None while a submission is queued or on the device (the ticket stays valid), the synchronous call's
    bits once it has finished (the ticket is consumed: a second poll or a wait fails); a caller can hold several tickets
    and take whichever comes back first — what the pool's workers do."""
    import time
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=5, peaky=10.0), 1)
    cases = [_legal_case(20 + 7 * i, 300 + i) for i in range(6)]
    want = [nn.infer_legal(*c) for c in cases]
    # held back by a target nobody reaches: not done until the half-second limit has passed
    nn.set_coalesce(1024, 500000)
    t0 = time.perf_counter()
    held = nn.submit_infer_legal(*cases[0])
    assert held.try_wait() is None and time.perf_counter() - t0 < 0.3
    nn.set_coalesce(0, 0)
    p, v = held.wait()
    assert np.array_equal(p, want[0][0]) and np.array_equal(v, want[0][1])
    for _ in range(20):
        tickets = {i: nn.submit_infer_legal(*cases[i]) for i in range(6)}
        deadline = time.perf_counter() + 10.0
        while tickets and time.perf_counter() < deadline:
            for i in list(tickets):
                out = tickets[i].try_wait()
                if out is None:
                    continue
                assert np.array_equal(out[0], want[i][0]) and np.array_equal(out[1], want[i][1])
                with pytest.raises(KamiError):
                    tickets[i].try_wait()
                del tickets[i]
        assert not tickets


def test_a_launch_goes_when_every_caller_has_submitted():
    """kh_set_coalesce_callers: with a target the round would otherwise wait out (target 512, half a second), a batch
    that holds a submission of each of the 3 callers goes at once; with the rule off the same round waits for the
    quiet period."""
    import time
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, C, R, seed=3, peaky=10.0), 1)
    x = np.random.default_rng(0).random((8, 8, 8, F), dtype=np.float32)
    want = nn.infer(x)
    nn.submit_infer(x).wait()                                    # the queue's threads and buffers exist
    nn.set_coalesce(512, 480000)                                 # quiet period 60 ms

    def round_of_three():
        t0 = time.perf_counter()
        for t in [nn.submit_infer(x) for _ in range(3)]:
            p, v = t.wait()
            assert np.array_equal(p, want[0]) and np.array_equal(v, want[1])
        return time.perf_counter() - t0
    slow = round_of_three()
    nn.set_coalesce_callers(3)
    fast = min(round_of_three() for _ in range(3))
    nn.set_coalesce_callers(0)
    nn.set_coalesce(0, 0)
    assert slow > 0.05 and fast < 0.02, (slow, fast)
    with pytest.raises(KamiError):
        nn.set_coalesce_callers(L.KH_MAX_OUTSTANDING + 1)


def test_queue_attributes_nan_to_the_submission_that_holds_it():
    F, C, R = 30, 64, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, C, R, seed=3), 1)
    good = np.random.default_rng(0).random((6, 8, 8, F), dtype=np.float32)
    bad = good.copy(); bad[3, 1, 1, 2] = np.nan
    want = nn.infer(good)
    nn.set_coalesce(1024, 20000)
    t1, t2, t3 = nn.submit_infer(good), nn.submit_infer(bad), nn.submit_infer(good)
    nn.set_coalesce(0, 0)
    assert np.array_equal(t1.wait()[0], want[0])
    with pytest.raises(KamiError) as ei:
        t2.wait()
    assert ei.value.status == L.KH_ERR_NAN_POLICY and str(ei.value) == "inference policy output contains NaN"
    assert np.array_equal(t3.wait()[0], want[0])


def test_concurrent_small_callers_are_coalesced():
    """evaluate.cpp / selfplay.cpp from several threads at kami's default batch of 16, through this repository's search
    call (records + legal actions): the synchronous kh_encode_infer_legal calls that are inside the engine together
    are merged into common launches; every caller still gets its own rows' bits.  (kh_infer keeps private slots.)"""
    import threading
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=4, peaky=10.0), 1)
    cases = [_legal_case(64, 40 + i) for i in range(8)]
    want = [nn.infer_legal(*c) for c in cases]
    bad = []
    calls = 200

    def work(i):
        for _ in range(calls):
            p, v = nn.infer_legal(*cases[i])
            if not (np.array_equal(p, want[i][0]) and np.array_equal(v, want[i][1])):
                bad.append(i)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not bad
    launches, rows = nn.coalesce_stats()
    # calls that met another one inside the engine went through the queue (how many is up to thread timing: the
    # interpreter serialises the Python side of each call), and some launch held more than one caller's 64 positions
    assert rows >= 128 and rows % 64 == 0 and launches < rows // 64, (launches, rows)
    # the plane / full-policy call stays on private slots, concurrent callers included
    x = np.random.default_rng(1).random((16, 8, 8, F), dtype=np.float32)
    w0 = nn.infer(x)
    th = [threading.Thread(target=lambda: [nn.infer(x) for _ in range(10)]) for _ in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert nn.coalesce_stats() == (launches, rows) and np.array_equal(nn.infer(x)[0], w0[0])


def test_queue_under_buffer_pressure():
    """Twelve threads keep two 300-position submissions each in flight with a launch target of 1 024: merge buffers
    fill up (a submission that does not fit closes the batch) and submitters have to wait for one to come back from
    the device.  A ticket is reserved before that wait (a free ticket found by two threads at once was round 2's
    first bug in this queue: 'ticket already waited for'); every result equals the synchronous call's bits."""
    import threading
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=4, peaky=10.0), 1)
    cases = [_legal_case(300, 100 + i) for i in range(12)]
    want = [nn.infer_legal(*c) for c in cases]
    nn.set_coalesce(1024, 100)
    errors = []

    def work(i):
        try:
            for _ in range(30):
                t1 = nn.submit_infer_legal(*cases[i])
                t2 = nn.submit_infer_legal(*cases[i])
                for t in (t1, t2):
                    p, v = t.wait()
                    if not (np.array_equal(p, want[i][0]) and np.array_equal(v, want[i][1])):
                        errors.append((i, "bits"))
        except Exception as e:                      # noqa: BLE001
            errors.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(cases))]
    [t.start() for t in th]
    [t.join() for t in th]
    nn.set_coalesce(0, 0)
    assert not errors, errors[:3]
    launches, rows = nn.coalesce_stats()
    assert rows == 12 * 30 * 2 * 300 and rows / launches > 300


def test_weight_swap_while_threads_infer():
    """nn.cpp:166,206: read() replaces the weights while inference threads are inside infer().  Here the swap is atomic
    and never stalls a caller: six threads keep calling (directly and through the queue) while the main thread swaps
    between two parameter sets; every result must be exactly one set's output, never a mixture."""
    import threading
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    blobs = [W.random_weights(F, C, R, seed=s, peaky=10.0) for s in (1, 2)]
    xs = [np.random.default_rng(i).random((8 + 24 * (i % 2), 8, 8, F), dtype=np.float32) for i in range(6)]
    want = []
    for b in blobs:
        nn.load_weights(b, 1)
        want.append([nn.infer(x) for x in xs])
    stop = threading.Event()
    bad, seen = [], [set() for _ in xs]

    def work(i):
        while not stop.is_set():
            p, v = nn.infer(xs[i])
            k = [j for j in (0, 1) if np.array_equal(p, want[j][i][0]) and np.array_equal(v, want[j][i][1])]
            if not k:
                bad.append(i)
            else:
                seen[i].add(k[0])

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(xs))]
    [t.start() for t in th]
    for g in range(60):
        nn.load_weights(blobs[g & 1], g + 2)
    stop.set()
    [t.join() for t in th]
    assert not bad
    assert nn.get_generation() == 61 and all(len(s) == 2 for s in seen)      # every thread saw both generations


@pytest.mark.parametrize("sets", [2, 3])
def test_selfplay_pool_pipelined_through_the_queue(sets):
    """The pool with two halves (or three thirds) of every worker's trees in flight (kh_submit_encode_infer_legal /
    kh_wait) and the engine merging the workers' submissions: BASELINE configs[1]'s shape (256 games, two leaves per
    tree = 512 positions in flight), four workers; launches hold several workers' leaves."""
    from kami_amd import search as S
    F, C, R = 30, 64, 6
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=5, peaky=5.0), 1)
    pool = S.Pool(nn, games=256, threads=4, nodes=64, leaves_per_tree=2, seed=12, pipeline=sets, coalesce_target=512, coalesce_wait_us=300)
    st = pool.run(min_evals=200000, max_seconds=20.0)
    assert st.evals >= 200000 and st.moves > st.evals // 80
    launches, rows = nn.coalesce_stats()
    assert rows == st.evals and rows / launches > 128 / sets * 1.5, (launches, rows)     # one submission of a worker is 128 / sets leaves
    recs = pool.drain()
    assert st.records == len(recs) and st.games_finished == st.white_wins + st.black_wins + st.draws
    for r in recs[:100]:
        v = np.array(r.visits[:r.nact])
        assert 0 < r.nact <= S.MAX_RECORD_ACTIONS and abs(v.sum() - 1.0) < 1e-3


@pytest.mark.parametrize("mode", [L.KH_VALUE_REFERENCE_FLAT, L.KH_VALUE_PER_SAMPLE0])
def test_registered_caller_buffers_give_the_same_bits(mode):
    """kh_pin_buffer: kh_infer with registered input / policy buffers takes the chunked two-stream path (plain DMA out
    of the caller's pages, upload of one part under the kernel and download of the previous one).  Same bits as the
    pageable path at every batch size — odd ones, ones below the chunking thresholds, 300 (second row of the reference's
    flat value copy-out) — and the NaN contract holds; an unregistered pointer cannot be unpinned."""
    F, C, R = 119, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=mode)
    nn.load_weights(W.random_weights(F, C, R, seed=6, peaky=10.0), 1)
    xin = np.zeros((600, 8, 8, F), np.float32)
    pol = np.zeros((600, 4672), np.float32)
    nn.pin(xin); nn.pin(pol)
    try:
        rng = np.random.default_rng(3)
        for B in (1, 2, 63, 64, 255, 300, 512, 599):
            x = rng.random((B, 8, 8, F), dtype=np.float32)
            want_p, want_v = nn.infer(x)                                     # pageable buffers
            xin[:B] = x
            val = np.empty(B, np.float32)
            got_p, got_v = nn.infer(xin[:B], B, pol[:B], val)                # registered buffers
            assert got_p is not want_p and np.array_equal(got_p, want_p) and np.array_equal(got_v, want_v)
        xin[5, 3, 3, 7] = np.nan
        with pytest.raises(KamiError) as ei:
            nn.infer(xin[:64], 64, pol[:64], np.empty(64, np.float32))
        assert ei.value.status == L.KH_ERR_NAN_POLICY
        xin[5, 3, 3, 7] = 0.5
        nn.infer(xin[:64], 64, pol[:64], np.empty(64, np.float32))            # and the flags are clean again
    finally:
        nn.unpin(xin); nn.unpin(pol)
    with pytest.raises(KamiError):
        nn.unpin(xin)


def test_bench_two_ranks_control_flow(tmp_path):
    """bench.py under torch.distributed.run with 2 ranks (sharing this box's single GPU over gloo:
    RCCL refuses duplicate devices): barrier, max-over-ranks and the whole-job aggregate."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29100 + os.getpid() % 1000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "20", "--warmup", "3", "--no-cpu-baseline"]
    env = dict(os.environ, KAMI_DIST_BACKEND="gloo", OMP_NUM_THREADS="1")
    out = subprocess.run(cmd, check=True, timeout=600, env=env, capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1                         # rank 0 only
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 20
    assert d["value"] > 0 and abs(d["value"] - 2 * 512 * 20 / (d["ms_per_step"] * 20 * 1e-3)) / d["value"] < 0.02
    assert "cpu_baseline" not in d and d["roofline"]["bound"] == "mfma"


def _run_rccl_worker(tmp_path, nproc):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29300 + os.getpid() % 1000
    worker = os.path.join(root, "tests", "_rccl_worker.py")
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if nproc == 1:
        env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        cmd = [sys.executable, worker, str(tmp_path)]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), worker, str(tmp_path)]
    r = subprocess.run(cmd, timeout=600, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.load(open(tmp_path / f"rank{k}.json")) for k in range(nproc)]


def test_rccl_backend_single_rank_group(tmp_path):
    """The collectives of rows f3 / (e) through the PRODUCTION backend ("nccl" = RCCL) on this box's one GPU: a world of
    one rank is still an RCCL communicator, and it is where a host tensor handed to the backend fails.  The helpers
    place their tensors by the group's backend (kami_amd.dist.collective_device)."""
    from kami_amd import weights as W
    res = _run_rccl_worker(tmp_path, 1)[0]
    ref = W.random_weights(30, 8, 1, seed=77)
    assert res["backend"].lower() == "nccl" and res["world"] == 1
    assert abs(res["dt_max"] - 0.05) < 1e-12
    assert res["inserted"] == 0 and res["total"] == 3                     # nothing to merge from a peer, own records kept
    assert res["compact"] == [list(range(0, 8))]
    assert res["wgen"] == 41 and res["wn"] == ref.size and abs(res["wsum"] - float(ref.astype(np.float64).sum())) < 1e-9


def test_rccl_backend_two_ranks(tmp_path):
    """Same worker, one rank per GPU over RCCL / xGMI — runs where the box has >= 2 GPUs (the driver's 8-GPU node),
    skips on the one-GPU box: replay merge rank-major into the root, weight broadcast, max over ranks."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    from kami_amd import weights as W
    res = _run_rccl_worker(tmp_path, 2)
    ref = W.random_weights(30, 8, 1, seed=77)
    assert all(abs(r["dt_max"] - 0.10) < 1e-12 for r in res)
    assert res[0]["inserted"] == 4 and res[0]["total"] == 7 and res[1]["inserted"] == 0
    assert res[0]["compact"] == [list(range(0, 8)), list(range(10, 22))] and res[1]["compact"] == []
    assert all(r["wgen"] == 41 and abs(r["wsum"] - float(ref.astype(np.float64).sum())) < 1e-9 for r in res)


def _dropin_env(root):
    """Environment for the drop-in binaries under oracle/_ref/dropin: this tree's kami_amd first on the library path.
    Their rpath ($ORIGIN/../../../kami_amd) only holds while oracle/_ref sits inside this tree, and the binaries
    may be built elsewhere and brought in; LD_LIBRARY_PATH is searched before the rpath, so the library they load
    is always this checkout's."""
    import os
    env = dict(os.environ)
    lib = os.path.join(root, "kami_amd")
    env["LD_LIBRARY_PATH"] = lib + (os.pathsep + env["LD_LIBRARY_PATH"] if env.get("LD_LIBRARY_PATH") else "")
    return env


def test_reference_programs_on_the_cpp_mirror(tmp_path):
    """The reference's OWN test/nndisk.cpp, compiled unmodified against kami_amd/host/nn.h and
    libkamihip.so (make -C kami_amd/host dropin; binary under oracle/_ref/dropin, built in the build
    container only): infer -> write -> read -> infer must print no mismatch (test/nndisk.cpp:24-29)."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", "test_nndisk")
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    r = subprocess.run([exe], cwd=tmp_path, env=_dropin_env(root), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "mismatch" not in r.stderr and "mismatch" not in r.stdout
    assert "Saved model to" in r.stdout


def test_reference_nntrain_program_on_the_cpp_mirror(tmp_path):
    """The reference's OWN test/nntrain.cpp (512 random trajectories through NN::train with the default
    256-filter net, 8 epochs), compiled unmodified against the C++ mirror: runs to completion on the
    device and reports a finite, decreasing loss."""
    import os, re, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", "test_nntrain")
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    r = subprocess.run([exe], cwd=tmp_path, env=_dropin_env(root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    m = re.search(r"Generated model 1, average loss ([-0-9.e+]+) to ([-0-9.e+]+) over 8 epochs", r.stdout)
    assert m, r.stdout
    first, last = float(m.group(1)), float(m.group(2))
    assert np.isfinite([first, last]).all() and last < first
    assert "Finished in" in r.stdout


@pytest.mark.parametrize("program", ["kami", "kami_native"])
def test_reference_kami_program_full_cycle_on_the_cpp_mirror(tmp_path, program):
    """`kami`: the reference's OWN program (kami.cpp + selfplay.cpp + evaluate.cpp + mcts.h + env.h +
    neocortex, compiled unmodified against the C++ NN mirror, no libtorch): self-play on its inference
    threads through kh_infer, a trainer thread that clones the model, trains the clone (kh_train), gates
    it against the current model (evaluate.cpp) and swaps it in through write() / read() — one full
    generation on the device.
    `kami_native`: the same unmodified kami.cpp + options.cpp on THIS repository's whole host side
    (kami_amd/host: selfplay, evaluate, mcts, env, chess rules, replay buffer, NN; no neocortex / thc):
    the drop-in the north star describes — env.h / evaluate.h / selfplay.h surface kept, the search and the
    worker pool ours, leaves sent as compact records through kh_encode_infer_legal."""
    import os, subprocess, time, threading
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", program)
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    opts = dict(filters=16, residuals=1, selfplay_batch=16, selfplay_nodes=16, inference_threads=2, training_threads=1,
                replaybuffer_size=128, rpb_train_pct=40, training_sample_pct=60, training_epochs=2, training_batchsize=8,
                training_mlr=5, evaluate_batch=8, evaluate_games=8, evaluate_nodes=8, evaluate_target_pct=0,
                model_path=str(tmp_path / "model.bin"), engine_dtype="bf16")
    (tmp_path / "options.yml").write_text("".join(f"{k}: {v}\n" for k, v in opts.items()))
    proc = subprocess.Popen([exe], cwd=tmp_path, env=_dropin_env(root), stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    t = threading.Thread(target=lambda: lines.extend(iter(proc.stdout.readline, "")), daemon=True)
    t.start()
    deadline = time.time() + 150
    done = False
    while time.time() < deadline and not done and proc.poll() is None:
        time.sleep(1.0)
        done = any("candidate accepted" in l or "candidate rejected" in l for l in lines)
    try:
        proc.stdin.write("status\n" + ("pgn\n" if program == "kami_native" else "") + "quit\n"); proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    out = "".join(lines)
    assert done, out[-3000:]
    assert "training generation 0" in out and "Generated model 1" in out, out[-3000:]
    assert "evaluating model generation 1" in out
    if "candidate accepted" in out:
        assert "using new generation 1" in out and os.path.exists(tmp_path / "model.bin")
    # the only complaint allowed is the start-up warning about the not-yet-existing model file (kami.cpp:46-49)
    complaints = [l for l in out.splitlines() if "ERROR" in l or "failed" in l]
    assert all("model read from" in l for l in complaints), complaints
    assert "Total experiences:" in out
    if program == "kami_native":
        assert "[White \"KAMI generation" in out and (" 1-0 {" in out or " 0-1 {" in out or " 1/2-1/2 {" in out)


def test_kami_native_two_evaluators_in_one_process(tmp_path):
    """One process, TWO engines (option engine_devices = 2; on a one-GPU box both land on device 0, on a node one per
    GPU): inference thread i feeds engine i % 2, finished games of both go into the one replay ring, an accepted candidate
    is published to both engines (selfplay.cpp:21-35,96-109,176-184,282-283).  The unmodified kami.cpp plays, trains,
    gates and swaps a generation on it."""
    import os, subprocess, time, threading
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", "kami_native")
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    opts = dict(filters=16, residuals=1, selfplay_batch=16, selfplay_nodes=16, inference_threads=4, training_threads=1,
                replaybuffer_size=128, rpb_train_pct=40, training_sample_pct=60, training_epochs=2, training_batchsize=8,
                training_mlr=5, evaluate_batch=8, evaluate_games=8, evaluate_nodes=8, evaluate_target_pct=0,
                model_path=str(tmp_path / "model.bin"), engine_dtype="bf16", engine_devices=2)
    (tmp_path / "options.yml").write_text("".join(f"{k}: {v}\n" for k, v in opts.items()))
    proc = subprocess.Popen([exe], cwd=tmp_path, env=_dropin_env(root), stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    t = threading.Thread(target=lambda: lines.extend(iter(proc.stdout.readline, "")), daemon=True)
    t.start()
    deadline = time.time() + 150
    while time.time() < deadline and proc.poll() is None and not any("candidate accepted" in l for l in lines):
        time.sleep(1.0)
    time.sleep(3.0)                       # a few rounds on the new generation
    try:
        proc.stdin.write("status\nquit\n"); proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    out = "".join(lines)
    assert "Selfplay: 2 evaluators" in out, out[-3000:]
    assert "kami::NN: MI355X engine" in out            # the mirror says which arithmetic it computes in
    assert "candidate accepted: using new generation 1" in out, out[-3000:]
    assert "INFER" not in out, out[-3000:]            # no inference thread died
    # (the threads' own lines interleave on stdout: counted, not matched one by one)
    assert out.count("Starting inference thread:") == 4 and out.count("Terminating inference thread:") == 4


def test_pool_with_two_engines_and_weight_publish():
    """ks_pool_create_multi: one pool, two engines (both on device 0 here), workers sharded over them, ONE record ring;
    ks_pool_publish_weights puts a new generation on both; pipelined and blocking schedules."""
    from kami_amd import search as S
    F, C, R = 30, 64, 2
    blob0, blob1 = W.random_weights(F, C, R, seed=1, peaky=5.0), W.random_weights(F, C, R, seed=2, peaky=5.0)
    engines = [NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0) for _ in range(2)]
    for e in engines:
        e.load_weights(blob0, 3)
    for pipeline in (0, 1):
        pool = S.Pool(engines, games=96, threads=4, nodes=24, leaves_per_tree=2, seed=5, pipeline=pipeline, coalesce_target=48, coalesce_wait_us=100)
        st = pool.run(min_evals=4000, max_seconds=20.0)
        assert st.evals >= 4000 and st.moves > 0
        pool.publish_weights(blob1, 4)
        assert [e.get_generation() for e in engines] == [4, 4]
        st2 = pool.run(min_evals=2000, max_seconds=20.0)
        assert st2.evals >= st.evals + 2000
        recs = pool.drain()
        assert st2.games_finished == 0 or len(recs) > 0
        pool.close()
        for e in engines:
            e.load_weights(blob0, 3)
    # both engines really evaluated: each one's queue / call counters moved (the pipelined run goes through the queues)
    assert all(e.coalesce_stats()[0] > 0 for e in engines)
    with pytest.raises(RuntimeError, match="every engine needs a worker"):
        S.Pool(engines, games=8, threads=1, nodes=8)
    for e in engines:
        e.close()


@pytest.mark.parametrize("program", ["kami", "kami_native"])
def test_configs0_literal_one_game_64_sims(tmp_path, program):
    """BASELINE configs[0] literally — 1 self-play game, 64 MCTS sims per move (test/selfplay.cpp's path: one inference
    thread, selfplay_batch 1, selfplay_nodes 64, the 2x64 default net of options.def.yml) — with the engine as the
    evaluator: the reference's own program on the C++ mirror (`kami`), and the same kami.cpp on this repository's
    host side (`kami_native`).  It plays whole games of batch-1 evaluations and fills its replay buffer; the model
    it boots from (`model_path`, kami.cpp:39-51) is a checkpoint in the REFERENCE's format (tests/golden, written by the
    reference's NN::write), so the literal shape also exercises NN::read on a torch archive."""
    import os, re, shutil, subprocess, time, threading
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", program)
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    shutil.copy(os.path.join(root, "tests", "golden", "ref_checkpoint_f30_c8_r1.pt"), tmp_path / "ref.pt")
    opts = dict(filters=8, residuals=1, selfplay_batch=1, selfplay_nodes=64, inference_threads=1, training_threads=0,
                replaybuffer_size=4096, model_path=str(tmp_path / "ref.pt"), engine_dtype="bf16")
    (tmp_path / "options.yml").write_text("".join(f"{k}: {v}\n" for k, v in opts.items()))
    proc = subprocess.Popen([exe], cwd=tmp_path, env=_dropin_env(root), stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    t = threading.Thread(target=lambda: lines.extend(iter(proc.stdout.readline, "")), daemon=True)
    t.start()
    try:
        time.sleep(12.0)
        proc.stdin.write("status\nquit\n"); proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    out = "".join(lines)
    assert "Current generation: 7" in out, out[-2000:]          # the archive's generation IValue (nn.cpp:196)
    m = re.search(r"Total experiences: (\d+)", out)
    assert m and int(m.group(1)) >= 20, out[-2000:]             # finished games reached the replay buffer
    assert "Error in command" not in out, out[-2000:]


# ------------------------------------------------------------------------------ full-size properties
def test_full_size_properties_headline_config():
    """BASELINE configs[1] at its full size (512 x 119x8x8, 6x64), where the oracle is too slow to
    be the checker for every row: size-independent properties instead."""
    F, C, R, B = 119, 64, 6, 512
    blob = W.random_weights(F, C, R, seed=20240607, peaky=20.0)
    x = np.random.default_rng(1).random((B, 8, 8, F), dtype=np.float32)
    out = {}
    for dtype in ("bf16", "f16", "f32"):
        nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
        nn.load_weights(blob, 1)
        p, vf, _ = nn.infer_full(x, want_logits=False)
        out[dtype] = (p, vf)
        assert np.isfinite(p).all() and (p >= 0).all()
        np.testing.assert_allclose(p.sum(1, dtype=np.float64), 1.0, atol=2e-5)       # softmax rows
        assert np.abs(vf).max() <= 1.0                                               # tanh range
        # batching invariance: the two halves evaluated separately give the same bits
        p2, vf2, _ = nn.infer_full(x[256:], want_logits=False)
        assert np.array_equal(p2, p[256:]) and np.array_equal(vf2, vf[256:])
        # permutation equivariance: rows follow their inputs
        perm = np.random.default_rng(2).permutation(B)
        p3, vf3, _ = nn.infer_full(x[perm], want_logits=False)
        assert np.array_equal(p3, p[perm]) and np.array_equal(vf3, vf[perm])
    # cross-precision agreement within the stated tolerances (f32 = exact MFMA path as the anchor)
    for dtype in ("bf16", "f16"):
        compare("full/configs1_6x64_B512_vs_f32mfma", dtype, (out[dtype][0], out[dtype][1], None), (out["f32"][0], out["f32"][1], None))
    # and a sample of rows against the oracle
    rows = [0, 1, 255, 256, 511]
    op, ovf, _ = ko.forward(blob, F, C, R, x[rows])
    for dtype in ("f32", "bf16", "f16"):
        compare("full/configs1_6x64_B512_rows_vs_oracle", dtype, (out[dtype][0][rows], out[dtype][1][rows], None), (op, ovf, None))


FULL_DEPTH = [
    # BASELINE configs[2]: 10 blocks x 128 filters, batch 1024, bf16
    ("configs2_10x128_B1024", "bf16", 119, 128, 10, 1024),
    # BASELINE configs[4]: 20 blocks x 256 filters, fp16, batch 2048 (and the batch 256 the bench variant times)
    ("configs4_20x256_B256", "f16", 119, 256, 20, 256),
    ("configs4_20x256_B2048", "f16", 119, 256, 20, 2048),
    # the other precision of each, at a batch the per-layer kernels' variants all see
    ("configs2_10x128_B1024", "f16", 119, 128, 10, 1024),
    ("configs4_20x256_B256", "bf16", 119, 256, 20, 256),
]


@pytest.mark.parametrize("name,dtype,F,C,R,B", FULL_DEPTH, ids=[f"{n}-{d}" for n, d, *_ in FULL_DEPTH])
def test_full_size_properties_wide_configs(name, dtype, F, C, R, B):
    """BASELINE configs[2] and configs[4] at their FULL depth and batch (nn.cpp:26-34,59-91): low-precision error
    grows with depth, so the wide nets are pinned where it is largest.  Size-independent properties on the whole
    batch; rows 0 / 1 / middle / last against the CPU oracle (4 evaluations of a 0.4 / 3.1 GFLOP net: cheap);
    cross-check of the same rows against the engine's exact-fp32 path."""
    blob = W.random_weights(F, C, R, seed=1000 + C + R, peaky=20.0)
    x = np.random.default_rng(B + C).random((B, 8, 8, F), dtype=np.float32)
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype)
    nn.load_weights(blob, 1)
    p, vf, lg = nn.infer_full(x)
    assert np.isfinite(p).all() and (p >= 0).all() and np.isfinite(lg).all()
    np.testing.assert_allclose(p.sum(1, dtype=np.float64), 1.0, atol=2e-5)           # softmax rows
    assert np.abs(vf).max() <= 1.0                                                   # tanh range
    # batching invariance: the second half evaluated alone gives the same bits (another workgroup schedule)
    h = B // 2
    p2, vf2, lg2 = nn.infer_full(x[h:])
    assert np.array_equal(p2, p[h:]) and np.array_equal(vf2, vf[h:]) and np.array_equal(lg2, lg[h:])
    # permutation equivariance: rows follow their inputs
    perm = np.random.default_rng(2).permutation(B)
    p3, vf3, _ = nn.infer_full(x[perm], want_logits=False)
    assert np.array_equal(p3, p[perm]) and np.array_equal(vf3, vf[perm])
    # rows against the oracle (fp32 CPU restatement of the reference, pinned by the reference's fixtures)
    rows = [0, 1, B // 2 - 1, B // 2, B - 1]
    want = ko.forward(blob, F, C, R, x[rows])
    compare(f"full/{name}_rows_vs_oracle", dtype, (p[rows], vf[rows], lg[rows]), want, tol_for(dtype, R))
    # and the engine's exact-fp32 arithmetic on 64 rows (fp32 MFMA path up to 128 filters, fp32 VALU kernels beyond)
    sub = np.unique(np.concatenate([rows, np.linspace(0, B - 1, 60).astype(int)]))
    nf = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nf.load_weights(blob, 1)
    fp, fvf, flg = nf.infer_full(x[sub])
    at = np.searchsorted(sub, rows)
    compare(f"full/{name}_rows_vs_oracle", "f32", (fp[at], fvf[at], flg[at]), want, tol_for("f32", R))
    compare(f"full/{name}_64rows_vs_f32", dtype, (p[sub], vf[sub], lg[sub]), (fp, fvf, flg), tol_for(dtype, R))


def test_selfplay_pool_literal_configs1_shape():
    """BASELINE configs[1] literally: 256 parallel games, 800 visits per move, batch-512 evaluations (two leaves of
    every tree in flight), 6-block x 64-filter net.  A few seconds of play: the pool runs at that shape, its batches
    ARE 512 wide, moves need 800 visits, records come out well-formed."""
    from kami_amd import search as S
    F, C, R = 30, 64, 6
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=5, peaky=5.0), 1)
    pool = S.Pool(nn, games=256, threads=1, nodes=800, leaves_per_tree=2, seed=11)
    st = pool.run(min_evals=600000, max_seconds=8.0)
    assert st.evals >= 256 * 800, st.evals                      # every game got past its first move's budget
    assert st.mean_batch >= 480, st.mean_batch                  # batch-512 evaluations (terminal leaves cost nothing)
    assert st.moves >= 256 and st.moves <= st.evals // 700 + 256 * 2
    for r in pool.drain()[:100]:
        v = np.array(r.visits[:r.nact])
        assert 0 < r.nact <= S.MAX_RECORD_ACTIONS and abs(v.sum() - 1.0) < 1e-3


def test_reference_checkpoint_ingest(tmp_path):
    """A checkpoint written by the reference's own NN::write (tests/golden/ref_checkpoint_f30_c8_r1.pt, generated from
    the blob of the net_f30_c8_r1 fixture): NN::read takes it (kh_load_checkpoint: zip + pickle walk, no libtorch), the
    generation follows, and the forward pass equals the reference's own outputs for that network."""
    import os
    from conftest import GOLDEN, load_net_fixture
    d = load_net_fixture(os.path.join(GOLDEN, "net_f30_c8_r1.npz"))
    ck = os.path.join(GOLDEN, "ref_checkpoint_f30_c8_r1.pt")
    for dtype in ("f32", "bf16"):
        nn = NN(8, 8, 30, 4672, filters=8, residuals=1, dtype=dtype)
        nn.read(ck)
        assert nn.get_generation() == 7
        check_forward(nn, d, dtype)
    # the C entry point in one call, and its shape check
    nn = NN(8, 8, 30, 4672, filters=8, residuals=1)
    assert nn._lib.kh_load_checkpoint(nn.handle, ck.encode()) == L.KH_OK and nn.get_generation() == 7
    p1, v1 = nn.infer(d["x"])
    np.testing.assert_allclose(v1, d["value"], atol=TOL["f32"]["value"], rtol=0)
    other = NN(8, 8, 30, 4672, filters=16, residuals=1)
    assert other._lib.kh_load_checkpoint(other.handle, ck.encode()) == L.KH_ERR_INVALID
    # write() -> read() of the engine's own container still round-trips after an archive ingest
    path = str(tmp_path / "m.bin")
    nn.write(path)
    twin = NN(8, 8, 30, 4672, filters=8, residuals=1)
    twin.read(path)
    p2, v2 = twin.infer(d["x"])
    assert twin.get_generation() == 7 and np.array_equal(p1, p2) and np.array_equal(v1, v2)


def test_encode_full_size_properties():
    """2^20 positions: structural invariants of Env::observe's output (env.h:202-262)."""
    n = 1 << 20
    boards = random_boards(n, seed=5)
    nn = NN(filters=8, residuals=0)
    planes = nn.encode(boards).reshape(n, 64, 30)
    assert np.array_equal(planes[:, :, :18], np.broadcast_to(planes[:, :1, :18], (n, 64, 18)))   # header broadcast (Q5)
    occ = (boards["color_occ"][:, 0] | boards["color_occ"][:, 1])
    typed = np.zeros(n, np.uint64)
    for t in range(6):
        typed |= boards["piece_occ"][:, t]
    npieces = np.array([bin(int(v)).count("1") for v in (occ & typed)[:4096]])
    assert np.array_equal(planes[:4096, :, 18:].sum((1, 2)).astype(int), npieces)               # one plane bit per piece
    assert set(np.unique(planes[:, 0, 14:18])) <= {0.0, 1.0, 2.0, 4.0, 8.0}                     # raw castle bits (Q2)
    assert np.array_equal(planes[:, 0, 0], (boards["ply"] & 1).astype(np.float32))


# ---------------------------------------------------------------------------------------------
# host search row: the self-play pool drives the engine with compact records

@pytest.mark.gpu
@pytest.mark.parametrize("leaves", [1, 4])
def test_selfplay_pool_feeds_engine(leaves):
    from kami_amd import search as S
    F, C, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, C, R, seed=5, peaky=5.0), 1)
    pool = S.Pool(nn, games=96, threads=3, nodes=24, leaves_per_tree=leaves, seed=3)
    st = pool.run(min_evals=40000, max_seconds=60.0)
    assert st.evals >= 40000 and st.batches > 0
    assert st.mean_batch >= 32                         # a worker's batch is (at least) one leaf of each of its 32 trees
    assert st.moves > st.evals // 30                   # >= one move per `nodes` visits (terminal visits are free)
    recs = pool.drain()
    assert st.records == len(recs)
    assert st.games_finished == st.white_wins + st.black_wins + st.draws
    for r in recs[:200]:
        v = np.array(r.visits[:r.nact])
        assert 0 < r.nact <= S.MAX_RECORD_ACTIONS and abs(v.sum() - 1.0) < 1e-3 and (v >= 0).all()
        assert r.value in (-1.0, 0.0, 1.0)
    # the records' boards encode like any other record (device encoder)
    b = np.frombuffer(b"".join(bytes(r.board) for r in recs[:64]), dtype=L.BOARD_DTYPE)
    planes = nn.encode(b)
    assert planes.shape == (len(b), 8, 8, 30) and np.isin(planes, [0, 1, 2, 4, 8]).all()


@pytest.mark.gpu
def test_pool_survives_a_failed_engine_call():
    """An engine without weights fails the pool's first batch; the virtual visits of that batch are taken
    back, so that the same pool plays normally once weights are loaded."""
    from kami_amd import search as S
    F, C, R = 30, 32, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    pool = S.Pool(nn, games=16, threads=2, nodes=16, leaves_per_tree=2, seed=4)
    with pytest.raises(RuntimeError, match="kh_load_weights"):
        pool.run(min_evals=100, max_seconds=10.0)
    nn.load_weights(W.random_weights(F, C, R, seed=6, peaky=5.0), 1)
    st = pool.run(min_evals=2000, max_seconds=30.0)
    assert st.evals >= 2000 and st.moves > 0


@pytest.mark.gpu
def test_pool_priors_are_the_reference_expansion():
    """One position: the priors the pool's evaluator call returns (kh_encode_infer_legal on Env::record +
    Env::actions) equal policy[a] / sum over legal a of the full policy row (mcts.h:273-276)."""
    from kami_amd import search as S
    F, C, R = 30, 32, 1
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(W.random_weights(F, C, R, seed=9, peaky=10.0), 1)
    env = S.Env()
    for a in (877, 657, 949):              # a few plies into a game (actions from the mcts fixture)
        env.push(a)
    rec = env.record()
    acts = np.array(env.actions(), np.int32)
    pri, val = nn.infer_legal(rec, np.array([0, len(acts)], np.int32), acts)
    p, v = nn.encode_infer(rec)
    want = p[0, acts] / p[0, acts].sum()
    np.testing.assert_allclose(pri, want, rtol=1e-5)
    assert abs(pri.sum() - 1.0) < 1e-5


def test_split_channel_tower_two_engines_at_once():
    """tower2s_kernel's workgroups wait for their partners inside the launch (two workgroups per board pair exchange half an
    image per layer).  Two engines launching it at the same time on their own streams — 2 x 256 workgroups for 256 CUs —
    must both finish (partners are neighbours in each XCD's dispatch order, so whatever is resident can always complete)
    and give the bits of a launch that had the chip to itself; a partner that never showed up would raise the NaN flag
    after a second instead of hanging the device."""
    import threading
    F, C, R, B = 119, 256, 3, 256
    blob = W.random_weights(F, C, R, seed=9, peaky=10.0)
    x = np.random.default_rng(3).random((B, 8, 8, F), dtype=np.float32)
    nns = [NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f16") for _ in range(2)]
    for nn in nns:
        nn.load_weights(blob, 1)
    want = nns[0].infer_full(x)
    errors = []

    def work(nn):
        try:
            for _ in range(40):
                got = nn.infer_full(x)
                if not all(np.array_equal(a, b) for a, b in zip(got, want)):
                    errors.append("bits")
        except Exception as e:                      # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(nn,)) for nn in nns]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors[:3]
