"""The held-out loss of the network as served (kh_eval_records, kh_eval_replay; NN.eval_records, NN.eval_replay).

The oracle is float64 NumPy over the outputs of kh_encode_infer_device — an entry point this work leaves alone — on the
same boards in the same chunks of KH_EVAL_CHUNK, so the forward's bits are identical by construction and what differs is
the double log (<= 1 ulp on either side), at most 96 + 256 double additions per record, and n for the totals: of order
400 * 2^-52 relative.  Asserted: |d| <= 1e-12 * max(1, |x|), four orders above that bound and five below what a single
fp32 step in the kernel would cause (1e-7).  Everything else here is bit for bit or exact."""
import ctypes as C
import os

import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from kami_amd.replay import DeviceReplay
from oracle import pyoracle as ko

from _records_util import GOLD, fixture_records, full_record
from test_gpu_device_api import DevBuf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")       # (before the first engine: torch finds no GPU when it is imported after one exists)

CHUNK = L.EVAL_CHUNK
TOL = 1e-12
_CACHE = {}
ENGINES = {"f32-16x1": ("f32", 16, 1, 2), "bf16-64x2": ("bf16", 64, 2, 5), "bf16-128x1": ("bf16", 128, 1, 6)}   # dtype, C, R, seed


def fixture():
    if "fix" not in _CACHE:
        z = np.load(os.path.join(GOLD, "observe_playouts.npz"), allow_pickle=False)
        boards = ko.boards_from_fens([s.decode() for s in z["fen"]], z["ply"])
        _CACHE["fix"] = fixture_records(seed=23, boards=boards)
    return _CACHE["fix"]


def records(n):
    """n - 3 fixture records and three hand-made ones behind them — no moves, the all-zero record, a 96-move record whose
    two largest visit shares tie — with a 96-move record and a record without moves put in front of the last chunk
    boundary as well (n - 5, n - 4: for n = CHUNK + 3 those are the last two rows of the first chunk)."""
    if n not in _CACHE:
        fix = fixture()
        rec = np.zeros(n, L.RECORD_DTYPE)
        rec[:n - 3] = fix[:n - 3]
        rec[n - 5] = full_record(seed=4)[0]
        rec[n - 5]["board"] = fix[700]["board"]
        rec[n - 4] = fix[40]
        rec[n - 4]["nact"] = 0
        rec[n - 3] = fix[41]                                        # behind the boundary: no moves, ...
        rec[n - 3]["nact"] = 0
        rec[n - 3]["value"] = -1.0
        # rec[n - 2]: ... the all-zero record, ...
        tie = full_record(seed=5)[0]                                # ... and 96 moves with a tie for the most visited
        tie["board"] = fix[800]["board"]
        tie["visits"][17] = tie["visits"][60] = tie["visits"].max() * np.float32(1.5)
        rec[n - 1] = tie
        _CACHE[n] = rec
    return _CACHE[n]


def test_the_records_are_what_the_tests_assume():
    for n in (73, CHUNK + 3):
        rec = records(n)
        assert [int(rec["nact"][i]) for i in (n - 5, n - 4, n - 3, n - 2, n - 1)] == [96, 0, 0, 0, 96]
        assert rec[n - 2].tobytes() == bytes(L.RECORD_DTYPE.itemsize)
        if n > CHUNK:
            assert n - 4 == CHUNK - 1 and n - 3 == CHUNK                # both kinds on both sides of the chunk boundary
        for i in range(n - 1):                                          # visit shares without ties, but for the last record
            k = int(rec["nact"][i])
            if k:
                v = rec["visits"][i, :k]
                assert np.count_nonzero(v == v.max()) == 1
        v = rec["visits"][n - 1]
        assert np.count_nonzero(v == v.max()) == 2 and int(np.argmax(v)) == 17


def engine(key, gen=3):
    dtype, C_, R, seed = ENGINES[key]
    nn = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype=dtype)
    nn.load_weights(W.random_weights(30, C_, R, seed=seed, peaky=10.0), gen)
    return nn


def served_outputs(nn, rec):
    """policy [n, 4672], value [n, 256] of kh_encode_infer_device on the records' boards, in chunks of KH_EVAL_CHUNK"""
    n = rec.size
    boards = np.ascontiguousarray(rec["board"])
    d_b = DevBuf(nn, boards.nbytes).put(boards)
    d_p, d_v = DevBuf(nn, min(n, CHUNK) * 4672 * 4), DevBuf(nn, min(n, CHUNK) * 256 * 4)
    pol, val = np.empty((n, 4672), np.float32), np.empty((n, 256), np.float32)
    for i0 in range(0, n, CHUNK):
        m = min(CHUNK, n - i0)
        assert nn._lib.kh_encode_infer_device(nn.handle, C.c_void_p(d_b.p.value + i0 * 80), m, d_p.p, d_v.p, None) == 0, L.last_error()
        assert nn._lib.kh_sync(nn.handle) == 0
        pol[i0:i0 + m], val[i0:i0 + m] = d_p.get((m, 4672)), d_v.get((m, 256))
    for b in (d_b, d_p, d_v):
        b.free()
    return pol, val


def oracle(rec, pol, val):
    n = rec.size
    lp, lv, agree = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    for i in range(n):
        k = int(rec["nact"][i])
        if k:
            p = pol[i, rec["actions"][i, :k].astype(np.int64)]
            lp[i] = -np.sum(rec["visits"][i, :k].astype(np.float64) * np.log(p.astype(np.float64) + 0.001))
            agree[i] = int(np.argmax(rec["visits"][i, :k]) == np.argmax(p))      # argmax: the first maximum
        d = val[i].astype(np.float64) - np.float64(rec["value"][i])
        lv[i] = np.sum(d * d) / 256
    with_moves = int(np.count_nonzero(rec["nact"]))
    return dict(lp=lp, lv=lv, policy_records=with_moves, policy_loss=lp.sum() / n, value_loss=lv.sum() / n,
                top1=agree.sum() / with_moves, agree=agree)


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want))))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_totals(a, b):
    return all(bits(getattr(a, f)).tolist() == bits(getattr(b, f)).tolist() for f in ("policy_loss", "value_loss", "top1")) and \
        all(getattr(a, f) == getattr(b, f) for f in ("records", "policy_records", "generation"))


def same_result(a, b):
    """every field and both per-record arrays, bit for bit"""
    return same_totals(a, b) and np.array_equal(bits(a.record_policy_loss), bits(b.record_policy_loss)) and \
        np.array_equal(bits(a.record_value_loss), bits(b.record_value_loss))


@pytest.mark.parametrize("key,n", [("f32-16x1", 73), ("bf16-64x2", 73), ("bf16-128x1", 73), ("f32-16x1", CHUNK + 3)])
def test_against_float64_numpy(key, n):
    rec = records(n)
    nn = engine(key)
    want = oracle(rec, *served_outputs(nn, rec))
    res = nn.eval_records(rec, per_record=True)
    worst = max(np.max(np.abs(res.record_policy_loss - want["lp"]) / np.maximum(1, np.abs(want["lp"]))),
                np.max(np.abs(res.record_value_loss - want["lv"]) / np.maximum(1, np.abs(want["lv"]))))
    print(f"{key} n={n}: worst per-record deviation {worst:.3e}; policy_loss {res.policy_loss!r} / {want['policy_loss']!r}, "
          f"value_loss {res.value_loss!r} / {want['value_loss']!r}, top1 {res.top1!r} / {want['top1']!r}")
    assert res.records == n and res.generation == 3
    assert res.policy_records == want["policy_records"] == n - 3      # exact
    assert res.top1 == want["top1"]                                   # exact: the same two integers divided
    assert np.all(res.record_policy_loss[rec["nact"] == 0] == 0.0)
    assert close(res.record_policy_loss, want["lp"]) and close(res.record_value_loss, want["lv"])
    assert close(res.policy_loss, want["policy_loss"]) and close(res.value_loss, want["value_loss"])
    without = nn.eval_records(rec)                                     # per_record=False: the same totals, no arrays
    assert without.record_policy_loss is None and without.record_value_loss is None and same_totals(without, res)
    # The tie pins "the first maximum wins": entries 17 and 60 share the most visits.  With the network's favourite move
    # in entry 17 the record agrees; with it in entry 60 it does not (a last-wins rule would say it does).
    tie = rec[n - 1:n]
    p = served_outputs(nn, tie)[0][0, tie["actions"][0].astype(np.int64)]
    best = int(np.argmax(p))
    assert np.count_nonzero(p == p.max()) == 1
    for entry, top1 in ((17, 1.0), (60, 0.0)):
        t = tie.copy()
        a = t["actions"][0].copy()
        a[[entry, best]] = a[[best, entry]]
        t["actions"][0] = a
        assert nn.eval_records(t).top1 == top1
    nn.close()


def test_slices_and_repeats_are_bit_identical():
    n = 73
    rec = records(n)
    nn = engine("f32-16x1")
    whole = nn.eval_records(rec, per_record=True)
    again = nn.eval_records(rec, per_record=True)
    assert same_result(whole, again)
    part = nn.eval_records(rec[5:n], per_record=True)
    assert part.records == n - 5
    assert np.array_equal(bits(part.record_policy_loss), bits(whole.record_policy_loss[5:]))
    assert np.array_equal(bits(part.record_value_loss), bits(whole.record_value_loss[5:]))
    nn.close()


@pytest.mark.parametrize("first,n", [(30, 20), (0, 37)])
def test_ring_equals_records(first, n):
    src = records(73)[73 - 50:]                                        # the hand-made ones among them
    nn = engine("f32-16x1")
    ring, twin = DeviceReplay(nn, 37, seed=9), DeviceReplay(nn, 37, seed=9)
    for r in (ring, twin):
        assert r.add(src[:20]) == 20 and r.add(src[20:]) == 30
    count = ring.count()
    got = nn.eval_replay(ring, first, n, per_record=True)
    want = nn.eval_records(ring.read(first, n), per_record=True)
    assert got.records == n and same_result(got, want)
    assert ring.count() == count == 50
    assert ring.select(8).tobytes() == twin.select(8).tobytes()         # no draw was made, nothing was moved
    if first == 0:
        assert same_result(nn.eval_replay(ring, per_record=True), want)  # n=None: the written slots
    empty = DeviceReplay(nn, 8)
    with pytest.raises(ValueError):
        nn.eval_replay(empty)
    for r in (ring, twin, empty):
        r.close()
    nn.close()


def test_no_side_effects_and_the_right_parameter_set():
    from test_gpu_train_records import same, state
    rec = records(73)
    nn = engine("f32-16x1", gen=3)
    blob = nn.get_weights().copy()
    before = state(nn)
    first = nn.eval_records(rec, per_record=True)
    assert same(state(nn), before) and first.generation == 3
    nn.train_records(rec[:32], epochs=1, batchsize=8)
    trained = nn.eval_records(rec, per_record=True)
    assert trained.generation == nn.get_generation() == 4 and trained.policy_loss != first.policy_loss
    nn.load_weights(blob, 3)
    assert same_result(nn.eval_records(rec, per_record=True), first)
    nn.close()


def test_beside_infer_from_other_threads():
    """kh_eval_* takes the device calls' lock, kh_infer a slot of its own: both from several threads at once, every result
    the one the call gives alone."""
    import threading
    rec = records(73)
    nn = engine("bf16-64x2")
    want = nn.eval_records(rec, per_record=True)
    planes = nn.encode(rec["board"][:16])
    p0, v0 = nn.infer(planes)
    errors = []

    def infer():
        try:
            for _ in range(20):
                p, v = nn.infer(planes)
                assert np.array_equal(p, p0) and np.array_equal(v, v0)
        except Exception as e:                                 # (an assertion in a thread would otherwise pass unseen)
            errors.append(e)

    def evaluate():
        try:
            for _ in range(10):
                assert same_result(nn.eval_records(rec, per_record=True), want)
        except Exception as e:
            errors.append(e)

    threads = [threading.Thread(target=f) for f in (infer, evaluate, infer, evaluate)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    nn.close()


def test_status():
    rec = records(73)
    dtype, C_, R, seed = ENGINES["f32-16x1"]
    nn = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype=dtype)
    with pytest.raises(KamiError) as ei:
        nn.eval_records(rec)
    assert ei.value.status == L.KH_ERR_NO_WEIGHTS
    ring = DeviceReplay(nn, 16)
    ring.add(rec[:16])
    with pytest.raises(KamiError) as ei:
        nn.eval_replay(ring)
    assert ei.value.status == L.KH_ERR_NO_WEIGHTS
    good = W.random_weights(30, C_, R, seed=seed, peaky=10.0)
    planes = None
    for name, status in (("valuefc.bias", L.KH_ERR_NAN_VALUE), ("policyconv2.bias", L.KH_ERR_NAN_POLICY)):
        blob = good.copy()
        W.split(blob, 30, C_, R)[name][0] = np.nan
        nn.load_weights(blob, 1)
        planes = nn.encode(rec["board"][:4]) if planes is None else planes
        with pytest.raises(KamiError) as served:
            nn.infer(planes)
        for call in (lambda: nn.eval_records(rec), lambda: nn.eval_replay(ring)):
            with pytest.raises(KamiError) as ei:
                call()
            assert ei.value.status == status == served.value.status and str(ei.value) == str(served.value)
    nn.load_weights(good, 1)
    # non-finite numbers of the records themselves are no error
    odd = rec[:8].copy()
    odd["value"][3] = np.nan
    res = nn.eval_records(odd, per_record=True)
    assert np.isnan(res.value_loss) and np.isnan(res.record_value_loss[3]) and np.isfinite(np.delete(res.record_value_loss, 3)).all()
    assert np.isfinite(res.policy_loss)
    # what is rejected before any device work
    twice = rec[:8].copy()
    twice["actions"][5, 2] = twice["actions"][5, 0]
    with pytest.raises(KamiError) as ei:
        nn.eval_records(twice)
    bad = C.c_int(-1)
    assert nn._lib.kh_records_validate(twice.ctypes.data, twice.size, C.byref(bad)) == L.KH_ERR_INVALID and bad.value == 5
    assert ei.value.status == L.KH_ERR_INVALID and str(ei.value) == L.last_error()
    for first, n in ((-1, 4), (16, 4), (0, 0), (0, 17), (3, -2)):
        with pytest.raises(KamiError) as ei:
            nn.eval_replay(ring, first, n)
        assert ei.value.status == L.KH_ERR_INVALID
    res = L.EvalResult()
    assert nn._lib.kh_eval_records(nn.handle, rec.ctypes.data, 0, C.byref(res), None, None) == L.KH_ERR_INVALID
    assert nn._lib.kh_eval_records(nn.handle, rec.ctypes.data, 8, None, None, None) == L.KH_ERR_INVALID
    wide = NN(8, 8, 119, 4672, filters=16, residuals=1, dtype="f32")
    wide.load_weights(W.random_weights(119, 16, 1, seed=1), 0)
    for call in (lambda: wide.eval_records(rec), lambda: wide.eval_replay(ring)):
        with pytest.raises(KamiError) as ei:
            call()
        assert ei.value.status == L.KH_ERR_INVALID and "features" in str(ei.value)
    ring.close(); wide.close(); nn.close()


KEYS_TODAY = {"evals", "games_finished", "records", "merged", "generation_before", "first_loss", "last_loss", "trained_on",
              "generation_after"}


def test_generation_with_a_holdout_ring():
    from kami_amd import search as S, cycle
    C_, R = 32, 2
    nn = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(30, C_, R, seed=21, peaky=3.0), 0)
    pool = S.Pool(nn, games=256, threads=4, nodes=16, seed=7)
    ring, held = DeviceReplay(nn, 4096, seed=2), DeviceReplay(nn, 1024, seed=3)
    kw = dict(play_evals=150000, play_seconds=60.0, epochs=2, batchsize=8, sample=256)
    fields = {"records", "policy_records", "policy_loss", "value_loss", "top1", "generation"}

    def check(out, gen_before, gen_trained):
        for key, gen in (("holdout_before", gen_before), ("holdout", gen_trained)):
            h = out[key]
            assert set(h) == fields and h["generation"] == gen and h["records"] == min(held.count(), 1024)
            assert np.isfinite([h["policy_loss"], h["value_loss"], h["top1"]]).all() and 0 <= h["top1"] <= 1
        assert out["holdout"]["policy_loss"] != out["holdout_before"]["policy_loss"]

    out = cycle.generation(nn, pool, ring, holdout=held, holdout_pct=25, **kw)
    assert out["records"] > 0 and out["held_out"] == out["records"] * 25 // 100
    assert held.count() == out["held_out"] and ring.count() + held.count() == out["records"]
    assert out["generation_after"] == out["generation_before"] + 1 == 1 and out["trained_on"] == 256
    check(out, 0, 1)
    # with a gate the candidate's figures come from the clone: generation 2 whether or not it is installed
    total = ring.count() + held.count()
    out = cycle.generation(nn, pool, ring, gate=dict(games=4, nodes=12, threads=2, target_pct=0), holdout=held, holdout_pct=25, **kw)
    assert out["held_out"] == out["records"] * 25 // 100 and ring.count() + held.count() == total + out["records"]
    check(out, 1, 2)
    assert out["accepted"] is True and out["generation_after"] == 2
    # without the two arguments: today's keys, and nothing goes into the hold-out ring
    aside = held.count()
    out = cycle.generation(nn, pool, ring, **kw)
    assert set(out) == KEYS_TODAY and held.count() == aside
    for r in (ring, held):
        r.close()
