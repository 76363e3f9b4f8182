"""kh_expand_records / kh_train_records: training straight from compact replay records (kh_record, 664 bytes).

The yardstick is kh_train itself, the path pinned to the reference's NN::train fixtures (tests/test_gpu_train.py):
the record path must equal it on the expanded arrays BIT FOR BIT — parameters, BatchNorm statistics, both losses,
generation, BatchNorm batch counter, and status + message of a failed call — so no tolerance appears here."""
import os

import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from kami_amd import nn as N
from oracle import pyoracle as ko

from _records_util import GOLD, fixture_records, full_record, scatter

_CACHE = {}


def records():
    """The 1 149 fixture positions with seeded visit shares and values, plus hand-made records: no moves, all 96 move
    slots, black to move, ply > 255."""
    if "rec" not in _CACHE:
        z = np.load(os.path.join(GOLD, "observe_playouts.npz"), allow_pickle=False)
        boards = ko.boards_from_fens([s.decode() for s in z["fen"]], z["ply"])
        rec = fixture_records(seed=11, boards=boards)
        black = int(np.flatnonzero(boards["ctm"] == 1)[5])
        hand = np.zeros(4, L.RECORD_DTYPE)
        hand[0] = rec[40]
        hand[0]["nact"] = 0                                       # no moves: an all-zero visit row
        hand[0]["value"] = -1.0
        hand[1] = full_record(seed=2)[0]                          # every action slot in use
        hand[1]["board"] = boards[700]
        hand[2] = rec[black]                                      # black to move: the point of view is flipped
        hand[2]["value"] = 1.0
        hand[3] = rec[900]
        hand[3]["board"]["ply"] = 300                             # ply > 255: the eight ply planes wrap
        hand[3]["board"]["halfmove_clock"] = 77
        assert hand[2]["board"]["ctm"] == 1
        _CACHE["rec"] = np.concatenate([rec, hand])
    return _CACHE["rec"]


def engine(C, R, blob, gen=3, F=30):
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="f32")
    nn.load_weights(blob, gen)
    return nn


def state(nn):
    return nn.get_weights().view(np.uint32), nn.get_generation(), nn.bn_batches()


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def pick(n, seed):
    """n records, the hand-made ones among them when there is room"""
    rec = records()
    idx = np.random.default_rng(seed).choice(rec.size - 4, n, replace=False)
    if n >= 8:
        idx[:4] = np.arange(rec.size - 4, rec.size)
    return rec[idx].copy()


@pytest.mark.gpu
def test_expand_is_exact():
    rec = records()
    assert rec.size == 1153                                       # three chunks of kh_expand_records
    nn = engine(16, 1, W.random_weights(30, 16, 1, seed=1))
    planes, obs_p, obs_v = nn.expand_records(rec)
    want = nn.encode(rec["board"])
    assert planes.shape == want.shape == (rec.size, 8, 8, 30)
    assert np.array_equal(planes.view(np.uint32), want.view(np.uint32))
    want_p, want_v = scatter(rec)
    assert np.array_equal(obs_p, want_p) and np.array_equal(obs_v, want_v)
    assert np.count_nonzero(obs_p[-4]) == 0 and np.count_nonzero(obs_p[-3]) == 96
    # every form of input, outputs wanted one at a time (the C call takes NULL for the others)
    lib = L.load()
    one = np.empty((rec.size, 4672), np.float32)
    assert lib.kh_expand_records(nn.handle, rec.ctypes.data, rec.size, None, one.ctypes.data, None) == L.KH_OK
    assert np.array_equal(one, want_p)
    p2, _, v2 = nn.expand_records(rec[600:].tobytes())
    assert np.array_equal(p2, planes[600:]) and np.array_equal(v2, obs_v[600:])
    # records_to_arrays, the host preparation the dense path needs today, gives the same arrays
    from kami_amd import cycle
    ct = (L.Record * 64).from_buffer_copy(rec[-64:].tobytes())
    a, b, c = cycle.records_to_arrays(nn, ct)
    assert np.array_equal(a.reshape(-1), planes[-64:].reshape(-1)) and np.array_equal(b, obs_p[-64:]) and np.array_equal(c, obs_v[-64:])


CASES = [(16, 1, 11, 4, 2),        # ragged last batch at a small width
         (64, 2, 307, 8, 2),       # the reference's defaults: ring 512 x 60 %, batch 8: ragged last batch
         (64, 1, 5, 8, 1),         # the first batch is shorter than the batch size
         (256, 1, 40, 8, 2),       # 256 filters: the matrix-core convolutions with channel slices
         (64, 1, 257, 257, 1)]     # one batch of 257: the record expansion feeds the large-batch step (two-board convolutions,
                                   # weight-gradient ranges of two boards, an odd batch)


@pytest.mark.gpu
@pytest.mark.parametrize("C,R,n,batch,epochs", CASES)
def test_train_records_is_the_dense_path_bit_for_bit(C, R, n, batch, epochs):
    blob = W.random_weights(30, C, R, seed=7, peaky=3.0)
    rec = pick(n, seed=C + n)
    dense, compact = engine(C, R, blob), engine(C, R, blob)
    fd, ld = dense.train(*dense.expand_records(rec), epochs=epochs, batchsize=batch)
    fc, lc = compact.train_records(rec, epochs=epochs, batchsize=batch)
    print(f"C={C} R={R} n={n} batch={batch} epochs={epochs}: dense loss {fd!r} -> {ld!r}, records loss {fc!r} -> {lc!r}")
    assert (fd, ld) == (fc, lc) and np.isfinite([fd, ld]).all()
    sd, sc = state(dense), state(compact)
    assert sd[1:] == sc[1:] == (4, epochs * -(-n // batch))
    assert np.array_equal(sd[0], sc[0])
    assert not np.array_equal(sd[0], blob.view(np.uint32))          # it trained


@pytest.mark.gpu
def test_short_first_batch_after_an_earlier_call():
    """The batch rows live on the device from call to call.  kh_train starts every call from zeroed staging rows, so a
    first batch shorter than the batch size trains on its own rows followed by zeros — not by an earlier call's rows."""
    C, R = 32, 1
    blob = W.random_weights(30, C, R, seed=9, peaky=3.0)
    dense, compact = engine(C, R, blob), engine(C, R, blob)
    for nn in (dense, compact):                                    # both engines have trained before, on other records
        nn.train_records(pick(16, seed=1), epochs=1, batchsize=8)
        nn.load_weights(blob, 3)
    rec = pick(5, seed=2)
    ld = dense.train(*dense.expand_records(rec), epochs=2, batchsize=8)
    lc = compact.train_records(rec, epochs=2, batchsize=8)
    assert ld == lc and same(state(dense), state(compact))


@pytest.mark.gpu
def test_one_engine_alternating_paths():
    C, R = 64, 1
    blob = W.random_weights(30, C, R, seed=5, peaky=3.0)
    nn = engine(C, R, blob)
    for batch, n in ((8, 43), (12, 50)):                           # a new batch size records the step again
        rec = pick(n, seed=batch)
        runs = []
        for path in ("records", "dense", "records"):
            nn.load_weights(blob, 3)
            if path == "dense":
                loss = nn.train(*nn.expand_records(rec), epochs=2, batchsize=batch)
            else:
                loss = nn.train_records(rec, epochs=2, batchsize=batch)
            runs.append((loss, state(nn)))
        assert runs[0][0] == runs[1][0] == runs[2][0]
        assert same(runs[0][1], runs[1][1]) and same(runs[2][1], runs[1][1])
        assert runs[1][1][1] == 4
    # without a reload in between: the second call trains the first call's result, whichever path made it
    a, b = engine(C, R, blob), engine(C, R, blob)
    rec = pick(24, seed=3)
    x = a.expand_records(rec)
    a.train(*x, epochs=1, batchsize=8); a.train_records(rec, epochs=1, batchsize=8); a.train(*x, epochs=1, batchsize=8)
    b.train_records(rec, epochs=1, batchsize=8); b.train(*x, epochs=1, batchsize=8); b.train_records(rec, epochs=1, batchsize=8)
    assert same(state(a), state(b)) and a.get_generation() == 6


@pytest.mark.gpu
@pytest.mark.parametrize("detect", [False, True])
def test_nan_share_fails_like_the_dense_path(detect):
    C, R = 16, 1
    blob = W.random_weights(30, C, R, seed=4, peaky=3.0)
    rec = pick(30, seed=6)
    order = np.empty(2 * 30, np.int32)
    assert L.load().kh_train_order(30, 2, order.ctypes.data) == L.KH_OK
    victim = int(np.flatnonzero(rec["nact"] > 0)[10])
    rec["visits"][victim, 0] = np.nan                              # reaches the loss in the batch that holds the record
    first_bad = int(np.flatnonzero(order[:30] == victim)[0]) // 4
    dense, compact = engine(C, R, blob), engine(C, R, blob)
    x = dense.expand_records(rec)
    assert np.isnan(x[1]).sum() == 1
    errs = []
    for call in (lambda: dense.train(*x, epochs=2, batchsize=4, detect_anomaly=detect),
                 lambda: compact.train_records(rec, epochs=2, batchsize=4, detect_anomaly=detect)):
        with pytest.raises(KamiError) as ei:
            call()
        errs.append((ei.value.status, str(ei.value)))
    print(errs)
    assert errs[0] == errs[1] == (L.KH_ERR_NAN_POLICY, f"training loss is NaN (epoch 0, batch {first_bad})")
    for nn in (dense, compact):                                    # a failed call leaves the engine as it was
        assert same(state(nn), (blob.view(np.uint32), 3, 0))
    # and both engines still train, identically, afterwards
    rec["visits"][victim, 0] = 0.5
    ld = dense.train(*dense.expand_records(rec), epochs=1, batchsize=4)
    lc = compact.train_records(rec, epochs=1, batchsize=4)
    assert ld == lc and same(state(dense), state(compact))


@pytest.mark.gpu
def test_detect_anomaly_on_clean_data_changes_nothing():
    C, R = 16, 1
    blob = W.random_weights(30, C, R, seed=4, peaky=3.0)
    rec = pick(21, seed=8)
    a, b = engine(C, R, blob), engine(C, R, blob)
    la = a.train_records(rec, epochs=2, batchsize=4, detect_anomaly=True)
    lb = b.train_records(rec, epochs=2, batchsize=4, detect_anomaly=False)
    assert la == lb and same(state(a), state(b))


@pytest.mark.gpu
def test_rejected_arguments():
    C, R = 16, 1
    blob = W.random_weights(30, C, R, seed=4, peaky=3.0)
    nn = engine(C, R, blob)
    rec = pick(12, seed=1)
    bad = rec.copy()
    bad["actions"][7, 1] = bad["actions"][7, 0]                    # a duplicated action
    for call in (lambda: nn.train_records(bad, epochs=1, batchsize=4), lambda: nn.expand_records(bad)):
        with pytest.raises(KamiError) as ei:
            call()
        assert ei.value.status == L.KH_ERR_INVALID and "record 7:" in str(ei.value) and "twice" in str(ei.value)
    for kw in (dict(batchsize=1), dict(epochs=0)):                 # kh_train's own argument checks
        with pytest.raises(KamiError) as ei:
            nn.train_records(rec, **kw)
        with pytest.raises(KamiError) as ed:
            nn.train(*nn.expand_records(rec), **kw)
        assert ei.value.status == ed.value.status == L.KH_ERR_INVALID and str(ei.value) == str(ed.value)
    with pytest.raises(KamiError) as ei:
        nn.train_records(rec[:0], epochs=1, batchsize=4)
    assert ei.value.status == L.KH_ERR_INVALID
    assert same(state(nn), (blob.view(np.uint32), 3, 0))
    fresh = NN(8, 8, 30, 4672, filters=C, residuals=R, dtype="f32")
    with pytest.raises(KamiError) as ei:
        fresh.train_records(rec, epochs=1, batchsize=4)
    assert ei.value.status == L.KH_ERR_NO_WEIGHTS
    # no encoder for other plane counts: the record calls reject the engine
    wide = engine(C, R, W.random_weights(119, C, R, seed=4), F=119)
    for call in (lambda: wide.train_records(rec, epochs=1, batchsize=4), lambda: wide.expand_records(rec)):
        with pytest.raises(KamiError) as ei:
            call()
        assert ei.value.status == L.KH_ERR_INVALID and "features == 30" in str(ei.value)
    assert wide.get_generation() == 3


@pytest.mark.gpu
def test_from_the_pool_through_the_compact_ring():
    from kami_amd import search as S, cycle
    from kami_amd.replay import CompactReplay
    C, R = 32, 2
    nn = NN(8, 8, 30, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(30, C, R, seed=21, peaky=3.0), 0)
    pool = S.Pool(nn, games=256, threads=4, nodes=16, seed=7)
    st = pool.run(min_evals=150000, max_seconds=60.0)
    payload = pool.drain_bytes()
    assert st.games_finished > 0 and len(payload) == st.records * 664 > 0
    assert N.validate_records(payload) == st.records
    ring = CompactReplay(4096, seed=1)
    assert ring.add_bytes(payload) == st.records
    sel = ring.select(200)
    a, b = nn.clone(), nn.clone()
    la = a.train_records(sel, epochs=2, batchsize=8)
    ct = (L.Record * sel.size).from_buffer_copy(sel.tobytes())
    planes, mcts, vals = cycle.records_to_arrays(b, ct)
    lb = b.train(planes.reshape(-1, 8, 8, 30), mcts, vals, epochs=2, batchsize=8)
    assert la == lb and same(state(a), state(b)) and a.get_generation() == 1
    # the whole generation on a compact ring
    ring2 = CompactReplay(4096, seed=2)
    out = cycle.generation(nn, pool, ring2, play_evals=150000, play_seconds=60.0, epochs=2, batchsize=8, sample=256)
    assert out["records"] > 0 and ring2.count() == out["records"]
    assert out["generation_after"] == out["generation_before"] + 1 == 1 and out["trained_on"] == 256
    assert np.isfinite([out["first_loss"], out["last_loss"]]).all()


@pytest.mark.gpu
def test_kami_native_with_replay_compact(tmp_path):
    """The unmodified kami.cpp on this repository's host side with option replay_compact: 1 — finished games go into the
    compact ring as records (no encode call), the trainer thread selects records and trains the candidate from them
    (NN::train_records), the gate and the swap follow as ever."""
    import subprocess, threading, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", "kami_native")
    if not os.path.exists(exe) or b"kh_train_records" not in open(exe, "rb").read():      # (the symbol it imports for the option)
        pytest.skip("oracle/_ref/dropin/kami_native is not built from this tree (needs the reference tree at build time)")
    opts = dict(filters=16, residuals=1, selfplay_batch=16, selfplay_nodes=16, inference_threads=2, training_threads=1,
                replaybuffer_size=128, rpb_train_pct=40, training_sample_pct=60, training_epochs=2, training_batchsize=8,
                training_mlr=5, evaluate_batch=8, evaluate_games=8, evaluate_nodes=8, evaluate_target_pct=0,
                model_path=str(tmp_path / "model.bin"), engine_dtype="bf16", replay_compact=1)
    (tmp_path / "options.yml").write_text("".join(f"{k}: {v}\n" for k, v in opts.items()))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(root, "kami_amd") + (os.pathsep + env["LD_LIBRARY_PATH"] if env.get("LD_LIBRARY_PATH") else "")
    proc = subprocess.Popen(["timeout", "-k", "10", "240", exe], cwd=tmp_path, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)
    lines = []
    t = threading.Thread(target=lambda: lines.extend(iter(proc.stdout.readline, "")), daemon=True)
    t.start()
    deadline = time.time() + 150
    done = False
    while time.time() < deadline and not done and proc.poll() is None:
        time.sleep(1.0)
        done = any("candidate accepted" in l or "candidate rejected" in l for l in lines)
    try:
        proc.stdin.write("quit\n"); proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    out = "".join(lines)
    assert done, out[-3000:]
    assert "training generation 0 with 76 trajectories" in out and "Generated model 1, average loss" in out, out[-3000:]
    complaints = [l for l in out.splitlines() if "ERROR" in l or "failed" in l or "INFER" in l]
    assert all("model read from" in l for l in complaints), complaints
