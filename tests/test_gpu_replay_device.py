"""The replay ring in device memory (kh_replay_*, kh_train_replay; kami_amd.replay.DeviceReplay).

The yardsticks are the host ring (CompactReplay: ks_ring_*), kh_records_validate and kh_train_records: the device ring
holds and returns the host ring's bytes, its validator gives the host validator's verdict in the host's words, and
training from it equals kh_train_records on what the host ring would have selected, BIT FOR BIT — so no tolerance
appears here."""
import ctypes as C
import threading

import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from kami_amd import nn as N
from kami_amd.replay import CompactReplay, DeviceReplay

from test_gpu_train_records import engine, records, same, state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")       # (before the first engine: torch finds no GPU when it is imported after one exists)

_CACHE = {}
SIZE = L.RECORD_DTYPE.itemsize


def recs():
    """The fixture records and the hand-made ones (no moves, all 96 slots, black to move, ply > 255), every one with a
    value of its own, none of them 0: a slot tells which record it holds, and whether it was written at all."""
    if "rec" not in _CACHE:
        rec = records().copy()
        rec["value"] = (np.arange(rec.size, dtype=np.float32) + 1) / 2048
        _CACHE["rec"] = rec
    return _CACHE["rec"]


def hand():
    return recs()[-4:]


def small_engine():
    return engine(16, 1, W.random_weights(30, 16, 1, seed=1))


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).tobytes()


def add_raw(ring, rec, n=None, offset=0):
    """kh_replay_add_device with stream = NULL from a torch allocation -> (status, bad_index, message)"""
    t = torch.from_numpy(np.frombuffer(raw(rec) + b"\0" * 16, np.uint8).copy()).cuda(ring.device)
    torch.cuda.synchronize()                                  # the ring's own stream is not ordered behind torch's
    bad = C.c_int(7)
    rc = ring.lib.kh_replay_add_device(ring.handle, C.c_void_p(t.data_ptr() + offset), rec.size if n is None else n, None, C.byref(bad))
    return rc, bad.value, (L.last_error() if rc else "")


def add_by(way, ring, rec):
    if way == "host":
        assert ring.add(rec) == rec.size
    elif way == "tensor":
        assert ring.add_tensor(torch.from_numpy(np.frombuffer(raw(rec), np.uint8).copy()).cuda(ring.device)) == rec.size
    elif way == "tensor on a stream":                          # the upload is queued on the caller's stream just before the add
        with torch.cuda.stream(torch.cuda.Stream()):
            t = torch.from_numpy(np.frombuffer(raw(rec), np.uint8).copy()).pin_memory().to(f"cuda:{ring.device}", non_blocking=True)
            assert ring.add_tensor(t) == rec.size
    else:
        assert add_raw(ring, rec) == (L.KH_OK, -1, "")


@pytest.mark.parametrize("way", ["host", "tensor", "tensor on a stream", "raw"])
def test_ring_equals_the_host_ring_byte_for_byte(way):
    cap = 7
    nn = small_engine()
    src = np.concatenate([hand(), recs()[:60]]).copy()
    src["board"]["pad"] = np.random.default_rng(3).integers(1, 255, (src.size, 6))       # pad bytes travel as given
    host, dev = CompactReplay(cap, seed=5), DeviceReplay(nn, cap, seed=5)
    want, head, pos = np.zeros(cap, L.RECORD_DTYPE), 0, 0
    assert raw(dev.read(0, cap)) == raw(want)
    for n in (5, 4, 0, 16, 7, 1, 3):          # wraps; nothing; more than the ring holds; exactly full; half-filled workgroups
        batch = src[pos:pos + n]
        pos += n
        host.add(batch)
        add_by(way, dev, batch)
        for i in range(n):
            want[(head + i) % cap] = batch[i]
        head = (head + n) % cap
        assert dev.count() == host.count() == pos and dev.size() == host.size() == cap
        assert raw(dev.read(0, cap)) == raw(want), n
    assert raw(dev.read(5, 4)) == raw(want[[5, 6, 0, 1]])                                 # a read wraps too, and draws nothing
    assert raw(dev.select(64)) == raw(host.select(64))
    assert raw(dev.select(0)) == raw(host.select(0)) == b""
    host.clear(), dev.clear()
    assert dev.count() == host.count() == 0
    assert raw(dev.select(8)) == raw(host.select(8)) == bytes(8 * SIZE)
    batch = src[pos:pos + cap]                                 # the generator went on through the clear: same draws on both
    host.add(batch), add_by(way, dev, batch)
    assert raw(dev.read(0, cap)) == raw(batch)                 # head is back at 0
    assert raw(dev.select(40)) == raw(host.select(40))
    dev.close(), host.close()


def test_ring_outlives_its_engine():
    nn = small_engine()
    dev = DeviceReplay(nn, 9, seed=1)
    dev.add(recs()[:5])
    nn.close()
    assert raw(dev.read(0, 5)) == raw(recs()[:5]) and dev.add(recs()[5:8]) == 3 and dev.count() == 8
    dev.close()
    dev.close()


def valid12():
    """12 valid records with at least 12 moves each, the one with all 96 slots in use at index 4"""
    rec = recs()
    out = rec[np.flatnonzero(rec["nact"] >= 12)[:12]].copy()
    out[4] = hand()[1]
    assert out[4]["nact"] == 96 and (out["nact"] >= 12).all()
    return out


def defects():
    def nact_low(r): r["nact"][3] = -1
    def nact_high(r): r["nact"][3] = 97
    def action_low(r): r["actions"][3, 2] = -1
    def action_high(r): r["actions"][3, 2] = 4672
    def twice_3_70(r): r["actions"][4, 70] = r["actions"][4, 3]            # the two registers of the lane layout
    def twice_0_1(r): r["actions"][6, 1] = r["actions"][6, 0]
    def range_10_twice_5(r): r["actions"][7, 10] = 5000; r["actions"][7, 5] = r["actions"][7, 1]
    def range_2_twice_5(r): r["actions"][7, 2] = 5000; r["actions"][7, 5] = 5000
    def records_9_2(r): r["actions"][9, 0] = -7; r["nact"][2] = 200
    def record_0(r): r["actions"][0, 11] = r["actions"][0, 4]
    return [(nact_low, 3, "record 3: nact -1 outside"), (nact_high, 3, "record 3: nact 97 outside"),
            (action_low, 3, "record 3: action -1 (entry 2) outside"), (action_high, 3, "record 3: action 4672 (entry 2) outside"),
            (twice_3_70, 4, "(entry 70)"), (twice_0_1, 6, "(entry 1)"), (range_10_twice_5, 7, "twice (entry 5)"),
            (range_2_twice_5, 7, "action 5000 (entry 2) outside"), (records_9_2, 2, "record 2: nact 200 outside"),
            (record_0, 0, "record 0:")]


@pytest.mark.parametrize("way", ["raw", "host", "tensor"])
def test_device_validation_equals_the_hosts(way):
    cap = 8                                                    # 12 records in one add: records 0..3 would never be written
    nn = small_engine()
    lib = L.load()
    host, dev = CompactReplay(cap, seed=9), DeviceReplay(nn, cap, seed=9)
    host.add(recs()[200:205]), dev.add(recs()[200:205])
    before = raw(dev.read(0, cap))
    assert before == raw(np.concatenate([recs()[200:205], np.zeros(3, L.RECORD_DTYPE)]))
    for spoil, where, words in defects():
        rec = valid12()
        spoil(rec)
        bad = C.c_int(7)
        want = (lib.kh_records_validate(rec.ctypes.data, rec.size, C.byref(bad)), bad.value, L.last_error())
        assert want[:2] == (L.KH_ERR_INVALID, where) and words in want[2], want
        if way == "raw":
            got = add_raw(dev, rec)
        elif way == "host":
            bad = C.c_int(7)
            got = (lib.kh_replay_add(dev.handle, rec.ctypes.data, rec.size, C.byref(bad)), bad.value, L.last_error())
        else:
            with pytest.raises(KamiError) as ei:
                dev.add_tensor(torch.from_numpy(np.frombuffer(raw(rec), np.uint8).copy()).cuda())
            got = (ei.value.status, ei.value.bad_index, str(ei.value))
        print(spoil.__name__, got)
        assert got == want
        assert raw(dev.read(0, cap)) == before and dev.count() == 5
    # entries behind nact are not judged, and travel as they are
    rec = valid12()
    rec["nact"][5] = 4
    rec["actions"][5, 4:] = np.resize(np.array([-1, 4672, 9, 9, 32767, -32768], np.int16), 92)
    assert N.validate_records(rec) == 12
    host.add(rec), add_by(way, dev, rec)
    assert raw(dev.read(0, cap)) != before and dev.count() == 17
    assert raw(dev.read(1, 2)) == raw(rec[4:6])               # head was 5: record i in slot (5 + i) % 8, records 0..3 never written
    assert raw(dev.select(48)) == raw(host.select(48))         # the failed adds moved neither head nor the generator


def test_add_device_argument_checks():
    nn = small_engine()
    lib = L.load()
    dev = DeviceReplay(nn, 8, seed=9)
    dev.add(recs()[:3])
    before = raw(dev.read(0, 8))
    rec = valid12()[:3].copy()
    t = torch.from_numpy(np.frombuffer(raw(rec) + bytes(8), np.uint8).copy()).cuda()
    torch.cuda.synchronize()

    def call(ptr, n):
        bad = C.c_int(7)
        rc = lib.kh_replay_add_device(dev.handle, C.c_void_p(ptr), n, None, C.byref(bad))
        assert bad.value == -1                                 # the records are not to blame
        return rc, L.last_error() if rc else ""

    assert call(rec.ctypes.data, 3) == (L.KH_ERR_INVALID, "d_rec is not device memory of device 0")
    assert call(t.data_ptr() + 4, 3) == (L.KH_ERR_INVALID, "d_rec must be 8-byte aligned")
    rc, msg = call(t.data_ptr(), 1 << 24)                      # (11 GB: past the end of whatever block the allocator cut this from)
    assert rc == L.KH_ERR_INVALID and "do not fit its allocation" in msg
    rc, msg = call(t.data_ptr(), -1)
    assert rc == L.KH_ERR_INVALID and "n >= 0" in msg
    assert call(None, 2)[0] == L.KH_ERR_INVALID
    assert call(None, 0) == (L.KH_OK, "")
    assert raw(dev.read(0, 8)) == before and dev.count() == 3
    for wrong in (t.cpu(), t[:2 * SIZE].view(torch.int8), t[:2 * SIZE + 1], t[: 4 * SIZE: 2], np.zeros(SIZE, np.uint8)):
        with pytest.raises(ValueError):
            dev.add_tensor(wrong)


def test_add_device_rejects_another_gpus_memory():
    if torch.cuda.device_count() < 2:
        pytest.skip("a tensor on another device needs a second GPU")
    nn = small_engine()
    dev = DeviceReplay(nn, 8, seed=9)
    rec = valid12()[:3].copy()
    other = torch.from_numpy(np.frombuffer(raw(rec), np.uint8).copy()).to("cuda:1")
    torch.cuda.synchronize()
    bad = C.c_int(7)
    assert dev.lib.kh_replay_add_device(dev.handle, C.c_void_p(other.data_ptr()), 3, None, C.byref(bad)) == L.KH_ERR_INVALID
    assert "not device memory of device 0" in L.last_error() and bad.value == -1
    with pytest.raises(ValueError):
        dev.add_tensor(other)
    assert raw(dev.read(0, 8)) == bytes(8 * SIZE) and dev.count() == 0


def rings(nn, cap, added, seed, start=0):
    """a host ring and a device ring with the same `added` records, put in by three adds"""
    host, dev = CompactReplay(cap, seed=seed), DeviceReplay(nn, cap, seed=seed)
    src = np.concatenate([hand(), recs()[start:start + added]])[:added]
    for part in np.array_split(src, 3):
        host.add(part), dev.add(part)
    return host, dev


#              C, R, capacity, added, n, batch, epochs, the ring's seed, optimizer options
TRAIN_CASES = [(16, 1, 13, 13, 11, 4, 2, 1, {}),         # ragged last batch
               (64, 1, 40, 25, 5, 8, 1, 65, {}),         # the first batch is shorter than the batch size; with this seed the five
                                                         # draws take two never-written slots and three written ones
               (16, 1, 6, 20, 24, 8, 2, 3, {}),          # more draws than slots: duplicates in a batch; the ring wrapped three times
               (64, 1, 300, 300, 257, 257, 1, 4, {}),    # the large-batch step
               (16, 1, 50, 50, 30, 8, 2, 5, dict(momentum=0.9, nesterov=True, weight_decay=1e-4, max_grad_norm=2.0))]


@pytest.mark.parametrize("C_,R,cap,added,n,batch,epochs,seed,optim", TRAIN_CASES)
def test_train_replay_is_train_records_on_the_host_rings_draws(C_, R, cap, added, n, batch, epochs, seed, optim):
    blob = W.random_weights(30, C_, R, seed=7, peaky=3.0)
    a, b = engine(C_, R, blob), engine(C_, R, blob)
    host, dev = rings(b, cap, added, seed=seed)
    sel = host.select(n)
    if added < cap:
        assert (sel["value"] == 0).any() and (sel["value"] != 0).any()      # zero slots and written ones
    la = a.train_records(sel, epochs=epochs, batchsize=batch, **optim)
    lb = b.train_replay(dev, n, epochs=epochs, batchsize=batch, **optim)
    print(f"C={C_} cap={cap} n={n} batch={batch}: records loss {la!r}, replay loss {lb!r}")
    assert la == lb and np.isfinite(la).all()
    assert same(state(a), state(b)) and a.get_generation() == 4
    assert not np.array_equal(state(b)[0], blob.view(np.uint32))            # it trained
    if optim:
        na, nb = a.last_grad_norms(), b.last_grad_norms()
        assert na.size == epochs * -(-n // batch) and np.array_equal(na.view(np.uint32), nb.view(np.uint32))
    # a second call goes on in the draw sequence: n draws per call, and the ring is as it was
    la = a.train_records(host.select(n), epochs=epochs, batchsize=batch, **optim)
    lb = b.train_replay(dev, n, epochs=epochs, batchsize=batch, **optim)
    assert la == lb and same(state(a), state(b)) and a.get_generation() == 5
    assert raw(dev.select(16)) == raw(host.select(16))


def test_train_replay_rejections_and_clones():
    C_, R = 16, 1
    blob = W.random_weights(30, C_, R, seed=4, peaky=3.0)
    a, b = engine(C_, R, blob), engine(C_, R, blob)
    host, dev = rings(b, 20, 20, seed=3)
    # rejected by the argument checks: the same words as kh_train_records, and no draw is consumed
    for kw in (dict(batchsize=1), dict(epochs=0), dict(batchsize=4, momentum=1.5)):
        with pytest.raises(KamiError) as ea:
            a.train_records(recs()[:12], **kw)
        with pytest.raises(KamiError) as eb:
            b.train_replay(dev, 12, **kw)
        assert ea.value.status == eb.value.status == L.KH_ERR_INVALID and str(ea.value) == str(eb.value)
    with pytest.raises(KamiError) as eb:
        b.train_replay(dev, 0, batchsize=4)
    assert eb.value.status == L.KH_ERR_INVALID
    fresh = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="f32")
    with pytest.raises(KamiError) as eb:
        fresh.train_replay(dev, 12, batchsize=4)
    assert eb.value.status == L.KH_ERR_NO_WEIGHTS
    wide = engine(C_, R, W.random_weights(119, C_, R, seed=4), F=119)
    with pytest.raises(KamiError) as eb:
        wide.train_replay(dev, 12, batchsize=4)
    assert eb.value.status == L.KH_ERR_INVALID and "features == 30" in str(eb.value)
    assert same(state(b), (blob.view(np.uint32), 3, 0))
    assert raw(dev.select(10)) == raw(host.select(10))
    # a clone trains from the ring of its original
    ca, cb = a.clone(), b.clone()
    la = ca.train_records(host.select(16), epochs=2, batchsize=8)
    lb = cb.train_replay(dev, 16, epochs=2, batchsize=8)
    assert la == lb and same(state(ca), state(cb)) and cb.get_generation() == 4 and b.get_generation() == 3
    # NaN weights under detect_anomaly: the same failure, the parameters stay, the draws are spent
    nan = blob.copy()
    nan[:64] = np.nan
    errs = []
    for nn, call in ((a, lambda: a.train_records(host.select(16), epochs=1, batchsize=8, detect_anomaly=True)),
                     (b, lambda: b.train_replay(dev, 16, epochs=1, batchsize=8, detect_anomaly=True))):
        nn.load_weights(nan, 3)
        with pytest.raises(KamiError) as ei:
            call()
        errs.append((ei.value.status, str(ei.value)))
        assert np.array_equal(nn.get_weights().view(np.uint32), nan.view(np.uint32)) and nn.get_generation() == 3
    print(errs)
    assert errs[0] == errs[1] and errs[0][0] in (L.KH_ERR_NAN_POLICY, L.KH_ERR_NAN_VALUE)
    assert raw(dev.select(10)) == raw(host.select(10))


def test_concurrent_adds():
    nn = small_engine()
    dev = DeviceReplay(nn, 128, seed=0)
    src = recs()[300:396].copy()
    src["value"] = np.arange(96, dtype=np.float32) + 1        # call c of thread t holds 1 + 24 t + 3 c .. + 2
    errors = []

    def work(t):
        try:
            for c in range(8):
                first = 24 * t + 3 * c
                assert dev.add(src[first:first + 3]) == 3
        except Exception as e:                                 # (an assertion in a thread would otherwise pass unseen)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and dev.count() == 96
    got = dev.read(0, 128)
    assert raw(got[96:]) == bytes(32 * SIZE)
    starts = got["value"][0:96:3].astype(int)
    assert sorted(starts.tolist()) == list(range(1, 97, 3))    # every call once, in whatever order
    for k in range(32):                                        # ... and each call's three records side by side, verbatim
        first = int(starts[k]) - 1
        assert raw(got[3 * k:3 * k + 3]) == raw(src[first:first + 3])


def test_generation_on_a_device_ring():
    from kami_amd import search as S, cycle
    C_, R = 32, 2
    nn = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(30, C_, R, seed=21, peaky=3.0), 0)
    pool = S.Pool(nn, games=256, threads=4, nodes=16, seed=7)
    ring = DeviceReplay(nn, 4096, seed=2)
    kw = dict(play_evals=150000, play_seconds=60.0, epochs=2, batchsize=8, sample=256)
    out = cycle.generation(nn, pool, ring, **kw)
    assert out["records"] > 0 and ring.count() == out["records"]
    assert out["generation_after"] == out["generation_before"] + 1 == 1 and out["trained_on"] == 256
    assert np.isfinite([out["first_loss"], out["last_loss"]]).all()
    assert N.validate_records(ring.read(0, min(ring.count(), 4096))) > 0
    # with a gate a clone trains from the ring
    before = ring.count()
    out = cycle.generation(nn, pool, ring, gate=dict(games=4, nodes=12, threads=2, target_pct=0), **kw)
    assert ring.count() == before + out["records"] and out["trained_on"] == 256
    assert np.isfinite([out["first_loss"], out["last_loss"]]).all()
    assert out["accepted"] is True and out["gate_games"] >= 1 and out["generation_after"] == out["generation_before"] + 1 == 2


def test_one_rank_rccl_payload_stays_on_the_device(tmp_path):
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 30300 + os.getpid() % 1000
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "_rccl_replay_worker.py"), str(tmp_path)], timeout=600, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.load(open(tmp_path / "rank0.json"))
    assert res["backend"].lower() == "nccl" and res["parts"] == 1 and res["cuda"] is True and res["dtype"] == "torch.uint8"
    assert res["added"] == 9 and res["count"] == 9 and res["same_bytes"] is True and res["rest_zero"] is True
