"""The device replay ring's C boundary without a GPU (kh_replay_*, kh_train_replay), and gather_compact(as_tensor=True)
over two gloo ranks."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

from kami_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kh_replay_create", "kh_replay_destroy", "kh_replay_add", "kh_replay_add_device", "kh_replay_count", "kh_replay_size",
         "kh_replay_clear", "kh_replay_read", "kh_replay_select", "kh_train_replay"]


def test_symbols_exported_and_listed():
    lib = L.load()
    for n in NAMES:
        assert n in L.SYMBOLS and hasattr(lib, n), n


def test_create_rejects_before_any_device_work():
    lib = L.load()
    h = C.c_void_p(1)
    assert lib.kh_replay_create(None, 16, 0, C.byref(h)) == L.KH_ERR_INVALID
    assert not h.value                                        # a failed create hands out nothing
    assert lib.kh_replay_create(None, 16, 0, None) == L.KH_ERR_INVALID
    # the capacity is judged first: no engine, no device needed
    for cap in (0, -3, (1 << 24) + 1):
        assert lib.kh_replay_create(None, cap, 0, C.byref(h)) == L.KH_ERR_INVALID
        assert f"capacity {cap} outside [1, {1 << 24}]" in L.last_error()


def test_null_ring_is_harmless():
    lib = L.load()
    rec = np.zeros(2, L.RECORD_DTYPE)
    bad = C.c_int(5)
    assert lib.kh_replay_count(None) == 0 and lib.kh_replay_size(None) == 0
    lib.kh_replay_destroy(None)
    assert lib.kh_replay_clear(None) == L.KH_ERR_INVALID
    assert lib.kh_replay_add(None, rec.ctypes.data, 2, C.byref(bad)) == L.KH_ERR_INVALID and bad.value == -1
    assert lib.kh_replay_add_device(None, None, 0, None, None) == L.KH_ERR_INVALID
    assert lib.kh_replay_read(None, 0, 2, rec.ctypes.data) == L.KH_ERR_INVALID
    assert lib.kh_replay_select(None, 2, rec.ctypes.data) == L.KH_ERR_INVALID
    cfg = L.TrainConfig(0.005, 1, 4, 0, 0.0, 0.0, 0.0, 0)
    assert lib.kh_train_replay(None, None, 4, C.byref(cfg), None, None) == L.KH_ERR_INVALID


def test_two_rank_gloo_gather_as_tensor(tmp_path):
    port = 33000 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "_dist_gather_tensor_worker.py"), str(tmp_path)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    subprocess.run(cmd, check=True, timeout=300, env=env, capture_output=True)
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    # rank r contributed 3 + r records tagged 100 r + i
    assert res[0]["n"] == 2 and res[0]["tensor"] and res[0]["equal"] == [True, True]
    assert res[0]["bytes"] == [3 * 664, 4 * 664] and res[0]["values"] == [[0, 1, 2], [100, 101, 102, 103]]
    assert res[0]["empty"] == [0, 0]
    assert res[1]["n"] == 0 and res[1]["bytes"] == [] and res[1]["empty"] == []


def test_gather_without_a_group():
    import torch
    from kami_amd.replay import gather_compact
    payload = (np.arange(664 * 2) % 251).astype(np.uint8).tobytes()
    assert gather_compact(None, payload, 664) == [payload]
    (t,) = gather_compact(None, payload, 664, as_tensor=True)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device.type == "cpu" and t.numpy().tobytes() == payload
    (t,) = gather_compact(None, b"", 664, as_tensor=True)
    assert t.numel() == 0 and t.dtype == torch.uint8
