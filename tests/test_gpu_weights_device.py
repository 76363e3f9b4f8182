"""kh_load_weights_device: a parameter set installed from a blob in device memory, its serving layouts written by the
kernels of weights_pack.hip.  The yardstick is the host packer of the same build (kh_load_weights) and the tolerance
is zero: two engines of one configuration, one installed each way, must give the same bits for policy, value tensor and
logits, the same kh_get_weights and the same generation.

Which case reads which buffer of a Weights (weights.hip: plan_tower, plan_layers, plan_simple; choose_plan picks the
kernel by batch size):

    test_small_nets          tw_stream (F=30: the stem in one pass; F=119: four 32-plane quarters; centre-first permuted
                             3x3 layers; the 6-of-8-fragment policyconv2 chunks; the parity chunk), tw_par (folded shifts,
                             policy bias, value conv), tw_fc4; C=24: channel padding of all of them
    test_wide_128            ly_w4 (tower128_kernel at batch 700, heads inside: ly_wh, ly_misc with fc4), tower2b<128>
                             (batch 300), the per-layer kernels on ly_w / ly_shift (batch 40)
    test_wide_256            ly_w2b (CBC 256) through tower2s_kernel (batch 64) and tower2b<256> (batch 300)
    test_generic_layout      ly_w with padded Co / Ci (C=96), ly_shift, per-layer heads (F=30: no ly_w2b)
    test_ragged_wide_stem    a stem with CiP = 256 of which 200 channels are live (F=200: beyond the whole-network kernel)
    test_f32                 the fp32 fragments' (PK_F32) ly_w, ly_shift, ly_misc; `simple` (scale, shift, the [tap][ci][co] transpose)
                             in a child process with KAMI_F32_SIMPLE=1
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from kami_amd import NN, KamiError, _lib as L, weights as W
from _weights_device_util import _ptr, host_and_device_agree, install_device, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")       # (before the first engine: torch finds no GPU when it is imported after one exists)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blobs_for(F, C_, R, seed):
    return [W.random_weights(F, C_, R, seed=seed), W.random_weights(F, C_, R, seed=seed + 1, peaky=10.0)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("F,filters", [(30, 24), (30, 64), (119, 24), (119, 64)])
def test_small_nets(dtype, F, filters):
    assert host_and_device_agree(dtype, F, filters, 2, [37], blobs_for(F, filters, 2, 1)) == []


def test_wide_128():
    assert host_and_device_agree("bf16", 119, 128, 2, [700, 300, 40], blobs_for(119, 128, 2, 3)) == []


def test_wide_256():
    assert host_and_device_agree("f16", 119, 256, 1, [64, 300], blobs_for(119, 256, 1, 5)) == []


@pytest.mark.parametrize("filters", [96, 128])
def test_generic_layout(filters):
    assert host_and_device_agree("bf16", 30, filters, 2, [40], blobs_for(30, filters, 2, 7)) == []


def test_ragged_wide_stem():
    assert host_and_device_agree("bf16", 200, 64, 1, [3], blobs_for(200, 64, 1, 21)) == []


@pytest.mark.parametrize("filters", [64, 128])
def test_f32(filters):
    assert host_and_device_agree("f32", 30, filters, 1, [20], blobs_for(30, filters, 1, 9)) == []


def test_f32_simple_layers_in_a_child_process():
    env = dict(os.environ, KAMI_F32_SIMPLE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_weights_device_child.py")], timeout=300, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == []


def random_boards(n, seed):
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
    return b


@pytest.mark.parametrize("filters", [64, 128])
def test_encode_infer_after_a_device_install(filters):
    """The fused ingest (board records in, no planes in memory) reads the same set."""
    F, R = 30, 2
    blob = W.random_weights(F, filters, R, seed=11, peaky=10.0)
    host = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
    dev = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
    host.load_weights(blob, 1)
    assert install_device(dev, blob, 1) == L.KH_OK
    boards = random_boards(77, 2)
    assert same_bits(dev.encode_infer(boards), host.encode_infer(boards))


def test_refused_calls_leave_the_installed_set():
    """A wrong nfloats, a host pointer and a null pointer: KH_ERR_INVALID each (the checks are host-side, before any device
    work), and the generation installed before still answers with its own bits."""
    F, filters, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
    blob = W.random_weights(F, filters, R, seed=13, peaky=10.0)
    other = W.random_weights(F, filters, R, seed=14)
    assert install_device(nn, blob, 5) == L.KH_OK
    x = np.random.default_rng(0).random((37, 8, 8, F), dtype=np.float32)
    want = nn.infer_full(x)
    lib = nn._lib
    assert install_device(nn, other, 6, nfloats=other.size - 1) == L.KH_ERR_INVALID
    assert f"{other.size - 1} floats, expected {other.size}" in L.last_error()
    assert lib.kh_load_weights_device(nn.handle, _ptr(other), other.size, 6, None) == L.KH_ERR_INVALID      # host memory
    assert "not device memory" in L.last_error()
    assert lib.kh_load_weights_device(nn.handle, None, other.size, 6, None) == L.KH_ERR_INVALID
    assert "null" in L.last_error()
    assert nn.get_generation() == 5 and same_bits(nn.infer_full(x), want)
    assert np.array_equal(nn.get_weights().view(np.uint32), blob.view(np.uint32))


@pytest.mark.parametrize("dtype,F,filters", [("bf16", 119, 64), ("bf16", 30, 128), ("f32", 30, 64)])
def test_blob_may_be_overwritten_once_the_call_returns(dtype, F, filters):
    R = 1
    blob = W.random_weights(F, filters, R, seed=15, peaky=10.0)
    host = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype=dtype)
    dev = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype=dtype)
    host.load_weights(blob, 2)
    assert install_device(dev, blob, 2, zero_after=True) == L.KH_OK
    x = np.random.default_rng(1).random((37, 8, 8, F), dtype=np.float32)
    assert same_bits(dev.infer_full(x), host.infer_full(x))
    assert np.array_equal(dev.get_weights().view(np.uint32), blob.view(np.uint32))


def test_nn_load_weights_takes_a_cuda_tensor():
    F, filters, R = 119, 64, 2
    blob = W.random_weights(F, filters, R, seed=17, peaky=10.0)
    a = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="f16")
    b = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="f16")
    a.load_weights(blob, 9)
    t = torch.from_numpy(blob).to("cuda:0")
    for stream in (None, torch.cuda.Stream()):                   # torch's default stream, and one of the caller's
        if stream is None:
            b.load_weights(t * 1.0, 9)                           # (a product queued on the stream just before the call)
        else:
            with torch.cuda.stream(stream):
                b.load_weights(t * 1.0, 9)
        x = np.random.default_rng(2).random((37, 8, 8, F), dtype=np.float32)
        assert b.get_generation() == 9 and same_bits(b.infer_full(x), a.infer_full(x))
        assert np.array_equal(b.get_weights().view(np.uint32), blob.view(np.uint32))
    b.load_weights(torch.from_numpy(blob), 10)                   # a CPU tensor takes the host path
    assert b.get_generation() == 10 and same_bits(b.infer_full(x), a.infer_full(x))
    with pytest.raises(ValueError):
        b.load_weights(t.double(), 11)
    with pytest.raises(ValueError):
        b.load_weights(t[:-1], 11)
    with pytest.raises(ValueError):
        b.load_weights(torch.cat([t, t])[::2], 11)
    assert b.get_generation() == 10


def test_device_install_while_threads_infer():
    """As test_weight_swap_while_threads_infer, the swaps made by kh_load_weights_device: every answer is set A's or set
    B's, never a mixture."""
    F, filters, R = 30, 64, 2
    nn = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
    blobs = [W.random_weights(F, filters, R, seed=s, peaky=10.0) for s in (1, 2)]
    xs = [np.random.default_rng(i).random((8 + 24 * (i % 2), 8, 8, F), dtype=np.float32) for i in range(4)]
    want = []
    for b in blobs:
        nn.load_weights(b, 1)                                    # the host packer says what each set answers
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
    try:
        for g in range(40):
            assert install_device(nn, blobs[g & 1], g + 2) == L.KH_OK
    finally:
        stop.set()
        [t.join() for t in th]
    assert not bad
    assert nn.get_generation() == 41 and all(len(s) == 2 for s in seen)


@pytest.mark.parametrize("filters", [64, 128])
def test_trained_set_equals_its_blob_through_the_host_packer(filters):
    """kh_train installs its result with the device packer, from the trainer's own parameters: the trained engine and a
    fresh engine given kh_get_weights through kh_load_weights (the host packer) answer with the same bits."""
    F, R, n = 30, 1, 24
    rng = np.random.default_rng(filters)
    nn = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, filters, R, seed=19, peaky=5.0), 1)
    x = rng.random((n, 8, 8, F), dtype=np.float32)
    p = rng.random((n, 4672), dtype=np.float32)
    p /= p.sum(1, keepdims=True)
    v = rng.uniform(-1, 1, n).astype(np.float32)
    for call in range(2):                                        # the second call trains the set the first one left on the device
        nn.train(x, p, v, mlr=5, epochs=1, batchsize=8)
        assert nn.get_generation() == 2 + call
        fresh = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype="bf16")
        fresh.load_weights(nn.get_weights(), nn.get_generation())
        q = rng.random((37, 8, 8, F), dtype=np.float32)
        assert same_bits(nn.infer_full(q), fresh.infer_full(q))
        fresh.close()


def test_rccl_broadcast_tensor_is_installed_from_device_memory(tmp_path):
    """broadcast_weights(as_tensor=True) through RCCL (a world of one rank, as test_rccl_backend_single_rank_group) hands
    NN.load_weights a device tensor."""
    port = 29400 + os.getpid() % 1000
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rccl_tensor_worker.py"), str(tmp_path)], timeout=600, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.load(open(tmp_path / "rank0.json"))
    assert res == {"is_tensor": True, "device": "cuda", "gen": 45, "generation": 45, "same": True, "weights": True}
