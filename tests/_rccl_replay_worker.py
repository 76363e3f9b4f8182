"""Worker for tests/test_gpu_replay_device.py: gather_compact(as_tensor=True) through torch.distributed's "nccl" backend
(= RCCL on ROCm) leaves the root's payloads in device memory, and DeviceReplay.add_tensor takes them from there.  Runs
as a world of ONE rank (still an RCCL communicator: same backend, same tensor placement rules, no peer)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kami_amd import NN, _lib as L, dist as kd, weights as W     # noqa: E402
from kami_amd.replay import DeviceReplay, gather_compact        # noqa: E402


def main():
    out_dir = sys.argv[1]
    rank, local_rank, world = kd.env_rank()
    dist = kd.init("nccl", single_rank_group=True)
    assert dist is not None and str(dist.get_backend()).lower() == "nccl"
    n = 9
    rng = np.random.default_rng(5)
    rec = np.zeros(n, L.RECORD_DTYPE)
    rec["value"] = 1 + np.arange(n)
    rec["nact"] = 3 + np.arange(n)
    for i in range(n):
        k = int(rec["nact"][i])
        rec["actions"][i, :k] = np.sort(rng.choice(4672, k, replace=False))
        rec["visits"][i, :k] = 1.0 / k
    rec["board"]["piece_occ"] = rng.integers(0, 2 ** 63, (n, 6), dtype=np.uint64)
    payload = rec.tobytes()
    parts = gather_compact(dist, payload, L.RECORD_DTYPE.itemsize, root=0, as_tensor=True)
    nn = NN(8, 8, 30, 4672, filters=16, residuals=1, dtype="f32", device=local_rank)
    nn.load_weights(W.random_weights(30, 16, 1, seed=1), 0)
    ring = DeviceReplay(nn, 12, seed=0)
    added = sum(ring.add_tensor(t) for t in parts)
    got = ring.read(0, 12)
    res = {"rank": rank, "backend": str(dist.get_backend()), "parts": len(parts), "cuda": all(bool(t.is_cuda) for t in parts),
           "dtype": str(parts[0].dtype), "added": added, "count": ring.count(), "same_bytes": got[:n].tobytes() == payload,
           "rest_zero": got[n:].tobytes() == bytes(3 * L.RECORD_DTYPE.itemsize)}
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    ring.close()
    nn.close()
    kd.barrier(dist)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
