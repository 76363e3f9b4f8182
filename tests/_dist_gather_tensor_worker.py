"""Worker for tests/test_replay_device_abi.py: gather_compact(as_tensor=True) against as_tensor=False under
torch.distributed.run, gloo backend."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kami_amd import _lib as L                               # noqa: E402
from kami_amd import dist as kd                              # noqa: E402
from kami_amd.replay import gather_compact                   # noqa: E402


def main():
    import torch
    out_dir = sys.argv[1]
    rank, local_rank, world = kd.env_rank()
    dist = kd.init("gloo")
    n = 3 + rank                                              # rank r holds 3 + r records
    rec = np.zeros(n, L.RECORD_DTYPE)
    rec["value"] = 100 * rank + np.arange(n)
    rec["nact"] = 2
    rec["actions"][:, 0], rec["actions"][:, 1] = rank, 10 + np.arange(n)
    rec["visits"][:, :2] = 0.5
    size = L.RECORD_DTYPE.itemsize
    as_bytes = gather_compact(dist, rec.tobytes(), size, root=0)
    tensors = gather_compact(dist, rec.tobytes(), size, root=0, as_tensor=True)
    empty = gather_compact(dist, b"", size, root=0, as_tensor=True)          # nothing to gather on any rank
    res = {"rank": rank, "bytes": [len(b) for b in as_bytes], "n": len(tensors),
           "tensor": all(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device.type == "cpu" for t in tensors),
           "equal": [t.numpy().tobytes() == b for t, b in zip(tensors, as_bytes)],
           "values": [t.numpy().view(L.RECORD_DTYPE)["value"].astype(int).tolist() for t in tensors],
           "empty": [int(t.numel()) for t in empty]}
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
