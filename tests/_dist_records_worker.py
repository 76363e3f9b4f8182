"""Worker for tests/test_records.py: gather_compact -> CompactReplay.add_bytes under torch.distributed.run, gloo backend."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kami_amd import _lib as L                               # noqa: E402
from kami_amd import dist as kd                              # noqa: E402
from kami_amd import nn as N                                 # noqa: E402
from kami_amd.replay import CompactReplay, gather_compact    # noqa: E402


def main():
    out_dir = sys.argv[1]
    rank, local_rank, world = kd.env_rank()
    dist = kd.init("gloo")
    n = 3 + rank                                              # rank r holds 3 + r records
    rec = np.zeros(n, L.RECORD_DTYPE)
    rec["value"] = 100 * rank + np.arange(n)
    rec["nact"] = 2
    rec["actions"][:, 0], rec["actions"][:, 1] = rank, 10 + np.arange(n)
    rec["visits"][:, :2] = 0.5
    ring = CompactReplay(7, seed=rank)
    added = [ring.add_bytes(blob) for blob in gather_compact(dist, rec.tobytes(), L.RECORD_DTYPE.itemsize, root=0)]
    # the ring is exactly full on the root: draws cover every slot, and the ring's order is read back through the tags
    got = ring.select(500)
    res = {"rank": rank, "count": ring.count(), "added": added, "valid": N.validate_records(got[:7]) if ring.count() else 0,
           "slots": sorted(set(got["value"].astype(int).tolist())) if ring.count() else []}
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
