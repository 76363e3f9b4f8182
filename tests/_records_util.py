"""Record builders shared by tests/test_records.py and tests/test_gpu_train_records.py (test infrastructure)."""
import os

import numpy as np

from kami_amd import _lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_records(seed=0, boards=None):
    """One record per position of observe_playouts.npz: its legal actions, seeded random visit shares normalised per
    record, a seeded value in [-1, 1]; `boards` (kh_board array) fills the board field when given."""
    z = np.load(os.path.join(GOLD, "observe_playouts.npz"), allow_pickle=False)
    nact, actions = z["nact"], z["actions"]
    n = nact.size
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, L.RECORD_DTYPE)
    if boards is not None:
        rec["board"] = boards
    rec["nact"] = nact
    rec["value"] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    for i in range(n):
        k = int(nact[i])
        rec["actions"][i, :k] = actions[i, :k]
        v = rng.random(k).astype(np.float32) + np.float32(1e-3)
        rec["visits"][i, :k] = v / v.sum(dtype=np.float32)
    return rec


def full_record(seed=1):
    """A record with all 96 action slots in use."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(1, L.RECORD_DTYPE)
    rec["nact"] = 96
    rec["actions"][0] = np.sort(rng.choice(4672, 96, replace=False)).astype(np.int16)
    v = rng.random(96).astype(np.float32)
    rec["visits"][0] = v / v.sum(dtype=np.float32)
    rec["value"] = 0.25
    return rec


def scatter(rec):
    """obs_p, obs_v as kh_expand_records defines them, in NumPy."""
    obs_p = np.zeros((rec.size, 4672), np.float32)
    for i in range(rec.size):
        k = int(rec["nact"][i])
        obs_p[i, rec["actions"][i, :k]] = rec["visits"][i, :k]
    return obs_p, rec["value"].astype(np.float32)
