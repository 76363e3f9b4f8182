"""Compact replay records (kh_record) on the host: layout, kh_records_validate, the compact ring (ks_ring_*,
kami_amd.replay.CompactReplay) and the two-rank merge into it.  No GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kami_amd import _lib as L
from kami_amd import nn as N
from kami_amd import search as S
from kami_amd.replay import CompactReplay

from _records_util import fixture_records, full_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_layout():
    assert C.sizeof(L.Record) == 664 and L.RECORD_DTYPE.itemsize == 664
    for name, off in (("board", 0), ("value", 80), ("nact", 84), ("actions", 88), ("visits", 280)):
        assert getattr(L.Record, name).offset == off
        assert L.RECORD_DTYPE.fields[name][1] == off
    # kami_amd.search.Record is still there and describes the same bytes
    assert C.sizeof(S.Record) == 664 and C.sizeof(S.Board) == 80
    assert [(n, getattr(S.Record, n).offset, getattr(S.Record, n).size) for n, _ in S.Record._fields_] == \
           [(n, getattr(L.Record, n).offset, getattr(L.Record, n).size) for n, _ in L.Record._fields_]
    r = S.Record()
    r.value, r.nact = 0.5, 2
    r.actions[0], r.actions[1], r.visits[1] = 7, 4671, 0.75
    a = N.as_records(bytes(r))
    assert a.size == 1 and a["value"][0] == 0.5 and a["nact"][0] == 2 and a["actions"][0, 1] == 4671 and a["visits"][0, 1] == 0.75


def test_as_records_takes_every_form():
    rec = fixture_records()[:5]
    ct = (L.Record * 5).from_buffer_copy(rec.tobytes())
    for form in (rec, rec.tobytes(), rec.view(np.uint8), ct, list(ct)):
        assert N.as_records(form).tobytes() == rec.tobytes()
    with pytest.raises(ValueError):
        N.as_records(rec.tobytes()[:-1])


def test_validate_accepts():
    assert N.validate_records(np.zeros(3, L.RECORD_DTYPE)) == 3          # the all-zero record: what an unwritten ring slot holds
    assert N.validate_records(full_record()) == 1
    rec = fixture_records(seed=3)
    assert rec.size == 1149 and int(rec["nact"].max()) <= 56
    assert N.validate_records(rec) == 1149
    assert N.validate_records(rec[:0]) == 0


def _set_nact(v):
    return lambda rec, at: rec["nact"].__setitem__(at, v)


def _set_action(k, v):
    return lambda rec, at: rec["actions"].__setitem__((at, k), v)


def _duplicate(rec, at):
    rec["actions"][at, 5] = rec["actions"][at, 2]


@pytest.mark.parametrize("at,breakit,rule", [
    (7, _set_nact(97), "nact 97 outside [0, 96]"),
    (0, _set_nact(-1), "nact -1 outside [0, 96]"),
    (20, _set_action(95, 4672), "action 4672 (entry 95) outside [0, 4672)"),      # record 20 is the 96-action one
    (11, _set_action(3, -1), "action -1 (entry 3) outside [0, 4672)"),
    (13, _duplicate, "appears twice"),
], ids=["nact97", "nact-1", "action4672", "action-1", "duplicate"])
def test_validate_rejects(at, breakit, rule):
    rec = np.concatenate([fixture_records(seed=4)[:20], full_record()])
    assert N.validate_records(rec) == 21
    breakit(rec, at)
    with pytest.raises(N.KamiError) as ei:
        N.validate_records(rec)
    assert ei.value.status == L.KH_ERR_INVALID and ei.value.bad_index == at
    assert f"record {at}:" in str(ei.value) and rule in str(ei.value)
    # entries at and beyond nact are not judged
    ok = fixture_records(seed=4)[:3]
    ok["actions"][1, 60:] = -5
    assert N.validate_records(ok) == 3


def _tagged(lo, hi):
    rec = np.zeros(hi - lo, L.RECORD_DTYPE)
    rec["value"] = np.arange(lo, hi, dtype=np.float32)
    rec["nact"] = 1
    rec["actions"][:, 0] = np.arange(lo, hi)
    rec["visits"][:, 0] = 1.0
    return rec


def test_ring_semantics():
    ring = CompactReplay(5, seed=9)
    assert ring.size() == 5 and ring.count() == 0
    # before anything is added every slot is the zero record
    assert ring.select(16).tobytes() == np.zeros(16, L.RECORD_DTYPE).tobytes()
    ring.add(_tagged(1, 4))
    assert ring.count() == 3
    got = ring.select(200)
    assert set(got["value"].tolist()) == {0.0, 1.0, 2.0, 3.0}           # added records, or the zero record of an unwritten slot
    ring.add(_tagged(4, 8))                                              # 7 added: wraps, 1 and 2 are overwritten
    assert ring.count() == 7 and ring.size() == 5
    got = ring.select(400)
    assert set(got["value"].tolist()) == {3.0, 4.0, 5.0, 6.0, 7.0}
    assert np.array_equal(got["actions"][:, 0], got["value"].astype(np.int16)) and N.validate_records(got) == 400
    ring.clear()
    assert ring.count() == 0 and set(ring.select(50)["value"].tolist()) == {0.0}


def test_ring_select_is_reproducible():
    picks = []
    for _ in range(2):
        ring = CompactReplay(64, seed=1234)
        ring.add(_tagged(0, 64))
        picks.append(ring.select(300)["value"].copy())
    assert np.array_equal(picks[0], picks[1])
    assert len(set(picks[0].tolist())) > 32                              # draws over the whole ring ...
    assert len(set(picks[0].tolist())) < 300                             # ... with replacement
    other = CompactReplay(64, seed=1235)
    other.add(_tagged(0, 64))
    assert not np.array_equal(other.select(300)["value"], picks[0])


def test_ring_add_bytes():
    ring = CompactReplay(8)
    payload = _tagged(0, 3).tobytes()
    assert ring.add_bytes(payload) == 3 and ring.add_bytes(b"") == 0 and ring.count() == 3
    with pytest.raises(ValueError):
        ring.add_bytes(payload[:-1])
    with pytest.raises(ValueError):
        ring.add_bytes(payload + b"\0")
    assert ring.count() == 3
    with pytest.raises(ValueError):
        CompactReplay(0)


def test_two_rank_gloo_compact_ring(tmp_path):
    port = 31000 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "_dist_records_worker.py"), str(tmp_path)]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    subprocess.run(cmd, check=True, timeout=300, env=env, capture_output=True)
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    # rank r contributed 3 + r records tagged 100 r + i: the root's ring holds both ranks', rank-major
    assert res[0]["count"] == 7 and res[0]["slots"] == [0, 1, 2, 100, 101, 102, 103]
    assert res[0]["added"] == [3, 4] and res[0]["valid"] == 7
    assert res[1]["count"] == 0 and res[1]["added"] == []
