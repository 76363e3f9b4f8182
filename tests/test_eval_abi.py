"""kh_eval_* without a GPU: the result struct's layout, the argument checks that need no engine, the hold-out split of
cycle.generation (cycle.split_holdout) and generation()'s own argument checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kami_amd import _lib as L
from kami_amd import cycle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = L.RECORD_DTYPE.itemsize


def test_result_struct_is_64_bytes_on_both_sides(tmp_path):
    assert C.sizeof(L.EvalResult) == 64 and L.EVAL_DTYPE.itemsize == 64
    offsets = {name: getattr(L.EvalResult, name).offset for name, _ in L.EvalResult._fields_}
    assert offsets == {"records": 0, "policy_records": 8, "policy_loss": 16, "value_loss": 24, "top1": 32, "generation": 40,
                       "reserved": 44}
    assert {k: v[1] for k, v in L.EVAL_DTYPE.fields.items()} == offsets
    # the C side, from the header itself
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "kami_hip.h"\n'
                   "_Static_assert(sizeof(kh_eval_result) == 64, \"size\");\n"
                   "_Static_assert(offsetof(kh_eval_result, policy_loss) == 16 && offsetof(kh_eval_result, top1) == 32 &&\n"
                   "               offsetof(kh_eval_result, generation) == 40 && offsetof(kh_eval_result, reserved) == 44, \"offsets\");\n"
                   f"_Static_assert(KH_EVAL_CHUNK == {L.EVAL_CHUNK}, \"chunk\");\n")
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")
    assert cc, "no C compiler (the build needs one)"
    r = subprocess.run([cc, "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_arguments_are_invalid():
    lib = L.load()
    res = L.EvalResult()
    rec = np.zeros(1, L.RECORD_DTYPE)
    assert lib.kh_eval_records(None, rec.ctypes.data, 1, C.byref(res), None, None) == L.KH_ERR_INVALID
    assert "null" in L.last_error()
    assert lib.kh_eval_replay(None, None, 0, 1, C.byref(res), None, None) == L.KH_ERR_INVALID
    assert "null" in L.last_error()
    assert res.records == 0


def payload(k):
    """k records whose first four bytes hold their index"""
    raw = np.zeros((k, SIZE), np.uint8)
    raw[:, :4] = np.arange(k, dtype="<u4").view(np.uint8).reshape(k, 4)
    raw[:, 4:] = (np.arange(k)[:, None] * 7 + np.arange(SIZE - 4)[None, :]) % 251
    return raw.tobytes()


@pytest.mark.parametrize("k", [0, 1, 3, 200])
@pytest.mark.parametrize("pct", [1, 25, 50])
def test_split_holdout_bytes(k, pct):
    p = payload(k)
    train, held = cycle.split_holdout(p, SIZE, pct)
    assert isinstance(train, bytes) and isinstance(held, bytes)
    assert len(train) % SIZE == 0 and len(held) % SIZE == 0
    assert len(held) // SIZE == k * pct // 100                    # the tail rule
    assert train + held == p
    if held:
        first = int(np.frombuffer(held[:4], "<u4")[0])
        assert first == k - k * pct // 100                         # ... and it is the LAST records that are held


def test_split_holdout_rejects_partial_records_and_bad_pct():
    with pytest.raises(ValueError):
        cycle.split_holdout(payload(3)[:-1], SIZE, 25)
    with pytest.raises(ValueError):
        cycle.split_holdout(payload(3) + b"\0", SIZE, 25)
    for pct in (-1, 51, 100):
        with pytest.raises(ValueError):
            cycle.split_holdout(payload(3), SIZE, pct)


def test_split_holdout_slices_a_tensor_where_it_lies():
    import torch
    p = payload(9)
    t = torch.frombuffer(bytearray(p), dtype=torch.uint8)
    train, held = cycle.split_holdout(t, SIZE, 34)                 # 9 * 34 // 100 = 3
    assert train.numel() == 6 * SIZE and held.numel() == 3 * SIZE
    assert train.data_ptr() == t.data_ptr() and held.data_ptr() == t.data_ptr() + 6 * SIZE      # views, not copies
    assert held.is_contiguous() and bytes(held.numpy()) == p[6 * SIZE:]
    with pytest.raises(ValueError):
        cycle.split_holdout(t[:-1], SIZE, 34)


class NeverPlayed:
    """A pool that must not be reached: generation() judges its hold-out arguments first."""

    def __getattr__(self, name):
        raise AssertionError(f"generation() touched the pool ({name}) before rejecting its arguments")


@pytest.mark.parametrize("kw", [dict(holdout=object(), holdout_pct=25), dict(holdout=None, holdout_pct=25),
                                dict(holdout=b"ring", holdout_pct=10)])
def test_generation_rejects_a_holdout_that_is_no_device_ring(kw):
    with pytest.raises(ValueError, match="DeviceReplay"):
        cycle.generation(NeverPlayed(), NeverPlayed(), None, play_evals=1, **kw)


@pytest.mark.parametrize("pct", [0, -1, 51, 100, 2.5])
def test_generation_rejects_a_holdout_pct_out_of_range(pct):
    from kami_amd.replay import DeviceReplay
    ring = object.__new__(DeviceReplay)                            # no engine behind it: never used
    ring.handle = None
    with pytest.raises(ValueError, match="holdout_pct"):
        cycle.generation(NeverPlayed(), NeverPlayed(), None, play_evals=1, holdout=ring, holdout_pct=pct)
