"""Replay records: the reference's in-process ring (kami/replaybuffer.h:10-92) and its multi-GPU
merge.  A record is (observation[obsize], mcts policy[psize], result) in fp32 — 26 372 bytes at
F = 30.  `add` / `select_batch` / `count` / `size` / `clear` keep the reference's meaning
(uniform selection WITH replacement over the whole ring, replaybuffer.h:61-84, including slots
not yet written — they read as zeros here where the reference reads uninitialised memory).

`gather` is new (the reference is single-process): every rank contributes the records it added
since the last gather; they are gathered to the root and merged into its ring in rank-major order (the reference's
insertion order is thread-racy, so any fixed order is acceptable — SURVEY §8e).  It runs over
torch.distributed: RCCL/xGMI with device tensors on GPUs, gloo on CPU.  Never on the timed
evaluation path.
"""
from __future__ import annotations

import numpy as np


class ReplayBuffer:
    def __init__(self, obsize: int, psize: int, bufsize: int, seed: int | None = None):
        self.obsize, self.psize, self.bufsize = obsize, psize, bufsize
        self.input_buffer = np.zeros((bufsize, obsize), np.float32)
        self.mcts_buffer = np.zeros((bufsize, psize), np.float32)
        self.result_buffer = np.zeros((bufsize,), np.float32)
        self.write_index = 0
        self.total = 0
        self._fresh = []                 # ring slots written since the last gather
        self._rng = np.random.default_rng(seed)

    def clear(self) -> None:             # replaybuffer.h:31-34
        self.total = 0
        self.write_index = 0
        self._fresh = []

    def add(self, inp, mcts, result: float) -> None:      # replaybuffer.h:36-56
        i = self.write_index
        self.input_buffer[i] = inp
        self.mcts_buffer[i] = mcts
        self.result_buffer[i] = result
        self._fresh.append(i)
        self.write_index = (i + 1) % self.bufsize
        self.total += 1

    def size(self) -> int:
        return self.bufsize

    def count(self) -> int:
        return self.total

    def select_batch(self, n: int):      # replaybuffer.h:61-84
        src = self._rng.integers(0, self.bufsize, n)
        return self.input_buffer[src].copy(), self.mcts_buffer[src].copy(), self.result_buffer[src].copy()

    # ---- multi-GPU merge ---------------------------------------------------------------
    def _pack_fresh(self) -> np.ndarray:
        idx = np.asarray(self._fresh[-self.bufsize:], dtype=np.int64)
        rec = np.empty((len(idx), self.obsize + self.psize + 1), np.float32)
        rec[:, :self.obsize] = self.input_buffer[idx]
        rec[:, self.obsize:self.obsize + self.psize] = self.mcts_buffer[idx]
        rec[:, -1] = self.result_buffer[idx]
        return rec

    def gather(self, dist, root: int = 0, device: str | None = None) -> int:
        """Merge every rank's fresh records into `root`'s ring.  Returns how many records the
        root inserted (0 on the other ranks)."""
        import torch
        mine = self._pack_fresh()
        self._fresh = []
        if dist is None:
            return 0
        from .dist import collective_device
        device = device or collective_device(dist)
        world, rank = dist.get_world_size(), dist.get_rank()
        counts = torch.zeros(world, dtype=torch.int64, device=device)
        counts[rank] = mine.shape[0]
        dist.all_reduce(counts)
        width = self.obsize + self.psize + 1
        nmax = int(counts.max().item())
        if nmax == 0:
            return 0
        pad = torch.zeros((nmax, width), dtype=torch.float32, device=device)
        pad[:mine.shape[0]] = torch.from_numpy(mine).to(device)
        # gather TO THE ROOT (only the trainer rank consumes the records: an all-gather would move world x the bytes,
        # which matters at 26 KB per dense row); fixed shapes, one collective
        outs = [torch.empty_like(pad) for _ in range(world)] if rank == root else None
        dist.gather(pad, gather_list=outs, dst=root)
        inserted = 0
        if rank == root:
            for r in range(world):
                if r == root:
                    continue            # the root's own records are already in its ring
                recs = outs[r][:int(counts[r].item())].cpu().numpy()
                for rec in recs:
                    self.add(rec[:self.obsize], rec[self.obsize:self.obsize + self.psize], float(rec[-1]))
                    inserted += 1
            self._fresh = []
        return inserted


class CompactReplay:
    """The same ring over compact records (kh_record, 664 bytes instead of 26 372): libkamisearch.so's ks_ring_*,
    the one implementation the C++ host uses too.  `select(n)` returns `n` uniform draws with replacement over the whole
    ring (a never-written slot is the all-zero record, a valid sample) as a NumPy record array — what
    NN.train_records takes.  `seed` makes the draws repeatable."""

    def __init__(self, bufsize: int, seed: int = 0):
        from . import search as S
        from . import _lib as L
        self._S, self._dtype = S, L.RECORD_DTYPE
        self.lib = S.load()
        self.h = self.lib.ks_ring_new(int(bufsize), int(seed) & (2 ** 64 - 1))
        if not self.h:
            raise ValueError(self.lib.ks_last_error().decode())

    def add(self, records) -> int:
        """Records in any form NN.train_records takes; returns how many went in."""
        from .nn import as_records
        rec = as_records(records)
        if self.lib.ks_ring_add(self.h, rec.ctypes.data, rec.size):
            raise ValueError(self.lib.ks_last_error().decode())
        return rec.size

    def add_bytes(self, payload: bytes) -> int:
        """A payload of whole records, as gather_compact returns them per rank."""
        if len(payload) % self._dtype.itemsize:
            raise ValueError(f"{len(payload)} bytes are not a whole number of {self._dtype.itemsize}-byte records")
        return self.add(payload) if payload else 0

    def size(self) -> int:
        return self.lib.ks_ring_size(self.h)

    def count(self) -> int:
        return self.lib.ks_ring_count(self.h)

    def clear(self) -> None:
        self.lib.ks_ring_clear(self.h)

    def select(self, n: int) -> np.ndarray:
        out = np.zeros(int(n), self._dtype)
        if self.lib.ks_ring_select(self.h, int(n), out.ctypes.data):
            raise ValueError(self.lib.ks_last_error().decode())
        return out

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.ks_ring_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class DeviceReplay:
    """CompactReplay with the ring in device memory (kh_replay_*), on the GPU of the engine `nn`: the same slots, the
    same draws for the same seed and calls, records validated as they are added (a failed add raises KamiError with
    kh_records_validate's message and `.bad_index`, and changes nothing).  `add_tensor` takes records that are already
    in device memory — the root's end of an RCCL gather — and `nn.train_replay(ring, n)` trains from the ring in place.
    The ring outlives `nn`; any engine with features == 30 on that GPU may train from it."""

    def __init__(self, nn, bufsize: int, seed: int = 0):
        import ctypes as C
        from . import _lib as L
        from .nn import KamiError
        self._C, self._L, self._err, self._dtype = C, L, KamiError, L.RECORD_DTYPE
        self.lib = L.load()
        self.device = nn.cfg.device
        self.handle = C.c_void_p()
        self._chk(self.lib.kh_replay_create(nn.handle, int(bufsize), int(seed) & (2 ** 64 - 1), C.byref(self.handle)))
        _LIVE_RINGS.add(self)

    def _chk(self, rc: int, bad=None) -> None:
        if rc != self._L.KH_OK:
            err = self._err(rc, self._L.last_error())
            if bad is not None:
                err.bad_index = bad.value
            raise err

    def add(self, records) -> int:
        """Records in any form NN.train_records takes; returns how many went in."""
        from .nn import as_records
        rec = as_records(records)
        bad = self._C.c_int(-1)
        self._chk(self.lib.kh_replay_add(self.handle, rec.ctypes.data, rec.size, self._C.byref(bad)), bad)
        return rec.size

    def add_bytes(self, payload: bytes) -> int:
        """A payload of whole records, as gather_compact returns them per rank."""
        if len(payload) % self._dtype.itemsize:
            raise ValueError(f"{len(payload)} bytes are not a whole number of {self._dtype.itemsize}-byte records")
        return self.add(payload) if payload else 0

    def add_tensor(self, t) -> int:
        """Whole records in a contiguous uint8 CUDA tensor on the ring's GPU (anything else: ValueError), added where
        they lie by kh_replay_add_device on torch's current stream."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"device records must be a uint8 tensor, not {getattr(t, 'dtype', type(t))}")
        if not t.is_contiguous():
            raise ValueError("device records must be contiguous")
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"device records are on {t.device}, the ring on GPU {self.device}")
        if t.numel() % self._dtype.itemsize:
            raise ValueError(f"{t.numel()} bytes are not a whole number of {self._dtype.itemsize}-byte records")
        n = t.numel() // self._dtype.itemsize
        if n == 0:
            return 0
        stream = torch.cuda.current_stream(t.device)
        if not stream.cuda_stream:             # the legacy default stream has no handle to order behind: drain it
            stream.synchronize()
        bad = self._C.c_int(-1)
        self._chk(self.lib.kh_replay_add_device(self.handle, self._C.c_void_p(t.data_ptr()), n, self._C.c_void_p(stream.cuda_stream),
                                                self._C.byref(bad)), bad)
        return n

    def size(self) -> int:
        return self.lib.kh_replay_size(self.handle)

    def count(self) -> int:
        return self.lib.kh_replay_count(self.handle)

    def clear(self) -> None:
        self._chk(self.lib.kh_replay_clear(self.handle))

    def read(self, first_slot: int, n: int) -> np.ndarray:
        """Slots first_slot .. first_slot + n - 1 (mod the capacity) as a NumPy record array; no draw is made."""
        out = np.zeros(int(n), self._dtype)
        self._chk(self.lib.kh_replay_read(self.handle, int(first_slot), int(n), out.ctypes.data))
        return out

    def select(self, n: int) -> np.ndarray:
        out = np.zeros(int(n), self._dtype)
        self._chk(self.lib.kh_replay_select(self.handle, int(n), out.ctypes.data))
        return out

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.kh_replay_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# rings still open when the interpreter exits are freed while the HIP runtime is still up (as nn.py does for engines)
import atexit
import weakref

_LIVE_RINGS = weakref.WeakSet()


@atexit.register
def _close_rings():
    for ring in list(_LIVE_RINGS):
        try:
            ring.close()
        except Exception:
            pass


def gather_compact(dist, payload: bytes, record_bytes: int, root: int = 0, device: str | None = None, as_tensor: bool = False):
    """Merge fixed-size compact records (ks_record, 664 bytes: board + sparse visit distribution + value —
    include/kami_search.h) over the ranks: 40x less traffic than the dense 26 372-byte rows `gather` moves.
    Every rank passes its own records; returns the list of every rank's payload (rank-major) on `root`, and
    [] elsewhere.  One size all-reduce + one gather of uint8 to the root (RCCL over xGMI with device tensors: the
    root's seven direct links carry one rank's payload each; gloo on CPU).
    as_tensor=True: the payloads as uint8 tensors, outs[r][:count], where the collective left them — device memory under
    RCCL (what DeviceReplay.add_tensor takes: the records never visit the host), CPU tensors under gloo or without a
    group."""
    import torch
    if dist is None:
        if not as_tensor:
            return [payload]
        return [torch.frombuffer(bytearray(payload), dtype=torch.uint8) if payload else torch.zeros(0, dtype=torch.uint8)]
    from .dist import collective_device
    device = device or collective_device(dist)
    world, rank = dist.get_world_size(), dist.get_rank()
    assert len(payload) % record_bytes == 0
    counts = torch.zeros(world, dtype=torch.int64, device=device)
    counts[rank] = len(payload)
    dist.all_reduce(counts)
    nmax = int(counts.max().item())
    if nmax == 0:
        if rank != root:
            return []
        return [torch.zeros(0, dtype=torch.uint8, device=device) for _ in range(world)] if as_tensor else [b""] * world
    pad = torch.zeros(nmax, dtype=torch.uint8, device=device)
    if payload:
        pad[:len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(device)
    outs = [torch.empty_like(pad) for _ in range(world)] if rank == root else None
    dist.gather(pad, gather_list=outs, dst=root)
    if rank != root:
        return []
    if as_tensor:
        return [outs[r][:int(counts[r].item())] for r in range(world)]
    return [outs[r][:int(counts[r].item())].cpu().numpy().tobytes() for r in range(world)]
