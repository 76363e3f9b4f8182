"""Host-side mirror of the reference's evaluator class, over the C ABI.

`NN` keeps the method set and argument meaning of `kami::NN` (kami/nn/nn.h:40-73):
`NN(width, height, features, psize)`, `infer`, `read`, `write`, `get_generation`, `isCUDA`,
`obsize`, `polsize`, `clone`; the two option keys the reference's module reads
(`filters`, `residuals`, nn.cpp:42-43) are explicit constructor arguments here.
`infer` raises RuntimeError with the reference's messages on NaN outputs (nn.cpp:176-180).
The C++ twin used to drop into kami.cpp is kami_amd/host/nn.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from . import weights as W

PSIZE = 4672
NFEATURES = 30
OBSIZE = 8 * 8 * NFEATURES
VALUE_WIDTH = 256


class KamiError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(msg)
        self.status = status


def _chk(rc: int) -> None:
    if rc != L.KH_OK:
        raise KamiError(rc, L.last_error())


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _is_tensor(x) -> bool:
    """A torch.Tensor, without importing torch for callers that never pass one."""
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


def check_device_blob(t, nfloats: int, device: int) -> None:
    """What kh_load_weights_device needs of a tensor, checked before the C call: float32, contiguous, `nfloats` elements,
    in the memory of GPU `device`.  ValueError otherwise."""
    import torch
    if t.dtype != torch.float32:
        raise ValueError(f"device blob must be float32, not {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("device blob must be contiguous")
    if t.numel() != nfloats:
        raise ValueError(f"device blob has {t.numel()} floats, expected {nfloats}")
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError(f"device blob is on {t.device}, the engine on GPU {device}")


def read_checkpoint(path: str):
    """kh_checkpoint_read: -> (blob, features, filters, residuals, generation) of a checkpoint file — a libtorch
    archive written by the reference's NN::write (nn.cpp:189-202) or an engine KAMW blob.  Needs no GPU."""
    lib = L.load()
    F, Cc, R, gen, n = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    p = path.encode()
    _chk(lib.kh_checkpoint_read(p, C.byref(F), C.byref(Cc), C.byref(R), C.byref(gen), None, 0, C.byref(n)))
    blob = np.empty(n.value, np.float32)
    _chk(lib.kh_checkpoint_read(p, None, None, None, None, _ptr(blob), blob.size, None))
    return blob, F.value, Cc.value, R.value, gen.value


def read_bn_batches(path: str) -> int:
    """The BatchNorm num_batches_tracked counter a checkpoint holds (kh_checkpoint_read_ex): the first layer's for a
    libtorch archive, 0 for a KAMW blob.  Needs no GPU."""
    lib = L.load()
    nbt, n = C.c_int64(), C.c_size_t()
    _chk(lib.kh_checkpoint_read_ex(path.encode(), None, None, None, None, C.byref(nbt), None, 0, C.byref(n)))
    return nbt.value


def write_checkpoint(path: str, blob: np.ndarray, features: int, filters: int, residuals: int, generation: int,
                     bn_batches: int = 0) -> None:
    """kh_checkpoint_write: the blob as the reference's own checkpoint format (a libtorch archive that kami's
    NN::read, nn.cpp:204-222, and torch.jit.load open), every BatchNorm's num_batches_tracked = bn_batches.
    The file appears only once complete.  Needs no GPU."""
    lib = L.load()
    b = np.ascontiguousarray(blob, dtype=np.float32)
    _chk(lib.kh_checkpoint_write(path.encode(), features, filters, residuals, generation, bn_batches, _ptr(b), b.size))


def as_records(records) -> np.ndarray:
    """Records in any of the forms the record calls take -> a contiguous array of _lib.RECORD_DTYPE: a ctypes `Record`
    array (or a list of `Record`s), a `bytes` payload of whole records, or a NumPy structured / uint8 array of them."""
    if isinstance(records, np.ndarray):
        if records.dtype == L.RECORD_DTYPE:
            return np.ascontiguousarray(records).reshape(-1)
        raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    elif isinstance(records, (list, tuple)):
        raw = np.frombuffer(b"".join(bytes(r) for r in records), np.uint8)
    else:
        raw = np.frombuffer(records, np.uint8)         # bytes, bytearray, a ctypes array: anything with a buffer
    if raw.size % L.RECORD_DTYPE.itemsize:
        raise ValueError(f"{raw.size} bytes are not a whole number of {L.RECORD_DTYPE.itemsize}-byte records")
    return raw.view(L.RECORD_DTYPE)


def validate_records(records) -> int:
    """kh_records_validate: the number of records if every one is usable as a training sample (0 <= nact <= 96, actions
    in [0, 4672) and pairwise distinct); otherwise KamiError with `.bad_index` = the first offending record.  No GPU."""
    rec = as_records(records)
    bad = C.c_int(-1)
    rc = L.load().kh_records_validate(_ptr(rec), rec.size, C.byref(bad))
    if rc != L.KH_OK:
        err = KamiError(rc, L.last_error())
        err.bad_index = bad.value
        raise err
    return rec.size


class EvalResult:
    """What NN.eval_records / NN.eval_replay return (kh_eval_result): `records`, `policy_records` (those with nact > 0),
    `policy_loss` and `value_loss` (means over the records, in double), `top1` (share of policy_records whose most
    visited move is the network's most likely one among the record's moves), `generation` of the evaluated weights.
    With per_record=True also `record_policy_loss` / `record_value_loss`, float64 [records]; None otherwise."""
    FIELDS = ("records", "policy_records", "policy_loss", "value_loss", "top1", "generation")

    def __init__(self, res, record_policy_loss=None, record_value_loss=None):
        for f in self.FIELDS:
            setattr(self, f, getattr(res, f))
        self.record_policy_loss, self.record_value_loss = record_policy_loss, record_value_loss

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return "EvalResult(" + ", ".join(f"{f}={getattr(self, f)!r}" for f in self.FIELDS) + ")"


class Ticket:
    """An outstanding kh_submit_*: keeps the caller-side buffers alive until wait() (the engine reads and writes them)."""

    def __init__(self, nn, ticket, outputs, keep):
        self._nn, self._t, self._out, self._keep = nn, ticket, outputs, keep

    def wait(self):
        _chk(self._nn._lib.kh_wait(self._nn._h, self._t))
        return self._out

    def try_wait(self):
        """kh_try_wait: the outputs if the submission has finished (the ticket is consumed, as by wait()), else None."""
        done = C.c_int(0)
        _chk(self._nn._lib.kh_try_wait(self._nn._h, self._t, C.byref(done)))
        return self._out if done.value else None


# engines still open when the interpreter exits are closed while the HIP runtime is still up (module teardown order
# is arbitrary otherwise, and an engine owns streams, the queue's dispatcher thread and device memory)
import atexit
import weakref

_LIVE = weakref.WeakSet()


def _close_pools(nn=None):
    import sys
    search = sys.modules.get(__package__ + ".search")
    if search is not None:
        search.close_pools_of(nn)


@atexit.register
def _close_all():
    _close_pools()                      # pools first: they hold engine handles
    for nn in list(_LIVE):
        try:
            nn.close()
        except Exception:
            pass


class NN:
    def __init__(self, width: int = 8, height: int = 8, features: int = NFEATURES,
                 psize: int = PSIZE, *, filters: int = 256, residuals: int = 2,
                 dtype: str = "f32", value_mode: int = L.KH_VALUE_REFERENCE_FLAT,
                 device: int = 0):
        self._lib = L.load()
        self.cfg = L.Config(width=width, height=height, features=features, psize=psize,
                            filters=filters, residuals=residuals, dtype=L.DTYPES[dtype],
                            value_mode=value_mode, device=device)
        self.dtype = dtype
        self._h = C.c_void_p()
        _chk(self._lib.kh_create(C.byref(self.cfg), C.byref(self._h)))
        _LIVE.add(self)

    # -- kami::NN surface ---------------------------------------------------------------
    def get_generation(self) -> int:
        return self._lib.kh_generation(self._h)

    @staticmethod
    def _train_config(mlr, epochs, batchsize, detect_anomaly, momentum, nesterov, weight_decay, max_grad_norm):
        return L.TrainConfig(mlr / 1000.0, epochs, batchsize, 1 if detect_anomaly else 0,
                             momentum, weight_decay, max_grad_norm, 1 if nesterov else 0)

    def train(self, inputs: np.ndarray, obs_p: np.ndarray, obs_v: np.ndarray, *, mlr: int = 5, epochs: int = 8,
              batchsize: int = 8, detect_anomaly: bool = False, momentum: float = 0.0, nesterov: bool = False,
              weight_decay: float = 0.0, max_grad_norm: float = 0.0):
        """NN::train (nn.cpp:224-377) on the device; option names and defaults of nn.cpp:236-238.
        Returns (average loss of the first epoch, of the last epoch); the generation goes up by one.
        detect_anomaly (nn.cpp:231-232,329-344): every batch's input and the forward's two outputs are checked for NaN,
        and the call fails with the reference's messages.
        momentum / nesterov / weight_decay / max_grad_norm (all off by default: the reference's plain SGD): what
        clip_grad_norm_(params, max_grad_norm) followed by torch.optim.SGD(lr, momentum, 0, weight_decay, nesterov).step()
        does, with a velocity that lives for this call (kami_hip.h, kh_train_config); last_grad_norms() has the norms."""
        x = np.ascontiguousarray(inputs, dtype=np.float32)
        p = np.ascontiguousarray(obs_p, dtype=np.float32)
        v = np.ascontiguousarray(obs_v, dtype=np.float32)
        n = x.shape[0]
        assert p.shape == (n, PSIZE) and v.shape == (n,)
        cfg = self._train_config(mlr, epochs, batchsize, detect_anomaly, momentum, nesterov, weight_decay, max_grad_norm)
        first, last = C.c_float(), C.c_float()
        _chk(self._lib.kh_train(self._h, x.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                                v.ctypes.data_as(C.c_void_p), n, C.byref(cfg), C.byref(first), C.byref(last)))
        self._blob = self.get_weights()
        return first.value, last.value

    def train_records(self, records, *, mlr: int = 5, epochs: int = 8, batchsize: int = 8, detect_anomaly: bool = False,
                      momentum: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0, max_grad_norm: float = 0.0):
        """kh_train_records: train() on compact records (as_records: ctypes, bytes or NumPy), expanded per batch on the
        device — the same result as train(*expand_records(records)) with the same options, bit for bit, without the dense
        arrays."""
        rec = as_records(records)
        cfg = self._train_config(mlr, epochs, batchsize, detect_anomaly, momentum, nesterov, weight_decay, max_grad_norm)
        first, last = C.c_float(), C.c_float()
        _chk(self._lib.kh_train_records(self._h, _ptr(rec), rec.size, C.byref(cfg), C.byref(first), C.byref(last)))
        self._blob = self.get_weights()
        return first.value, last.value

    def train_replay(self, replay, n: int, *, mlr: int = 5, epochs: int = 8, batchsize: int = 8, detect_anomaly: bool = False,
                     momentum: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0, max_grad_norm: float = 0.0):
        """kh_train_replay: train_records(replay.select(n)) for a replay.DeviceReplay on this engine's GPU, bit for bit,
        with the records read where they lie in device memory: only the sample order is uploaded."""
        cfg = self._train_config(mlr, epochs, batchsize, detect_anomaly, momentum, nesterov, weight_decay, max_grad_norm)
        first, last = C.c_float(), C.c_float()
        _chk(self._lib.kh_train_replay(self._h, replay.handle, int(n), C.byref(cfg), C.byref(first), C.byref(last)))
        self._blob = self.get_weights()
        return first.value, last.value

    def eval_records(self, records, per_record: bool = False) -> "EvalResult":
        """kh_eval_records: the loss of the network AS SERVED (this engine's dtype, inference-mode BatchNorm) on compact
        records (as_records: ctypes, bytes or NumPy), computed on the device in double.  Changes nothing: weights,
        generation and bn_batches() stay.  -> EvalResult."""
        rec = as_records(records)
        return self._eval(rec.size, per_record, lambda res, lp, lv: self._lib.kh_eval_records(self._h, _ptr(rec), rec.size, res, lp, lv))

    def eval_replay(self, ring, first_slot: int = 0, n: Optional[int] = None, per_record: bool = False) -> "EvalResult":
        """kh_eval_replay: eval_records(ring.read(first_slot, n)) for a replay.DeviceReplay on this engine's GPU, bit for
        bit, with the records read where they lie; no draw is made.  n=None: the written slots, min(count, size) — an
        empty ring raises ValueError."""
        if n is None:
            n = min(ring.count(), ring.size())
            if n == 0:
                raise ValueError("eval_replay on an empty ring")
        n = int(n)
        return self._eval(n, per_record,
                          lambda res, lp, lv: self._lib.kh_eval_replay(self._h, ring.handle, int(first_slot), n, res, lp, lv))

    def _eval(self, n, per_record, call) -> "EvalResult":
        res = L.EvalResult()
        lp = np.zeros(max(n, 0), np.float64) if per_record else None
        lv = np.zeros(max(n, 0), np.float64) if per_record else None
        _chk(call(C.byref(res), _ptr(lp) if per_record else None, _ptr(lv) if per_record else None))
        return EvalResult(res, lp, lv)

    def last_grad_norms(self) -> np.ndarray:
        """kh_train_grad_norms: the gradient norm before clipping of every step of the last completed train() /
        train_records() call that ran with max_grad_norm > 0, in step order (empty if it did not clip)."""
        steps = C.c_int(0)
        _chk(self._lib.kh_train_grad_norms(self._h, None, 0, C.byref(steps)))
        out = np.empty(steps.value, np.float32)
        if steps.value:
            _chk(self._lib.kh_train_grad_norms(self._h, _ptr(out), out.size, C.byref(steps)))
        return out[:steps.value]

    def expand_records(self, records):
        """kh_expand_records: -> (planes [n,8,8,30], obs_p [n,4672], obs_v [n]), the dense arrays train() takes."""
        rec = as_records(records)
        n = rec.size
        planes = np.empty((n, 8, 8, NFEATURES), np.float32)
        obs_p = np.empty((n, PSIZE), np.float32)
        obs_v = np.empty((n,), np.float32)
        _chk(self._lib.kh_expand_records(self._h, _ptr(rec), n, _ptr(planes), _ptr(obs_p), _ptr(obs_v)))
        return planes, obs_p, obs_v

    def get_weights(self) -> np.ndarray:
        """The engine's current fp32 parameters in blob order (kh_get_weights)."""
        n = self._lib.kh_weight_count(self.cfg.features, self.cfg.filters, self.cfg.residuals)
        out = np.empty(n, np.float32)
        _chk(self._lib.kh_get_weights(self._h, _ptr(out), n))
        return out

    def isCUDA(self) -> bool:            # nn.h:62 — true: the engine only exists on the GPU
        return True

    def obsize(self) -> int:
        return self.cfg.width * self.cfg.height * self.cfg.features

    def polsize(self) -> int:
        return self.cfg.psize

    def infer(self, input: np.ndarray, batch: Optional[int] = None,
              policy: Optional[np.ndarray] = None, value: Optional[np.ndarray] = None):
        """nn.cpp:155-187.  input [batch,8,8,F] fp32 -> (policy [batch,4672], value [batch])."""
        x = np.ascontiguousarray(input, dtype=np.float32)
        if batch is None:
            batch = x.size // self.obsize()
        if x.size != batch * self.obsize():
            raise ValueError("input size does not match batch * obsize()")
        if policy is None:
            policy = np.empty((batch, PSIZE), np.float32)
        if value is None:
            value = np.empty((batch,), np.float32)
        _chk(self._lib.kh_infer(self._h, _ptr(x), batch, _ptr(policy), _ptr(value)))
        return policy, value

    def read(self, path: str) -> None:
        """NN::read (nn.cpp:204-222): the reference's own libtorch archives and the engine's KAMW blobs.  An archive's
        BatchNorm batch counter comes along (bn_batches())."""
        blob, F, Cc, R, gen = read_checkpoint(path)
        if (F, Cc, R) != (self.cfg.features, self.cfg.filters, self.cfg.residuals):
            raise KamiError(L.KH_ERR_INVALID, "checkpoint shape does not match this NN")
        _chk(self._lib.kh_load_checkpoint(self._h, path.encode()))
        self._blob = blob

    def write(self, path: str, format: str = "kamw") -> None:
        """NN::write (nn.cpp:189-202).  format="kamw" (the default): the engine's KAMW container; format="torch": the
        reference's own libtorch archive (kh_write_checkpoint), which a stock kami reads.  read() takes both back."""
        if format == "torch":
            _chk(self._lib.kh_write_checkpoint(self._h, path.encode()))
        elif format == "kamw":
            W.save(path, self.get_weights(), self.cfg.features, self.cfg.filters, self.cfg.residuals, self.get_generation())
        else:
            raise ValueError(f"format must be 'kamw' or 'torch', not {format!r}")

    def bn_batches(self) -> int:
        """kh_bn_batches: the reference's BatchNorm num_batches_tracked for the current weights (training-mode forwards
        so far; from the archive after read(), 0 after load_weights())."""
        v = C.c_int64()
        _chk(self._lib.kh_bn_batches(self._h, C.byref(v)))
        return v.value

    def clone(self) -> "NN":
        other = object.__new__(NN)
        other._lib, other.cfg, other.dtype = self._lib, self.cfg, self.dtype
        other._blob = self._blob
        other._h = C.c_void_p()
        _chk(self._lib.kh_clone(self._h, C.byref(other._h)))
        _LIVE.add(other)
        return other

    # -- engine extras ------------------------------------------------------------------
    _blob: Optional[np.ndarray] = None

    def load_weights(self, blob, generation: int = 0) -> None:
        """kh_load_weights from anything NumPy takes or a CPU torch.Tensor; a CUDA torch.Tensor (float32, contiguous,
        kh_weight_count elements, on the engine's device: anything else raises ValueError) is installed where it is, by
        kh_load_weights_device on torch's current stream — same bits either way."""
        if _is_tensor(blob):
            if blob.is_cuda:
                check_device_blob(blob, self._lib.kh_weight_count(self.cfg.features, self.cfg.filters, self.cfg.residuals),
                                  self.cfg.device)
                import torch
                stream = torch.cuda.current_stream(blob.device)
                if not stream.cuda_stream:         # the legacy default stream has no handle to order behind: drain it
                    stream.synchronize()
                _chk(self._lib.kh_load_weights_device(self._h, C.c_void_p(blob.data_ptr()), blob.numel(), generation,
                                                      C.c_void_p(stream.cuda_stream)))
                self._blob = None                  # (get_weights() has the host copy)
                return
            blob = blob.detach().numpy()
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        _chk(self._lib.kh_load_weights(self._h, _ptr(blob), blob.size, generation))
        self._blob = blob

    def infer_full(self, input: np.ndarray, want_logits: bool = True):
        """-> (policy [B,4672], value_full [B,256], logits [B,4672] or None)"""
        x = np.ascontiguousarray(input, dtype=np.float32)
        batch = x.size // self.obsize()
        policy = np.empty((batch, PSIZE), np.float32)
        vfull = np.empty((batch, VALUE_WIDTH), np.float32)
        logits = np.empty((batch, PSIZE), np.float32) if want_logits else None
        _chk(self._lib.kh_infer_full(self._h, _ptr(x), batch, _ptr(policy), _ptr(vfull),
                                     _ptr(logits) if want_logits else None))
        return policy, vfull, logits

    def encode(self, boards: np.ndarray) -> np.ndarray:
        """Env::observe (env.h:202-262) for kh_board records -> [n,8,8,30] fp32."""
        b = np.ascontiguousarray(boards, dtype=L.BOARD_DTYPE)
        out = np.empty((b.shape[0], 8, 8, NFEATURES), np.float32)
        _chk(self._lib.kh_encode(self._h, _ptr(b), b.shape[0], _ptr(out)))
        return out

    def encode_infer(self, boards: np.ndarray):
        b = np.ascontiguousarray(boards, dtype=L.BOARD_DTYPE)
        n = b.shape[0]
        policy = np.empty((n, PSIZE), np.float32)
        value = np.empty((n,), np.float32)
        _chk(self._lib.kh_encode_infer(self._h, _ptr(b), n, _ptr(policy), _ptr(value)))
        return policy, value

    def infer_legal(self, input_or_boards: np.ndarray, action_offsets: np.ndarray, actions: np.ndarray):
        """Legal-move policy gather (MCTS::expand, mcts.h:273-276): -> (priors [sum of counts], value [B]).
        `input_or_boards` is either fp32 planes [B,8,8,F] or kh_board records."""
        offs = np.ascontiguousarray(action_offsets, dtype=np.int32)
        acts = np.ascontiguousarray(actions, dtype=np.int32)
        n = offs.size - 1
        priors = np.empty((int(offs[-1]),), np.float32)
        value = np.empty((n,), np.float32)
        if input_or_boards.dtype == L.BOARD_DTYPE:
            b = np.ascontiguousarray(input_or_boards)
            _chk(self._lib.kh_encode_infer_legal(self._h, _ptr(b), n, _ptr(offs), _ptr(acts), _ptr(priors), _ptr(value)))
        else:
            x = np.ascontiguousarray(input_or_boards, dtype=np.float32)
            _chk(self._lib.kh_infer_legal(self._h, _ptr(x), n, _ptr(offs), _ptr(acts), _ptr(priors), _ptr(value)))
        return priors, value

    # -- submit / wait (the engine's coalescing queue) -------------------------------------
    def submit_infer(self, input: np.ndarray) -> "Ticket":
        """kh_submit_infer: queue a small batch of planes; Ticket.wait() -> (policy, value).  Submissions queued while a
        launch is in flight are evaluated as one launch."""
        x = np.ascontiguousarray(input, dtype=np.float32)
        batch = x.size // self.obsize()
        policy = np.empty((batch, PSIZE), np.float32)
        value = np.empty((batch,), np.float32)
        t = C.c_int64()
        _chk(self._lib.kh_submit_infer(self._h, _ptr(x), batch, _ptr(policy), _ptr(value), C.byref(t)))
        return Ticket(self, t.value, (policy, value), (x,))

    def submit_infer_legal(self, boards: np.ndarray, action_offsets: np.ndarray, actions: np.ndarray) -> "Ticket":
        """kh_submit_encode_infer_legal; Ticket.wait() -> (priors, value)."""
        b = np.ascontiguousarray(boards, dtype=L.BOARD_DTYPE)
        offs = np.ascontiguousarray(action_offsets, dtype=np.int32)
        acts = np.ascontiguousarray(actions, dtype=np.int32)
        n = offs.size - 1
        priors = np.empty((max(1, int(offs[-1])),), np.float32)
        value = np.empty((n,), np.float32)
        t = C.c_int64()
        _chk(self._lib.kh_submit_encode_infer_legal(self._h, _ptr(b), n, _ptr(offs), _ptr(acts), _ptr(priors), _ptr(value), C.byref(t)))
        return Ticket(self, t.value, (priors[:int(offs[-1])], value), (b, offs, acts, priors))

    def pin(self, array: np.ndarray) -> None:
        """kh_pin_buffer: register a long-lived numpy buffer used as infer()'s input / policy (unpin before freeing it)."""
        _chk(self._lib.kh_pin_buffer(self._h, _ptr(array), array.nbytes))

    def unpin(self, array: np.ndarray) -> None:
        _chk(self._lib.kh_unpin_buffer(self._h, _ptr(array)))

    def set_coalesce(self, target_batch: int = 0, max_wait_us: int = 0) -> None:
        _chk(self._lib.kh_set_coalesce(self._h, target_batch, max_wait_us))


    def set_coalesce_callers(self, callers: int):
        """With a target set: a batch also goes once it holds `callers` submissions (0: off)."""
        _chk(self._lib.kh_set_coalesce_callers(self._h, callers))

    def coalesce_stats(self):
        """(launches made by the queue, positions they held)"""
        a, b = C.c_int64(), C.c_int64()
        _chk(self._lib.kh_coalesce_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _close_pools(self)          # a self-play pool on this engine is closed with it
            self._lib.kh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
