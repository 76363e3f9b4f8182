"""ctypes loader for libkamihip.so — the C ABI declared in include/kami_hip.h."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libkamihip.so")

KH_OK, KH_ERR_INVALID, KH_ERR_HIP, KH_ERR_NO_WEIGHTS = 0, 1, 2, 3
KH_ERR_NAN_POLICY, KH_ERR_NAN_VALUE, KH_ERR_NO_DEVICE = 4, 5, 6
KH_F32, KH_BF16, KH_F16 = 0, 1, 2
KH_VALUE_REFERENCE_FLAT, KH_VALUE_PER_SAMPLE0 = 0, 1
KH_MAX_OUTSTANDING = 64
DTYPES = {"f32": KH_F32, "fp32": KH_F32, "bf16": KH_BF16, "f16": KH_F16, "fp16": KH_F16}


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("features", C.c_int32),
                ("psize", C.c_int32), ("filters", C.c_int32), ("residuals", C.c_int32),
                ("dtype", C.c_int32), ("value_mode", C.c_int32), ("device", C.c_int32),
                ("reserved", C.c_int32 * 7)]


# numpy view of kh_board (80 bytes)
BOARD_DTYPE = np.dtype([("piece_occ", "<u8", (6,)), ("color_occ", "<u8", (2,)),
                        ("ply", "<i4"), ("halfmove_clock", "<i4"),
                        ("ctm", "u1"), ("castle_rights", "u1"), ("pad", "u1", (6,))])
assert BOARD_DTYPE.itemsize == 80

class Board(C.Structure):
    """kh_board; same bytes as BOARD_DTYPE."""
    _fields_ = [("piece_occ", C.c_uint64 * 6), ("color_occ", C.c_uint64 * 2), ("ply", C.c_int32), ("halfmove_clock", C.c_int32),
                ("ctm", C.c_uint8), ("castle_rights", C.c_uint8), ("pad", C.c_uint8 * 6)]


MAX_RECORD_ACTIONS = 96


class Record(C.Structure):
    """kh_record (664 bytes): one finished-game position as self-play produces it and kh_train_records consumes it."""
    _fields_ = [("board", Board), ("value", C.c_float), ("nact", C.c_int32),
                ("actions", C.c_int16 * MAX_RECORD_ACTIONS), ("visits", C.c_float * MAX_RECORD_ACTIONS)]


# numpy view of kh_record
RECORD_DTYPE = np.dtype([("board", BOARD_DTYPE), ("value", "<f4"), ("nact", "<i4"),
                         ("actions", "<i2", (MAX_RECORD_ACTIONS,)), ("visits", "<f4", (MAX_RECORD_ACTIONS,))])
assert C.sizeof(Board) == 80 and C.sizeof(Record) == 664 and RECORD_DTYPE.itemsize == 664

# every symbol include/kami_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
class TrainConfig(C.Structure):
    """kh_train_config (32 bytes); the optimizer fields default to 0 = the reference's plain SGD."""
    _fields_ = [("lr", C.c_float), ("epochs", C.c_int32), ("batch", C.c_int32), ("detect_anomaly", C.c_int32),
                ("momentum", C.c_float), ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("nesterov", C.c_int32)]


class EvalResult(C.Structure):
    """kh_eval_result (64 bytes): what kh_eval_records / kh_eval_replay report."""
    _fields_ = [("records", C.c_int64), ("policy_records", C.c_int64), ("policy_loss", C.c_double), ("value_loss", C.c_double),
                ("top1", C.c_double), ("generation", C.c_int32), ("reserved", C.c_int32 * 5)]


# numpy view of kh_eval_result
EVAL_DTYPE = np.dtype([("records", "<i8"), ("policy_records", "<i8"), ("policy_loss", "<f8"), ("value_loss", "<f8"),
                       ("top1", "<f8"), ("generation", "<i4"), ("reserved", "<i4", (5,))])
EVAL_CHUNK = 1024        # KH_EVAL_CHUNK
assert C.sizeof(EvalResult) == 64 and EVAL_DTYPE.itemsize == 64


SYMBOLS = {
    "kh_weight_count": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "kh_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "kh_destroy": (None, [_P]),
    "kh_load_weights": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "kh_load_weights_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "kh_train": (C.c_int, [_P, _P, _P, _P, C.c_int, C.POINTER(TrainConfig), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "kh_train_config_check": (C.c_int, [C.POINTER(TrainConfig)]),
    "kh_train_grad_norms": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "kh_train_order": (C.c_int, [C.c_int, C.c_int, _P]),
    "kh_train_conv_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kh_records_validate": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "kh_expand_records": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "kh_train_records": (C.c_int, [_P, _P, C.c_int, C.POINTER(TrainConfig), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "kh_replay_create": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "kh_replay_destroy": (None, [_P]),
    "kh_replay_add": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "kh_replay_add_device": (C.c_int, [_P, _P, C.c_int, _P, C.POINTER(C.c_int)]),
    "kh_replay_count": (C.c_int64, [_P]),
    "kh_replay_size": (C.c_int, [_P]),
    "kh_replay_clear": (C.c_int, [_P]),
    "kh_replay_read": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "kh_replay_select": (C.c_int, [_P, C.c_int, _P]),
    "kh_train_replay": (C.c_int, [_P, _P, C.c_int, C.POINTER(TrainConfig), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "kh_eval_records": (C.c_int, [_P, _P, C.c_int, C.POINTER(EvalResult), _P, _P]),
    "kh_eval_replay": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(EvalResult), _P, _P]),
    "kh_checkpoint_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kh_checkpoint_read_ex": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int64), _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kh_load_checkpoint": (C.c_int, [_P, C.c_char_p]),
    "kh_checkpoint_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_size_t]),
    "kh_write_checkpoint": (C.c_int, [_P, C.c_char_p]),
    "kh_bn_batches": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "kh_get_weights": (C.c_int, [_P, _P, C.c_size_t]),
    "kh_generation": (C.c_int, [_P]),
    "kh_clone": (C.c_int, [_P, C.POINTER(_P)]),
    "kh_infer": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "kh_pin_buffer": (C.c_int, [_P, _P, C.c_size_t]),
    "kh_unpin_buffer": (C.c_int, [_P, _P]),
    "kh_infer_full": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "kh_encode": (C.c_int, [_P, _P, C.c_int, _P]),
    "kh_encode_infer": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "kh_infer_legal": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    "kh_encode_infer_legal": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P]),
    "kh_submit_infer": (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    "kh_submit_encode_infer_legal": (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "kh_wait": (C.c_int, [_P, C.c_int64]),
    "kh_try_wait": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_int)]),
    "kh_set_coalesce": (C.c_int, [_P, C.c_int, C.c_int]),
    "kh_set_coalesce_callers": (C.c_int, [_P, C.c_int]),
    "kh_coalesce_stats": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "kh_infer_device": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "kh_encode_device": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "kh_encode_infer_device": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "kh_time_infer_device": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_float)]),
    "kh_time_encode_device": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.POINTER(C.c_float)]),
    "kh_dev_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "kh_dev_free": (C.c_int, [_P, _P]),
    "kh_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "kh_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "kh_sync": (C.c_int, [_P]),
    "kh_device_count": (C.c_int, []),
    "kh_last_error": (C.c_char_p, []),
    "kh_version": (C.c_char_p, []),
}

_lib = None


def load():
    """Load libkamihip.so; fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension is not built "
                "(run `python -m kami_amd.build`); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (load().kh_last_error() or b"").decode("utf-8", "replace")      # (a message may quote bytes of a malformed file)
