"""kh_train_config's optimizer fields and kh_train_config_check, without a GPU: the struct's size and offsets against
the header (a C program compiled with the host compiler), what the check accepts and rejects, the exported symbols."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from kami_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["lr", "epochs", "batch", "detect_anomaly", "momentum", "weight_decay", "max_grad_norm", "nesterov"]


def test_train_config_is_32_bytes():
    assert C.sizeof(L.TrainConfig) == 32
    assert [f[0] for f in L.TrainConfig._fields_] == FIELDS
    cfg = L.TrainConfig(0.005, 8, 8, 1)                      # positional construction as before: the new fields stay zero
    assert (cfg.momentum, cfg.weight_decay, cfg.max_grad_norm, cfg.nesterov) == (0.0, 0.0, 0.0, 0)


def test_train_config_offsets_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "a host C compiler is needed"
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kami_hip.h"\nint main(void)\n{\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(kh_train_config, {f}));\n' for f in FIELDS)
                   + '    printf("sizeof %zu\\n", sizeof(kh_train_config));\n    return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == C.sizeof(L.TrainConfig) == 32
    assert {f: int(v) for f, v in got.items()} == {f: getattr(L.TrainConfig, f).offset for f in FIELDS}


def _check(**kw):
    cfg = L.TrainConfig(0.005, 8, 8, 0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    rc = L.load().kh_train_config_check(C.byref(cfg))
    return rc, L.last_error()


def test_train_config_check_accepts():
    lib = L.load()
    zeroed = L.TrainConfig()
    zeroed.epochs, zeroed.batch = 1, 2                       # (all-zero epochs / batch are the existing rejections)
    assert lib.kh_train_config_check(C.byref(zeroed)) == L.KH_OK
    assert _check()[0] == L.KH_OK
    assert _check(momentum=0.9, nesterov=1, weight_decay=1e-4, max_grad_norm=5.0)[0] == L.KH_OK
    assert _check(momentum=0.999, max_grad_norm=1e30)[0] == L.KH_OK


@pytest.mark.parametrize("field,value,names", [
    ("momentum", float("nan"), "momentum"), ("momentum", float("inf"), "momentum"), ("momentum", -0.1, "momentum"),
    ("momentum", 1.0, "momentum"), ("momentum", 1.5, "momentum"),
    ("weight_decay", float("nan"), "weight_decay"), ("weight_decay", float("inf"), "weight_decay"), ("weight_decay", -1e-4, "weight_decay"),
    ("max_grad_norm", float("nan"), "max_grad_norm"), ("max_grad_norm", float("-inf"), "max_grad_norm"), ("max_grad_norm", -1.0, "max_grad_norm"),
    ("nesterov", 2, "nesterov"), ("nesterov", -1, "nesterov"),
    ("nesterov", 1, "nesterov"),                             # with momentum == 0
    ("batch", 1, "batch"), ("epochs", 0, "epochs"),
])
def test_train_config_check_rejects(field, value, names):
    extra = {"momentum": 0.9} if field == "nesterov" and value != 1 else {}
    rc, msg = _check(**extra, **{field: value})
    assert rc == L.KH_ERR_INVALID and names in msg, (rc, msg)


def test_train_config_check_rejects_null():
    assert L.load().kh_train_config_check(None) == L.KH_ERR_INVALID


def test_new_symbols_are_exported():
    lib = C.CDLL(L.LIB_PATH)
    for name in ("kh_train_config_check", "kh_train_grad_norms"):
        assert hasattr(lib, name), name
        assert name in L.SYMBOLS
    with open(os.path.join(ROOT, "include", "kami_hip.h")) as f:
        header = f.read()
    assert "kh_train_config_check(" in header and "kh_train_grad_norms(" in header
