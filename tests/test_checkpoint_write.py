"""Writing checkpoints in the reference's own format (NN::write, nn.cpp:189-202): kh_checkpoint_write and the layers on
top of it (kami_amd.nn.write_checkpoint, NN.write(format="torch"), python -m kami_amd.checkpoint).  CPU only: the
writer needs no engine.  torch.jit.load is the independent loader; oracle/_ref/kami_ref, when built, is the reference's
own NN::read."""
import os
import struct
import subprocess
import sys
import zipfile

import numpy as np
import pytest

from kami_amd import _lib as L
from kami_amd import torch_archive as TA
from kami_amd import weights as W
from kami_amd.nn import KamiError, NN, read_bn_batches, read_checkpoint, write_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CKPT = os.path.join(GOLDEN, "ref_checkpoint_f30_c8_r1.pt")
KAMI_REF = os.path.join(ROOT, "oracle", "_ref", "kami_ref")


def _torch():
    return pytest.importorskip("torch")


def check_loads_under_torch(path, blob, F, C, R, generation, bn_batches):
    """torch.jit.load(path): every tensor of the blob bit for bit under its reference name and shape, every BatchNorm's
    num_batches_tracked == bn_batches (int64), .generation == generation.  -> the state dict."""
    torch = _torch()
    m = torch.jit.load(path, map_location="cpu")
    sd = m.state_dict()
    specs = W.tensor_specs(F, C, R)
    counters = [k for k in sd if k.endswith("num_batches_tracked")]
    assert set(sd) == {n for n, _ in specs} | set(counters)
    assert len(counters) == 3 + 2 * R
    parts = W.split(blob, F, C, R)
    for name, shape in specs:
        t = sd[name]
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape), name
        assert np.array_equal(t.numpy().view(np.uint32), parts[name].view(np.uint32)), name
    for k in counters:
        assert sd[k].dtype == torch.int64 and sd[k].dim() == 0 and int(sd[k]) == bn_batches, k
    assert m.generation == generation
    return sd


SHAPES = [(30, 8, 0), (30, 64, 2), (119, 32, 1), (30, 128, 10), (119, 256, 20)]


@pytest.mark.parametrize("F,C,R", SHAPES, ids=[f"f{F}_c{C}_r{R}" for F, C, R in SHAPES])
def test_written_archive_loads_under_torch(tmp_path, F, C, R):
    blob = W.random_weights(F, C, R, seed=F + C + R, peaky=3.0)
    gen, nbt = 11 + R, 3 * C + 5
    p = str(tmp_path / "m.pt")
    write_checkpoint(p, blob, F, C, R, gen, nbt)
    check_loads_under_torch(p, blob, F, C, R, gen, nbt)
    # and the engine's own reader takes it back, counter included
    b2, F2, C2, R2, g2 = read_checkpoint(p)
    assert (F2, C2, R2, g2) == (F, C, R, gen) and np.array_equal(b2.view(np.uint32), blob.view(np.uint32))
    assert read_bn_batches(p) == nbt
    assert os.listdir(tmp_path) == ["m.pt"]                 # no temporary file left next to it


def test_archive_layout(tmp_path):
    """STORED members with valid CRCs, tensor bytes on 64-byte boundaries, one root directory, no zip64."""
    F, C, R = 30, 16, 1
    p = str(tmp_path / "m.pt")
    write_checkpoint(p, W.random_weights(F, C, R, seed=2), F, C, R, 3)
    raw = open(p, "rb").read()
    with zipfile.ZipFile(p) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert {i.filename.split("/")[0] for i in infos} == {"archive"}
        names = {i.filename[len("archive/"):] for i in infos}
        assert {"data.pkl", "code/__torch__.py", "constants.pkl", "version", "byteorder"} <= names
        assert z.read("archive/version") == b"3\n" and z.read("archive/byteorder") == b"little"
        assert z.read("archive/constants.pkl") == b"\x80\x02).", "an empty tuple"
        assert z.read("archive/data.pkl")[:2] == b"\x80\x02"
        for i in infos:
            assert i.compress_type == zipfile.ZIP_STORED and i.file_size < 2 ** 32
            nl, xl = struct.unpack_from("<HH", raw, i.header_offset + 26)
            assert (i.header_offset + 30 + nl + xl) % 64 == 0, i.filename
    assert raw[-22:-18] == b"PK\x05\x06" and b"PK\x06\x06" not in raw[-200:]


def test_fixture_round_trip(tmp_path):
    """The reference's own checkpoint, read and written again: both readers give the same blob and generation, and
    torch.jit.load sees the same state dict (names, dtypes, shapes, values, order) as in the fixture."""
    torch = _torch()
    blob, F, C, R, gen = read_checkpoint(CKPT)
    nbt = read_bn_batches(CKPT)
    p = str(tmp_path / "again.pt")
    write_checkpoint(p, blob, F, C, R, gen, nbt)
    for reader in (read_checkpoint, TA.load_reference_checkpoint):
        b2, F2, C2, R2, g2 = reader(p)
        assert (F2, C2, R2, g2) == (F, C, R, gen)
        assert np.array_equal(b2.view(np.uint32), blob.view(np.uint32))
    want = torch.jit.load(CKPT, map_location="cpu")
    got = torch.jit.load(p, map_location="cpu")
    sw, sg = want.state_dict(), got.state_dict()
    assert list(sw) == list(sg)
    for k in sw:
        assert sw[k].dtype == sg[k].dtype and sw[k].shape == sg[k].shape and torch.equal(sw[k], sg[k]), k
    assert got.generation == want.generation == gen


def test_bn_counter_read_back(tmp_path):
    """kh_checkpoint_read_ex: an archive's counter (the first BatchNorm's), 0 for a KAMW blob."""
    F, C, R = 30, 8, 1
    blob = W.random_weights(F, C, R, seed=4)
    p = str(tmp_path / "m.pt")
    write_checkpoint(p, blob, F, C, R, 2, 2 ** 40 + 3)       # needs the 8-byte pickle integer
    assert read_bn_batches(p) == 2 ** 40 + 3
    assert read_bn_batches(CKPT) == 0
    k = str(tmp_path / "m.kamw")
    W.save(k, blob, F, C, R, 2)
    assert read_bn_batches(k) == 0


@pytest.mark.skipif(not os.path.exists(KAMI_REF), reason="oracle/_ref/kami_ref not built (needs the reference tree at build time)")
@pytest.mark.parametrize("F,C,R", [(30, 8, 1), (119, 32, 2)])
def test_reference_nn_read_takes_the_written_archive(tmp_path, F, C, R):
    """kami_ref convert runs the reference's own NN::read (nn.cpp:204-222, libtorch's InputArchive) on the archive and
    dumps what it loaded: the same blob and generation."""
    blob = W.random_weights(F, C, R, seed=7, peaky=2.0)
    p, out = str(tmp_path / "m.pt"), str(tmp_path / "back.bin")
    write_checkpoint(p, blob, F, C, R, 5, 40)
    r = subprocess.run([KAMI_REF, "convert", p, str(F), str(C), str(R), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    b2, F2, C2, R2, g2 = W.load(out)
    assert (F2, C2, R2, g2) == (F, C, R, 5)
    assert np.array_equal(b2.view(np.uint32), blob.view(np.uint32))


def _write_rc(path, blob, F, C, R, gen=0, nbt=0, nfloats=None):
    lib = L.load()
    b = np.ascontiguousarray(blob, np.float32)
    return lib.kh_checkpoint_write(path.encode(), F, C, R, gen, nbt, b.ctypes.data, b.size if nfloats is None else nfloats)


def test_refusals(tmp_path):
    F, C, R = 30, 8, 1
    blob = W.random_weights(F, C, R, seed=1)
    p = str(tmp_path / "m.pt")
    assert _write_rc(p, blob, F, C, R, nfloats=blob.size - 1) == L.KH_ERR_INVALID
    assert _write_rc(p, blob, F, C, R + 1) == L.KH_ERR_INVALID            # the blob is not an R+1 network
    assert _write_rc(p, blob, 0, C, R) == L.KH_ERR_INVALID
    assert _write_rc(p, blob, F, 2000, R) == L.KH_ERR_INVALID
    assert _write_rc(p, blob, F, C, -1) == L.KH_ERR_INVALID
    assert _write_rc(p, blob, F, C, R, nbt=-1) == L.KH_ERR_INVALID
    assert os.listdir(tmp_path) == []
    with pytest.raises(KamiError) as ei:
        write_checkpoint(p, blob, F, C, 2, 0)
    assert ei.value.status == L.KH_ERR_INVALID and "floats" in str(ei.value)


def test_failed_write_leaves_no_file(tmp_path):
    F, C, R = 30, 8, 1
    blob = W.random_weights(F, C, R, seed=1)
    # a directory that does not exist
    missing = str(tmp_path / "nope" / "m.pt")
    assert _write_rc(missing, blob, F, C, R) == L.KH_ERR_INVALID
    assert not os.path.exists(os.path.dirname(missing))
    # the archive is complete, the final rename fails (the target is a directory): the temporary file goes
    target = tmp_path / "taken"
    target.mkdir()
    assert _write_rc(str(target), blob, F, C, R) == L.KH_ERR_INVALID
    assert os.listdir(tmp_path) == ["taken"] and os.listdir(target) == []
    # a directory this user may not write to (meaningless for root, who writes anyway)
    ro = tmp_path / "ro"
    ro.mkdir()
    os.chmod(ro, 0o500)
    try:
        if not os.access(str(ro), os.W_OK):
            assert _write_rc(str(ro / "m.pt"), blob, F, C, R) == L.KH_ERR_INVALID
            assert os.listdir(ro) == []
    finally:
        os.chmod(ro, 0o700)


def test_nn_write_default_is_still_kamw(tmp_path):
    """NN.write(path) without a format keeps writing the KAMW container (the engine itself is stood in for: the
    format choice is host code, the GPU test writes from a real engine)."""
    F, C, R = 30, 8, 1
    blob = W.random_weights(F, C, R, seed=1)
    nn = object.__new__(NN)
    nn.cfg = L.Config(width=8, height=8, features=F, psize=4672, filters=C, residuals=R)
    nn.get_weights = lambda: blob
    nn.get_generation = lambda: 4
    p = str(tmp_path / "m.bin")
    nn.write(p)
    assert open(p, "rb").read(4) == struct.pack("<i", W.MAGIC)
    assert W.load(p)[4] == 4
    with pytest.raises(ValueError):
        nn.write(p, format="onnx")


def test_converter_cli(tmp_path):
    """python -m kami_amd.checkpoint: a KAMW blob and a reference archive in, a reference archive out."""
    F, C, R = 30, 16, 2
    blob = W.random_weights(F, C, R, seed=9)
    src, dst = str(tmp_path / "m.kamw"), str(tmp_path / "m.pt")
    W.save(src, blob, F, C, R, generation=6)
    r = subprocess.run([sys.executable, "-m", "kami_amd.checkpoint", src, dst], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    check_loads_under_torch(dst, blob, F, C, R, 6, 0)
    # an archive in: generation and counter carried over
    again = str(tmp_path / "again.pt")
    write_checkpoint(src + ".pt", blob, F, C, R, 6, 77)
    r = subprocess.run([sys.executable, "-m", "kami_amd.checkpoint", src + ".pt", again], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    check_loads_under_torch(again, blob, F, C, R, 6, 77)
    # garbage in: an error, nothing written
    bad = str(tmp_path / "bad.bin")
    open(bad, "wb").write(b"not a checkpoint")
    r = subprocess.run([sys.executable, "-m", "kami_amd.checkpoint", bad, str(tmp_path / "x.pt")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and not os.path.exists(tmp_path / "x.pt")
