"""kh_infer's host-buffer I/O paths against each other: each path is chosen by the call's shape and the engine's settings,
and every path must hand back the same bits.  Run with -m gpu."""
import numpy as np
import pytest

from kami_amd import NN, _lib as L, weights as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mode", [L.KH_VALUE_REFERENCE_FLAT, L.KH_VALUE_PER_SAMPLE0])
def test_small_zero_copy_path_gives_the_staged_bits(dtype, mode, monkeypatch):
    """kh_infer at small batches takes the zero-copy path (the kernel reads the planes from and writes the policy rows
    into page-locked blocks itself, a second launch the values); an engine created under KAMI_SMALL_MAX=0 takes the
    staged path (one copy per argument) for the same calls.  Same bits at the size edges: 25 boards of 119 planes is the
    largest batch under the path's 768 KB limit, 102 of 30 planes likewise."""
    C, R = 64, 2
    rng = np.random.default_rng(8)
    for F, batches in ((119, (1, 16, 25)), (30, (1, 102))):
        blob = W.random_weights(F, C, R, seed=7, peaky=10.0)
        monkeypatch.delenv("KAMI_SMALL_MAX", raising=False)
        small = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype, value_mode=mode)
        monkeypatch.setenv("KAMI_SMALL_MAX", "0")
        staged = NN(8, 8, F, 4672, filters=C, residuals=R, dtype=dtype, value_mode=mode)
        try:
            small.load_weights(blob, 1)
            staged.load_weights(blob, 1)
            for B in batches:
                x = rng.random((B, 8, 8, F), dtype=np.float32)
                want_p, want_v = staged.infer(x)
                got_p, got_v = small.infer(x)
                assert np.array_equal(got_p, want_p) and np.array_equal(got_v, want_v), (F, B)
        finally:
            small.close()
            staged.close()
