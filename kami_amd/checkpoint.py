"""Checkpoint converter: python -m kami_amd.checkpoint IN OUT

IN is an engine KAMW blob or a libtorch archive written by the reference's NN::write (nn.cpp:189-202); OUT is
written in the reference's own format, which a stock kami's NN::read (nn.cpp:204-222) loads.  The network shape,
the generation and (from an archive) the BatchNorm batch counter are carried over.  No GPU is needed.
"""
from __future__ import annotations

import argparse
import sys

from .nn import KamiError, read_bn_batches, read_checkpoint, write_checkpoint


def convert(src: str, dst: str):
    """-> (features, filters, residuals, generation, bn_batches) of what was written."""
    blob, F, C, R, gen = read_checkpoint(src)
    nbt = read_bn_batches(src)
    write_checkpoint(dst, blob, F, C, R, gen, nbt)
    return F, C, R, gen, nbt


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kami_amd.checkpoint", description=__doc__.split("\n\n")[0])
    ap.add_argument("src", help="KAMW blob or reference (libtorch) checkpoint")
    ap.add_argument("dst", help="reference checkpoint to write")
    a = ap.parse_args(argv)
    try:
        F, C, R, gen, nbt = convert(a.src, a.dst)
    except KamiError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    print(f"{a.dst}: {F} features, {C} filters, {R} residual blocks, generation {gen}, bn batches {nbt}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
