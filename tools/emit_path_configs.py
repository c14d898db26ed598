"""Which kernels pack the crack codes of bench.py's configurations behind k_trail_items: k_trail_emit, or
k_trail_offsets + k_trail_expand + k_finish (ckl_encoder_emit_path), with the LDS k_trail_emit's plan asks for.
The volumes are bench.py's own (same generator, seed, cell), the first slices of each: the plan goes by the largest
slice's crack edges and chain capacity, not by the depth."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

from crackle_amd import distributed as ckd
from crackle_amd import synth

DEV = torch.device("cuda:0")
SLICES = 16
# name, (sx, sy), dtype, data, cell
CONFIGS = [
  ("C2 1024x1024 u32", (1024, 1024), np.uint32, "voronoi", (32, 32, 8)),
  ("C1 512x512 u32", (512, 512), np.uint32, "voronoi", (32, 32, 8)),
  ("C3 slab 1024x1024 u64", (1024, 1024), np.uint64, "voronoi", (32, 32, 8)),
  ("C4 slab 2048x2048 u32", (2048, 2048), np.uint32, "voronoi", (32, 32, 8)),
  ("cell 16x16x4 1024x1024 u64", (1024, 1024), np.uint64, "voronoi", (16, 16, 4)),
  ("cell 12x12x4 1024x1024 u64", (1024, 1024), np.uint64, "voronoi", (12, 12, 4)),
  ("cell 8x8x4 1024x1024 u64", (1024, 1024), np.uint64, "voronoi", (8, 8, 4)),
  ("noise2000 1024x1024 u32", (1024, 1024), np.uint32, "noise2000", None),
  ("binary noise 1024x1024 u32", (1024, 1024), np.uint32, "binary", None),
]


def main():
  be = ckd.HipBackend(0)
  for name, (sx, sy), dt, data, cell in CONFIGS:
    shape = (sx, sy, SLICES)
    if data == "voronoi":
      vol = synth.voronoi_labels(shape, dt, seed=2, device=DEV, offset=(1 << 40) if dt == np.uint64 else 0, cell=cell)
    else:
      vol = synth.random_labels_device(shape, dt, seed=2, high=2000 if data == "noise2000" else 2, device=DEV)
    be.encode(vol, shape)
    fused, need = be.emit_path()
    print(f"{name:32s} {'k_trail_emit' if fused else 'three kernels':14s} LDS asked for {need:9d} bytes ({need / 1024:.1f} KiB)", flush=True)
    del vol


if __name__ == "__main__":
  sys.exit(main())
