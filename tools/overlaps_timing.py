"""Timing of overlaps (ckl_decoder_overlaps: both decode pipelines up to their run tables, then k_run_overlaps
and k_contacts_compact) at C1 (512 x 512 x 128) and C2 (1024 x 1024 x 512), uint32 Voronoi: A of cell
(32, 32, 8) against B, another seed of cell (16, 16, 4) -- an over-segmentation against a segmentation.
Per size, medians after a warm-up call, in one process:
  run tables   wall time of ckl_decoder_overlaps on two sessions made once, the device span session A reports
               (ckl_decoder_last_timing: from A's first kernel to the last copy, B's pipeline and the host
               synchronisations included), and the wall times of operations._overlap_counts (sessions, uploads
               and the numpy arrays included) and of crackle_amd.overlaps (the Python dict on top);
  voxels       the route without this function: both streams decoded into device tensors through
               HipDecodeSession, then torch.unique(a.to(int64) * 2**31 + b, return_counts=True), timed as
               decode and as unique (wall, device synchronised).
Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import ctypes as C
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crackle_amd
from crackle_amd import _lib, operations, synth
from crackle_amd.distributed import HipDecodeSession

SHAPES = {"c1": (512, 512, 128), "c2": (1024, 1024, 512)}
reps = 5
L = _lib.lib()


def volumes(shape):
  a = synth.voronoi_labels(shape, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")
  b = synth.voronoi_labels(shape, np.uint32, seed=3, cell=(16, 16, 4), device="cuda:0")
  return a, b


for name in (sys.argv[1:] or list(SHAPES)):
  shape = SHAPES[name]
  ta, tb = volumes(shape)
  bin_a = bytes(crackle_amd.compress(synth.as_numpy_f(ta)))
  bin_b = bytes(crackle_amd.compress(synth.as_numpy_f(tb)))
  del ta, tb
  torch.cuda.synchronize()

  # ---- the run tables
  ha, hb = C.c_void_p(), C.c_void_p()
  assert L.ckl_decoder_create(bin_a, len(bin_a), 0, -1, 0, C.byref(ha)) == _lib.CKL_OK, _lib.last_error()
  assert L.ckl_decoder_create(bin_b, len(bin_b), 0, -1, 0, C.byref(hb)) == _lib.CKL_OK, _lib.last_error()
  for h in (ha, hb):
    L.ckl_decoder_set_stage_events(h, 0)
  walls, spans = [], []
  for i in range(reps + 1):
    pp, cp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    t0 = time.perf_counter()
    assert L.ckl_decoder_overlaps(ha, hb, C.byref(pp), C.byref(cp), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
    t1 = time.perf_counter()
    span = C.c_float()
    L.ckl_decoder_last_timing(ha, C.byref(span), None)
    L.ckl_free(pp)
    L.ckl_free(cp)
    if i:      # the first call loads the code objects and grows the pools
      walls.append((t1 - t0) * 1e3)
      spans.append(span.value)
  L.ckl_decoder_destroy(ha)
  L.ckl_decoder_destroy(hb)
  arrays, py = [], []
  for i in range(3):
    t0 = time.perf_counter()
    pairs, counts = operations._overlap_counts(bin_a, bin_b)
    t1 = time.perf_counter()
    table = crackle_amd.overlaps(bin_a, bin_b)
    t2 = time.perf_counter()
    arrays.append((t1 - t0) * 1e3)
    py.append((t2 - t1) * 1e3)
  assert len(table) == n.value == counts.size
  del table, pairs, counts

  # ---- the voxels
  sx, sy, sz = shape
  sa, sb = HipDecodeSession(bin_a, 0, sz, 0), HipDecodeSession(bin_b, 0, sz, 0)
  out_a = torch.empty((sz, sy, sx), dtype=torch.int32, device="cuda:0")
  out_b = torch.empty((sz, sy, sx), dtype=torch.int32, device="cuda:0")
  decode, unique = [], []
  for i in range(reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sa.run(out_a)
    sb.run(out_b)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    keys, cnt = torch.unique(out_a.to(torch.int64) * (1 << 31) + out_b, return_counts=True)      # labels below 2^31
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert keys.numel() == n.value and int(cnt.sum()) == sx * sy * sz
    del keys, cnt
    if i:
      decode.append((t1 - t0) * 1e3)
      unique.append((t2 - t1) * 1e3)
  sa.close()
  sb.close()
  del out_a, out_b
  torch.cuda.empty_cache()
  voxels = np.median(decode) + np.median(unique)
  print(f"overlaps {name} {sx}x{sy}x{sz}: {n.value} pairs; streams {len(bin_a)} + {len(bin_b)} bytes\n"
        f"  run tables: ckl_decoder_overlaps wall median {np.median(walls):.3f} ms (min {min(walls):.3f}), "
        f"device span median {np.median(spans):.3f} ms (min {min(spans):.3f}); "
        f"operations._overlap_counts (sessions, uploads, numpy arrays) wall median {np.median(arrays):.1f} ms; crackle_amd.overlaps (the dict) wall median {np.median(py):.1f} ms\n"
        f"  voxels:     decode both median {np.median(decode):.3f} ms + torch.unique median {np.median(unique):.3f} ms = {voxels:.3f} ms; "
        f"HBM {2 * 4 * sx * sy * sz / 2**20:.0f} MiB of labels + {8 * sx * sy * sz / 2**20:.0f} MiB of keys before the sort\n"
        f"  ratio voxels / run tables (wall of ckl_decoder_overlaps): {voxels / np.median(walls):.2f}", flush=True)
