"""Timing of cutout (ckl_cutout: the decode pipeline up to the run tables over the box's z-range, then
k_paint_window, then a copy of the box alone) on the 1024 x 1024 x 512 u32 Voronoi volume, against the
only other way to the same array: decompress_range(b, z0, z1)[x0:x1, y0:y1], which paints, copies and
then crops the whole slices.  Per box: wall time of both, median of REPS calls after WARM warm-ups, and
from a session made once (ckl_decoder_cutout into a device buffer) the device time of k_paint_window
(its entry in the stage table) and of the whole span.

  python tools/cutout_timing.py [output file, default profiles/cutout_timing.txt]"""
import ctypes as C
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import crackle_amd
from crackle_amd import _lib, synth

WARM, REPS = 3, 20
BOXES = {
  "128^3 at an unaligned origin": (333, 461, 205, 333, 100, 228),
  "256 x 256 x 512": (100, 356, 300, 556, 0, 512),
  "512 x 512 x 64": (256, 768, 129, 641, 200, 264),
  "full plane x 64": (0, 1024, 0, 1024, 200, 264),
}


def median_ms(call):
  times = []
  for i in range(WARM + REPS):
    t0 = time.perf_counter()
    call()
    if i >= WARM:
      times.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(times)), min(times)


def device_times(binary, box):
  """(k_paint_window ms, span ms): medians over REPS runs of one session."""
  x0, x1, y0, y1, z0, z1 = box
  L = _lib.lib()
  handle = C.c_void_p()
  assert L.ckl_decoder_create(binary, len(binary), z0, z1, 0, C.byref(handle)) == _lib.CKL_OK, _lib.last_error()
  out = torch.empty(((x1 - x0) * (y1 - y0) * (z1 - z0),), dtype=torch.int32, device="cuda")
  paint, span = [], []
  for i in range(WARM + REPS):
    assert L.ckl_decoder_cutout(handle, x0, x1, y0, y1, out.data_ptr(), out.numel() * 4, 0, 0) == _lib.CKL_OK, _lib.last_error()
    ms, name, last = C.c_float(), C.c_char_p(), None
    k = 0
    while L.ckl_decoder_stage_timing(handle, k, C.byref(name), C.byref(ms)) == _lib.CKL_OK:
      last = (name.value.decode(), ms.value)
      k += 1
    assert last and last[0] == "k_paint_window", last
    total = C.c_float()
    L.ckl_decoder_last_timing(handle, C.byref(total), None)
    if i >= WARM:
      paint.append(last[1])
      span.append(total.value)
  L.ckl_decoder_destroy(handle)
  return float(np.median(paint)), float(np.median(span))


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cutout_timing.txt")
  vol = synth.as_numpy_f(synth.voronoi_labels((1024, 1024, 512), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"))
  binary = bytes(crackle_amd.compress(vol))
  torch.cuda.synchronize()
  lines = [
    f"cutout timing: 1024 x 1024 x 512 uint32 Voronoi, stream of {len(binary)} bytes; wall ms = median (min) of {REPS} calls after {WARM} warm-ups",
    "box | cutout() wall ms | decompress_range()[crop] wall ms | ratio | k_paint_window device ms | session span device ms | box MiB | slices MiB",
  ]
  for name, box in BOXES.items():
    x0, x1, y0, y1, z0, z1 = box
    expr = np.s_[x0:x1, y0:y1, z0:z1]
    got = crackle_amd.cutout(binary, expr)
    assert np.array_equal(got, vol[expr]), name
    assert np.array_equal(crackle_amd.decompress_range(binary, z0, z1)[x0:x1, y0:y1], vol[expr]), name
    cut, cut_min = median_ms(lambda: crackle_amd.cutout(binary, expr))
    crop, crop_min = median_ms(lambda: crackle_amd.decompress_range(binary, z0, z1)[x0:x1, y0:y1])
    paint, span = device_times(binary, box)
    lines.append(
      f"{name} | {cut:.2f} ({cut_min:.2f}) | {crop:.2f} ({crop_min:.2f}) | {crop / cut:.2f}x | {paint:.3f} | {span:.3f} | "
      f"{got.nbytes / 2**20:.0f} | {1024 * 1024 * (z1 - z0) * 4 / 2**20:.0f}")
    print(lines[-1], flush=True)
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
