"""Timing of crop_boxes and crop (ckl_crop_boxes: one decode session's run tables -> k_erode_run_labels once, then per box
k_crop_cuts, k_crop_labels, k_pool_planes -> the encoder's crack and label stages, no voxel anywhere) on the 2 x 2 x 2
grid of chunks of C1 (512 x 512 x 128 u32 Voronoi, cell (32, 32, 8): BASELINE.json's c1) and, with --headline, of the
1024 x 1024 x 512 volume of those cells:

  (a)  ckl_crop_boxes of the eight boxes: one call, one decode, host stream in, eight host streams out
  (b)  eight ckl_crop calls: eight decodes of the boxes' own z-ranges
  (n)  eight times compress(cutout(stream, box)) through this same library: the route the library had before

Same process, alternating, WARM warm-ups, median, minimum and maximum of REPS.  The device time of the cropping kernels
(HIP events around them, per box: k_crop_cuts, the host's wait for the cut count, k_crop_labels, k_pool_planes), summed
over the eight boxes, the shared TABLES run and the pieces are read from the [ckl crop host ms] lines (CKL_PROFILE) of
separate calls of (a).  The first result of (a) is checked against (n)'s.

  python tools/crop_timing.py [--headline] [--out FILE, default profiles/crop_timing.txt]"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import crackle_amd
from crackle_amd import _lib, synth

WARM, REPS = 2, 7
INPUTS = [("C1", (512, 512, 128)), ("headline", (1024, 1024, 512))]
L = _lib.lib()


def grid_of(shape):
  """the 2 x 2 x 2 grid of chunks"""
  return crackle_amd.chunk_boxes(shape, tuple(s // 2 for s in shape))


def route_a(stream, boxes):
  k = len(boxes)
  flat = (C.c_int64 * (6 * k))(*[v for b in boxes for v in b])
  outs, lens = (C.c_void_p * k)(), (C.c_uint64 * k)()
  assert L.ckl_crop_boxes(stream, len(stream), flat, k, 0, -1, 0, outs, lens) == _lib.CKL_OK, _lib.last_error()
  try:
    return [C.string_at(outs[i], lens[i]) for i in range(k)]
  finally:
    for i in range(k):
      L.ckl_free(outs[i])


def route_b(stream, boxes):
  got = []
  for b in boxes:
    out, n = C.c_void_p(), C.c_uint64()
    assert L.ckl_crop(stream, len(stream), *b, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
    try:
      got.append(C.string_at(out.value, n.value))
    finally:
      L.ckl_free(out)
  return got


def route_n(stream, boxes):
  return [bytes(crackle_amd.compress(np.asfortranarray(crackle_amd.cutout(stream, (slice(b[0], b[1]), slice(b[2], b[3]), slice(b[4], b[5])))))) for b in boxes]


def timed(calls, label):
  """calls: name -> function; alternating, WARM + REPS rounds: name -> (median ms, min ms, max ms)"""
  times = {k: [] for k in calls}
  for i in range(WARM + REPS):
    row = []
    for k, f in calls.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      f()
      torch.cuda.synchronize()
      ms = (time.perf_counter() - t0) * 1e3
      row.append(f"{k} {ms:.2f}")
      if i >= WARM:
        times[k].append(ms)
    print(f"  {label} round {i - WARM + 1 if i >= WARM else 'warm-up'}: " + " | ".join(row) + " ms", flush=True)
  return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def stage_lines(stream, boxes, reps=5):
  """Per profiled call of (a): the shared TABLES run, the cropping kernels' device time summed over the boxes, the pieces
  summed over the boxes; and the lines of the last call."""
  sys.stderr.flush()
  saved = os.dup(2)
  with tempfile.TemporaryFile(mode="w+b") as tmp:
    os.dup2(tmp.fileno(), 2)
    os.environ["CKL_PROFILE"] = "1"
    try:
      for _ in range(reps):
        route_a(stream, boxes)
    finally:
      del os.environ["CKL_PROFILE"]
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    mine = [l for l in tmp.read().decode().splitlines() if l.startswith("[ckl crop host ms]")]
  assert len(mine) == reps * len(boxes)
  tables, device, pieces = [], [], set()
  for r in range(reps):
    fields = [dict(w.split("=") for w in l.split()[4:]) for l in mine[r * len(boxes):(r + 1) * len(boxes)]]
    tables.append(sum(float(f["tables"]) for f in fields))
    device.append(sum(float(f["k_crop_device"]) for f in fields))
    pieces.add(sum(int(f["pieces"]) for f in fields))
  assert len(pieces) == 1
  spread = lambda v: f"{float(np.median(v)):.3f} ({min(v):.3f} - {max(v):.3f})"
  return spread(tables), spread(device), pieces.pop(), mine[-len(boxes):]


def main():
  args = sys.argv[1:]
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "crop_timing.txt")
  inputs = INPUTS if "--headline" in args else INPUTS[:1]
  lines = [
    f"crop timing: u32 Voronoi, cell (32, 32, 8), cut into its 2 x 2 x 2 grid of chunks; wall ms = median (min - max) of {REPS} rounds after {WARM} warm-ups, "
    "routes alternating in one process; tables and k_crop_device: ms over 5 profiled calls of (a), k_crop_device and pieces summed over the eight boxes",
    "input | bytes in | bytes out | pieces | (a) ckl_crop_boxes, one call | (b) 8 x ckl_crop | (n) 8 x compress(cutout) | tables | k_crop_device",
  ]
  for name, shape in inputs:
    vol = synth.as_numpy_f(synth.voronoi_labels(shape, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"))
    stream = bytes(crackle_amd.compress(vol))
    del vol
    boxes = grid_of(shape)
    assert len(boxes) == 8
    out = route_a(stream, boxes)
    assert out == route_n(stream, boxes) and out == route_b(stream, boxes)      # what is timed is right
    t = timed({"a": lambda: route_a(stream, boxes), "b": lambda: route_b(stream, boxes), "n": lambda: route_n(stream, boxes)}, name)
    tables, device, pieces, last = stage_lines(stream, boxes)
    cell = lambda k: f"{t[k][0]:.2f} ({t[k][1]:.2f} - {t[k][2]:.2f})"
    lines.append(f"{name} {'x'.join(map(str, shape))} | {len(stream)} | {sum(map(len, out))} | {pieces} | {cell('a')} | {cell('b')} | {cell('n')} | {tables} | {device}")
    lines.extend("  " + l for l in last)
    print("\n".join(lines[-1 - len(last):]), flush=True)
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
