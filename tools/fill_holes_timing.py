"""Timing of fill_holes (ckl_fill_holes: the decode pipeline up to the run tables, k_run_links in its background
mode, k_hole_scan, the label edit, the host's stream assembly; no voxel anywhere) at C1 (512 x 512 x 128 u32 Voronoi)
and C2 (1024 x 1024 x 512 u32 Voronoi) with voids punched in (one box of 1 - 6 voxels a side per 16384 voxels, set to
0), connectivity 6 and 26, against the route a user had before (`c1open`: the C1 volume with every third cell set to 0
as well, a background of a few large holes that reach the faces, which is what k_hole_scan's early-out is for):

  (a)   ckl_fill_holes(stream): one call, host stream in, host stream out (the edited labels around the input's cracks)
  (a+r) recompress(fill_holes(stream)): the same and the re-encode that removes the cracks of what was filled
  (b)   decompress(stream) on the device into a host array, the scipy restatement of tests/fill_holes_numpy.py
        (ndimage.label of the background, one look at every hole's surroundings), compress() of the result

(b) ends re-encoded, so (a+r) is its like; (a) alone leaves the false boundaries in.  One process.  (a) and (a+r)
alternate, WARM warm-ups, median and minimum of REPS, every round printed.  (b) takes seconds to minutes: it runs
B_REPS times per row (once at C2), its first run is the one checked byte for byte against (a+r), every run is printed.

Kernel times are not taken here: `--kernels` only runs ckl_fill_holes a few times per volume and connectivity, for a
separate `rocprofv3 --kernel-trace --stats -- python tools/fill_holes_timing.py --kernels c1 c2` (k_run_links and
k_hole_scan run once per call).

  python tools/fill_holes_timing.py [--kernels] [c1] [c1open] [c2] [--out FILE, default profiles/fill_holes_timing.txt]"""
import ctypes as C
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import torch
import crackle_amd
from crackle_amd import _lib, synth

WARM, REPS = 3, 12
B_REPS = {"c1": 3, "c1open": 3, "c2": 1}
VOLUMES = {"c1": (512, 512, 128), "c1open": (512, 512, 128), "c2": (1024, 1024, 512)}      # (without arguments: c1 and c2)
L = _lib.lib()


def make(shape, seed=5, open_background=False):
  vol = synth.as_numpy_f(synth.voronoi_labels(shape, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")).copy(order="F")
  if open_background:      # every third cell is background: large holes of many thousands of runs that reach the faces
    vol[vol % 3 == 0] = 0
  rng = np.random.RandomState(seed)
  n = shape[0] * shape[1] * shape[2] // 16384
  side = rng.randint(1, 7, (n, 3))
  at = (rng.random_sample((n, 3)) * (np.array(shape) - side + 1)).astype(np.int64)
  for (x, y, z), (dx, dy, dz) in zip(at.tolist(), side.tolist()):
    vol[x:x + dx, y:y + dy, z:z + dz] = 0
  return vol


def route_a(binary, conn):
  out, n, filled = C.c_void_p(), C.c_uint64(), C.c_uint64()
  assert L.ckl_fill_holes(binary, len(binary), conn, 0, C.byref(out), C.byref(n), C.byref(filled)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value), int(filled.value)
  finally:
    L.ckl_free(out)


def route_b(binary, conn, order):
  import fill_holes_numpy
  vol = crackle_amd.decompress(binary)
  r = fill_holes_numpy.fill_holes(vol, conn)
  return bytes(crackle_amd.compress(r.volume, markov_model_order=order)), r


def timed(calls, label, warm, reps):
  """calls: name -> function; alternating, warm + reps rounds, every round printed: name -> (median ms, min ms)"""
  times = {k: [] for k in calls}
  for i in range(warm + reps):
    row = []
    for k, f in calls.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      f()
      torch.cuda.synchronize()
      ms = (time.perf_counter() - t0) * 1e3
      row.append(f"{k} {ms:.2f}")
      if i >= warm:
        times[k].append(ms)
    print(f"  {label} round {i - warm + 1 if i >= warm else 'warm-up'}: " + " | ".join(row) + " ms", flush=True)
  return {k: (float(np.median(v)), min(v)) for k, v in times.items()}


def main():
  args = sys.argv[1:]
  kernels_only = "--kernels" in args
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "fill_holes_timing.txt")
  names = [a for a in args if a in VOLUMES] or ["c1", "c2"]
  lines = [
    f"fill_holes timing: u32 Voronoi, cell (32, 32, 8), one void of 1 - 6 voxels a side per 16384 voxels; wall ms = median (min) of {REPS} calls after {WARM} warm-ups "
    "for (a) and (a+r), which alternate in one process; (b): median (min) of the runs named, no warm-up",
    "volume | connectivity | holes filled / open / with several labels | bytes in | bytes out of (a) | (a) ckl_fill_holes | (a+r) recompress(fill_holes) | "
    "(b) decode to host + scipy + compress | runs of (b) | (b) / (a) | (b) / (a+r)",
  ]
  for name in names:
    shape = VOLUMES[name]
    binary = bytes(crackle_amd.compress(make(shape, open_background=name.endswith("open"))))
    torch.cuda.synchronize()
    order = crackle_amd.header(binary).markov_model_order
    for conn in (6, 26):
      if kernels_only:
        for _ in range(4):
          route_a(binary, conn)
        continue
      out, filled = route_a(binary, conn)
      clean = crackle_amd.recompress(out)
      b_ms, r = [], None
      for i in range(B_REPS[name]):
        t0 = time.perf_counter()
        got, r = route_b(binary, conn, order)
        b_ms.append((time.perf_counter() - t0) * 1e3)
        print(f"  {name} connectivity {conn} (b) run {i + 1}: {b_ms[-1]:.0f} ms", flush=True)
        if i == 0:      # what is timed is right: the two routes end with the same bytes
          assert got == clean and filled == r.filled
      t = timed({
        "a": lambda: route_a(binary, conn),
        "a+r": lambda: crackle_amd.recompress(route_a(binary, conn)[0]),
      }, f"{name} connectivity {conn}", WARM, REPS)
      b_med, b_min = float(np.median(b_ms)), min(b_ms)
      lines.append(f"{name} | {conn} | {r.filled} / {r.open} / {r.multi} | {len(binary)} | {len(out)} | {t['a'][0]:.2f} ({t['a'][1]:.2f}) | "
                   f"{t['a+r'][0]:.2f} ({t['a+r'][1]:.2f}) | {b_med:.0f} ({b_min:.0f}) | {len(b_ms)} | {b_med / t['a'][0]:.0f}x | {b_med / t['a+r'][0]:.0f}x")
      print(lines[-1], flush=True)
  if kernels_only:
    return
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
