"""Timing of overlay and mask_by (ckl_combine: two decode sessions' run tables -> k_erode_run_labels twice,
k_combine_cuts, k_combine_labels, k_pool_planes -> the encoder's crack and label stages, no voxel anywhere) on A = C1
(512 x 512 x 128 u32 Voronoi, cell (32, 32, 8): BASELINE.json's c1) and B = a second Voronoi of that shape, cell
(48, 48, 12), with the cells of even label zeroed (about half of them), per rule:

  (a)  ckl_combine(A's stream, B's stream, rule): one call, host streams in, host stream out
  (n)  compress(np.where(...)) of two decompress calls through this same library: the route the library had before

Same process, alternating, WARM warm-ups, median, minimum and maximum of REPS.  The device time of the combining kernels
together (HIP events around them: both k_erode_run_labels, k_combine_cuts, the host's wait for the cut count,
k_combine_labels, k_pool_planes) and the pieces are read from the [ckl combine host ms] line (CKL_PROFILE) of separate
calls.  The first result of (a) is checked against (n)'s.

  python tools/combine_timing.py [--out FILE, default profiles/combine_timing.txt]"""
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
SHAPE = (512, 512, 128)
RULES = (("overlay", _lib.CKL_COMBINE_OVERLAY), ("mask_by", _lib.CKL_COMBINE_KEEP_WHERE), ("mask_by(invert)", _lib.CKL_COMBINE_DROP_WHERE))
L = _lib.lib()


def route_a(a, b, rule):
  out, n = C.c_void_p(), C.c_uint64()
  assert L.ckl_combine(a, len(a), b, len(b), rule, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def route_n(a, b, rule):
  va, vb = crackle_amd.decompress(a), crackle_amd.decompress(b)
  if rule == _lib.CKL_COMBINE_OVERLAY:
    v = np.where(vb != 0, vb, va)
  elif rule == _lib.CKL_COMBINE_KEEP_WHERE:
    v = np.where(vb != 0, va, 0)
  else:
    v = np.where(vb != 0, 0, va)
  return bytes(crackle_amd.compress(np.asfortranarray(v.astype(va.dtype))))


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


def stage_line(a, b, rule, reps=5):
  """Device time of the combining kernels and the pieces, from the [ckl combine host ms] lines of `reps` profiled calls."""
  sys.stderr.flush()
  saved = os.dup(2)
  vals, lines, pieces = [], [], set()
  with tempfile.TemporaryFile(mode="w+b") as tmp:
    os.dup2(tmp.fileno(), 2)
    os.environ["CKL_PROFILE"] = "1"
    try:
      for _ in range(reps):
        route_a(a, b, rule)
    finally:
      del os.environ["CKL_PROFILE"]
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    for line in tmp.read().decode().splitlines():
      if line.startswith("[ckl combine host ms]"):
        fields = dict(w.split("=") for w in line.split()[4:])
        lines.append(line)
        vals.append(float(fields["k_combine_device"]))
        pieces.add(int(fields["pieces"]))
  assert len(vals) == reps and len(pieces) == 1
  return float(np.median(vals)), min(vals), max(vals), pieces.pop(), lines[-1]


def main():
  args = sys.argv[1:]
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "combine_timing.txt")
  vol_a = synth.as_numpy_f(synth.voronoi_labels(SHAPE, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"))
  vol_b = synth.as_numpy_f(synth.voronoi_labels(SHAPE, np.uint32, seed=3, cell=(48, 48, 12), device="cuda:0")).copy(order="F")
  vol_b[vol_b % 2 == 0] = 0
  a, b = bytes(crackle_amd.compress(vol_a)), bytes(crackle_amd.compress(vol_b))
  lines = [
    f"combine timing: {'x'.join(map(str, SHAPE))} u32 Voronoi A, cell (32, 32, 8), {len(a)} bytes; B cell (48, 48, 12) with {100 * float((vol_b == 0).mean()):.1f} % of its voxels 0, "
    f"{len(b)} bytes; wall ms = median (min - max) of {REPS} calls after {WARM} warm-ups, routes alternating in one process",
    "rule | bytes out | pieces | (a) ckl_combine | k_combine_device | (n) compress(np.where(decompress, decompress))",
  ]
  for name, rule in RULES:
    out = route_a(a, b, rule)
    assert out == route_n(a, b, rule)      # what is timed is right
    t = timed({"a": lambda: route_a(a, b, rule), "n": lambda: route_n(a, b, rule)}, name)
    ms, ms_min, ms_max, pieces, stage = stage_line(a, b, rule)
    cell = lambda k: f"{t[k][0]:.2f} ({t[k][1]:.2f} - {t[k][2]:.2f})"
    lines.append(f"{name} | {len(out)} | {pieces} | {cell('a')} | {ms:.3f} ({ms_min:.3f} - {ms_max:.3f}) | {cell('n')}")
    lines.append(f"  {stage}")
    print(lines[-2], flush=True)
    print(lines[-1], flush=True)
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
