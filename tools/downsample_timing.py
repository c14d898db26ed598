"""Timing of downsample (ckl_downsample: the decoder's run tables -> k_erode_run_labels, k_pool_cuts, k_pool_labels,
k_pool_planes -> the encoder's crack and label stages for the pooled shape, no voxel anywhere) at C1 (512 x 512 x 128 u32
Voronoi, cell (32, 32, 8): BASELINE.json's c1), per factor (2, 2, 1) and (2, 2, 2):

  (a)  ckl_downsample(stream): one call, host stream in, host stream out
  (m)  mode_pooling_2x2x1(stream) of the same stream, 2 x 2 x 1 whatever the factor: the route the library had before,
       which paints the whole volume, pools it and encodes slice by slice, then stacks the slices on the host
  (n)  compress(pool(decompress(stream))) with the pooling in numpy on the host (tests/downsample_numpy.py's arithmetic)

Same process, alternating, WARM warm-ups, median, minimum and maximum of REPS.  The device time of the pooling kernels
together (HIP events around them, the host's wait for the cut count between k_pool_cuts and k_pool_labels included)
and the pieces are read from the [ckl downsample host ms] line (CKL_PROFILE) of separate calls.  The first result of
(a) is checked against (n)'s, and for (2, 2, 1) its voxels against (m)'s.

  python tools/downsample_timing.py [--out FILE, default profiles/downsample_timing.txt]"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import crackle_amd
import downsample_numpy
from crackle_amd import _lib, synth

WARM, REPS = 2, 7
SHAPE = (512, 512, 128)
FACTORS = ((2, 2, 1), (2, 2, 2))
L = _lib.lib()


def route_a(binary, factor):
  out, n = C.c_void_p(), C.c_uint64()
  assert L.ckl_downsample(binary, len(binary), *factor, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def route_m(binary):
  return crackle_amd.mode_pooling_2x2x1(binary)


def route_n(binary, factor):
  return bytes(crackle_amd.compress(downsample_numpy.downsample(crackle_amd.decompress(binary), factor)))


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


def stage_line(binary, factor, reps=5):
  """Device time of the pooling kernels and the pieces, from the [ckl downsample host ms] lines of `reps` profiled calls."""
  sys.stderr.flush()
  saved = os.dup(2)
  vals, lines, pieces = [], [], set()
  with tempfile.TemporaryFile(mode="w+b") as tmp:
    os.dup2(tmp.fileno(), 2)
    os.environ["CKL_PROFILE"] = "1"
    try:
      for _ in range(reps):
        route_a(binary, factor)
    finally:
      del os.environ["CKL_PROFILE"]
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    for line in tmp.read().decode().splitlines():
      if line.startswith("[ckl downsample host ms]"):
        fields = dict(w.split("=") for w in line.split()[4:])
        lines.append(line)
        vals.append(float(fields["k_pool_device"]))
        pieces.add(int(fields["pieces"]))
  assert len(vals) == reps and len(pieces) == 1
  return float(np.median(vals)), min(vals), max(vals), pieces.pop(), lines[-1]


def main():
  args = sys.argv[1:]
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "downsample_timing.txt")
  binary = bytes(crackle_amd.compress(synth.as_numpy_f(synth.voronoi_labels(SHAPE, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"))))
  lines = [
    f"downsample timing: {'x'.join(map(str, SHAPE))} u32 Voronoi, cell (32, 32, 8), {len(binary)} bytes in; wall ms = median (min - max) of {REPS} calls "
    f"after {WARM} warm-ups, routes alternating in one process",
    "factor | bytes out | pieces | (a) ckl_downsample | k_pool_device | (m) mode_pooling_2x2x1 of the same stream | (n) compress(numpy pool(decompress))",
  ]
  try:
    pooled_m = crackle_amd.decompress(route_m(binary))
  except ValueError as e:      # its pooled slices disagree on the crack format: there is nothing to time
    pooled_m = None
    lines.append(f"(m) raises on this stream: {e}")
  for factor in FACTORS:
    out = route_a(binary, factor)
    assert out == route_n(binary, factor)      # what is timed is right
    if factor == (2, 2, 1) and pooled_m is not None:
      assert np.array_equal(crackle_amd.decompress(out), pooled_m)
    calls = {"a": lambda: route_a(binary, factor), "m": lambda: route_m(binary), "n": lambda: route_n(binary, factor)}
    if pooled_m is None:
      del calls["m"]
    t = timed(calls, f"factor {factor}")
    ms, ms_min, ms_max, pieces, stage = stage_line(binary, factor)
    cell = lambda k: f"{t[k][0]:.2f} ({t[k][1]:.2f} - {t[k][2]:.2f})" if k in t else "-"
    lines.append(f"{factor} | {len(out)} | {pieces} | {cell('a')} | {ms:.3f} ({ms_min:.3f} - {ms_max:.3f}) | {cell('m')} | {cell('n')}")
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
