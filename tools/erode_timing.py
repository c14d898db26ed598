"""Timing of erode (ckl_erode: the decoder's run tables -> k_erode_run_labels, k_erode_terms, k_erode_keep,
k_erode_planes -> the encoder's crack and label stages, no voxel anywhere) at C1 (512 x 512 x 128 u32 Voronoi) and C2
(1024 x 1024 x 512 u32 Voronoi), connectivity 6 and 26, erode_border as by default, against what a user could do before
with everything on the device:

  (a)  ckl_erode(stream): one call, host stream in, host stream out
  (b1) ckl_decoder_create + ckl_decoder_run painting the volume into a device tensor, the erosion as torch comparisons
       of shifted slices of that tensor, ckl_encoder_create + ckl_encoder_run from the result; sessions made and
       destroyed per call, the volume buffer allocated once outside the clock
  (b2) the same with both sessions made once: ckl_decoder_run + torch + ckl_encoder_run only

Same process, alternating, WARM warm-ups, median and minimum of REPS; the first result of (b1) and (b2) is checked byte
for byte against (a).  The device time of the four erode kernels together is read from the [ckl erode host ms] line
(CKL_PROFILE) of separate calls; their algorithmic bytes come from the shapes and the run count of the volume.

Peak device memory is taken per route in a fresh child process (`--hbm a|b2 NAME CONN`): the most that
hipMemGetInfo's used bytes rose above their value at the child's start, sampled every millisecond by a thread while
the route runs three times, and the value after the last run (the library's pool keeps what it once took).

  python tools/erode_timing.py [c1] [c2] [--out FILE, default profiles/erode_timing.txt]"""
import ctypes as C
import itertools
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import crackle_amd
from crackle_amd import _lib, synth

WARM, REPS = 3, 12
VOLUMES = {"c1": (512, 512, 128), "c2": (1024, 1024, 512)}
HBM_PEAK = 8.0e12      # bytes per second
L = _lib.lib()


def offsets(conn):
  reach = {6: 1, 18: 2, 26: 3}[conn]
  return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, o)) <= reach]


def route_a(binary, conn):
  out, n = C.c_void_p(), C.c_uint64()
  assert L.ckl_erode(binary, len(binary), conn, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def torch_erode(vol, conn):
  """vol: (sz, sy, sx) int32 on the device; erode_border: every voxel on a face goes."""
  sz, sy, sx = vol.shape
  centre = vol[1:-1, 1:-1, 1:-1]
  keep = centre != 0
  for dx, dy, dz in offsets(conn):
    keep &= vol[1 + dz:sz - 1 + dz, 1 + dy:sy - 1 + dy, 1 + dx:sx - 1 + dx] == centre
  out = torch.zeros_like(vol)
  out[1:-1, 1:-1, 1:-1] = torch.where(keep, centre, 0)
  return out


def _paint(dec, vol):
  assert L.ckl_decoder_run(dec, vol.data_ptr(), vol.numel() * 4, 0, 0) == _lib.CKL_OK, _lib.last_error()


def _encode(enc, vol, shape, order):
  out, n = C.c_void_p(), C.c_uint64()
  sx, sy, sz = shape
  assert L.ckl_encoder_run(enc, vol.data_ptr(), sx, sy, sz, 0, 1, order, 0, 1, 0, None, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def route_b1(binary, buf, shape, conn, order):
  dec, enc = C.c_void_p(), C.c_void_p()
  assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(dec)) == _lib.CKL_OK, _lib.last_error()
  try:
    _paint(dec, buf)
  finally:
    L.ckl_decoder_destroy(dec)
  eroded = torch_erode(buf, conn)
  torch.cuda.synchronize()      # (the library's streams wait for the default stream; this is the user's own hand-over)
  assert L.ckl_encoder_create(*shape, 4, 0, C.byref(enc)) == _lib.CKL_OK, _lib.last_error()
  try:
    return _encode(enc, eroded, shape, order)
  finally:
    L.ckl_encoder_destroy(enc)


class Kept:
  def __init__(self, binary, shape):
    self.dec, self.enc, self.shape = C.c_void_p(), C.c_void_p(), shape
    assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(self.dec)) == _lib.CKL_OK, _lib.last_error()
    assert L.ckl_encoder_create(*shape, 4, 0, C.byref(self.enc)) == _lib.CKL_OK, _lib.last_error()

  def __call__(self, buf, conn, order):
    _paint(self.dec, buf)
    eroded = torch_erode(buf, conn)
    torch.cuda.synchronize()
    return _encode(self.enc, eroded, self.shape, order)

  def close(self):
    L.ckl_decoder_destroy(self.dec)
    L.ckl_encoder_destroy(self.enc)


def timed(calls, label):
  """calls: name -> function; alternating, WARM + REPS rounds, every round printed: name -> (median ms, min ms)"""
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
  return {k: (float(np.median(v)), min(v)) for k, v in times.items()}


def stage_line(binary, conn, reps=5):
  """Device time of the four erode kernels (HIP events around them) and the last [ckl erode host ms] line of `reps` profiled calls."""
  sys.stderr.flush()
  saved = os.dup(2)
  vals, lines = [], []
  with tempfile.TemporaryFile(mode="w+b") as tmp:
    os.dup2(tmp.fileno(), 2)
    os.environ["CKL_PROFILE"] = "1"
    try:
      for _ in range(reps):
        route_a(binary, conn)
    finally:
      del os.environ["CKL_PROFILE"]
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    for line in tmp.read().decode().splitlines():
      if line.startswith("[ckl erode host ms]"):
        lines.append(line)
        vals.append(float(dict(w.split("=") for w in line.split()[4:])["k_erode_device"]))
  assert len(vals) == reps
  return float(np.median(vals)), lines[-1]


def kernel_bytes(shape, runs):
  """What the four kernels' algorithm moves, from the shapes.  Per 32-pixel word: k_erode_terms reads the decoder's V
  word and word_base (8 B; the words of the neighbour rows are the neighbour threads' own) and writes P, C, D (12 B);
  k_erode_keep reads them (12 B) and writes K (4 B); k_erode_planes reads K (4 B) and writes V and H (8 B).  Per run:
  k_erode_run_labels reads the component id and its label (12 B) and writes the label (8 B), k_erode_terms reads it
  (8 B; the up to eight other rows that look at the run find it in the cache)."""
  sx, sy, sz = shape
  words = (sx + 31) // 32 * sy * sz
  return words * 48 + runs * 28


def make(shape):
  dvol = synth.voronoi_labels(shape, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")      # (sz, sy, sx)
  runs = int(shape[1] * shape[2] + torch.count_nonzero(dvol[:, :, 1:] != dvol[:, :, :-1]).item())
  binary = bytes(crackle_amd.compress(synth.as_numpy_f(dvol)))
  del dvol
  torch.cuda.empty_cache()
  return binary, runs


def used_bytes():
  free, total = torch.cuda.mem_get_info(0)
  return total - free


def hbm_child(route, name, conn):
  """Runs in a fresh process: prints `peak_bytes end_bytes` above the start of this process' own device use."""
  shape = VOLUMES[name]
  binary, _ = make(shape)
  order = crackle_amd.header(binary).markov_model_order
  torch.cuda.synchronize()
  base = used_bytes()
  peak, stop = [0], threading.Event()

  def sample():
    while not stop.is_set():
      peak[0] = max(peak[0], used_bytes() - base)
      time.sleep(0.001)

  th = threading.Thread(target=sample)
  th.start()
  try:
    if route == "a":
      for _ in range(3):
        route_a(binary, conn)
    else:
      buf = torch.empty((shape[2], shape[1], shape[0]), dtype=torch.int32, device="cuda:0")
      kept = Kept(binary, shape)
      for _ in range(3):
        kept(buf, conn, order)
      kept.close()
    torch.cuda.synchronize()
  finally:
    stop.set()
    th.join()
  end = used_bytes() - base
  print(f"HBM {max(peak[0], end)} {end}", flush=True)


def hbm(route, name, conn):
  r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hbm", route, name, str(conn)], capture_output=True, text=True, timeout=600)
  for line in r.stdout.splitlines():
    if line.startswith("HBM "):
      return int(line.split()[1]), int(line.split()[2])
  raise RuntimeError(f"no figure from the child: {r.stdout[-500:]} {r.stderr[-500:]}")


def main():
  args = sys.argv[1:]
  if args[:1] == ["--hbm"]:
    hbm_child(args[1], args[2], int(args[3]))
    return
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "erode_timing.txt")
  names = [a for a in args if a in VOLUMES] or ["c1", "c2"]
  lines = [
    f"erode timing: u32 Voronoi, cell (32, 32, 8), erode_border; wall ms = median (min) of {REPS} calls after {WARM} warm-ups, routes alternating in one process",
    "volume | connectivity | bytes in | bytes out | (a) ckl_erode | (b1) decode + torch + encode, sessions per call | (b2) the same, sessions kept | "
    "(b1) / (a) | (b2) / (a) | peak HBM of (a) | peak HBM of (b2), its volume buffer included",
  ]
  for name in names:
    shape = VOLUMES[name]
    sx, sy, sz = shape
    voxels = sx * sy * sz
    binary, runs = make(shape)
    order = crackle_amd.header(binary).markov_model_order
    buf = torch.empty((sz, sy, sx), dtype=torch.int32, device="cuda:0")      # route (b)'s volume, outside the clock
    for conn in (6, 26):
      out = route_a(binary, conn)
      kept = Kept(binary, shape)
      assert route_b1(binary, buf, shape, conn, order) == out and kept(buf, conn, order) == out      # what is timed is right
      t = timed({
        "a": lambda: route_a(binary, conn),
        "b1": lambda: route_b1(binary, buf, shape, conn, order),
        "b2": lambda: kept(buf, conn, order),
      }, f"{name} connectivity {conn}")
      kept.close()
      ms, stage = stage_line(binary, conn)
      nbytes = kernel_bytes(shape, runs)
      hbm_a, hbm_b = hbm("a", name, conn), hbm("b2", name, conn)
      lines.append(f"{name} | {conn} | {len(binary)} | {len(out)} | {t['a'][0]:.2f} ({t['a'][1]:.2f}) | {t['b1'][0]:.2f} ({t['b1'][1]:.2f}) | "
                   f"{t['b2'][0]:.2f} ({t['b2'][1]:.2f}) | {t['b1'][0] / t['a'][0]:.2f}x | {t['b2'][0] / t['a'][0]:.2f}x | "
                   f"{hbm_a[0] / 2**20:.0f} MiB | {hbm_b[0] / 2**20:.0f} MiB")
      print(lines[-1], flush=True)
      lines.append(f"  erode kernels (run labels, terms, keep, planes): {ms:.3f} ms device (median of 5 profiled calls); {nbytes} algorithmic bytes = "
                   f"{nbytes / voxels:.3f} B/voxel ({runs} runs); {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM roofline")
      lines.append(f"  {stage}")
      print(lines[-2], flush=True)
      print(lines[-1], flush=True)
    del buf
    torch.cuda.empty_cache()
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
