"""Timing of dilate (ckl_dilate: the decoder's run tables -> k_erode_run_labels, k_dilate_nonzero, k_dilate_gain,
k_dilate_mode, k_dilate_planes -> the encoder's crack and label stages, no voxel anywhere) at C1 (512 x 512 x 128 u32
Voronoi) and C2 (1024 x 1024 x 512 u32 Voronoi) with every label that is a multiple of 5 set to background,
connectivity 6 and 26:

  (a)  ckl_dilate(stream): one call, host stream in, host stream out
  (r)  ckl_recompress(stream) of the same stream: the same road without the dilate kernels, so (a) - (r) is what
       dilation costs (its kernels, the host's wait for the gained count, and an encoder that sees another volume)

Same process, alternating, WARM warm-ups, median, minimum and maximum of REPS.  The device time of the dilate kernels
together (HIP events around them, the host's wait for the gained count between k_dilate_gain and k_dilate_mode
included) and the gained count are read from the [ckl dilate host ms] line (CKL_PROFILE) of separate calls; the
algorithmic bytes come from the shapes, the run count and the gained count.  The first result of (a) is checked against
torch's own dilation of the volume where that is cheap (C1).

  python tools/dilate_timing.py [c1] [c2] [--out FILE, default profiles/dilate_timing.txt]
                                [--record LABEL=FILE ...] [--records-only]

--record appends the "(a)" column of outputs of tools/recompress_timing.py and tools/erode_timing.py, taken with the
library before this change (twice: the run-to-run spread) and after it: k_component_labels_from_runs gained a branch.
With --records-only nothing is timed and the records are added to the file that is there."""
import ctypes as C
import itertools
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

WARM, REPS = 3, 12
VOLUMES = {"c1": (512, 512, 128), "c2": (1024, 1024, 512)}
ZERO_EVERY = 5
HBM_PEAK = 8.0e12      # bytes per second
L = _lib.lib()


def offsets(conn):
  reach = {6: 1, 18: 2, 26: 3}[conn]
  return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, o)) <= reach]


def _call(fn, binary, *args):
  out, n = C.c_void_p(), C.c_uint64()
  assert fn(binary, len(binary), *args, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def route_a(binary, conn):
  return _call(L.ckl_dilate, binary, conn, 0, -1, 0)


def route_r(binary):
  return _call(L.ckl_recompress, binary, -1, 0)


def torch_dilate(vol, conn):
  """vol: (sz, sy, sx) int32 on the device.  The mode with ties to the smallest, by counting every candidate."""
  pad = torch.nn.functional.pad(vol, (1, 1, 1, 1, 1, 1))
  sz, sy, sx = vol.shape
  views = [pad[1 + dz:1 + dz + sz, 1 + dy:1 + dy + sy, 1 + dx:1 + dx + sx] for dx, dy, dz in offsets(conn)]
  best = torch.zeros_like(vol)
  best_n = torch.zeros_like(vol)
  for cand in views:
    n = torch.zeros_like(vol)
    for other in views:
      n += (other == cand).to(vol.dtype)
    better = (cand != 0) & ((n > best_n) | ((n == best_n) & (cand < best)))
    best = torch.where(better, cand, best)
    best_n = torch.where(better, n, best_n)
  return torch.where(vol != 0, vol, best)


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


def stage_line(binary, conn, reps=5):
  """Device time of the dilate kernels and the gained count, from the [ckl dilate host ms] lines of `reps` profiled calls."""
  sys.stderr.flush()
  saved = os.dup(2)
  vals, lines, gained = [], [], set()
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
      if line.startswith("[ckl dilate host ms]"):
        fields = dict(w.split("=") for w in line.split()[4:])
        lines.append(line)
        vals.append(float(fields["k_dilate_device"]))
        gained.add(int(fields["gained"]))
  assert len(vals) == reps and len(gained) == 1
  return float(np.median(vals)), min(vals), max(vals), gained.pop(), lines[-1]


def kernel_bytes(shape, runs, gained):
  """What the kernels' algorithm moves, from the shapes.  Per 32-pixel word: k_dilate_nonzero reads the decoder's V word
  and word_base (8 B) and writes N (4 B); k_dilate_gain reads N (4 B; the words of the neighbour rows are the
  neighbour threads' own) and writes gain and gain_off (12 B); k_dilate_mode reads gain and gain_off (12 B);
  k_dilate_planes reads V, word_base, gain and gain_off (20 B) and writes V and H (8 B): 68 B.  Per run:
  k_erode_run_labels reads the component id and its label (12 B) and writes the label (8 B), k_dilate_nonzero and
  k_dilate_planes read it (16 B): 36 B.  Per gained pixel: k_dilate_mode writes its label (8 B) and k_dilate_planes reads
  it for its own row and for the row below (16 B): 24 B; the neighbour rows' words and labels that k_dilate_mode looks up
  were read by the kernels before it and are counted as cache hits."""
  sx, sy, sz = shape
  words = (sx + 31) // 32 * sy * sz
  return words * 68 + runs * 36 + gained * 24


def make(shape):
  dvol = synth.voronoi_labels(shape, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")      # (sz, sy, sx)
  ivol = dvol.view(torch.int32)      # the same memory (the labels are far below 2^31): torch has no arithmetic on uint32
  ivol[ivol % ZERO_EVERY == 0] = 0
  runs = int(shape[1] * shape[2] + torch.count_nonzero(ivol[:, :, 1:] != ivol[:, :, :-1]).item())
  background = float(torch.count_nonzero(ivol == 0).item()) / ivol.numel()
  binary = bytes(crackle_amd.compress(synth.as_numpy_f(dvol)))
  return binary, runs, background, ivol


def recorded(spec):
  """LABEL=FILE: the "(a)" column of a recompress_timing or erode_timing output."""
  label, path = spec.split("=", 1)
  rows, col = [], None
  for line in open(path).read().splitlines():
    cells = [c.strip() for c in line.split("|")]
    if col is None:
      hits = [i for i, c in enumerate(cells) if c.startswith("(a) ckl_")]
      if hits:
        col, what = hits[0], cells[hits[0]]
      continue
    if len(cells) > col and not line.startswith(" "):
      rows.append(" ".join(cells[:2 if "erode" in what else 1]) + ": " + cells[col])
  return f"  {label}: {what}, median (min) ms: " + "; ".join(rows)


def main():
  args = sys.argv[1:]
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "dilate_timing.txt")
  records = [args[i + 1] for i, a in enumerate(args) if a == "--record"]
  names = [a for a in args if a in VOLUMES] or ["c1", "c2"]
  if "--records-only" in args:      # the timing file is there already: only the records are added to it
    names, lines = [], open(path).read().splitlines()
  else:
    lines = []
  lines += [] if "--records-only" in args else [
    f"dilate timing: u32 Voronoi, cell (32, 32, 8), every label that is a multiple of {ZERO_EVERY} background; wall ms = median (min - max) of {REPS} calls "
    f"after {WARM} warm-ups, routes alternating in one process",
    "volume | connectivity | background | bytes in | bytes out | gained voxels | (a) ckl_dilate | (r) ckl_recompress of the same stream | (a) - (r)",
  ]
  for name in names:
    shape = VOLUMES[name]
    voxels = shape[0] * shape[1] * shape[2]
    binary, runs, background, ivol = make(shape)
    for conn in (6, 26):
      out = route_a(binary, conn)
      if name == "c1":      # what is timed is right
        want = torch_dilate(ivol, conn)
        assert out == bytes(crackle_amd.compress(synth.as_numpy_f(want.view(torch.uint32))))
        del want
      assert route_r(binary) == binary
      t = timed({"a": lambda: route_a(binary, conn), "r": lambda: route_r(binary)}, f"{name} connectivity {conn}")
      ms, ms_min, ms_max, gained, stage = stage_line(binary, conn)
      nbytes = kernel_bytes(shape, runs, gained)
      lines.append(f"{name} | {conn} | {100 * background:.1f} % | {len(binary)} | {len(out)} | {gained} ({100 * gained / voxels:.2f} %) | "
                   f"{t['a'][0]:.2f} ({t['a'][1]:.2f} - {t['a'][2]:.2f}) | {t['r'][0]:.2f} ({t['r'][1]:.2f} - {t['r'][2]:.2f}) | {t['a'][0] - t['r'][0]:.2f}")
      print(lines[-1], flush=True)
      lines.append(f"  dilate kernels (run labels, nonzero, gain, the host's wait for the count, mode, planes): {ms:.3f} ms device (median of 5 profiled calls, "
                   f"{ms_min:.3f} - {ms_max:.3f}); {nbytes} algorithmic bytes = {nbytes / voxels:.3f} B/voxel ({runs} runs); "
                   f"{nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM roofline")
      lines.append(f"  {stage}")
      print(lines[-2], flush=True)
      print(lines[-1], flush=True)
    del ivol
    torch.cuda.empty_cache()
  if records:
    lines.append("recompress and erode before and after this change (k_component_labels_from_runs gained a branch):")
    lines += [recorded(r) for r in records]
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  main()
