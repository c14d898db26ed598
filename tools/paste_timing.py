"""Timing of paste (ckl_paste: the slices of the box's z-range decoded into a slab in HBM, k_paste_box, the encoder on
that slab, zsplit / zstack on the host) on the 1024 x 1024 x 512 u32 Voronoi volume of the bench, against the same
edit composed from the functions the package had before it:

  (a) crackle_amd.paste(stream, box, data)
  (b) decompress_range(stream, z0, z1) -> numpy assignment -> compress(slab) -> zsplit / zstack

Cases: a 128^3 box in the middle of the volume (a slab of 128 slices, 512 MiB, which (b) takes across the link once
in each direction) and a whole plane of one slice (4 MiB).  Per case both routes alternate in one process, WARM warm-up
rounds, then the median and minimum wall time of REPS rounds.  Both routes must return the same bytes (the edits keep
the volume's crack format, and the stream is at markov order 0).

The parent process only starts children, each under a time limit of its own: one that writes the stream to
tool_out/, then one per case; it stops at the first that fails.

  python tools/paste_timing.py [output file, default profiles/paste_timing.txt]"""
import os
import subprocess
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 12
SHAPE = (1024, 1024, 512)
STREAM = os.path.join(ROOT, "tool_out", "paste_timing_stream.ckl")
CASES = {
  "128^3 box in the middle": (448, 576, 448, 576, 192, 320),
  "whole plane of one slice": (0, 1024, 0, 1024, 256, 257),
}
LIMIT_STREAM_S, LIMIT_CASE_S = 420, 420


def make_stream():
  import crackle_amd
  from crackle_amd import synth
  vol = synth.as_numpy_f(synth.voronoi_labels(SHAPE, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"))
  binary = bytes(crackle_amd.compress(vol))
  os.makedirs(os.path.dirname(STREAM), exist_ok=True)
  with open(STREAM, "wb") as f:
    f.write(binary)
  print(f"stream of {len(binary)} bytes", flush=True)


def composed(binary, box, data):
  """The edit by the functions the package had before paste.  (The two ranges come from zsplit's range helper, as
  paste takes them: the public zsplit(binary, z) would also cut the parts that are thrown away.)"""
  import crackle_amd
  from crackle_amd import operations
  x0, x1, y0, y1, z0, z1 = box
  slab = crackle_amd.decompress_range(binary, z0, z1)
  slab[x0:x1, y0:y1, :] = data
  middle = crackle_amd.compress(slab)
  before = operations._zrange(binary, 0, z0) if z0 > 0 else b""
  after = operations._zrange(binary, z1, SHAPE[2]) if z1 < SHAPE[2] else b""
  return crackle_amd.zstack([part for part in (before, middle, after) if part])


def run_case(name):
  import torch
  import crackle_amd
  from crackle_amd import synth
  box = CASES[name]
  x0, x1, y0, y1, z0, z1 = box
  with open(STREAM, "rb") as f:
    binary = f.read()
  data = np.asfortranarray(synth.as_numpy_f(synth.voronoi_labels((x1 - x0, y1 - y0, z1 - z0), np.uint32, seed=3, cell=(32, 32, 8))))
  idx = np.s_[x0:x1, y0:y1, z0:z1]
  calls = {"a": lambda: crackle_amd.paste(binary, idx, data), "b": lambda: composed(binary, box, data)}
  out = calls["a"]()
  assert out == calls["b"](), "the two routes disagree"
  assert np.array_equal(crackle_amd.cutout(out, idx), data)
  times = {k: [] for k in calls}
  for i in range(WARM + REPS):
    for k, f in calls.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      f()
      torch.cuda.synchronize()
      if i >= WARM:
        times[k].append((time.perf_counter() - t0) * 1e3)
  a, b = times["a"], times["b"]
  slab_mib = SHAPE[0] * SHAPE[1] * (z1 - z0) * 4 / 2**20
  print(f"RESULT {name} | {data.nbytes / 2**20:.0f} | {slab_mib:.0f} | {len(out)} | {np.median(a):.2f} ({min(a):.2f}) | {np.median(b):.2f} ({min(b):.2f}) | {np.median(b) / np.median(a):.2f}x", flush=True)
  # every round, in the order taken: the spread is part of the result
  print(f"RESULT   rounds (a): {' '.join(f'{t:.1f}' for t in a)}", flush=True)
  print(f"RESULT   rounds (b): {' '.join(f'{t:.1f}' for t in b)}", flush=True)


def child(args, limit):
  cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
  done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
  sys.stdout.write(done.stdout)
  if done.returncode != 0:
    raise SystemExit(f"{' '.join(args)}: exit status {done.returncode}; nothing more is started")
  return done.stdout


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paste_timing.txt")
  lines = [
    f"paste timing: {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} uint32 Voronoi, {child(['--make-stream'], LIMIT_STREAM_S).strip()}, markov order 0; "
    f"wall ms = median (min) of {REPS} calls after {WARM} warm-ups, the two routes alternating in one process per case",
    "(a) paste(); (b) decompress_range -> numpy assignment -> compress -> zsplit / zstack; both return the same bytes",
    "case | box MiB | slab MiB | bytes out | (a) wall ms | (b) wall ms | (b) / (a)",
  ]
  for name in CASES:
    out = child(["--case", name], LIMIT_CASE_S)
    lines += [line[len("RESULT "):] for line in out.splitlines() if line.startswith("RESULT ")]
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


if __name__ == "__main__":
  if sys.argv[1:2] == ["--make-stream"]:
    make_stream()
  elif sys.argv[1:2] == ["--case"]:
    run_case(sys.argv[2])
  else:
    main()
