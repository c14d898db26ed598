"""Timing of recompress (ckl_recompress: the decoder's run tables -> k_label_planes_from_runs -> the encoder's crack
and label stages, no voxel anywhere) on the 1024 x 1024 x 512 u32 Voronoi stream of the bench, as it is and after a
remap that merges labels (v % 50), against the only route there was before: ckl_decoder_run painting the volume into a
device buffer and ckl_encoder_run from that buffer.

  (a)  ckl_recompress(stream): one call, host stream in, host stream out
  (b1) the same one-shot shape by the old route: ckl_decoder_create + ckl_decoder_run + ckl_encoder_create +
       ckl_encoder_run, sessions made and destroyed per call, the 2 GiB volume buffer allocated once outside the clock
  (b2) the old route with both sessions made once, as bench.py drives them: ckl_decoder_run + ckl_encoder_run only

Same process, alternating, WARM warm-ups, median and minimum of REPS.  The device time of k_label_planes_from_runs is
read from the [ckl recompress host ms] line (CKL_PROFILE) of separate calls; its algorithmic bytes come from the shapes
and the run count of the volume.

  python tools/recompress_timing.py [output file, default profiles/recompress_timing.txt]"""
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

WARM, REPS = 3, 20
SHAPE = (1024, 1024, 512)
HBM_PEAK = 8.0e12      # bytes per second


def route_a(binary):
  return crackle_amd.recompress(binary)


def _paint(L, dec, vol):
  assert L.ckl_decoder_run(dec, vol.data_ptr(), vol.numel() * 4, 0, 0) == _lib.CKL_OK, _lib.last_error()


def _encode(L, enc, vol, order):
  out, n = C.c_void_p(), C.c_uint64()
  sx, sy, sz = SHAPE
  assert L.ckl_encoder_run(enc, vol.data_ptr(), sx, sy, sz, 0, 1, order, 0, 1, 0, None, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


def route_b1(binary, vol, order):
  L = _lib.lib()
  dec, enc = C.c_void_p(), C.c_void_p()
  assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(dec)) == _lib.CKL_OK, _lib.last_error()
  try:
    _paint(L, dec, vol)
  finally:
    L.ckl_decoder_destroy(dec)
  assert L.ckl_encoder_create(*SHAPE, 4, 0, C.byref(enc)) == _lib.CKL_OK, _lib.last_error()
  try:
    return _encode(L, enc, vol, order)
  finally:
    L.ckl_encoder_destroy(enc)


def timed(calls):
  """calls: name -> function; alternating, WARM + REPS rounds: name -> (median ms, min ms)"""
  times = {k: [] for k in calls}
  for i in range(WARM + REPS):
    for k, f in calls.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      f()
      torch.cuda.synchronize()
      if i >= WARM:
        times[k].append((time.perf_counter() - t0) * 1e3)
  return {k: (float(np.median(v)), min(v)) for k, v in times.items()}


def kernel_device_ms(binary, reps=5):
  """k_label_planes_from_runs' device time (HIP events around it), from the stage lines of `reps` profiled calls."""
  sys.stderr.flush()
  saved = os.dup(2)
  vals, lines = [], []
  with tempfile.TemporaryFile(mode="w+b") as tmp:
    os.dup2(tmp.fileno(), 2)
    os.environ["CKL_PROFILE"] = "1"
    try:
      for _ in range(reps):
        crackle_amd.recompress(binary)
    finally:
      del os.environ["CKL_PROFILE"]
      os.dup2(saved, 2)
      os.close(saved)
    tmp.seek(0)
    for line in tmp.read().decode().splitlines():
      if line.startswith("[ckl recompress host ms]"):
        lines.append(line)
        vals.append(float(dict(w.split("=") for w in line.split()[4:])["k_label_planes_from_runs_device"]))
  assert len(vals) == reps
  return float(np.median(vals)), lines[-1]


def kernel_bytes(runs):
  """What the kernel's algorithm moves, from the shapes: per 32-pixel word the decoder's V word and word_base (4 + 4 B)
  and the two plane words it writes (8 B) — the words of the row above come from the cache, the neighbour thread read
  them — and per run the component id and its label (4 + 8 B), fetched by the row itself and by the row below."""
  sx, sy, sz = SHAPE
  words = (sx + 31) // 32 * sy * sz
  return words * 16 + 2 * runs * 12


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "recompress_timing.txt")
  sx, sy, sz = SHAPE
  dvol = synth.voronoi_labels(SHAPE, np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")      # (sz, sy, sx)
  runs = int(sy * sz + torch.count_nonzero(dvol[:, :, 1:] != dvol[:, :, :-1]).item())
  vol = synth.as_numpy_f(dvol)
  plain = bytes(crackle_amd.compress(vol))
  merged_stream = crackle_amd.remap(plain, {int(v): int(v) % 50 for v in crackle_amd.labels(plain)})
  # what is timed is right: the merged stream recompressed is compress() of the merged volume
  want = bytes(crackle_amd.compress(np.asfortranarray(vol % np.uint32(50))))
  assert crackle_amd.recompress(merged_stream) == want and crackle_amd.recompress(plain) == plain
  del vol
  buf = torch.empty((sx * sy * sz,), dtype=torch.int32, device="cuda:0")      # route (b)'s volume
  L = _lib.lib()
  voxels = sx * sy * sz
  lines = [
    f"recompress timing: {sx} x {sy} x {sz} uint32 Voronoi; wall ms = median (min) of {REPS} calls after {WARM} warm-ups, routes alternating in one process",
    f"device memory for the volume: route (a) 0 bytes, route (b) {voxels * 4} bytes ({voxels * 4 / 2**30:.0f} GiB); planes of (a): {2 * kernel_words() * 4 / 2**20:.0f} MiB",
    "stream | bytes in | bytes out | (a) ckl_recompress | (b1) decode + encode, sessions per call | (b2) decode + encode, sessions kept | (b1) / (a) | (b2) / (a)",
  ]
  for name, binary in (("as it is", plain), ("after remap v % 50", merged_stream)):
    order = crackle_amd.header(binary).markov_model_order
    dec, enc = C.c_void_p(), C.c_void_p()
    assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(dec)) == _lib.CKL_OK, _lib.last_error()
    assert L.ckl_encoder_create(sx, sy, sz, 4, 0, C.byref(enc)) == _lib.CKL_OK, _lib.last_error()

    def kept():
      _paint(L, dec, buf)
      return _encode(L, enc, buf, order)

    out = route_a(binary)
    assert route_b1(binary, buf, order) == out and kept() == out
    t = timed({"a": lambda: route_a(binary), "b1": lambda: route_b1(binary, buf, order), "b2": kept})
    L.ckl_decoder_destroy(dec)
    L.ckl_encoder_destroy(enc)
    lines.append(f"{name} | {len(binary)} | {len(out)} | {t['a'][0]:.2f} ({t['a'][1]:.2f}) | {t['b1'][0]:.2f} ({t['b1'][1]:.2f}) | "
                 f"{t['b2'][0]:.2f} ({t['b2'][1]:.2f}) | {t['b1'][0] / t['a'][0]:.2f}x | {t['b2'][0] / t['a'][0]:.2f}x")
    print(lines[-1], flush=True)
    ms, stage = kernel_device_ms(binary)
    nbytes = kernel_bytes(runs)
    lines.append(f"  k_label_planes_from_runs: {ms:.3f} ms device (median of 5 profiled calls); {nbytes} algorithmic bytes = {nbytes / voxels:.3f} B/voxel "
                 f"({runs} runs); {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM roofline")
    lines.append(f"  {stage}")
    print(lines[-2], flush=True)
  text = "\n".join(lines) + "\n"
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, "w") as f:
    f.write(text)
  print(text)


def kernel_words():
  sx, sy, sz = SHAPE
  return (sx + 31) // 32 * sy * sz


if __name__ == "__main__":
  main()
