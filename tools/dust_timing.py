"""Timing of dust (ckl_dust: the decode pipeline up to the run tables, k_run_links, k_cc_voxels, the label edit, the
host's stream assembly; no voxel anywhere) at C1 (512 x 512 x 128 u32 Voronoi) and C2 (1024 x 1024 x 512 u32
Voronoi), connectivity 6 and 26, threshold = the median component size, against the route a user had before:

  (a)   ckl_dust(stream): one call, host stream in, host stream out (the edited labels around the input's cracks)
  (a+r) recompress(dust(stream)): the same and the re-encode that removes the cracks of what was removed
  (b)   connected_components(stream, return_mapping=True), voxel_counts of the result, both streams decoded into
        device tensors (ckl_decoder_create + ckl_decoder_run per call: the component stream is new every time), the
        voxels of the small ids zeroed with torch, the volume encoded again (ckl_encoder_run, the session kept).
        The two 4-byte volumes and the mask are allocated once, outside the clock.

(b) ends re-encoded, so (a+r) is its like; (a) alone leaves the false boundaries in.  One process, the routes
alternating, WARM warm-ups, median and minimum of REPS, every round printed.

Kernel times are not taken here: `--kernels` only runs ckl_dust a few times per volume and connectivity, for a
separate `rocprofv3 --kernel-trace --stats -- python tools/dust_timing.py --kernels c1 c2` (k_run_links and
k_cc_voxels run once per call).

  python tools/dust_timing.py [--kernels] [c1] [c2] [--out FILE, default profiles/dust_timing.txt]"""
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

WARM, REPS = 3, 12
VOLUMES = {
  "c1": ((512, 512, 128), lambda: synth.voronoi_labels((512, 512, 128), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")),
  "c2": ((1024, 1024, 512), lambda: synth.voronoi_labels((1024, 1024, 512), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0")),
}
L = _lib.lib()


def route_a(binary, threshold, conn):
  out, n, removed = C.c_void_p(), C.c_uint64(), C.c_uint64()
  assert L.ckl_dust(binary, len(binary), threshold, conn, 0, 0, C.byref(out), C.byref(n), C.byref(removed)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value), int(removed.value)
  finally:
    L.ckl_free(out)


def _decode(binary, vol):
  dec = C.c_void_p()
  assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(dec)) == _lib.CKL_OK, _lib.last_error()
  try:
    assert L.ckl_decoder_run(dec, vol.data_ptr(), vol.numel() * 4, 0, 0) == _lib.CKL_OK, _lib.last_error()
  finally:
    L.ckl_decoder_destroy(dec)


def route_b(binary, threshold, conn, shape, enc, vol, ids, order):
  ccl, mapping = crackle_amd.connected_components(binary, connectivity=conn, return_mapping=True)
  counts = crackle_amd.voxel_counts(ccl)
  small = torch.zeros(len(mapping) + 1, dtype=torch.bool)
  for i, c in counts.items():
    if i and c < threshold:
      small[i] = True
  _decode(binary, vol)
  _decode(ccl, ids)
  vol.masked_fill_(small.to("cuda:0").index_select(0, ids), 0)
  out, n = C.c_void_p(), C.c_uint64()
  sx, sy, sz = shape
  assert L.ckl_encoder_run(enc, vol.data_ptr(), sx, sy, sz, 0, 1, order, 0, 1, 0, None, C.byref(out), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
  try:
    return C.string_at(out.value, n.value)
  finally:
    L.ckl_free(out)


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


def main():
  args = sys.argv[1:]
  kernels_only = "--kernels" in args
  path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "dust_timing.txt")
  names = [a for a in args if a in VOLUMES] or list(VOLUMES)
  lines = [
    f"dust timing: u32 Voronoi, cell (32, 32, 8), threshold = median component size; wall ms = median (min) of {REPS} calls after {WARM} warm-ups, routes alternating in one process",
    "volume | connectivity | threshold | components removed / all | bytes in | bytes out of (a) | (a) ckl_dust | (a+r) recompress(dust) | (b) components + counts + 2 decodes + torch + encode | (b) / (a) | (b) / (a+r)",
  ]
  for name in names:
    shape, make = VOLUMES[name]
    binary = bytes(crackle_amd.compress(synth.as_numpy_f(make())))
    torch.cuda.synchronize()
    order = crackle_amd.header(binary).markov_model_order
    n_vox = shape[0] * shape[1] * shape[2]
    for conn in (6, 26):
      ccl = crackle_amd.connected_components(binary, connectivity=conn)
      sizes = np.array([c for i, c in crackle_amd.voxel_counts(ccl).items() if i], dtype=np.int64)
      threshold = int(np.median(sizes))
      if kernels_only:
        for _ in range(4):
          route_a(binary, threshold, conn)
        continue
      enc = C.c_void_p()
      assert L.ckl_encoder_create(*shape, 4, 0, C.byref(enc)) == _lib.CKL_OK, _lib.last_error()
      vol = torch.empty((n_vox,), dtype=torch.int32, device="cuda:0")
      ids = torch.empty((n_vox,), dtype=torch.int32, device="cuda:0")
      out, removed = route_a(binary, threshold, conn)
      assert removed == int(np.count_nonzero(sizes < threshold))
      # what is timed is right: the two routes end with the same bytes
      clean = crackle_amd.recompress(out)
      assert route_b(binary, threshold, conn, shape, enc, vol, ids, order) == clean
      t = timed({
        "a": lambda: route_a(binary, threshold, conn),
        "a+r": lambda: crackle_amd.recompress(route_a(binary, threshold, conn)[0]),
        "b": lambda: route_b(binary, threshold, conn, shape, enc, vol, ids, order),
      }, f"{name} connectivity {conn}")
      L.ckl_encoder_destroy(enc)
      del vol, ids
      lines.append(f"{name} | {conn} | {threshold} | {removed} / {sizes.size} | {len(binary)} | {len(out)} | {t['a'][0]:.2f} ({t['a'][1]:.2f}) | "
                   f"{t['a+r'][0]:.2f} ({t['a+r'][1]:.2f}) | {t['b'][0]:.2f} ({t['b'][1]:.2f}) | {t['b'][0] / t['a'][0]:.2f}x | {t['b'][0] / t['a+r'][0]:.2f}x")
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
