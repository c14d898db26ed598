"""Timing of connected_components (ckl_connected_components: the decode pipeline up to the run tables,
k_run_links, the k_cc_* numbering kernels, then the host's stream assembly) at C1 (512 x 512 x 128 u32
Voronoi) and C2 (1024 x 1024 x 512 u32 Voronoi) for connectivity 6 and 26, with contacts() on the same
stream in the same run.  Per call: wall time of the C entry point (session, upload, kernels, copies and
assembly included) and of the Python function.  Kernel times: run it under
rocprofv3 --kernel-trace --stats (k_run_links runs once per call and connectivity, k_run_contacts once
per contacts call).

  python tools/connected_components_timing.py [c1] [c2]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crackle_amd
from crackle_amd import _lib, operations, synth

VOLUMES = {
  "c1": lambda: synth.voronoi_labels((512, 512, 128), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"),
  "c2": lambda: synth.voronoi_labels((1024, 1024, 512), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"),
}
reps = 5
L = _lib.lib()


def _native(binary, connectivity):
  out, n, cnt = C.c_void_p(), C.c_uint64(), C.c_uint64()
  t0 = time.perf_counter()
  rc = L.ckl_connected_components(binary, len(binary), connectivity, 0, C.byref(out), C.byref(n), None, C.byref(cnt))
  t1 = time.perf_counter()
  assert rc == _lib.CKL_OK, _lib.last_error()
  L.ckl_free(out)
  return (t1 - t0) * 1e3, int(cnt.value), int(n.value)


for name in (sys.argv[1:] or list(VOLUMES)):
  binary = bytes(crackle_amd.compress(synth.as_numpy_f(VOLUMES[name]())))
  torch.cuda.synchronize()
  for conn in (6, 26):
    walls = []
    for i in range(reps + 1):
      ms, n_comp, n_bytes = _native(binary, conn)
      if i:      # the first call loads the code objects and grows the pools
        walls.append(ms)
    t0 = time.perf_counter()
    out = crackle_amd.connected_components(binary, connectivity=conn)
    t_py = (time.perf_counter() - t0) * 1e3
    print(f"connected_components {name} connectivity {conn}: {n_comp} components, {len(binary)} -> {n_bytes} bytes; "
          f"ckl_connected_components wall median {np.median(walls):.3f} ms (min {min(walls):.3f}); "
          f"crackle_amd.connected_components wall {t_py:.1f} ms", flush=True)
  walls = []
  for i in range(reps + 1):
    t0 = time.perf_counter()
    pairs, faces = operations._contacts_counts(binary)
    if i:
      walls.append((time.perf_counter() - t0) * 1e3)
  print(f"contacts {name}: {pairs.shape[0]} pairs; _contacts_counts wall median {np.median(walls):.3f} ms (min {min(walls):.3f})", flush=True)
