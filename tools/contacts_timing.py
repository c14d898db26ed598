"""Timing of contacts (ckl_decoder_contacts: the decode pipeline up to the run tables, then
k_run_contacts and k_contacts_compact) at C1 (512 x 512 x 128 u32 Voronoi), C2 (1024 x 1024 x 512 u32
Voronoi) and one noise volume.  Per call: wall time of ckl_decoder_contacts on a session made once,
the device span the session reports (ckl_decoder_last_timing: from the first kernel to the last
copy, the passes' host synchronisations included) and the wall time of crackle_amd.contacts (session,
upload and the Python dict included).  Kernel times: run it under rocprofv3 --kernel-trace --stats."""
import ctypes as C
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import crackle_amd
from crackle_amd import _lib, synth

VOLUMES = {
  "c1": lambda: synth.voronoi_labels((512, 512, 128), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"),
  "c2": lambda: synth.voronoi_labels((1024, 1024, 512), np.uint32, seed=2, cell=(32, 32, 8), device="cuda:0"),
  "noise": lambda: synth.random_labels_device((512, 512, 32), np.uint32, seed=5, high=2000, device="cuda:0"),
}
reps = 5
L = _lib.lib()
for name in (sys.argv[1:] or list(VOLUMES)):
  binary = bytes(crackle_amd.compress(synth.as_numpy_f(VOLUMES[name]())))
  torch.cuda.synchronize()
  handle = C.c_void_p()
  assert L.ckl_decoder_create(binary, len(binary), 0, -1, 0, C.byref(handle)) == _lib.CKL_OK, _lib.last_error()
  L.ckl_decoder_set_stage_events(handle, 0)
  walls, spans = [], []
  for i in range(reps + 1):
    pp, fp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    t0 = time.perf_counter()
    assert L.ckl_decoder_contacts(handle, C.byref(pp), C.byref(fp), C.byref(n)) == _lib.CKL_OK, _lib.last_error()
    t1 = time.perf_counter()
    span = C.c_float()
    L.ckl_decoder_last_timing(handle, C.byref(span), None)
    L.ckl_free(pp)
    L.ckl_free(fp)
    if i:      # the first call loads the code objects and grows the pools
      walls.append((t1 - t0) * 1e3)
      spans.append(span.value)
  L.ckl_decoder_destroy(handle)
  t0 = time.perf_counter()
  areas = crackle_amd.contacts(binary)
  t_py = (time.perf_counter() - t0) * 1e3
  print(f"contacts {name}: {n.value} pairs; ckl_decoder_contacts wall median {np.median(walls):.3f} ms (min {min(walls):.3f}), "
        f"device span median {np.median(spans):.3f} ms (min {min(spans):.3f}); crackle_amd.contacts wall {t_py:.1f} ms ({len(areas)} pairs)", flush=True)
