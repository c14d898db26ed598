"""The sharded codec with the HIP backend: two ranks (gloo) on one GPU encode the halves of a
volume; the merged stream must be the reference's whole-volume stream, byte for byte, and every
rank must decode its z-range.  Exercises what the CPU tests cannot: the device-side re-keying,
the deferred transfer of the crack codes into the page-locked shared mapping and the combined
label-section crc."""
import functools
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from crackle_amd import synth

pytestmark = pytest.mark.gpu
WORLD = 2


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


@functools.lru_cache(maxsize=None)
def _volume(kind):
  """Generated on the GPU (the 2048 x 2048 case takes 12 s on a host core) and kept per process."""
  import torch
  dev = torch.device("cuda", 0)
  if kind == "voronoi":
    return synth.as_numpy_f(synth.voronoi_labels((256, 192, 12), np.uint32, seed=41, cell=(16, 16, 4), device=dev))
  if kind == "wide":
    v = synth.as_numpy_f(synth.voronoi_labels((128, 96, 8), np.uint32, seed=42, cell=(16, 16, 4), modulus=200, device=dev)).copy(order="F")
    v[3:9, 4:7, 6] = 70000      # the widest label lives in the second slab only
    return v
  if kind == "noise":
    return synth.random_labels((96, 80, 6), np.uint32, seed=43, high=2000)
  if kind == "u64":
    # C3's label type: stored width 8, labels above 2^40 and two above 2^63, one per slab
    v = synth.as_numpy_f(synth.voronoi_labels((1024, 64, 8), np.uint64, seed=44, cell=(32, 32, 4), offset=1 << 40, device=dev)).copy(order="F")
    v[5:11, 7:12, 1] = (1 << 63) + 5
    v[200:260, 30:33, 6] = (1 << 64) - 1
    return v
  if kind == "pin_counts":
    # 392 single-component ids of a label beside fewer than 256 pins per label: two-byte counts (the reference writes
    # one-byte counts that overflow); the pillars cross the slab boundary
    v = np.zeros((128, 128, 4), np.uint8, order="F")
    v[::9, ::9, 1:3] = 1
    v[4::9, 4::9, 1:3] = 2
    return v
  if kind == "c4":
    # C4's slice shape: 2048 x 2048 (x_width = y_width = 2, component_width = 4)
    return synth.as_numpy_f(synth.voronoi_labels((2048, 2048, 4), np.uint32, seed=45, cell=(32, 32, 8), device=dev))
  if kind in ("pairs_at_half", "pairs_below_half"):
    # exactly H = voxels // 2 equal linear neighbours (the first IMPERMISSIBLE count) and H - 1: the stretch of equal
    # voxels ends the volume and, at H, begins with the first slab's last voxel, so the pair that straddles the slabs
    # is one of the H (tests/test_threshold_volumes_cpu.py)
    import threshold_volumes
    h = 64 * 33 * 4 // 2
    return threshold_volumes.sharded_volume(h if kind == "pairs_at_half" else h - 1)
  raise ValueError(kind)


CASES = [
  ("voronoi", 0, False, None), ("voronoi", 3, False, None), ("wide", 0, False, None), ("noise", 0, False, None), ("voronoi", 0, True, None),
  ("wide", 0, False, "CKL_SHARDED_LEGACY"),      # unique labels exchanged after the slab encode
  ("voronoi", 0, False, "CKL_TEST_MERGE_FAIL"),  # the in-encode exchange fails on every rank: fallback
  ("u64", 0, False, None), ("u64", 5, False, "CKL_SHARDED_LEGACY"), ("u64", 5, True, None),      # BASELINE.json configs[3]: uint64 labels
  ("voronoi", 5, True, None), ("c4", 5, True, None), ("c4", 5, False, None),                       # configs[4]: pins + markov order 5, 2048 x 2048
  # the pin stage sharded by rows (ckl_pins_rows_*): the whole volume must not be collected on rank 0 ...
  ("voronoi", 0, True, "CKL_TEST_NO_COLLECT"), ("u64", 5, True, "CKL_TEST_NO_COLLECT"), ("c4", 5, True, "CKL_TEST_NO_COLLECT"),
  # ... unless asked for, or when the chosen pins' id lists pass their budget (here: one entry)
  ("voronoi", 5, True, "CKL_PINS_ON_ROOT"), ("voronoi", 0, True, "CKL_PIN_IDS_BUDGET"),
  ("pin_counts", 0, True, None), ("pin_counts", 0, True, "CKL_TEST_NO_COLLECT"),
  # the crack format on either side of pixel_pairs = voxels // 2, the deciding pair across the slab boundary
  ("pairs_at_half", 0, False, None), ("pairs_below_half", 0, False, None), ("pairs_at_half", 0, True, None),
]
ENVS = ("CKL_SHARDED_LEGACY", "CKL_TEST_MERGE_FAIL", "CKL_TEST_NO_COLLECT", "CKL_PINS_ON_ROOT", "CKL_PIN_IDS_BUDGET")


def _worker(rank, port, q):
  """Both ranks run every case in one process group (a spawn per case costs half a minute of
  imports on a fresh box); each case gets its own codec and its own environment."""
  import torch
  from crackle_amd import distributed as ckd
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=WORLD)
  try:
    dev = torch.device("cuda", 0)
    for index, (kind, order, pins, env) in enumerate(CASES):
      for name in ENVS:
        os.environ.pop(name, None)
      if env:
        os.environ[env] = "1"
      try:
        vol = _volume(kind)
        sx, sy, sz = vol.shape
        szl = sz // WORLD
        signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[vol.dtype.itemsize]
        slab = torch.from_numpy(np.ascontiguousarray(vol[:, :, rank * szl:(rank + 1) * szl].transpose(2, 1, 0)).view(signed)).to(dev)
        codec = ckd.ShardedCodec(ckd.HipBackend(0, zero_copy=True), rank=rank, world=WORLD, device="cpu", compute_device=dev)
        binary = None
        for _ in range(2):      # the second call reuses the shared mapping
          binary = codec.compress(slab, (sx, sy, szl), markov_model_order=order, allow_pins=pins)
        session = codec.open_decoder(binary, (sx, sy, szl))
        back = torch.zeros_like(slab)
        session.run(back)
        torch.cuda.synchronize()
        q.put((rank, index, None if binary is None else bytes(binary), bool(torch.equal(back, slab)), None))
        del session, codec, slab, back
      except Exception as exc:      # reported per case; the other rank would otherwise wait for ever
        q.put((rank, index, None, False, repr(exc)))
        raise
  finally:
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def sharded_results():
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
  for p in procs:
    p.start()
  results = {}
  failed = None
  for _ in range(WORLD * len(CASES)):
    rank, index, binary, ok, err = q.get(timeout=300)
    results[(rank, index)] = (binary, ok, err)
    if err:
      failed = err
      break
  for p in procs:
    p.join(timeout=120 if failed is None else 5)
    if p.is_alive():
      p.terminate()
  if failed is None:
    for p in procs:
      assert p.exitcode == 0
  return results


@pytest.mark.parametrize("index", range(len(CASES)), ids=[f"{k}-m{o}-{'pins' if p else 'flat'}{'-' + e if e else ''}" for k, o, p, e in CASES])
def test_sharded_hip_backend_equals_whole_volume(checker, sharded_results, index):
  kind, order, pins, env = CASES[index]
  for rank in range(WORLD):
    assert (rank, index) in sharded_results, "the ranks stopped before this case"
    assert sharded_results[(rank, index)][2] is None, sharded_results[(rank, index)][2]
  vol = _volume(kind)
  whole = checker.compress(vol, markov_model_order=order, allow_pins=pins)
  if kind == "pin_counts":
    # the checker's stream overflows its counts: the single-process stream instead, read back by the checker
    import crackle_amd
    whole = crackle_amd.compress(vol, allow_pins=True)
    assert np.array_equal(checker.decompress(whole).reshape(vol.shape, order="F"), vol)
  if kind.startswith("pairs_"):
    import crackle_amd
    assert crackle_amd.header(whole).crack_format == (0 if kind == "pairs_at_half" else 1), "the volume left the threshold"
  assert sharded_results[(0, index)][0] == whole, "merged slab streams differ from the whole-volume stream"
  assert sharded_results[(1, index)][0] is None
  assert sharded_results[(0, index)][1] and sharded_results[(1, index)][1], "a rank decoded its z-range wrongly"


# ---- BASELINE.json configs[3] and configs[4] at FULL size, two ranks on the one GPU -----------------
FULL = [
  ("c3_1024x1024x1024_u64", (1024, 1024, 1024), np.uint64, 0, False),
  ("c4_2048x2048x256_u32_pins_m5", (2048, 2048, 256), np.uint32, 5, True),
]


def _full_worker(rank, port, q):
  import hashlib
  import torch
  from crackle_amd import distributed as ckd
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=WORLD)
  try:
    dev = torch.device("cuda", 0)
    for index, (name, (sx, sy, sz), dt, order, pins) in enumerate(FULL):
      szl = sz // WORLD
      off = (1 << 40) if np.dtype(dt).itemsize == 8 else 0
      slab = synth.voronoi_labels((sx, sy, sz), dt, seed=2, device=dev, offset=off, z_range=(rank * szl, (rank + 1) * szl))
      codec = ckd.ShardedCodec(ckd.HipBackend(0, zero_copy=True), rank=rank, world=WORLD, device="cpu", compute_device=dev)
      if pins:
        os.environ["CKL_TEST_NO_COLLECT"] = "1"      # the pin stage works on rows: no rank may ask for the whole volume
      binary = codec.compress(slab, (sx, sy, szl), markov_model_order=order, allow_pins=pins)
      os.environ.pop("CKL_TEST_NO_COLLECT", None)
      digest = None if binary is None else (len(binary), hashlib.sha256(binary.view() if hasattr(binary, "view") else bytes(binary)).hexdigest())
      session = codec.open_decoder(binary, (sx, sy, szl))
      back = torch.empty_like(slab)
      session.run(back)
      torch.cuda.synchronize()
      q.put((rank, index, digest, bool(torch.equal(back, slab))))
      session.close()
      del session, codec, slab, back, binary
      torch.cuda.empty_cache()
  finally:
    dist.destroy_process_group()


def test_sharded_full_size_configs_equal_the_single_process_stream():
  """1024 x 1024 x 1024 uint64 and 2048 x 2048 x 256 uint32 with pins + markov order 5, each as two
  z-slabs on two ranks: the merged stream must be, byte for byte, the stream one process writes for
  the whole volume (whose slabs are pinned to the reference's sha256 in tests/test_gpu_strips.py),
  and every rank must decode its half."""
  import hashlib
  import torch
  from crackle_amd import distributed as ckd
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_full_worker, args=(r, port, q)) for r in range(WORLD)]
  for p in procs:
    p.start()
  results = {}
  for _ in range(WORLD * len(FULL)):
    rank, index, digest, ok = q.get(timeout=900)
    results[(rank, index)] = (digest, ok)
  for p in procs:
    p.join(timeout=120)
    assert p.exitcode == 0
  dev = torch.device("cuda", 0)
  be = ckd.HipBackend(0, zero_copy=True)
  import json
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest_xl.json")) as f:
    xl = json.load(f)
  for index, (name, (sx, sy, sz), dt, order, pins) in enumerate(FULL):
    off = (1 << 40) if np.dtype(dt).itemsize == 8 else 0
    vol = synth.voronoi_labels((sx, sy, sz), dt, seed=2, device=dev, offset=off)
    whole = be.encode(vol, (sx, sy, sz), pins, True, order, None)
    want = (len(whole), hashlib.sha256(whole.view() if hasattr(whole, "view") else bytes(whole)).hexdigest())
    del vol, whole
    torch.cuda.empty_cache()
    assert results[(0, index)][0] == want, name
    if name in xl:      # the reference's own sha256 for the whole volume (tests/gen_golden.py --xl)
      assert want == (xl[name]["length"], xl[name]["sha256"]), name
    assert results[(1, index)][0] is None
    assert results[(0, index)][1] and results[(1, index)][1], name


# ---- the row-sharded pin stage over four ranks (rows and slices that do not divide evenly) ------------------------
def _pins4_worker(rank, world, port, q):
  import torch
  from crackle_amd import distributed as ckd
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  os.environ["CKL_TEST_NO_COLLECT"] = "1"
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    dev = torch.device("cuda", 0)
    out = []
    for shape, dt, order, cell in (((190, 150, 12), np.uint32, 0, (16, 16, 4)), ((64, 3, 8), np.uint16, 2, (8, 2, 2)), ((130, 97, 20), np.uint64, 5, (16, 16, 4))):
      sx, sy, sz = shape
      szl = sz // world
      off = (1 << 40) if np.dtype(dt).itemsize == 8 else 0
      slab = synth.voronoi_labels(shape, dt, seed=77, device=dev, offset=off, cell=cell, z_range=(rank * szl, (rank + 1) * szl))
      codec = ckd.ShardedCodec(ckd.HipBackend(0, zero_copy=True), rank=rank, world=world, device="cpu", compute_device=dev)
      binary = codec.compress(slab, (sx, sy, szl), markov_model_order=order, allow_pins=True)
      session = codec.open_decoder(binary, (sx, sy, szl))
      back = torch.zeros_like(slab)
      session.run(back)
      torch.cuda.synchronize()
      out.append((None if binary is None else bytes(binary), bool(torch.equal(back, slab))))
      session.close()
    q.put((rank, out))
  except Exception as exc:      # the other ranks would wait in a collective for ever: the parent ends them
    q.put((rank, repr(exc)))
    raise
  finally:
    dist.destroy_process_group()


def test_pin_stage_by_rows_over_four_ranks(checker):
  """Four HIP ranks on the one GPU (gloo): 150 and 97 rows over four ranks (38 / 37 and 25 / 24), three rows
  over four ranks (one rank holds none), uint64 labels; merged bytes against the reference's whole-volume stream."""
  world = 4
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_pins4_worker, args=(r, world, port, q)) for r in range(world)]
  for p in procs:
    p.start()
  got = {}
  for _ in range(world):
    rank, res = q.get(timeout=240)
    if isinstance(res, str):
      for p in procs:
        p.terminate()
      pytest.fail(f"rank {rank}: {res}")
    got[rank] = res
  for p in procs:
    p.join(timeout=120)
    assert p.exitcode == 0
  cases = (((190, 150, 12), np.uint32, 0, (16, 16, 4)), ((64, 3, 8), np.uint16, 2, (8, 2, 2)), ((130, 97, 20), np.uint64, 5, (16, 16, 4)))
  for i, (shape, dt, order, cell) in enumerate(cases):
    off = (1 << 40) if np.dtype(dt).itemsize == 8 else 0
    whole = synth.as_numpy_f(synth.voronoi_labels(shape, dt, seed=77, offset=off, cell=cell))
    want = checker.compress(whole, markov_model_order=order, allow_pins=True)
    assert got[0][i][0] == want, (shape, dt, order)
    for r in range(world):
      assert got[r][i][1], (r, shape)
