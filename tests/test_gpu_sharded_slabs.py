"""The sharded codec with the HIP backend on slabs of unequal depth, empty slabs included, and at the widths of the
merged label list: four ranks (gloo) on one GPU run the table of tests/sharded_slabs.py in one spawn.  The merged
stream must be the checker's whole-volume stream, byte for byte, and every rank must decode exactly its own slab
into a device buffer whose surroundings stay untouched.

On the device this reaches what tests/test_sharded_slabs_cpu.py cannot: k_flat_section writing keys against a caller's
list that is longer than the slab's own (or than the slab has components), the hand-over of the hash pass's unsorted
labels to the exchange, the re-keying in torch after the encode, and the encoder's callback meeting a rank that has
no encoder to call it from."""
import os

import numpy as np
import pytest

import sharded_slabs as S
from decode_session import GUARD, PATTERN

pytestmark = pytest.mark.gpu
WORLD = S.WORLD
CASES = S.CASES


def _worker(rank, port, q):
  """Every rank runs every case in one process group; each case gets its own codec and its own environment.  A
  failure is reported for its case and ends the rank: the parent ends the others, which would wait for it."""
  import torch
  import torch.distributed as dist
  from crackle_amd import distributed as ckd
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  torch.set_num_threads(1)      # four ranks of small host tensor work: thread pools only get in each other's way
  dist.init_process_group("gloo", rank=rank, world_size=WORLD)
  try:
    dev = torch.device("cuda", 0)
    for index, (name, depths, order, pins, env) in enumerate(CASES):
      for switch in S.ENVS:
        os.environ.pop(switch, None)
      if env:
        os.environ[env] = "1"
      try:
        vol = S.volume(name)
        sx, sy, _ = vol.shape
        depth = depths[rank]
        signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[vol.dtype.itemsize]
        slab = torch.from_numpy(np.ascontiguousarray(S.slab(vol, depths, rank).transpose(2, 1, 0)).view(signed)).to(dev)
        codec = ckd.ShardedCodec(ckd.HipBackend(0, zero_copy=True), rank=rank, world=WORLD, device="cpu", compute_device=dev)
        binary = None
        for _ in range(2):      # the second call reuses the shared mapping, sized by the case before
          binary = codec.compress(slab, (sx, sy, depth), markov_model_order=order, allow_pins=pins)
        session = codec.open_decoder(binary, (sx, sy, depth))
        nbytes = slab.numel() * slab.element_size()
        buf = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=dev)
        out = buf[GUARD:GUARD + nbytes]
        session.run(out)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        guards = bool((host[:GUARD] == PATTERN).all() and (host[GUARD + nbytes:] == PATTERN).all())
        same = bool(np.array_equal(host[GUARD:GUARD + nbytes], slab.cpu().numpy().reshape(-1).view(np.uint8)))
        q.put((rank, index, None if binary is None else bytes(binary), same, guards, None))
        session.close()
        del session, codec, slab, buf, out
      except Exception as exc:
        q.put((rank, index, None, False, False, repr(exc)))
        raise
  finally:
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def sharded_results():
  return S.run_table(_worker, len(CASES), 300)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[S.case_id(c) for c in CASES])
def test_sharded_hip_backend_on_uneven_slabs(checker, sharded_results, index):
  results, stopped = sharded_results
  name, depths, order, pins, env = CASES[index]
  for rank in range(WORLD):
    assert (rank, index) in results, f"the ranks stopped before this case: {stopped}"
    assert results[(rank, index)][3] is None, results[(rank, index)][3]
  vol = S.volume(name)
  whole = checker.compress(vol, markov_model_order=order, allow_pins=pins)
  if name in S.CRACK_FORMAT:
    import crackle_amd
    assert crackle_amd.header(whole).crack_format == S.CRACK_FORMAT[name], "the volume left the threshold"
  assert results[(0, index)][0] == whole, "merged slab streams differ from the whole-volume stream"
  for rank in range(1, WORLD):
    assert results[(rank, index)][0] is None
  assert all(results[(rank, index)][2] for rank in range(WORLD)), "bytes around a rank's decoded slab were written"
  wrong = [rank for rank in range(WORLD) if not results[(rank, index)][1]]
  assert not wrong, f"ranks {wrong} decoded something else than their slabs"
