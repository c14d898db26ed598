"""The sharded codec on slabs of unequal depth, empty slabs included, and at the widths of the merged label list
(tests/sharded_slabs.py), without a GPU: first every volume is pinned to what the table claims of it, then four gloo
ranks run the table with the CPU oracle as their backend.  The merged stream must be the whole-volume stream of the
oracle's encoder, byte for byte, and every rank must decode exactly its own slab."""
import os

import numpy as np
import pytest
import torch.distributed as dist

import sharded_slabs as S
import threshold_volumes

WORLD = S.WORLD


# ---- (a) the volumes are what the table says -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.CLAIMS))
def test_volume_holds_its_claims(checker, name):
  depths, per_slab, merged, crackless, pairs, half = S.CLAIMS[name]
  vol = S.volume(name)
  assert sum(depths) == vol.shape[2]
  got = S.measure(name, depths)
  assert got[0] == per_slab, "distinct labels per slab"
  assert got[1] == merged, "distinct labels of the whole volume"
  assert got[2] == crackless, "slabs without a crack edge"
  assert (got[3], got[4]) == (pairs, half), "pixel_pairs and voxels // 2"
  binary = checker.compress(vol)
  assert np.array_equal(checker.decompress(binary).reshape(vol.shape, order="F"), vol)


def test_claims_cover_every_volume_of_the_table():
  assert {c[0] for c in S.CASES} == set(S.CLAIMS)
  for name, depths, _, _, _ in S.CASES:
    assert len(depths) == WORLD and sum(depths) == S.volume(name).shape[2], (name, depths)


def test_merge_volumes_cross_the_key_widths():
  """Every slab's own list is narrower than the merged one exactly where the names say: 255 | 256 and 65535 | 65536."""
  width = threshold_volumes.byte_width
  want = {"merge200_255": (1, 1), "merge200_256": (1, 2), "merge200_257": (1, 2), "merge40000_65535": (2, 2), "merge40000_65536": (2, 4),
          "merge40000_65537": (2, 4), "merge255_1": (1, 2), "lone_label": (1, 4)}
  assert set(want) == set(S.MERGE_VOLUMES)
  for name, (narrowest, merged_width) in want.items():
    _, per_slab, merged, _, _, _ = S.CLAIMS[name]
    assert (min(width(n) for n in per_slab), width(merged)) == (narrowest, merged_width), name
  # lone_label: the merged list is longer than the one-label slab has components
  assert S.crack_edges(S.volume("lone_label")[:, :, :1]) == 0 and S.CLAIMS["lone_label"][2] > 1


def test_pairs_volumes_decide_across_the_empty_rank():
  """The stretch of equal voxels begins with slice 1's last voxel at H pairs and with slice 2's first at H - 1: with
  depths (2, 0, 2, 0) the deciding pair is the one between rank 0's last voxel and rank 2's first."""
  cut = 64 * 33 * 2
  at, below = (threshold_volumes.flat(S.volume(n)) for n in ("pairs_at_half", "pairs_below_half"))
  assert at[cut - 1] == at[cut] and below[cut - 1] != below[cut]
  assert threshold_volumes.pairs(S.volume("pairs_at_half")) == S.PAIRS_H == S.volume("pairs_at_half").size // 2
  assert threshold_volumes.pairs(S.volume("pairs_below_half")) == S.PAIRS_H - 1


# ---- (b) the table on four gloo ranks with the oracle backend ---------------------------------------------------------
# the switches of the table are read by the HIP backend's roads only: here every (volume, depths, order, pins) once
CPU_CASES = list(dict.fromkeys(c[:4] for c in S.CASES))


def _worker(rank, port, q):
  import sys
  sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
  from oracle_backend import OracleBackend
  from crackle_amd import distributed as ckd
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  import torch
  torch.set_num_threads(1)      # four ranks of small tensor work: thread pools only get in each other's way
  for name in S.ENVS:
    os.environ.pop(name, None)
  dist.init_process_group("gloo", rank=rank, world_size=WORLD)
  try:
    for index, (name, depths, order, pins) in enumerate(CPU_CASES):
      try:
        vol = S.volume(name)
        sx, sy, _ = vol.shape
        slab = S.slab(vol, depths, rank)
        codec = ckd.ShardedCodec(OracleBackend(), rank=rank, world=WORLD, device="cpu")
        binary = codec.compress(slab, (sx, sy, depths[rank]), markov_model_order=order, allow_pins=pins)
        session = codec.open_decoder(binary, (sx, sy, depths[rank]))
        back = np.full(slab.shape, 0xA5, dtype=slab.dtype, order="F")
        session.run(back)
        q.put((rank, index, None if binary is None else bytes(binary), bool(np.array_equal(back, slab)), None))
      except Exception as exc:      # reported per case: the other ranks would wait in a collective for ever
        q.put((rank, index, None, False, repr(exc)))
        raise
    # depths that do not add up to the stream's sz (rank 2 claims a slice too many): ValueError on EVERY rank
    try:
      name, depths = "voronoi10", S.UNEQUAL
      vol = S.volume(name)
      sx, sy, _ = vol.shape
      codec = ckd.ShardedCodec(OracleBackend(), rank=rank, world=WORLD, device="cpu")
      binary = codec.compress(S.slab(vol, depths, rank), (sx, sy, depths[rank]))
      try:
        codec.open_decoder(binary, (sx, sy, depths[rank] + (1 if rank == 2 else 0)))
        verdict = "no error"
      except ValueError as exc:
        verdict = "ValueError: " + str(exc)
      q.put((rank, len(CPU_CASES), verdict, True, None))
    except Exception as exc:
      q.put((rank, len(CPU_CASES), None, False, repr(exc)))
      raise
  finally:
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def oracle_results():
  return S.run_table(_worker, len(CPU_CASES) + 1, 180)


@pytest.mark.parametrize("index", range(len(CPU_CASES)), ids=[S.case_id(c + (None,)) for c in CPU_CASES])
def test_sharded_oracle_backend_equals_whole_volume(port, oracle_results, index):
  results, stopped = oracle_results
  name, depths, order, pins = CPU_CASES[index]
  for rank in range(WORLD):
    assert (rank, index) in results, f"the ranks stopped before this case: {stopped}"
    assert results[(rank, index)][2] is None, results[(rank, index)][2]
  vol = S.volume(name)
  whole = port.compress(vol, markov_model_order=order, allow_pins=pins)
  if name in S.CRACK_FORMAT:
    import crackle_amd
    assert crackle_amd.header(whole).crack_format == S.CRACK_FORMAT[name], "the volume left the threshold"
  assert results[(0, index)][0] == whole, "merged slab streams differ from the whole-volume stream"
  for rank in range(1, WORLD):
    assert results[(rank, index)][0] is None
  wrong = [rank for rank in range(WORLD) if not results[(rank, index)][1]]
  assert not wrong, f"ranks {wrong} decoded something else than their slabs"


def test_depths_that_do_not_add_up_raise_on_every_rank(oracle_results):
  results, stopped = oracle_results
  for rank in range(WORLD):
    assert (rank, len(CPU_CASES)) in results, f"the ranks stopped before this step: {stopped}"
    assert results[(rank, len(CPU_CASES))][0] == "ValueError: sharded decode: the ranks' depths (3, 3, 3, 2) do not add up to the stream's 10 slices"
