"""Which exception every consumer of a decoded stream raises for one damaged slice, and that the
integrity check reports that slice and no other.  All of them read a slice's error word through the
decoder's one mapping (ckl_decode.hip: slice_error), whatever stage of the pipeline they stop at.

Streams: the 64 x 64 x 16 golden voronoi volume with flat labels and with pins + markov order 5.
Slice k = 7 is damaged in one of two ways:

  crc      bit 0 of slice k's word in the tail of per-slice crc32c values (the last 4 sz bytes of the
           stream) is flipped: the crack code decodes, its component image no longer matches.
  boc      the first four bytes of slice k's crack code, the byte length of its index of crack start
           points, are overwritten with 0xFFFFFFFF: the index would reach far past the slice's code,
           which the crack parser refuses before it reads a single symbol (ERR_BOC)."""
import numpy as np
import pytest

import crackle_amd
from util import golden

pytestmark = pytest.mark.gpu

K = 7
KINDS = {"crc": "crack code crc mismatch", "boc": "crack code is malformed or corrupted"}
STREAMS = ("c0_voronoi_u8", "c0_voronoi_u8_pins_m5")


def _damaged(name, damage):
  good = golden()[name]
  head = crackle_amd.header(good)
  assert (head.sx, head.sy, head.sz) == (64, 64, 16)
  bad = bytearray(good)
  if damage == "crc":
    bad[len(good) - 4 * head.sz + 4 * K] ^= 1
  else:
    hb = head.header_bytes
    lens = np.frombuffer(good, dtype="<u4", offset=hb, count=head.sz)
    at = hb + head.grid_index_bytes + head.num_label_bytes + head.markov_model_bytes + int(lens[:K].sum())
    assert lens[K] > 4
    bad[at:at + 4] = b"\xff\xff\xff\xff"
  return bytes(bad)


def _raises(damage, call):
  with pytest.raises(RuntimeError) as info:
    call()
  assert type(info.value) is RuntimeError
  msg = str(info.value)
  print(call.__name__ if hasattr(call, "__name__") else call, "->", msg)
  assert msg == f"crackle: {KINDS[damage]} on z={K}", msg


@pytest.fixture(scope="module", params=[(s, d) for s in STREAMS for d in KINDS], ids=lambda p: f"{p[0]}-{p[1]}")
def case(request):
  name, damage = request.param
  return name, damage, _damaged(name, damage)


def test_decompress(case):
  _, damage, bad = case
  _raises(damage, lambda: crackle_amd.decompress(bad))


def test_decompress_of_a_range_without_the_slice(case):
  name, _, bad = case
  whole = crackle_amd.decompress(golden()[name])
  assert np.array_equal(crackle_amd.decompress_range(bad, 0, K), whole[:, :, :K])
  assert np.array_equal(crackle_amd.decompress_range(bad, K + 1, None), whole[:, :, K + 1:])


def test_voxel_counts(case):
  _, damage, bad = case
  _raises(damage, lambda: crackle_amd.voxel_counts(bad))


def test_contacts(case):
  _, damage, bad = case
  _raises(damage, lambda: crackle_amd.contacts(bad))


def test_connected_components(case):
  name, damage, bad = case
  if name != STREAMS[0]:
    return      # the flat stream only
  _raises(damage, lambda: crackle_amd.connected_components(bad))


def test_point_cloud(case):
  _, damage, bad = case
  _raises(damage, lambda: crackle_amd.point_cloud(bad))


def test_voxel_connectivity_graph_4(case):
  """Connectivity 4 stops at the crack planes: the crc of the component image is never looked at."""
  name, damage, bad = case
  if damage == "crc":
    want = crackle_amd.voxel_connectivity_graph(golden()[name], connectivity=4)
    assert np.array_equal(crackle_amd.voxel_connectivity_graph(bad, connectivity=4), want)
  else:
    _raises(damage, lambda: crackle_amd.voxel_connectivity_graph(bad, connectivity=4))


def test_voxel_connectivity_graph_6(case):
  _, damage, bad = case
  _raises(damage, lambda: crackle_amd.voxel_connectivity_graph(bad, connectivity=6))


def test_integrity_check_flags_the_slice_and_raises_nothing(case):
  _, _, bad = case
  report = crackle_amd.check(bad)
  assert report == {"header": True, "crack_index": True, "labels": True, "z": [K]}, report
  assert not crackle_amd.ok(bad)
