"""contacts without a GPU: the numpy restatement (tests/contacts_numpy.py) against the reference's own
output, and the range errors that crackle_amd.contacts and fastcrackle.contacts raise before any
device work.

tests/golden/contacts.json was recorded once from the compiled reference by a driver kept outside
the repository that #includes src/operations.hpp and calls
crackle::operations::contacts(buf, n, z_start, z_end, wx, wy, wz) (src/operations.hpp:850-1021) on
every stream of tests/golden/golden.npz and the signed volumes of contacts_numpy.signed_volumes()
(compressed by the reference; their sha256 under "streams"), at every anisotropy of
contacts_numpy.ANISOTROPIES and every range of contacts_numpy.ranges(sz), plus the whole C1 volume at
(1, 1, 1).  Per case: the pair count and the sha256 of the sorted (a u64, b u64, area f32) records
(contacts_numpy.digest); the records themselves for cases with at most 64 pairs; or the error text.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import contacts_numpy as cn
import golden_cases
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
  with open(os.path.join(HERE, "golden", "contacts.json")) as f:
    return json.load(f)


def test_fixture_covers_the_grid():
  want = _fixture()
  cases = cn.inputs()
  assert sorted(golden()) == sorted(golden_cases.small_cases())
  assert set(want["streams"]) == set(cn.signed_volumes()) | {"c1"}
  for name, (lab, _) in cases.items():
    for at in cn.ANISOTROPIES:
      for rt, _, _ in cn.ranges(lab.shape[2]):
        assert cn.case_key(name, at, rt) in want["cases"], (name, at, rt)


def test_signed_streams_are_the_recorded_ones(checker):
  """The signed volumes regenerate to the streams the fixture was recorded from."""
  want = _fixture()["streams"]
  for name, (lab, kw) in cn.signed_volumes().items():
    assert hashlib.sha256(checker.compress(lab, **kw)).hexdigest() == want[name], name


def test_numpy_restatement_matches_the_reference():
  """contacts_numpy on the inputs of every recorded stream equals the reference's output: bit for bit
  at (1,1,1), (4,4,40) and (0.5,2,8), within the reference's own rounding at (1.1,0.7,3.3)."""
  want = _fixture()["cases"]
  for name, (lab, _) in sorted(cn.inputs().items()):
    sz = lab.shape[2]
    for at in cn.ANISOTROPIES:
      for rt, z0, z1 in cn.ranges(sz):
        w = want[cn.case_key(name, at, rt)]
        if "error" in w:
          with pytest.raises(RuntimeError) as e:
            cn.clamp_range(sz, z0, z1)
          assert str(e.value) == w["error"], name
          continue
        zs, ze = cn.clamp_range(sz, z0, z1)
        cn.check_case(w, cn.contacts_numpy(lab, zs, ze), at)


def test_component_image_decides_in_plane_faces():
  """Touching components of one label (a rewritten label table) give (a, a) pairs from in-plane faces
  only; z faces compare labels."""
  comp = np.zeros((4, 2, 2), np.uint32, order="F")
  comp[2:, :, :] = 1
  comp[:, :, 1] = 2
  lab = np.full((4, 2, 2), 5, np.uint32, order="F")
  got = cn.contacts_numpy(lab, 0, -1, components=comp)
  assert got == {(5, 5): [2, 0, 0]}
  lab[:, :, 1] = 7
  got = cn.contacts_numpy(lab, 0, -1, components=comp)
  assert got == {(5, 5): [2, 0, 0], (5, 7): [0, 0, 8]}


def test_signed_keys_are_sign_extended():
  lab = np.array([[[-1], [-2]], [[0], [3]]], dtype=np.int16)
  got = cn.contacts_numpy(np.asfortranarray(lab), 0, -1)
  assert got == {(3, 2**64 - 2): [1, 0, 0], (2**64 - 2, 2**64 - 1): [0, 1, 0]}


def test_range_errors_before_device_work(checker):
  """sz == 0 and z_start >= z_end raise the reference's RuntimeError from the range rule alone."""
  import crackle_amd
  from crackle_amd import fastcrackle, operations
  empty = checker.compress(np.zeros((0, 0, 0), np.uint8, order="F"))
  for call in (lambda: crackle_amd.contacts(empty), lambda: fastcrackle.contacts(empty, 0, -1, 1.0, 1.0, 1.0)):
    with pytest.raises(RuntimeError, match=r"^crackle: Invalid range: 0 - 0$"):
      call()
  b = checker.compress(np.ones((4, 3, 5), np.uint16, order="F"))
  for z0, z1, msg in ((3, 2, "3 - 2"), (2, 2, "2 - 2"), (9, 4, "4 - 4"), (0, 0, "0 - 0")):
    with pytest.raises(RuntimeError, match=f"^crackle: Invalid range: {msg}$"):
      operations._contacts_counts(b, z0, z1)
    with pytest.raises(RuntimeError, match=f"^crackle: Invalid range: {msg}$"):
      fastcrackle.contacts(b, z0, z1, 1.0, 1.0, 1.0)


def test_no_voxels_in_a_slice_returns_empty(checker):
  """sx * sy == 0 with sz > 0: {} without a device, as the reference (src/operations.hpp:899-901)."""
  import crackle_amd
  from crackle_amd import fastcrackle
  b = checker.compress(np.zeros((5, 0, 3), np.uint32, order="F"))
  assert crackle_amd.contacts(b) == {}
  assert fastcrackle.contacts(b, 0, -1, 1.0, 1.0, 1.0) == {}
