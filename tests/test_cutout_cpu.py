"""Host-side checks of cutout() and CrackleArray (crackle_amd/array.py): the index normalisation
against numpy, its errors, the shortcuts that never reach a device and the array's metadata.  What
needs the decoder (the C entry points' argument errors included: a session needs a device) is in
tests/test_gpu_cutout.py."""
import numpy as np
import pytest

import crackle_amd
from crackle_amd.array import normalize_index
import golden_cases
from util import golden

SHAPE = (7, 5, 3)
VOL = np.arange(7 * 5 * 3).reshape(SHAPE)
SMALL = golden_cases.small_cases()


def _apply(vol, expr):
  """vol[expr] rebuilt from normalize_index alone: the box, then steps and dropped axes."""
  idx = normalize_index(expr, vol.shape)
  for (a, b, step, _), dim in zip(idx, vol.shape):
    assert 0 <= a <= b <= dim and step >= 1
  box = vol[tuple(slice(a, b) for a, b, _, _ in idx)]
  return box[tuple(0 if is_int else slice(None, None, step) for _, _, step, is_int in idx)]


S = np.s_
EXPRESSIONS = [
  S[0], S[6], S[-1], S[-7], S[3, 4, 2], S[-2, -5, -3], S[2, 1], S[4:],
  S[:], S[1:6], S[1:6:2], S[::3], S[::7], S[::100], S[-3:], S[:-2], S[-6:-1:2], S[2:2], S[5:3], S[7:], S[0:0],
  S[1:6, 2:4, 1:3], S[1:6:2, ::2, ::2], S[:, :, 1], S[:, 3], S[2, :, ::2], S[1:4, -1], S[::2, 1:5:3, -1],
  S[...], S[..., 1], S[..., 1, 2], S[1, ...], S[1, ..., 2], S[1:3, ..., ::2], S[..., 2:4, :], S[0, 1, ...], S[..., 0, 1, 2], S[0, 1, 2, ...],
  S[np.int64(3)], S[np.int32(-1), np.uint8(2)], S[np.int64(1):np.int64(5):np.int64(2)],
]


@pytest.mark.parametrize("expr", EXPRESSIONS, ids=[repr(e) for e in EXPRESSIONS])
def test_index_normalisation_against_numpy(expr):
  got, want = _apply(VOL, expr), VOL[expr]
  assert np.shape(got) == np.shape(want) and np.array_equal(got, want)


def test_the_box_is_no_larger_than_the_elements_taken():
  assert normalize_index(S[1:7:4, ::3, 2:2], SHAPE) == [(1, 6, 4, False), (0, 4, 3, False), (2, 2, 1, False)]
  assert normalize_index(S[-1], SHAPE) == [(6, 7, 1, True), (0, 5, 1, False), (0, 3, 1, False)]


@pytest.mark.parametrize("expr,error", [
  (S[8:], ValueError), (S[:8], ValueError), (S[-8:], ValueError), (S[:-8], ValueError), (S[:, :6], ValueError), (S[:, :, 4:], ValueError),
  (S[::-1], ValueError), (S[5:1:-2], ValueError), (S[:, ::-1], ValueError), (S[::0], ValueError),
  (S[..., ...], ValueError), (S[..., 1, ...], ValueError),
  (S[7], IndexError), (S[-8], IndexError), (S[0, 5], IndexError), (S[0, 0, 3], IndexError), (S[0, 0, -4], IndexError),
  (S[0, 0, 0, 0], IndexError), (S[:, :, :, :], IndexError),
  (S[None], TypeError), (S[1.5], TypeError), (S[[1, 2]], TypeError), (S[True], TypeError),
], ids=repr)
def test_index_errors(expr, error):
  with pytest.raises(error):
    normalize_index(expr, SHAPE)


def test_numpy_accepts_what_the_stricter_checks_refuse():
  """The checks taken from the reference are stricter than numpy, which clamps and reverses."""
  assert VOL[8:].shape == (0, 5, 3) and VOL[:100].shape == SHAPE and VOL[::-1].shape == SHAPE


def test_host_shortcuts_need_no_device():
  g = golden()
  ones = crackle_amd.cutout(g["kat_ones_300"], S[10:20, 290:, 1])      # single label
  assert ones.shape == (10, 10) and ones.dtype == np.uint32 and (ones == 1).all()
  assert np.array_equal(crackle_amd.cutout(g["kat_ones_300"], S[::7, 5, ::2]), SMALL["kat_ones_300"][0][::7, 5, ::2])
  assert not crackle_amd.cutout(g["zeros_50"], S[..., 2]).any()
  absent = crackle_amd.cutout(g["kat_4x4"], S[1:3, :, 0], label=3)      # a label the stream does not hold
  assert absent.dtype == bool and absent.shape == (2, 4) and not absent.any()
  empty = crackle_amd.cutout(g["empty_000"], S[:, :, :])      # no voxels
  assert empty.shape == (0, 0, 0) and empty.dtype == np.uint8
  with pytest.raises(IndexError):
    crackle_amd.cutout(g["empty_000"], 0)
  none = crackle_amd.cutout(g["c0_voronoi_u8"], S[5:5, :, 3:9])      # an empty box of a stream that has voxels
  assert none.shape == (0, 64, 6) and none.dtype == np.uint8
  with pytest.raises(ValueError):
    crackle_amd.cutout(g["c0_voronoi_u8"], S[:65])


def test_crackle_array_metadata():
  vol = SMALL["c0_voronoi_u8"][0]
  binary = golden()["c0_voronoi_u8"]
  arr = crackle_amd.CrackleArray(binary)
  assert arr.binary == binary and len(arr) == len(binary)
  assert arr.shape == vol.shape == (64, 64, 16) and arr.ndim == 3
  assert arr.dtype == np.uint8 and arr.size == vol.size and arr.nbytes == vol.nbytes
  assert arr.min() == int(vol.min()) and arr.max() == int(vol.max())
  present = int(vol[3, 4, 5])
  assert present in arr and 300 not in arr and -1 not in arr
  kat = crackle_amd.CrackleArray(golden()["kat_4x4"])
  assert 7 in kat and 0 in kat and 3 not in kat and (kat.min(), kat.max()) == (0, 7)
  assert arr.num_labels() == len(np.unique(vol)) and np.array_equal(arr.labels(), np.unique(vol))
  assert arr.header().sz == 16
  for name in ("__setitem__", "remap", "astype", "refit", "renumber", "save", "each", "cache_meta", "__add__"):
    assert not hasattr(arr, name), name
  ones = crackle_amd.CrackleArray(golden()["kat_ones_300"])
  assert np.array_equal(ones[298:, :2, 0], SMALL["kat_ones_300"][0][298:, :2, 0])      # __getitem__ is cutout
