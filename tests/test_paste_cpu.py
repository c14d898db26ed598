"""Host-side checks of paste() and CrackleArray.paste (crackle_amd/array.py) and of ckl_paste's declaration: the
surface, the empty box, the errors that never reach a device, and the precondition of every byte claim that
tests/test_gpu_paste.py makes (tests/paste_volumes.py).  What needs the kernels is in tests/test_gpu_paste.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crackle_amd
import paste_volumes as pv
from crackle_amd import _lib
from recompress_volumes import as_signed
from util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = np.s_


def test_surface():
  assert hasattr(crackle_amd, "paste") and "paste" in crackle_amd.__all__
  assert hasattr(crackle_amd.CrackleArray, "paste")
  assert not hasattr(crackle_amd.CrackleArray, "__setitem__")      # tests/test_cutout_cpu.py pins it: paste returns a new array


def test_ckl_paste_is_declared_and_exported():
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  assert re.search(r"\bint\s+ckl_paste\s*\(", text)
  assert "ckl_paste" in _lib.EXPORTS and hasattr(_lib.lib(), "ckl_paste")
  assert len(_lib.EXPORTS["ckl_paste"][1]) == 15
  assert _lib.lib().ckl_abi_version() == 1      # an entry was added, none changed


def test_an_empty_box_returns_the_stream():
  g = golden()
  for name in ("c0_voronoi_u8", "c0_voronoi_u8_pins_m5", "kat_ones_300"):
    b = g[name]
    for expr in (S[5:5], S[:, 3:3, 1:2], S[..., 2:2], S[4:2]):
      assert crackle_amd.paste(b, expr, 1) == b, (name, expr)
    assert crackle_amd.paste(b, S[2:2, :4, :1], np.zeros((0, 4, 1), np.uint8)) == b
    arr = crackle_amd.CrackleArray(b).paste(S[5:5], 1)
    assert isinstance(arr, crackle_amd.CrackleArray) and arr.binary == b
  # the C entry point: a copy of the stream, no device
  b = g["c0_voronoi_u8"]
  out, n = C.c_void_p(), C.c_uint64()
  rc = _lib.lib().ckl_paste(b, len(b), None, _lib.MEM_HOST, 0, 1, 3, 3, 0, 64, 0, 16, 0, C.byref(out), C.byref(n))
  assert rc == _lib.CKL_OK, _lib.last_error()
  assert C.string_at(out.value, n.value) == b
  _lib.lib().ckl_free(out)
  # the stream without voxels: every box is empty
  assert crackle_amd.paste(g["empty_000"], S[:, :, :], 1) == g["empty_000"]


INDEX_ERRORS = [S[:65], S[-65:], S[::-1], S[::0], S[..., ...], S[64], S[0, 0, 16], S[0, 0, 0, 0], S[None], S[1.5], S[[1, 2]], S[True]]


@pytest.mark.parametrize("expr", INDEX_ERRORS, ids=repr)
def test_index_errors_are_cutouts(expr):
  b = golden()["c0_voronoi_u8"]
  with pytest.raises(Exception) as want:
    crackle_amd.cutout(b, expr)
  with pytest.raises(type(want.value)) as got:
    crackle_amd.paste(b, expr, 1)
  assert type(got.value) is type(want.value) and str(got.value) == str(want.value)


def test_data_errors_reach_no_device():
  b = golden()["c0_voronoi_u8"]      # 64 x 64 x 16, uint8
  for expr, shape in ((S[1:5, 2:4, 3:9], (3, 2, 6)), (S[1:5, 2, 3:9], (4, 2, 6)), (S[::2, :, 0], (31, 64)), (S[5], (16, 64)), (S[..., 1:3], (3,))):
    with pytest.raises(ValueError):
      crackle_amd.paste(b, expr, np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):      # as numpy's own assignment
      np.zeros((64, 64, 16), np.uint8)[expr] = np.zeros(shape, np.uint8)
  with pytest.raises(ValueError):      # numpy's rule, also for a box without voxels
    crackle_amd.paste(b, S[5:5], np.zeros((3,), np.uint8))
  for value in (256, -1, 1 << 40):
    with pytest.raises(OverflowError):
      crackle_amd.paste(b, S[1:5, 2:4, 3:9], value)
  with pytest.raises(OverflowError):
    crackle_amd.paste(golden()["kat_ones_300"], S[0, 0, 0], 1 << 32)
  with pytest.raises(OverflowError):
    crackle_amd.CrackleArray(b).paste(S[...], np.int64(300))


def test_signed_streams_are_refused_as_compress_refuses_them():
  b = as_signed(golden()["c0_voronoi_u8"])
  assert crackle_amd.header(b).signed
  with pytest.raises(TypeError) as info:
    crackle_amd.paste(b, S[1:5, 2:4, 3:9], 1)
  with pytest.raises(TypeError) as want:
    crackle_amd.compress(np.zeros((2, 2, 2), np.int8))
  assert str(info.value) == str(want.value)
  with pytest.raises(TypeError):
    crackle_amd.CrackleArray(b).paste(S[5:5], 1)      # (before the empty box is answered)
  out, n = C.c_void_p(), C.c_uint64()
  rc = _lib.lib().ckl_paste(b, len(b), None, _lib.MEM_HOST, 0, 1, 1, 5, 2, 4, 3, 9, 0, C.byref(out), C.byref(n))
  assert rc == _lib.CKL_ERR_ARG and "Signed" in _lib.last_error()


def test_c_entry_argument_errors_need_no_device():
  b = golden()["c0_voronoi_u8"]
  L = _lib.lib()
  out, n = C.c_void_p(), C.c_uint64()

  def call(box, has_box, value, x0, x1, y0, y1, z0, z1, mem=_lib.MEM_HOST):
    return L.ckl_paste(b, len(b), box, mem, has_box, value, x0, x1, y0, y1, z0, z1, 0, C.byref(out), C.byref(n))

  for bounds, axis in (((0, 65, 0, 4, 0, 1), "x range"), ((5, 4, 0, 4, 0, 1), "x range"), ((-1, 4, 0, 4, 0, 1), "x range"),
                       ((0, 4, 3, 65, 0, 1), "y range"), ((0, 4, 0, 4, 5, 17), "z range"), ((0, 4, 0, 4, 3, 2), "z range")):
    assert call(None, 0, 1, *bounds) == _lib.CKL_ERR_ARG, bounds
    assert "paste" in _lib.last_error() and axis in _lib.last_error(), (bounds, _lib.last_error())
  assert call(None, 0, 256, 0, 4, 0, 4, 0, 1) == _lib.CKL_ERR_ARG and "does not fit" in _lib.last_error()
  assert call(None, 1, 0, 0, 4, 0, 4, 0, 1) == _lib.CKL_ERR_ARG      # has_box without a box
  assert call(None, 0, 1, 0, 4, 0, 4, 0, 1, mem=7) == _lib.CKL_ERR_ARG
  assert L.ckl_paste(b[:10], 10, None, 0, 0, 1, 0, 4, 0, 4, 0, 1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_FORMAT


def test_the_geometries_cover_both_paints_of_a_slab_decoded_x_fastest():
  """ckl_paste decodes its slab x fastest whatever the stream's order (RunRequest::x_fastest).  On the general
  pipeline that is k_paint_runs<OUT, true> for a width that is a multiple of 4 and k_paint_runs<OUT, false> in mode 1
  otherwise; a C-order stream reaches either only through the flag, so the geometries hold one of each, and every
  geometry has a splice case."""
  assert len(pv.GEOMETRIES) == len(pv.GEOMETRY_IDS) == len(set(pv.GEOMETRY_IDS)) == 5
  for (shape, dtype, order), name in zip(pv.GEOMETRIES, pv.GEOMETRY_IDS):
    assert name == "%dx%dx%d-u%d-%s" % (*shape, 8 * np.dtype(dtype).itemsize, order)
    vol = pv.volume(shape, dtype, order)
    assert vol.shape == shape and vol.dtype == dtype and vol.flags.f_contiguous == (order == "F") and not vol.flags.writeable
  c_order = [shape[0] % 4 for shape, _, order in pv.GEOMETRIES if order == "C"]
  assert 0 in c_order and any(c_order), c_order
  assert pv.GEOMETRIES[4] == ((90, 61, 5), np.uint32, "C")
  assert {id(case.geometry) for case in pv.SPLICES} == {id(g) for g in pv.GEOMETRIES}


@pytest.mark.parametrize("case", pv.SPLICES, ids=repr)
def test_splice_cases_keep_the_crack_format(case, checker):
  """The precondition of `paste(compress(V), idx, data) == compress(V')` in tests/test_gpu_paste.py: the checker gives
  both volumes the same crack format (so the stack of V's untouched slices and the edited slab under V's format is the
  stream of V'), the z-range is not the whole depth, and the edit changes the volume."""
  vol, new = case.volume(), case.edited()
  assert new.flags.f_contiguous == vol.flags.f_contiguous and not np.array_equal(new, vol)
  before, after = crackle_amd.header(checker.compress(vol)), crackle_amd.header(checker.compress(new))
  assert before.crack_format == after.crack_format
  assert before.crack_format == (crackle_amd.CrackFormat.PERMISSIBLE if pv.permissible(vol) else crackle_amd.CrackFormat.IMPERMISSIBLE)
  assert before.label_format == crackle_amd.LabelFormat.FLAT and before.format_version == 1
  assert bool(before.fortran_order) == bool(vol.flags.f_contiguous) == bool(after.fortran_order)
  z0, z1, _, _ = crackle_amd.array.normalize_index(case.idx, vol.shape)[2]
  assert (z0, z1) != (0, vol.shape[2])


def test_the_noise_slab_alone_would_flip_the_format(checker):
  """tests/test_gpu_paste.py pastes this slab to see the input's crack format imposed on it."""
  vol, idx, data = pv.smooth_and_noise()
  new = pv.edited(vol, idx, data)
  fmt = lambda arr: crackle_amd.header(checker.compress(arr)).crack_format
  assert fmt(vol) == fmt(new) == crackle_amd.CrackFormat.IMPERMISSIBLE
  assert fmt(np.asfortranarray(new[idx])) == crackle_amd.CrackFormat.PERMISSIBLE
