"""The encoder's slice limit, checked before any device call (check_dims, crackle_amd/csrc/ckl_encode.hip): slices of
2^30 or more crack vertices, (sx + 1) (sy + 1) >= 2^30, are refused.  Larger slices once encoded into streams the
decoder refused, and one encode of that size faulted on the device."""
import ctypes as C

from crackle_amd import _lib

REFUSED = [(32767, 32767), (32767, 32768), (65536, 16384), (46336, 46339), (46340, 46340), ((1 << 31) - 1, 1)]
ADMITTED = [(32766, 32767), (32767, 32766), (46336, 23000), (1 << 29, 0)]


def test_encoder_refuses_slices_of_2_30_crack_vertices():
  L = _lib.lib()
  h = C.c_void_p()
  for sx, sy in REFUSED:
    assert (sx + 1) * (sy + 1) >= 1 << 30
    assert L.ckl_encoder_create(sx, sy, 1, 1, 0, C.byref(h)) == _lib.CKL_ERR_ARG, (sx, sy)
    assert "2^30" in _lib.last_error() or "too large" in _lib.last_error(), (sx, sy)


def test_encoder_admits_slices_below_2_30_crack_vertices():
  """The admitted side: an encoder is created, or (without a device) the refusal is the missing device's."""
  L = _lib.lib()
  h = C.c_void_p()
  for sx, sy in ADMITTED:
    assert (sx + 1) * (sy + 1) < 1 << 30
    rc = L.ckl_encoder_create(sx, sy, 1, 1, 0, C.byref(h))
    if rc == _lib.CKL_OK:
      L.ckl_encoder_destroy(h)
      h = C.c_void_p()
    else:
      assert rc == _lib.CKL_ERR_NO_DEVICE, (sx, sy, rc, _lib.last_error())
