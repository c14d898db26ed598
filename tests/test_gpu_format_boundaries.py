"""GPU tests at the edges of the format's field widths and markov orders, against the checker (the compiled reference
where it was built).  Every case first parses the stream the checker writes and asserts the widths it is meant to
reach (the pin section's combined byte: count, depth and component-id widths; the flat section's key width; the
per-slice component-count width), so a case that stops reaching its edge fails instead of covering nothing.  Then:
the encoder's bytes are the checker's, and the decoder gets the input back on the strip path and the general run
pipeline, as label images and over a z-window.

Pin count fields of 4 bytes are reached by two labels of 65 536 pins each (1024 x 1024 x 2).  Pin depths of 4 bytes
would need more than 65 536 slices and are not covered.  Component ids of 1 byte cannot meet depths of 2 bytes (257
slices hold at least 257 components), so the split threshold (index + depth width) / id width takes the values 1, 2
and 5 here (3 in the golden fixtures), never 6.

Orders 9 - 13 run k_crack_match with the model in global memory (the LDS holds models of order <= 8); the encoder's
histogram at order 13 has 4^13 rows (1 GiB of counters)."""
import numpy as np
import pytest

import crackle_amd
from crackle_amd import synth

pytestmark = pytest.mark.gpu

FLAT, PINS = 0, 2


def _bw(x):
  return 1 if x <= 0xFF else 2 if x <= 0xFFFF else 4 if x <= 0xFFFFFFFF else 8


def layout(binary):
  """The label section's widths, and for pin sections every label's record: {label: (pins [(index, depth)], n_ids)}."""
  h = crackle_amd.header(binary)
  sec = binary[h.header_bytes + h.grid_index_bytes:][:h.num_label_bytes]
  sw, sxy = h.stored_data_width, h.sx * h.sy
  out = dict(fmt=h.label_format, comp=_bw(sxy))
  if h.label_format == FLAT:
    nu = int.from_bytes(sec[0:8], "little")
    p = 8 + sw * nu
    out.update(key=_bw(nu), unique=nu, most_components=max(int.from_bytes(sec[p + out["comp"] * z:p + out["comp"] * (z + 1)], "little") for z in range(h.sz)))
    return out
  n = int.from_bytes(sec[sw:sw + 8], "little")
  out["bgcolor"] = int.from_bytes(sec[0:sw], "little")
  labels = [int.from_bytes(sec[sw + 8 + sw * i:sw + 8 + sw * (i + 1)], "little") for i in range(n)]
  p = sw + 8 + sw * n
  out["most_components"] = max(int.from_bytes(sec[p + out["comp"] * z:p + out["comp"] * (z + 1)], "little") for z in range(h.sz))
  p += out["comp"] * h.sz
  c = sec[p]
  p += 1
  npw, dw, ccw = 1 << (c & 3), 1 << ((c >> 2) & 3), 1 << ((c >> 4) & 3)
  iw = _bw((h.sx * h.sy * h.sz) & 0xFFFFFFFF)
  out.update(npins=npw, depth=dw, cc=ccw, index=iw, threshold=(iw + dw) // ccw)
  recs = {}
  for lab in labels:
    k = int.from_bytes(sec[p:p + npw], "little")
    p += npw
    idx = [int.from_bytes(sec[p + iw * j:p + iw * (j + 1)], "little") for j in range(k)]
    p += iw * k
    depths = [int.from_bytes(sec[p + dw * j:p + dw * (j + 1)], "little") for j in range(k)]
    p += dw * k
    m = int.from_bytes(sec[p:p + npw], "little")
    p += npw + ccw * m
    recs[lab] = (list(zip(np.cumsum(idx).tolist(), depths)), m)
  out["records"] = recs
  out["records_end"] = p == len(sec)
  return out


def _columns(sx, sy, sz, div, per_row):
  x, y, _ = np.meshgrid(np.arange(sx), np.arange(sy), np.arange(sz), indexing="ij")
  return np.asfortranarray((x // div[0] + per_row * (y // div[1]) + 1).astype(np.uint16))


def depth2():
  return _columns(8, 8, 257, (2, 2), 4)


def depth1_control():
  return np.asfortranarray(depth2()[:, :, :256])


def depth_300_changed():
  a = _columns(8, 8, 300, (2, 2), 4)
  a[3, 3, 150] = 99
  return a


def depth2_ids():
  a = _columns(8, 8, 257, (4, 2), 2)
  a[0, 0, 0] = 99
  a[7, 7, 256] = 98
  a[3, 5, 128] = 98
  return a


def threshold5():
  x, y, _ = np.meshgrid(np.arange(128), np.arange(128), np.arange(8), indexing="ij")
  a = np.asfortranarray((x // 32 + 4 * (y // 32) + 1).astype(np.uint8))
  a[0:2, 0:2, 1:4] = 50
  a[40:42, 40:42, 1:8] = 50
  a[100, 3, 5] = 60
  return a


def npins2():
  a = np.zeros((128, 128, 4), np.uint16, order="F")
  a[::4, ::4, :] = 1
  a[2::4, 2::4, :] = 2
  return a


def npins4():
  a = np.zeros((1024, 1024, 2), np.uint8, order="F")
  a[::8, ::2, :] = 1
  a[4::8, 1::2, :] = 2
  return a


def cc4():
  a = np.zeros((600, 600, 2), np.uint8, order="F")
  a[::2, ::2, 0] = 1
  a[:, :, 1] = 2
  return a


def count_overflow():
  a = np.zeros((128, 128, 4), np.uint8, order="F")
  a[::9, ::9, 0:2] = 1
  a[4::9, 4::9, 0:2] = 2
  return a


def count_overflow_voronoi():
  return synth.as_numpy_f(synth.voronoi_labels((1024, 248, 4), np.uint8, seed=11, cell=(4, 4, 2)))


def unique(sx, sy):
  """sx * sy labels, one component each, in both of two equal slices."""
  s = np.arange(sx * sy, dtype=np.uint32).reshape((sx, sy, 1), order="F")
  return np.asfortranarray(np.concatenate([s, s], axis=2))


def voronoi(sx, sy):
  return synth.as_numpy_f(synth.voronoi_labels((sx, sy, 3), np.uint16, seed=5, cell=(16, 16, 2)))


# name, volume, allow_pins, expected widths, z-window
CASES = [
  ("pin_depth_w2", depth2, True, dict(fmt=PINS, npins=1, depth=2, cc=2, index=2, threshold=2), (100, 200)),
  ("pin_depth_w1_256", depth1_control, True, dict(fmt=PINS, npins=1, depth=1, cc=2, index=2, threshold=1), (100, 200)),
  ("pin_depth_300_flat", depth_300_changed, True, dict(fmt=FLAT, key=1, comp=1), (100, 200)),
  ("pin_depth_w2_ids", depth2_ids, True, dict(fmt=PINS, npins=1, depth=2, cc=2, index=2, threshold=2), (100, 200)),
  ("pin_threshold5", threshold5, True, dict(fmt=PINS, npins=1, depth=1, cc=1, index=4, threshold=5), (2, 6)),
  ("pin_count_w2", npins2, True, dict(fmt=PINS, npins=2, depth=1, cc=2, index=4, threshold=2), (1, 3)),
  ("pin_count_w4", npins4, True, dict(fmt=PINS, npins=4, depth=1, cc=4, index=4, threshold=1, comp=4), (1, 2)),
  ("pin_cc_w4", cc4, True, dict(fmt=PINS, npins=1, depth=1, cc=4, index=4, threshold=1, comp=4), (1, 2)),
  ("pin_count_overflow", count_overflow, True, dict(fmt=PINS, npins=2, depth=1, cc=2, index=4, threshold=2), (1, 3)),
  ("pin_count_overflow_voronoi", count_overflow_voronoi, True, dict(fmt=PINS, npins=2, depth=1, cc=2, index=4, threshold=2, comp=4), (1, 3)),
  ("flat_key_w2_65535", lambda: unique(255, 257), False, dict(fmt=FLAT, key=2, comp=2, unique=65535), (1, 2)),
  ("flat_key_w4_65536", lambda: unique(256, 256), False, dict(fmt=FLAT, key=4, comp=4, unique=65536), (1, 2)),
  ("flat_key_w4_65792", lambda: unique(257, 256), False, dict(fmt=FLAT, key=4, comp=4, unique=65792), (1, 2)),
  ("comp_w2_65535", lambda: voronoi(255, 257), False, dict(fmt=FLAT, comp=2), (1, 2)),
  ("comp_w4_65536", lambda: voronoi(256, 256), False, dict(fmt=FLAT, comp=4), (1, 2)),
]
OVERFLOW = ("pin_count_overflow", "pin_count_overflow_voronoi")


def _label_choices(arr, lay):
  """Labels for decompress(label=): the background colour of a pin section, the label of its deepest pin and a label
  with ids only; for flat sections the first, middle and last unique label."""
  if lay["fmt"] == FLAT:
    u = np.unique(arr)
    return [int(u[0]), int(u[len(u) // 2]), int(u[-1])]
  recs = lay["records"]
  deep = max((lab for lab in recs if recs[lab][0]), key=lambda lab: max(d for _, d in recs[lab][0]), default=None)
  ids_only = [lab for lab in recs if not recs[lab][0] and recs[lab][1]]
  return [lay["bgcolor"]] + ([deep] if deep is not None else []) + ids_only[:1]


@pytest.mark.parametrize("name,make,pins,want,window", CASES, ids=[c[0] for c in CASES])
def test_format_boundary(name, make, pins, want, window, checker, monkeypatch):
  arr = make()
  ref_bytes = checker.compress(arr, allow_pins=pins)
  if name in OVERFLOW:
    # the reference's one-byte counts overflow (its records run past the section); the encoder here widens them
    lay = layout(ref_bytes)
    assert lay["fmt"] == PINS and lay["npins"] == 1 and not lay["records_end"]
    binary = crackle_amd.compress(arr, allow_pins=pins)
    assert binary != ref_bytes
    assert np.array_equal(checker.decompress(binary).reshape(arr.shape, order="F"), arr)
  else:
    binary = ref_bytes
    assert crackle_amd.compress(arr, allow_pins=pins) == binary, name
  lay = layout(binary)
  assert {k: lay.get(k) for k in want} == want, name
  if lay["fmt"] == PINS:
    assert lay["records_end"]
  if name.startswith("pin_depth_w2"):
    assert max(d for pins_, _ in lay["records"].values() for _, d in pins_) == 256
  if name == "pin_depth_w2_ids":
    assert any(not p and m for p, m in lay["records"].values()), "no label with ids only"
  if name in ("pin_threshold5", "pin_cc_w4"):
    assert any(m for _, m in lay["records"].values()), "no single-component ids"
  if name in ("flat_key_w4_65536", "flat_key_w4_65792", "pin_count_w4", "pin_cc_w4"):
    assert lay["most_components"] >= 65536, "no slice of 65 536 components"

  z0, z1 = window
  for general in (False, True):
    if general:
      monkeypatch.setenv("CKL_DECODE_GENERAL", "1")
    else:
      monkeypatch.delenv("CKL_DECODE_GENERAL", raising=False)
    path = "general" if general else "strip"
    assert np.array_equal(crackle_amd.decompress(binary), arr), (name, path)
    for lab in _label_choices(arr, lay):
      assert np.array_equal(crackle_amd.decompress(binary, label=lab), arr == lab), (name, path, lab)
    assert np.array_equal(crackle_amd.decompress_range(binary, z0, z1), arr[:, :, z0:z1]), (name, path, window)
  monkeypatch.delenv("CKL_DECODE_GENERAL", raising=False)


def test_pin_window_inside_a_deep_pin():
  """z in [100, 200) of 257-deep pins: every decoded slice lies strictly inside each pin's run."""
  arr = depth2()
  binary = crackle_amd.compress(arr, allow_pins=True)
  lay = layout(binary)
  sxy = arr.shape[0] * arr.shape[1]
  assert all(i // sxy == 0 and d == 256 for p, _ in lay["records"].values() for i, d in p)
  for z0, z1 in ((100, 200), (1, 256), (255, 257), (0, 1)):
    assert np.array_equal(crackle_amd.decompress_range(binary, z0, z1), arr[:, :, z0:z1]), (z0, z1)
    lab = int(arr[5, 5, 0])
    assert np.array_equal(crackle_amd.decompress_range(binary, z0, z1, label=lab), arr[:, :, z0:z1] == lab), (z0, z1)


def _markov_volume():
  return synth.as_numpy_f(synth.voronoi_labels((48, 40, 4), np.uint32, seed=3, cell=(16, 16, 4)))


@pytest.mark.parametrize("order", range(8, 14))
def test_markov_order(order, checker, monkeypatch):
  """Orders 8 - 13: the encoder's bytes are the checker's; the decoder reads them with the model in global memory,
  with the parallel and the serial markov decode, on the strip path and the general run pipeline."""
  arr = _markov_volume()
  want = checker.compress(arr, markov_model_order=order)
  assert crackle_amd.header(want).markov_model_order == order
  assert crackle_amd.compress(arr, markov_model_order=order) == want
  for env in (None, "CKL_MARKOV_SERIAL", "CKL_DECODE_GENERAL"):
    monkeypatch.delenv("CKL_MARKOV_SERIAL", raising=False)
    monkeypatch.delenv("CKL_DECODE_GENERAL", raising=False)
    if env:
      monkeypatch.setenv(env, "1")
    assert np.array_equal(crackle_amd.decompress(want), arr), (order, env)
    assert np.array_equal(crackle_amd.decompress_range(want, 1, 3), arr[:, :, 1:3]), (order, env)


def test_markov_reencode_to_13_and_back(checker):
  arr = _markov_volume()
  b0 = checker.compress(arr)
  b13 = crackle_amd.reencode(b0, 13)
  assert b13 == checker.compress(arr, markov_model_order=13)
  assert crackle_amd.reencode(b13, 0) == b0
  assert crackle_amd.reencode(b13, 9) == checker.compress(arr, markov_model_order=9)
  assert np.array_equal(crackle_amd.decompress(b13), arr)
