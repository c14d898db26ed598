"""crackle_amd.remap / mask / mask_except: host-only rewrites of header and label section (crackle_amd/operations.py).
Checked on the port's decoder: decompress(out) is numpy's mapping of decompress(in), and the bytes are a canonical
FLAT stream (ascending unique list without duplicates, keys at the width of the new count, is_sorted set, label crc
right, everything outside header and label section the input's)."""
import os

import numpy as np
import pytest

import crackle_amd
from crackle_amd import _lib
import label_table_volumes as ltv
import recompress_volumes as rv

HERE = os.path.dirname(os.path.abspath(__file__))


def _decode(port, b):
  head = crackle_amd.header(b)
  return port.decompress(b).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")


def _layout(b):
  head = crackle_amd.header(b)
  off = head.header_bytes + head.grid_index_bytes
  sec = b[off:off + head.num_label_bytes]
  return head, b[head.header_bytes:off], sec, b[off + head.num_label_bytes:]


def _check_canonical(out, src):
  head, zindex, sec, rest = _layout(out)
  h0, zindex0, _, rest0 = _layout(src)
  assert head.label_format == 0 and head.is_sorted and head.format_version == 1
  u = crackle_amd.labels(out)
  assert np.all(np.diff(u.astype(np.uint64).astype(object)) > 0), "ascending, no duplicates"
  claims = ltv.read_claims(out)      # also asserts the section's length from U, the widths and N
  assert claims["U"] == len(u) and claims["key_width"] == ltv.byte_width(len(u))
  assert head.stored_data_width == ltv.byte_width(int(u.max()))
  assert head.data_width == max(h0.data_width, ltv.byte_width(int(u.max())))
  assert (head.sx, head.sy, head.sz, head.crack_format, head.markov_model_order, head.fortran_order) == \
         (h0.sx, h0.sy, h0.sz, h0.crack_format, h0.markov_model_order, h0.fortran_order)
  # z-index, markov model, crack codes and slice crcs are the input's bytes; the label crc is the section's
  crcs = 4 * (head.sz + 1)
  assert zindex == zindex0
  assert rest[:-crcs] == rest0[:-crcs] and rest[-crcs + 4:] == rest0[-crcs + 4:]
  assert int.from_bytes(rest[-crcs:-crcs + 4], "little") == _lib.lib().ckl_crc32c(sec, len(sec)) == crackle_amd.labels_crc(out)
  # components per slice copied
  cw = ltv.byte_width(head.sx * head.sy)
  o, o0 = 8 + len(u) * head.stored_data_width, 8 + ltv.read_claims(src)["U"] * h0.stored_data_width
  assert sec[o:o + head.sz * cw] == _layout(src)[2][o0:o0 + head.sz * cw]


def _apply(arr, mapping):
  out = arr.astype(np.uint64)
  res = out.copy()
  for k, v in mapping.items():
    res[out == k] = v
  return res


@pytest.fixture(scope="module")
def voronoi(port):
  lab = rv.VORONOI.volume()
  return lab, port.compress(lab, markov_model_order=2)


def test_remap_decodes_to_the_mapped_volume(voronoi, port):
  lab, b = voronoi
  mapping = {int(v): (int(v) * 7 + 3) % 251 for v in np.unique(lab)}
  out = crackle_amd.remap(b, mapping)
  assert np.array_equal(_decode(port, out), _apply(lab, mapping))
  _check_canonical(out, b)
  assert crackle_amd.header(out).data_width == 1
  # keys the stream does not hold are ignored; parallel is accepted
  extra = dict(mapping)
  extra.update({k: 5 for k in (100000, 254) if k not in mapping})
  assert len(extra) > len(mapping) and crackle_amd.remap(b, extra, parallel=4) == out


def test_two_labels_merged_give_a_shorter_list(voronoi, port):
  lab, b = voronoi
  a, c = (int(v) for v in np.unique(lab)[:2])
  out = crackle_amd.remap(b, {a: c}, preserve_missing_labels=True)
  assert crackle_amd.num_labels(out) == crackle_amd.num_labels(b) - 1
  assert not crackle_amd.contains(out, a) and crackle_amd.contains(out, c)
  assert np.array_equal(_decode(port, out), _apply(lab, {a: c}))
  _check_canonical(out, b)
  # the merged stream's floordiv twin: remap canonicalises where the in-place rewrite leaves duplicates
  m = rv.floordiv_mapping(lab, 2)
  assert np.array_equal(_decode(port, crackle_amd.remap(b, m)), lab // 2)
  assert len(crackle_amd.labels(crackle_amd.remap(b, m))) == len(np.unique(lab // 2))


def test_key_width_follows_the_unique_count(port):
  lab256 = ltv.components_volume((64, 8, 1), 300, ltv.by_appearance(ltv.ascending(256, 1000, 3)), np.uint16)
  b = port.compress(lab256)
  assert ltv.read_claims(b)["key_width"] == 2
  vals = [int(v) for v in np.unique(lab256)]
  out = crackle_amd.remap(b, {vals[0]: vals[1]}, preserve_missing_labels=True)      # 256 -> 255 labels
  assert ltv.read_claims(out)["U"] == 255 and ltv.read_claims(out)["key_width"] == 1
  assert np.array_equal(_decode(port, out), _apply(lab256, {vals[0]: vals[1]}))
  _check_canonical(out, b)
  lab255 = ltv.components_volume((64, 8, 1), 300, ltv.by_appearance(ltv.ascending(255, 1000, 3)), np.uint16)
  b = port.compress(lab255)
  assert ltv.read_claims(b)["key_width"] == 1
  # the other side of the threshold: 257 -> 256 labels keeps two-byte keys, and a 255-label stream keeps one-byte keys
  lab257 = ltv.components_volume((64, 8, 1), 300, ltv.by_appearance(ltv.ascending(257, 1000, 3)), np.uint16)
  b = port.compress(lab257)
  vals = [int(v) for v in np.unique(lab257)]
  out = crackle_amd.remap(b, {vals[0]: vals[1]}, preserve_missing_labels=True)
  assert ltv.read_claims(out)["U"] == 256 and ltv.read_claims(out)["key_width"] == 2
  assert np.array_equal(_decode(port, out), _apply(lab257, {vals[0]: vals[1]}))
  # a remap never splits a label, so the count only grows against a list with duplicates (the in-place floordiv
  # rewrite): 512 entries of 256 values come out as 256 labels with two-byte keys, one merge more as 255 with one byte
  lab = ltv.components_volume((64, 16, 1), 600, ltv.by_appearance(ltv.ascending(512, 0, 1)), np.uint16)
  halves = rv.floordiv_stream(port.compress(lab), 2)
  assert ltv.read_claims(halves)["U"] == 512 and len(np.unique(crackle_amd.labels(halves))) == 256
  one_less = crackle_amd.remap(halves, {0: 1}, preserve_missing_labels=True)
  assert ltv.read_claims(one_less)["U"] == 255 and ltv.read_claims(one_less)["key_width"] == 1
  again = crackle_amd.remap(halves, {}, preserve_missing_labels=True)
  assert ltv.read_claims(again)["U"] == 256 and ltv.read_claims(again)["key_width"] == 2
  assert np.array_equal(_decode(port, again), lab // 2)
  assert np.array_equal(_decode(port, one_less), _apply(lab // 2, {0: 1}))


def test_a_wider_value_grows_the_data_width(voronoi, port):
  lab, b = voronoi
  v = int(np.unique(lab)[3])
  out = crackle_amd.remap(b, {v: 300}, preserve_missing_labels=True)
  head = crackle_amd.header(out)
  assert head.data_width == 2 and head.stored_data_width == 2
  got = _decode(port, out)
  assert got.dtype == np.uint16 and np.array_equal(got, _apply(lab, {v: 300}))
  _check_canonical(out, b)
  # never shrinks: a uint16 stream whose labels all fit a byte keeps its data width
  wide = port.compress(lab.astype(np.uint16))
  small = crackle_amd.remap(wide, {int(k): int(k) // 2 for k in np.unique(lab)})
  assert crackle_amd.header(small).data_width == 2 and crackle_amd.header(small).stored_data_width == 1
  big = crackle_amd.remap(b, {v: (1 << 64) - 1}, preserve_missing_labels=True)
  assert crackle_amd.header(big).data_width == 8 and int(_decode(port, big).max()) == (1 << 64) - 1


def test_missing_labels(voronoi):
  lab, b = voronoi
  labels = [int(v) for v in np.unique(lab)]
  with pytest.raises(KeyError) as err:
    crackle_amd.remap(b, {v: 1 for v in labels[1:]})
  assert err.value.args[0] == labels[0]
  with pytest.raises(KeyError):
    crackle_amd.remap(b, {})
  assert crackle_amd.remap(b, {}, preserve_missing_labels=True) == crackle_amd.remap(b, {v: v for v in labels})
  for bad in (-1, 1 << 64):
    with pytest.raises(ValueError):
      crackle_amd.remap(b, {labels[0]: bad}, preserve_missing_labels=True)


def test_mask_and_mask_except(voronoi, port):
  lab, b = voronoi
  labels = [int(v) for v in np.unique(lab)]
  gone = labels[::3]
  out = crackle_amd.mask(b, gone)
  assert np.array_equal(_decode(port, out), _apply(lab, {v: 0 for v in gone}))
  assert out == crackle_amd.remap(b, {v: 0 for v in gone}, preserve_missing_labels=True)
  _check_canonical(out, b)
  assert np.array_equal(_decode(port, crackle_amd.mask(b, gone, value=77)), _apply(lab, {v: 77 for v in gone}))
  keep = labels[:5] + [100000]      # an absent label among those to keep
  out = crackle_amd.mask_except(b, keep)
  assert np.array_equal(_decode(port, out), _apply(lab, {v: 0 for v in labels[5:]}))
  assert sorted(int(v) for v in crackle_amd.labels(out)) == sorted(set(labels[:5]) | {0})
  _check_canonical(out, b)
  everything = crackle_amd.mask_except(b, [], value=9)
  assert crackle_amd.num_labels(everything) == 1 and int(_decode(port, everything).min()) == 9


def test_c_order_and_uint64(port):
  lab = np.ascontiguousarray(rv.voronoi((40, 36, 5), np.uint64, 3, cell=(8, 8, 2), offset=1 << 40))
  assert not lab.flags.f_contiguous
  b = port.compress(lab)
  assert not crackle_amd.header(b).fortran_order
  m = {int(v): int(v) >> 3 for v in np.unique(lab)}
  out = crackle_amd.remap(b, m)
  assert np.array_equal(_decode(port, out), lab >> np.uint64(3))
  _check_canonical(out, b)


def test_refusals(voronoi, port):
  lab, b = voronoi
  pins = port.compress(lab, allow_pins=True)
  assert crackle_amd.header(pins).label_format == 2
  for f in (lambda s: crackle_amd.remap(s, {1: 2}, preserve_missing_labels=True), lambda s: crackle_amd.mask(s, [1]), lambda s: crackle_amd.mask_except(s, [1])):
    with pytest.raises(ValueError, match=r"recompress\(\)"):
      f(pins)
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    v0 = z[[k for k in z.files if "." not in k][0]].tobytes()
  assert crackle_amd.header(v0).format_version == 0
  with pytest.raises(ValueError, match="version 0"):
    crackle_amd.remap(v0, {}, preserve_missing_labels=True)
  signed = rv.as_signed(b)
  assert crackle_amd.header(signed).signed
  for f in (lambda: crackle_amd.remap(signed, {}, preserve_missing_labels=True), lambda: crackle_amd.mask(signed, [1]),
            lambda: crackle_amd.mask_except(signed, [1]), lambda: crackle_amd.recompress(signed)):
    with pytest.raises(TypeError, match="Signed integer data types are not currently supported."):
      f()
  with pytest.raises(ValueError, match="allow_pins"):
    crackle_amd.recompress(b, allow_pins=True)


def test_empty_stream(port):
  b = port.compress(np.zeros((5, 0, 3), dtype=np.uint8, order="F"))
  assert crackle_amd.remap(b, {1: 2}) == b and crackle_amd.mask(b, [1]) == b and crackle_amd.mask_except(b, [1]) == b


def test_recompress_answers_without_a_device_where_it_can(voronoi, port):
  """Streams without voxels are their header, as compress gives it; signed streams are refused at the C boundary too."""
  import ctypes as C
  for shape in ((0, 0, 0), (5, 0, 3)):
    arr = np.zeros(shape, dtype=np.uint16, order="F")
    b = port.compress(arr, markov_model_order=2)
    assert len(b) == 29 and crackle_amd.recompress(b) == b
    assert crackle_amd.recompress(b, markov_model_order=0) == port.compress(arr)
  signed = rv.as_signed(voronoi[1])
  out, n = C.c_void_p(), C.c_uint64()
  assert _lib.lib().ckl_recompress(signed, len(signed), -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
  assert "Signed integer data types" in _lib.last_error()


def test_crackle_array_methods(voronoi, port):
  lab, b = voronoi
  arr = crackle_amd.CrackleArray(b)
  labels = [int(v) for v in np.unique(lab)]
  # (CrackleArray has no remap method: tests/test_cutout_cpu.py pins its absence; the function takes arr.binary)
  for out, want in ((arr.mask(labels[:2], value=4), crackle_amd.mask(b, labels[:2], value=4)),
                    (arr.mask_except(labels[:2]), crackle_amd.mask_except(b, labels[:2]))):
    assert isinstance(out, crackle_amd.CrackleArray) and out.binary == want and out.shape == arr.shape
  assert callable(arr.recompress)
