"""GPU tests of crackle_amd.connected_components (ckl_connected_components: the decoder up to the run
tables, k_run_links and the k_cc_* numbering kernels of ckl_components3d.hpp, then the host's
ckl_relabel_components) against the scipy restatement of tests/cc3d_numpy.py, which works from the
input arrays.  tests/test_connected_components_cpu.py covers the stream writer on its own.

Byte identity with compress(expected) is asserted where the input came from compress() and the
encoder picks the input's crack format for the relabelled volume (checked first, see the docstring of
connected_components); the volumes here are not near that threshold."""
import os

import numpy as np
import pytest

import cc3d_numpy
import crackle_amd
from crackle_amd import _lib, codec, synth
from test_connected_components_cpu import isolated_voxels, stripes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CONNECTIVITIES = (6, 18, 26)
ENCODINGS = (dict(), dict(allow_pins=True), dict(markov_model_order=5))


def _run(binary, connectivity, want, mapping, checker, reference_kw=None):
  """The result stream of `binary` against the restated volume `want` (and, with reference_kw, against
  compress(want) byte for byte)."""
  out, got_map = crackle_amd.connected_components(binary, connectivity=connectivity, return_mapping=True)
  assert crackle_amd.connected_components(binary, connectivity=connectivity) == out
  head = crackle_amd.header(out)
  order = "F" if head.fortran_order else "C"
  got = crackle_amd.decompress(out)
  assert got.dtype == np.uint32 and np.array_equal(got, want)
  assert got_map == mapping
  assert np.array_equal(checker.decompress(out).reshape(want.shape, order=order), want)
  assert crackle_amd.ok(out)
  if reference_kw is not None:
    ref = checker.compress(want if head.fortran_order else np.ascontiguousarray(want), **reference_kw)
    assert crackle_amd.header(ref).crack_format == head.crack_format, "volume on the crack format threshold"
    assert out == ref
  return out


def _parity(lab, checker, connectivities=CONNECTIVITIES, encodings=ENCODINGS):
  for conn in connectivities:
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    for kw in encodings:
      b = checker.compress(lab, **kw)
      _run(b, conn, want, mapping, checker, dict(markov_model_order=kw.get("markov_model_order", 0)))


@pytest.mark.parametrize("shape,cell,order", [
  ((128, 64, 9), (12, 12, 3), "F"),      # sx % 4 == 0, power-of-two rows
  ((97, 61, 7), (12, 12, 3), "F"),       # odd widths
  ((96, 80, 6), (12, 12, 3), "C"),       # C order: numbering still by (x, y, z) indices
])
def test_voronoi_with_recurring_labels(checker, shape, cell, order):
  lab = synth.as_numpy_f(synth.voronoi_labels(shape, np.uint32, seed=31, cell=cell, modulus=40))
  if order == "C":
    lab = np.ascontiguousarray(lab)
  want, _ = cc3d_numpy.connected_components(lab, 26)
  assert want.max() > len(np.unique(lab)), "labels recur in separate places"
  _parity(lab, checker)


@pytest.mark.parametrize("shape,high", [
  ((64, 48, 5), 3),       # diagonals decide almost everything
  ((130, 70, 4), 2),      # more than 2048 runs a slice: several workgroups per slice
])
def test_noise(checker, shape, high):
  lab = synth.random_labels(shape, np.uint8, seed=21, high=high)
  if high == 2:
    assert np.count_nonzero(np.diff(lab[:, :, 0].ravel(order="F").astype(np.int16))) > 2048
  c6, _ = cc3d_numpy.connected_components(lab, 6)
  c26, _ = cc3d_numpy.connected_components(lab, 26)
  assert c26.max() < c6.max()
  _parity(lab, checker)


def test_checkerboard(checker):
  x, y, z = np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij")
  lab = np.asfortranarray(((x + y + z) % 2).astype(np.uint8))
  b = checker.compress(lab)
  for conn in CONNECTIVITIES:
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    assert want.max() == (512 if conn == 6 else 1)
    _run(b, conn, want, mapping, checker, dict())


def test_combs_that_join_in_the_last_slice(checker):
  """Two interleaved combs of one label: their teeth run through every slice and the spines that
  join them lie in the last slice only, so ids given early must merge late."""
  lab = np.zeros((33, 12, 10), np.uint16, order="F")
  lab[0:33:4, 1:6, :] = 5       # teeth of comb A
  lab[2:33:4, 6:11, :] = 5      # teeth of comb B
  lab[:, 1, 9] = 5              # spine of A
  lab[:, 10, 9] = 5             # spine of B
  lab[16, :, 9] = 5             # the bridge between the spines
  lab[1:33:4, 3, 2] = 8         # something else in between
  for conn in CONNECTIVITIES:
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    assert list(mapping.values()).count(5) == 1
    for kw in ENCODINGS[:2]:
      _run(checker.compress(lab, **kw), conn, want, mapping, checker, dict())
  cut = lab.copy(order="F")
  cut[:, :, 9] = 0
  want, mapping = cc3d_numpy.connected_components(cut, 26)
  assert list(mapping.values()).count(5) == 17
  _run(checker.compress(cut), 26, want, mapping, checker, dict())


def test_staircase_forty_deep(checker):
  """A one-voxel-thick staircase through (8, 8, 40): a chain of 40 unions, one per slice."""
  lab = np.zeros((8, 8, 40), np.uint8, order="F")
  def at(i):      # a serpentine through the rows: consecutive positions are face neighbours
    return (i % 8 if (i // 8) % 2 == 0 else 7 - i % 8), i // 8
  for z in range(40):
    lab[at(z) + (z,)] = 3
    if z + 1 < 40:
      lab[at(z + 1) + (z,)] = 3      # the step under the next slice's voxel
  for conn in CONNECTIVITIES:
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    _run(checker.compress(lab), conn, want, mapping, checker, dict())
  want, _ = cc3d_numpy.connected_components(lab, 26)
  assert want.max() == 1


def test_pieces_that_touch_at_a_corner_only(checker):
  lab = np.zeros((6, 6, 3), np.uint32, order="F")
  lab[0:2, 0:2, 0] = 9
  lab[2:4, 2:4, 0] = 9      # in-plane corner of the first block: an edge neighbour in 3D
  lab[4:6, 4:6, 1] = 9      # corner neighbour of the second block across z
  lab[0, 5, 2] = 9
  lab[0, 4, 1] = 9          # edge neighbour across z
  counts = {}
  for conn in CONNECTIVITIES:
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    counts[conn] = int(want.max())
    for kw in ENCODINGS:
      _run(checker.compress(lab, **kw), conn, want, mapping, checker, dict(markov_model_order=kw.get("markov_model_order", 0)))
  assert counts == {6: 5, 18: 3, 26: 2}


def test_degenerate_shapes(checker):
  for shape in ((1, 37, 6), (41, 1, 6), (33, 27, 1), (1, 1, 9), (1, 1, 1)):
    lab = synth.random_labels(shape, np.uint16, seed=6, high=3)
    _parity(lab, checker, encodings=ENCODINGS[:2])
  for lab in (np.zeros((20, 18, 4), np.uint32, order="F"), np.full((20, 18, 4), 77, np.uint64, order="F")):
    for conn in CONNECTIVITIES:
      want, mapping = cc3d_numpy.connected_components(lab, conn)
      assert want.max() == (1 if lab.any() else 0)
      _run(checker.compress(lab), conn, want, mapping, checker, dict())
  for shape in ((0, 0, 0), (5, 0, 3), (4, 4, 0)):
    b = checker.compress(np.zeros(shape, np.uint16, order="F"), markov_model_order=3)
    out, mapping = crackle_amd.connected_components(b, return_mapping=True)
    assert mapping == {}
    assert out == checker.compress(np.zeros(shape, np.uint32, order="F"), markov_model_order=3)
    got = crackle_amd.decompress(out)
    assert got.size == 0 and got.dtype == np.uint32


def test_every_dtype(checker):
  for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
    lab = synth.random_labels((31, 29, 5), dt, seed=3, high=4)
    if dt == np.uint64:
      lab = np.asfortranarray(lab * np.uint64(1 << 40))
    _parity(lab, checker, connectivities=(6, 26), encodings=ENCODINGS[:2])
  for dt in (np.int8, np.int16, np.int32, np.int64):
    lab = np.asfortranarray((synth.random_labels((31, 29, 5), np.int64, seed=4, high=5) - 2).astype(dt))
    want, mapping = cc3d_numpy.connected_components(lab, 26)
    assert min(mapping.values()) == -2 and np.all((want == 0) == (lab == 0))
    _parity(lab, checker, connectivities=(6, 26), encodings=ENCODINGS[:2])


def _floordiv_stream(binary):
  """What the reference's floordiv_scalar(binary, 2) writes for a flat stream: the unique list
  rewritten v // 2 at its stored width, the label-section crc32c fixed, the crack codes unchanged."""
  b = bytearray(binary)
  head = crackle_amd.header(bytes(b))
  n, off = codec._label_section(bytes(b), head)
  uniq = np.frombuffer(bytes(b), dtype=head.stored_dtype, offset=off, count=n)
  b[off:off + uniq.nbytes] = (uniq // 2).astype(head.stored_dtype).tobytes()
  start = head.header_bytes + head.grid_index_bytes
  crc = _lib.lib().ckl_crc32c(bytes(b[start:start + head.num_label_bytes]), head.num_label_bytes)
  at = len(b) - (head.sz * 4 + 4)
  b[at:at + 4] = int(crc).to_bytes(4, "little")
  return bytes(b)


def test_label_merged_stream(checker):
  """Touching 2D components that share a label after a label-table rewrite are one component, even
  at connectivity 6: equality is by label."""
  lab = synth.as_numpy_f(synth.voronoi_labels((72, 64, 6), np.uint8, seed=8, cell=(8, 8, 2)))
  b = _floordiv_stream(checker.compress(lab))
  merged = np.asfortranarray(lab // 2)
  for conn in CONNECTIVITIES:
    want, mapping = cc3d_numpy.connected_components(merged, conn)
    _run(b, conn, want, mapping, checker)


@pytest.mark.parametrize("make", [isolated_voxels, stripes])
@pytest.mark.parametrize("shape,n", [((64, 32, 1), 255), ((64, 32, 1), 256), ((512, 512, 1), 65535), ((512, 512, 1), 65536)])
def test_key_width_edges_on_the_device(checker, make, shape, n):
  lab = make(shape, n)
  want, mapping = cc3d_numpy.connected_components(lab, 6)
  assert want.max() == n
  _run(checker.compress(lab), 6, want, mapping, checker, dict())


def test_medium_volume(checker):
  lab = synth.as_numpy_f(synth.voronoi_labels((256, 256, 32), np.uint32, seed=5, cell=(32, 32, 8), modulus=50))
  b = checker.compress(lab)
  for conn in (6, 26):
    want, mapping = cc3d_numpy.connected_components(lab, conn)
    _run(b, conn, want, mapping, checker, dict())


def test_repeatable(checker):
  """The same stream three times gives identical bytes: nothing depends on the order atomics land."""
  lab = synth.random_labels((130, 70, 6), np.uint8, seed=11, high=2)
  b = checker.compress(lab)
  outs = [crackle_amd.connected_components(b, connectivity=26, return_mapping=True) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2]


def test_errors(checker):
  lab = synth.as_numpy_f(synth.voronoi_labels((48, 40, 5), np.uint16, seed=12, cell=(8, 8, 2)))
  b = checker.compress(lab)
  with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
    crackle_amd.connected_components(b, connectivity=4)
  with pytest.raises(ValueError, match="binary_image=True is not supported"):
    crackle_amd.connected_components(b, binary_image=True)
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    v0 = z[[k for k in z.files if "." not in k][0]].tobytes()
  with pytest.raises(ValueError, match="version 0"):
    crackle_amd.connected_components(v0)
  # a corrupted label section: slice 1 claims one component more, slice 2 one fewer
  head = crackle_amd.header(b)
  n, off = codec._label_section(b, head)
  at = off + n * head.stored_data_width
  cw = 2      # components per slice are stored at the byte width of sx * sy = 1920
  bad = bytearray(b)
  for z, d in ((1, 1), (2, -1)):
    v = int.from_bytes(bad[at + z * cw:at + (z + 1) * cw], "little") + d
    bad[at + z * cw:at + (z + 1) * cw] = v.to_bytes(cw, "little")
  with pytest.raises(RuntimeError, match="component count does not match the label section"):
    crackle_amd.decompress(bytes(bad))
  with pytest.raises(RuntimeError, match="component count does not match the label section"):
    crackle_amd.connected_components(bytes(bad))
