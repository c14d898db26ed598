"""Stream surgery on .ckl bytes without decoding — the slab merge the sharded encoder is built
on, exposed with the reference's names (crackle/operations.py:424-662: zstack, zsplit,
zshatter).  Host only (native: ckl_zstack / ckl_zsplit); FLAT label streams.  The consumers
array_equal, mode_pooling_2x2x1, point_cloud, contacts, overlaps, connected_components and dust run on the device.
The label edits remap, mask and mask_except rewrite header and label section on the host; recompress
re-encodes a stream from its own labels on the device (ckl_recompress), without decoding a voxel.  erode and dilate
take the same road with the eroded or dilated labels at its end (ckl_erode, ckl_dilate); opening and closing are one
after the other.  downsample takes it with the pooled labels, and a smaller volume, at its end (ckl_downsample).
overlay and mask_by take it with two streams of one shape at its start and a rule on their labels (ckl_combine)."""
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .codec import contains, header, labels


def _take(out: C.c_void_p, n: C.c_uint64) -> bytes:
  try:
    return C.string_at(out.value, n.value)
  finally:
    _lib.lib().ckl_free(out)


def _checked_connectivity(what: str, connectivity: int) -> None:
  if connectivity not in (6, 18, 26):
    raise ValueError(f"{what}: connectivity must be 6, 18 or 26. Got: {connectivity}")


def _checked_order(what: str, markov_model_order: Optional[int]) -> None:
  if markov_model_order is not None and int(markov_model_order) < 0:
    raise ValueError(f"{what}: markov_model_order must not be negative. Got: {int(markov_model_order)}")


def _reencode(what: str, entry: str, binary: bytes, edit_args: tuple, markov_model_order: Optional[int], device: int) -> bytes:
  """The call that recompress, erode and dilate share: `entry` is the library's function, which takes the stream,
  the operation's own arguments, the order (-1: the stream's own), the device and the output pair."""
  from .codec import _raise
  b = bytes(binary)
  if header(b).signed:
    raise TypeError("Signed integer data types are not currently supported.")
  _checked_order(what, markov_model_order)
  order = -1 if markov_model_order is None else int(markov_model_order)
  out, n = C.c_void_p(), C.c_uint64()
  rc = getattr(_lib.lib(), entry)(b, len(b), *edit_args, order, int(device), C.byref(out), C.byref(n))
  if rc != _lib.CKL_OK:
    _raise(rc)
  return _take(out, n)


def zstack(images: Sequence[bytes]) -> bytes:
  """Concatenates the streams of consecutive z-slabs into the stream of the whole volume
  (crackle/operations.py:424-548); byte-identical to compress() of the whole when the slabs
  agree on the crack format (automated_test.py:468-487).  The result's label list is the sorted union of the slabs'
  lists, which may be out of order or hold duplicates.  FLAT label streams of format version 1 only: a pin label
  stream or a version 0 stream raises ValueError (recompress() gives a FLAT version 1 stream first), and so do slabs
  that disagree on shape, dtype, crack format or markov order, as in the reference ("All crack formats must match.")."""
  bufs = [bytes(b) for b in images]
  if not bufs:
    raise ValueError("zstack needs at least one stream")
  # The reference brings every input to markov order 0 first (operations.py:447-457).  Slabs
  # that share one model (the sharded encoder's, or the parts of one stream) are merged as they
  # are; otherwise the codes are re-encoded to order 0 on the device, like the reference.
  heads = [header(b) for b in bufs]
  def _model(b, h):
    off = h.header_bytes + h.grid_index_bytes + h.num_label_bytes
    return b[off:off + h.markov_model_bytes]
  orders = {h.markov_model_order for h in heads}
  if orders != {0} and (len(orders) > 1 or len({_model(b, h) for b, h in zip(bufs, heads)}) > 1):
    from .codec import reencode
    bufs = [reencode(b, 0) for b in bufs]
  L = _lib.lib()
  arr = (C.c_char_p * len(bufs))(*bufs)
  lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
  out, n = C.c_void_p(), C.c_uint64()
  if L.ckl_zstack(arr, lens, len(bufs), C.byref(out), C.byref(n)) != _lib.CKL_OK:
    raise ValueError(_lib.last_error())
  return _take(out, n)


def _zrange(binary: bytes, z_start: int, z_end: int) -> bytes:
  out, n = C.c_void_p(), C.c_uint64()
  if _lib.lib().ckl_zsplit(binary, len(binary), z_start, z_end, C.byref(out), C.byref(n)) != _lib.CKL_OK:
    raise ValueError(_lib.last_error())
  return _take(out, n)


def zsplit(binary: bytes, z: int) -> Tuple[bytes, bytes, bytes]:
  """(before, middle, after) streams around slice z (crackle/operations.py:626-647); empty
  ranges come back as b''.  Each part keeps the labels its slices use, in the order of the input's list.  Pin label
  streams and format version 0 raise ValueError, as for zstack."""
  head = header(binary)
  if z < 0 or z >= head.sz:
    raise ValueError(f"{z} is outside the range 0 to {head.sz}.")
  before = _zrange(binary, 0, z) if z > 0 else b""
  middle = _zrange(binary, z, z + 1)
  after = _zrange(binary, z + 1, head.sz) if z + 1 < head.sz else b""
  return before, middle, after


def zshatter(binary: bytes) -> List[bytes]:
  """One stream per z-slice (crackle/operations.py:649-662)."""
  head = header(binary)
  return [_zrange(binary, z, z + 1) for z in range(head.sz)]


def array_equal(binary1: bytes, binary2: bytes, parallel: int = 0, device: int = 0) -> bool:
  """Do the two streams hold the same array, whatever their encoding: dtype, FLAT or pin labels, format version,
  markov order, memory order, label list in or out of order or with duplicates, false boundaries.

  Shapes and label sets are compared on the host, as the reference compares them first (crackle/operations.py:966-994;
  it compares the lists as stored, which calls a remapped stream unequal to its own canonical form).  The voxels are
  then compared on the device through the contingency table of the two streams (ckl_overlaps): the arrays are equal
  iff no voxel pairs two different labels.  The reference's fastcrackle.array_equal (src/operations.hpp:1039-1184,
  kept as ckl_array_equal) compares the component counts of the slices and reads both streams through the first
  one's component -> label table, so it calls a stream with false boundaries unequal to its re-encoding and cannot
  see labels exchanged between components; it still answers for streams without voxels."""
  b1, b2 = bytes(binary1), bytes(binary2)
  h1, h2 = header(b1), header(b2)
  if h1.sx != h2.sx or h1.sy != h2.sy or h1.sz != h2.sz:
    return False
  u1, u2 = np.unique(labels(b1)), np.unique(labels(b2))
  if u1.size != u2.size or np.any(u1 != u2):
    return False
  if h1.voxels() == 0:
    eq = C.c_int(0)
    if _lib.lib().ckl_array_equal(b1, len(b1), b2, len(b2), int(device), C.byref(eq)) != _lib.CKL_OK:
      raise RuntimeError(_lib.last_error())
    return bool(eq.value)
  pairs, _ = _overlap_counts(b1, b2, 0, -1, device)
  return bool((pairs[:, 0] == pairs[:, 1]).all())


def _mode_pooling_slices(binary: bytes, z_start: int = 0, z_end: int = -1, device: int = 0) -> List[bytes]:
  """fastcrackle.mode_pooling_2x2x1 (src/fastcrackle.cpp:620-639): one pooled stream per slice."""
  b = bytes(binary)
  out, n, lens, cnt = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  if L.ckl_mode_pooling_2x2x1(b, len(b), int(z_start), int(z_end), int(device), C.byref(out), C.byref(n), C.byref(lens), C.byref(cnt)) != _lib.CKL_OK:
    raise RuntimeError(_lib.last_error())
  try:
    sizes = list((C.c_uint64 * cnt.value).from_address(lens.value)) if cnt.value else []
    blob = C.string_at(out.value, n.value) if n.value else b""
  finally:
    if out.value:
      L.ckl_free(out)
    if lens.value:
      L.ckl_free(lens)
  res, at = [], 0
  for m in sizes:
    res.append(blob[at:at + m])
    at += m
  return res


def mode_pooling_2x2x1(binary: bytes, parallel: int = 0, device: int = 0) -> bytes:
  """Downsamples a segmentation 2 x 2 x 1 by the reference's pooling rule
  (crackle/operations.py:1023-1026: the per-slice streams of fastcrackle.mode_pooling_2x2x1, stacked).  Every pooled
  slice is compressed on its own and picks its own crack format; where the slices do not all pick the same one
  (noise of two or three labels does that) zstack cannot join them and raises ValueError, as the reference does."""
  return zstack(_mode_pooling_slices(binary, 0, -1, device))


def _point_cloud_raw(binary: bytes, z_start: int, z_end: int, label_list, skip_background: bool, device: int) -> Dict[int, np.ndarray]:
  """fastcrackle.point_cloud (src/fastcrackle.cpp:315-345 -> ckl_point_cloud): dict label -> flat
  uint16 array of (x, y, z) triples."""
  b = bytes(binary)
  sel = None if label_list is None else np.ascontiguousarray(label_list, dtype=np.uint64)
  lab_p, off_p, pts_p, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  rc = L.ckl_point_cloud(b, len(b), int(z_start), int(z_end), None if sel is None else sel.ctypes.data,
                         0 if sel is None else sel.size, int(sel is not None), int(bool(skip_background)), int(device),
                         C.byref(lab_p), C.byref(off_p), C.byref(pts_p), C.byref(n))
  if rc != _lib.CKL_OK:
    raise RuntimeError(_lib.last_error())
  try:
    k = int(n.value)
    if k == 0:
      return {}
    labs = np.ctypeslib.as_array(C.cast(lab_p, C.POINTER(C.c_uint64)), shape=(k,)).tolist()
    offs = (3 * np.ctypeslib.as_array(C.cast(off_p, C.POINTER(C.c_uint64)), shape=(k + 1,))).tolist()
    # one copy out of the library's buffer; the labels' arrays are views of it
    pts = np.ctypeslib.as_array(C.cast(pts_p, C.POINTER(C.c_uint16)), shape=(offs[k],)).copy() if offs[k] else np.zeros(0, np.uint16)
    return {labs[i]: pts[offs[i]:offs[i + 1]] for i in range(k)}
  finally:
    for p in (lab_p, off_p, pts_p):
      if p.value:
        L.ckl_free(p)


def point_cloud(
  binary: bytes, label: Optional[Union[int, List[int]]] = None, parallel: int = 0,
  z_start: int = -1, z_end: int = -1, skip_background: bool = True, device: int = 0,
) -> Union[np.ndarray, Dict[int, np.ndarray]]:
  """Surface point clouds of the labels without decompressing the image (crackle/codec.py:804-872).

  Without `label`: dict label -> (N, 3) uint16 array of (x, y, z).  With an int: that label's
  array; with a list: the dict restricted to those labels.  A label the image does not contain
  raises ValueError.  The reference narrows an unspecified z-range to the slices that hold the
  labels (z_range_for_label); slices without them contribute no points, so the whole range is
  traced here instead.  Points come in the order the reference gives with parallel = 1."""
  scalar_input = False
  if isinstance(label, (int, np.integer)):
    scalar_input = True
    label = [int(label)]
  head = header(binary)
  if isinstance(label, (list, tuple)):
    for lbl in label:
      if not contains(binary, lbl):
        raise ValueError(f"Label {lbl} not contained in image.")
  if z_start == -1:
    z_start = 0
  if z_end == -1:
    z_end = head.sz
  ptc = _point_cloud_raw(binary, z_start, z_end, label, skip_background, device)
  if len(ptc) == 0:
    if label:
      return np.zeros([0, 3], dtype=np.uint16, order="C")
    return {}
  for lbl, pts in ptc.items():
    ptc[lbl] = np.asarray(pts, dtype=np.uint16, order="C").reshape([len(pts) // 3, 3], order="C")
  if scalar_input:
    return ptc[label[0]]
  return ptc


def _contacts_counts(binary: bytes, z_start: int = 0, z_end: int = -1, device: int = 0):
  """ckl_decoder_contacts over the range, clamped by operations::contacts' rule first
  (src/operations.hpp:878-888): (pairs uint64 [n, 2], faces uint64 [n, 3]), ascending by (a, b)."""
  b = bytes(binary)
  head = header(b)
  sz = int(head.sz)
  zs = max(min(int(z_start), sz - 1), 0)
  ze = sz if z_end < 0 else int(z_end)
  ze = max(min(ze, sz), 0)
  if zs >= ze:
    raise RuntimeError(f"crackle: Invalid range: {zs} - {ze}")
  empty = (np.zeros((0, 2), np.uint64), np.zeros((0, 3), np.uint64))
  if int(head.sx) * int(head.sy) == 0:
    return empty
  L = _lib.lib()
  handle = C.c_void_p()
  if L.ckl_decoder_create(b, len(b), zs, ze, int(device), C.byref(handle)) != _lib.CKL_OK:
    raise RuntimeError(_lib.last_error())
  pp, fp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
  try:
    if L.ckl_decoder_contacts(handle, C.byref(pp), C.byref(fp), C.byref(n)) != _lib.CKL_OK:
      raise RuntimeError(_lib.last_error())
    k = int(n.value)
    if k == 0:
      return empty
    pairs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint64)), shape=(k, 2)).copy()
    faces = np.ctypeslib.as_array(C.cast(fp, C.POINTER(C.c_uint64)), shape=(k, 3)).copy()
    return pairs, faces
  finally:
    for p in (pp, fp):
      if p.value:
        L.ckl_free(p)
    L.ckl_decoder_destroy(handle)


def contacts(
  binary: bytes, anisotropy: Tuple[float, float, float] = (1.0, 1.0, 1.0), device: int = 0,
) -> Dict[Tuple[int, int], float]:
  """6-connected contact area between touching labels (crackle/operations.py:956-964,
  src/operations.hpp:850-1021): {(a, b): area} with a <= b as uint64 (signed labels
  sign-extended, so -1 is 2**64 - 1); label 0 is left out.  In-plane faces count between
  different components of a slice, so a stream whose label table was rewritten without
  re-encoding reports pairs (a, a); z faces count between different labels.

  One difference from the reference, on purpose: the device counts the faces of every pair per
  axis exactly, and the area is the float32 nearest to nx*wy*wz + ny*wx*wz + nz*wx*wy (face
  areas as float32 products of the float32 weights, the sum in float64).  The reference adds one
  float32 per face; both agree wherever its running sum is exact (integer or dyadic weights
  below 2^24 units of the smallest face), and beyond that the reference's sum rounds or stalls
  (at 16777216.0 with unit weights) where this one does not."""
  wx, wy, wz = (np.float32(w) for w in anisotropy)
  ax, ay, az = float(np.float32(wy * wz)), float(np.float32(wx * wz)), float(np.float32(wx * wy))
  pairs, faces = _contacts_counts(binary, 0, -1, device)
  out = {}
  for (a, b), (nx, ny, nz) in zip(pairs.tolist(), faces.tolist()):
    out[(a, b)] = float(np.float32(nx * ax + ny * ay + nz * az))
  return out


def _overlap_counts(binary_a: bytes, binary_b: bytes, z_start: int = 0, z_end: int = -1, device: int = 0):
  """ckl_overlaps over the range: (pairs uint64 [n, 2], counts uint64 [n]), ascending by (a, b)."""
  from .codec import _raise
  a, b = bytes(binary_a), bytes(binary_b)
  ha, hb = header(a), header(b)
  if (ha.sx, ha.sy, ha.sz) != (hb.sx, hb.sy, hb.sz):
    raise ValueError(
      f"overlaps: the volumes differ in shape: {ha.sx} x {ha.sy} x {ha.sz} and {hb.sx} x {hb.sy} x {hb.sz}")
  L = _lib.lib()
  pp, cp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
  try:
    rc = L.ckl_overlaps(a, len(a), b, len(b), int(z_start), int(z_end), int(device), C.byref(pp), C.byref(cp), C.byref(n))
    if rc != _lib.CKL_OK:
      _raise(rc)
    k = int(n.value)
    if k == 0:
      return np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)
    pairs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint64)), shape=(k, 2)).copy()
    counts = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(k,)).copy()
    return pairs, counts
  finally:
    for p in (pp, cp):
      if p.value:
        L.ckl_free(p)


def overlaps(
  binary_a: bytes, binary_b: bytes, z_start: int = 0, z_end: int = -1, device: int = 0,
) -> Dict[Tuple[int, int], int]:
  """The contingency table (overlap matrix) of two segmentations of one volume: {(a, b): voxels}
  for every pair of labels for which some voxel has label a in binary_a and b in binary_b, the
  input of variation of information, Rand indices, per-object IoU and split / merge counts.  The
  reference has no such function.

  Labels are uint64 values (signed labels sign-extended, so -3 is 2**64 - 3).  Label 0 is a label
  like any other and nothing is dropped: the counts sum to the voxels of the range, the sums over b
  are the voxel counts of binary_a and the sums over a those of binary_b.  The pair is ordered, not
  min / max.  The streams must agree in shape (ValueError otherwise) and may differ in everything
  else: dtype, FLAT or pin labels, format version, crack format, markov order, memory order.  The
  z-range is clamped as by the other consumers; one without a slice raises RuntimeError.

  Nothing is decoded to voxels: the device intersects the runs of the two streams row by row
  (ckl_overlaps).  A damaged slice raises what decompress raises for that stream."""
  pairs, counts = _overlap_counts(binary_a, binary_b, z_start, z_end, device)
  return {(a, b): n for (a, b), n in zip(pairs.tolist(), counts.tolist())}


def relabel_components(binary: bytes, new_ids) -> bytes:
  """The stream with 2D component i of its slices (stream order) given the value new_ids[i]: uint32,
  FLAT labels, everything but header and label section copied (ckl_relabel_components; host only)."""
  b = bytes(binary)
  ids = np.ascontiguousarray(new_ids, dtype=np.uint64)
  out, n = C.c_void_p(), C.c_uint64()
  if _lib.lib().ckl_relabel_components(b, len(b), ids.ctypes.data, ids.size, C.byref(out), C.byref(n)) != _lib.CKL_OK:
    raise ValueError(_lib.last_error())
  return _take(out, n)


def connected_components(
  binary: bytes, connectivity: int = 26, binary_image: bool = False,
  memory_target: int = int(100e6), progress: bool = False,
  return_mapping: bool = False, device: int = 0,
) -> Union[bytes, Tuple[bytes, Dict[int, int]]]:
  """3D connected component labelling of a stream, as a new stream (crackle/operations.py:859-934,
  which needs the cc3d package; like it this returns bytes, whatever its docstring says).

  Every voxel whose label is not 0 is foreground (negative labels too); label 0 stays 0.  Two
  foreground voxels are in one component when a chain of voxels with the SAME LABEL joins them by
  6-, 18- or 26-neighbour steps (`connectivity`).  With return_mapping: also {component id:
  original label}, labels as crackle_amd.labels(binary) reports them.

  Numbering is this project's own definition: components are numbered 1 .. N in the order of their
  first voxel, x fastest, then y, then z, in array indices, whatever the stream's fortran_order
  flag.  (cc3d.connected_components is expected to give the same order for a Fortran-ordered volume;
  that package was not at hand to check.)

  Nothing is decoded to voxels.  The crack codes already hold the 4-connected components of every
  slice, and in-plane neighbours with one label are one such component, so no crack changes: the
  device links the 2D components across rows, diagonals and slices (ckl_connected_components) and
  only header and label section are written anew; z-index, markov model, crack codes and slice crcs
  are the input's bytes.  The output is uint32 with FLAT labels, format version 1.  It equals
  compress(result.astype(uint32), markov_model_order=m) byte for byte when the input came from
  compress() with markov order m and the encoder picks the same crack_format for the relabelled
  volume.  The encoder takes that format from pixel_pairs < voxels / 2 (src/crackle.hpp:48-55);
  relabelling can only lower pixel_pairs, at row and slice wrap-arounds, so only a volume sitting on
  that threshold comes out with the other format.  This function always keeps the input's.

  memory_target and progress are accepted for the reference's signature and ignored: there are no
  slabs.  binary_image=True (all nonzero voxels one foreground) merges different labels, which
  removes cracks and needs a re-encode: ValueError.  Format version 0 streams carry no crack crcs:
  ValueError.  FLAT and pin label streams are accepted."""
  _checked_connectivity("connected_components", connectivity)
  if binary_image:
    raise ValueError(
      "connected_components: binary_image=True is not supported: merging different labels removes "
      "cracks, which needs a re-encode of the crack codes.")
  b = bytes(binary)
  head = header(b)
  if head.format_version == 0:
    raise ValueError("connected_components: format version 0 streams have no crack crcs to carry over; re-compress first.")
  L = _lib.lib()
  out, n, lab, cnt = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
  rc = L.ckl_connected_components(b, len(b), int(connectivity), int(device), C.byref(out), C.byref(n),
                                  C.byref(lab) if return_mapping else None, C.byref(cnt))
  if rc != _lib.CKL_OK:
    if rc == _lib.CKL_ERR_ARG:
      raise ValueError(_lib.last_error())
    raise RuntimeError(_lib.last_error())
  try:
    result = C.string_at(out.value, n.value)
    if not return_mapping:
      return result
    k = int(cnt.value)
    orig = np.ctypeslib.as_array(C.cast(lab, C.POINTER(C.c_uint64)), shape=(k,)).copy() if k else np.zeros(0, np.uint64)
    if head.signed:
      orig = orig.view(np.int64)
    return result, {i + 1: v for i, v in enumerate(orig.tolist())}
  finally:
    L.ckl_free(out)
    if lab.value:
      L.ckl_free(lab)


def relabel_values(binary: bytes, values) -> bytes:
  """The stream with 2D component i of its slices (stream order) given the label values[i], at the input's data
  width, as the canonical FLAT stream dust() documents (ckl_relabel_values; host only)."""
  b = bytes(binary)
  vals = np.ascontiguousarray(values, dtype=np.uint64)
  out, n = C.c_void_p(), C.c_uint64()
  if _lib.lib().ckl_relabel_values(b, len(b), vals.ctypes.data, vals.size, C.byref(out), C.byref(n)) != _lib.CKL_OK:
    raise ValueError(_lib.last_error())
  return _take(out, n)


def dust(
  binary: bytes, threshold: int, connectivity: int = 26, binary_image: bool = False,
  invert: bool = False, return_removed: bool = False, device: int = 0,
) -> Union[bytes, Tuple[bytes, int]]:
  """The stream without its "dust" (cc3d's dust; the reference has none): every voxel of a 3D component with fewer
  than `threshold` voxels becomes 0, nothing else changes.  With return_removed: also the number of 3D components
  set to 0.

  A component is what connected_components documents: a maximal set of voxels with the same nonzero label joined
  by 6-, 18- or 26-neighbour steps; equality is by label, so touching 2D components that share a label after
  remap() are one component.  binary_image=True groups all nonzero voxels instead, whatever their labels; only the
  grouping changes, survivors keep their own labels.  invert=True removes the components with `threshold` voxels
  or more instead.  A threshold of 0 or 1 without invert removes nothing.

  Nothing is decoded to voxels and no crack changes: the device links the 2D components of the slices as
  connected_components does, sums the run lengths of every 3D component and rewrites the labels (ckl_dust).  The
  result is a canonical FLAT stream, format version 1, as remap() documents its result: the unique list ascending
  without duplicates, without the labels nothing carries any more and with 0 when something was removed, the keys
  at the width of the new count, the stored width from the largest remaining label, is_sorted set.  Data width
  and fortran_order flag are the input's; z-index, markov model, crack codes and slice crcs are the input's bytes.
  If nothing is removed and the input is a FLAT version 1 stream from compress(), the output is the input.
  Removed components keep their cracks ("false boundaries"): recompress(dust(b)) is the whole clean-up pass.

  FLAT and pin label streams are accepted (a pin stream comes back FLAT).  Format version 0 raises ValueError,
  signed streams TypeError, a negative threshold or one of 2^64 or more ValueError, a connectivity other than
  6, 18 or 26 ValueError.  The stream of an empty volume is returned as it is, without a device.  A damaged slice
  raises what decompress raises for it."""
  from .codec import _raise
  _checked_connectivity("dust", connectivity)
  threshold = int(threshold)
  if threshold < 0:
    raise ValueError(f"dust: threshold must not be negative. Got: {threshold}")
  if threshold >= 1 << 64:
    raise ValueError(f"dust: threshold must be below 2^64. Got: {threshold}")
  b = bytes(binary)
  head = header(b)
  if head.format_version == 0:
    raise ValueError("dust: format version 0 streams have no crack crcs to carry over; recompress() first.")
  if head.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  if head.voxels() == 0:
    return (b, 0) if return_removed else b
  flags = (_lib.CKL_DUST_BINARY_IMAGE if binary_image else 0) | (_lib.CKL_DUST_INVERT if invert else 0)
  out, n, removed = C.c_void_p(), C.c_uint64(), C.c_uint64()
  rc = _lib.lib().ckl_dust(b, len(b), threshold, int(connectivity), flags, int(device), C.byref(out), C.byref(n),
                           C.byref(removed) if return_removed else None)
  if rc != _lib.CKL_OK:
    _raise(rc)
  result = _take(out, n)
  return (result, int(removed.value)) if return_removed else result


def fill_holes(binary: bytes, connectivity: int = 6, return_filled: bool = False, device: int = 0) -> Union[bytes, Tuple[bytes, int]]:
  """The stream with its enclosed background voids filled (the fill_holes of fill_voids and fastmorph; the
  reference has none).  With return_filled: also the number of holes filled.

  A hole is a maximal set of voxels with label 0 joined by 6-, 18- or 26-neighbour steps: `connectivity` is the
  background's, and at 6 the surrounding object only needs to be 26-connected around the hole.  A hole is filled
  with label L when both hold: (1) none of its voxels lies on a face of the volume (x = 0, x = sx - 1, y = 0,
  y = sy - 1, z = 0 or z = sz - 1); (2) every face neighbour of its voxels that is not itself in the hole carries
  the same label L, where only the 6 face neighbours count, whatever `connectivity` is.  Every other hole stays 0:
  one on the border, and one that touches two or more labels by faces.  Nothing else changes.  So a volume with
  sz = 1 has no fillable hole, diagonal contact with a second label does not prevent filling, and, equality being
  by label, background components separated only by "false boundaries" (the output of dust() or mask() before
  recompress()) are one hole.

  Nothing is decoded to voxels and no crack changes: the device links label 0's 2D components as
  connected_components links the others, scans the face neighbours of every background run into one state word
  per hole and rewrites the labels (ckl_fill_holes).  The result is a canonical FLAT stream, format version 1, as
  dust() documents its own: the unique list ascending without duplicates (label 0 leaves it when every hole was
  filled), the keys at the width of the new count, the stored width from the largest remaining label, is_sorted
  set.  Data width and fortran_order flag are the input's; z-index, markov model, crack codes and slice crcs are
  the input's bytes.  If nothing is filled and the input is a FLAT version 1 stream from compress(), the output is
  the input.  Filled holes keep their cracks ("false boundaries") until recompress().

  FLAT and pin label streams are accepted (a pin stream comes back FLAT).  A connectivity other than 6, 18 or 26
  raises ValueError, format version 0 ValueError, signed streams TypeError.  The stream of an empty volume is
  returned as it is, without a device.  A damaged slice raises what decompress raises for it.

  Not done: filling holes with more than one surrounding label (an `ambiguous=` policy), a size limit on holes,
  per-label filling that swallows enclosed foreign labels (fastmorph's remove_enclosed), z-ranges, a sharded
  version."""
  from .codec import _raise
  _checked_connectivity("fill_holes", connectivity)
  b = bytes(binary)
  head = header(b)
  if head.format_version == 0:
    raise ValueError("fill_holes: format version 0 streams have no crack crcs to carry over; recompress() first.")
  if head.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  if head.voxels() == 0:
    return (b, 0) if return_filled else b
  out, n, filled = C.c_void_p(), C.c_uint64(), C.c_uint64()
  rc = _lib.lib().ckl_fill_holes(b, len(b), int(connectivity), int(device), C.byref(out), C.byref(n),
                                 C.byref(filled) if return_filled else None)
  if rc != _lib.CKL_OK:
    _raise(rc)
  result = _take(out, n)
  return (result, int(filled.value)) if return_filled else result


# ---- label edits: remap / mask / mask_except on the host, recompress on the device ------------------------------------
def _byte_width(x: int) -> int:
  return 1 if x <= 0xFF else 2 if x <= 0xFFFF else 4 if x <= 0xFFFFFFFF else 8


def _crc8(data: bytes) -> int:
  """The header's checksum (src/crc.hpp:23-49)."""
  crc = 0xFF
  for byte in data:
    crc ^= byte
    for _ in range(8):
      crc = (crc >> 1) ^ 0xE7 if crc & 1 else crc >> 1
  return crc


def _editable_header(binary: bytes, what: str):
  head = header(binary)
  if head.format_version == 0:
    raise ValueError(f"{what}: format version 0 streams have no label crc to rewrite; recompress() first.")
  if head.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  if head.voxels() != 0 and head.label_format != 0:
    raise ValueError(f"{what}: pin label streams have no label per component to rewrite; recompress() gives a FLAT stream first.")
  return head


def _flat_section(binary: bytes, head):
  """(unique labels, the components-per-slice block as bytes, the key of every component) of a FLAT label section
  (src/labels.hpp:92-155)."""
  off = head.header_bytes + head.grid_index_bytes
  sec = binary[off:off + head.num_label_bytes]
  n_uniq = int.from_bytes(sec[:8], "little")
  uniq = np.frombuffer(sec, dtype=f"<u{head.stored_data_width}", count=n_uniq, offset=8)
  at = 8 + n_uniq * head.stored_data_width
  per_slice = sec[at:at + head.sz * _byte_width(head.sx * head.sy)]
  at += len(per_slice)
  kw = _byte_width(n_uniq)
  keys = np.frombuffer(sec, dtype=f"<u{kw}", count=(len(sec) - at) // kw, offset=at)
  return uniq, per_slice, keys


def _with_labels(binary: bytes, head, new_values: np.ndarray) -> bytes:
  """The stream with label i of its unique list replaced by new_values[i] (uint64), as a canonical FLAT stream."""
  _, per_slice, keys = _flat_section(binary, head)
  uniq, inverse = np.unique(new_values, return_inverse=True)
  top = int(uniq[-1])
  stored_width = _byte_width(top)
  data_width = max(head.data_width, stored_width)
  section = b"".join((
    len(uniq).to_bytes(8, "little"), uniq.astype(f"<u{stored_width}").tobytes(), per_slice,
    inverse.astype(np.uint64)[keys].astype(f"<u{_byte_width(len(uniq))}").tobytes(),
  ))
  fmt = int.from_bytes(binary[5:7], "little")
  fmt &= ~0xF & ~(1 << 13)      # data width, stored width; "not sorted" cleared
  fmt |= {1: 0, 2: 1, 4: 2, 8: 3}[data_width] | ({1: 0, 2: 1, 4: 2, 8: 3}[stored_width] << 2)
  body = binary[4:5] + fmt.to_bytes(2, "little") + binary[7:20] + len(section).to_bytes(8, "little")
  off = head.header_bytes + head.grid_index_bytes
  rest = binary[off + head.num_label_bytes:]
  crcs_at = len(rest) - 4 * (head.sz + 1)
  crc = _lib.lib().ckl_crc32c(section, len(section))
  return b"".join((binary[:4], body, bytes([_crc8(body[1:])]), binary[head.header_bytes:off], section,
                   rest[:crcs_at], crc.to_bytes(4, "little"), rest[crcs_at + 4:]))


def remap(binary: bytes, mapping: dict, preserve_missing_labels: bool = False, parallel: int = 0) -> bytes:
  """The stream in which every voxel v has the value mapping[v] (crackle/codec.py:747-776): only header and label
  section are rewritten, z-index, markov model, crack codes and slice crcs are the input's bytes.  A label of the
  stream without a key raises KeyError unless preserve_missing_labels, which keeps it; keys the stream does not
  hold are ignored.  `parallel` is accepted and ignored.

  One difference from the reference, on purpose: its remap overwrites the unique list in place, which leaves it
  unsorted, with duplicates where labels were merged, and clears is_sorted.  Here the result is always a canonical
  FLAT stream, what the reference's condense_unique (crackle/codec.py:778-802) would make of that: the unique list
  ascending without duplicates, the keys re-indexed at the width of the new count, the stored width from the
  largest label, the data width grown (never shrunk) to hold it, is_sorted set.  contains() and the decoder's
  label table rely on the sorted list, so every function of this package keeps working on the result.

  Merged labels keep the crack between their components ("false boundaries"): recompress() removes them.
  Pin label streams (recompress() gives a FLAT stream first) and format version 0 raise ValueError, signed streams
  TypeError, new values outside 0 .. 2^64 - 1 ValueError."""
  b = bytes(binary)
  head = _editable_header(b, "remap")
  for v in mapping.values():
    if not 0 <= int(v) < (1 << 64):
      raise ValueError(f"remap: value {v} is outside 0 .. 2^64 - 1")
  if head.voxels() == 0:
    return b
  uniq, _, _ = _flat_section(b, head)
  new_values = np.empty(len(uniq), dtype=np.uint64)
  for i, label in enumerate(uniq.tolist()):
    if label in mapping:
      new_values[i] = int(mapping[label])
    elif preserve_missing_labels:
      new_values[i] = label
    else:
      raise KeyError(label)
  return _with_labels(b, head, new_values)


def mask(binary: bytes, labels: list, value: int = 0, parallel: int = 0) -> bytes:
  """The stream with every label in `labels` replaced by `value` (crackle/operations.py:1028-1046); see remap()."""
  return remap(binary, {int(label): value for label in labels}, preserve_missing_labels=True, parallel=parallel)


def mask_except(binary: bytes, labels: list, value: int = 0, parallel: int = 0) -> bytes:
  """The stream with every label NOT in `labels` replaced by `value` (crackle/operations.py:1048-1070); see remap()."""
  b = bytes(binary)
  head = _editable_header(b, "mask_except")
  if head.voxels() == 0:
    return remap(b, {}, preserve_missing_labels=True)
  keep = {int(label) for label in labels}
  uniq, _, _ = _flat_section(b, head)
  return remap(b, {label: value for label in uniq.tolist() if label not in keep}, preserve_missing_labels=True, parallel=parallel)


def recompress(
  binary: bytes, memory_target: int = int(4e9), allow_pins: bool = False,
  markov_model_order: Optional[int] = None, device: int = 0,
) -> bytes:
  """compress(decompress(binary), markov_model_order=m), byte for byte, without the voxels
  (crackle/operations.py:664-857 decodes slabs and compresses them again): the stream re-encoded from its own labels,
  which removes the cracks remap() and mask() leave between components that now share a label.  m is the input's
  order unless markov_model_order is given.  The output has FLAT labels, format version 1, whatever the input had
  (FLAT, pins, version 0), and the input's data width and fortran_order flag.

  On the device the decoder runs up to its run tables and component -> label map; one kernel writes the encoder's
  "labels differ" planes and the volume's statistics from them, and the encoder's crack and label stages follow
  (ckl_recompress).  memory_target is accepted and ignored: there are no slabs.  allow_pins=True raises ValueError
  (pins need the voxel columns), signed streams TypeError as compress does; a damaged slice raises what
  decompress raises for it."""
  if allow_pins:
    raise ValueError("recompress: allow_pins is not supported: pins are found along the voxel columns, which are never decoded here.")
  return _reencode("recompress", "ckl_recompress", binary, (), markov_model_order, device)


def erode(
  binary: bytes, connectivity: int = 26, erode_border: bool = True,
  markov_model_order: Optional[int] = None, device: int = 0,
) -> bytes:
  """compress(eroded, markov_model_order=m), byte for byte, where eroded is the stream's volume with every label
  peeled back by one voxel (fastmorph's erode; the reference has none), without the voxels.

  A voxel keeps its label L != 0 iff every neighbour of the structuring element carries L; otherwise it becomes 0.
  The element is the 6, 18 or 26 offsets (dx, dy, dz) in {-1, 0, 1}^3 with 0 < |dx| + |dy| + |dz| <= 1, 2, 3.
  Equality is by label: the false boundaries that remap, mask, dust or fill_holes leave erode nothing.  With
  erode_border a neighbour outside the volume counts as different (every voxel on a face of the volume goes);
  without it such neighbours are ignored, which for these elements is edge replication.  One iteration per call.

  m is the input's order unless markov_model_order is given.  The output has FLAT labels, format version 1,
  whatever the input had (FLAT, pins, version 0), the input's data width and fortran_order flag, and the stored
  width of the largest label that survives; when nothing survives it is the stream of an all-zero volume.

  On the device the decoder runs up to its run tables; the keep bit of every pixel is worked out from the runs
  (ckl_erode.hpp), the encoder's planes are the XOR of that bit plane with itself shifted by one pixel and by one
  row, and the encoder's crack and label stages follow as for recompress (ckl_erode).  Signed streams raise
  TypeError, a bad connectivity or a negative order ValueError; a damaged slice raises what decompress raises for
  it; the stream of an empty volume comes back as recompress returns it, without a device."""
  _checked_connectivity("erode", connectivity)
  flags = 0 if erode_border else _lib.CKL_ERODE_KEEP_BORDER
  return _reencode("erode", "ckl_erode", binary, (int(connectivity), flags), markov_model_order, device)


def dilate(
  binary: bytes, connectivity: int = 26, markov_model_order: Optional[int] = None, device: int = 0,
) -> bytes:
  """compress(dilated, markov_model_order=m), byte for byte, where dilated is the stream's volume with every label
  grown by one voxel into the background (the reference has none), without the voxels.  One iteration per call.

  This project's definition: a voxel whose label is not 0 keeps it.  For a voxel with label 0 the counted
  neighbours are the 6, 18 or 26 offsets of erode()'s structuring element, (dx, dy, dz) in {-1, 0, 1}^3 with
  0 < |dx| + |dy| + |dz| <= 1, 2, 3, that lie inside the volume and carry a label other than 0.  If there are none
  the voxel stays 0.  Otherwise it takes the label that occurs most often among them, and among labels tied for
  most often the smallest, compared as unsigned 64-bit values.  Neighbours outside the volume do not exist, so
  there is no border flag.  Equality is by label: the false boundaries that remap, mask, dust or fill_holes leave
  change nothing.

  This is meant to be fastmorph's multilabel dilate(background_only=True).  That package was not at hand: the tie
  rule is this project's own and was not checked against fastmorph.

  m is the input's order unless markov_model_order is given.  The output has FLAT labels, format version 1,
  whatever the input had (FLAT, pins, version 0), and the input's data width and fortran_order flag, exactly as
  erode() documents its own result.  A stream in which nothing is gained (no label 0, or no 0 next to a label)
  comes back as recompress(binary) returns it.

  On the device the decoder runs up to its run tables; a "label != 0" bit plane of every row gives the gained
  pixels, each gained pixel's label is the mode of its neighbours' labels read through the runs, the encoder's
  planes are written from the runs and the gained labels together, and the encoder's crack and label stages follow
  as for recompress (ckl_dilate.hpp).  Signed streams raise TypeError, a bad connectivity or a negative order
  ValueError; a damaged slice raises what decompress raises for it; the stream of an empty volume comes back as
  recompress returns it, without a device.

  Not done: background_only=False (every voxel takes its neighbourhood's mode), grey-level dilation, several
  iterations in one call, fused opening or closing, z-ranges, a sharded version, dilate in the stream-kind test
  matrix."""
  _checked_connectivity("dilate", connectivity)
  return _reencode("dilate", "ckl_dilate", binary, (int(connectivity), 0), markov_model_order, device)


def downsample(
  binary: bytes, factor: Tuple[int, int, int] = (2, 2, 1), num_mips: int = 1,
  markov_model_order: Optional[int] = None, device: int = 0,
) -> List[bytes]:
  """A resolution pyramid of the stream: a list of num_mips streams, entry 0 the downsample of binary, entry k the
  downsample of entry k - 1.  Each equals compress(pooled, markov_model_order=m), byte for byte, where pooled is the
  level before it pooled by `factor`, in the input's dtype, without the voxels.  Level k has shape ceil(s / f) per
  axis of level k - 1; an axis of size 0 or 1 keeps its size.

  factor is (2, 2, 1) or (2, 2, 2).  Label 0 is an ordinary label in both rules.

  (2, 2, 1) is the reference's rule (src/operations.hpp:1254-1293): with a, b, c, d at (x, y), (x + 1, y),
  (x, y + 1), (x + 1, y + 1): a == b -> a, a == c -> a, b == c -> b, else d.  Where the block is cut by an odd sx or
  sy, the voxel at its origin is copied.  So decompress(downsample(b)[0]) equals decompress(mode_pooling_2x2x1(b))
  wherever the latter does not raise (it raises when its pooled slices pick different crack formats; this does not).

  (2, 2, 2) takes the label that occurs most often among the block's voxels that exist: a block holds 8 voxels, or
  4, 2 or 1 at odd ends.  Ties go to the smallest label, compared as unsigned 64-bit values: dilate()'s tie rule,
  which does not depend on memory order.  At an odd sz the last output slice pools 2 x 2 x 1 blocks by this rule,
  not by the reference's.

  m is the input's order unless markov_model_order is given.  Every level has FLAT labels, format version 1,
  whatever the input had (FLAT, pins, version 0), the input's data width and fortran_order flag, and the crack format
  the pooled volume itself selects.

  The levels are chained on the host, one device call each (ckl_downsample), with the stream crossing the host
  between them; fusing them is not done.  On the device the decoder runs up to its run tables; no dense label volume
  exists, neither the input's nor the pooled one: an output row can change its label only where one of the 2 * fz
  input rows under it has a break, the rule is evaluated there with one label fetch per input run, the encoder's
  planes are written from those pooled runs, and the encoder's crack and label stages follow for the pooled shape
  (ckl_downsample.hpp).  Signed streams raise TypeError, another factor, num_mips < 1 or a negative order
  ValueError; a damaged slice raises what decompress raises for it; a stream without voxels becomes the header-only
  stream of the pooled shape, without a device.

  Not done: other factors, a sparse mode that prefers non-zero labels, averaging."""
  try:
    f = tuple(int(v) for v in factor)
  except (TypeError, ValueError):
    f = ()
  if f not in ((2, 2, 1), (2, 2, 2)):
    raise ValueError(f"downsample: factor must be (2, 2, 1) or (2, 2, 2). Got: {factor}")
  if int(num_mips) < 1:
    raise ValueError(f"downsample: num_mips must be at least 1. Got: {num_mips}")
  levels = []
  for _ in range(int(num_mips)):
    binary = _reencode("downsample", "ckl_downsample", binary, (*f, 0), markov_model_order, device)
    levels.append(binary)
  return levels


def _combine(what: str, rule: int, binary: bytes, other: bytes, markov_model_order: Optional[int], device: int) -> bytes:
  """The call that overlay and mask_by share (ckl_combine), after the refusals the host decides."""
  from .codec import _raise
  a, b = bytes(binary), bytes(other)
  ha, hb = header(a), header(b)
  if (ha.sx, ha.sy, ha.sz) != (hb.sx, hb.sy, hb.sz):
    raise ValueError(
      f"{what}: the volumes differ in shape: {ha.sx} x {ha.sy} x {ha.sz} and {hb.sx} x {hb.sy} x {hb.sz}")
  if ha.signed or hb.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  _checked_order(what, markov_model_order)
  order = -1 if markov_model_order is None else int(markov_model_order)
  out, n = C.c_void_p(), C.c_uint64()
  rc = _lib.lib().ckl_combine(a, len(a), b, len(b), int(rule), 0, order, int(device), C.byref(out), C.byref(n))
  if rc != _lib.CKL_OK:
    _raise(rc)
  return _take(out, n)


def overlay(binary: bytes, other: bytes, markov_model_order: Optional[int] = None, device: int = 0) -> bytes:
  """compress(V, markov_model_order=m), byte for byte, where V = B where B != 0, else A, with A = decompress(binary)
  and B = decompress(other): the objects of `other` put on top of `binary`, without the voxels of either (the
  reference has none).  overlay(other, binary) is the other direction: A's background filled from B.

  The two streams must agree in shape (ValueError otherwise) and may differ in everything else: dtype, FLAT or pin
  labels, format version, crack format, markov order, memory order, unsorted or merged label lists.  Label 0 of
  `other` is the only special value.  Equality is by label: the false boundaries that remap, mask, dust or fill_holes
  leave in either stream change nothing.

  V has the unsigned dtype whose width is the larger of the two streams' data widths.  m is binary's order unless
  markov_model_order is given, and the fortran_order flag is binary's.  The output has FLAT labels, format version 1,
  whatever the inputs had, the crack format the combined volume itself selects, and the stored width of the largest
  label that survives; when nothing survives it is the stream of an all-zero volume, as erode() documents.

  On the device both decoders run up to their run tables, side by side; no dense label volume exists: a row can
  change its combined label only where one of the two streams has a break, the rule is evaluated there with one
  label fetch per run of either stream, the encoder's planes are written from those labelled cuts by downsample()'s
  own kernel, and the encoder's crack and label stages follow as for recompress (ckl_combine.hpp).  Signed streams
  raise TypeError, a negative order ValueError; a damaged slice raises what decompress raises for that stream,
  binary's first; streams without voxels come back as the header-only stream of their shape, without a device, as
  recompress returns it.

  Not done: where(cond, a, b) over three streams, a joint (product) segmentation with fresh ids, a fill value other
  than 0, z-ranges, a sharded version, a place in the thread-job and stream-kind matrices of the existing test
  files."""
  return _combine("overlay", _lib.CKL_COMBINE_OVERLAY, binary, other, markov_model_order, device)


def mask_by(binary: bytes, other: bytes, invert: bool = False, markov_model_order: Optional[int] = None, device: int = 0) -> bytes:
  """compress(V, markov_model_order=m), byte for byte, where V = A where (B != 0) != invert, else 0, with
  A = decompress(binary) and B = decompress(other): `binary` cut down to the mask that `other` is (invert: to what
  lies outside it), without the voxels of either (the reference has none).

  The two streams must agree in shape (ValueError otherwise) and may differ in everything else, as overlay()
  documents.  other's labels never appear in the result, only whether they are 0.  Equality is by label: false
  boundaries in either stream change nothing.

  The data width, the fortran_order flag and the default m are binary's.  The output has FLAT labels, format version
  1, whatever the inputs had, the crack format the combined volume itself selects, and the stored width of the
  largest label that survives; when nothing survives it is the stream of an all-zero volume, as erode() documents.

  The device side, the refusals, damaged slices and streams without voxels are overlay()'s (ckl_combine.hpp).

  Not done: where(cond, a, b) over three streams, a joint (product) segmentation with fresh ids, a fill value other
  than 0, z-ranges, a sharded version, a place in the thread-job and stream-kind matrices of the existing test
  files."""
  rule = _lib.CKL_COMBINE_DROP_WHERE if invert else _lib.CKL_COMBINE_KEEP_WHERE
  return _combine("mask_by", rule, binary, other, markov_model_order, device)


def opening(
  binary: bytes, connectivity: int = 26, erode_border: bool = True,
  markov_model_order: Optional[int] = None, device: int = 0,
) -> bytes:
  """dilate(erode(binary)): objects thinner than the structuring element go, the others get their rim back where
  the background allows it.  erode() and dilate() document the two steps; connectivity and erode_border are
  theirs.  The first step keeps the stream's markov order, the last takes markov_model_order.  These are two device
  calls with the stream crossing the host between them; fusing them is not done."""
  _checked_order("opening", markov_model_order)
  peeled = erode(binary, connectivity=connectivity, erode_border=erode_border, device=device)
  return dilate(peeled, connectivity=connectivity, markov_model_order=markov_model_order, device=device)


def closing(
  binary: bytes, connectivity: int = 26, erode_border: bool = True,
  markov_model_order: Optional[int] = None, device: int = 0,
) -> bytes:
  """erode(dilate(binary)): pits and gaps narrower than the structuring element are filled with the labels around
  them.  dilate() and erode() document the two steps; connectivity and erode_border are theirs.  The first step
  keeps the stream's markov order, the last takes markov_model_order.  These are two device calls with the stream
  crossing the host between them; fusing them is not done."""
  _checked_order("closing", markov_model_order)
  grown = dilate(binary, connectivity=connectivity, device=device)
  return erode(grown, connectivity=connectivity, erode_border=erode_border, markov_model_order=markov_model_order, device=device)
