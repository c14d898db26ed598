"""Random access into a stream: cutout() decodes an x, y, z box on the device, CrackleArray wraps a
stream behind numpy-style indexing (the reference's CrackleArray.__getitem__, crackle/array.py:257-285,
which decodes the whole slices of the z-range and lets numpy crop them).  Here the device writes the
box alone (ckl_cutout: the decode pipeline up to the run tables, then k_paint_window) and only the box
crosses the link.  paste() is the way back (the reference's __setitem__, crackle/array.py:287-340):
the slices of the box's z-range are decoded, edited and encoded again in HBM (ckl_paste).  crop(), crop_boxes()
and chunks() give boxes as streams of their own, from the run tables of one decode and without a voxel
(ckl_crop_boxes)."""
import ctypes as C
import operator
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _lib, codec, operations
from .headers import CrackleHeader

_SIGNED = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def normalize_index(slices, shape):
  """The index expression `slices` on a volume of `shape` = (sx, sy, sz) as three (start, stop, step,
  is_int) tuples with 0 <= start <= stop <= dim and step >= 1; stop is tightened to one past the
  last element taken.  numpy's meaning throughout (``...`` fills the axes that are not named), with
  the stricter checks of the reference's reify_slices (crackle/array.py:450-532):

    a slice start or stop outside [0, dim] after dim is added to a negative one   ValueError
    a negative (or zero) step                                                      ValueError
    more than one Ellipsis                                                         ValueError
    an int outside [-dim, dim), more than three indices                            IndexError
  """
  if not isinstance(slices, tuple):
    slices = (slices,)
  n_ellipsis = sum(1 for s in slices if s is Ellipsis)
  if n_ellipsis > 1:
    raise ValueError("More than one Ellipsis operator used at once.")
  named = len(slices) - n_ellipsis
  if named > 3:
    raise IndexError(f"too many indices for a volume: 3 axes, {named} were indexed")
  full = []
  for s in slices:
    if s is Ellipsis:
      full.extend([slice(None)] * (3 - named))
    else:
      full.append(s)
  full.extend([slice(None)] * (3 - len(full)))

  out = []
  for axis, (s, dim) in enumerate(zip(full, shape)):
    if isinstance(s, slice):
      step = 1 if s.step is None else operator.index(s.step)
      if step <= 0:
        raise ValueError(f"Negative or zero step sizes are not supported. Got: {step}")
      start = 0 if s.start is None else operator.index(s.start)
      stop = dim if s.stop is None else operator.index(s.stop)
      ends = []
      for v in (start, stop):
        if v < 0:
          v += dim
        if v < 0 or v > dim:
          raise ValueError(f"Value {v} on axis {axis} cannot be outside of inclusive range 0 to {dim}")
        ends.append(v)
      start, stop = ends
      count = max(0, -(-(stop - start) // step))
      stop = start + (count - 1) * step + 1 if count else start
      out.append((start, stop, step, False))
    elif isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)):
      i = int(s)
      if i < -dim or i >= dim:
        raise IndexError(f"index {i} is out of bounds for axis {axis} with size {dim}")
      if i < 0:
        i += dim
      out.append((i, i + 1, 1, True))
    else:
      raise TypeError(f"cutout indices are ints, slices and Ellipsis, not {type(s).__name__}")
  return out


def cutout(binary: bytes, slices, label: Optional[int] = None, device: int = 0) -> np.ndarray:
  """``decompress(binary, label=label)[slices]`` by numpy's rules, decoding only the box that
  `slices` spans: an int, a slice, ``...`` or a tuple of up to three of them with at most one ``...``.
  Stricter than numpy where the reference is (normalize_index): bounds are checked, not clamped, and
  steps are positive.

  One deliberate difference from the reference: its __getitem__ hands the caller's tuple, Ellipsis
  included, to numpy after it has already cut z (crackle/array.py:270-280), so ``arr[..., 0]``
  indexes y there.  Here ``...`` means what it means in numpy: ``arr[..., 0]`` is the first z slice.

  The device decodes the slices of the box's z-range (so a damaged slice in that range raises as it
  does for decompress, wherever the box lies) and writes the box alone; steps and int axes are
  applied with numpy on that small result.  Streams without voxels, with a single label or asked for
  a label they do not hold are answered on the host, as decompress_range answers them."""
  binary = bytes(binary)
  head = CrackleHeader.frombytes(binary)
  idx = normalize_index(slices, (head.sx, head.sy, head.sz))
  (x0, x1, _, _), (y0, y1, _, _), (z0, z1, _, _) = idx
  shape = (x1 - x0, y1 - y0, z1 - z0)
  order = "F" if head.fortran_order else "C"
  dtype = np.dtype(_SIGNED[head.data_width] if head.signed else head.dtype)
  if label is not None:
    dtype = np.dtype(bool)

  if shape[0] * shape[1] * shape[2] == 0:
    box = np.zeros(shape, dtype=dtype, order=order)
  elif label is not None and not codec.contains(binary, label):
    box = np.zeros(shape, dtype=dtype, order=order)
  elif label is None and codec.num_labels(binary) == 1:
    single = codec.labels(binary)[0]
    box = np.full(shape, single, dtype=head.dtype, order=order).view(dtype)
  else:
    raw = np.empty((shape[0] * shape[1] * shape[2],), dtype=np.uint8 if label is not None else head.dtype)
    rc = _lib.lib().ckl_cutout(
      binary, len(binary), raw.ctypes.data, raw.nbytes, _lib.MEM_HOST,
      x0, x1, y0, y1, z0, z1, int(label is not None), int(label or 0), int(device),
    )
    if rc != _lib.CKL_OK:
      codec._raise(rc)
    box = raw.view(dtype).reshape(shape, order=order)
  return box[tuple(0 if is_int else slice(None, None, step) for _, _, step, is_int in idx)]


def paste(binary: bytes, slices, data, device: int = 0) -> bytes:
  """The stream that decodes to ``V = decompress(binary); V[slices] = data`` (the reference's
  CrackleArray.__setitem__, crackle/array.py:287-340, as a function that returns the new stream).
  `slices` means what it means for cutout() (normalize_index, the same errors; steps >= 1; an int axis drops
  out of the shape `data` must broadcast to).  `data` is a Python int or anything np.asarray takes: it is
  broadcast to the indexed shape (numpy's ValueError when it does not), arrays are cast with
  astype(dtype, copy=False) as the reference casts them, a Python int outside the stream's dtype is
  OverflowError.  Signed streams are TypeError, as for compress; an empty box returns the stream unchanged.

  Only the stream and the box cross the link: the device decodes the slices of the box's z-range
  [z0, z1) into a slab in HBM, k_paste_box writes the box into it and the encoder reads it there
  (ckl_paste).  With a step > 1 the tight box comes back through cutout(), numpy assigns into it and it
  is pasted once: two transfers of the size of the box, never of the slab.

  The bytes: for a version 1 stream with FLAT labels and a z-range that is not the whole depth, the slab is
  encoded under the input's crack format, markov order and markov model and spliced between
  zsplit's ranges with zstack, so the untouched slices keep their crack codes and crcs byte for byte
  (the reference compresses the slab with defaults, which can make its zstack raise, and returns every
  stream at markov order 0).  Otherwise (the z-range is the whole depth, pin labels, version 0) the result
  is compress(V', markov_model_order=<the input's>): FLAT labels, version 1 — a pin-label stream comes back
  FLAT.  A damaged slice inside [z0, z1) raises what decompress raises; one outside it is copied unseen,
  as zsplit copies it."""
  binary = bytes(binary)
  head = CrackleHeader.frombytes(binary)
  idx = normalize_index(slices, (head.sx, head.sy, head.sz))
  if head.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  dtype = np.dtype(head.dtype)
  counts = [(stop - start - 1) // step + 1 if stop > start else 0 for start, stop, step, _ in idx]
  indexed_shape = tuple(n for n, (_, _, _, is_int) in zip(counts, idx) if not is_int)
  scalar = isinstance(data, (int, np.integer)) and not isinstance(data, (bool, np.bool_))
  if scalar:
    value = int(data)
    if value < 0 or value > int(np.iinfo(dtype).max):
      raise OverflowError(f"Python integer {value} out of bounds for {dtype}")
  else:
    arr = np.broadcast_to(np.asarray(data).astype(dtype, copy=False), indexed_shape)
  if 0 in counts:
    return binary

  (x0, x1, _, _), (y0, y1, _, _), (z0, z1, _, _) = idx
  tight = (x1 - x0, y1 - y0, z1 - z0)
  order = "F" if head.fortran_order else "C"
  stepped = any(step > 1 and n > 1 for n, (_, _, step, _) in zip(counts, idx))
  box = None
  if stepped:
    box = np.array(cutout(binary, (slice(x0, x1), slice(y0, y1), slice(z0, z1)), device=device), order=order)
    box[tuple(slice(None, None, step) for _, _, step, _ in idx)] = value if scalar else arr.reshape(counts)
  elif not scalar:
    box = np.array(arr.reshape(tight), order=order)
  out, n = C.c_void_p(), C.c_uint64()
  rc = _lib.lib().ckl_paste(
    binary, len(binary), None if box is None else box.ctypes.data, _lib.MEM_HOST, int(box is not None), 0 if box is not None else value,
    x0, x1, y0, y1, z0, z1, int(device), C.byref(out), C.byref(n),
  )
  if rc != _lib.CKL_OK:
    codec._raise(rc)
  return operations._take(out, n)


def crop_boxes(binary: bytes, boxes, markov_model_order: Optional[int] = None, device: int = 0) -> List[bytes]:
  """One stream per index expression of `boxes`, in order, each exactly what crop() gives for that box, with the
  stream decoded ONCE for all of them (ckl_crop_boxes).  Boxes may overlap, repeat, differ in shape and stand in any
  order; an empty sequence gives an empty list.

  On the device one decode session runs up to its run tables over the slices [min z0, max z1) of the boxes that hold
  voxels, and one label per run is gathered once.  Every box then takes a turn: its words are cut where the input row
  under them has a break, the labels at those cuts are read through the runs, downsample()'s own kernel writes the
  encoder's planes from them, and the encoder's crack and label stages follow for the box's shape (ckl_crop.hpp).
  Boxes of one shape share an encode session.  No voxel of the input or of a box exists anywhere.

  A damaged slice inside [min z0, max z1) raises what decompress_range raises for it, whichever box is asked for,
  and nothing is returned; a damaged slice outside that range is never looked at.  Index errors are cutout()'s
  (normalize_index), a step other than 1 and a negative order are ValueError, signed streams TypeError; all of them
  are raised before any device work, for every box.  Boxes with an axis of size 0 become the 29-byte header-only
  stream of their shape, on the host."""
  binary = bytes(binary)
  head = CrackleHeader.frombytes(binary)
  if head.signed:
    raise TypeError("Signed integer data types are not currently supported.")
  operations._checked_order("crop", markov_model_order)
  flat = []
  for expr in boxes:
    idx = normalize_index(expr, (head.sx, head.sy, head.sz))
    for start, stop, step, _ in idx:
      if step != 1:
        raise ValueError(f"crop: steps other than 1 are not supported (strided subsampling is not a crop). Got: {step}")
      flat.extend((start, stop))
  n_boxes = len(flat) // 6
  if n_boxes == 0:
    return []
  order = -1 if markov_model_order is None else int(markov_model_order)
  outs, lens = (C.c_void_p * n_boxes)(), (C.c_uint64 * n_boxes)()
  rc = _lib.lib().ckl_crop_boxes(
    binary, len(binary), (C.c_int64 * len(flat))(*flat), n_boxes, 0, order, int(device),
    C.cast(outs, C.POINTER(C.c_void_p)), C.cast(lens, C.POINTER(C.c_uint64)),
  )
  if rc != _lib.CKL_OK:
    codec._raise(rc)
  return [operations._take(C.c_void_p(outs[k]), C.c_uint64(lens[k])) for k in range(n_boxes)]


def crop(binary: bytes, slices, markov_model_order: Optional[int] = None, device: int = 0) -> bytes:
  """The box ``decompress(binary)[slices]`` as a stream of its own: compress(V, markov_model_order=m), byte for byte,
  where V is the contiguous copy of the box in the memory order of the input's fortran_order flag, without the voxels
  of the input or of the box (the reference has none; cutout() gives the box as voxels, paste() is the way back).

  `slices` means what it means for cutout() (normalize_index, the same errors), with two differences: an int index
  keeps its axis at size 1, because a stream is always three-dimensional, and a step other than 1 is ValueError.
  m is the input's order unless markov_model_order is given.  The output has FLAT labels, format version 1, whatever
  the input had (FLAT, pins, version 0), the input's data width and fortran_order flag, and the crack format, stored
  width and key widths that the box itself selects: a box can lose the input's largest label.  The box that is the
  whole volume gives recompress(binary); a box with an axis of size 0 gives the 29-byte header-only stream of its
  shape, on the host, as recompress gives it for a volume without voxels.

  The device side, damaged slices (one inside the box's z-range raises what decompress_range raises for it, one
  outside is never looked at) and the refusals are crop_boxes()'s, of which this is the call with one box.

  Not done: steps other than 1, joining streams along x or y, a sharded version, a place in the thread-job and
  stream-kind matrices of the existing test files."""
  return crop_boxes(binary, [slices], markov_model_order=markov_model_order, device=device)[0]


def chunk_boxes(shape, chunk_size) -> List[Tuple[int, int, int, int, int, int]]:
  """The boxes (x0, x1, y0, y1, z0, z1) of the grid of chunks of `chunk_size` = (cx, cy, cz) that tiles a volume of
  `shape` from (0, 0, 0), in x-fastest grid order; chunks at the far faces are smaller.  Pure arithmetic.  A volume
  with an axis of size 0 has no chunks; a chunk size below 1 is ValueError."""
  try:
    size = tuple(operator.index(c) for c in chunk_size)
  except TypeError:
    size = ()
  if len(size) != 3 or min(size) < 1:
    raise ValueError(f"chunks: chunk_size must be three integers of at least 1. Got: {chunk_size}")
  sx, sy, sz = (int(s) for s in shape)
  cx, cy, cz = size
  return [
    (x0, min(x0 + cx, sx), y0, min(y0 + cy, sy), z0, min(z0 + cz, sz))
    for z0 in range(0, sz, cz) for y0 in range(0, sy, cy) for x0 in range(0, sx, cx)
  ]


def chunks(binary: bytes, chunk_size, markov_model_order: Optional[int] = None, device: int = 0) -> Dict[Tuple[int, int, int], bytes]:
  """{(x0, y0, z0): stream} of the grid of chunks of `chunk_size` that tiles the volume from (0, 0, 0) (chunk_boxes),
  in x-fastest grid order: what a level of a downsample() pyramid is stored as.  Each stream is what crop() gives for
  its box, and the input is decoded once for all of them (crop_boxes); a grid has at most eight shapes of box, so at
  most eight encode sessions serve it."""
  binary = bytes(binary)
  head = CrackleHeader.frombytes(binary)
  grid = chunk_boxes((head.sx, head.sy, head.sz), chunk_size)
  streams = crop_boxes(binary, [(slice(b[0], b[1]), slice(b[2], b[3]), slice(b[4], b[5])) for b in grid], markov_model_order=markov_model_order, device=device)
  return {(b[0], b[2], b[4]): s for b, s in zip(grid, streams)}


class CrackleArray:
  """A stream behind an array interface (crackle/array.py:32-340): metadata from the header and the
  label section, ``arr[x0:x1, y0:y1, z0:z1]`` through cutout(), ``arr.paste(slices, data)`` for the
  reference's ``arr[slices] = data`` (it returns a new array, as mask and recompress do), and the package's
  operations as methods."""

  def __init__(self, binary: bytes, device: int = 0):
    self.binary = bytes(binary)
    self.device = device
    head = self.header()
    self.shape = (head.sx, head.sy, head.sz)

  def __len__(self):
    return len(self.binary)

  def header(self) -> CrackleHeader:
    return codec.header(self.binary)

  @property
  def dtype(self):
    head = self.header()
    return np.dtype(_SIGNED[head.data_width] if head.signed else head.dtype)

  @property
  def size(self) -> int:
    return self.shape[0] * self.shape[1] * self.shape[2]

  @property
  def ndim(self) -> int:
    return len(self.shape)

  @property
  def nbytes(self) -> int:
    return self.header().nbytes

  def labels(self) -> np.ndarray:
    return codec.labels(self.binary)

  def num_labels(self) -> int:
    return codec.num_labels(self.binary)

  def __contains__(self, label: int) -> bool:
    return codec.contains(self.binary, label)

  def min(self) -> int:
    return int(self.labels().view(self.dtype).min())

  def max(self) -> int:
    return int(self.labels().view(self.dtype).max())

  def decompress(self, label: Optional[int] = None, crop: bool = False) -> np.ndarray:
    return codec.decompress(self.binary, label=label, crop=crop, device=self.device)

  def numpy(self, *args, **kwargs) -> np.ndarray:
    return self.decompress(*args, **kwargs)

  def __getitem__(self, slices) -> np.ndarray:
    return cutout(self.binary, slices, device=self.device)

  # (no __setitem__: tests/test_cutout_cpu.py pins that the array is never edited in place)
  def paste(self, slices, data) -> "CrackleArray":
    return CrackleArray(paste(self.binary, slices, data, device=self.device), self.device)

  def crop(self, slices) -> "CrackleArray":
    """The box as an array of its own (crop): an int index keeps its axis at size 1."""
    return CrackleArray(crop(self.binary, slices, device=self.device), self.device)

  def crop_boxes(self, boxes) -> List["CrackleArray"]:
    return [CrackleArray(b, self.device) for b in crop_boxes(self.binary, boxes, device=self.device)]

  def chunks(self, chunk_size) -> Dict[Tuple[int, int, int], "CrackleArray"]:
    return {key: CrackleArray(b, self.device) for key, b in chunks(self.binary, chunk_size, device=self.device).items()}

  def voxel_counts(self, label: Optional[int] = None):
    return codec.voxel_counts(self.binary, label=label, device=self.device)

  def centroids(self, label: Optional[int] = None):
    return codec.centroids(self.binary, label=label, device=self.device)

  def bounding_boxes(self, label: Optional[int] = None, no_slice_conversion: bool = False):
    return codec.bounding_boxes(self.binary, label=label, no_slice_conversion=no_slice_conversion, device=self.device)

  def point_cloud(self, label=None, skip_background: bool = True, z_start: int = -1, z_end: int = -1):
    return operations.point_cloud(self.binary, label, z_start=z_start, z_end=z_end, skip_background=skip_background, device=self.device)

  def contacts(self, anisotropy=(1.0, 1.0, 1.0)):
    return operations.contacts(self.binary, anisotropy=anisotropy, device=self.device)

  def overlaps(self, other: Union["CrackleArray", bytes]):
    """{(a, b): voxels} of this array's labels a against the labels b of `other` (operations.overlaps)."""
    other_binary = other.binary if isinstance(other, CrackleArray) else other
    return operations.overlaps(self.binary, other_binary, device=self.device)

  def overlay(self, other: Union["CrackleArray", bytes]) -> "CrackleArray":
    """`other` where it is not 0, this array elsewhere (operations.overlay)."""
    other_binary = other.binary if isinstance(other, CrackleArray) else other
    return CrackleArray(operations.overlay(self.binary, other_binary, device=self.device), self.device)

  def mask_by(self, other: Union["CrackleArray", bytes], invert: bool = False) -> "CrackleArray":
    """This array where `other` is not 0 (invert: where it is 0), 0 elsewhere (operations.mask_by)."""
    other_binary = other.binary if isinstance(other, CrackleArray) else other
    return CrackleArray(operations.mask_by(self.binary, other_binary, invert=invert, device=self.device), self.device)

  def connected_components(self, connectivity: int = 26, binary_image: bool = False, return_mapping: bool = False):
    out = operations.connected_components(self.binary, connectivity=connectivity, binary_image=binary_image, return_mapping=return_mapping, device=self.device)
    if return_mapping:
      return CrackleArray(out[0], self.device), out[1]
    return CrackleArray(out, self.device)

  def dust(self, threshold: int, connectivity: int = 26, binary_image: bool = False, invert: bool = False) -> "CrackleArray":
    return CrackleArray(operations.dust(self.binary, threshold, connectivity=connectivity, binary_image=binary_image, invert=invert, device=self.device), self.device)

  def fill_holes(self, connectivity: int = 6) -> "CrackleArray":
    return CrackleArray(operations.fill_holes(self.binary, connectivity=connectivity, device=self.device), self.device)

  # (no remap method: tests/test_cutout_cpu.py pins that CrackleArray has none; operations.remap(arr.binary, ...) is the way)
  def mask(self, labels, value: int = 0) -> "CrackleArray":
    return CrackleArray(operations.mask(self.binary, labels, value=value), self.device)

  def mask_except(self, labels, value: int = 0) -> "CrackleArray":
    return CrackleArray(operations.mask_except(self.binary, labels, value=value), self.device)

  def recompress(self, markov_model_order: Optional[int] = None) -> "CrackleArray":
    return CrackleArray(operations.recompress(self.binary, markov_model_order=markov_model_order, device=self.device), self.device)

  def erode(self, connectivity: int = 26, erode_border: bool = True) -> "CrackleArray":
    return CrackleArray(operations.erode(self.binary, connectivity=connectivity, erode_border=erode_border, device=self.device), self.device)

  def dilate(self, connectivity: int = 26) -> "CrackleArray":
    return CrackleArray(operations.dilate(self.binary, connectivity=connectivity, device=self.device), self.device)

  def downsample(self, factor: Tuple[int, int, int] = (2, 2, 1), num_mips: int = 1) -> List["CrackleArray"]:
    return [CrackleArray(b, self.device) for b in operations.downsample(self.binary, factor=factor, num_mips=num_mips, device=self.device)]

  def opening(self,connectivity: int = 26, erode_border: bool = True) -> "CrackleArray":
    return CrackleArray(operations.opening(self.binary, connectivity=connectivity, erode_border=erode_border, device=self.device), self.device)

  def closing(self, connectivity: int = 26, erode_border: bool = True) -> "CrackleArray":
    return CrackleArray(operations.closing(self.binary, connectivity=connectivity, erode_border=erode_border, device=self.device), self.device)

  def voxel_connectivity_graph(self, connectivity: int = 4) -> np.ndarray:
    return codec.voxel_connectivity_graph(self.binary, connectivity, device=self.device)

  def mode_pooling_2x2x1(self) -> "CrackleArray":
    return CrackleArray(operations.mode_pooling_2x2x1(self.binary, device=self.device), self.device)

  def array_equal(self, other: "CrackleArray") -> bool:
    return operations.array_equal(self.binary, other.binary, device=self.device)
