"""Volumes for the label edits (crackle_amd.remap / mask / mask_except) and for recompress (ckl_recompress:
k_label_planes_from_runs and the encoder behind it).  Plain numpy on top of crackle_amd.synth; shared by the CPU test
that pins what every volume is (tests/test_recompress_volumes_cpu.py) and the GPU tests that run the kernels on them
(tests/test_gpu_recompress.py).

A merged case is a volume and a divisor: the stream of the volume is remapped v -> v // divisor, which merges labels
and leaves the cracks between their components in place; recompress must give compress(volume // divisor).  What the
cases are about is the crack format, which the encoder takes from lib::pixel_pairs < voxels / 2 (src/crackle.hpp:48-55,
src/lib.hpp:249-256): equal neighbours in x-fastest order over the whole volume, so the last pixel of a row counts
against the first of the next row and the last of a slice against the first of the next slice."""
import numpy as np

from crackle_amd import synth


def voronoi(shape, dtype, seed, cell=(16, 16, 4), **kw):
  return synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=seed, cell=cell, **kw))


def noise(shape, dtype, seed, high):
  return synth.random_labels(shape, dtype, seed=seed, high=high)


def linear_pairs(arr):
  """lib::pixel_pairs: equal neighbours of the x-fastest sequence, wrap-arounds included."""
  f = np.asarray(arr).reshape(-1, order="F")
  return int(np.count_nonzero(f[1:] == f[:-1]))


def interior_x_pairs(arr):
  """Equal neighbours inside the rows alone: what a count without the wrap-arounds would give."""
  arr = np.asarray(arr)
  return int(np.count_nonzero(arr[1:, :, :] == arr[:-1, :, :]))


def permissible(arr):
  """The crack format compress picks: PERMISSIBLE when pixel_pairs < voxels / 2."""
  return linear_pairs(arr) < np.asarray(arr).size // 2


def floordiv_mapping(arr, divisor):
  return {int(v): int(v) // divisor for v in np.unique(arr)}


class Merged:
  def __init__(self, id, make, divisor):
    self.id, self._make, self.divisor = id, make, divisor

  def volume(self):
    return self._make()

  def merged(self):
    return np.asfortranarray(self.volume() // self.volume().dtype.type(self.divisor))

  def __repr__(self):
    return self.id


VORONOI = Merged("voronoi-72x64x6-u8", lambda: voronoi((72, 64, 6), np.uint8, 8, cell=(8, 8, 2)), 2)
NOISE_FLIPS = Merged("noise-130x70x4-seed21", lambda: noise((130, 70, 4), np.uint8, 21, 4), 2)
NOISE_STAYS = Merged("noise-130x70x4-seed22", lambda: noise((130, 70, 4), np.uint8, 22, 4), 2)
NOISE_BY_ONE = Merged("noise-97x61x7-seed25", lambda: noise((97, 61, 7), np.uint8, 25, 4), 2)
NOISE_WIDTH = Merged("noise-130x70x4-u16-high300", lambda: noise((130, 70, 4), np.uint16, 21, 300), 150)
MERGED = [VORONOI, NOISE_FLIPS, NOISE_STAYS, NOISE_BY_ONE, NOISE_WIDTH]


def as_signed(binary):
  """The same stream with the header's signed flag set (and its crc8 redone): what compress refuses to write."""
  fmt = int.from_bytes(binary[5:7], "little") | (1 << 8)
  head = bytearray(binary[:28])
  head[5:7] = fmt.to_bytes(2, "little")
  crc = 0xFF
  for byte in head[5:28]:
    crc ^= byte
    for _ in range(8):
      crc = (crc >> 1) ^ 0xE7 if crc & 1 else crc >> 1
  return bytes(head) + bytes([crc]) + bytes(binary[29:])


def _crc8(data):
  crc = 0xFF
  for byte in data:
    crc ^= byte
    for _ in range(8):
      crc = (crc >> 1) ^ 0xE7 if crc & 1 else crc >> 1
  return crc


def permuted_stream(binary, fn=lambda v: (7 * v) % 41):
  """What the reference's remap writes for a flat stream (crackle/codec.py:747-776): the unique list rewritten v -> fn(v)
  in place, in whatever order that leaves it and with the duplicates it makes, bit 13 of the format field ("not
  sorted") set, the header's crc8 and the label crc32c redone.  The default is injective on 0 .. 40, keeps 0 and is
  not monotone."""
  import crackle_amd
  from crackle_amd import _lib, codec
  b = bytearray(binary)
  head = crackle_amd.header(bytes(b))
  assert head.format_version == 1 and head.label_format == 0
  n, off = codec._label_section(bytes(b), head)
  uniq = np.frombuffer(bytes(b), dtype=head.stored_dtype, offset=off, count=n)
  new = np.array([fn(int(v)) for v in uniq.tolist()], dtype=np.uint64)
  assert int(new.max()) <= np.iinfo(head.stored_dtype).max, "a new value does not fit the stored width"
  b[off:off + uniq.nbytes] = new.astype(head.stored_dtype).tobytes()
  b[5:7] = (int.from_bytes(b[5:7], "little") | (1 << 13)).to_bytes(2, "little")
  b[28] = _crc8(b[5:28])
  start = head.header_bytes + head.grid_index_bytes
  crc = _lib.lib().ckl_crc32c(bytes(b[start:start + head.num_label_bytes]), head.num_label_bytes)
  at = len(b) - (head.sz * 4 + 4)
  b[at:at + 4] = int(crc).to_bytes(4, "little")
  return bytes(b)


def floordiv_stream(binary, divisor=2):
  """What the reference's floordiv_scalar writes for a flat stream (as tests/test_gpu_connected_components.py builds
  its merged input): the unique list rewritten v // divisor in place, duplicates and all, the label crc fixed."""
  import crackle_amd
  from crackle_amd import _lib, codec
  b = bytearray(binary)
  head = crackle_amd.header(bytes(b))
  n, off = codec._label_section(bytes(b), head)
  uniq = np.frombuffer(bytes(b), dtype=head.stored_dtype, offset=off, count=n)
  b[off:off + uniq.nbytes] = (uniq // divisor).astype(head.stored_dtype).tobytes()
  start = head.header_bytes + head.grid_index_bytes
  crc = _lib.lib().ckl_crc32c(bytes(b[start:start + head.num_label_bytes]), head.num_label_bytes)
  at = len(b) - (head.sz * 4 + 4)
  b[at:at + 4] = int(crc).to_bytes(4, "little")
  return bytes(b)
