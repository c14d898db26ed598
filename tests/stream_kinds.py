"""Every kind of stream the library accepts or produces, and the volume each one decodes to.  Plain numpy on top of
tests/fill_holes_volumes.py, tests/dust_volumes.py, tests/paste_volumes.py and tests/recompress_volumes.py; shared by
the CPU test that pins what the kinds are (tests/test_stream_kinds_cpu.py) and the GPU test that sends every kind
through every operation (tests/test_gpu_stream_kinds.py).  No GPU at import.

A kind is a Kind record: the stream, the volume it must decode to (numpy on the base volume or one of the
restatements tests/*_numpy.py, never a decode by this library), and what the cells of the matrix need beside it:

  source    the checker's compress() of the base volume over the kind's slices: what overlaps(b, source) pairs the
            kind with and what structure_equal compares it with
  base      that base volume (so overlaps(b, source) is overlaps_numpy(expected, base))
  cracks    a volume with the 2D components of the kind's crack codes in every slice: what contacts counts in-plane
            faces between.  `base` for every kind that keeps its cracks, the expected volume for one that re-encodes,
            and for the pasted kind the one in the re-encoded slices, the other in the rest
  keeps     whether the kind's cracks are the source's (structure_equal(b, source))
  other     another segmentation of the same shape: the second argument of overlaps / array_equal and the source of
            pasted boxes

kinds_host needs the checker alone (its compress) and the host side of the library; kinds_device runs the device
editors."""
import functools

import numpy as np

import cc3d_numpy
import dust_numpy
import dust_volumes
import erode_numpy
import fill_holes_numpy
import fill_holes_volumes
import gen_golden
import paste_volumes
import recompress_volumes as rv

DUST = (100, 26)       # threshold, connectivity of the dusted kinds
FILL = 6
COMPONENTS = 26
ERODE = (6, False)     # connectivity, erode_border
PERMUTE = lambda v: (7 * v) % 41
PERMUTE_MERGE = lambda v: ((7 * v) % 41) // 2

HOST_KINDS = ["flat", "pins", "markov5", "c-order", "v0", "remapped", "floordiv", "permuted", "permuted-merged",
              "zsplit-mid", "zsplit-tail", "restacked"]
DEVICE_KINDS = ["dusted", "filled", "dusted-filled", "components", "pasted", "eroded", "recompressed"]
LARGE_KINDS = ["large-flat", "large-remapped", "large-dusted"]
UNSORTED = ("permuted", "permuted-merged", "zsplit-mid")


class Kind:
  def __init__(self, name, stream, expected, base, source, other, cracks=None, keeps=True, mapping=None):
    self.name, self.stream, self.expected, self.base, self.source, self.other = name, bytes(stream), expected, base, source, other
    self.cracks = base if cracks is None else cracks
    self.keeps = keeps
    self.mapping = mapping      # components: {component id: original label}
    for v in (expected, base, other):
      v.setflags(write=False)

  def __repr__(self):
    return self.name


# ---- base volumes ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def volume_a():
  vol = fill_holes_volumes.punched((97, 61, 7), "F")
  vol.setflags(write=False)
  return vol


@functools.lru_cache(maxsize=None)
def volume_a8():
  vol = np.asfortranarray(volume_a().astype(np.uint8))
  vol.setflags(write=False)
  return vol


@functools.lru_cache(maxsize=None)
def volume_b():
  vol = fill_holes_volumes.punched((96, 80, 6), "C")
  vol.setflags(write=False)
  return vol


@functools.lru_cache(maxsize=None)
def volume_large():
  """Noise of four labels: more than 2048 runs in every slice, several workgroups of the run kernels."""
  vol = dust_volumes.noise((130, 70, 4), 4)
  vol.setflags(write=False)
  return vol


def other_of(vol):
  """Another segmentation of vol's shape, dtype and memory order (paste_volumes.other, cast as paste() casts)."""
  order = "F" if vol.flags.f_contiguous else "C"
  out = paste_volumes.other(vol.shape, np.uint32, order).astype(vol.dtype, order=order)
  return out


def box_of(shape):
  """An odd-offset, odd-width box that is no whole plane; two inner slices where the volume has them."""
  sx, sy, sz = shape
  z = slice(1, 3) if sz >= 4 else slice(0, sz)
  box = (slice(3, 40), slice(5, sy - 6), z)
  assert box[0].start % 2 == 1 and (box[0].stop - box[0].start) % 2 == 1 and box[0].stop < sx and box[1].stop > box[1].start
  return box


def like(vol, arr):
  """arr in vol's memory order."""
  return np.asfortranarray(arr) if vol.flags.f_contiguous else np.ascontiguousarray(arr)


def runs_per_slice(vol):
  """Runs of equal labels along x, per slice: what the decoder's run kernels work on."""
  v = np.asarray(vol)
  return ((v[1:, :, :] != v[:-1, :, :]).sum(axis=(0, 1)) + v.shape[1]).tolist()


def false_boundaries(vol, divisor=2):
  """(along x, along y): in-plane faces between different labels that vol // divisor gives one label."""
  v = np.asarray(vol)
  m = v // v.dtype.type(divisor)
  return (int(((v[1:] != v[:-1]) & (m[1:] == m[:-1])).sum()), int(((v[:, 1:] != v[:, :-1]) & (m[:, 1:] == m[:, :-1])).sum()))


# ---- what the editors do, in numpy ------------------------------------------------------------------------------------

def np_remap(vol):
  return like(vol, vol // vol.dtype.type(2))


def np_dust(vol):
  return dust_numpy.dust(vol, DUST[0], DUST[1])[0]


def np_fill(vol):
  return fill_holes_numpy.fill_holes(vol, FILL).volume


def np_components(vol):
  return like(vol, cc3d_numpy.connected_components(vol, COMPONENTS)[0])


def np_paste(vol):
  box = box_of(vol.shape)
  return paste_volumes.edited(vol, box, other_of(vol)[box])


def np_erode(vol):
  return erode_numpy.erode(vol, *ERODE)


def np_recompress(vol):
  return vol


def lookup(vol, fn):
  table = np.array([fn(v) for v in range(int(vol.max()) + 1)], dtype=vol.dtype)
  return like(vol, table[vol])


def decode(checker, binary):
  """The checker's decode of a stream, as an array in the stream's memory order."""
  import crackle_amd
  head = crackle_amd.header(binary)
  return checker.decompress(binary).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")


def stored_list(binary):
  """The unique list of a FLAT stream as it is stored (a pin stream: its list without the background colour)."""
  import crackle_amd
  from crackle_amd import codec
  head = crackle_amd.header(binary)
  n, off = codec._label_section(binary, head)
  return np.frombuffer(binary, dtype=head.stored_dtype, offset=off, count=n).astype(head.dtype)


def stats_numpy(vol):
  """{label: (count, integer coordinate sums [3], [xmin, ymin, zmin, xmax, ymax, zmax])} of the labels vol holds."""
  v = np.asarray(vol)
  out = {}
  uniq, inverse = np.unique(v, return_inverse=True)
  inverse = inverse.reshape(v.shape)
  for i, lab in enumerate(uniq.tolist()):
    where = np.argwhere(inverse == i)
    out[int(lab)] = (len(where), where.sum(axis=0).astype(np.uint64), where.min(axis=0).tolist() + where.max(axis=0).tolist())
  return out


# ---- the kinds ---------------------------------------------------------------------------------------------------------

def kinds_host(vol, checker, only=None):
  """The kinds the host can make from vol: Kind records, in the order of HOST_KINDS."""
  import crackle_amd
  other = other_of(vol)
  order = "F" if vol.flags.f_contiguous else "C"
  flat = checker.compress(vol)
  half = np_remap(vol)
  sz = vol.shape[2]

  def part(arr, z0, z1):
    return like(vol, arr[:, :, z0:z1])

  def kind(name, stream, expected, z=(0, sz), **kw):
    base = part(vol, *z)
    source = flat if z == (0, sz) else checker.compress(base)
    return Kind(name, stream, expected, base, source, part(other, *z), **kw)

  out = []
  want = HOST_KINDS if only is None else only
  remapped = crackle_amd.remap(flat, rv.floordiv_mapping(vol, 2))
  permuted = rv.permuted_stream(flat, PERMUTE)
  for name in want:
    if name == "flat":
      out.append(kind(name, flat, vol))
    elif name == "pins":
      out.append(kind(name, checker.compress(vol, allow_pins=True), vol))
    elif name == "markov5":
      out.append(kind(name, checker.compress(vol, markov_model_order=5), vol))
    elif name == "c-order":
      b = volume_b()
      assert vol is volume_a(), "the C-order kind has a base volume of its own"
      s = checker.compress(b)
      out.append(Kind(name, s, b, b, s, other_of(b)))
    elif name == "v0":
      out.append(kind(name, gen_golden.to_v0(flat), vol))
    elif name == "remapped":
      out.append(kind(name, remapped, half))
    elif name == "floordiv":
      out.append(kind(name, rv.floordiv_stream(flat), half))
    elif name == "permuted":
      out.append(kind(name, permuted, lookup(vol, PERMUTE)))
    elif name == "permuted-merged":
      out.append(kind(name, rv.permuted_stream(flat, PERMUTE_MERGE), lookup(vol, PERMUTE_MERGE)))
    elif name == "zsplit-mid":
      out.append(kind(name, crackle_amd.zsplit(permuted, 3)[1], part(lookup(vol, PERMUTE), 3, 4), z=(3, 4)))
    elif name == "zsplit-tail":
      out.append(kind(name, crackle_amd.zsplit(remapped, 2)[2], part(half, 3, sz), z=(3, sz)))
    elif name == "restacked":
      out.append(kind(name, crackle_amd.zstack(crackle_amd.zshatter(remapped)), half))
    else:
      raise KeyError(name)
  assert [k.name for k in out] == list(want)
  return out


def kinds_device(vol, checker, only=None):
  """The kinds only the device can make from vol, in the order of DEVICE_KINDS."""
  import crackle_amd
  other = other_of(vol)
  flat = checker.compress(vol)
  remapped = crackle_amd.remap(flat, rv.floordiv_mapping(vol, 2))
  half = np_remap(vol)
  box = box_of(vol.shape)
  out = []
  want = DEVICE_KINDS if only is None else only
  for name in want:
    if name == "dusted":
      out.append(Kind(name, crackle_amd.dust(flat, DUST[0], connectivity=DUST[1]), np_dust(vol), vol, flat, other))
    elif name == "filled":
      out.append(Kind(name, crackle_amd.fill_holes(flat, FILL), np_fill(vol), vol, flat, other))
    elif name == "dusted-filled":
      s = crackle_amd.fill_holes(crackle_amd.dust(flat, DUST[0], connectivity=DUST[1]), FILL)
      out.append(Kind(name, s, np_fill(np_dust(vol)), vol, flat, other))
    elif name == "components":
      v8 = like(vol, vol.astype(np.uint8))
      assert int(vol.max()) < 256
      flat8 = checker.compress(v8)
      ccl, mapping = cc3d_numpy.connected_components(v8, COMPONENTS)
      o8 = other_of(v8)
      out.append(Kind(name, crackle_amd.connected_components(flat8, COMPONENTS), like(vol, ccl), v8, flat8, o8, mapping=mapping))
    elif name == "pasted":
      want_vol = paste_volumes.edited(half, box, other[box])
      # paste() re-encodes the slices of the box's z-range alone: the others keep the remapped stream's cracks
      cracks = vol.copy(order="K")
      cracks[:, :, box[2]] = want_vol[:, :, box[2]]
      out.append(Kind(name, crackle_amd.paste(remapped, box, other[box]), want_vol, vol, flat, other, cracks=cracks, keeps=False))
    elif name == "eroded":
      want_vol = np_erode(vol)
      out.append(Kind(name, crackle_amd.erode(flat, ERODE[0], erode_border=ERODE[1]), want_vol, vol, flat, other, cracks=want_vol, keeps=False))
    elif name == "recompressed":
      out.append(Kind(name, crackle_amd.recompress(remapped), half, vol, flat, other, cracks=half, keeps=False))
    else:
      raise KeyError(name)
  return out


def kinds_large(checker, device):
  """flat, remapped and (with device) dusted of the large volume."""
  vol = volume_large()
  out = kinds_host(vol, checker, only=["flat", "remapped"])
  if device:
    out += kinds_device(vol, checker, only=["dusted"])
  for k in out:
    k.name = "large-" + k.name
  return out
