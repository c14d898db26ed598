"""Volumes aimed at the size decisions of the encoder's flat label table (crackle_amd/csrc/ckl_encode_labels.hip: flat_section
and its kernels; ckl_encode.hip: crc32c_device, k_copy_bytes, k_code_offsets).  Plain numpy; shared by the CPU test that pins every
case against the checker's own stream (tests/test_label_table_volumes_cpu.py) and by the GPU tests that run the kernels
on them (tests/test_gpu_label_table.py).

What a case controls, and what the encoder decides from it:
  N  2D (4-connected) components in total    hash pass before the sort (N > 8192), hash table size (2 N rounded up),
                                             keys sorted when the hash pass is switched off
  U  distinct labels                         keys sorted on the default path, padded sort size (2048 * 2^k >= keys), key
                                             width (U <= 255, <= 65535), blocks of 2048 in unique_heads
  L  bytes of the label section              frame of the crc32c on the device (G workgroups, P bytes per thread)

The construction (components_volume).  In every slice the first n - 1 pixels in raster order are single-pixel components
that cycle through values[1:] by their running index over the whole volume; the rest of the slice is one stretch of
values[0].  Horizontal neighbours differ because the cycle has two labels or more, vertical neighbours because their
indices differ by sx, which must be no multiple of the cycle's length.  The stretch has one pixel at least (a slice
"of single pixels only" ends in a stretch of one), so values[0] is in every slice and U = len(values) as soon as the
single pixels are as many as the cycle is long.

Components are numbered in raster order of their first pixels, slice by slice, so the table sees the labels in the
order component_labels() returns: the cycle, then values[0] at each slice's end.

Out of reach of tests that take seconds, and left out: more than 2^26 components (the hash pass's upper bound) and
slices of more than 2^32 pixels (component counts of 8 bytes)."""
import numpy as np

MAX64 = (1 << 64) - 1
HASH_ABOVE = 8192          # flat_section: hash pass for N > 8192
SORT_BLOCK = 2048          # k_bitonic_first / k_bitonic_local, kUniqItems


def byte_width(x):
  return 1 if x <= 0xFF else 2 if x <= 0xFFFF else 4 if x <= 0xFFFFFFFF else 8


def section_length(u, stored_width, sz, comp_width, n):
  """u64 num_unique | unique[u] : stored_width | components per slice [sz] : comp_width | key[n] : byte_width(u)"""
  return 8 + u * stored_width + sz * comp_width + n * byte_width(u)


def padded_sort_size(n_sort):
  n_pad = SORT_BLOCK
  while n_pad < n_sort:
    n_pad <<= 1
  return n_pad


def hash_slots(n):
  slots = 16384
  while slots < 2 * n:
    slots <<= 1
  return slots


def crc_frame(length):
  """(G, P) of crc32c_device for a section of `length` bytes."""
  p, g = 128, 1
  while g < 256 and g * 256 * p < length:
    g <<= 1
  if g * 256 * p < length:
    p = ((length + g * 256 - 1) // (g * 256) + 15) // 16 * 16
  return g, p


# ---- the construction ------------------------------------------------------------------------------------------------
def _per_slice(shape, n_components):
  sx, sy, sz = (int(s) for s in shape)
  n = int(n_components)
  if not sz <= n <= sx * sy * sz:
    raise ValueError(f"{n} components do not fit {sz} slices of {sx * sy} pixels, one each at least")
  return np.array([n // sz + (1 if z < n % sz else 0) for z in range(sz)], dtype=np.int64)


def _checked_values(shape, n_components, values, dtype):
  sx = int(shape[0])
  vals = np.asarray(values, dtype=np.uint64).reshape(-1)
  if vals.size == 0 or np.unique(vals).size != vals.size:
    raise ValueError("values must be distinct and at least one")
  if int(vals.max()) > int(np.iinfo(dtype).max):
    raise ValueError(f"{int(vals.max())} does not fit {np.dtype(dtype).name}")
  per = _per_slice(shape, n_components)
  singles = per - 1
  m = vals.size - 1
  if int(singles.sum()) < m:
    raise ValueError(f"{int(singles.sum())} single pixels cannot show {m} labels: U would fall short of len(values)")
  if int(singles.max()) >= 1 and m < 1:
    raise ValueError("single pixels need a label of their own")
  if int(singles.max()) >= 2 and m < 2:
    raise ValueError("two single pixels side by side need two labels to cycle through")
  if int(singles.max()) > sx and sx % m == 0:
    raise ValueError(f"sx = {sx} is a multiple of the cycle's length {m}: vertical neighbours would merge")
  return vals, per


def component_labels(shape, n_components, values, dtype=np.uint64):
  """The label of every component in the encoder's component order (uint64)."""
  vals, per = _checked_values(shape, n_components, values, dtype)
  out = np.empty(int(per.sum()), dtype=np.uint64)
  m = vals.size - 1
  o = k = 0
  for n in per:
    s = int(n) - 1
    if s:
      out[o:o + s] = vals[1 + (k + np.arange(s, dtype=np.int64)) % m]
    out[o + s] = vals[0]
    o += s + 1
    k += s
  return out


def components_volume(shape, n_components, values, dtype):
  """An F-ordered volume with exactly n_components 2D components, spread over the slices as evenly as they go, and
  exactly the labels in `values` (see the module's docstring); refuses arguments that would give another count."""
  sx, sy, sz = (int(s) for s in shape)
  vals, per = _checked_values(shape, n_components, values, dtype)
  sxy = sx * sy
  f = np.full(sxy * sz, vals[0], dtype=np.uint64)
  m = vals.size - 1
  k = 0
  for z, n in enumerate(per):
    s = int(n) - 1
    if s:
      f[z * sxy:z * sxy + s] = vals[1 + (k + np.arange(s, dtype=np.int64)) % m]
    k += s
  return np.asfortranarray(f.astype(dtype).reshape((sx, sy, sz), order="F"))


def count_components(arr):
  """2D 4-connected components of every slice, by union-find over the equal neighbours (slow, plain: small volumes)."""
  arr = np.asarray(arr)
  sx, sy, sz = arr.shape
  total = 0
  for z in range(sz):
    a = arr[:, :, z]
    parent = np.arange(sx * sy)

    def find(i):
      while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
      return i

    idx = np.arange(sx * sy).reshape(sx, sy, order="F")
    for p, q in ((idx[1:, :][a[1:, :] == a[:-1, :]], idx[:-1, :][a[1:, :] == a[:-1, :]]),
                 (idx[:, 1:][a[:, 1:] == a[:, :-1]], idx[:, :-1][a[:, 1:] == a[:, :-1]])):
      for i, j in zip(p.tolist(), q.tolist()):
        ri, rj = find(i), find(j)
        if ri != rj:
          parent[max(ri, rj)] = min(ri, rj)
    total += sum(1 for i in range(sx * sy) if find(i) == i)
  return total


# ---- value sets: written in the order of first appearance, by_appearance() turns them into `values` ------------------
def by_appearance(labels):
  """values for components_volume such that the labels first appear in the given order, as long as the first slice
  holds them all (the stretch's label, values[0], comes last in its slice)."""
  labels = np.asarray(labels, dtype=np.uint64)
  return np.concatenate((labels[-1:], labels[:-1]))


def ascending(u, base=1, step=1):
  return np.uint64(base) + np.uint64(step) * np.arange(u, dtype=np.uint64)


def descending(u, base=1, step=1):
  return ascending(u, base, step)[::-1].copy()


def permuted(u, base=1, step=1):
  """A fixed permutation: i -> (1000003 i + 12345) mod u (1000003 is prime and larger than every u used here)."""
  assert u < 1000003
  i = (np.arange(u, dtype=np.uint64) * np.uint64(1000003) + np.uint64(12345)) % np.uint64(u)
  return np.uint64(base) + np.uint64(step) * i


ORDERS = {"asc": ascending, "desc": descending, "perm": permuted}


def low32_equal(u):
  """Equal in their low 32 bits, different above: k << 33 | 5."""
  return (np.arange(u, dtype=np.uint64) << np.uint64(33)) | np.uint64(5)


def dense(u):
  """0 .. u - 1."""
  return np.arange(u, dtype=np.uint64)


def pow2_multiples(u, shift=40):
  """k << shift for k = 1 .. u: nothing in the low bits."""
  return np.arange(1, u + 1, dtype=np.uint64) << np.uint64(shift)


# ---- cases -----------------------------------------------------------------------------------------------------------
class Case:
  """One volume and what its stream must say: n components, u labels, the label section's length, the key width."""

  def __init__(self, id, shape, dtype, n, u, values, markov=0):
    self.id, self.shape, self.dtype, self.n, self.u, self.markov = id, tuple(shape), dtype, int(n), int(u), int(markov)
    self._values = values      # an array, or a function without arguments that returns one (large sets are made late)

  @property
  def values(self):
    v = self._values() if callable(self._values) else self._values
    v = np.asarray(v, dtype=np.uint64)
    assert v.size == self.u, (self.id, v.size, self.u)
    return v

  def volume(self):
    return components_volume(self.shape, self.n, self.values, self.dtype)

  @property
  def stored_width(self):
    return byte_width(int(self.values.max()))

  @property
  def key_width(self):
    return byte_width(self.u)

  @property
  def length(self):
    sx, sy, sz = self.shape
    return section_length(self.u, self.stored_width, sz, byte_width(sx * sy), self.n)

  @property
  def claims(self):
    return {"N": self.n, "U": self.u, "key_width": self.key_width, "L": self.length}

  def __repr__(self):
    return self.id


def read_claims(stream):
  """N, U, key width and L as a stream's header and flat label section state them."""
  import crackle_amd
  head = crackle_amd.header(stream)
  assert head.label_format == 0, "flat labels expected"
  off = head.header_bytes + head.grid_index_bytes
  sec = stream[off:off + head.num_label_bytes]
  u = int.from_bytes(sec[:8], "little")
  cw = byte_width(head.sx * head.sy)
  o = 8 + u * head.stored_data_width
  per = np.frombuffer(sec, dtype={1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}[cw], count=head.sz, offset=o)
  n = int(per.astype(np.uint64).sum())
  o += head.sz * cw
  kw = byte_width(u)
  assert len(sec) == o + n * kw == section_length(u, head.stored_data_width, head.sz, cw, n)
  return {"N": n, "U": u, "key_width": kw, "L": head.num_label_bytes}


def read_component_labels(stream):
  """The label of every component as the stream's keys name it (uint64)."""
  import crackle_amd
  head = crackle_amd.header(stream)
  off = head.header_bytes + head.grid_index_bytes
  sec = stream[off:off + head.num_label_bytes]
  u = int.from_bytes(sec[:8], "little")
  uniq = np.frombuffer(sec, dtype=f"<u{head.stored_data_width}", count=u, offset=8).astype(np.uint64)
  o = 8 + u * head.stored_data_width + head.sz * byte_width(head.sx * head.sy)
  kw = byte_width(u)
  keys = np.frombuffer(sec, dtype=f"<u{kw}", count=(len(sec) - o) // kw, offset=o)
  return uniq[keys]


def _rows(n, sx, sz=1, spare=1):
  """sy such that sz slices of sx x sy hold n components and `spare` rows more."""
  return -(-n // (sx * sz)) + spare


THREE = np.array([7, 200, 90], dtype=np.uint64)      # U = 3: the hash pass collapses everything, sort-all sorts N keys of three values


def hash_threshold_cases():
  """N on both sides of 8192 (hash pass or not) and of 16384, 32768 (the table doubles): with U about N / 2, with
  U = 3, and (where the table is used) with U = N, which fills the table to exactly one half just below a step."""
  out = []
  for n in (8192, 8193, 16384, 16385, 32768, 32769):
    shape = (127, _rows(n, 127, 3), 3)
    u = n // 2 + 1
    out.append(Case(f"N{n}-U{u}", shape, np.uint32, n, u, lambda u=u: by_appearance(permuted(u, 70000, 7))))
    out.append(Case(f"N{n}-U3", shape, np.uint8, n, 3, THREE))
  for n in (16384, 16385, 32768, 32769):
    out.append(Case(f"N{n}-U{n}-half-full", (127, _rows(n, 127), 1), np.uint32, n, n, lambda n=n: by_appearance(permuted(n, 3, 5))))
  return out


def sort_size_cases():
  """The default path sorts the U distinct labels the hash pass found (N > 8192): U on both sides of the padded sizes
  2048, 4096, 8192, 16384, and 65537 and 2^18, in three value orders.  2048 runs k_bitonic_first alone, 4096 one
  k_bitonic_step, 8192 the first k_bitonic_step2; 16384, 32768, 131072 and 262144 both parities of the global steps.
  Every unique_heads block starts with a head here (distinct keys): U at 2047 / 2048 / 2049 multiples."""
  out = []
  for u in (2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8192, 8193, 16385, 65537, 1 << 18):
    n = 8704 if u <= 8192 else u + (0 if u == 1 << 18 else 37)
    orders = ("asc", "desc", "perm") if u in (2048, 2049, 4096, 4097, 8192, 8193, 16385, 65537, 1 << 18) else ("perm",)
    for order in orders:
      out.append(Case(f"U{u}-N{n}-pad{padded_sort_size(u)}-{order}", (509, _rows(n, 509), 1), np.uint32, n, u,
                      lambda u=u, order=order: by_appearance(ORDERS[order](u, 100000, 3))))
  return out


def sort_all_cases():
  """At most 8192 components: every component's label is sorted (N keys), so N sits on the padded sizes and on the
  2048-key blocks of unique_heads.  Distinct labels in three orders make every block start with a head.  With three
  labels, one slice and an odd N the two cycling labels have (N - 1) / 2 components each and the stretch's label one:
  as the smallest ("low") it shifts the sorted keys by one, so that for N = 4097 key 2048 continues the run of key
  2047; as the largest ("high") the runs end at 2047 and 4095 and keys 2048 and 4096 are heads.
  10239 .. 10241 take the hash pass by default and five or six blocks of keys when it is switched off."""
  out = []
  for n in (2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192):
    shape = (127, _rows(n, 127), 1)
    for order in ("asc", "desc", "perm"):
      out.append(Case(f"N{n}-distinct-{order}", shape, np.uint32, n, n, lambda n=n, order=order: by_appearance(ORDERS[order](n, 5, 11))))
    out.append(Case(f"N{n}-three-low", shape, np.uint16, n, 3, np.array([2, 300, 400], dtype=np.uint64)))
    out.append(Case(f"N{n}-three-high", shape, np.uint16, n, 3, np.array([500, 300, 400], dtype=np.uint64)))
  for n in (10239, 10240, 10241):
    shape = (127, _rows(n, 127), 1)
    out.append(Case(f"N{n}-three-low", shape, np.uint16, n, 3, np.array([2, 300, 400], dtype=np.uint64)))
    out.append(Case(f"N{n}-three-high", shape, np.uint16, n, 3, np.array([500, 300, 400], dtype=np.uint64)))
  return out


def key_width_cases():
  """U = 255 / 256 and 65535 / 65536 behind the hash pass, and 255 / 256 below it."""
  out = []
  for u, n in ((255, 8300), (256, 8300), (65535, 66000), (65536, 66000), (255, 4000), (256, 4000)):
    out.append(Case(f"U{u}-N{n}-keys{byte_width(u)}", (509, _rows(n, 509), 1), np.uint32, n, u, lambda u=u: by_appearance(permuted(u, 1 << 20, 9))))
  return out


def edge_value_cases():
  """The all-ones uint64 label is the hash table's empty marker (and what the sort pads with): alone, as one of two,
  beside 0, among thousands; labels that differ only above bit 32; 0xFFFFFFFF in a uint32 volume, which is no marker;
  0 among dense small labels; multiples of 2^40 and 2^32."""
  u64, out = np.uint64, []
  arr = lambda *v: np.array(v, dtype=np.uint64)
  # (1, 1, sz): every slice is one component of values[0].  (2, 1, sz): one single pixel of values[1] and values[0]
  for tag, sz in (("hash", 8193), ("sorted", 4096)):
    out.append(Case(f"only-max-{tag}", (1, 1, sz), u64, sz, 1, arr(MAX64)))
  for tag, sz in (("hash", 4097), ("sorted", 2048)):
    out.append(Case(f"max-and-max-1-{tag}", (2, 1, sz), u64, 2 * sz, 2, arr(MAX64 - 1, MAX64)))
    out.append(Case(f"max-1-and-max-{tag}", (2, 1, sz), u64, 2 * sz, 2, arr(MAX64, MAX64 - 1)))
    out.append(Case(f"zero-and-max-{tag}", (2, 1, sz), u64, 2 * sz, 2, arr(0, MAX64)))
  for tag, n in (("hash", 8300), ("sorted", 4000)):
    shape = (127, _rows(n, 127), 1)
    out.append(Case(f"low32-equal-{tag}", shape, u64, n, 3001, lambda: by_appearance(low32_equal(3001)[::-1])))
    out.append(Case(f"low32-equal-and-max-{tag}", shape, u64, n, 3002, lambda: np.concatenate((arr(MAX64), low32_equal(3001)))))
    out.append(Case(f"u32-all-ones-{tag}", shape, np.uint32, n, 5, arr(0xFFFFFFFF, 0, 0xFFFFFFFE, 5, 0x7FFFFFFF)))
    out.append(Case(f"u64-low-word-all-ones-{tag}", shape, u64, n, 4, arr(0xFFFFFFFF, MAX64, 0xFFFFFFFF00000000, 1 << 32)))
  out.append(Case("only-u32-all-ones-hash", (1, 1, 8193), np.uint32, 8193, 1, arr(0xFFFFFFFF)))
  shape = (127, _rows(8300, 127), 1)
  out.append(Case("dense-from-zero-hash", shape, np.uint16, 8300, 4097, lambda: by_appearance(dense(4097))))
  out.append(Case("multiples-of-2^40-hash", shape, u64, 8300, 4097, lambda: by_appearance(pow2_multiples(4097, 40))))
  out.append(Case("multiples-of-2^32-hash", shape, u64, 8300, 4097, lambda: by_appearance(pow2_multiples(4097, 32)[::-1])))
  return out


def many_slices_cases():
  """k_code_offsets gives each of its 256 threads ceil(sz / 256) slices: sz on both sides of 256, 512 and 1024."""
  out = []
  for sz in (255, 256, 257, 512, 513, 1024, 1025):
    for markov in (0, 1):
      out.append(Case(f"sz{sz}-m{markov}", (9, 8, sz), np.uint8, 3 * sz + 1, 3, THREE, markov=markov))
  return out


def volume_for_length(length):
  """A Case whose label section has exactly `length` bytes.

  269 .. 65548: one row of uint8 pixels, three labels, every pixel a component: L = 8 + 3 + 2 + sx.
  From 786444 on, multiples of 4 only: uint64 labels from 2^40 on, (256, 256, sz), U >= 65536:
  L = 8 + 8 U + 4 sz + 4 N, with the fewest slices that reach it."""
  length = int(length)
  if 8 + 3 + 2 + 256 <= length <= 8 + 3 + 2 + 65535:
    sx = length - 13
    return Case(f"L{length}-row", (sx, 1, 1), np.uint8, sx, 3, THREE)
  if length % 4 == 0 and length >= 8 + 8 * 65536 + 4 + 4 * 65536:
    sxy = 65536
    for sz in range(1, 13):
      t = (length - 8) // 4 - sz          # 2 U + N
      v = sxy * sz
      if 3 * v - 2 * sz + 2 < t:
        continue
      n = min(v, t - 2 * 65536)
      if (t - n) % 2:
        n -= 1
      u = (t - n) // 2
      if 65536 <= u <= n - sz + 1 and n >= sz:
        return Case(f"L{length}-u64", (256, 256, sz), np.uint64, n, u, lambda u=u: by_appearance(permuted(u, 1 << 40, 3)))
  raise ValueError(f"no construction for a label section of {length} bytes")


MIB8 = 8 << 20
# (wanted, used): where wanted + 1 is out of reach (the wide family has multiples of 4 only) the next reachable length
CRC_LENGTHS = [(32768, 32768), (32769, 32769), (65536, 65536), (65537, 65537), (1 << 20, 1 << 20), ((1 << 20) + 1, (1 << 20) + 4),
               (MIB8, MIB8), (MIB8 + 1, MIB8 + 4)]
# small, large, small, large: the piece length P goes 128, 144, 128, 144, 128 (crc32c_device caches the shifts of one P)
CRC_ORDER = [32768, MIB8 + 4, 65536, MIB8, 32769, MIB8 + 4, 65537, 1 << 20, (1 << 20) + 4]


def crc_cases():
  return {used: volume_for_length(used) for _, used in CRC_LENGTHS}


class MergedCase:
  """Two z-slabs of one volume, encoded apart against the merged list of both and stacked."""

  def __init__(self, id, first, second):
    self.id, self.first, self.second = id, first, second

  def slabs(self):
    return [self.first.volume(), self.second.volume()]

  def whole(self):
    return np.asfortranarray(np.concatenate(self.slabs(), axis=2))

  def __repr__(self):
    return self.id


def merged_cases():
  """sorted: both slabs at most 8192 components (their lists arrive sorted).  unsorted: more (the lists arrive as the
  hash pass left them).  longer-than-N: a slab of ten components against a merged list of thousands.  The slabs'
  label sets overlap in part, so that merged keys differ from local ones."""
  shape = (127, 24, 2)
  big = (127, 48, 2)
  return [
    MergedCase("sorted", Case("a", shape, np.uint32, 3000, 2500, lambda: by_appearance(permuted(2500, 70000, 4))),
               Case("b", shape, np.uint32, 3001, 2000, lambda: by_appearance(permuted(2000, 70002, 6)))),
    MergedCase("unsorted", Case("a", big, np.uint32, 9000, 6000, lambda: by_appearance(permuted(6000, 70000, 4))),
               Case("b", big, np.uint32, 8193, 5000, lambda: by_appearance(permuted(5000, 70002, 6)))),
    MergedCase("longer-than-N", Case("a", shape, np.uint32, 10, 7, np.array([70004, 1 << 20, 70000, 70016, 90001, 70008, 3], dtype=np.uint64)),
               Case("b", shape, np.uint32, 5000, 4000, lambda: by_appearance(permuted(4000, 70000, 4)))),
  ]
