"""One ckl_decoder driven through every entry point of include/crackle_amd.h, for the tests that let different
entry points meet on one session (tests/test_gpu_decode_session.py), and the order in which they meet.

DecodeSession is a thin ctypes wrapper in the style of Session in tests/test_gpu_cutout.py: one method per entry
point, every result copied to host numpy data.  The device outputs (run, cutout, vcg) go into a torch buffer that
carries a 0xA5 pattern in front of and behind the bytes the call may write; the pattern is checked after every call.
A call that returns an error code raises RuntimeError with the library's message and leaves the session open.

schedule(ops) is the order of the calls: an Eulerian circuit of the complete digraph with loops over the
operations, so every ordered pair (a, b), (a, a) included, occurs at adjacent positions exactly once.  It is
constructed (Hierholzer's algorithm over successor lists in the given order), not drawn: the same list on every
call, starting with the operation passed first.  Pure Python; tests/test_decode_session_cpu.py checks it."""
import ctypes as C

import numpy as np

# the nine entry points as tests/test_gpu_decode_session.py names them
OPS = ("P", "L", "C", "K", "S", "T", "V4", "V6", "X")
GUARD = 64      # bytes of pattern on either side of a device output
PATTERN = 0xA5


def schedule(ops):
  """Every ordered pair of `ops`, loops included, at adjacent positions exactly once: len(ops)^2 + 1 entries that
  begin and end with ops[0]."""
  ops = list(ops)
  if len(set(ops)) != len(ops):
    raise ValueError("schedule: the operations must be distinct")
  if not ops:
    return []
  # Hierholzer: walk unused edges until stuck (always back at the start of the walk: in-degree = out-degree), then
  # back up to the last vertex that still has one.  Successors are taken in the order given, loop first.
  unused = {a: [b for b in reversed([a] + [o for o in ops if o != a])] for a in ops}
  stack, circuit = [ops[0]], []
  while stack:
    v = stack[-1]
    if unused[v]:
      stack.append(unused[v].pop())
    else:
      circuit.append(stack.pop())
  circuit.reverse()
  return circuit


def around(pivot, ops):
  """The short schedule: every other operation once behind `pivot` and once in front of it."""
  out = [pivot]
  for o in ops:
    if o != pivot:
      out += [o, pivot]
  return out


def hand_over(first, ops, again=("P", "L", "C")):
  """The hand-over schedule: `first`, then every other operation once, then `again`."""
  return [first] + [o for o in ops if o != first] + list(again)


def pairs_of(sequence):
  """The ordered pairs at adjacent positions of a sequence of operations."""
  return set(zip(sequence[:-1], sequence[1:]))


class DecodeSession:
  """ckl_decoder_create(binary, z0, z1), or ckl_decoder_create_device when `device_stream` (a torch uint8 tensor on
  the device that holds the same bytes) is given.  `binary` is always needed: sizes come from its header."""

  def __init__(self, binary, z0=0, z1=-1, device_stream=None):
    import crackle_amd
    from crackle_amd import _lib
    self._lib = _lib
    self.L = _lib.lib()
    self.binary = bytes(binary)
    self.head = crackle_amd.header(self.binary)
    self.z0 = int(z0)
    self.z1 = int(self.head.sz if z1 < 0 else z1)
    self.ns = self.z1 - self.z0
    self.order = "F" if self.head.fortran_order else "C"
    self.table_capacity = crackle_amd.num_labels(self.binary) + 1
    self.device_stream = device_stream      # must outlive the session
    self.h = C.c_void_p()
    if device_stream is None:
      rc = self.L.ckl_decoder_create(self.binary, len(self.binary), self.z0, self.z1, 0, C.byref(self.h))
    else:
      assert device_stream.is_cuda and device_stream.numel() == len(self.binary)
      rc = self.L.ckl_decoder_create_device(device_stream.data_ptr(), len(self.binary), self.z0, self.z1, 0, C.byref(self.h))
    if rc != _lib.CKL_OK:
      raise RuntimeError(_lib.last_error())
    self._hip = None

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def close(self):
    if self.h:
      self.L.ckl_decoder_destroy(self.h)
      self.h = C.c_void_p()

  def _check(self, rc):
    if rc != self._lib.CKL_OK:
      raise RuntimeError(self._lib.last_error())

  def _device_output(self, nbytes, call):
    """call(pointer, nbytes) into a fresh torch buffer; the used bytes on the host.  The pattern around them must
    be intact, whatever the call returned."""
    import torch
    buf = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    rc = call(buf.data_ptr() + GUARD, nbytes)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == PATTERN).all(), "bytes in front of the output were written"
    assert (host[GUARD + nbytes:] == PATTERN).all(), "bytes behind the output were written"
    self._check(rc)
    return host[GUARD:GUARD + nbytes]

  def _labels(self, raw, shape, label):
    dtype = bool if label is not None else self.head.dtype
    return raw.view(np.uint8).view(dtype).reshape(shape, order=self.order)

  # ---- the entry points ----
  def run(self, label=None):
    """ckl_decoder_run: the volume of the range, or the bool image of `label`."""
    width = 1 if label is not None else self.head.data_width
    n = self.head.sx * self.head.sy * self.ns * width
    raw = self._device_output(n, lambda p, cap: self.L.ckl_decoder_run(self.h, p, cap, int(label is not None), int(label or 0)))
    return self._labels(raw, (self.head.sx, self.head.sy, self.ns), label)

  def cutout(self, box, label=None):
    """ckl_decoder_cutout of box = (x0, x1, y0, y1) over the session's slices."""
    x0, x1, y0, y1 = box
    width = 1 if label is not None else self.head.data_width
    n = (x1 - x0) * (y1 - y0) * self.ns * width
    raw = self._device_output(n, lambda p, cap: self.L.ckl_decoder_cutout(self.h, x0, x1, y0, y1, p, cap, int(label is not None), int(label or 0)))
    return self._labels(raw, (x1 - x0, y1 - y0, self.ns), label)

  def vcg(self, connectivity):
    """ckl_decoder_vcg: one byte per voxel of the range, as the library lays them out."""
    n = self.head.sx * self.head.sy * self.ns
    return self._device_output(n, lambda p, cap: self.L.ckl_decoder_vcg(self.h, p, cap, int(connectivity))).copy()

  def check(self):
    """ckl_decoder_check: the verdict word of every slice of the range."""
    errs = np.full((self.ns,), 0xFFFFFFFF, dtype=np.uint32)
    self._check(self.L.ckl_decoder_check(self.h, errs.ctypes.data, errs.size))
    return errs

  def label_stats(self):
    """ckl_decoder_label_stats: (labels uint64 [n], counts uint64 [n], sums uint64 [n, 3], boxes uint32 [n, 6])."""
    cap = self.table_capacity
    lab = np.zeros((cap,), np.uint64)
    cnt = np.zeros((cap,), np.uint64)
    sums = np.zeros((cap, 3), np.uint64)
    box = np.zeros((cap, 6), np.uint32)
    n = C.c_uint64()
    self._check(self.L.ckl_decoder_label_stats(self.h, cap, lab.ctypes.data, cnt.ctypes.data, sums.ctypes.data, box.ctypes.data, C.byref(n)))
    n = int(n.value)
    return lab[:n], cnt[:n], sums[:n], box[:n]

  def contacts(self):
    """ckl_decoder_contacts: (pairs uint64 [n, 2] ascending by (a, b), faces uint64 [n, 3]); the library's two
    arrays are released with ckl_free."""
    pp, fp, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    try:
      self._check(self.L.ckl_decoder_contacts(self.h, C.byref(pp), C.byref(fp), C.byref(n)))
      k = int(n.value)
      if k == 0:
        return np.zeros((0, 2), np.uint64), np.zeros((0, 3), np.uint64)
      pairs = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint64)), shape=(k, 2)).copy()
      faces = np.ctypeslib.as_array(C.cast(fp, C.POINTER(C.c_uint64)), shape=(k, 3)).copy()
      return pairs, faces
    finally:
      for p in (pp, fp):
        if p.value:
          self.L.ckl_free(p)

  def crack_planes(self):
    """ckl_decoder_crack_planes: (plane V, plane H) of every slice of the range, uint32 [ns, rows, row_words],
    copied from the session's own buffer with hipMemcpy."""
    pv, ph, row_words, plane_words = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint64()
    self._check(self.L.ckl_decoder_crack_planes(self.h, C.byref(pv), C.byref(ph), C.byref(row_words), C.byref(plane_words)))
    if self._hip is None:
      self._hip = C.CDLL("libamdhip64.so")
    words = int(plane_words.value) * self.ns
    out = []
    for p in (pv, ph):
      host = np.zeros((words,), np.uint32)
      assert p.value and self._hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(p.value), C.c_size_t(host.nbytes), 2) == 0
      out.append(host.reshape(self.ns, -1, int(row_words.value)))
    return out[0], out[1]

  def stages(self):
    """ckl_decoder_stage_timing: the kernels of the last call, in launch order."""
    names = []
    for i in range(64):
      name, ms = C.c_char_p(), C.c_float()
      if self.L.ckl_decoder_stage_timing(self.h, i, C.byref(name), C.byref(ms)) != self._lib.CKL_OK:
        break
      names.append(name.value.decode())
    return names
