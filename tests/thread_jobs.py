"""What the threaded tests run: a catalogue of job kinds over every entry family of the library, the schedule that
puts every pair of kinds on the device at the same time, and the child process that runs a scenario and prints one
JSON document (python -m thread_jobs SCENARIO THREADS, from tests/).  tests/test_thread_jobs_cpu.py pins the catalogue
without a GPU; tests/test_gpu_threads.py starts the children.

A kind is a list of inputs; an input is a callable with the result it has to give.  Every expected result is there
before a thread starts and never comes from the library under test: bytes from the checker (compress, reencode,
mode_pooling_2x2x1, and its point_cloud and voxel_connectivity_graph, which depend on the stream's cracks), everything
else from the numpy restatements the other tests use (tests/*_numpy.py, stream_kinds.stats_numpy).  Building the
catalogue does not load libcrackle_amd.so.  An editor whose bytes the checker cannot predict (connected_components,
dust, fill_holes, paste: they keep the source's cracks) is checked by decoding its result in the same job and
comparing the volume with numpy.

Where the dynamic LDS of a kernel depends on the input, a kind has inputs on both sides of 64 KiB (lds_sides): the
limit of such a kernel is a property of the process, so the large input of one thread and the small one of another
are what a per-call setting would get wrong.  The host rules are restated here from the code (ckl_encode.hip:
trail_walk_lds, the clds line of crack_pass, emit_plan; ckl_encode_labels.hip: flat_resolve_cap; ckl_operations.hip: lds_comps *
kStatsBytesPerComp, vis_words) for a device with MAX_LDS bytes of LDS per workgroup; the GPU test checks that figure
and compares the two rules tests/test_gpu_consumer_edges.py restates as well with that file's functions.

A round of the schedule has four jobs, one per thread.  Jobs with two sessions at once (overlaps, array_equal, the
editors: a decoder and an encoder) take a round beyond the session cache's four sets; the many-sessions scenario does
so with five threads."""
import importlib.util
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
  if p not in sys.path:
    sys.path.insert(0, p)

import cc3d_numpy
import contacts_numpy as cn
import dilate_numpy
import dust_numpy
import erode_numpy
import fill_holes_numpy
import fill_holes_volumes
import overlaps_numpy as on
import paste_volumes
import recompress_volumes as rv
import stream_kinds as sk
from test_gpu_trail_long_segments import crack_graph
from util import flat_1d

THREADS = 4            # a process has four hardware queues on these machines, a command 16 CPUs
CALLS_PER_ROUND = 8
MAX_LDS = 160 * 1024   # LDS per workgroup of gfx950 (hipDeviceAttributeMaxSharedMemoryPerBlock): asserted on the device
LDS_LINE = 64 * 1024   # a straddling pair has one input above it; the other needs a few KiB
LDS_SMALL = 16 * 1024
EMIT_STATIC_LDS = 4168     # k_trail_emit's own arrays (profiles/trail_emit_ab.txt, section 3)


# ---- volumes -----------------------------------------------------------------------------------------------------------

def cells(shape, cell, dtype, modulus=251):
  """Cells of cell x cell pixels, every one a 2D component; neighbours never share a label (1 and nx are not 0 mod 251)."""
  sx, sy, sz = shape
  nx = -(-sx // cell)
  x, y, z = np.meshgrid(np.arange(sx) // cell, np.arange(sy) // cell, np.arange(sz), indexing="ij")
  assert nx % modulus not in (0, 1, modulus - 1)
  return np.asfortranarray((1 + (x + nx * y + 7 * z) % modulus).astype(dtype))


def stripes(shape, dtype):
  """Rows of period 5 along y (labels 1 2 1 2 2): four straight cracks of sx moves per five rows, border to border, no
  vertex of degree 3 or 4: many crack edges (the emit kernel's word buffer) on few nodes (its chain tables)."""
  sx, sy, sz = shape
  row = np.array([1, 2, 1, 2, 2], dtype)[np.arange(sy) % 5]
  return np.asfortranarray(np.broadcast_to(row[None, :, None], shape).astype(dtype))


def dots(shape, dtype):
  """Isolated pixels on a background, every third column and every second row: closed loops without a node, so the
  label stage starts beside the walk (the strip kernels), with more strip components than the first resolve table holds."""
  sx, sy, sz = shape
  vol = np.ones(shape, dtype, order="F")
  xs, ys = np.meshgrid(np.arange(1, sx - 1, 3), np.arange(1, sy - 1, 2), indexing="ij")
  for z in range(sz):
    vol[xs, ys, z] = 2 + (xs + 5 * ys + z) % 200
  return vol


def halves(shape, dtype):
  vol = np.ones(shape, dtype, order="F")
  vol[shape[0] // 2:, :, :] = 2
  vol[:, shape[1] // 2:, 1:] += 2
  return vol


def planes(shape, dtype):
  """A few large regions on one large slice: the contour tracer's visited bits pass 64 KiB, its contours stay few."""
  sx, sy, sz = shape
  vol = np.ones(shape, dtype, order="F")
  vol[sx // 3:, :, :] = 2
  vol[:, sy // 2:, :] += 2
  vol[sx // 5:sx // 5 + 40, sy // 7:sy // 7 + 33, :] = 9
  return vol


def _ro(v):
  v.setflags(write=False)
  return v


def volumes():
  a = sk.volume_a()                                                          # 97 x 61 x 7 uint32, F: the general decode path
  return {
    "a": a, "a8": sk.volume_a8(), "a64": _ro(np.asfortranarray(a.astype(np.uint64))),
    "b": sk.volume_b(),                                                      # 96 x 80 x 6 uint32, C order
    "s": _ro(fill_holes_volumes.punched((96, 64, 5), "F")),                  # sx % 4 == 0, F: the strip decode path
    "s8": _ro(np.asfortranarray(fill_holes_volumes.punched((96, 64, 5), "F").astype(np.uint8))),
    "t": _ro(fill_holes_volumes.punched((64, 52, 4), "F")),
    "noise": sk.volume_large(),                                              # 130 x 70 x 4 uint8
    "cells": _ro(cells((272, 272, 2), 4, np.uint32)),
    "cells64": _ro(cells((272, 272, 2), 4, np.uint64)),
    "deep": _ro(cells((96, 96, 6), 4, np.uint32, modulus=577)),              # hundreds of labels with columns in z: pins
    "stripes": _ro(stripes((1000, 300, 1), np.uint8)),
    "dots": _ro(dots((272, 272, 2), np.uint32)),
    "halves": _ro(halves((64, 48, 3), np.uint32)),
    "halves8": _ro(halves((64, 48, 3), np.uint8)),
    "halves64": _ro(halves((64, 48, 3), np.uint64)),
    "planes": _ro(planes((768, 704, 1), np.uint32)),
    "tiny": _ro(halves((16, 16, 2), np.uint8)),
  }


# ---- the host rules, restated --------------------------------------------------------------------------------------------

def max_special(vol):
  """Most crack vertices of degree 1, 3 or 4 in one slice (IMPERMISSIBLE cracks: between differing pixels)."""
  best = 0
  for z in range(vol.shape[2]):
    deg, _ = crack_graph(np.asarray(vol[:, :, z]))
    best = max(best, int(np.isin(deg, (1, 3, 4)).sum()))
  return best


def corners(sl):
  """Crack vertices of one slice with exactly an edge to the right and an edge down (trail_corner_mask: R & D & ~L & ~U)."""
  sx, sy = sl.shape
  right = np.zeros((sx + 2, sy + 2), bool)      # [X + 1, Y + 1]: the edge from vertex (X, Y) to (X + 1, Y); one cell of margin
  down = np.zeros((sx + 2, sy + 2), bool)       # the edge from (X, Y) to (X, Y + 1)
  right[1:sx + 1, 2:sy + 1] = sl[:, 1:] != sl[:, :-1]
  down[2:sx + 1, 1:sy + 1] = sl[1:, :] != sl[:-1, :]
  left, up = np.roll(right, 1, axis=0), np.roll(down, 1, axis=1)
  return int((right & down & ~left & ~up).sum())


def chain_capacity(vol):
  """kcap of the fullest slice (crack_pass): its special vertices and corners, rounded up past a multiple of 16."""
  best = 0
  for z in range(vol.shape[2]):
    sl = np.asarray(vol[:, :, z])
    deg, _ = crack_graph(sl)
    best = max(best, (int(np.isin(deg, (1, 3, 4)).sum()) + corners(sl) + 16) // 16 * 16)
  return best


def max_edges(vol):
  return max(crack_graph(np.asarray(vol[:, :, z]))[1] for z in range(vol.shape[2]))


def is_impermissible(vol):
  """The encoder keeps cracks between differing pixels when they are the fewer (the straddling volumes rely on it)."""
  v = np.asarray(vol)
  differing = int((v[1:] != v[:-1]).sum() + (v[:, 1:] != v[:, :-1]).sum())
  pairs = v[1:].size + v[:, 1:].size
  return differing < pairs - differing


def trail_walk_lds(special, max_lds=MAX_LDS):
  lds = (special + 256) * 16 + 1024
  return min(max_lds - 1024, max(lds, 4096)) // 16 * 16


def trail_components_lds(special, max_lds=MAX_LDS):
  clds = (special + 1024) * 12
  return min(max_lds - 1024, max(clds, 1024)) // 16 * 16


def emit_plan(edges, kcap, max_lds=MAX_LDS):
  """(k_trail_emit runs, its dynamic LDS): tcap chains staged, wcap words of 16 code points, static + dynamic within 80 KiB."""
  tcap = min(2048, (kcap + 15) // 16 * 16)
  wcap = min((edges + edges // 8 + 1024 + 15) // 16, 1 << 28)
  dyn = 4 * (2 * tcap + max(3 * tcap, wcap))
  return EMIT_STATIC_LDS + dyn <= min(80 * 1024, max_lds), dyn


def strip_components_min(vol):
  """2D components of the fullest slice: a slice has at least as many strip components."""
  from scipy import ndimage
  best = 0
  for z in range(vol.shape[2]):
    sl = np.asarray(vol[:, :, z])
    best = max(best, sum(int(ndimage.label(sl == l)[1]) for l in np.unique(sl).tolist()))
  return best


def resolve_tables(max_lds=MAX_LDS):
  """(first, largest) table of k_slice_resolve_enc in entries: 40 KiB beside the walks, then a CU's LDS less 8 KiB."""
  cap = lambda lds: min(0xFFFF, (lds - (1024 + 64) * 4) // 4)
  return cap(40960), cap(max_lds - 8192)


def labels_at_walk(special, max_lds=MAX_LDS):
  """The label stage starts beside the walk, on the strip kernels (encode_typed)."""
  return special < 5000 and 2 * ((special + 256) * 16 + 1024) + 40960 <= max_lds


def stats_lds(max_comp, max_lds=MAX_LDS):
  fit = ((max_lds - 1024) // 36) & ~1
  return min((max_comp + 1) & ~1, fit) * 36


def contour_visited_lds(sx, sy, max_lds=MAX_LDS):
  """Bytes of the tracer's visited bits when they are in LDS, else None."""
  words = (sx * sy + 31) // 32
  return words * 4 if words * 4 + 256 <= max_lds else None


def lds_sides(vols, max_lds=MAX_LDS):
  """{kernel: (bytes the large input asks for, bytes the small one does)} for the straddling pairs of the catalogue."""
  comps = lambda v: strip_components_min(v)
  first, largest = resolve_tables(max_lds)
  big_emit = emit_plan(max_edges(vols["stripes"]), chain_capacity(vols["stripes"]), max_lds)
  small_emit = emit_plan(max_edges(vols["a8"]), chain_capacity(vols["a8"]), max_lds)
  assert big_emit[0] and small_emit[0], "both take k_trail_emit"
  assert labels_at_walk(max_special(vols["dots"]), max_lds) and first < comps(vols["dots"]) <= largest
  assert labels_at_walk(max_special(vols["halves"]), max_lds) and comps(vols["halves"]) <= first
  return {
    "k_trail_walk": (trail_walk_lds(max_special(vols["cells64"]), max_lds), trail_walk_lds(max_special(vols["a64"]), max_lds)),
    "k_trail_components": (trail_components_lds(max_special(vols["cells64"]), max_lds), trail_components_lds(max_special(vols["halves64"]), max_lds)),
    "k_trail_emit": (big_emit[1], small_emit[1]),
    "k_slice_resolve_enc": (largest * 4, first * 4),
    "k_run_stats": (stats_lds(comps(vols["cells"]), max_lds), stats_lds(comps(vols["a"]), max_lds)),
    "k_trace_contours": (contour_visited_lds(*vols["planes"].shape[:2], max_lds), contour_visited_lds(*vols["a"].shape[:2], max_lds)),
    "k_markov_hist": (4 ** 6 * 4 * 4, 4 ** 3 * 4 * 4),
  }


# ---- the catalogue -----------------------------------------------------------------------------------------------------------

class Input:
  def __init__(self, name, call, want, same=None, slice_pixels=(), volume=None):
    self.name, self.call, self.want = name, call, want
    self.volume = volume      # where `want` is a stream: the volume it has to decode to, from numpy
    self.same = same if same is not None else (lambda got, want: got == want)
    self.slice_pixels = tuple(slice_pixels)      # sx * sy of the streams and volumes the call sends to the device

  def run(self):
    """(ok, text of the exception or of the mismatch)."""
    try:
      got = self.call()
    except BaseException as e:      # noqa: a thread reports whatever ended its call
      return False, f"{type(e).__name__}: {e}"
    try:
      return (True, "") if self.same(got, self.want) else (False, "wrong result")
    except BaseException as e:
      return False, f"comparison failed: {type(e).__name__}: {e}"


class Refused(Input):
  """A call that has to raise `exc` with exactly `text`, on the host, before any device work."""

  def __init__(self, name, call, exc, text):
    super().__init__(name, call, (exc, text))

  def run(self):
    exc, text = self.want
    try:
      self.call()
    except exc as e:
      return (True, "") if type(e).__name__ == exc.__name__ and str(e) == text else (False, f"{type(e).__name__}: {e}")
    except BaseException as e:
      return False, f"{type(e).__name__}: {e}"
    return False, "no exception"


def same_array(got, want):
  return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def same_arrays(got, want):
  return sorted(got) == sorted(want) and all(np.array_equal(np.asarray(got[k]).ravel(), np.asarray(want[k]).ravel()) for k in want)


def same_bytes(got, want):
  return bytes(got) == want


_fastcrackle = []
_fastcrackle_lock = threading.Lock()


def fastcrackle():
  """The pybind11 module, loaded once (tests/test_fastcrackle_module.py loads it the same way)."""
  with _fastcrackle_lock:
    if not _fastcrackle:
      from crackle_amd import build as ckl_build
      spec = importlib.util.spec_from_file_location("fastcrackle", ckl_build.fastcrackle_path())
      mod = importlib.util.module_from_spec(spec)
      spec.loader.exec_module(mod)
      _fastcrackle.append(mod)
    return _fastcrackle[0]


def _px(*vs):
  return tuple(int(v.shape[0]) * int(v.shape[1]) for v in vs)


def catalogue(chk, only=None):
  """{kind: [Input, ...]}: at least two inputs each.  chk is the checker (oracle.best()).  only: the kinds to build."""
  import crackle_amd
  from crackle_amd import FormatError, _lib, operations as ops
  V = volumes()
  loaded_before = _lib._lib is not None
  streams = {}

  def S(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in streams:
      streams[key] = chk.compress(V[name], **kw)
    return streams[key]

  def stats(name):
    return sk.stats_numpy(V[name])

  def label_of(name):
    st = {l: s[0] for l, s in stats(name).items() if l != 0}
    return max(st, key=lambda l: (st[l], -l))

  def decoded(editor):
    """The editor's stream decoded in the same job, with whatever else the editor returned."""
    def call():
      out = editor()
      if isinstance(out, tuple):
        return (crackle_amd.decompress(out[0]),) + tuple(out[1:])
      return crackle_amd.decompress(out)
    return call

  def same_edit(got, want):
    if isinstance(want, tuple):
      return same_array(got[0], want[0]) and tuple(got[1:]) == tuple(want[1:])
    return same_array(got, want)

  def compress_inputs(specs):
    return [Input(f"{n} {kw}", (lambda n=n, kw=kw: crackle_amd.compress(V[n], **kw)), S(n, **kw), same_bytes, _px(V[n]), V[n]) for n, kw in specs]

  K = {}

  def kind(name, make):
    if only is None or name in only:
      K[name] = make()

  kind("compress-u8", lambda: compress_inputs([("stripes", {}), ("a8", {}), ("halves8", {})]))
  kind("compress-u64", lambda: compress_inputs([("cells64", {}), ("a64", {}), ("halves64", {})]))
  kind("compress-u32-strips", lambda: compress_inputs([("dots", {}), ("halves", {})]))
  kind("compress-markov", lambda: compress_inputs([("s", dict(markov_model_order=6)), ("s", dict(markov_model_order=0)), ("t", dict(markov_model_order=3))]))
  kind("compress-pins", lambda: compress_inputs([("deep", dict(allow_pins=True)), ("a", dict(allow_pins=True))]))

  def decompress_inputs(specs):
    return [Input(f"{n} {kw}", (lambda n=n, kw=kw: crackle_amd.decompress(S(n, **kw))), V[n], same_array, _px(V[n])) for n, kw in specs if S(n, **kw)]
  kind("decompress-strips", lambda: decompress_inputs([("s", {}), ("t", {})]))
  kind("decompress-general", lambda: decompress_inputs([("a", {}), ("b", {})]))
  kind("decompress-markov", lambda: decompress_inputs([("a", dict(markov_model_order=5)), ("s", dict(markov_model_order=3))]))
  kind("decompress-label", lambda: [
    Input(n, (lambda n=n: crackle_amd.decompress(S(n), label=label_of(n))), V[n] == label_of(n), same_array, _px(V[n])) for n in ("a", "s") if S(n)])
  kind("decompress-range", lambda: [
    Input(f"{n} {z0}:{z1}", (lambda n=n, z0=z0, z1=z1: crackle_amd.decompress_range(S(n), z0, z1)), sk.like(V[n], V[n][:, :, z0:z1]), same_array, _px(V[n]))
    for n, z0, z1 in (("a", 1, 6), ("b", 2, 5)) if S(n)])

  def stats_inputs(call, want_of, same=None):
    return [Input(n, (lambda n=n: call(S(n))), want_of(stats(n)), same, _px(V[n])) for n in ("cells", "a") if S(n)]
  kind("voxel_counts", lambda: stats_inputs(crackle_amd.voxel_counts, lambda st: {l: s[0] for l, s in st.items()}))
  kind("centroids", lambda: stats_inputs(crackle_amd.centroids, lambda st: {l: s[1].astype(np.float64) / np.float64(s[0]) for l, s in st.items()},
                                           lambda got, want: same_arrays(got, want) and all(got[l].dtype == np.float64 for l in got)))
  kind("bounding_boxes", lambda: stats_inputs(lambda b: {l: [int(v) for v in box] for l, box in crackle_amd.bounding_boxes(b, no_slice_conversion=True).items()},
                                                lambda st: {l: list(s[2]) for l, s in st.items()}))
  kind("point_cloud", lambda: [
    Input(n, (lambda n=n: crackle_amd.point_cloud(S(n))), chk.point_cloud(S(n), 0, -1, None, True), same_arrays, _px(V[n])) for n in ("planes", "a")])
  kind("voxel_connectivity_graph", lambda: [
    Input(f"{n} {c}", (lambda n=n, c=c: crackle_amd.voxel_connectivity_graph(S(n), c)), chk.voxel_connectivity_graph(S(n), c), same_array, _px(V[n]))
    for n, c in (("a", 4), ("s", 6))])

  def contacts_want(n, aniso):
    cc2d = chk.connected_components(np.asfortranarray(V[n]))[0]
    return cn.areas(cn.contacts_numpy(V[n], components=cc2d), aniso)
  kind("contacts", lambda: [
    Input(f"{n} {an}", (lambda n=n, an=an: crackle_amd.contacts(S(n), anisotropy=an)), contacts_want(n, an), None, _px(V[n]))
    for n, an in (("a", (1.0, 1.0, 1.0)), ("s", (4.0, 4.0, 40.0)))])

  def other(n):
    return chk.compress(sk.other_of(V[n]))
  kind("overlaps", lambda: [
    Input(n, (lambda n=n, o=other(n): crackle_amd.overlaps(S(n), o)), on.overlaps_numpy(V[n], sk.other_of(V[n])), None, _px(V[n])) for n in ("a", "s") if S(n)])

  def components_want(n, c):
    ccl, mapping = cc3d_numpy.connected_components(V[n], c)
    return sk.like(V[n], ccl), mapping
  kind("connected_components", lambda: [
    Input(f"{n} {c}", decoded(lambda n=n, c=c: crackle_amd.connected_components(S(n), c, return_mapping=True)), components_want(n, c), same_edit, _px(V[n]))
    for n, c in (("a8", 26), ("s8", 6)) if S(n)])
  kind("dust", lambda: [
    Input(f"{n} {c}", decoded(lambda n=n, c=c: crackle_amd.dust(S(n), sk.DUST[0], connectivity=c, return_removed=True)),
          dust_numpy.dust(V[n], sk.DUST[0], connectivity=c), same_edit, _px(V[n]))
    for n, c in (("a", 26), ("noise", 6)) if S(n)])

  def filled_want(n, c):
    f = fill_holes_numpy.fill_holes(V[n], c)
    return f.volume, f.filled
  kind("fill_holes", lambda: [
    Input(f"{n} {c}", decoded(lambda n=n, c=c: crackle_amd.fill_holes(S(n), c, return_filled=True)), filled_want(n, c), same_edit, _px(V[n]))
    for n, c in (("a", 6), ("s", 26)) if S(n)])

  kind("recompress", lambda: [
    Input("a markov 5", lambda: crackle_amd.recompress(S("a", markov_model_order=5)), S("a", markov_model_order=5), same_bytes, _px(V["a"]), V["a"]),
    Input("b to markov 2", lambda: crackle_amd.recompress(S("b"), markov_model_order=2), S("b", markov_model_order=2), same_bytes, _px(V["b"]), V["b"]),
  ] if S("a", markov_model_order=5) and S("b") else None)
  kind("erode", lambda: [
    Input(f"{n} {c} {border}", (lambda n=n, c=c, border=border: crackle_amd.erode(S(n), c, erode_border=border)),
          chk.compress(sk.like(V[n], erode_numpy.erode(V[n], c, border))), same_bytes, _px(V[n]), sk.like(V[n], erode_numpy.erode(V[n], c, border)))
    for n, c, border in (("a", 6, True), ("s", 26, False)) if S(n)])
  kind("dilate", lambda: [
    Input(f"{n} {c}", (lambda n=n, c=c: crackle_amd.dilate(S(n), c)), chk.compress(sk.like(V[n], dilate_numpy.dilate(V[n], c))), same_bytes, _px(V[n]), sk.like(V[n], dilate_numpy.dilate(V[n], c)))
    for n, c in (("a", 26), ("s", 6)) if S(n)])
  kind("cutout", lambda: [
    Input(n, (lambda n=n: crackle_amd.cutout(S(n), sk.box_of(V[n].shape))), V[n][sk.box_of(V[n].shape)], same_array, _px(V[n])) for n in ("a", "b") if S(n)])

  def paste_input(n):
    box = sk.box_of(V[n].shape)
    data = sk.other_of(V[n])[box]
    return Input(n, decoded(lambda: crackle_amd.paste(S(n), box, data)), paste_volumes.edited(V[n], box, data), same_edit, _px(V[n]))
  kind("paste", lambda: [paste_input(n) for n in ("a", "s") if S(n)])

  def reencode_input(n, kw, order):
    return Input(f"{n} {kw} to {order}", (lambda: crackle_amd.reencode(S(n, **kw), order)), chk.reencode(S(n, **kw), order), same_bytes, _px(V[n]), V[n])
  kind("reencode", lambda: [reencode_input("a", {}, 3), reencode_input("s", dict(markov_model_order=5), 0)])
  kind("mode_pooling_2x2x1", lambda: [
    Input(n, (lambda n=n: ops._mode_pooling_slices(S(n))), [bytes(b) for b in chk.mode_pooling_2x2x1(S(n))], lambda got, want: [bytes(b) for b in got] == want, _px(V[n]))
    for n in ("a", "s")])
  kind("array_equal", lambda: [
    Input("a and a markov 2", lambda: crackle_amd.array_equal(S("a"), S("a", markov_model_order=2)), True, None, _px(V["a"])),
    Input("s and another", lambda o=other("s"): crackle_amd.array_equal(S("s"), o), False, None, _px(V["s"])),
  ] if S("a") and S("a", markov_model_order=2) and S("s") else None)

  def fc_compress(n, order):
    return Input(f"{n} markov {order}", (lambda: fastcrackle().compress(np.asfortranarray(V[n]), False, True, order, False, True, 0, 0)),
                 S(n, markov_model_order=order), same_bytes, _px(V[n]), V[n])
  kind("fastcrackle.compress", lambda: [fc_compress("a8", 0), fc_compress("s", 3)])
  kind("fastcrackle.decompress", lambda: [
    Input(f"{n} {kw}", (lambda n=n, kw=kw: fastcrackle().decompress(S(n, **kw), 0, -1, 0, None)), flat_1d(V[n]), same_array, _px(V[n]))
    for n, kw in (("a", {}), ("s", dict(markov_model_order=3))) if S(n, **kw)])

  def abi_error(entry, stream):
    """The C entry point itself, so that the text is the calling thread's ckl_last_error()."""
    import ctypes as C
    out, n = C.c_void_p(), C.c_uint64()
    rc = getattr(_lib.lib(), entry)(stream, len(stream), -1, 0, C.byref(out), C.byref(n))
    if rc != _lib.CKL_OK:
      raise RuntimeError(f"{rc}: {_lib.last_error()}")

  def header_error(nbytes):
    import ctypes as C
    info = _lib.HeaderInfo()
    rc = _lib.lib().ckl_header_info_from_bytes(b"crkl\x01" + bytes(nbytes - 5), nbytes, C.byref(info))
    if rc != _lib.CKL_OK:
      raise RuntimeError(f"{rc}: {_lib.last_error()}")

  signed = "Signed integer data types are not currently supported."
  kind("refused", lambda: [
    Refused("ten bytes", lambda: crackle_amd.decompress(b"crkl\x01" + bytes(5)), FormatError, "crackle: Input too small to be a valid stream. Bytes: 10"),
    Refused("signed to recompress", lambda: crackle_amd.recompress(rv.as_signed(S("a"))), TypeError, signed),
    Refused("signed to dust", lambda: crackle_amd.dust(rv.as_signed(S("a")), 10), TypeError, signed),
    Refused("reversed range to fastcrackle.contacts", lambda: fastcrackle().contacts(S("a"), 5, 2), RuntimeError, "crackle: Invalid range: 5 - 2"),
    Refused("ten bytes to fastcrackle", lambda: fastcrackle().decompress(b"crkl\x01" + bytes(5), 0, -1, 1, None), RuntimeError,
            "crackle: Input too small to be a valid stream. Bytes: 10"),
    Refused("signed to ckl_recompress", lambda: abi_error("ckl_recompress", rv.as_signed(S("a"))), RuntimeError, f"{_lib.CKL_ERR_ARG}: {signed}"),
    Refused("eleven bytes to the header", lambda: header_error(11), RuntimeError, f"{_lib.CKL_ERR_FORMAT}: crackle: Input too small to be a valid stream. Bytes: 11"),
    Refused("thirteen bytes to the header", lambda: header_error(13), RuntimeError, f"{_lib.CKL_ERR_FORMAT}: crackle: Input too small to be a valid stream. Bytes: 13"),
  ] if S("a") else None)
  kind("tiny-voxel_counts", lambda: [
    Input("tiny", lambda: crackle_amd.voxel_counts(S("tiny")), {l: s[0] for l, s in stats("tiny").items()}, None, _px(V["tiny"])) if S("tiny") else None] * 2)

  assert loaded_before or _lib._lib is None, "the catalogue's expectations must not come from the library under test"
  for name, inputs in K.items():
    assert len(inputs) >= 2, name
  return K


SCHEDULED = [
  "compress-u8", "compress-u64", "compress-u32-strips", "compress-markov", "compress-pins",
  "decompress-strips", "decompress-general", "decompress-markov", "decompress-label", "decompress-range",
  "voxel_counts", "centroids", "bounding_boxes", "point_cloud", "voxel_connectivity_graph", "contacts", "overlaps",
  "connected_components", "dust", "fill_holes", "recompress", "erode", "dilate", "cutout", "paste", "reencode",
  "mode_pooling_2x2x1", "array_equal", "fastcrackle.compress", "fastcrackle.decompress", "refused",
]
COLD = ["compress-u8", "decompress-strips", "voxel_counts", "fastcrackle.compress"]


# ---- the schedule -------------------------------------------------------------------------------------------------------

def schedule(n_kinds, threads=THREADS):
  """Rounds of `threads` jobs (kind index, first input) such that every unordered pair of kinds shares a round, and
  every kind shares one with itself, the two jobs starting on different inputs (they alternate, so they stay on
  different inputs).  First the rounds (k, k, k + 1, k + 1), then greedily the pairs that are left."""
  assert threads == 4 and n_kinds >= 4
  left = {(a, b) for a in range(n_kinds) for b in range(a, n_kinds)}
  rounds = []

  def add(jobs):
    rounds.append(jobs)
    for i in range(len(jobs)):
      for j in range(i + 1, len(jobs)):
        a, b = sorted((jobs[i][0], jobs[j][0]))
        if a != b or jobs[i][1] != jobs[j][1]:
          left.discard((a, b))

  for k in range(0, n_kinds, 2):
    k2 = k + 1 if k + 1 < n_kinds else 0
    add([(k, 0), (k, 1), (k2, 0), (k2, 1)])
  while left:
    a, b = min(left)
    chosen = [a, b]
    while len(chosen) < threads:
      gain = lambda c: sum((min(c, x), max(c, x)) in left for x in chosen)
      chosen.append(max((c for c in range(n_kinds) if c not in chosen), key=lambda c: (gain(c), -c)))
    add([(k, 0) for k in chosen])
  return rounds


def pairs_of(rounds):
  """The unordered pairs (a, b), a <= b, the rounds put side by side; (a, a) only for jobs that start on different inputs."""
  out = set()
  for jobs in rounds:
    for i in range(len(jobs)):
      for j in range(i + 1, len(jobs)):
        a, b = sorted((jobs[i][0], jobs[j][0]))
        if a != b or jobs[i][1] != jobs[j][1]:
          out.add((a, b))
  return out


# ---- the child ---------------------------------------------------------------------------------------------------------------

def _checker():
  from oracle import oracle
  return oracle.best()


def _run_job(records, where, kind, inputs, first, calls):
  for i in range(calls):
    k = (first + i) % len(inputs)
    t0 = time.perf_counter()
    ok, text = inputs[k].run()
    records.append(list(where) + [kind, inputs[k].name, t0, time.perf_counter(), ok, text])


def _threads(targets):
  ts = [threading.Thread(target=t) for t in targets]
  for t in ts:
    t.start()
  for t in ts:
    t.join()


def scenario_cold(threads):
  """The process's first library calls, `threads` of them at the same time."""
  from crackle_amd import _lib
  K = catalogue(_checker(), only=COLD)
  fastcrackle()      # loaded, not called
  assert _lib._lib is None
  names = COLD[:threads] if threads > 1 else COLD
  barrier = threading.Barrier(threads)
  records = [[] for _ in names]

  def worker(slot):
    barrier.wait()
    _run_job(records[slot], (0, slot), names[slot], K[names[slot]], 0, 1 + CALLS_PER_ROUND * len(K[names[slot]]))
  if threads > 1:
    _threads([lambda s=s: worker(s) for s in range(len(names))])
  else:
    for s in range(len(names)):
      worker(s)
  return [r for rec in records for r in rec]


def scenario_pairs(threads):
  """The schedule, one barrier per round; with one thread the same jobs one after the other."""
  K = catalogue(_checker(), only=SCHEDULED)
  rounds = schedule(len(SCHEDULED))
  records = [[] for _ in range(THREADS)]
  barrier = threading.Barrier(threads)

  def worker(slot):
    for r, jobs in enumerate(rounds):
      barrier.wait()
      for s in ([slot] if threads > 1 else range(THREADS)):
        kind, first = SCHEDULED[jobs[s][0]], jobs[s][1]
        _run_job(records[s], (r, s), kind, K[kind], first, CALLS_PER_ROUND)
  if threads > 1:
    _threads([lambda s=s: worker(s) for s in range(THREADS)])
  else:
    worker(0)
  return [r for rec in records for r in rec]


def scenario_sessions(threads, sessions=200):
  """`threads` threads create and destroy `sessions` decode sessions each while one more encodes and decodes."""
  import crackle_amd
  chk = _checker()
  K = catalogue(chk, only=["tiny-voxel_counts"])
  V = volumes()
  big, big_stream = V["cells"], chk.compress(V["cells"])
  done = threading.Event()
  records = [[] for _ in range(threads + 1)]
  barrier = threading.Barrier(threads + 1 if threads > 1 else 1)
  encode = Input("cells", lambda: crackle_amd.compress(big), big_stream, same_bytes)
  decode = Input("cells", lambda: crackle_amd.decompress(big_stream), big, same_array)

  def short(slot):
    barrier.wait()
    _run_job(records[slot], (0, slot), "tiny-voxel_counts", K["tiny-voxel_counts"], 0, sessions)

  def long():
    barrier.wait()
    n = 0
    while n < 4 or not done.is_set():
      _run_job(records[threads], (0, threads), "compress", [encode], 0, 1)
      _run_job(records[threads], (0, threads), "decompress", [decode], 0, 1)
      n += 1

  if threads > 1:
    ts = [threading.Thread(target=short, args=(s,)) for s in range(threads)]
    tl = threading.Thread(target=long)
    for t in ts + [tl]:
      t.start()
    for t in ts:
      t.join()
    done.set()
    tl.join()
  else:
    short(0)
    done.set()
    long()
  return [r for rec in records for r in rec]


SCENARIOS = {"cold": scenario_cold, "pairs": scenario_pairs, "sessions": scenario_sessions}


def main(argv):
  name, threads = argv[0], int(argv[1])
  t0 = time.perf_counter()
  records = SCENARIOS[name](threads)
  from crackle_amd import _lib
  doc = {"scenario": name, "threads": threads, "seconds": time.perf_counter() - t0, "library": _lib.LIB_PATH, "records": records}
  sys.stdout.write(json.dumps(doc) + "\n")
  sys.stdout.flush()
  return 0


if __name__ == "__main__":
  sys.exit(main(sys.argv[1:]))
