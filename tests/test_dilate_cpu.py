"""dilate without a GPU: the restatement (tests/dilate_numpy.py) pinned by a literal triple loop, by erosion of the
complement on one-label volumes and by the literal answers of the hand-built neighbourhoods; what the volumes of
tests/dilate_volumes.py hold (none of them is vacuous); the public surface, the errors decided on the host (through
Python and through the C entry), the arguments of opening and closing, and the pass-through of empty volumes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import crackle_amd
import dilate_numpy
import dilate_volumes as volumes
import erode_numpy
from crackle_amd import _lib, operations
from crackle_amd.operations import dilate      # (the feature under test: without it nothing here runs)
from recompress_volumes import as_signed, interior_x_pairs, linear_pairs, permissible
from util import golden

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CONNECTIVITIES = volumes.CONNECTIVITIES


def _restate(vol, conn):
  out = dilate_numpy.dilate(vol, conn)
  assert out.dtype == vol.dtype and out.shape == vol.shape
  assert out.flags.f_contiguous == vol.flags.f_contiguous and out.flags.c_contiguous == vol.flags.c_contiguous
  assert np.array_equal(out[vol != 0], vol[vol != 0])      # a label is never overwritten
  return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _triple_loop(vol, conn):
  sx, sy, sz = vol.shape
  out = vol.copy()
  for x in range(sx):
    for y in range(sy):
      for z in range(sz):
        if vol[x, y, z] != 0:
          continue
        seen = {}
        for dx, dy, dz in erode_numpy.offsets(conn):
          a, b, c = x + dx, y + dy, z + dz
          if 0 <= a < sx and 0 <= b < sy and 0 <= c < sz and vol[a, b, c] != 0:
            seen[int(vol[a, b, c])] = seen.get(int(vol[a, b, c]), 0) + 1
        if seen:
          most = max(seen.values())
          out[x, y, z] = min(label for label, n in seen.items() if n == most)
  return out


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_restatement_is_the_literal_triple_loop(conn):
  rng = np.random.default_rng(1234 + conn)
  for labels, share in ((3, 0.5), (6, 0.7), (2, 0.2)):
    vol = np.asfortranarray(rng.integers(1, labels + 1, (9, 7, 5)).astype(np.uint16))
    vol[rng.random(vol.shape) < share] = 0
    assert np.array_equal(_restate(vol, conn), _triple_loop(vol, conn))
  wide = np.asfortranarray(rng.choice(np.array([0, 0, 3, volumes.HIGH_1, volumes.HIGH_2, volumes.TOP], np.uint64), (9, 7, 5)))
  assert np.array_equal(_restate(wide, conn), _triple_loop(wide, conn))


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_one_label_dilation_is_erosion_of_the_complement(conn):
  rng = np.random.default_rng(99)
  for shape in ((9, 7, 5), (33, 6, 4), (1, 6, 5), (12, 1, 1)):
    vol = np.asfortranarray((rng.random(shape) < 0.3).astype(np.uint8))
    want = 1 - erode_numpy.erode((1 - vol).astype(np.uint8), conn, erode_border=False)
    assert np.array_equal(_restate(vol, conn), want)


@pytest.mark.parametrize("offset", volumes.NEIGHBOURS, ids=lambda o: "%+d%+d%+d" % o)
def test_restatement_which_neighbour_counts(offset):
  vol = volumes.probe(offset)
  assert vol.shape == (9, 9, 9) and int(np.count_nonzero(vol)) == 1
  literal = {1: (True, True, True), 2: (False, True, True), 3: (False, False, True)}[sum(map(abs, offset))]
  for conn, gained in zip(CONNECTIVITIES, literal):
    assert volumes.probe_centre_gained(offset, conn) == gained
    out = _restate(vol, conn)
    assert (out[volumes.PROBE_CENTRE] == 3) == gained and out[volumes.PROBE_CENTRE] in (0, 3)
    assert int(np.count_nonzero(out)) == 1 + conn      # the voxel and its whole element, well inside the volume


@pytest.mark.parametrize("name,dtype,entries,answers", volumes.MODE_CASES, ids=[c[0] for c in volumes.MODE_CASES])
def test_restatement_mode_and_tie_rule(name, dtype, entries, answers):
  vol = volumes.mode_case(dtype, entries)
  assert vol[volumes.MODE_CENTRE] == 0 and int(np.count_nonzero(vol)) == len(entries)
  for conn, answer in zip(CONNECTIVITIES, answers):
    assert int(_restate(vol, conn)[volumes.MODE_CENTRE]) == answer
  if name == "face-edge-corner":
    assert len(set(answers)) == 3


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
SEAMS_MEASURED = {      # the shares measured for the issue, in per cent (lowest, highest over the two shapes)
  6: dict(contested=(38, 38), tied=(30, 31), not_smallest=(3.7, 4.0), not_largest=(34, 34), still_zero=(17, 19)),
  18: dict(contested=(60, 62), tied=(15, 16), not_smallest=(22, 24), not_largest=(39, 39), still_zero=(14, 16)),
  26: dict(contested=(62, 64), tied=(12, 12), not_smallest=(26, 28), not_largest=(38, 38), still_zero=(13, 15)),
}
SEAMS_FLOORS = dict(contested=0.20, tied=0.05, not_smallest=0.02, not_largest=0.20, still_zero=0.05)


@pytest.mark.parametrize("shape,order", volumes.GENERATED, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_seams_are_contested(shape, order):
  vol = volumes.seams(shape, order)
  assert vol.flags.c_contiguous == (order == "C") and vol.flags.f_contiguous == (order == "F")
  lab = volumes.voronoi(shape, "F")
  assert np.array_equal(vol[vol != 0], lab[np.asarray(vol) != 0]) and (vol == 0).sum() > (lab == 0).sum()
  for conn in CONNECTIVITIES:
    st = volumes.stats(vol, conn)
    assert st["gained"] > 1000
    for key, floor in SEAMS_FLOORS.items():
      assert st[key] >= floor, (shape, conn, key, st)
      low, high = SEAMS_MEASURED[conn][key]
      assert low - 1.5 <= 100 * st[key] <= high + 1.5, (shape, conn, key, st)      # what the issue measured, to its rounding


def test_generated_volumes_are_not_vacuous():
  vols = [("dtype-" + np.dtype(dt).name, volumes.for_dtype(dt)) for dt in (np.uint8, np.uint16, np.uint32, np.uint64)]
  vols += [("many-words", volumes.seams(volumes.MANY_WORDS)), ("strip_path", volumes.strip_path()), ("run_pipeline", volumes.run_pipeline())]
  assert int(volumes.for_dtype(np.uint64).max()) > 1 << 40
  for name, vol in vols:
    zeros = int((vol == 0).sum())
    assert 0.05 * vol.size <= zeros <= 0.6 * vol.size, (name, zeros / vol.size)
    for conn in CONNECTIVITIES:
      out = _restate(vol, conn)
      gained = zeros - int((out == 0).sum())
      assert gained >= 0.02 * vol.size and np.unique(out[(vol == 0) & (out != 0)]).size >= 3, (name, conn, gained)
  # like the originals they are made for: one takes the encoder's strip kernels by its size, the other has rows wider than a strip
  assert volumes.strip_path().shape == (320, 288, 5) and volumes.run_pipeline().shape == (32800, 3, 2)
  assert -(-volumes.MANY_WORDS[0] // 32) * volumes.MANY_WORDS[1] == 400
  assert not (volumes.no_background() == 0).any()
  for conn in CONNECTIVITIES:
    assert np.array_equal(_restate(volumes.no_background((30, 20, 4)), conn), volumes.no_background((30, 20, 4)))
    assert int(np.count_nonzero(_restate(volumes.single_voxel(), conn))) == 1 + conn
    assert not _restate(np.zeros((37, 6, 5), np.uint16, order="F"), conn).any()


def test_edge_volumes_are_what_they_say():
  for sx in volumes.EDGE_SX:
    shape = (sx, 4, 3)
    cols = volumes.edges(shape, "columns")
    for c in volumes.EDGE_COLUMNS + (sx - 1,):
      if c < sx:
        assert not cols[c].any()
    if sx >= 32:
      assert cols[1, 0, 0] != 0 and cols[30, 0, 0] == cols[1, 0, 0] and cols[1, 0, 0] != cols[1, 1, 0]
    if sx >= 64:
      assert cols[33, 0, 0] not in (0, cols[30, 0, 0]) and cols[62, 0, 0] == cols[33, 0, 0]
    tail = volumes.edges(shape, "tail-label")
    head = volumes.edges(shape, "tail-background")
    if sx >= 4:
      # a neighbour taken across the row's end would gain these pixels; no element does
      assert tail[sx - 1, 0, 0] != 0 and tail[0, 1, 0] == 0 and head[0, 1, 0] != 0 and head[sx - 1, 0, 0] == 0
      for conn in CONNECTIVITIES:
        assert not _restate(tail, conn)[0].any() and not _restate(head, conn)[sx - 1].any()
        assert _restate(tail, conn)[1].all() and _restate(head, conn)[sx - 2].all()
    full = volumes.edges(shape, "all-gained")
    ones = volumes.edges(shape, "one-pixel-labels")
    assert not full[:, 1::2].any() and full[:, 0::2].all() and not ones[:, 1::2].any()
    assert np.array_equal(ones[:, 0, 0], np.arange(1, sx + 1)) and np.array_equal(ones[:, 2, 0], np.arange(3, sx + 3))
    for conn in CONNECTIVITIES:
      assert _restate(full, conn).all() and _restate(ones, conn).all()
    if sx >= 3:
      assert _restate(ones, 6)[1, 1, 0] == 2 and _restate(ones, 18)[1, 1, 0] == 2      # 2 above and 4 below; 1 2 3 above, 3 4 5 below, 2 and 4 in the next slice: ties


def test_format_cases_change_and_keep_the_crack_format():
  flips, stays = (volumes.rows(p) for _, p in volumes.FORMAT_CASES)
  for vol in (flips, stays):
    assert vol.shape == (1, 36, 4) and interior_x_pairs(vol) == 0 and permissible(vol)      # all pairs are wrap-arounds
  for conn in CONNECTIVITIES:
    out = _restate(flips, conn)
    assert not permissible(out) and linear_pairs(out) >= out.size // 2 and interior_x_pairs(out) == 0
    out = _restate(stays, conn)
    assert permissible(out) and not np.array_equal(out, stays)


def test_pit_is_closed():
  vol = volumes.pit()
  block = vol.copy()
  block[10, 5, 6] = block[8, 5, 4] = 6
  for conn in CONNECTIVITIES:
    for border in (True, False):
      want = block.copy()
      if conn == 6:
        want[10, 5, 6] = 0      # the voxel above the pit has no face neighbour in the block: it is not gained, and the pit opens again
      assert np.array_equal(erode_numpy.erode(_restate(vol, conn), conn, border), want)
    opened = _restate(erode_numpy.erode(vol, conn, True), conn)
    assert opened[8, 5, 4] == 0 and opened[10, 5, 6] == 0 and opened.any()


# ---- the surface -------------------------------------------------------------------------------------------------------
def test_surface():
  assert crackle_amd.dilate is operations.dilate and {"dilate", "opening", "closing"} <= set(crackle_amd.__all__)
  sig = inspect.signature(crackle_amd.dilate)
  assert list(sig.parameters) == ["binary", "connectivity", "markov_model_order", "device"]
  assert [p.default for p in sig.parameters.values()][1:] == [26, None, 0]
  for fn in (crackle_amd.opening, crackle_amd.closing):
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["binary", "connectivity", "erode_border", "markov_model_order", "device"]
    assert [p.default for p in sig.parameters.values()][1:] == [26, True, None, 0]
    for words in ("two device calls", "crossing the host", "fusing them is not done"):
      assert words in " ".join(fn.__doc__.split())
  sig = inspect.signature(crackle_amd.CrackleArray.dilate)
  assert list(sig.parameters) == ["self", "connectivity"] and sig.parameters["connectivity"].default == 26
  for name in ("opening", "closing"):
    sig = inspect.signature(getattr(crackle_amd.CrackleArray, name))
    assert list(sig.parameters) == ["self", "connectivity", "erode_border"]
  text = open(os.path.join(ROOT, "include", "crackle_amd.h")).read()
  assert re.search(r"\bint\s+ckl_dilate\s*\(\s*const uint8_t\*\s*buf,\s*uint64_t n,\s*int connectivity,\s*int flags,\s*int markov_model_order,\s*"
                   r"int device,\s*uint8_t\*\*\s*out,\s*uint64_t\*\s*out_len\s*\)", text)
  assert _lib.EXPORTS["ckl_dilate"] == (C.c_int, [
    C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)])
  assert hasattr(C.CDLL(_lib.LIB_PATH), "ckl_dilate")
  assert _lib.lib().ckl_abi_version() == 1      # an entry was added, none changed
  doc = " ".join(operations.dilate.__doc__.split())
  for words in ("occurs most often", "the smallest", "unsigned 64-bit", "Equality is by label", "One iteration per call", "byte for byte",
                "not checked against fastmorph", "Not done", "background_only=False"):
    assert words in doc, words


def test_errors_need_no_device():
  binary = golden()["c0_voronoi_u8"]
  for conn in (4, 8, 0, 27, -6):
    for call in (lambda: crackle_amd.dilate(binary, connectivity=conn), lambda: crackle_amd.CrackleArray(binary).dilate(connectivity=conn),
                 lambda: crackle_amd.opening(binary, connectivity=conn), lambda: crackle_amd.closing(binary, connectivity=conn),
                 lambda: crackle_amd.CrackleArray(binary).opening(conn), lambda: crackle_amd.CrackleArray(binary).closing(conn)):
      with pytest.raises(ValueError, match="connectivity must be 6, 18 or 26"):
        call()
  for fn in (crackle_amd.dilate, crackle_amd.opening, crackle_amd.closing):
    with pytest.raises(ValueError, match=fn.__name__ + ": markov_model_order must not be negative"):
      fn(binary, markov_model_order=-1)
  signed = as_signed(binary)
  assert crackle_amd.header(signed).signed
  for fn in (crackle_amd.dilate, crackle_amd.opening, crackle_amd.closing):
    with pytest.raises(TypeError, match="Signed integer data types are not currently supported"):
      fn(signed)
  with pytest.raises(TypeError):
    crackle_amd.CrackleArray(signed).dilate()
  # the ABI refuses the same on its own; flags must be 0
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  for buf, conn, flags, order in ((binary, 4, 0, -1), (binary, 0, 0, -1), (signed, 26, 0, -1), (binary, 26, 1, -1), (binary, 26, 2, -1), (binary, 6, 0, 16)):
    assert L.ckl_dilate(buf, len(buf), conn, flags, order, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG
    assert out.value is None and n.value == 0
  assert b"connectivity must be 6, 18 or 26" in (L.ckl_dilate(binary, len(binary), 5, 0, -1, 0, C.byref(out), C.byref(n)), L.ckl_last_error())[1]
  assert b"flags must be 0" in (L.ckl_dilate(binary, len(binary), 6, 4, -1, 0, C.byref(out), C.byref(n)), L.ckl_last_error())[1]
  assert L.ckl_dilate(binary, len(binary), 6, 0, -1, 0, None, C.byref(n)) == _lib.CKL_ERR_ARG
  assert L.ckl_dilate(binary[:10], 10, 6, 0, -1, 0, C.byref(out), C.byref(n)) != _lib.CKL_OK


def test_opening_and_closing_hand_their_arguments_on(monkeypatch):
  calls = []

  def fake_erode(binary, connectivity=26, erode_border=True, markov_model_order=None, device=0):
    calls.append(("erode", binary, connectivity, erode_border, markov_model_order, device))
    return binary + b"e"

  def fake_dilate(binary, connectivity=26, markov_model_order=None, device=0):
    calls.append(("dilate", binary, connectivity, markov_model_order, device))
    return binary + b"d"

  monkeypatch.setattr(operations, "erode", fake_erode)
  monkeypatch.setattr(operations, "dilate", fake_dilate)
  assert operations.opening(b"s", 18, False, 3, 2) == b"sed"
  assert calls == [("erode", b"s", 18, False, None, 2), ("dilate", b"se", 18, 3, 2)]      # the first step keeps the stream's order
  del calls[:]
  assert operations.closing(b"s", connectivity=6, markov_model_order=0) == b"sde"
  assert calls == [("dilate", b"s", 6, None, 0), ("erode", b"sd", 6, True, 0, 0)]
  del calls[:]
  arr = crackle_amd.CrackleArray(golden()["c0_voronoi_u8"])
  assert arr.opening(6, False).binary == arr.binary + b"ed" and arr.closing().binary == arr.binary + b"de"
  assert [c[0] for c in calls] == ["erode", "dilate", "dilate", "erode"] and calls[0][2:4] == (6, False) and calls[3][2:4] == (26, True)


@pytest.mark.parametrize("shape", [(0, 0, 0), (5, 0, 3), (4, 4, 0)])
def test_empty_volumes_come_back_as_recompress_returns_them(checker, shape):
  arr = np.zeros(shape, np.uint16, order="F")
  b = checker.compress(arr, markov_model_order=3)
  want = crackle_amd.recompress(b)
  assert want == b
  for conn in CONNECTIVITIES:
    assert crackle_amd.dilate(b, connectivity=conn) == want
    assert crackle_amd.opening(b, connectivity=conn) == want and crackle_amd.closing(b, connectivity=conn, erode_border=False) == want
  assert crackle_amd.dilate(b, markov_model_order=0) == crackle_amd.recompress(b, markov_model_order=0) == checker.compress(arr)
  assert crackle_amd.CrackleArray(b).dilate(18).binary == want
  # the C entry answers from the host alone too
  out, n = C.c_void_p(), C.c_uint64()
  L = _lib.lib()
  assert L.ckl_dilate(b, len(b), 6, 0, -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_OK
  try:
    assert C.string_at(out.value, n.value) == want
  finally:
    L.ckl_free(out)
