"""One decode session asked for everything, in every order (include/crackle_amd.h: ckl_decoder_run with and without
a label, _cutout, _check, _label_stats, _contacts, _vcg at connectivity 4 and 6, _crack_planes).  The session struct
(crackle_amd/csrc/ckl_decoder.hpp) carries path decisions, error words, the stage table, buffers that exist only
after some kind of call and buffers typed by the last call from one call to the next; every other test opens a
session for one kind of call.  Here tests/decode_session.py's schedule runs every ordered pair of the nine
operations back to back on one session, and every result is compared exactly with an expectation that was computed
before the session existed:

  P, L, C   numpy on the array the stream was made from
  K         zeros
  S         numpy: counts from np.unique, integer coordinate sums (z from the volume's origin), boxes from argwhere,
            the quirk of a pin stream's unlisted background as ckl_decoder_label_stats documents it
  T         contacts_numpy
  V4, V6    a fresh session's single call on the same stream (tests/test_gpu_parity.py pins that call to the reference)
  X         a fresh session's single call.  This leg compares the session with a fresh session, not with an
            independent restatement of the crack decoder; it also asserts that neither plane is all zero.

The session kinds are the smallest shapes that put a session on each path (asserted from ckl_decoder_stage_timing
after the first P, with the names of tests/test_gpu_paths.py); the hand-overs (strip table overflow, CKL_REC_CAP,
CKL_RESOLVE_CAP) are forced as in tests/test_gpu_strips.py and then asked for everything else.  The natural
resolve_cap -> resolve_cap_max retry needs more slices than the chip has CUs at 1024 x 1024: out of scope here."""
import functools
import itertools

import numpy as np
import pytest

import contacts_numpy as cn
import crackle_amd
import decode_session as ds
import golden_cases
from crackle_amd import codec, synth
from decode_session import DecodeSession
from test_gpu_paths import FAST_FLAT, FAST_PINS, SLOW, STRIP_V1
from util import golden, label_format

pytestmark = pytest.mark.gpu

EVERY_PAIR = set(itertools.product(ds.OPS, repeat=2))
# what the general run pipeline may report (ckl_decode.hip: decoder_run, general_pipeline and its resolve stages)
GENERAL = SLOW | {"memset", "k_run_union_seams", "k_run_count", "k_run_rank", "k_label_map", "k_run_labels", "k_check"}
# the strip path behind the rasterising front end, rows that are not a power of two of plane words
RASTER_STRIP_V1 = ["k_decode_cracks"] + STRIP_V1[1:]
SLICE_BAD_CRC = 0x10      # CKL_SLICE_BAD_CRC


# ---- the expectations ------------------------------------------------------------------------------------------

def _box(shape):
  """Odd x-offset, odd width, not a whole plane."""
  sx, sy, _ = shape
  box = (3, 40, 5, sy - 6)
  assert box[0] % 2 == 1 and (box[1] - box[0]) % 2 == 1 and box[1] < sx and box[3] - box[2] > 0
  return box


def stats_numpy(vol, binary, z0, z1):
  """(labels, counts, sums, boxes) of slices [z0, z1) as ckl_decoder_label_stats documents them: one row per label of
  the stream's table (a pin stream's background colour included), ascending; a label absent from the range has count
  0 and the reference's initial box (minima 0xFFFFFFFF, maxima 0); z from the volume's origin.  The unlisted
  background of a pin stream has minima 0, and an all-zero box when it is absent."""
  head = crackle_amd.header(binary)
  n, off = codec._label_section(binary, head)
  table = np.frombuffer(binary, dtype=head.stored_dtype, offset=off, count=n).astype(np.uint64)
  bg = None
  if head.label_format != crackle_amd.LabelFormat.FLAT:
    at = head.header_bytes + head.grid_index_bytes
    bg = int.from_bytes(binary[at:at + head.stored_data_width], "little")
    if bg in set(table.tolist()):
      bg = None      # listed: nothing special
    else:
      table = np.append(table, np.uint64(bg))
  table = np.unique(table)
  part = np.ascontiguousarray(vol[:, :, z0:z1]).astype(np.uint64)
  present, inverse, count = np.unique(part.reshape(-1), return_inverse=True, return_counts=True)
  row = np.searchsorted(table, present)
  assert (table[row] == present).all(), "the volume holds a label the stream's table lacks"
  where = np.argwhere(np.ones(part.shape, bool)).astype(np.int64)      # (x, y, z) of every voxel, in part's C order
  where[:, 2] += z0
  inverse = inverse.reshape(-1)
  counts = np.zeros((len(table),), np.uint64)
  sums = np.zeros((len(table), 3), np.int64)
  lo = np.full((len(table), 3), 0xFFFFFFFF, np.int64)
  hi = np.zeros((len(table), 3), np.int64)
  counts[row] = count.astype(np.uint64)
  np.add.at(sums, row[inverse], where)
  np.minimum.at(lo, row[inverse], where)
  np.maximum.at(hi, row[inverse], where)
  boxes = np.concatenate([lo, hi], axis=1).astype(np.uint32)
  if bg is not None:
    i = int(np.searchsorted(table, np.uint64(bg)))
    boxes[i, :3] = 0
    if counts[i] == 0:
      boxes[i, 3:] = 0
  return table, counts, sums.astype(np.uint64), boxes


def contacts_arrays(vol, z0, z1):
  """contacts_numpy as the two arrays the session returns: pairs ascending by (a, b), faces per axis."""
  faces = cn.contacts_numpy(vol, z0, z1)
  keys = sorted(faces)
  return (np.array(keys, np.uint64).reshape(-1, 2), np.array([faces[k] for k in keys], np.uint64).reshape(-1, 3))


class Case:
  """A stream, the range of a session over it, and what every operation must return there."""

  def __init__(self, vol, binary, z0=0, z1=None):
    self.vol, self.binary = vol, binary
    self.z0, self.z1 = z0, vol.shape[2] if z1 is None else z1
    self.label = int(vol[vol.shape[0] // 2, vol.shape[1] // 2, self.z0])
    self.box = _box(vol.shape)
    self.want = self._expectations()

  def _expectations(self):
    vol, z0, z1 = self.vol, self.z0, self.z1
    x0, x1, y0, y1 = self.box
    part = vol[:, :, z0:z1]
    want = {
      "P": part, "L": part == self.label, "C": vol[x0:x1, y0:y1, z0:z1],
      "K": np.zeros((z1 - z0,), np.uint32),
      "S": stats_numpy(vol, self.binary, z0, z1),
      "T": contacts_arrays(vol, z0, z1),
    }
    assert want["L"].any() and not want["L"].all()
    # one fresh session per call: nothing of one call is there for the next
    for op in ("V4", "V6", "X"):
      with DecodeSession(self.binary, z0, z1) as fresh:
        want[op] = call(fresh, op, self)
    assert want["X"][0].any() and want["X"][1].any(), "a crack plane is all zero"
    assert want["V4"].any() and not np.array_equal(want["V4"], want["V6"])
    return want


def call(sess, op, case):
  if op == "P":
    return sess.run()
  if op == "L":
    return sess.run(label=case.label)
  if op == "C":
    return sess.cutout(case.box)
  if op == "K":
    return sess.check()
  if op == "S":
    return sess.label_stats()
  if op == "T":
    return sess.contacts()
  if op in ("V4", "V6"):
    return sess.vcg(int(op[1]))
  assert op == "X"
  return sess.crack_planes()


def _same(got, want):
  if isinstance(want, tuple):
    return isinstance(got, tuple) and len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
  return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _where(got, want):
  """A few words on a mismatch, for the assertion's message."""
  if isinstance(want, tuple):
    return [i for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
  if got.shape != want.shape or got.dtype != want.dtype:
    return (got.shape, got.dtype, want.shape, want.dtype)
  return np.argwhere(got != want)[:4].tolist()


def drive(sess, sequence, case):
  """Every call of the sequence on the session, each compared with the case's expectation; returns the operations
  that ran and the stage names behind every P, by position."""
  ran, stages, prev = [], {}, None
  for i, op in enumerate(sequence):
    got = call(sess, op, case)
    want = case.want[op]
    assert _same(got, want), f"{op} behind {prev} (call {i} of the schedule) differs: {_where(got, want)}"
    if op == "P":
      stages[i] = [n for n in sess.stages() if n != "memset"]
    ran.append(op)
    prev = op
  return ran, stages


# ---- the session kinds -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _voronoi_case(shape, dtype, order, z0, z1, **opts):
  offset = (1 << 40) if np.dtype(dtype) == np.uint64 else 0
  vol = synth.as_numpy_f(synth.voronoi_labels(shape, dtype, seed=31, cell=(8, 8, 3), offset=offset))
  vol = np.ascontiguousarray(vol) if order == "C" else np.asfortranarray(vol)
  binary = bytes(crackle_amd.compress(vol, **opts))
  want_format = 2 if opts.get("allow_pins") else 0
  assert label_format(binary) == want_format, "the stream does not have the label format the case is about"
  assert bool(crackle_amd.header(binary).fortran_order) == (order == "F")
  return Case(vol, binary, z0, z1)


def _is_general(names):
  return SLOW <= set(names) <= GENERAL


PINS = dict(allow_pins=True, markov_model_order=3)
# id: (shape, dtype, order, z0, z1, encoder options), the stages of a P
KINDS = {
  "a-flat-strips": (((128, 64, 9), np.uint32, "F", 0, None), {}, FAST_FLAT),
  "b-pin-strips": (((128, 64, 9), np.uint32, "F", 0, None), PINS, FAST_PINS),
  "c-general-C-order": (((96, 80, 6), np.uint8, "C", 0, None), {}, None),
  "d-general-slow-paint": (((97, 61, 7), np.uint16, "F", 0, None), {}, None),
  "e-u64-strips": (((64, 48, 5), np.uint64, "F", 0, None), {}, STRIP_V1),
  "f-flat-strips-range": (((128, 64, 9), np.uint32, "F", 2, 7), {}, FAST_FLAT),
  "f-pin-strips-range": (((128, 64, 9), np.uint32, "F", 2, 7), PINS, FAST_PINS),
  # the pin stream's background colour is not in its unique list and occurs in slices 0 .. 3 only: over [4, 9) its row
  # of the statistics is the all-zero box with count 0
  "f-pin-strips-range-without-background": (((128, 64, 9), np.uint32, "F", 4, 9), PINS, FAST_PINS),
}


def _assert_path(stages, strip_names, what):
  """Every P of the sequence on the path the case is about: the strip kernels named (a strip session that does not
  hand over must stay on them whatever was called in between), or the general pipeline."""
  assert stages, "the sequence holds no P"
  for i, names in sorted(stages.items()):
    if strip_names is None:
      assert _is_general(names), f"{what}: P at call {i} decoded by {names}"
    else:
      assert names == strip_names, f"{what}: P at call {i} decoded by {names}"


@pytest.mark.parametrize("first", ["P", "T"])
@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
def test_every_ordered_pair_on_one_session(kind, first):
  """The whole circuit, once with a P as the session's first call (the path is asserted before anything else ran) and
  once with contacts first, which builds the run tables and the label table before any paint."""
  args, opts, strip_names = KINDS[kind]
  case = _voronoi_case(*args, **opts)
  if kind.startswith("d-"):
    assert case.vol.shape[0] % 4 != 0      # k_paint_runs<OUT, false>
  if kind.endswith("without-background"):
    _, counts, _, boxes = case.want["S"]
    assert int(((counts == 0) & (boxes == 0).all(axis=1)).sum()) == 1 and int((counts == 0).sum()) > 1
  sequence = ds.schedule([first] + [o for o in ds.OPS if o != first])
  assert sequence[0] == first
  with DecodeSession(case.binary, case.z0, case.z1) as sess:
    ran, stages = drive(sess, sequence, case)
  assert ds.pairs_of(ran) == EVERY_PAIR and len(ran) == 82
  _assert_path(stages, strip_names, kind)


def test_a_session_on_a_stream_in_device_memory():
  """(g) ckl_decoder_create_device: every operation once behind P and once in front of it."""
  import torch
  args, opts, strip_names = KINDS["a-flat-strips"]
  case = _voronoi_case(*args, **opts)
  stream = torch.from_numpy(np.frombuffer(case.binary, np.uint8).copy()).to("cuda")
  sequence = ds.around("P", ds.OPS)
  with DecodeSession(case.binary, case.z0, case.z1, device_stream=stream) as sess:
    ran, stages = drive(sess, sequence, case)
  others = [o for o in ds.OPS if o != "P"]
  assert ds.pairs_of(ran) == {("P", o) for o in others} | {(o, "P") for o in others}
  _assert_path(stages, strip_names, "device stream")
  assert stream.cpu().numpy().tobytes() == case.binary      # the caller's stream is read in place, never written


# ---- the hand-overs ------------------------------------------------------------------------------------------------

FIRST = ["P", "L", "V6", "C", "S", "X"]
PAINTS = ("P", "L", "V6")      # the calls that ask for Goal::PAINT: only they run the strip path


@functools.lru_cache(maxsize=None)
def _noise_case():
  """The volume of test_strip_overflow_hands_over_to_the_general_pipeline (tests/test_gpu_strips.py)."""
  noise = synth.random_labels((256, 256, 4), np.uint32, seed=5, high=2000)
  return Case(noise, bytes(crackle_amd.compress(noise)))


def _hand_over_case():
  return _voronoi_case((320, 288, 5), np.uint32, "F", 0, None)


def _assert_handed_over_to_general(sequence, stages, what):
  """The first paint of the sequence ran the strip path, which overflowed: that call is answered by the general
  pipeline from the planes the strip path left (no crack kernel in its table), every later P by the general pipeline
  from the start."""
  first_paint = min(i for i, op in enumerate(sequence) if op in PAINTS)
  for i, names in sorted(stages.items()):
    assert set(names) <= GENERAL and "k_run_index" in names and "k_paint_runs" in names, f"{what}: P at call {i} decoded by {names}"
    if i == first_paint:
      assert "k_decode_cracks" not in names, f"{what}: the first strip run did not hand over: {names}"
    else:
      assert _is_general(names), f"{what}: P at call {i} decoded by {names}"
  assert any(i > first_paint for i in stages)


@pytest.mark.parametrize("first", FIRST)
def test_strip_overflow_hand_over_then_everything_else(first):
  case = _noise_case()
  sequence = ds.hand_over(first, ds.OPS)
  with DecodeSession(case.binary) as sess:
    ran, stages = drive(sess, sequence, case)
  assert ran == sequence
  _assert_handed_over_to_general(sequence, stages, "noise")


@pytest.mark.parametrize("first", FIRST)
def test_record_list_hand_over_then_everything_else(first, monkeypatch):
  """CKL_REC_CAP=3 (read when the session is built): the first strip run overflows its record lists and the session
  takes the rasterising front end for this and all later strip runs."""
  case = _hand_over_case()
  sequence = ds.hand_over(first, ds.OPS)
  monkeypatch.setenv("CKL_REC_CAP", "3")
  with DecodeSession(case.binary) as sess:
    ran, stages = drive(sess, sequence, case)
  assert ran == sequence
  for i, names in sorted(stages.items()):
    assert names == RASTER_STRIP_V1, f"CKL_REC_CAP=3: P at call {i} decoded by {names}"


@pytest.mark.parametrize("first", FIRST)
def test_without_the_switches_the_hand_over_volume_stays_on_the_record_kernels(first):
  """The volume of the two forced hand-overs is on k_crack_match and the strip kernels when nothing is forced, whatever
  the session was asked first: what the tests around this one see is the hand-over, not the volume."""
  case = _hand_over_case()
  with DecodeSession(case.binary) as sess:
    ran, stages = drive(sess, ds.hand_over(first, ds.OPS), case)
  _assert_path(stages, STRIP_V1, "320 x 288 x 5")


@pytest.mark.parametrize("first", FIRST)
def test_resolve_table_hand_over_then_everything_else(first, monkeypatch):
  """CKL_RESOLVE_CAP=7 (read by every strip run): k_slice_resolve's table overflows and the session goes to the
  general pipeline."""
  case = _hand_over_case()
  sequence = ds.hand_over(first, ds.OPS)
  with DecodeSession(case.binary) as sess:
    monkeypatch.setenv("CKL_RESOLVE_CAP", "7")
    ran, stages = drive(sess, sequence, case)
  assert ran == sequence
  _assert_handed_over_to_general(sequence, stages, "CKL_RESOLVE_CAP=7")


# ---- a damaged slice -----------------------------------------------------------------------------------------------

def _damaged():
  """tests/test_gpu_paste.py: test_a_damaged_slice_inside_and_outside_the_range.  The stored crc of slice 3 of golden
  c0_voronoi_u8 is changed: a detected error, not a fault."""
  vol = golden_cases.small_cases()["c0_voronoi_u8"][0]
  good = golden()["c0_voronoi_u8"]
  sz = vol.shape[2]
  bad = bytearray(good)
  bad[len(good) - 4 * sz + 4 * 3] ^= 0x10
  return vol, good, bytes(bad)


def test_a_damaged_slice_is_reported_by_every_call_and_by_no_other():
  vol, good, bad = _damaged()
  case = Case(vol, good)      # (label and box; the expectations of the good stream are not used)
  with pytest.raises(RuntimeError) as info:
    crackle_amd.decompress(bad)
  message = str(info.value)
  assert type(info.value) is RuntimeError and "z=3" in message
  want = np.zeros((vol.shape[2],), np.uint32)
  want[3] = SLICE_BAD_CRC
  prev = None
  with DecodeSession(bad) as sess:
    for op in ("K", "P", "K", "C", "K", "S", "K", "T", "K", "L", "K"):
      if op == "K":
        got = sess.check()
        assert np.array_equal(got, want), f"K behind {prev}: verdicts {got.tolist()}"
      else:
        with pytest.raises(RuntimeError) as got:
          call(sess, op, case)
        assert type(got.value) is RuntimeError and str(got.value) == message, f"{op} behind {prev}: {got.value}"
      prev = op


def test_a_damaged_slice_across_the_hand_over_to_the_general_pipeline(monkeypatch):
  """CKL_RESOLVE_CAP=7 on the stream with the wrong crc: the first P runs the strip kernels, every slice overflows
  k_slice_resolve's table before its crc is compared, so the words that kernel leaves in the host's mapped memory are
  clean; the general pipeline finishes the call and raises.  The K behind it must report slice 3 from its own run
  (decoder_run resets flags_by_resolve; without that it would hand out the strip run's clean words)."""
  vol, good, bad = _damaged()
  case = Case(vol, good)
  with pytest.raises(RuntimeError) as info:
    crackle_amd.decompress(bad)
  message = str(info.value)
  want = np.zeros((vol.shape[2],), np.uint32)
  want[3] = SLICE_BAD_CRC
  prev = None
  with DecodeSession(bad) as sess:
    monkeypatch.setenv("CKL_RESOLVE_CAP", "7")
    for op in ("P", "K", "L", "K", "C", "K", "P", "K"):
      if op == "K":
        got = sess.check()
        assert np.array_equal(got, want), f"K behind {prev}: verdicts {got.tolist()}"
      else:
        with pytest.raises(RuntimeError) as got:
          call(sess, op, case)
        assert type(got.value) is RuntimeError and str(got.value) == message, f"{op} behind {prev}: {got.value}"
      prev = op
    monkeypatch.delenv("CKL_RESOLVE_CAP")
    # handed over for good: a clean range of the same session kind is covered above; here the path is what is left to see
    with pytest.raises(RuntimeError):
      sess.run()
    assert _is_general([n for n in sess.stages() if n != "memset"]), sess.stages()


def test_a_damaged_crack_code_gets_the_verdict_of_a_fresh_session_behind_every_raise():
  """tests/test_gpu_cutout.py: test_a_damaged_slice_raises_as_for_a_decode.  One byte in the middle of slice 3's crack
  code is flipped: the strip kernels (P, L) and the general pipeline (C, S, T, K) each find it in their own way, and a
  K must report what the general pipeline found in that K, never the words an earlier call left in the host's
  mapped memory.  The expected verdicts are a fresh session's single K; every other call raises what decompress raises."""
  vol, good, _ = _damaged()
  head = crackle_amd.header(good)
  zidx = np.frombuffer(good, dtype="<u4", offset=head.header_bytes, count=head.sz).astype(np.int64)
  start = head.header_bytes + head.grid_index_bytes + head.num_label_bytes + head.markov_model_bytes + int(zidx[:3].sum())
  bad = bytearray(good)
  bad[start + int(zidx[3]) // 2] ^= 0x04
  bad = bytes(bad)
  case = Case(vol, good)
  with pytest.raises(RuntimeError) as info:
    crackle_amd.decompress(bad)
  message = str(info.value)
  assert type(info.value) is RuntimeError and "z=3" in message
  with DecodeSession(bad) as fresh:
    want = fresh.check()
  assert np.flatnonzero(want).tolist() == [3]
  prev = None
  with DecodeSession(bad) as sess:
    for op in ("K", "P", "K", "C", "K", "S", "K", "T", "K", "L", "K", "V6", "K"):
      if op == "K":
        got = sess.check()
        assert np.array_equal(got, want), f"K behind {prev}: verdicts {got.tolist()}, a fresh session's {want.tolist()}"
      else:
        with pytest.raises(RuntimeError) as got:
          call(sess, op, case)
        assert type(got.value) is RuntimeError and str(got.value) == message, f"{op} behind {prev}: {got.value}"
      prev = op


def test_a_session_beside_the_damaged_slice_passes_the_whole_schedule():
  vol, good, bad = _damaged()
  sz = vol.shape[2]
  case = Case(vol, good, 4, sz)      # expectations: numpy, and fresh sessions over the same slices of the good stream
  sequence = ds.schedule(ds.OPS)
  with DecodeSession(bad, 4, sz) as sess:
    ran, stages = drive(sess, sequence, case)
  assert ds.pairs_of(ran) == EVERY_PAIR
  assert ran.count("K") == 9      # (every one of them compared with zeros)
