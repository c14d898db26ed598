"""GPU tests of the encoder's flat label table at its own size thresholds (crackle_amd/csrc/ckl_encode_labels.hip:
flat_section with k_label_hash_*, k_pad_copy_u64, k_bitonic_first / step / step2 / local, k_unique_*, k_flat_section;
ckl_encode.hip: crc32c_device with k_crc32c_pieces / k_crc32c_fold; k_copy_bytes; k_code_offsets).

The volumes come from tests/label_table_volumes.py, which aims N (components), U (labels) and L (label section bytes) at
the numbers the code decides by; tests/test_label_table_volumes_cpu.py pins every one of them against the port on the
CPU.  The check throughout: crackle_amd.compress(arr) equals the checker's stream, section by section and whole, on the
default path, with the hash pass switched off (CKL_LABEL_SORT_ALL), with the double sort steps switched off
(CKL_BITONIC_SINGLE_STEPS) and, above 8192 components, with the run pipeline's gather feeding the table
(CKL_ENC_LABEL_RUNS); and the checker's stream itself states the N, U, key width and L the case is about.

Left out (volumes far beyond a few seconds): more than 2^26 components, where the hash pass is skipped again, and
component counts of 8 bytes.  The pin label section and the decoder's label parsing have tests of their own
(test_gpu_pins.py, test_gpu_format_boundaries.py)."""
import ctypes as C

import numpy as np
import pytest

import crackle_amd
import label_table_volumes as ltv
from gen_golden import sections

pytestmark = pytest.mark.gpu

SWITCHES = ("CKL_LABEL_SORT_ALL", "CKL_BITONIC_SINGLE_STEPS", "CKL_ENC_LABEL_RUNS")


def _same(got, want, what):
  """Section by section, so that a failure names the section and the first byte, then whole."""
  gs, ws = sections(got), sections(want)
  for name, w in ws.items():
    g = gs.get(name)
    if g != w:
      at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
      raise AssertionError(f"{what}: section '{name}' differs from byte {at} on ({len(g)} bytes, {len(w)} wanted)")
  ok = got == want
  assert ok, f"{what}: sections equal, streams differ"


def _check(case, checker, monkeypatch):
  arr = case.volume()
  kw = dict(markov_model_order=case.markov)
  want = checker.compress(arr, **kw)
  assert ltv.read_claims(want) == case.claims, case.id
  passes = [None, "CKL_LABEL_SORT_ALL", "CKL_BITONIC_SINGLE_STEPS"] + (["CKL_ENC_LABEL_RUNS"] if case.n > ltv.HASH_ABOVE else [])
  for switch in passes:      # read by the library at every call
    for name in SWITCHES:
      monkeypatch.delenv(name, raising=False)
    if switch:
      monkeypatch.setenv(switch, "1")
    _same(crackle_amd.compress(arr, **kw), want, f"{case.id} {switch or 'default'}")
  for name in SWITCHES:
    monkeypatch.delenv(name, raising=False)
  back = crackle_amd.decompress(want)
  ok = back.dtype == arr.dtype and np.array_equal(back, arr)
  assert ok, case.id
  return want


def _ids(cases):
  return [c.id for c in cases]


HASH = ltv.hash_threshold_cases()
SORT = ltv.sort_size_cases()
SORT_ALL = ltv.sort_all_cases()
KEYS = ltv.key_width_cases()
EDGE = ltv.edge_value_cases()
SLICES = ltv.many_slices_cases()
MERGED = ltv.merged_cases()


@pytest.mark.parametrize("case", HASH, ids=_ids(HASH))
def test_hash_threshold_and_table_size(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


@pytest.mark.parametrize("case", SORT, ids=_ids(SORT))
def test_sort_sizes_behind_the_hash_pass(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


@pytest.mark.parametrize("case", SORT_ALL, ids=_ids(SORT_ALL))
def test_sort_sizes_and_block_edges_of_all_keys(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


@pytest.mark.parametrize("case", KEYS, ids=_ids(KEYS))
def test_key_width(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


@pytest.mark.parametrize("case", EDGE, ids=_ids(EDGE))
def test_edge_values(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


@pytest.mark.parametrize("case", SLICES, ids=_ids(SLICES))
def test_many_slices(case, checker, monkeypatch):
  _check(case, checker, monkeypatch)


# ---- streams that stay in HBM: the section's crc32c on the device, the copy into the resident stream -----------------
def _to_device(arr):
  """(sx, sy, sz) numpy -> the (sz, sy, sx) tensor the backends take (unsigned labels as their bit patterns)."""
  import torch
  bits = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[arr.dtype.itemsize]
  return torch.from_numpy(np.ascontiguousarray(np.transpose(arr, (2, 1, 0))).view(bits)).to("cuda:0")


def test_section_crc_and_resident_copy_at_the_frame_sizes(checker):
  """L on both sides of 32768 (one workgroup or two), 65536, 2^20 and 8 MiB (where the piece length leaves 128), in an
  order that changes the cached shift tables more than twice.  After host_wait() the host bytes are the checker's; the
  HBM stream read back is the same bytes (k_copy_bytes: the sections' offsets take every alignment over these cases); a
  decoder opened on the HBM stream returns the volume."""
  import torch
  from crackle_amd import distributed as ckd
  hip = C.CDLL("libamdhip64.so")
  cases = ltv.crc_cases()
  made = {}
  for length in ltv.CRC_ORDER:
    case = cases[length]
    if length not in made:
      arr = case.volume()
      want = checker.compress(arr)
      assert ltv.read_claims(want) == case.claims and case.length == length
      made[length] = (_to_device(arr), want)
    vol, want = made[length]
    shape, item = case.shape, vol.element_size()
    be = ckd.HipBackend(0, zero_copy=True)
    be.keep_device_stream(shape, item, True)
    be.async_host_copy(shape, item, True)
    try:
      stream = be.encode(vol, shape, False, True, 0, None)
      be.host_wait()
      _same(bytes(stream), want, f"L = {length}, (G, P) = {ltv.crc_frame(length)}: host bytes")
      ds = be.device_stream()
      assert len(ds) == len(want)
      back = np.zeros(len(want), dtype=np.uint8)
      assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(ds.ptr), C.c_size_t(len(want)), 2) == 0
      _same(back.tobytes(), want, f"L = {length}: stream in HBM")
      out = torch.empty_like(vol)
      s = be.open_decoder(ds, 0, shape[2])
      s.run(out)
      s.close()
      torch.cuda.synchronize()
      assert torch.equal(out, vol), length
    finally:
      be.async_host_copy(shape, item, False)
      be.keep_device_stream(shape, item, False)


# ---- keys against a caller's merged list (ckl_encode_overrides.merge_unique) -----------------------------------------
def _encode_slab(be, arr, head, merge):
  from crackle_amd.distributed import FLAT
  overrides = {"crack_format": head.crack_format, "label_format": FLAT, "stored_width": head.stored_data_width, "merge_unique": merge}
  return bytes(be.encode(_to_device(arr), arr.shape, False, True, 0, overrides))


@pytest.mark.parametrize("case", MERGED, ids=_ids(MERGED))
def test_keys_against_a_merged_list(case, checker):
  """Two z-slabs encoded apart, each against np.unique of both slabs' labels, stack to the checker's stream of the
  whole volume: lists that arrive sorted (at most 8192 components), as the hash pass left them (more), and a merged
  list far longer than the slab has components."""
  from crackle_amd import distributed as ckd
  slabs, whole = case.slabs(), case.whole()
  want = checker.compress(whole)
  head = crackle_amd.header(want)
  merged = np.unique(np.concatenate([s.reshape(-1) for s in slabs])).astype(np.uint64)
  assert ltv.read_claims(want)["U"] == merged.size
  be = ckd.HipBackend(0)
  streams = []
  for part, claim in zip(slabs, (case.first, case.second)):
    seen = []

    def merge(local, part=part, seen=seen):
      seen.append(local.copy())
      assert local.dtype == np.uint64 and local.size == np.unique(local).size
      assert set(local.tolist()) == set(np.unique(part).tolist())
      return merged

    stream = _encode_slab(be, part, head, merge)
    assert len(seen) == 1
    if claim.n <= ltv.HASH_ABOVE:
      assert np.all(np.diff(seen[0].astype(np.float64)) > 0) and np.array_equal(seen[0], np.sort(seen[0]))      # the sorted branch hands over a sorted list
    got = ltv.read_claims(stream)
    assert got["N"] == claim.n and got["U"] == merged.size
    assert np.array_equal(crackle_amd.labels(stream).astype(np.uint64), merged)
    back = crackle_amd.decompress(stream)
    ok = back.dtype == part.dtype and np.array_equal(back, part)
    assert ok, case.id
    streams.append(stream)
  _same(crackle_amd.zstack(streams), want, f"merged {case.id}")


@pytest.mark.parametrize("case", MERGED[:2], ids=_ids(MERGED[:2]))
def test_a_merged_list_without_one_of_the_slabs_labels_is_refused(case, checker):
  """A list as long as the right one that lacks a label of the slab: keys by binary search would name the label's
  neighbour and the stream would decode to another volume.  Before this check the encoder wrote that stream (it
  compared lengths only); now the section kernel reports the label it did not find and the encode fails."""
  from crackle_amd import distributed as ckd
  slabs, whole = case.slabs(), case.whole()
  head = crackle_amd.header(checker.compress(whole))
  merged = np.unique(whole).astype(np.uint64)
  part = slabs[0]
  mine = np.unique(part).astype(np.uint64)
  lost = mine[mine.size // 2]
  wrong = np.sort(np.concatenate((merged[merged != lost], np.array([int(merged.max()) + 9], dtype=np.uint64))))
  assert wrong.size == merged.size >= mine.size and lost not in wrong
  be = ckd.HipBackend(0)
  with pytest.raises(RuntimeError, match="lacks a label"):
    _encode_slab(be, part, head, lambda local: wrong)
  # the session is good for the next encode
  assert np.array_equal(crackle_amd.decompress(_encode_slab(be, part, head, lambda local: merged)), part)
