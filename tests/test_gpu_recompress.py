"""GPU tests of crackle_amd.recompress (ckl_recompress: the decoder's run tables -> k_label_planes_from_runs -> the
encoder's crack and label stages, crackle_amd/csrc/ckl_recompress.hpp, ckl_recompress.hip, ckl_encode.hip and ckl_encode_labels.hip).

The check throughout: recompress(stream, ...) equals the checker's compress of the volume the stream decodes to,
byte for byte, under the requested markov order (default: the stream's), once on the default label path and once
with the run pipeline forced (CKL_ENC_LABEL_RUNS), and crackle_amd.ok() accepts the result.  The volumes and what
each of them is about: tests/recompress_volumes.py, pinned on the CPU by tests/test_recompress_volumes_cpu.py."""
import os
import re

import numpy as np
import pytest

import crackle_amd
from crackle_amd import codec
import recompress_volumes as rv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PERMISSIBLE, IMPERMISSIBLE = 1, 0


def _check(stream, want_arr, checker, monkeypatch, order=None, capfd=None, marks=(), verify=True):
  """order: the markov_model_order argument (None: keep the stream's).  marks: what the encoder's host timer line of
  the default path must name (f:enqueue_strips, f:resolve_retry, f:enqueue_runs, f:wait_strips / f:wait_runs)."""
  head = crackle_amd.header(stream)
  m = head.markov_model_order if order is None else order
  want = checker.compress(want_arr, fortran_order=head.fortran_order, markov_model_order=m)
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  if capfd is not None:
    monkeypatch.setenv("CKL_PROFILE", "1")
    capfd.readouterr()
  got = crackle_amd.recompress(stream, markov_model_order=order)
  if capfd is not None:
    monkeypatch.delenv("CKL_PROFILE", raising=False)
    err = capfd.readouterr().err.splitlines()
    mine = [l for l in err if l.startswith("[ckl recompress host ms]")]
    assert len(mine) == 1, err
    fields = dict(w.split("=") for w in mine[0].split()[4:])
    assert list(fields)[:6] == ["tables", "label_planes", "graph", "cracks", "labels", "assembly"], mine[0]
    assert float(fields["label_planes"]) > 0 and float(fields["k_label_planes_from_runs_device"]) > 0
    enc = [l for l in err if l.startswith("[ckl encode host ms]")]
    seen = sorted(w.split("=")[0] for w in enc[-1].split() if w.startswith("f:"))
    for mark in marks:
      assert mark in seen, f"{mark} not among {seen}"
  assert got == want, f"default label path {want_arr.shape} {want_arr.dtype} order={order}"
  monkeypatch.setenv("CKL_ENC_LABEL_RUNS", "1")
  assert crackle_amd.recompress(stream, markov_model_order=order) == want, f"run pipeline forced {want_arr.shape} {want_arr.dtype} order={order}"
  monkeypatch.delenv("CKL_ENC_LABEL_RUNS", raising=False)
  out = crackle_amd.header(got)
  assert out.label_format == 0 and out.format_version == 1 and out.data_width == head.data_width and out.fortran_order == head.fortran_order
  if verify:
    assert crackle_amd.ok(got)
  return got


def _remapped(vol, mapping, checker, **kw):
  return crackle_amd.remap(checker.compress(vol, **kw), mapping)


# ---- unchanged streams -------------------------------------------------------------------------------------------------
UNCHANGED = [((128, 64, 9), "F", 51), ((97, 61, 7), "F", 52), ((96, 80, 6), "C", 53)]


@pytest.fixture(scope="module", params=UNCHANGED, ids=lambda p: "x".join(map(str, p[0])) + p[1])
def plain(request):
  shape, layout, seed = request.param
  arr = rv.voronoi(shape, np.uint32, seed, cell=(16, 16, 4))
  if layout == "C":
    arr = np.ascontiguousarray(arr)
    assert not arr.flags.f_contiguous
  return arr


@pytest.mark.parametrize("kw", [dict(), dict(allow_pins=True), dict(markov_model_order=5)], ids=["flat", "pins", "markov5"])
def test_unchanged_stream_comes_back_canonical(plain, kw, checker, monkeypatch):
  b = checker.compress(plain, **kw)
  assert crackle_amd.header(b).label_format == (2 if kw.get("allow_pins") else 0)
  got = _check(b, plain, checker, monkeypatch)
  if not kw.get("allow_pins"):
    assert got == b
  assert crackle_amd.header(got).markov_model_order == kw.get("markov_model_order", 0)


@pytest.mark.parametrize("order", [0, 3])
def test_explicit_markov_order(plain, order, checker, monkeypatch):
  got = _check(checker.compress(plain, markov_model_order=5), plain, checker, monkeypatch, order=order)
  assert crackle_amd.header(got).markov_model_order == order


def _v0_fixtures():
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    return {k: z[k].tobytes() for k in z.files if "." not in k}


@pytest.mark.parametrize("name", sorted(_v0_fixtures()))
def test_version_0_stream(name, checker, monkeypatch):
  b0 = _v0_fixtures()[name]
  head = crackle_amd.header(b0)
  assert head.format_version == 0 and not head.signed
  arr = checker.decompress(b0).reshape((head.sx, head.sy, head.sz), order="F" if head.fortran_order else "C")
  _check(b0, arr, checker, monkeypatch)


# ---- merged streams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rv.MERGED, ids=repr)
def test_merged_stream(case, checker, monkeypatch, capfd):
  vol, merged = case.volume(), case.merged()
  remapped = _remapped(vol, rv.floordiv_mapping(vol, case.divisor), checker)
  got = _check(remapped, merged, checker, monkeypatch, capfd=capfd)
  head = crackle_amd.header(got)
  assert head.crack_format == (PERMISSIBLE if rv.permissible(merged) else IMPERMISSIBLE)
  assert len(got) < len(remapped)
  assert head.stored_data_width == (1 if int(merged.max()) < 256 else 2)
  assert np.array_equal(crackle_amd.decompress(got), merged)


def test_merged_by_an_in_place_rewrite_of_the_unique_list(checker, monkeypatch):
  vol = rv.VORONOI.volume()
  b = rv.floordiv_stream(checker.compress(vol))
  u = crackle_amd.labels(b)
  assert len(np.unique(u)) < len(u)      # duplicates in the list
  got = _check(b, rv.VORONOI.merged(), checker, monkeypatch)
  assert len(got) < len(b)


def test_mask_except_five_labels(checker, monkeypatch):
  vol = rv.VORONOI.volume()
  keep = [int(v) for v in np.unique(vol)[[0, 7, 20, 33, 50]]]
  b = crackle_amd.mask_except(checker.compress(vol, markov_model_order=2), keep)
  want = np.asfortranarray(np.where(np.isin(vol, keep), vol, 0).astype(vol.dtype))
  got = _check(b, want, checker, monkeypatch)
  assert sorted(int(v) for v in crackle_amd.labels(got)) == sorted(keep + [0])
  assert len(got) < len(b)


def test_mask_of_every_label_resets_the_markov_order(checker, monkeypatch):
  vol = rv.VORONOI.volume()
  b = crackle_amd.mask(checker.compress(vol, markov_model_order=5), [int(v) for v in np.unique(vol)])
  assert crackle_amd.header(b).markov_model_order == 5 and crackle_amd.num_labels(b) == 1
  got = _check(b, np.zeros(vol.shape, dtype=vol.dtype, order="F"), checker, monkeypatch)
  head = crackle_amd.header(got)
  assert head.markov_model_order == 0 and crackle_amd.num_labels(got) == 1      # no cracks: compress resets the order
  # asked for explicitly it is reset all the same
  assert crackle_amd.header(_check(b, np.zeros(vol.shape, dtype=vol.dtype, order="F"), checker, monkeypatch, order=3)).markov_model_order == 0


# ---- word and row edges ------------------------------------------------------------------------------------------------
EDGES = [(sx, 9, 3) for sx in (31, 32, 33, 64, 65)] + [(1, 37, 6), (41, 1, 6), (33, 27, 1), (1, 1, 1)]


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "x".join(map(str, s)))
def test_word_and_row_edges(shape, checker, monkeypatch):
  vol = rv.noise(shape, np.uint8, 60 + shape[0], 3)
  merged = np.asfortranarray(vol // 2)
  b = _remapped(vol, rv.floordiv_mapping(vol, 2), checker)
  got = _check(b, merged, checker, monkeypatch)
  assert crackle_amd.header(got).crack_format == (PERMISSIBLE if rv.permissible(merged) else IMPERMISSIBLE)
  _check(checker.compress(vol, markov_model_order=1), vol, checker, monkeypatch)


@pytest.mark.parametrize("shape", [(0, 0, 0), (5, 0, 3)], ids=lambda s: "x".join(map(str, s)))
def test_streams_without_voxels(shape, checker, monkeypatch):
  arr = np.zeros(shape, dtype=np.uint16, order="F")
  b = checker.compress(arr, markov_model_order=2)
  got = _check(b, arr, checker, monkeypatch, verify=False)
  assert got == b and len(got) == 29
  assert crackle_amd.recompress(b, markov_model_order=0) == checker.compress(arr)


# ---- the label stage's paths -------------------------------------------------------------------------------------------
def _merge_mod(vol, k):
  return {int(v): int(v) % k for v in np.unique(vol)}, np.asfortranarray((vol % vol.dtype.type(k)))


def test_strip_path_and_its_hand_over(checker, monkeypatch, capfd):
  vol = rv.voronoi((320, 288, 5), np.uint32, 32)
  mapping, merged = _merge_mod(vol, 13)
  b = _remapped(vol, mapping, checker)
  got = _check(b, merged, checker, monkeypatch, capfd=capfd, marks=("f:enqueue_strips", "f:wait_strips"))
  assert len(got) < len(b)
  for switch, value in (("CKL_ENC_RESOLVE_CAP", "7"), ("CKL_ENC_STRIP_CAP", "64")):
    monkeypatch.setenv(switch, value)
    # the strips were launched, a table overflowed, the run pipeline redid the volume
    assert _check(b, merged, checker, monkeypatch, capfd=capfd, marks=("f:enqueue_strips", "f:enqueue_runs", "f:wait_runs")) == got
    monkeypatch.delenv(switch)


def test_resolve_again_with_a_whole_cu(checker, monkeypatch, capfd):
  # more strip components per slice than the resolve's table beside the walk holds, fewer than a CU's LDS does
  # (tests/test_gpu_encoder_strips.py: 21 760 single pixels in a background); pairs of them merged
  a = np.full((1024, 512, 2), 7, dtype=np.uint32, order="F")
  xs, ys = np.arange(1, 1024, 4), np.arange(1, 512, 6)
  ids = 100 + np.arange(xs.size * ys.size, dtype=np.uint32).reshape(xs.size, ys.size)
  for z in range(2):
    a[np.ix_(xs, ys, [z])] = (ids + 50000 * z)[:, :, None]
  b = _remapped(a, rv.floordiv_mapping(a, 2), checker)
  _check(b, np.asfortranarray(a // 2), checker, monkeypatch, capfd=capfd, marks=("f:enqueue_strips", "f:resolve_retry", "f:wait_strips"))


def test_rows_wider_than_a_strip(checker, monkeypatch, capfd):
  vol = rv.voronoi((32800, 3, 2), np.uint8, 33, cell=(16, 2, 1))
  mapping, merged = _merge_mod(vol, 5)
  _check(_remapped(vol, mapping, checker), merged, checker, monkeypatch, capfd=capfd, marks=("f:enqueue_runs", "f:wait_runs"))


def test_slices_over_the_overlap_limit_label_before_the_graph(checker, monkeypatch, capfd):
  vol = rv.voronoi((1600, 1500, 2), np.uint8, 34, cell=(32, 32, 2))
  assert vol.shape[0] * vol.shape[1] > 1536 * 1536
  mapping, merged = _merge_mod(vol, 7)
  _check(_remapped(vol, mapping, checker), merged, checker, monkeypatch, capfd=capfd, marks=("f:enqueue_runs", "f:wait_runs"))


# ---- widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_every_unsigned_width(dtype, checker, monkeypatch):
  offset = (1 << 40) if dtype == np.uint64 else 0
  vol = rv.voronoi((97, 61, 5), dtype, 35, cell=(8, 8, 3), modulus=200, offset=offset)
  mapping = {int(v): offset + (int(v) - offset) // 3 for v in np.unique(vol)}
  merged = np.asfortranarray((offset + (vol.astype(np.uint64) - np.uint64(offset)) // np.uint64(3)).astype(dtype))
  if dtype == np.uint64:
    assert int(merged.min()) >= (1 << 40)
  got = _check(_remapped(vol, mapping, checker, markov_model_order=2), merged, checker, monkeypatch)
  assert np.array_equal(crackle_amd.decompress(got), merged)
  _check(checker.compress(vol, allow_pins=True), vol, checker, monkeypatch)


def test_signed_streams_are_refused(checker):
  b = rv.as_signed(checker.compress(rv.VORONOI.volume()))
  with pytest.raises(TypeError, match="Signed integer data types are not currently supported."):
    crackle_amd.recompress(b)
  from crackle_amd import _lib
  import ctypes as C
  out, n = C.c_void_p(), C.c_uint64()
  assert _lib.lib().ckl_recompress(b, len(b), -1, 0, C.byref(out), C.byref(n)) == _lib.CKL_ERR_ARG


def test_medium_volume(checker, monkeypatch, capfd):
  vol = rv.voronoi((256, 256, 32), np.uint32, 5, cell=(32, 32, 8), modulus=50)
  b = _remapped(vol, rv.floordiv_mapping(vol, 5), checker, markov_model_order=3)
  got = _check(b, np.asfortranarray(vol // 5), checker, monkeypatch, capfd=capfd)
  assert len(got) < len(b)
  arr = crackle_amd.CrackleArray(b).recompress()
  assert isinstance(arr, crackle_amd.CrackleArray) and arr.binary == got


def test_repeatable(checker):
  vol = rv.VORONOI.volume()
  b = _remapped(vol, rv.floordiv_mapping(vol, 2), checker, markov_model_order=4)
  outs = [crackle_amd.recompress(b) for _ in range(3)]
  assert outs[0] == outs[1] == outs[2] == checker.compress(rv.VORONOI.merged(), markov_model_order=4)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(checker):
  lab = rv.voronoi((48, 40, 5), np.uint16, 12, cell=(8, 8, 2))
  b = checker.compress(lab)
  with pytest.raises(ValueError, match="allow_pins"):
    crackle_amd.recompress(b, allow_pins=True)
  assert crackle_amd.recompress(b, memory_target=1) == b      # accepted and ignored
  # a damaged slice: what decompress raises for it
  head = crackle_amd.header(b)
  lens = [int.from_bytes(b[29 + 4 * z:33 + 4 * z], "little") for z in range(head.sz)]
  codes = head.header_bytes + head.grid_index_bytes + head.num_label_bytes
  bad = bytearray(b)
  bad[codes + lens[0] + lens[1] + lens[2] // 2] ^= 0xFF
  with pytest.raises(Exception) as seen:
    crackle_amd.decompress(bytes(bad))
  assert "z=2" in str(seen.value)
  with pytest.raises(type(seen.value), match=re.escape(str(seen.value))):
    crackle_amd.recompress(bytes(bad))
  # a corrupted label section: slice 1 claims one component more, slice 2 one fewer
  n, off = codec._label_section(b, head)
  at = off + n * head.stored_data_width
  cw = 2      # components per slice are stored at the byte width of sx * sy = 1920
  bad = bytearray(b)
  for z, d in ((1, 1), (2, -1)):
    v = int.from_bytes(bad[at + z * cw:at + (z + 1) * cw], "little") + d
    bad[at + z * cw:at + (z + 1) * cw] = v.to_bytes(cw, "little")
  with pytest.raises(RuntimeError, match="component count does not match the label section"):
    crackle_amd.recompress(bytes(bad))
