"""GPU tests of paste (crackle_amd/csrc/ckl_paste.hip: k_paste_box and ckl_paste; crackle_amd/array.py: paste,
CrackleArray.paste).  Expected voxels are always numpy's V[idx] = data on the array the stream was made from; expected
bytes come from the checker (whose precondition tests/test_paste_cpu.py asserts for the same cases,
tests/paste_volumes.py) or are put together from the functions the package had before paste.

The slab k_paste_box writes into is the library's: no test can lay a pattern around it.  What a test can see of a
store outside the box is the decoded volume, so every comparison is of the whole volume, not of the box."""
import ctypes as C
import os

import numpy as np
import pytest

import crackle_amd
import golden_cases
import paste_volumes as pv
from crackle_amd import _lib, codec, operations, synth
from crackle_amd.array import normalize_index
from util import golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
S = np.s_
SMALL = golden_cases.small_cases()


def _assert_volume(binary, want, what=None):
  got = crackle_amd.decompress(binary)
  assert got.dtype == want.dtype and got.shape == want.shape
  assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])


def _splices(idx, shape, head):
  """Case 1 of paste(): version 1, FLAT labels, a z-range that is not the whole depth."""
  z0, z1, _, _ = normalize_index(idx, shape)[2]
  return head.format_version == 1 and head.label_format == crackle_amd.LabelFormat.FLAT and (z0, z1) != (0, shape[2])


def _sections(binary):
  """(stored markov model, crack code of every slice) of a stream."""
  h = crackle_amd.header(binary)
  zidx = np.frombuffer(binary, dtype="<u4", offset=h.header_bytes, count=h.sz).astype(np.int64)
  model_at = h.header_bytes + h.grid_index_bytes + h.num_label_bytes
  codes_at = model_at + h.markov_model_bytes
  offs = codes_at + np.concatenate(([0], np.cumsum(zidx)))
  return binary[model_at:codes_at], [binary[int(offs[z]):int(offs[z + 1])] for z in range(h.sz)]


def _v0_streams():
  with np.load(os.path.join(HERE, "golden", "v0.npz")) as z:
    return {k: z[k].tobytes() for k in z.files if "." not in k}


# ---- arithmetic of k_paste_box ---------------------------------------------------------------------------

def _arithmetic_boxes(shape, itemsize):
  """x0 over every residue modulo the 16-byte chunk (V voxels) times the widths 1, V - 1, V, V + 1, at rows and
  slices that touch the volume's first and last ones; then the box positions: first and last column, the full row,
  a single voxel, the corner voxels, a whole plane of one slice."""
  sx, sy, sz = shape
  V = 16 // itemsize
  yz = [(0, 1, 0, 1), (sy - 1, sy, sz - 1, sz), (3, sy - 2, 1, sz - 1), (0, sy, 2, 3), (5, 7, 0, sz), (1, 4, sz - 2, sz)]
  boxes = []
  for r in range(V):
    for w in sorted({1, V - 1, V, V + 1} - {0}):
      y0, y1, z0, z1 = yz[len(boxes) % len(yz)]
      boxes.append((1 + r, 1 + r + w, y0, y1, z0, z1))
  boxes += [
    (0, 1, 0, sy, 0, 2), (sx - 1, sx, 0, sy, sz - 2, sz), (0, sx, 7, 9, 1, 2), (0, sx, 0, 1, 0, 1), (0, sx, sy - 1, sy, sz - 1, sz),
    (sx // 2, sx // 2 + 1, sy // 2, sy // 2 + 1, 2, 3), (0, 1, 0, 1, 0, 1), (sx - 1, sx, sy - 1, sy, sz - 1, sz),
    (0, sx, 0, sy, 1, 2), (0, sx, 0, sy, sz - 1, sz), (sx - V - 1, sx, 2, 5, 0, 1),
  ]
  for x0, x1, y0, y1, z0, z1 in boxes:
    assert 0 <= x0 < x1 <= sx and 0 <= y0 < y1 <= sy and 0 <= z0 < z1 <= sz
  return boxes


@pytest.mark.parametrize("shape,dtype,order", pv.GEOMETRIES, ids=pv.GEOMETRY_IDS)
def test_box_arithmetic(shape, dtype, order, checker):
  """One paste after the other into the same stream, every box first with array data and then with the scalar fill,
  numpy doing the same to the array; the volume is compared whole every eighth box (in turn behind the array and
  behind the fill) and at the end."""
  vol, src = pv.volume(shape, dtype, order), pv.other(shape, dtype, order)
  binary = checker.compress(vol)
  want = vol.copy(order="K")
  boxes = _arithmetic_boxes(shape, np.dtype(dtype).itemsize)
  for k, (x0, x1, y0, y1, z0, z1) in enumerate(boxes):
    idx = S[x0:x1, y0:y1, z0:z1]
    for data in (src[idx], int(src[x0, y0, z0]) if k % 2 else int(vol[x1 - 1, y1 - 1, z1 - 1])):
      binary = crackle_amd.paste(binary, idx, data)
      want[idx] = data
      if not np.isscalar(data) and k % 16 == 15:      # (the array data, before the fill covers it)
        _assert_volume(binary, want, boxes[k - 15:k + 1])
    if k % 16 == 7:
      _assert_volume(binary, want, boxes[max(0, k - 15):k + 1])
  _assert_volume(binary, want, boxes[-16:])
  assert not np.array_equal(want, vol)
  head = crackle_amd.header(binary)
  assert bool(head.fortran_order) == (order == "F") and head.data_width == np.dtype(dtype).itemsize


@pytest.mark.parametrize("shape,dtype,order", [pv.GEOMETRIES[i] for i in (0, 2, 3, 4)], ids=[pv.GEOMETRY_IDS[i] for i in (0, 2, 3, 4)])
def test_a_device_box_through_the_abi(shape, dtype, order, checker):
  """The box handed over as a device pointer (a torch buffer), one element behind the buffer's start so that it is
  aligned to nothing else, laid out as ckl_cutout writes it; the buffer, pattern around the box included, is unchanged
  afterwards."""
  import torch
  vol, src = pv.volume(shape, dtype, order), pv.other(shape, dtype, order)
  binary = checker.compress(vol)
  sx, sy, sz = shape
  item = np.dtype(dtype).itemsize
  L = _lib.lib()
  for x0, x1, y0, y1, z0, z1 in ((3, sx - 2, 1, sy - 1, 1, sz - 1), (1, 2, 0, sy, 0, sz), (0, sx, 0, sy, sz - 1, sz)):
    idx = S[x0:x1, y0:y1, z0:z1]
    box = src[idx]
    raw = np.full((box.size * item + 64,), 0xA5, np.uint8)
    raw[item:item + box.size * item] = np.frombuffer(box.tobytes(order="F" if order == "F" else "C"), np.uint8)
    buf = torch.from_numpy(raw).to("cuda")
    out, n = C.c_void_p(), C.c_uint64()
    rc = L.ckl_paste(binary, len(binary), buf.data_ptr() + item, _lib.MEM_DEVICE, 1, 0, x0, x1, y0, y1, z0, z1, 0, C.byref(out), C.byref(n))
    assert rc == _lib.CKL_OK, _lib.last_error()
    got = C.string_at(out.value, n.value)
    L.ckl_free(out)
    assert np.array_equal(buf.cpu().numpy(), raw)
    _assert_volume(got, pv.edited(vol, idx, box), idx)
    assert got == crackle_amd.paste(binary, idx, box)      # the host box takes the same way behind its upload
  # the fill through the ABI uploads nothing: a null box is fine
  out, n = C.c_void_p(), C.c_uint64()
  rc = L.ckl_paste(binary, len(binary), None, _lib.MEM_DEVICE, 0, 3, 2, 9, 1, 4, 1, 2, 0, C.byref(out), C.byref(n))
  assert rc == _lib.CKL_OK, _lib.last_error()
  got = C.string_at(out.value, n.value)
  L.ckl_free(out)
  _assert_volume(got, pv.edited(vol, S[2:9, 1:4, 1:2], 3))


# ---- the bytes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", pv.SPLICES, ids=repr)
def test_splice_bytes_at_markov_0(case, checker):
  vol, new = case.volume(), case.edited()
  got = crackle_amd.paste(checker.compress(vol), case.idx, case.data())
  assert got == checker.compress(new)
  _assert_volume(got, new)


@pytest.mark.parametrize("order", [1, 4])
def test_splice_bytes_under_the_inputs_model(order):
  """The input carries a model the test built (stats_to_model of markov_hist), so the expected stream can be put
  together from the encoder's overrides, zsplit's ranges and zstack: the functions the package had before paste."""
  import torch
  from crackle_amd import distributed as ckd
  shape = (96, 80, 6)
  dev = torch.device("cuda", 0)
  t = synth.voronoi_labels(shape, np.uint32, seed=23, cell=(16, 16, 4), device=dev)
  vol = np.asfortranarray(synth.as_numpy_f(t))
  assert not pv.permissible(vol)
  be = ckd.HipBackend(0)
  model = ckd.stats_to_model(be.markov_hist(t.clone(), shape, 0, order))
  binary = bytes(be.encode(t.clone(), shape, False, True, order, {"model": model}))
  head = crackle_amd.header(binary)
  assert head.markov_model_order == order and head.crack_format == crackle_amd.CrackFormat.IMPERMISSIBLE
  _assert_volume(binary, vol)
  other = synth.as_numpy_f(synth.voronoi_labels(shape, np.uint32, seed=29, cell=(16, 16, 4)))
  for idx in (S[10:70, 5:60, 2:4], S[:, 40:, 0:3], S[3:4, 3:4, 5]):
    z0, z1, _, _ = normalize_index(idx, shape)[2]
    new = pv.edited(vol, idx, other[idx])
    slab = np.ascontiguousarray(new[:, :, z0:z1].transpose(2, 1, 0)).view(np.int32)
    forced = {"crack_format": int(head.crack_format), "label_format": 0, "model": model}
    mid = bytes(ckd.HipBackend(0).encode(torch.from_numpy(slab).to(dev), (shape[0], shape[1], z1 - z0), False, True, order, forced))
    parts = ([operations._zrange(binary, 0, z0)] if z0 > 0 else []) + [mid] + ([operations._zrange(binary, z1, shape[2])] if z1 < shape[2] else [])
    want = operations.zstack(parts)
    got = crackle_amd.paste(binary, idx, other[idx])
    assert got == want, idx
    _assert_volume(got, new, idx)
    # directly: the model and every untouched slice's crack code and crc are the input's bytes
    assert crackle_amd.header(got).markov_model_order == order
    (model_in, codes_in), (model_out, codes_out) = _sections(binary), _sections(got)
    assert model_in == model_out and len(model_in) == head.markov_model_bytes
    crc_in, crc_out = codec.crack_crcs(binary), codec.crack_crcs(got)
    for z in [z for z in range(shape[2]) if not z0 <= z < z1]:
      assert codes_in[z] == codes_out[z] and crc_in[z] == crc_out[z], (idx, z)


def test_the_inputs_crack_format_is_imposed_on_the_slab(checker):
  """Binary noise over two whole slices of a smooth volume: encoded on its own the slab is PERMISSIBLE (the CPU file
  asserts it), and a stack of both formats does not exist."""
  vol, idx, data = pv.smooth_and_noise()
  binary = checker.compress(vol)
  new = pv.edited(vol, idx, data)
  got = crackle_amd.paste(binary, idx, data)
  assert crackle_amd.header(got).crack_format == crackle_amd.header(binary).crack_format == crackle_amd.CrackFormat.IMPERMISSIBLE
  _assert_volume(got, new)
  assert got == checker.compress(new)      # (the whole volume stays IMPERMISSIBLE: tests/test_paste_cpu.py)


# ---- the label table ---------------------------------------------------------------------------------------

def test_a_label_that_is_overwritten_leaves_the_table(checker):
  vol = pv.volume(*pv.GEOMETRIES[0])
  label = int(vol[40, 30, 3])
  where = np.argwhere(vol == label)
  lo, hi = where.min(axis=0), where.max(axis=0) + 1
  idx = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
  assert (hi[2] - lo[2]) < vol.shape[2]
  spare = int(vol[0, 0, 0])
  assert spare != label
  data = np.where(vol[idx] == label, spare, vol[idx]).astype(vol.dtype)
  new = pv.edited(vol, idx, data)
  got = crackle_amd.paste(checker.compress(vol), idx, data)
  assert label in np.unique(vol) and label not in np.unique(new)
  assert np.array_equal(crackle_amd.labels(got), np.unique(new)) and not crackle_amd.contains(got, label)
  _assert_volume(got, new)


def test_a_wider_label_widens_the_stored_width(checker):
  vol = np.asfortranarray(pv.volume(*pv.GEOMETRIES[1]) % np.uint32(251))
  binary = checker.compress(vol)
  assert crackle_amd.header(binary).stored_data_width == 1 and crackle_amd.header(binary).data_width == 4
  idx = S[3:9, 4:8, 2:3]
  got = crackle_amd.paste(binary, idx, 70000)
  new = pv.edited(vol, idx, 70000)
  assert crackle_amd.header(got).stored_data_width == 4
  assert np.array_equal(crackle_amd.labels(got), np.unique(new))
  _assert_volume(got, new)


def test_a_single_label_stream(checker):
  """kat_ones_300: the Python layer answers its decode on the host; ckl_paste fills the slab with the paste kernel."""
  binary = golden()["kat_ones_300"]
  vol = SMALL["kat_ones_300"][0]
  assert crackle_amd.num_labels(binary) == 1
  src = synth.random_labels(vol.shape, np.uint32, seed=5, high=4)
  for idx, data in ((S[10:20, 290:, 1], 5), (S[1:4, 1:4, :], 1), (S[7:150, 3:299, 0], src[7:150, 3:299, 0]), (S[::9, ::7, :], src[::9, ::7, :])):
    new = pv.edited(vol, idx, data)
    got = crackle_amd.paste(binary, idx, data)
    _assert_volume(got, new, idx)
    assert np.array_equal(crackle_amd.labels(got), np.unique(new))
  assert crackle_amd.paste(binary, S[1:4, 1:4, :], 1) == checker.compress(vol)      # whole depth: compress of the same volume


# ---- the whole re-encode -----------------------------------------------------------------------------------

def test_whole_reencode_of_pin_version_0_and_whole_depth_streams(checker):
  g = golden()
  v0 = _v0_streams()
  cases = []
  vol = SMALL["c0_voronoi_u8_pins_m5"][0]
  cases.append(("pins", g["c0_voronoi_u8_pins_m5"], vol, S[3:40, 5:9, 2:5], 9))
  cases.append(("pins-array", g["c0_voronoi_u8_pins"], vol, S[1:63, 60:, 0:1], vol[1:63, :4, 7:8]))
  for name in ("c0_voronoi_u8", "c0_voronoi_u8_c", "rand_17x13x5_uint64_F_m3_p1"):      # flat F, flat C, pins + markov
    v = SMALL[name][0]
    assert crackle_amd.header(v0[name]).format_version == 0
    cases.append(("v0-" + name, v0[name], v, S[2:9, 1:7, 1:3], int(v[0, 0, 0])))
  v = pv.volume(*pv.GEOMETRIES[1])
  cases.append(("flat-whole-depth", checker.compress(v), v, S[20:77, 3:50, :], pv.other(*pv.GEOMETRIES[1])[20:77, 3:50, :]))
  cases.append(("flat-whole-depth-m3", checker.compress(v, markov_model_order=3), v, S[5, 6, :], 77))
  vc = pv.volume(*pv.GEOMETRIES[2])
  cases.append(("flat-C-whole-depth", checker.compress(vc), vc, S[:, 10:12], pv.other(*pv.GEOMETRIES[2])[:, 10:12]))
  for name, binary, vol, idx, data in cases:
    head = crackle_amd.header(binary)
    assert not _splices(idx, vol.shape, head), name
    new = pv.edited(vol, idx, data)
    got = crackle_amd.paste(binary, idx, data)
    assert got == checker.compress(new, markov_model_order=head.markov_model_order), name
    out = crackle_amd.header(got)
    assert out.label_format == crackle_amd.LabelFormat.FLAT and out.format_version == 1 and bool(out.fortran_order) == bool(head.fortran_order), name
    _assert_volume(got, new, name)


# ---- indices -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,dtype,order", [pv.GEOMETRIES[i] for i in (0, 2, 4)], ids=[pv.GEOMETRY_IDS[i] for i in (0, 2, 4)])
def test_stepped_and_int_indices(shape, dtype, order, checker):
  vol, src = pv.volume(shape, dtype, order), pv.other(shape, dtype, order)
  binary = checker.compress(vol)
  arr = crackle_amd.CrackleArray(binary)
  sx, sy, sz = shape
  for idx, data in (
    (S[3:90:4, ::3, 1::2], src[3:90:4, ::3, 1::2]), (S[3:90:4, ::3, 1::2], 9), (S[5, :, 2], src[5, :, 2]), (S[..., 0], src[0, :, 0]),
    (S[-1], src[4, :, :1]), (S[::2, 7], src[::2, 7, :]), (S[1:80:5, 2, ::4], src[1:80:5, 3:4, 0]), (S[::50, ::50, ::50], [[[1]]]), (S[2:3, 4:5, ::2], True),
  ):
    new = pv.edited(vol, idx, data)
    got = arr.paste(idx, data)
    assert isinstance(got, crackle_amd.CrackleArray) and got.shape == arr.shape and got.dtype == arr.dtype
    _assert_volume(got.binary, new, idx)


@pytest.mark.parametrize("shape,dtype,order", pv.GEOMETRIES, ids=pv.GEOMETRY_IDS)
def test_paste_of_a_cutout_is_the_identity(shape, dtype, order, checker):
  vol = pv.volume(shape, dtype, order)
  binary = checker.compress(vol)
  head = crackle_amd.header(binary)
  sx, sy, sz = shape
  for idx in (S[1:sx - 1, 2:9, 1:3], S[:, :, 0], S[sx - 5:, :, sz - 1:], S[3:30:4, ::3, 1::2], S[4, 5, 2], S[2:20, 3:9, :], S[...]):
    got = crackle_amd.paste(binary, idx, crackle_amd.cutout(binary, idx))
    _assert_volume(got, vol, idx)
    if _splices(idx, shape, head):
      assert got == binary, idx
  assert _splices(S[:, :, 0], shape, head) and not _splices(S[...], shape, head)


# ---- a damaged slice ---------------------------------------------------------------------------------------

def test_a_damaged_slice_inside_and_outside_the_range():
  """The stored crc of slice 3 is changed.  A paste whose z-range holds the slice raises what the decode raises; one
  that leaves it out succeeds and copies the slice, wrong crc and all, as zsplit copies it."""
  vol = SMALL["c0_voronoi_u8"][0]
  good = golden()["c0_voronoi_u8"]
  sz = vol.shape[2]
  bad = bytearray(good)
  bad[len(good) - 4 * sz + 4 * 3] ^= 0x10
  bad = bytes(bad)
  assert crackle_amd.check(bad)["z"] == [3]
  with pytest.raises(RuntimeError) as info:
    crackle_amd.decompress(bad)
  message = str(info.value)
  assert "z=3" in message
  for idx in (S[1:5, 1:5, 2:5], S[60:, 60:, 3], S[0, 0, :]):
    with pytest.raises(RuntimeError) as got:
      crackle_amd.paste(bad, idx, 1)
    assert type(got.value) is type(info.value) and str(got.value) == message, idx
  for idx in (S[1:5, 1:5, 6:9], S[:, :, 4], S[10:20, :, :3]):
    z0, z1, _, _ = normalize_index(idx, vol.shape)[2]
    new = pv.edited(vol, idx, 1)
    got = crackle_amd.paste(bad, idx, 1)
    assert crackle_amd.check(got)["z"] == [3]
    assert np.array_equal(codec.crack_crcs(got)[[z for z in range(sz) if not z0 <= z < z1]], codec.crack_crcs(bad)[[z for z in range(sz) if not z0 <= z < z1]])
    assert np.array_equal(crackle_amd.cutout(got, S[:, :, z0:z1]), new[:, :, z0:z1])
    assert np.array_equal(crackle_amd.decompress_range(got, 4, sz), new[:, :, 4:])
    assert np.array_equal(crackle_amd.decompress_range(got, 0, 3), new[:, :, :3])
