"""The catalogue of the threaded tests (tests/thread_jobs.py) is sound, without a GPU: its expected values agree
wherever two independent sources give them, its LDS pairs straddle by the restated host rules, its schedule puts every
pair side by side, its inputs use more slice sizes than geom_table keeps tables, and every call of the "refused" kind
is refused on the host, with its exact text, on a machine that may have no device at all."""
import functools

import numpy as np

import crackle_amd
import stream_kinds as sk
import thread_jobs as tj


@functools.lru_cache(maxsize=None)
def _checker():
  from oracle import oracle
  return oracle.best()


@functools.lru_cache(maxsize=None)
def _catalogue():
  return tj.catalogue(_checker())


def test_the_catalogue_has_every_kind_and_never_asks_the_library():
  from crackle_amd import _lib
  loaded = _lib._lib is not None
  K = _catalogue()
  assert loaded or _lib._lib is None
  assert set(tj.SCHEDULED) | {"tiny-voxel_counts"} == set(K) and len(tj.SCHEDULED) == len(set(tj.SCHEDULED)) == 31
  assert set(tj.COLD) <= set(K)
  for name, inputs in K.items():
    assert len(inputs) >= 2, name
    assert name == "tiny-voxel_counts" or len({i.name for i in inputs}) == len(inputs), name


def test_streams_from_the_checker_decode_to_the_numpy_volumes():
  """Every expected stream (compress, recompress, erode, dilate, reencode, fastcrackle.compress) against the volume numpy says it holds."""
  n = 0
  for name, inputs in _catalogue().items():
    for i in inputs:
      if i.volume is None:
        continue
      assert isinstance(i.want, bytes), (name, i.name)
      got = sk.decode(_checker(), i.want)
      assert got.dtype == i.volume.dtype and np.array_equal(got, i.volume), (name, i.name)
      n += 1
  assert n >= 22


def test_statistics_agree_between_numpy_and_the_checker():
  K, chk = _catalogue(), _checker()
  V = tj.volumes()
  for i, name in zip(K["voxel_counts"], ("cells", "a")):
    b = chk.compress(V[name])
    assert i.want == chk.voxel_counts(b), name
    assert sum(i.want.values()) == V[name].size
  for i, name in zip(K["centroids"], ("cells", "a")):
    ref = chk.centroids(chk.compress(V[name]))
    assert sorted(ref) == sorted(i.want) and all(np.array_equal(ref[l], i.want[l]) for l in ref), name
  for i, name in zip(K["bounding_boxes"], ("cells", "a")):
    assert {l: [int(v) for v in box] for l, box in chk.bounding_boxes(chk.compress(V[name])).items()} == i.want, name
  for i, name in zip(K["point_cloud"], ("planes", "a")):
    assert sorted(i.want) == sorted(l for l in np.unique(V[name]).tolist() if l != 0), name
  for i, (name, c) in zip(K["voxel_connectivity_graph"], (("a", 4), ("s", 6))):
    assert np.array_equal((i.want[:-1] & 1) != 0, V[name][:-1] == V[name][1:]), name      # the +x bit: FLAT streams of the checker have no false boundaries
  for i, name in zip(K["overlaps"], ("a", "s")):
    assert sum(i.want.values()) == V[name].size
    assert {a for a, _ in i.want} == set(np.unique(V[name]).tolist())
  for i in K["mode_pooling_2x2x1"]:
    assert all(crackle_amd.header(b).sz == 1 for b in i.want) and len(i.want) in (7, 5)
  for i, name in zip(K["decompress-label"], ("a", "s")):
    assert i.want.dtype == bool and i.want.any() and not i.want.all(), name
  assert K["array_equal"][0].want is True and K["array_equal"][1].want is False
  assert not np.array_equal(V["s"], sk.other_of(V["s"]))


def test_the_decode_inputs_take_the_paths_their_kinds_name():
  """decoder_build: the strip path needs F order and sx % 4 == 0."""
  V = tj.volumes()
  for n in ("s", "t"):
    assert V[n].flags.f_contiguous and V[n].shape[0] % 4 == 0
  assert V["a"].shape[0] % 4 != 0 and not V["b"].flags.f_contiguous
  heads = [crackle_amd.header(_checker().compress(V[n], markov_model_order=m)) for n, m in (("a", 5), ("s", 3))]
  assert [h.markov_model_order for h in heads] == [5, 3]
  pins = crackle_amd.header(_checker().compress(V["deep"], allow_pins=True))
  assert pins.label_format != crackle_amd.LabelFormat.FLAT, "the pin stage's volume has to end in a pin stream"
  assert len(np.unique(V["deep"])) >= 64, "the per-label regions of the pin stage split over threads from 64 labels on (grain 32)"


def test_every_lds_pair_straddles():
  """One input above 64 KiB, where only a raised limit lets the kernel start, the other where no limit is ever asked
  for (48 KiB: allow_dynamic_lds returns at once), and a few KiB wherever the code can ask for so little."""
  V = tj.volumes()
  sides = tj.lds_sides(V)
  assert set(sides) == {"k_trail_walk", "k_trail_components", "k_trail_emit", "k_slice_resolve_enc", "k_run_stats", "k_trace_contours", "k_markov_hist"}
  for kernel, (large, small) in sides.items():
    print(kernel, large, small)
    assert large is not None and small is not None, kernel
    assert tj.LDS_LINE < large <= tj.MAX_LDS or (kernel == "k_markov_hist" and large == tj.LDS_LINE), (kernel, large)
    assert small <= 48 * 1024, (kernel, small)
    if kernel != "k_slice_resolve_enc":      # (its first table is the 40 KiB the label stream has beside two walks, whatever the slice)
      assert small <= tj.LDS_SMALL, (kernel, small)
  # the volumes are encoded with the cracks the rules above count
  for n in ("cells64", "stripes", "dots", "a8", "a64", "halves", "halves64"):
    assert tj.is_impermissible(V[n]), n
    assert crackle_amd.header(_checker().compress(V[n])).crack_format == crackle_amd.CrackFormat.IMPERMISSIBLE, n
  assert max(v.size for v in V.values()) < 1 << 20 and max(v.shape[2] for v in V.values()) <= 7


def test_the_schedule_covers_every_pair():
  n = len(tj.SCHEDULED)
  rounds = tj.schedule(n)
  assert all(len(jobs) == tj.THREADS for jobs in rounds)
  assert all(0 <= k < n and first in (0, 1) for jobs in rounds for k, first in jobs)
  want = {(a, b) for a in range(n) for b in range(a, n)}
  assert tj.pairs_of(rounds) == want and len(want) == n * (n + 1) // 2
  # a kind beside itself starts on two different inputs
  for jobs in rounds:
    for i in range(len(jobs)):
      for j in range(i + 1, len(jobs)):
        assert jobs[i] != jobs[j]
  assert len(rounds) <= n * (n + 1) // 2 // 4, "greedy, not one round per pair"
  print(len(rounds), "rounds")


def test_more_slice_sizes_than_geom_tables():
  sizes = {px for inputs in _catalogue().values() for i in inputs for px in i.slice_pixels}
  assert len(sizes) > 4, sizes
  scheduled = {px for name in tj.SCHEDULED for i in _catalogue()[name] for px in i.slice_pixels}
  assert len(scheduled) > 4


def test_every_refused_input_is_refused_on_the_host():
  """Run here, where there may be no device: the exact text, not "no usable HIP device", so the call ended in the host's parse."""
  for i in _catalogue()["refused"]:
    assert isinstance(i, tj.Refused)
    assert i.run() == (True, ""), i.name
  texts = [i.want[1] for i in _catalogue()["refused"]]
  assert len(set(texts)) >= 5
  assert not any("HIP" in t for t in texts)
