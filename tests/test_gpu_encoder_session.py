"""One encode session driven through its single-use caches, in one process: the label planes that ckl_encoder_stats
leaves for the run that follows, the crack trail that ckl_encoder_markov_stats leaves beside them, and the run that
packs that trail under a forced model (the sharded encoder's sequence: stats -> markov_hist -> encode with the agreed
formats and model).  Every stream is compared, byte for byte, with the one-shot encode of the same volume and options
by a fresh session (test_gpu_parity.py pins that one to the reference; the unforced ones are checked against the
checker here as well).

Volumes: 96 x 80 x 6 (the vectorised planes kernel) and 100 x 80 x 3 (100 is no multiple of 4 uint32 labels: the
generic one), Voronoi cells (few crack edges: most neighbours are equal, so the volume chooses IMPERMISSIBLE) and
noise (nearly every edge a crack: PERMISSIBLE), markov orders 1 and 3."""
import functools

import numpy as np
import pytest
import torch

from crackle_amd import distributed as ckd
from crackle_amd import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PERMISSIBLE, IMPERMISSIBLE, FLAT = 1, 0, 0

SHAPES = [(96, 80, 6), (100, 80, 3)]
KINDS = ["voronoi", "noise"]
ORDERS = [1, 3]
CASES = [(s, k, o) for s in SHAPES for k in KINDS for o in ORDERS]
IDS = [f"{'x'.join(map(str, s))}-{k}-m{o}" for s, k, o in CASES]
parametrize = pytest.mark.parametrize("shape,kind,order", CASES, ids=IDS)


@functools.lru_cache(maxsize=None)
def _volume(shape, kind):
  """(device tensor, numpy view): never written to (the tests encode clones)."""
  if kind == "voronoi":
    t = synth.voronoi_labels(shape, np.uint32, seed=23, cell=(16, 16, 4), device=DEV)
  else:
    t = synth.random_labels_device(shape, np.uint32, seed=29, high=2000, device=DEV)
  return t, synth.as_numpy_f(t)


def _natural(shape, kind):
  """The formats an unforced encode of the volume chooses (crackle.hpp:50-64, 233-235; no pins here)."""
  arr = _volume(shape, kind)[1]
  f = arr.reshape(-1, order="F")
  pairs = int(np.count_nonzero(f[1:] == f[:-1]))
  crack = PERMISSIBLE if pairs < arr.size // 2 else IMPERMISSIBLE
  assert crack == (IMPERMISSIBLE if kind == "voronoi" else PERMISSIBLE)      # the two kinds cover both formats
  mx = int(arr.max())
  return dict(crack_format=crack, label_format=FLAT, stored_width=1 if mx < 256 else 2 if mx < 65536 else 4)


@functools.lru_cache(maxsize=None)
def _hist(shape, kind, order):
  """The volume's markov histogram under its natural crack format, by a fresh session."""
  hist = ckd.HipBackend(0).markov_hist(_volume(shape, kind)[0].clone(), shape, _natural(shape, kind)["crack_format"], order)
  hist.setflags(write=False)
  return hist


def _model(shape, kind, order):
  return ckd.stats_to_model(_hist(shape, kind, order))


@functools.lru_cache(maxsize=None)
def _one_shot(shape, kind, order, forced_crack=None, with_model=False):
  """The reference of every case: a fresh session's only encode."""
  ov = None
  if forced_crack is not None or with_model:
    ov = dict(_natural(shape, kind))
    if forced_crack is not None:
      ov["crack_format"] = forced_crack
    if with_model:
      ov["model"] = _model(shape, kind, order)
  return bytes(ckd.HipBackend(0).encode(_volume(shape, kind)[0].clone(), shape, False, True, order, ov))


def _other(kind):
  return "noise" if kind == "voronoi" else "voronoi"


@parametrize
def test_one_shot_references(shape, kind, order, checker):
  """What the cases below compare with: the unforced one-shot stream is the checker's, and forcing the natural formats
  and the volume's own model changes no byte of it."""
  plain = _one_shot(shape, kind, order)
  assert plain == checker.compress(_volume(shape, kind)[1], markov_model_order=order)
  assert _one_shot(shape, kind, order, with_model=True) == plain
  assert _one_shot(shape, kind, order, _natural(shape, kind)["crack_format"]) == plain


@parametrize
def test_stats_hist_encode_then_another_volume(shape, kind, order):
  """(a) stats -> markov_hist -> encode with the natural formats and the histogram's model: cached planes, cached
  trail.  (b) the same session at once encodes other voxels at the same address, unforced: nothing of (a) is left."""
  be = ckd.HipBackend(0)
  vol = _volume(shape, kind)[0].clone()
  arr = _volume(shape, kind)[1]
  nat = _natural(shape, kind)
  mx, pairs, first, last = be.stats(vol, shape)
  f = arr.reshape(-1, order="F")
  assert (mx, first, last) == (int(arr.max()), int(f[0]), int(f[-1]))
  assert (PERMISSIBLE if pairs < arr.size // 2 else IMPERMISSIBLE) == nat["crack_format"]
  hist = be.markov_hist(vol, shape, nat["crack_format"], order)
  assert np.array_equal(hist, _hist(shape, kind, order))
  got = bytes(be.encode(vol, shape, False, True, order, dict(nat, model=ckd.stats_to_model(hist))))
  assert got == _one_shot(shape, kind, order, with_model=True)
  assert got == _one_shot(shape, kind, order)
  # (b)
  vol.copy_(_volume(shape, _other(kind))[0])
  torch.cuda.synchronize()
  assert bytes(be.encode(vol, shape, False, True, order, None)) == _one_shot(shape, _other(kind), order)


@parametrize
def test_hist_without_stats_then_plain_encode(shape, kind, order):
  """(c) no planes are cached, so markov_hist keeps no trail either; the encode that follows builds everything."""
  be = ckd.HipBackend(0)
  vol = _volume(shape, kind)[0].clone()
  hist = be.markov_hist(vol, shape, _natural(shape, kind)["crack_format"], order)
  assert np.array_equal(hist, _hist(shape, kind, order))
  assert bytes(be.encode(vol, shape, False, True, order, None)) == _one_shot(shape, kind, order)
  # ... and the same with a forced model: overrides alone reuse nothing either
  hist = be.markov_hist(vol, shape, _natural(shape, kind)["crack_format"], order)
  got = bytes(be.encode(vol, shape, False, True, order, dict(_natural(shape, kind), model=ckd.stats_to_model(hist))))
  assert got == _one_shot(shape, kind, order, with_model=True)


@parametrize
def test_stats_then_the_other_crack_format(shape, kind, order):
  """(d) the planes of stats are reused under overrides that force the crack format the volume would not choose: the
  graph is built for the forced format (device and host agree, or the run fails)."""
  be = ckd.HipBackend(0)
  vol = _volume(shape, kind)[0].clone()
  nat = _natural(shape, kind)
  forced = PERMISSIBLE + IMPERMISSIBLE - nat["crack_format"]
  be.stats(vol, shape)
  got = bytes(be.encode(vol, shape, False, True, order, dict(nat, crack_format=forced)))
  assert got == _one_shot(shape, kind, order, forced)
  assert got != _one_shot(shape, kind, order)
  # the trail that markov_hist leaves for the natural format does not serve the other one
  be.stats(vol, shape)
  be.markov_hist(vol, shape, nat["crack_format"], order)
  hist = ckd.HipBackend(0).markov_hist(vol, shape, forced, order)
  got = bytes(be.encode(vol, shape, False, True, order, dict(nat, crack_format=forced, model=ckd.stats_to_model(hist))))
  assert got == _one_shot(shape, kind, order, forced)


@parametrize
def test_hist_of_one_order_then_encode_of_another(shape, kind, order):
  """(e) stats -> markov_hist with the other order -> encode with `order` and its own model: the cached trail was made
  for another order and is rebuilt."""
  be = ckd.HipBackend(0)
  vol = _volume(shape, kind)[0].clone()
  nat = _natural(shape, kind)
  be.stats(vol, shape)
  other = ORDERS[1 - ORDERS.index(order)]
  assert np.array_equal(be.markov_hist(vol, shape, nat["crack_format"], other), _hist(shape, kind, other))
  got = bytes(be.encode(vol, shape, False, True, order, dict(nat, model=_model(shape, kind, order))))
  assert got == _one_shot(shape, kind, order, with_model=True)
