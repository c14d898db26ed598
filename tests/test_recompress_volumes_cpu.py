"""The inputs of tests/test_gpu_recompress.py are what they claim to be: checked on the port, without a device, so
that a changed generator cannot quietly blunt a GPU test.  The figures were taken with the port and crackle_amd.synth."""
import numpy as np

import recompress_volumes as rv

PERMISSIBLE, IMPERMISSIBLE = 1, 0


def _crack_format(stream):
  return (int.from_bytes(stream[5:7], "little") >> 4) & 1


def _stored_width(stream):
  return 1 << ((int.from_bytes(stream[5:7], "little") >> 2) & 3)


def _data_width(stream):
  return 1 << (int.from_bytes(stream[5:7], "little") & 3)


def test_voronoi_has_false_boundaries(port):
  lab, merged = rv.VORONOI.volume(), rv.VORONOI.merged()
  assert lab.shape == (72, 64, 6) and lab.dtype == np.uint8
  assert len(port.compress(lab)) == 4222
  assert len(port.compress(merged)) == 4129
  # neighbours that differ before the merge and are equal after it: the cracks a remapped stream keeps
  false_x = np.count_nonzero((lab[1:] != lab[:-1]) & (merged[1:] == merged[:-1]))
  false_y = np.count_nonzero((lab[:, 1:] != lab[:, :-1]) & (merged[:, 1:] == merged[:, :-1]))
  assert false_x > 0 and false_y > 0


def test_noise_flips_its_format_by_the_wrap_pairs(port):
  lab, merged = rv.NOISE_FLIPS.volume(), rv.NOISE_FLIPS.merged()
  assert lab.shape == (130, 70, 4) and lab.dtype == np.uint8 and int(lab.max()) == 3
  assert rv.permissible(lab) and _crack_format(port.compress(lab)) == PERMISSIBLE
  assert merged.size // 2 == 18200
  assert rv.linear_pairs(merged) == 18330
  assert rv.interior_x_pairs(merged) == 18196      # alone they would say PERMISSIBLE
  assert not rv.permissible(merged) and _crack_format(port.compress(merged)) == IMPERMISSIBLE


def test_noise_stays_permissible(port):
  merged = rv.NOISE_STAYS.merged()
  assert rv.linear_pairs(merged) == 18181 and merged.size // 2 == 18200
  assert _crack_format(port.compress(rv.NOISE_STAYS.volume())) == PERMISSIBLE
  assert _crack_format(port.compress(merged)) == PERMISSIBLE


def test_noise_one_pair_over_the_threshold(port):
  lab, merged = rv.NOISE_BY_ONE.volume(), rv.NOISE_BY_ONE.merged()
  assert lab.shape == (97, 61, 7)
  assert merged.size // 2 == 20709
  assert rv.linear_pairs(merged) == 20710      # one missed slice or row wrap pair flips the format
  assert rv.interior_x_pairs(merged) < 20709
  assert _crack_format(port.compress(merged)) == IMPERMISSIBLE


def test_noise_stored_width_shrinks(port):
  lab, merged = rv.NOISE_WIDTH.volume(), rv.NOISE_WIDTH.merged()
  assert lab.dtype == np.uint16 and int(lab.max()) > 255 and int(merged.max()) <= 255
  a, b = port.compress(lab), port.compress(merged)
  assert (_data_width(a), _stored_width(a)) == (2, 2)
  assert (_data_width(b), _stored_width(b)) == (2, 1)


def test_port_round_trip_is_the_identity_on_canonical_streams(port):
  for case in rv.MERGED:
    lab = case.volume()
    for kw in (dict(), dict(markov_model_order=3)):
      b = port.compress(lab, **kw)
      back = port.decompress(b).reshape(lab.shape, order="F")
      assert np.array_equal(back, lab)
      assert port.compress(np.asfortranarray(back), **kw) == b


def test_floordiv_stream_keeps_duplicates(port):
  lab = rv.VORONOI.volume()
  b = rv.floordiv_stream(port.compress(lab))
  import crackle_amd
  u = crackle_amd.labels(b)
  assert len(np.unique(u)) < len(u)
  assert np.array_equal(port.decompress(b).reshape(lab.shape, order="F"), lab // 2)
