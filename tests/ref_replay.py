"""TEST INFRASTRUCTURE: the compiled reference's answers to the calls the live-reference tests make,
kept as data so that those tests run where oracle/_ref could not be built (the reference's sources
are not part of this repository).

  tests/golden/ref_calls.pkl.xz   {key: ("ok", result) | ("err", message)}, pickled, xz-compressed

The key is a digest of the method name and every argument (arrays by dtype, shape, memory order and
bytes), so a replayed call answers only for exactly the inputs that were recorded; any other call
fails.  Regenerate with the compiled reference present:

  CKL_REF_RECORD=1 python -m pytest tests/test_oracle.py -q
"""
import hashlib
import lzma
import os
import pickle

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls.pkl.xz")


def _feed(h, v):
  if isinstance(v, np.ndarray):
    h.update(b"nd:%s:%r:%d%d:" % (v.dtype.str.encode(), v.shape, v.flags.f_contiguous, v.flags.c_contiguous))
    h.update(v.tobytes(order="A"))
  elif isinstance(v, (bytes, bytearray, memoryview)):
    h.update(b"by:%d:" % len(bytes(v)))
    h.update(bytes(v))
  elif isinstance(v, (list, tuple)):
    h.update(b"seq%d(" % len(v))
    for x in v:
      _feed(h, x)
    h.update(b")")
  elif isinstance(v, dict):
    h.update(b"map%d(" % len(v))
    for k in sorted(v):
      _feed(h, k)
      _feed(h, v[k])
    h.update(b")")
  else:
    h.update(b"%s:%s;" % (type(v).__name__.encode(), repr(v).encode()))


def key(method, args, kwargs):
  h = hashlib.sha256(method.encode() + b"|")
  _feed(h, list(args))
  _feed(h, dict(kwargs))
  return h.hexdigest()


class RecordingReference:
  """Wraps the live reference: every call goes through and its answer is kept for save()."""

  def __init__(self, live):
    self._live, self._calls = live, {}

  def __getattr__(self, name):
    fn = getattr(self._live, name)
    if not callable(fn):
      return fn

    def call(*args, **kwargs):
      k = key(name, args, kwargs)
      try:
        out = fn(*args, **kwargs)
      except RuntimeError as exc:
        self._calls[k] = ("err", str(exc))
        raise
      self._calls[k] = ("ok", out)
      return out
    return call

  def save(self, path=PATH):
    with lzma.open(path, "wb", preset=9 | lzma.PRESET_EXTREME) as f:
      pickle.dump(self._calls, f, protocol=4)


class RecordedReference:
  """Answers the recorded calls as the live reference did, error messages included."""

  def __init__(self, path=PATH):
    with lzma.open(path, "rb") as f:
      self._calls = pickle.load(f)

  def __getattr__(self, name):
    if name.startswith("_"):
      raise AttributeError(name)

    def call(*args, **kwargs):
      k = key(name, args, kwargs)
      assert k in self._calls, f"reference call {name}() with these arguments was never recorded: regenerate {os.path.basename(PATH)} (see tests/ref_replay.py)"
      status, out = self._calls[k]
      if status == "err":
        raise RuntimeError(out)
      return out
    return call
