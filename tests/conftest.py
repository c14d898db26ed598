import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def pytest_configure(config):
  config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def port():
  from oracle import oracle
  return oracle.port()


@pytest.fixture(scope="session")
def ref():
  """The reference compiled in place (oracle/_ref); where it was never built, its recorded answers to
  the same calls (tests/ref_replay.py).  CKL_REF_RECORD=1 records them from the live reference."""
  from oracle import oracle
  import ref_replay
  live = oracle.ref()
  if os.environ.get("CKL_REF_RECORD"):
    assert live is not None, "CKL_REF_RECORD needs the compiled reference (oracle/_ref)"
    rec = ref_replay.RecordingReference(live)
    yield rec
    rec.save()
    return
  yield live if live is not None else ref_replay.RecordedReference()


@pytest.fixture(scope="session")
def checker():
  from oracle import oracle
  return oracle.best()
