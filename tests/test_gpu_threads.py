"""The library under concurrent host threads: python -m thread_jobs (tests/thread_jobs.py) in a fresh child process per
scenario, four threads inside libcrackle_amd.so at once, every result compared in the thread with an expectation that
was there before the threads started, and the same child with one thread as the control.

  cold      four threads make the process's first library calls at the same time (compress, decompress, voxel_counts,
            fastcrackle.compress), then run their kind's inputs eight times
  pairs     the schedule: every pair of the 31 job kinds, and every kind beside itself on its two inputs, shares a
            round of eight calls per thread behind a barrier
  sessions  four threads create and destroy 200 decode sessions each while a fifth encodes and decodes

One child at a time; a child that is killed by its time limit or dies of a signal fails its test and every later test
of the module without another child being started.

The time limits are ten times the child's single-threaded duration on an MI355X: 2.0 s of interpreter start and
imports in front of every child, then the scenario itself (catalogue, first use of the device and the calls): cold
0.57 s, pairs 6.16 s, sessions 0.46 s with one thread; 0.49 s, 4.76 s and 0.59 s with four.  A call takes 0.4 ms
(voxel_connectivity_graph, decompress) to 21 ms (compress of the volume that repeats the label stage's resolve)."""
import functools
import json
import os
import subprocess
import sys

import pytest

import thread_jobs as tj

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = {"cold": 26, "pairs": 82, "sessions": 25}      # seconds: ten times (2.0 + 0.57), (2.0 + 6.16), (2.0 + 0.46)
DEAD = []      # why no further child may start


@functools.lru_cache(maxsize=None)
def child(scenario, threads):
  if DEAD:
    pytest.fail(f"not started: {DEAD[0]}")
  cmd = [sys.executable, "-m", "thread_jobs", scenario, str(threads)]
  try:
    p = subprocess.run(cmd, cwd=HERE, capture_output=True, text=True, timeout=TIMEOUT[scenario])
  except subprocess.TimeoutExpired as e:
    DEAD.append(f"{scenario} with {threads} threads was killed after {TIMEOUT[scenario]} s (a deadlock, or a hang on the device)")
    pytest.fail(DEAD[0] + "\n" + str(e.stderr or "")[-4000:])
  if p.returncode < 0:
    DEAD.append(f"{scenario} with {threads} threads died of signal {-p.returncode}")
    pytest.fail(DEAD[0] + "\n" + p.stderr[-4000:])
  assert p.returncode == 0, p.stderr[-6000:]
  doc = json.loads(p.stdout.strip().splitlines()[-1])
  assert doc["scenario"] == scenario and doc["threads"] == threads
  print(f"{scenario} with {threads} thread(s): {doc['seconds']:.2f} s, {len(doc['records'])} calls")
  return doc


def wrong(doc):
  return [r for r in doc["records"] if not r[6]]


def results(doc):
  """What the records say apart from when: (round, slot, kind, input, ok, text), sorted."""
  return sorted((r[0], r[1], r[2], r[3], r[6], r[7]) for r in doc["records"])


def overlap(recs_a, recs_b):
  """Some call of the one was inside the library while some call of the other was."""
  return any(max(a[4], b[4]) < min(a[5], b[5]) for a in recs_a for b in recs_b)


def test_the_restated_rules_hold_on_this_device():
  """thread_jobs restates the host rules for 160 KiB of LDS per workgroup; tests/test_gpu_consumer_edges.py reads the
  device and restates two of them as well."""
  import test_gpu_consumer_edges as edges
  assert edges._max_lds() == tj.MAX_LDS
  V = tj.volumes()
  for n in ("planes", "a"):
    sx, sy = V[n].shape[:2]
    assert edges.pc_lds_visited(sx, sy) == (tj.contour_visited_lds(sx, sy) is not None) is True
  for comps in (4624, 19, 4521, 4522, 4523):
    assert edges.stats_lds_comps(comps) * 36 == tj.stats_lds(comps)


def test_cold_start():
  doc = child("cold", tj.THREADS)
  assert not wrong(doc), wrong(doc)[:8]
  by_slot = {s: [r for r in doc["records"] if r[1] == s] for s in range(tj.THREADS)}
  assert [by_slot[s][0][2] for s in range(tj.THREADS)] == tj.COLD
  assert all(len(by_slot[s]) >= 1 + 2 * tj.CALLS_PER_ROUND for s in by_slot)
  # the first calls themselves met: each thread's first call began before every other thread's first call had ended
  first = [by_slot[s][0] for s in range(tj.THREADS)]
  assert max(r[4] for r in first) < min(r[5] for r in first), [(r[2], r[4], r[5]) for r in first]
  for a in range(tj.THREADS):
    for b in range(a + 1, tj.THREADS):
      assert overlap(by_slot[a], by_slot[b]), (a, b)
  control = child("cold", 1)
  assert results(control) == results(doc)


def test_all_pairs():
  doc = child("pairs", tj.THREADS)
  bad = wrong(doc)
  assert not bad, (len(bad), bad[:8])
  rounds = tj.schedule(len(tj.SCHEDULED))
  assert len(doc["records"]) == len(rounds) * tj.THREADS * tj.CALLS_PER_ROUND
  refused = [r for r in doc["records"] if r[2] == "refused"]
  assert refused and all(r[6] and r[7] == "" for r in refused)      # every refused call raised exactly its own text
  by = {}
  for r in doc["records"]:
    by.setdefault((r[0], r[1]), []).append(r)
  met, missed = set(), []
  for ri, jobs in enumerate(rounds):
    for i in range(len(jobs)):
      for j in range(i + 1, len(jobs)):
        a, b = sorted((jobs[i][0], jobs[j][0]))
        if (a != b or jobs[i][1] != jobs[j][1]) and overlap(by[(ri, i)], by[(ri, j)]):
          met.add((a, b))
  for pair in sorted(tj.pairs_of(rounds)):
    if pair not in met:
      missed.append((tj.SCHEDULED[pair[0]], tj.SCHEDULED[pair[1]]))
  assert not missed, f"{len(missed)} pairs never overlapped: {missed[:10]}"
  # a kind beside itself ran its two inputs at the same time at least once
  for ri, jobs in enumerate(rounds[:(len(tj.SCHEDULED) + 1) // 2]):
    for i, j in ((0, 1), (2, 3)):
      assert jobs[i][0] == jobs[j][0]
      assert any(a[3] != b[3] and max(a[4], b[4]) < min(a[5], b[5]) for a in by[(ri, i)] for b in by[(ri, j)]), tj.SCHEDULED[jobs[i][0]]


def test_all_pairs_single_threaded_control():
  """The same child with one thread gives the same results: a failure with four threads is the threads', not the catalogue's."""
  control = child("pairs", 1)
  assert not wrong(control), wrong(control)[:8]
  assert results(control) == results(child("pairs", tj.THREADS))


def test_many_short_sessions():
  doc = child("sessions", tj.THREADS)
  assert not wrong(doc), wrong(doc)[:8]
  short = [r for r in doc["records"] if r[2] == "tiny-voxel_counts"]
  long = [r for r in doc["records"] if r[1] == tj.THREADS]
  assert len(short) == tj.THREADS * 200 and len(long) >= 8
  for s in range(tj.THREADS):
    assert overlap([r for r in short if r[1] == s], long), s
    for t in range(s + 1, tj.THREADS):
      assert overlap([r for r in short if r[1] == s], [r for r in short if r[1] == t]), (s, t)
  control = child("sessions", 1)
  assert not wrong(control)
  assert {(r[2], r[3], r[6], r[7]) for r in control["records"]} == {(r[2], r[3], r[6], r[7]) for r in doc["records"]}
