"""The packed-word arithmetic of k_trail_emit (crackle_amd/csrc/ckl_code_words.hpp) on the host: the header compiles as
plain C++, tests/code_words_check.cpp sets both helpers against a byte per code point — place_codes128 for every
length 1 .. 64 at all 16 alignments, packed_code_diff behind every top code 0 .. 3 of the word in front and over
strings of 1 .. 64 code points."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "crackle_amd", "csrc")


def test_code_word_helpers_against_bytes(tmp_path):
  cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
  if not cxx:
    pytest.fail("no host C++ compiler")
  exe = str(tmp_path / "code_words_check")
  subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(HERE, "code_words_check.cpp"), "-o", exe], check=True)
  r = subprocess.run([exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.startswith("ok "), r.stdout
