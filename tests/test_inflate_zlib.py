"""The streaming zlib inflate without a device: inflate_zlib of mgp_inflate_core.h run on the
host under the sanitizers (tests/inflate_zlib_main.cpp, a stand-alone program, a child
process) over the corpus of tests/zlib_corpus.py."""

import shutil
import subprocess
from pathlib import Path

import pytest

import inflate_corpus as ic
import zlib_corpus as zc

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def zlib_program(tmp_path_factory):
    """tests/inflate_zlib_main.cpp with mgp_inflate_core.h, -fsanitize=address,undefined."""
    exe = tmp_path_factory.mktemp("inflate_zlib") / "inflate_zlib_main"
    cxx = shutil.which("g++") or "c++"
    # (the sanitizers' runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", f"-I{ROOT / 'mgatk2_amd' / 'csrc'}",
                    str(ROOT / "tests" / "inflate_zlib_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run_program(exe, cases, tmp_path, name):
    path = tmp_path / f"{name}.bin"
    ic.write_corpus_file(path, cases)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-3000:], r.stderr[-3000:])
    assert f"{len(cases)} cases" in r.stdout and " 0 failed" in r.stdout, r.stdout[-2000:]


def test_valid_streams_bit_equal(zlib_program, tmp_path):
    """Every valid stream (levels 0, 1, 4, 9, the three strategies, the sizes around the ring's
    half and whole, zeros, counts and noise, the far match across the ring's wrap, every
    header window size) gives status 0 and zlib's bytes."""
    cases = list(zc.valid_cases()) + list(zc.padded_cases())
    names = {c[0] for c in cases}
    assert len(cases) > 115 and {"zero262144_l9", "noise65537_l0", "rle200000", "wbits9", "far_match_wrap"} <= names
    run_program(zlib_program, cases, tmp_path, "valid")


def test_invalid_streams_give_their_status(zlib_program, tmp_path):
    """Bad CM, CINFO 8, FDICT and a bad FCHECK are invalid (1), a cut trailer and an output one
    byte short or long are size errors (2), a wrong Adler-32 and a trailing byte are check
    errors (3), a distance before the start is invalid (1)."""
    cases = list(zc.invalid_cases())
    assert [c[3] for c in cases] == [1, 1, 1, 1, 2, 2, 3, 3, 2, 2, 1]
    run_program(zlib_program, cases, tmp_path, "invalid")


def test_mutations_follow_zlib(zlib_program, tmp_path):
    """20,000 single-byte and single-bit mutations of the valid streams: no sanitizer report,
    status 0 exactly when zlib yields exactly isize bytes with eof and nothing unused, and then
    the same bytes."""
    cases = zc.mutations(20000)
    n_ok = sum(1 for c in cases if c[3] == ic.OK)
    assert 1000 < n_ok < 19000  # (both verdicts hold more than 5 % of the cases)
    run_program(zlib_program, cases, tmp_path, "mutations")
