"""CPU (no GPU): the launch policy of the tamper family is pure functions of one header (csrc/gswm_tamper_plan.h: tile_decide for the tile map and the
tile-weighted vote, robust_decide for the one-launch robust decode, all three on one geometry), and the square root of the robust decode's weight rule
(robust_isqrt) is the one the kernel calls.  tests/tamper_plan_cases.cpp, a host-only program, sweeps them and prints every input whose decision breaks an
invariant of a launch that no kernel checks, every refusal that does not come with its status and a decision of zeros, and every value whose root is not the
exact floor."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("tamper_plan") / "tamper_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tamper_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Robust decode: LDS <= 131 072 bytes; the row, the planes, the weights, the tiles' sums of levels and of squares and the message bytes lie in it in that
    order, disjoint and dword-aligned; the geometry is the lattice's; S lanes per message bit leave a wave whole bytes; every refusal has the status the
    specification gives it (in the order BAD_ARG, lattice, RAGGED, rounds) and decides nothing; for every accepted input the largest weight, vote, score and sum of
    squares, computed in 64 bits, fit int32; isqrt(v)^2 <= v < (isqrt(v) + 1)^2 over 0..2^24, at 15^2 x 16384, at 2^31 - 1 and 2^32 - 1, at every square past 2^24
    and its neighbours.  Map and vote, on the same grid: the status restated (own pointers, packed / keys, sizes, l, alignment, tile, lattice, row, RAGGED, the
    vote's copies x 65535 <= 2^31 - 1, and the order when an input breaks several); LDS == 64 nblk <= 131 072; the geometry that of the robust decision."""
    words = sweep.stderr.split()
    assert int(words[0]) > 1000000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"
    assert int(words[4]) > (1 << 24) + 3 * 61000 and words[5] == "roots,"


def test_the_sweep_reaches_every_refusal_and_every_lane_count(sweep):
    """vote_int32: the vote refused for copies x 65535 > 2^31 - 1; vote_at_int32: accepted at 32 768 copies, the last that fit"""
    seen = set(sweep.stderr.split()[6:])
    assert seen == {"ok", "lattice", "row", "ragged", "planes", "int32", "lds", "s0", "s1", "s2", "s3", "vote_int32", "vote_at_int32"}, seen
