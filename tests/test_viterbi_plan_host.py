"""CPU (no GPU): the launch policy of gsw_viterbi_decode swept by a host-only program (tests/viterbi_plan_cases.cpp over csrc/gswm_viterbi_plan.h), and the C
entry point's refusals, every one of them before any launch."""
import ctypes
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
    exe = tmp_path_factory.mktemp("viterbi_plan") / "viterbi_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "viterbi_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Every refusal has the status the specification gives it, BAD_ARG before UNSUPPORTED, and decides nothing.  For every accepted input: T = M / 2, I = T - 6,
    M / 16 info bytes of which M / 16 - 3 are payload; S is odd, coprime to M and the smallest such from isqrt(M) | 1 on, Sinv its inverse, and the kernel's index
    products fit 32 bits; a wave's LDS slice holds its five rows and is 16-byte aligned, the workgroup's slices fit 96 KiB; 1, 2 or 4 waves, filled by the
    batch and the most that fit; the grid covers every image once."""
    words = sweep.stderr.split()
    assert int(words[0]) > 500000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_every_path(sweep):
    seen = set(sweep.stderr.split()[4:])
    want = {"bad_arg", "unsupported", "waves1", "waves2", "waves4", "step_moved_on", "waves_cut_by_lds", "waves_cut_by_batch"}
    assert seen >= want, want - seen


def test_the_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)      # never dereferenced: every call below is refused before a launch

    def call(score=p, stride=256, B=1, M=256, info=p, message=p, metric=p, flips=p, ok=p):
        return lib.gsw_viterbi_decode(score, stride, B, M, info, message, metric, flips, ok, None)

    for kw in (dict(score=None), dict(info=None), dict(message=None), dict(metric=None), dict(flips=None), dict(ok=None), dict(score=odd), dict(metric=odd),
               dict(flips=odd), dict(ok=odd), dict(B=0), dict(B=-3), dict(M=48, stride=48), dict(M=0), dict(M=264, stride=264), dict(M=250), dict(stride=255),
               dict(stride=0), dict(M=8208, stride=8208, B=0), dict(M=8208, stride=100)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(M=8208, stride=8208), dict(M=16384, stride=16384), dict(M=1 << 20, stride=1 << 20)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw
