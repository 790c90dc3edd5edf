"""CPU (no GPU): the launch policy of gsw_viterbi_list_decode swept by a host-only program (tests/viterbi_list_plan_cases.cpp over
csrc/gswm_viterbi_list_plan.h), and the C entry point's refusals, every one of them before any launch."""
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
    exe = tmp_path_factory.mktemp("viterbi_list_plan") / "viterbi_list_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "viterbi_list_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Every refusal has the status the specification gives it, BAD_ARG (the list size included) before UNSUPPORTED, and decides nothing; UNSUPPORTED is exactly
    `M (5 + 1/16 + 9 L / 2) + 256 L`, rounded up to 16, above 163 840.  For every accepted input: the code sizes and the interleaver of section 4.29; every
    list full from step 6 + log2 L on; a wave's slice holds its six rows and is 16-byte aligned, as are the rows read 16 bytes at a time; a workgroup of 2 or 4
    waves stays within 80 KiB, one wave within 160 KiB; the waves are filled by the batch and the most that fit; the grid covers every image once.  Every
    multiple of 16 in 64 .. 2048 is served at every L."""
    words = sweep.stderr.split()
    assert int(words[0]) > 500000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_every_path(sweep):
    seen = set(sweep.stderr.split()[4:])
    want = {"bad_arg", "unsupported", "waves1", "waves2", "waves4", "L1", "L2", "L4", "L8", "waves_cut_by_lds", "waves_cut_by_batch", "lone_wave_above_half",
            "largest1=8256", "largest8=3936"}                      # L = 1 is served to the sweep's end, L = 8 to its bound
    assert seen >= want, want - seen


def test_the_python_restatement_of_the_bound_is_the_plan_s():
    import ecc_list_reference as LR
    from gswm_amd import codec
    assert [LR.largest_served(L) for L in (1, 2, 4, 8)] == [17104, 11600, 7056, 3936]
    for L in (1, 2, 4, 8):
        for M in (64, 80, 2048, LR.largest_served(L), LR.largest_served(L) + 16):
            assert codec.viterbi_list_wave_lds(M, L) == LR.wave_lds(M, L)
            assert (codec.viterbi_list_wave_lds(M, L) <= codec.VITERBI_LIST_LDS) == LR.served(M, L)


def test_the_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)      # never dereferenced: every call below is refused before a launch

    def call(score=p, stride=256, B=1, M=256, L=4, info=p, message=p, metric=p, flips=p, ok=p, rank=p, n_ok=p):
        return lib.gsw_viterbi_list_decode(score, stride, B, M, L, info, message, metric, flips, ok, rank, n_ok, None)

    for kw in (dict(score=None), dict(info=None), dict(message=None), dict(metric=None), dict(flips=None), dict(ok=None), dict(rank=None), dict(n_ok=None),
               dict(score=odd), dict(metric=odd), dict(flips=odd), dict(ok=odd), dict(rank=odd), dict(n_ok=odd), dict(B=0), dict(B=-3), dict(M=48, stride=48),
               dict(M=0), dict(M=264, stride=264), dict(M=250), dict(stride=255), dict(stride=0), dict(L=0), dict(L=3), dict(L=16), dict(L=-1), dict(L=5),
               dict(M=3952, stride=3952, L=8, B=0), dict(M=3952, stride=100, L=8), dict(M=3952, stride=3952, L=16), dict(M=1 << 20, stride=1 << 20, L=7)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(M=3952, stride=3952, L=8), dict(M=7072, stride=7072, L=4), dict(M=11616, stride=11616, L=2), dict(M=17120, stride=17120, L=1),
               dict(M=1 << 20, stride=1 << 20, L=1), dict(M=2147483632, stride=2147483632, L=8)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw
