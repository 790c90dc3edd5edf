"""CPU (no GPU): the launch policy of gsw_viterbi_decode_rate and gsw_viterbi_list_decode_rate swept by a host-only program
(tests/viterbi_rate_plan_cases.cpp over csrc/gswm_viterbi_rate_plan.h), built plain and with -fsanitize=address,undefined, and the C entry points'
refusals, every one of them before any launch."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def sweep(tmp_path_factory, request):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("viterbi_rate_plan_" + request.param) / "viterbi_rate_plan_cases"
    # the library's compiler on host code only; the library's optimisation level, or the two host sanitizers on a stand-alone program
    flags = ["-O3"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "viterbi_rate_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """N(t) equals a brute-force count and the issue's closed forms.  Every refusal has the status the specification gives it, BAD_ARG (the rate and the list
    size included) before UNSUPPORTED, and decides nothing.  At rate 0 the plan equals viterbi_decide's / viterbi_list_decide's field for field, refusals
    included.  For every accepted input: T the largest multiple of 8 with N(T) <= M, the 2 pad bits, the interleaver of section 4.29; the slice is
    4 M + 9 T + M + T / 8 (plain) or 4 M + 256 L + 9 T L + M + T / 8 (list), rounded up to 16; the plain workgroup within 96 KiB, list workgroups of 2 or 4
    waves within 80 KiB and one wave within 160 KiB; the waves filled by the batch and the most that fit; the grid covers every image once.  Every multiple
    of 16 in 64 .. 2048 is served at every L and rate, and every M up to 8192 by the plain read."""
    words = sweep.stderr.split()
    assert int(words[0]) > 5000000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_every_path(sweep):
    seen = set(sweep.stderr.split()[4:])
    want = {"bad_arg", "unsupported_plain", "unsupported_list", "waves1", "waves2", "waves4", "plain", "L1", "L2", "L4", "L8", "rate0", "rate1", "rate2", "spare",
            "tail_inside_a_period", "entry_inside_a_period", "plain_lds_near_the_limit", "lone_wave_above_half",
            "plain0=8192", "plain1=8192", "plain2=8192", "list0_8=3936", "list1_8=3040", "list2_8=2736"}
    assert seen >= want, want - seen


def test_the_python_restatements_of_the_bound_are_the_plan_s():
    import ecc_list_reference as LR
    import ecc_rate_reference as Q
    from gswm_amd import codec
    assert [[Q.largest_served(L, c) for L in (1, 2, 4, 8)] for c in Q.CODES] == [[17104, 11600, 7056, 3936], [14752, 9552, 5600, 3040], [13808, 8784, 5072, 2736]]
    assert Q.plain_wave_lds(8192, "conv34") == 97024 <= 96 * 1024
    for c in Q.CODES:
        for L in (1, 2, 4, 8):
            for M in (64, 80, 2048, Q.largest_served(L, c), Q.largest_served(L, c) + 16):
                assert codec.viterbi_list_wave_lds(M, L, c) == Q.list_wave_lds(M, L, c)
                assert (codec.viterbi_list_wave_lds(M, L, c) <= codec.VITERBI_LIST_LDS) == Q.served(M, L, c)
                if c == "conv":
                    assert codec.viterbi_list_wave_lds(M, L) == LR.wave_lds(M, L) == Q.list_wave_lds(M, L, c)


def test_the_entry_points_refuse_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)      # never dereferenced: every call below is refused before a launch

    def plain(score=p, stride=256, B=1, M=256, rate=1, info=p, message=p, metric=p, flips=p, ok=p):
        return lib.gsw_viterbi_decode_rate(score, stride, B, M, rate, info, message, metric, flips, ok, None)

    def lst(score=p, stride=256, B=1, M=256, rate=2, L=4, info=p, message=p, metric=p, flips=p, ok=p, rank=p, n_ok=p):
        return lib.gsw_viterbi_list_decode_rate(score, stride, B, M, rate, L, info, message, metric, flips, ok, rank, n_ok, None)

    for kw in (dict(score=None), dict(info=None), dict(message=None), dict(metric=None), dict(flips=None), dict(ok=None), dict(score=odd), dict(metric=odd),
               dict(flips=odd), dict(ok=odd), dict(B=0), dict(B=-3), dict(M=48, stride=48), dict(M=0), dict(M=264, stride=264), dict(stride=255), dict(rate=3),
               dict(rate=-1), dict(rate=3, M=8208, stride=8208), dict(B=0, M=8208, stride=8208)):
        assert plain(**kw) == N.GSW_ERR_BAD_ARG, kw
        assert lst(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(rank=None), dict(n_ok=None), dict(rank=odd), dict(n_ok=odd), dict(L=0), dict(L=3), dict(L=16), dict(L=-1),
               dict(M=2752, stride=2752, L=8, rate=7), dict(M=2752, stride=100, L=8), dict(M=1 << 20, stride=1 << 20, L=7)):
        assert lst(**kw) == N.GSW_ERR_BAD_ARG, kw
    for rate in (0, 1, 2):
        assert plain(M=8208, stride=8208, rate=rate) == N.GSW_ERR_UNSUPPORTED
        assert plain(M=2147483632, stride=2147483632, rate=rate) == N.GSW_ERR_UNSUPPORTED
        assert lst(M=2147483632, stride=2147483632, rate=rate, L=1) == N.GSW_ERR_UNSUPPORTED
    for kw in (dict(M=3056, stride=3056, L=8, rate=1), dict(M=2752, stride=2752, L=8, rate=2), dict(M=5616, stride=5616, L=4, rate=1),
               dict(M=5088, stride=5088, L=4, rate=2), dict(M=9568, stride=9568, L=2, rate=1), dict(M=8800, stride=8800, L=2, rate=2),
               dict(M=14768, stride=14768, L=1, rate=1), dict(M=13824, stride=13824, L=1, rate=2), dict(M=3952, stride=3952, L=8, rate=0)):
        assert lst(**kw) == N.GSW_ERR_UNSUPPORTED, kw
