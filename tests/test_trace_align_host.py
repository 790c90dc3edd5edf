"""CPU (no GPU): the aligned registry search before any device is asked -- the launch policy of gsw_counts_align swept by a host-only program
(tests/counts_align_plan_cases.cpp over csrc/gswm_counts_align_plan.h), the C entry point's refusals, the restatement of tests/trace_align_reference.py on the
shared-key case (sigma 4, fpr 1e-6: the conditions the search is built for, asserted on the restatement alone), the parser and the report line."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import align_reference as AR
import key_search_reference as R
import trace_align_reference as TR
from conftest import ROOT


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, detect, trace
    assert hasattr(trace, "trace_latents_aligned") and hasattr(trace, "trace_latents_keyed_aligned")
    return align, detect, trace


# ------------------------------------------------------------------------------------------------ the launch policy
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("counts_align_plan") / "counts_align_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "counts_align_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Every refusal has the status the specification gives it, in the order BAD_ARG, RAGGED, UNSUPPORTED (restated with 128-bit products), and decides nothing.
    For every accepted input: the row, its keystream and the reduction region lie in LDS in that order, disjoint, 16-byte aligned, within 64 + 64 + 8 KiB; the
    counting lanes are a multiple of the message units and their counters fit the reduction region; a lane's largest count fits seven vertical counters and a
    uint8 (words) or a uint16 (bytes), the groups together reach V; the grid covers every (image, alignment) exactly once and a chunk above 1 keeps 2048
    workgroups."""
    words = sweep.stderr.split()
    assert int(words[0]) > 200000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_both_paths(sweep):
    seen = set(sweep.stderr.split()[4:])
    assert seen >= {"bad_arg", "ragged", "unsupported", "words", "bytes", "chunk1", "chunk3", "chunk16", "lds>128K", "idle_lanes"}, seen


# ------------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_c_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                          # never dereferenced: every call below is refused before a launch
    key, nonce = bytes(32), bytes(16)

    def call(rows=p, B=1, C=4, H=8, W=8, l=1, al=p, A=1, key=key, nonce=nonce, M=64, out=p):
        return lib.gsw_counts_align(rows, B, C, H, W, l, al, A, key, nonce, M, out, None)

    for kw in (dict(rows=None), dict(al=None), dict(out=None), dict(key=None), dict(nonce=None), dict(al=odd), dict(out=odd), dict(B=0), dict(C=0), dict(H=-1),
               dict(W=0), dict(A=0), dict(l=0), dict(l=3), dict(M=0), dict(M=4), dict(M=12), dict(M=2056), dict(M=-8), dict(l=3, C=3, H=3, W=3),
               dict(M=12, C=1, H=3, W=3)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(C=1, H=3, W=3, M=8), dict(M=24), dict(C=3, H=5, W=8, M=64), dict(C=4, H=512, W=512, M=24), dict(C=1, H=3, W=3, M=8, B=65536)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    for kw in (dict(C=4, H=512, W=512, M=256), dict(C=4, H=256, W=512, l=2), dict(C=2 ** 30, H=2 ** 30, W=2 ** 30), dict(B=65536)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw


def test_symbol_is_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    assert "gsw_counts_align" in N.exported_symbols() and hasattr(lib, "gsw_counts_align")
    fn = lib.gsw_counts_align
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_counts_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev, int A, const uint8_t key[32]," in hdr
    import __graft_entry__ as E
    assert {"gswm_counts_align.inc", "gswm_counts_align_plan.h"} <= set(E.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert "gswm_counts_align.inc" in rule and "gswm_counts_align_plan.h" in rule
    assert '#include "gswm_counts_align.inc"' in open(os.path.join(csrc, "gswm_keyed.hip")).read()


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_of_counts_align_on_a_pattern():
    """an all-zero row under an all-zero keystream counts nothing, under an all-ones keystream V everywhere; the identity alignment of a random row is the plain
    vote count of tests/key_search_reference.py; every alignment keeps the total number of ones"""
    rng = np.random.default_rng(5)
    shape, M = (2, 4, 4), 16
    aligns = [(d, dy, dx) for d in range(8) for dy, dx in ((0, 0), (1, -2))]
    zero = np.zeros((1, 4), dtype=np.uint8)
    assert not TR.counts_align(zero, shape, 1, aligns, np.zeros(4, np.uint8), M).any()
    assert (TR.counts_align(zero, shape, 1, aligns, np.full(4, 255, np.uint8), M) == 2).all()
    rows = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    ks = rng.integers(0, 256, 4, dtype=np.uint8)
    c = TR.counts_align(rows, shape, 1, aligns, ks, M)
    assert c.shape == (3, 16, 16) and np.array_equal(c[:, 0], R.counts(rows, ks, 2))
    plain = TR.counts_align(rows, shape, 1, aligns, np.zeros(4, np.uint8), M)
    assert (plain.sum(axis=2) == np.unpackbits(rows, axis=1).sum(axis=1)[:, None]).all()


def test_restatement_of_the_merge_rule():
    S = np.zeros((1, 3, 4), dtype=np.int64)
    S[0, :, 0] = (5, 9, 9)          # record 0: its best alignment is 1, the lower of two equals
    S[0, :, 1] = (9, 1, 2)          # record 1 ties with record 0 and comes after it
    S[0, :, 2] = (-3, -3, -3)
    S[0, :, 3] = (10, 0, 0)
    rec, al, sc = TR.merge(S, 5)
    assert rec.tolist() == [[3, 0, 1, 2, -1]] and al.tolist() == [[0, 1, 0, 0, -1]] and sc.tolist() == [[10, 9, 9, -3, TR.INT32_MIN]]


@pytest.fixture(scope="module")
def SHARED(G):
    AL, D, T = G
    E = TR.SHARED
    s = TR.setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200 and cands[0] == (0, 0, 0)
    counts, S = TR.shared_scores(s["z16"], cands, s["ks"], s["registry"])
    return dict(s, cands=cands, counts=counts, S=S)


def test_the_restatement_alone_meets_the_shared_key_case(G, SHARED):
    AL, D, T = G
    E = TR.SHARED
    limit = math.log10(E["fpr"])
    M, n = 8 * E["msg_bytes"], int(np.prod(E["shape"]))
    cands = SHARED["cands"]
    host = TR.trace_host(SHARED["S"], n, T.log10_p_soft, T.log10_p_any)
    print("log10 p over U A pairs:", [round(h[3], 1) for h in host])
    for b, h in enumerate(host):                                             # six of six: the right row, the alignment that undoes the attack
        assert h[0] == E["rows"][b] and h[3] <= limit
        assert cands[h[1]] == AL.inverse(E["attacks"][b], 32, 32)
        assert np.array_equal(AR.apply_np(SHARED["attacked"][b], cands[h[1]]), SHARED["clean"][b])
    plain = TR.trace_host(SHARED["S"][:, :1], n, T.log10_p_soft, T.log10_p_any)     # without alignments: the identity alone, Bonferroni over U
    print("log10 p without alignments:", [round(h[3], 1) for h in plain])
    assert [h[3] <= limit for h in plain] == [True] + [False] * 5 and plain[0][0] == E["rows"][0]
    # the two-step route: the blind statistic under the key picks the alignment, Bonferroni over A
    rows = R.sign_rows(SHARED["z16"].reshape(6, -1).double().numpy())
    blind = AR.search_stats(rows, E["shape"], 1, cands, SHARED["ks"][None, :], E["msg_bytes"])[:, :, 0]
    bounds = [T.log10_p_any(D.log10_p_blind(int(blind[b].max()), M, n // M), len(cands)) for b in range(6)]
    print("log10 p of the blind route over A:", [round(p, 1) for p in bounds])
    assert sum(p <= limit for p in bounds) < 6
    # unwatermarked latents name nobody
    _, Sb = TR.shared_scores(SHARED["blank"], cands, SHARED["ks"], SHARED["registry"])
    none = TR.trace_host(Sb, n, T.log10_p_soft, T.log10_p_any)
    print("blank log10 p:", [round(h[3], 2) for h in none])
    assert len(none) == 4 and all(h[3] > limit for h in none)


# ------------------------------------------------------------------------------------------------ the public surface
def test_parser_refusals_by_name(capsys):
    from gswm_amd import trace as T
    base = ["--registry", "r.tsv"]
    shared = base + ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = T.build_parser().parse_args(shared)
    assert a.align == "none" and a.align_shift == 0
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--hard", "--top", "3", "--l", "2", "--tamper_map", "maps"])
    assert (a.align, a.align_shift, a.hard, a.top, a.l, a.tamper_map) == ("d4", 2, True, 3, 2, "maps")
    a = T.build_parser().parse_args(base + ["--per_record_keys", "--align", "flips", "--tamper_map", "maps"])
    assert a.per_record_keys and a.align == "flips"
    for extra, name in ((shared + ["--align", "d4", "--reliability", "7"], "--reliability"),
                        (base + ["--per_record_keys", "--align", "d4", "--keyed_reliability", "7"], "--keyed_reliability"),
                        (base + ["--per_record_keys", "--align", "flips", "--l", "2", "--window_reliability", "7"], "--window_reliability"),
                        (shared + ["--align_shift", "1"], "--align_shift"), (shared + ["--align", "d4", "--align_shift", "-1"], "--align_shift"),
                        (shared + ["--align", "rot"], "--align")):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(extra)
        err = capsys.readouterr().err
        assert name in err and ("--align" in err), (extra, err)


def test_format_line_with_and_without_an_alignment(G):
    AL, D, T = G
    c = T.Candidate("alice", 3, 900, 60, -12.3456)
    assert c.alignment is None and T.TraceResult().alignment is None
    plain = T.format_line("x.png", T.TraceResult([c], "alice"), 64)
    assert plain == "x.png, user: alice, agreement, 0.9375, log10 p, -12.346"
    c2 = T.Candidate("alice", 3, 900, 60, -12.3456, (5, 2, -1))
    line = T.format_line("x.png", T.TraceResult([c2], "alice", None, (5, 2, -1)), 64)
    assert line == plain + ", alignment: hflip+rot90 shift (2,-1)" == plain + ", alignment: " + AL.describe((5, 2, -1))
    assert "alignment" not in T.format_line("x.png", T.TraceResult([c2], None), 64)          # not attributed: the result names no alignment
