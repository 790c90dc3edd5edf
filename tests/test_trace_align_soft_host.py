"""CPU (no GPU): the aligned registry search ranked by reliability levels before any device is asked -- the launch policy of gsw_level_counts_align swept by a
host-only program (tests/level_counts_align_plan_cases.cpp over csrc/gswm_counts_align_soft_plan.h), the C entry point's refusals, the restatement of
tests/trace_align_soft_reference.py on patterns and on the two cases the search is built for (shared key at sigma 5.75, a key per record at sigma 5.0, fpr 1e-6:
the levels name six of six where the signs name fewer, asserted on the restatement alone), the parser and the report."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_reference as AR
import key_search_reference as R
import soft_reference as SR
import trace_align_reference as TR
import trace_align_soft_reference as TS
from conftest import ROOT


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, soft, trace
    assert hasattr(trace, "trace_latents_aligned_soft") and hasattr(trace, "trace_latents_keyed_aligned_soft")
    return align, soft, trace


# ------------------------------------------------------------------------------------------------ the launch policy
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("level_counts_align_plan") / "level_counts_align_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "level_counts_align_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Every refusal has the status the specification gives it, in the order BAD_ARG, RAGGED, UNSUPPORTED (restated with 128-bit products), and decides nothing.
    For every accepted input: the 1 + P rows, the keystream and the two halves of the reduction region lie in LDS in that order, disjoint, 16-byte aligned,
    within 128 KiB and equal to the restated layout; the counting lanes are a multiple of the message units; a lane's largest count fits its live counter
    planes (seven at most), 15 times it fits a uint16, the groups together reach V and |bias| + 15 V fits int32; the grid covers every (image, alignment)
    exactly once and a chunk above 1 keeps 2048 workgroups."""
    words = sweep.stderr.split()
    assert int(words[0]) > 1000000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_both_paths(sweep):
    seen = set(sweep.stderr.split()[4:])
    assert seen >= {"bad_arg", "ragged", "unsupported", "words", "bytes", "chunk1", "chunk3", "chunk16", "lds_at_cap", "idle_lanes", "4x128x128_p4", "cplanes1",
                    "cplanes2", "cplanes6"}, seen
    assert "cplanes7" not in seen                                              # the LDS cap binds before a lane's count reaches 64


# ------------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_c_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                          # never dereferenced: every call below is refused before a launch
    key, nonce = bytes(32), bytes(16)

    def call(signs=p, planes=p, P=4, B=1, C=4, H=8, W=8, al=p, A=1, key=key, nonce=nonce, M=64, bias=0, score=p, wsum=p):
        return lib.gsw_level_counts_align(signs, planes, P, B, C, H, W, al, A, key, nonce, M, bias, score, wsum, None)

    for kw in (dict(signs=None), dict(planes=None), dict(al=None), dict(score=None), dict(key=None), dict(nonce=None), dict(al=odd), dict(score=odd),
               dict(wsum=odd), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(A=0), dict(P=0), dict(P=5), dict(M=0), dict(M=4), dict(M=12), dict(M=2056),
               dict(M=-8), dict(P=0, C=3, H=3, W=3), dict(M=12, C=1, H=3, W=3)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(C=1, H=3, W=3, M=8), dict(M=24), dict(C=3, H=5, W=8, M=64), dict(C=4, H=512, W=512, M=24), dict(C=1, H=3, W=3, M=8, B=65536)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    for kw in (dict(C=4, H=256, W=256, M=256), dict(C=4, H=256, W=264, M=256, P=1), dict(C=4, H=128, W=264, M=256), dict(C=2 ** 30, H=2 ** 30, W=2 ** 30),
               dict(B=65536), dict(bias=2 ** 31 - 1), dict(bias=-2 ** 31), dict(bias=2 ** 31 - 15 * 4)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw


def test_symbol_is_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    assert "gsw_level_counts_align" in N.exported_symbols() and hasattr(lib, "gsw_level_counts_align")
    fn = lib.gsw_level_counts_align
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 16
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_level_counts_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev, int A," in hdr
    import __graft_entry__ as E
    assert {"gswm_counts_align_soft.inc", "gswm_counts_align_soft_plan.h"} <= set(E.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert "gswm_counts_align_soft.inc" in rule and "gswm_counts_align_soft_plan.h" in rule
    src = open(os.path.join(csrc, "gswm_keyed.hip")).read()
    assert src.index('#include "gswm_align_soft.inc"') < src.index('#include "gswm_counts_align.inc"') < src.index('#include "gswm_counts_align_soft.inc"')


def test_the_lds_bytes_of_the_package_are_the_plans():
    """`codec.level_counts_align_lds_bytes` restates the plan's layout for the refusal that precedes a launch: the figures of the plan header"""
    from gswm_amd import codec
    assert codec.level_counts_align_lds_bytes(4 * 128 * 128, 4, 256) == (40 + 8 + 32) * 1024
    assert codec.level_counts_align_lds_bytes(4 * 64 * 64, 4, 256) == (10 + 2 + 32) * 1024
    assert codec.level_counts_align_lds_bytes(4 * 256 * 256, 1, 256) == codec.LEVEL_COUNTS_ALIGN_LDS_CAP == 131072
    assert codec.level_counts_align_lds_bytes(8 * 17 * 25, 3, 200) == 4 * 432 + 64 * 7 + 2 * 250 * 16


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_of_level_counts_align_on_patterns():
    """all-zero levels give zeros; one plane of all ones gives 2 counts_align - V and wsum = V; the identity alignment of random levels is
    `soft_reference.soft_vote`; every alignment keeps sum_t wsum"""
    rng = np.random.default_rng(6)
    shape, M = (2, 4, 4), 16
    n, V = 32, 2
    aligns = [(d, dy, dx) for d in range(8) for dy, dx in ((0, 0), (1, -2))]
    signs = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    ks = rng.integers(0, 256, 4, dtype=np.uint8)
    score, wsum = TS.level_counts_align(signs, np.zeros((3, n), dtype=np.int64), shape, aligns, ks, M)
    assert score.shape == wsum.shape == (3, 16, M) and not score.any() and not wsum.any()
    score, wsum = TS.level_counts_align(signs, np.ones((3, n), dtype=np.int64), shape, aligns, ks, M)
    assert np.array_equal(score, 2 * TR.counts_align(signs, shape, 1, aligns, ks, M) - V) and (wsum == V).all()
    z = rng.standard_normal((3, n)).astype(np.float32)
    thr = np.linspace(0.1, 2.0, 15).astype(np.float32)
    lv = np.stack([SR.levels_of(z[b], thr) for b in range(3)])
    assert lv.max() > 8 and lv.min() == 0
    score, wsum = TS.level_counts_align(R.sign_rows(z.astype(np.float64)), lv, shape, aligns, ks, M)
    for b in range(3):
        vote = SR.soft_vote(z[b], ks, thr, M)
        assert np.array_equal(score[b, 0], vote["score"]) and np.array_equal(wsum[b, 0], vote["wsum"])
    assert (wsum.sum(axis=2) == lv.sum(axis=1)[:, None]).all()
    # the keyed score of records that share the key is the shared score of their messages
    s_al, w_al = TS.aligned_rows(R.sign_rows(z.astype(np.float64)), lv, shape, aligns)
    msgs = rng.integers(0, 256, (5, M // 8), dtype=np.uint8)
    cw = ks[None, :] ^ np.tile(msgs, (1, n // M))
    assert np.array_equal(TS.keyed_scores(s_al, w_al, cw), TS.shared_scores(score, msgs))


def _named(host, rows, attacks, cands, inverse, limit):
    return [h[0] == rows[b] and h[3] <= limit and cands[h[1]] == inverse(attacks[b], 32, 32) for b, h in enumerate(host)]


def test_the_restatement_alone_meets_the_shared_key_case(G):
    """sigma 5.75: the 15-level statistic with Hoeffding's bound names six of six with the alignment that undoes the attack, the sign statistic with its exact
    tail fewer; unwatermarked latents name nobody and every soft bound of theirs is 0.0.  The figures are in DESIGN.md section 4.26."""
    AL, S, T = G
    E = TS.SHARED
    limit = math.log10(E["fpr"])
    n = int(np.prod(E["shape"]))
    s = TS.shared_setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200 and float(s["z16"].max()) >= TS.SATURATES_AT > float(s["held"].max())
    thr = S.uniform_thresholds(s["held"], E["levels"]).numpy()                 # AFTER the latents are held
    _, Sl, wsq = TS.shared_search(s["held"], thr, cands, s["ks"], s["registry"])
    soft = TS.trace_host(Sl, wsq, S.log10_p, T.log10_p_any)
    print("levels, log10 p over U A pairs:", [round(h[3], 1) for h in soft])
    assert all(_named(soft, E["rows"], E["attacks"], cands, AL.inverse, limit))
    for b, h in enumerate(soft):
        assert np.array_equal(AR.apply_np(s["attacked"][b], cands[h[1]]), s["clean"][b])
    _, Ss = TR.shared_scores(s["held"], cands, s["ks"], s["registry"])
    sign = TR.trace_host(Ss, n, T.log10_p_soft, T.log10_p_any)
    print("signs, log10 p over U A pairs:", [round(h[3], 1) for h in sign])
    assert sum(_named(sign, E["rows"], E["attacks"], cands, AL.inverse, limit)) < 6
    thb = S.uniform_thresholds(s["held_blank"], E["levels"]).numpy()
    _, Sb, wb = TS.shared_search(s["held_blank"], thb, cands, s["ks"], s["registry"])
    none = TS.trace_host(Sb, wb, S.log10_p, T.log10_p_any)
    print("blank log10 p:", [h[3] for h in none])
    assert len(none) == 4 and all(h[3] == 0.0 for h in none)
    _, Sbs = TR.shared_scores(s["held_blank"], cands, s["ks"], s["registry"])
    assert all(h[3] > limit for h in TR.trace_host(Sbs, n, T.log10_p_soft, T.log10_p_any))


def test_the_restatement_alone_meets_the_keyed_case(G):
    """sigma 5.0, a key per record: levels six of six, signs fewer, blanks nobody"""
    AL, S, T = G
    E = TS.KEYED
    limit = math.log10(E["fpr"])
    n = int(np.prod(E["shape"]))
    s = TS.keyed_setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    thr = S.uniform_thresholds(s["held"], E["levels"]).numpy()
    Sl, wsq = TS.keyed_search(s["held"], thr, cands, s["records"])
    soft = TS.trace_host(Sl, wsq, S.log10_p, T.log10_p_any)
    print("keyed levels, log10 p over U A pairs:", [round(h[3], 1) for h in soft])
    assert all(_named(soft, E["rows"], E["attacks"], cands, AL.inverse, limit))
    sign = TR.trace_host(TR.keyed_search(s["held"], cands, s["records"]), n, T.log10_p_soft, T.log10_p_any)
    print("keyed signs, log10 p over U A pairs:", [round(h[3], 1) for h in sign])
    assert sum(_named(sign, E["rows"], E["attacks"], cands, AL.inverse, limit)) < 6
    thb = S.uniform_thresholds(s["held_blank"], E["levels"]).numpy()
    Sb, wb = TS.keyed_search(s["held_blank"], thb, cands, s["records"])
    none = TS.trace_host(Sb, wb, S.log10_p, T.log10_p_any)
    print("keyed blank log10 p:", [h[3] for h in none])
    assert all(h[3] == 0.0 for h in none)
    assert all(h[3] > limit for h in TR.trace_host(TR.keyed_search(s["held_blank"], cands, s["records"]), n, T.log10_p_soft, T.log10_p_any))


# ------------------------------------------------------------------------------------------------ the public surface
def test_parser_acceptance_and_refusals_by_name(capsys):
    from gswm_amd import trace as T
    base = ["--registry", "r.tsv"]
    shared = base + ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    assert T.build_parser().parse_args(shared).align_reliability is None
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_reliability", "15", "--top", "3", "--fpr", "1e-4", "--tamper_map", "maps"])
    assert (a.align, a.align_shift, a.align_reliability, a.top, a.fpr, a.tamper_map) == ("d4", 2, 15, 3, 1e-4, "maps")
    a = T.build_parser().parse_args(base + ["--per_record_keys", "--align", "flips", "--align_reliability", "1"])
    assert a.per_record_keys and a.align == "flips" and a.align_reliability == 1
    keyed = base + ["--per_record_keys"]
    for extra, names in ((shared + ["--align_reliability", "7"], ("--align_reliability", "--align")),
                         (shared + ["--align", "none", "--align_reliability", "7"], ("--align_reliability", "--align")),
                         (shared + ["--align", "d4", "--align_reliability", "7", "--hard"], ("--align_reliability", "--hard")),
                         (shared + ["--align", "d4", "--align_reliability", "7", "--l", "2"], ("--align_reliability", "--l 2")),
                         (keyed + ["--align", "d4", "--align_reliability", "7", "--l", "4"], ("--align_reliability", "--l 4")),
                         (shared + ["--align", "d4", "--align_reliability", "7", "--reliability", "7"], ("--align_reliability", "--reliability")),
                         (keyed + ["--align", "d4", "--align_reliability", "7", "--keyed_reliability", "7"], ("--align_reliability", "--keyed_reliability")),
                         (keyed + ["--align", "d4", "--align_reliability", "7", "--l", "1", "--window_reliability", "7"], ("--align_reliability", "--window_reliability")),
                         (shared + ["--align", "d4", "--align_reliability", "0"], ("--align_reliability",)),
                         (shared + ["--align", "d4", "--align_reliability", "16"], ("--align_reliability",)),
                         # the refusals that were there before stand
                         (shared + ["--align", "d4", "--reliability", "7"], ("--align", "--reliability")),
                         (keyed + ["--align", "d4", "--keyed_reliability", "7"], ("--align", "--keyed_reliability")),
                         (keyed + ["--align", "flips", "--l", "2", "--window_reliability", "7"], ("--align", "--window_reliability"))):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(extra)
        err = capsys.readouterr().err
        assert all(name in err for name in names), (extra, err)


def test_the_statistic_field_names_the_levels_and_the_candidates():
    from gswm_amd import trace as T
    shared = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_reliability", "15"])
    assert T._statistic_name(a) == "soft, 15 reliability levels over 200 alignments"
    a = T.build_parser().parse_args(shared + ["--align", "flips", "--align_reliability", "3"])
    assert T._statistic_name(a) == "soft, 3 reliability levels over 4 alignments"
    # without the flag nothing changes
    assert T._statistic_name(T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2"])) == "soft"
    assert T._statistic_name(T.build_parser().parse_args(shared + ["--align", "d4", "--hard"])) == "hard"
    assert T._statistic_name(T.build_parser().parse_args(shared + ["--reliability", "7"])) == "soft, 7 reliability levels"


def test_the_report_header_and_line(tmp_path, capsys):
    """`_report` on a made-up job: the header carries the statistic with its levels and the candidate count, the line the alignment"""
    from types import SimpleNamespace
    from gswm_amd import align as AL, trace as T
    shared = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_reliability", "15"])
    a.message_length = 64
    reg = T.Registry(8)
    reg.add("alice", bytes(8))
    c = T.Candidate("alice", 0, 9000, 60, -12.3456, (5, 2, -1))
    job = SimpleNamespace(path=str(tmp_path), files=[str(tmp_path / "x.png")])
    T._report(job, [T.TraceResult([c], "alice", None, (5, 2, -1))], a, reg, False)
    out = capsys.readouterr().out
    lines = (tmp_path / "trace.txt").read_text().splitlines()
    info = dict(l.split(",", 1) for l in lines[1:lines.index("=" * 40 + "Batch Start" + "=" * 40)])
    assert info["statistic"] == "soft, 15 reliability levels over 200 alignments" and info["alignments"] == "200" and info["align"] == "d4"
    line = "x.png, user: alice, agreement, 0.9375, log10 p, -12.346, alignment: " + AL.describe((5, 2, -1))
    assert line in lines and line in out


def test_host_tensors_are_refused_without_a_fallback():
    """there is no CPU path: the usual RuntimeError"""
    from gswm_amd import codec
    rows = codec.LevelRows(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 1, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                           torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        codec.level_counts_align(rows, (1, 8, 8), [(0, 0, 0)], bytes(32), bytes(16), 8)
