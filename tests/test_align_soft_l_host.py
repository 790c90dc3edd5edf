"""CPU (no GPU): reliability levels of multi-bit windows (l = 2, 4) through the alignment searches before any device is asked -- the two
launch policies swept by host-only programs (tests/level_align_l_plan_cases.cpp, tests/level_counts_align_l_plan_cases.cpp), the refusal table of every new
Python entry and of both C entry points (tests/align_soft_l_refusal_cases.py against tests/golden/align_soft_l_refusals.tsv), the ABI, the restatement of
tests/align_soft_l_reference.py on patterns and end to end, the parsers and the report header.

The noise of the end-to-end case.  tools/align_soft_l_sigma_walk.py walks sigma over a 0.25 grid up to 10 on the restatement (profiles/align_soft_l_sigma_walk.txt).
For none of the six (search, l) is there a sigma at which the 15-level statistic names all six images and the sign search fewer: up to sigma 3.75 both name six of
six everywhere (at 3.75 one level bound lies within 0.05 of the limit), and where the levels first lose an image (`FIRST_LOSS`: detect 4.0 at both l; shared key 5.25 at l = 4, 5.0 at l = 2; keyed 4.5 at l = 4, 5.0 at
l = 2) the signs still name at least as many.  No gap is claimed: the tests assert the exact reproduction at `SIGMA` = 3.5 and hold `FIRST_LOSS` to that."""
import collections
import csv
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_reference as AR
import align_soft_l_reference as ALR
import align_soft_l_refusal_cases as L
import key_search_soft_reference as KS
import soft_l_reference as SL
import trace_align_reference as TR
import trace_align_soft_reference as TS
from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "align_soft_l_refusals.tsv")
PY_ENTRIES = {"codec.level_rows_align_l", "codec.level_counts_align_l", "align.search_keys_soft_l", "align.extract_aligned_soft_l", "detect.detect_latents_aligned_soft_l",
              "trace.trace_latents_aligned_soft_l", "trace.trace_latents_keyed_aligned_soft_l"}
C_ENTRIES = {"gsw_level_rows_align_l", "gsw_level_counts_align_l"}


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, detect, soft, trace
    return align, soft, trace, detect


# ------------------------------------------------------------------------------------------------ the launch policies
def _sweep(tmp_path_factory, name):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp(name) / name
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def rows_sweep(tmp_path_factory):
    return _sweep(tmp_path_factory, "level_align_l_plan_cases")


@pytest.fixture(scope="module")
def counts_sweep(tmp_path_factory):
    return _sweep(tmp_path_factory, "level_counts_align_l_plan_cases")


def test_the_rows_plan_keeps_the_invariants_of_a_launch(rows_sweep):
    """Every status is the restated one (BAD_ARG, UNSUPPORTED, RAGGED, in that order, 128-bit products) and a refusal decides nothing.  For every accepted input:
    rowbytes is n l / 8; the staged rows are 1 + P strides of rowbytes padded to 16 within 64 KiB, or the SG form with at most 128 KiB of rows; the grid covers
    every (image, alignment) once; and at l = 1 the plan equals level_align_decide's byte for byte."""
    words = rows_sweep.stderr.split()
    assert int(words[0]) > 200000 and words[1] == "inputs,"
    assert not rows_sweep.stdout, rows_sweep.stdout.splitlines()[:10]
    assert words[2] == "0"
    seen = set(words[4:])
    assert seen >= {"bad_arg", "ragged", "unsupported", "lds@l1", "lds@l2", "lds@l4", "sg@l1", "sg@l2", "sg@l4", "chunk1", "chunk3", "chunk16", "l2_rows_at_phase_2",
                    "4x128x128_l4_p2_sg"}, seen


def test_the_counts_plan_keeps_the_invariants_of_a_launch(counts_sweep):
    """tests/level_counts_align_plan_cases.cpp's invariants with rows of n l bits: the LDS regions in order, disjoint, 16-byte aligned, within 128 KiB and equal to
    the restated layout; the counting lanes a multiple of the message units; a lane's largest count within its counter planes and 15 times it within a uint16;
    |bias| + 15 V within int32; the grid covers every (image, alignment) once; and at l = 1 the plan equals level_counts_align_decide's byte for byte."""
    words = counts_sweep.stderr.split()
    assert int(words[0]) > 1000000 and words[1] == "inputs,"
    assert not counts_sweep.stdout, counts_sweep.stdout.splitlines()[:10]
    assert words[2] == "0"
    seen = set(words[4:])
    assert seen >= {"bad_arg", "ragged", "unsupported", "words@l1", "words@l2", "words@l4", "bytes@l1", "bytes@l2", "bytes@l4", "chunk1", "chunk3", "chunk16",
                    "lds_at_cap", "idle_lanes", "4x64x64_l4_p4_80KiB", "cplanes1", "cplanes6"}, seen
    assert "cplanes7" not in seen                                              # the LDS cap binds before a lane's count reaches 64


def test_the_lds_bytes_of_the_package_are_the_plans():
    from gswm_amd import codec
    assert codec.level_counts_align_l_lds_bytes(4 * 64 * 64 * 4, 4, 256) == (40 + 8 + 32) * 1024       # l = 4: the row of 4 x 128 x 128 at l = 1
    assert codec.level_counts_align_l_lds_bytes(4 * 128 * 128 * 4, 1, 256) == codec.LEVEL_COUNTS_ALIGN_LDS_CAP
    assert codec.level_counts_align_l_lds_bytes(4 * 5 * 8 * 4, 2, 40) == 3 * 80 + 64 * 2 + 2 * 255 * 16


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbols_are_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    for name, nargs in (("gsw_level_rows_align_l", 13), ("gsw_level_counts_align_l", 17)):
        assert name in N.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
        assert f"int {name}(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int l, int B, int C, int H, int W, const int32_t* aligns_dev, int A," in hdr
    import __graft_entry__ as E
    new = {"gswm_align_soft_l.inc", "gswm_counts_align_soft_l.inc", "gswm_counts_align_soft_l_plan.h"}
    assert new <= set(E.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert all(f in rule for f in new)
    src = open(os.path.join(csrc, "gswm_keyed.hip")).read()
    assert src.index('#include "gswm_align_soft.inc"') < src.index('#include "gswm_counts_align_soft.inc"') < src.index('#include "gswm_align_soft_l.inc"') \
        < src.index('#include "gswm_counts_align_soft_l.inc"')


# ------------------------------------------------------------------------------------------------ the refusals
@pytest.fixture(scope="module")
def table():
    with open(TABLE, newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t", quoting=csv.QUOTE_NONE))
    return {(r["entry"], r["tag"]): r for r in rows}


def test_the_table_and_the_cases_name_the_same_rows(table):
    names = [c[:2] for c in L.CASES] + [c[:2] for c in L.C_CASES]
    assert len(names) == len(table) and set(names) == set(table)
    for entry, tag, where, _ in L.CASES:
        assert table[(entry, tag)]["where"] == where
    for symbol, tag, made_up, _ in L.C_CASES:
        assert table[(symbol, tag)]["where"] == ("made_up" if made_up else "null") and table[(symbol, tag)]["outcome"] == "status"


def test_the_table_covers_what_it_is_for(table):
    by_entry = collections.defaultdict(list)
    for (entry, tag), r in table.items():
        by_entry[entry].append((tag, r))
    assert set(by_entry) == PY_ENTRIES | C_ENTRIES
    for entry, rows in by_entry.items():
        tags = {tag for tag, _ in rows}
        assert sum(tag.startswith("two_") for tag in tags) >= 1, entry                             # the order of two faults
        if entry in C_ENTRIES:
            assert {r["message"] for _, r in rows} == {"1", "2", "3"}, entry                        # BAD_ARG, UNSUPPORTED, RAGGED; no row is accepted
            assert all(r["message"] == "1" for _, r in rows if r["where"] == "null"), entry
            assert {"l_0", "l_3", "l_8"} <= tags
        else:
            host = [r for tag, r in rows if tag.split("/")[0] == "host"]
            assert host and all(r["outcome"] == "RuntimeError" and "HIP device" in r["message"] for r in host), entry
            assert any(r["outcome"] == "Reached" for _, r in rows), entry
            assert {"l_1", "l_3", "l_True", "aligns_empty", "aligns_bad_entry", "lattice_ragged"} <= tags, entry
            l1 = dict(rows)["l_1"]
            assert l1["outcome"] == "ValueError" and f"use `{entry.split('.')[1][:-2]}`" in l1["message"], entry     # l = 1 points at the l = 1 name
    for entry in PY_ENTRIES - {"codec.level_rows_align_l", "codec.level_counts_align_l"}:
        tags = {tag for tag, _ in by_entry[entry]}
        assert "latents_3d" in tags and tags & {"levels_0", "levels_16"}, entry
    for entry in ("align.search_keys_soft_l", "trace.trace_latents_aligned_soft_l", "trace.trace_latents_keyed_aligned_soft_l"):
        assert dict(by_entry[entry])["table_window"]["outcome"] == "ValueError"                    # a table of the wrong window
    assert {r["message"] for r in table.values() if r["outcome"] == "Reached"} == {"gsw_level_rows_align_l", "gsw_level_counts_align_l", "gsw_level_pack_l"}


@pytest.mark.parametrize("entry", sorted(PY_ENTRIES))
def test_python_entries_refuse_as_recorded(table, entry):
    wrong = []
    for e, tag, where, thunk in L.CASES:
        if e == entry:
            want = table[(e, tag)]
            got = L.outcome(thunk, where)
            if got != (want["outcome"], want["message"]):
                wrong.append((tag, got, (want["outcome"], want["message"])))
    assert not wrong, wrong
    assert "is_cuda" not in vars(torch.Tensor) and not torch.zeros(1).is_cuda                      # the stand-in for the device is gone again


@pytest.mark.parametrize("symbol", sorted(C_ENTRIES))
def test_c_entries_return_as_recorded(table, symbol):
    """Rows with a null pointer everywhere; the rows whose pointers are made up only where no device could ever see them"""
    device = torch.cuda.is_available()
    wrong, ran = [], 0
    for s, tag, made_up, args in L.C_CASES:
        if s == symbol and not (made_up and device):
            got, ran = L.c_outcome(s, args), ran + 1
            if str(got) != table[(s, tag)]["message"]:
                wrong.append((tag, got, table[(s, tag)]["message"]))
    assert ran >= 8 and not wrong, wrong


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_patterns():
    """the identity keeps the rows; an alignment moves the l values of an element together (the restatement's rows are `align_reference.rows_align`'s, plane by
    plane); all-zero levels give zeros; one plane of all ones gives 2 counts_align - V and wsum = V; the identity alignment of real levels is
    `soft_l_reference.soft_vote`; every alignment keeps sum_t wsum; records that share a key score as their messages do"""
    rng = np.random.default_rng(28)
    shape = (2, 4, 4)
    n = 32
    aligns = [(d, dy, dx) for d in range(8) for dy, dx in ((0, 0), (1, -2))]
    for l, M in ((2, 16), (4, 32)):
        nb, V = n * l, n * l // M
        signs = rng.integers(0, 256, (3, nb // 8), dtype=np.uint8)
        planes = rng.integers(0, 256, (3, 3, nb // 8), dtype=np.uint8)
        ks = rng.integers(0, 256, nb // 8, dtype=np.uint8)
        s_al, p_al = ALR.level_rows_align_l(signs, planes, shape, l, aligns)
        assert np.array_equal(s_al[:, 0], signs) and np.array_equal(p_al[:, 0], planes)
        assert np.array_equal(s_al, AR.rows_align(signs, shape, l, aligns))
        for k in range(3):
            assert np.array_equal(p_al[:, :, k], AR.rows_align(planes[:, k], shape, l, aligns))
        score, wsum = ALR.level_counts_align_l(signs, np.zeros((3, nb), dtype=np.int64), shape, l, aligns, ks, M)
        assert score.shape == wsum.shape == (3, 16, M) and not score.any() and not wsum.any()
        score, wsum = ALR.level_counts_align_l(signs, np.ones((3, nb), dtype=np.int64), shape, l, aligns, ks, M)
        assert np.array_equal(score, 2 * TR.counts_align(signs, shape, l, aligns, ks, M) - V) and (wsum == V).all()
        z = torch.from_numpy(rng.standard_normal((3, *shape)).astype(np.float32))
        thr = np.stack([np.linspace(0.02, 0.6, 15)] * l).astype(np.float32)
        sg, lv, flags = ALR.rows_of(z, thr, l)
        assert lv.max() > 8 and lv.min() == 0 and not flags.any()
        score, wsum = ALR.level_counts_align_l(sg, lv, shape, l, aligns, ks, M)
        Z = SL.widen64(z)
        for b in range(3):
            vote = SL.soft_vote(Z[b], ks, thr, M, l)
            assert np.array_equal(score[b, 0], vote["score"]) and np.array_equal(wsum[b, 0], vote["wsum"])
        assert (wsum.sum(axis=2) == lv.sum(axis=1)[:, None]).all()
        s_al, w_al = ALR.aligned_rows(sg, lv, shape, l, aligns)
        msgs = rng.integers(0, 256, (5, M // 8), dtype=np.uint8)
        cw = ks[None, :] ^ np.tile(msgs, (1, nb // M))
        assert np.array_equal(TS.keyed_scores(s_al, w_al, cw), TS.shared_scores(score, msgs))
        assert np.array_equal(ALR.key_stats(sg, lv, shape, l, aligns, ks[None], M // 8)[:, :, 0], np.abs(score).sum(axis=2))


@pytest.fixture(scope="module", params=[4, 2])
def E2E(request, G):
    AL, S, T, D = G
    l = request.param
    E = ALR.E2E
    s = ALR.e2e_setup(l)
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200
    n = int(np.prod(E["shape"]))
    return dict(l=l, s=s, cands=cands, cw=TR.codewords(s["records"], n * l), want_al=ALR.restoring(cands), limit=math.log10(E["fpr"]), mods=(S, T, D))


@pytest.mark.parametrize("search", ["detect", "shared", "keyed"])
def test_the_restatement_end_to_end(G, E2E, search):
    """`SIGMA`: the 15-level statistic names all six with the alignment that restores the embedded lattice, none wrongly -- and so does the sign search: there is
    no gap to claim at l = 2, 4 (the module docstring).  At `FIRST_LOSS` the levels have lost an image and the signs name at least as many."""
    AL = G[0]
    e, l = E2E, E2E["l"]
    r = ALR.e2e_host(search, e["s"], l, ALR.SIGMA, e["cands"], e["cw"], e["mods"])
    assert [e["cands"][i] for i in e["want_al"]] == [AL.inverse(a, 32, 32) for a in ALR.E2E["attacks"]]      # the restoring alignment is `align.inverse`'s
    lev, sig = (ALR.named(r[k], r["rows"], e["want_al"], e["limit"]) for k in ("levels", "signs"))
    print(f"l = {l}, {search}, sigma {ALR.SIGMA}: levels {lev}, log10 p {[round(h[3], 1) for h in r['levels']]}; signs {sig}, {[round(h[3], 1) for h in r['signs']]}")
    assert lev == (6, 0) and sig == (6, 0)
    if search == "detect":                                                     # the soft vote under the named key: most, not all, bits of the message at this noise
        wrong = [int(np.unpackbits(np.frombuffer(h[4], dtype=np.uint8) ^ np.frombuffer(m, dtype=np.uint8)).sum()) for h, m in zip(r["levels"], e["s"]["msgs"])]
        assert max(wrong) < 32, wrong
    r = ALR.e2e_host(search, e["s"], l, ALR.FIRST_LOSS[(search, l)], e["cands"], e["cw"], e["mods"])
    lev, sig = (ALR.named(r[k], r["rows"], e["want_al"], e["limit"]) for k in ("levels", "signs"))
    print(f"l = {l}, {search}, sigma {ALR.FIRST_LOSS[(search, l)]}: levels {lev}, signs {sig}")
    assert lev[0] < 6 and lev[1] == 0 and sig[1] == 0 and sig[0] >= lev[0]


def test_unwatermarked_latents_name_nobody_on_the_restatement(G, E2E):
    AL, S, T, D = G
    e, l = E2E, E2E["l"]
    blank = TS.hold(e["s"]["blank"])
    thr = S.window_thresholds(blank, l, 15).numpy()
    assert all(h[3] > e["limit"] for h in ALR.detect_host(blank, thr, l, e["cands"], e["s"]["ks"], 8, T.log10_p_any))
    _, Sl, wsq = ALR.shared_search(blank, thr, l, e["cands"], e["s"]["ks"][0], e["s"]["registry"])
    assert all(h[3] > e["limit"] for h in ALR.trace_host(Sl, wsq, S.log10_p, T.log10_p_any))


# ------------------------------------------------------------------------------------------------ the public surface
def test_trace_parser_acceptance_and_refusals_by_name(capsys):
    from gswm_amd import trace as T
    base = ["--registry", "r.tsv"]
    shared = base + ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    keyed = base + ["--per_record_keys"]
    assert T.build_parser().parse_args(shared).align_window_reliability is None
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_window_reliability", "15", "--l", "4", "--top", "3", "--tamper_map", "maps"])
    assert (a.align, a.align_shift, a.align_window_reliability, a.l, a.top, a.tamper_map) == ("d4", 2, 15, 4, 3, "maps")
    a = T.build_parser().parse_args(keyed + ["--align", "flips", "--align_window_reliability", "1", "--l", "2"])
    assert a.per_record_keys and a.align == "flips" and a.align_window_reliability == 1 and a.l == 2
    ok = ["--align", "d4", "--align_window_reliability", "7", "--l", "2"]
    for extra, names in ((shared + ["--align_window_reliability", "7", "--l", "2"], ("--align_window_reliability", "--align")),
                         (shared + ["--align", "none", "--align_window_reliability", "7", "--l", "4"], ("--align_window_reliability", "--align")),
                         (shared + ["--align", "d4", "--align_window_reliability", "7"], ("--align_window_reliability", "--l 2", "--align_reliability")),
                         (shared + ["--align", "d4", "--align_window_reliability", "7", "--l", "1"], ("--align_window_reliability", "--align_reliability")),
                         (shared + ok + ["--hard"], ("--align_window_reliability", "--hard")),
                         (shared + ok + ["--reliability", "7"], ("--align_window_reliability", "--reliability")),
                         (keyed + ok + ["--keyed_reliability", "7"], ("--align_window_reliability", "--keyed_reliability")),
                         (keyed + ok + ["--window_reliability", "7"], ("--align_window_reliability", "--window_reliability")),
                         (shared + ok + ["--align_reliability", "7"], ("--align_window_reliability", "--align_reliability")),
                         (shared + ok + ["--pool", "all"], ("--pool",)),
                         (shared + ["--align", "d4", "--align_window_reliability", "0", "--l", "2"], ("--align_window_reliability",)),
                         (shared + ["--align", "d4", "--align_window_reliability", "16", "--l", "2"], ("--align_window_reliability",)),
                         # the refusals that were there before stand
                         (shared + ["--align", "d4", "--align_reliability", "7", "--l", "4"], ("--align_reliability", "--l 4")),
                         (keyed + ["--align", "flips", "--l", "2", "--window_reliability", "7"], ("--align", "--window_reliability")),
                         (shared + ["--pool", "all", "--pool_reliability", "7", "--l", "2"], ("--pool_reliability", "--l 2"))):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(extra)
        err = capsys.readouterr().err
        assert all(name in err for name in names), (extra, err)


def test_detect_cli_refusals_by_name(tmp_path):
    from gswm_amd import detect as D
    ring = tmp_path / "ring.tsv"
    ring.write_text("key0\t" + "00" * 32 + "\t" + "00" * 16 + "\n")
    base = ["--keyring", str(ring), "--single_image_path", "x.png"]
    a = D.build_parser().parse_args(base + ["--align", "d4", "--align_shift", "1", "--align_window_reliability", "15", "--l", "4"])
    assert (a.align, a.align_window_reliability, a.l) == ("d4", 15, 4)
    assert D.build_parser().parse_args(base).align_window_reliability == 0
    for extra, names in ((["--align_window_reliability", "7", "--l", "2"], ("--align_window_reliability", "--align")),
                         (["--align", "d4", "--align_window_reliability", "7"], ("--align_window_reliability", "--l 2", "--align_reliability")),
                         (["--align", "d4", "--align_window_reliability", "7", "--l", "2", "--align_reliability", "7"], ("--align_reliability",)),
                         (["--align", "d4", "--align_window_reliability", "7", "--l", "2", "--window_reliability", "7"], ("--window_reliability",)),
                         (["--align", "d4", "--align_window_reliability", "7", "--l", "2", "--reliability", "7"], ("--reliability",)),
                         # the refusal that was there before stands
                         (["--align", "d4", "--align_reliability", "7", "--l", "4"], ("--align_reliability", "--l 1"))):
        with pytest.raises(SystemExit) as e:
            D.main(base + extra)
        assert all(name in str(e.value) for name in names), (extra, str(e.value))


def test_the_statistic_field_and_the_report_header(tmp_path, capsys):
    from types import SimpleNamespace
    from gswm_amd import align as AL, trace as T
    shared = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = T.build_parser().parse_args(shared + ["--align", "flips", "--align_window_reliability", "3", "--l", "2"])
    assert T._statistic_name(a) == "soft, 3 reliability levels per window bit over 4 alignments"
    a = T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_window_reliability", "15", "--l", "4"])
    assert T._statistic_name(a) == "soft, 15 reliability levels per window bit over 200 alignments"
    # without the flag nothing changes
    assert T._statistic_name(T.build_parser().parse_args(shared + ["--align", "d4", "--align_shift", "2", "--align_reliability", "15"])) == "soft, 15 reliability levels over 200 alignments"
    assert T._statistic_name(T.build_parser().parse_args(shared + ["--align", "d4", "--l", "4"])) == "soft"
    a.message_length = 64
    reg = T.Registry(8)
    reg.add("alice", bytes(8))
    c = T.Candidate("alice", 0, 9000, 60, -12.3456, (5, 2, -1))
    job = SimpleNamespace(path=str(tmp_path), files=[str(tmp_path / "x.png")])
    T._report(job, [T.TraceResult([c], "alice", None, (5, 2, -1))], a, reg, False)
    out = capsys.readouterr().out
    lines = (tmp_path / "trace.txt").read_text().splitlines()
    info = dict(ln.split(",", 1) for ln in lines[1:lines.index("=" * 40 + "Batch Start" + "=" * 40)])
    assert info["statistic"] == "soft, 15 reliability levels per window bit over 200 alignments" and info["alignments"] == "200"
    line = "x.png, user: alice, agreement, 0.9375, log10 p, -12.346, alignment: " + AL.describe((5, 2, -1))
    assert line in lines and line in out


def test_the_l1_names_are_untouched():
    """the l = 1 twins keep their refusals of l > 1 where they had one, and the l = 1 C entry points their argument lists"""
    from gswm_amd import _native as N, detect as D
    assert len(N.lib().gsw_level_rows_align.argtypes) == 12 and len(N.lib().gsw_level_counts_align.argtypes) == 16
    with pytest.raises(ValueError, match="reliability cannot be combined with align"):
        D.detect_latents(torch.zeros(1, 4, 8, 8), L.keyring(), 32, reliability=3, align=L.FLIPS)
    assert KS.levels_of_planes(np.zeros((1, 2, 4), dtype=np.uint8)).shape == (1, 32)
