"""Blind detection ranked by reliability levels, host side: the Chernoff bound `detect.log10_p_blind_soft` against the unit-level
bound and the exact tail it must lie above, against brute-force enumeration, its shape and refusals, and against the independent restatement of
tests/key_search_soft_reference.py; the front end's flag, the refusals of `detect_latents`, the status codes gsw_key_search_soft_topk returns before any
launch, and the end-to-end experiment of tests/test_gpu_key_search_soft.py on the restatement alone (so that its seed is known to satisfy it).  No GPU."""
import ctypes
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import key_search_reference as R0  # noqa: E402
import key_search_soft_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def D():
    import gswm_amd  # noqa: F401
    from gswm_amd import detect
    return detect


# ------------------------------------------------------------------------------------------------ log10_p_blind_soft
def test_unit_levels_give_the_chernoff_bound_of_the_sign_statistic(D):
    M, V = 64, 64
    ones = np.ones(M * V, dtype=np.int64)
    for s in (600, 800, 1200, 4096):
        got, want = D.log10_p_blind_soft(s, ones, M), D._chernoff_log10(s, M, V)
        print(f"s {s}: soft bound {got:.12f}, unit-level Chernoff {want:.12f}, exact tail {D.log10_p_blind(s, M, V):.6f}")
        assert abs(got - want) <= 1e-9, (s, got, want)


def test_the_bound_lies_above_the_exact_tail(D):
    for M, V in ((64, 64), (8, 16), (16, 5)):
        ones = np.ones(M * V, dtype=np.int64)
        for s in range(0, M * V + 1, max(1, M * V // 97)):
            assert D.log10_p_blind_soft(s, ones, M) >= D.log10_p_blind(s, M, V) - 1e-12, (M, V, s)
        assert D.log10_p_blind_soft(M * V, ones, M) == pytest.approx(D.log10_p_blind(M * V, M, V), abs=1e-9)      # exact at the top


@pytest.mark.parametrize("levels", [(3, 1, 0, 7, 2, 15), (1, 1, 1, 1, 1, 1), (0, 5, 0, 5, 0, 9), (15, 14, 13, 12, 11, 10)])
def test_brute_force_over_all_sign_patterns(D, levels):
    """M = 2, V = 3: the 64 patterns of the six coins.  The true tail is <= 10^bound at every s and equal at the top."""
    M, V = 2, 3
    lv = np.array(levels, dtype=np.int64)                                   # element j on position j mod 2
    total = int(lv.sum())
    S = []
    for d in itertools.product((0, 1), repeat=M * V):
        x = (lv * (2 * np.array(d) - 1)).reshape(V, M).sum(axis=0)
        S.append(int(np.abs(x).sum()))
    S = np.array(S)
    assert S.max() == total
    for s in range(total + 1):
        tail = float((S >= s).sum()) / 64.0
        assert tail <= 10.0 ** D.log10_p_blind_soft(s, lv, M) * (1 + 1e-12), (s, tail)
    assert 10.0 ** D.log10_p_blind_soft(total, lv, M) == pytest.approx(float((S == total).sum()) / 64.0, rel=1e-12)


def test_shape_and_refusals(D):
    rng = np.random.default_rng(5)
    M = 16
    lv = rng.integers(0, 16, 64 * M)
    lv[3::M] = 0                                                            # a position without any weight: 0 with certainty
    law = D._SoftNullLaw(lv, M)
    total = int(lv.sum())
    assert law.total == total
    vals = [law.log10_bound(s) for s in range(0, total + 1, 37)] + [law.log10_bound(total)]
    assert vals[0] == 0.0 and law.log10_bound(int(law.mean0)) == 0.0 and all(math.isfinite(v) for v in vals)
    assert all(a >= b for a, b in zip(vals, vals[1:])) and vals[-1] < -200
    nz = (lv.reshape(64, M) > 0).sum(axis=0)
    assert vals[-1] == pytest.approx(sum((1 - int(c)) * math.log10(2.0) for c in nz if c > 0), abs=1e-9)       # prod_t 2 * 2^-(nonzero weights at t)
    assert D.log10_p_blind_soft(total, lv, M) == vals[-1]
    for bad in (-1, total + 1):
        with pytest.raises(ValueError, match="outside"):
            D.log10_p_blind_soft(bad, lv, M)
    with pytest.raises(ValueError, match="whole copies"):
        D.log10_p_blind_soft(0, lv[:-1], M)
    with pytest.raises(ValueError, match="levels must be in"):
        D.log10_p_blind_soft(0, lv + 1, M)
    with pytest.raises(ValueError, match="levels must be in"):
        D.log10_p_blind_soft(0, lv - 1, M)
    with pytest.raises(ValueError, match="integer"):
        D.log10_p_blind_soft(0, lv.astype(np.float64), M)
    doc = D.log10_p_blind_soft.__doc__
    assert "UPPER BOUND" in doc and "NOT the tail" in doc and "decades" in doc


def test_the_recursion_in_logarithms_is_the_recursion_in_probabilities(D, monkeypatch):
    rng = np.random.default_rng(9)
    lv = rng.integers(0, 16, 40 * 8)
    lin = D._SoftNullLaw(lv, 8)
    monkeypatch.setattr(D._SoftNullLaw, "LINEAR_MAX_COPIES", 0)
    log = D._SoftNullLaw(lv, 8)
    assert np.allclose(np.exp(lin.lp), np.exp(log.lp), rtol=1e-12, atol=0.0) and np.array_equal(np.isinf(lin.lp), np.isinf(log.lp))
    for s in (0, int(lin.mean0) + 50, lin.total // 2, lin.total):
        assert lin.log10_bound(s) == pytest.approx(log.log10_bound(s), abs=1e-9)
    # 2000 copies of unit weight: beyond float64 probabilities (2^-2000), finite in logarithms and exact at the top
    monkeypatch.undo()
    tall = D._SoftNullLaw(np.ones(2000 * 2, dtype=np.int64), 2)
    assert tall.log10_bound(4000) == pytest.approx(2 * (1 - 2000) * math.log10(2.0), rel=1e-12)
    assert tall.log10_bound(3000) == pytest.approx(D._chernoff_log10(3000, 2, 2000), abs=1e-9)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_bound_equals_the_independent_restatement(D):
    """both minimise the same convex function of theta; at the minimum an error e in theta costs e^2 K'' / 2, so 1e-9 decades is ample for either search"""
    rng = np.random.default_rng(21)
    for M, V, top in ((64, 64, 15), (8, 12, 3), (24, 7, 7)):
        lv = rng.integers(0, top + 1, M * V)
        law = D._SoftNullLaw(lv, M)
        laws = R.position_laws(lv, M)
        for s in sorted({0, int(law.mean0), int(law.mean0) + 1, int(law.mean0 * 1.2), int(law.mean0 * 2), law.total - 1, law.total}):
            if 0 <= s <= law.total:
                assert law.log10_bound(s) == pytest.approx(R.log10_bound(s, lv, M, laws), abs=1e-9), (M, V, s)
    planes = rng.integers(0, 256, (3, 4, 32), dtype=np.uint8)
    assert np.array_equal(D.levels_from_planes(planes), R.levels_of_planes(planes))
    assert np.array_equal(R.planes_of_levels(R.levels_of_planes(planes), 4), planes)


def test_restatement_with_unit_levels_is_the_sign_search(D):
    rng = np.random.default_rng(3)
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(5)]
    signs = rng.integers(0, 256, (3, 72), dtype=np.uint8)
    ks = R.keystreams(pairs, 576)
    for mb in (8, 9):
        assert np.array_equal(R.stats(signs, np.ones((3, 576), dtype=np.int64), ks, mb), R0.stats(signs, ks, mb))
    S = R.stats(signs, rng.integers(0, 16, (3, 576)), ks, 9)
    idx, st = R.topk(S, 8)
    assert idx[:, 5:].tolist() == [[-1] * 3] * 3 and st[0, 5:].tolist() == [R.INT32_MIN] * 3 and np.array_equal(idx[:, :5], np.argsort(-S, axis=1, kind="stable"))


def test_end_to_end_experiment_holds_on_the_restatement(D):
    """tests/test_gpu_key_search_soft.py's end-to-end case on the oracle's latents with the SAME uniforms and noise: 15 levels name all six keys at fpr 1e-4,
    the sign statistic at most three; four unwatermarked images name no key.  The device's latents differ from these by the embed's rounding (<= 1e-5 before
    noise of sigma 5 and the fp16 rounding), so every bound here keeps 0.3 decades from the limit.  (Printed: the bounds this seed gives.)"""
    from gswm_amd import soft, trace
    E = R.E2E
    pairs, msgs, u, noise, blank = R.e2e_setup()
    ks = R.keystreams(pairs, u.shape[1])
    z = (torch.from_numpy(R.e2e_host_latents(pairs, msgs, u)).float() + E["sigma"] * noise).half()
    limit = math.log10(E["fpr"])
    res = R.detect_soft_host(z, soft.uniform_thresholds(z, E["levels"]).numpy(), ks, E["msg_bytes"], trace.log10_p_any)
    sign = R0.detect_host(z, ks, E["msg_bytes"], D.log10_p_blind, trace.log10_p_any)
    print(f"15 levels: log10 p_any {[round(float(r[2]), 2) for r in res]}\nsigns:     log10 p_any {[round(float(r[2]), 2) for r in sign]}")
    assert [r[0] for r in res] == list(E["rows"]) and all(r[2] <= limit - 0.3 for r in res)
    assert sum(1 for r in sign if r[2] <= limit) <= 3 and all(abs(r[2] - limit) >= 0.3 for r in sign)
    bz = blank.half()
    none = R.detect_soft_host(bz, soft.uniform_thresholds(bz, E["levels"]).numpy(), ks, E["msg_bytes"], trace.log10_p_any)
    print(f"unwatermarked: log10 p_any {[round(float(r[2]), 2) for r in none]}")
    assert all(r[2] > limit + 1.0 for r in none)


# ------------------------------------------------------------------------------------------------ front end, wrappers
def test_cli_flag_and_detect_latents_refusals(D, capsys):
    base = ["--keyring", "ring.tsv"]
    assert D.build_parser().parse_args(base).reliability == 0
    assert D.build_parser().parse_args(base + ["--reliability", "15"]).reliability == 15
    for bad in ("16", "-1", "x"):
        with pytest.raises(SystemExit):
            D.build_parser().parse_args(base + ["--reliability", bad])
        assert "--reliability" in capsys.readouterr().err
    for extra in (["--l", "2"], ["--align", "flips"]):
        with pytest.raises(SystemExit, match="--reliability"):
            D.main(base + ["--reliability", "3"] + extra)
    ring = D.Keyring()
    ring.add("a", bytes(32), bytes(16))
    z = torch.zeros(2, 4, 8, 8)
    for bad in (16, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="reliability"):
            D.detect_latents(z, ring, 8, reliability=bad)
    with pytest.raises(ValueError, match="l = 2"):
        D.detect_latents(z, ring, 8, reliability=3, l=2)
    with pytest.raises(ValueError, match="align"):
        D.detect_latents(z, ring, 8, reliability=3, align=[(0, 0, 0)])
    with pytest.raises(ValueError, match="k must be"):
        D.detect_latents(z, ring, 8, reliability=3, k=9)
    with pytest.raises(ValueError, match="empty"):
        D.detect_latents(z, D.Keyring(), 8, reliability=3)
    with pytest.raises(IndexError):
        D.detect_latents(torch.zeros(1, 4, 10, 10), ring, 256, reliability=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.detect_latents(z, ring, 8, reliability=3)
    from gswm_amd import codec
    rows = codec.LevelRows(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 2, 32, dtype=torch.uint8), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.key_search_soft_topk(rows, 256, torch.zeros(4, 48, dtype=torch.uint8), 32)
    assert D.format_line("a.png", D.DetectResult([D.KeyCandidate("k7", 7, 90000, -12.25)], "k7", b"\x01", 0)) == "a.png, key: k7, log10 p, -12.250, message: 01"


# ------------------------------------------------------------------------------------------------ status codes that need no device
def test_c_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(72)                          # never dereferenced: every call below is refused before a launch

    def call(signs=p, planes=p, P=1, B=1, n=256, keys=p, stride=48, mb=4, K=1, k=1, idx=p, stat=p, ws=p):
        return lib.gsw_key_search_soft_topk(signs, planes, P, B, n, keys, stride, mb, K, k, idx, stat, ws, None)

    bad = [dict(signs=None), dict(planes=None), dict(keys=None), dict(idx=None), dict(stat=None), dict(ws=None), dict(P=0), dict(P=5), dict(P=-1),
           dict(B=0), dict(B=-3), dict(k=0), dict(k=9), dict(mb=0), dict(mb=257), dict(n=0), dict(n=-256), dict(K=0), dict(K=-1), dict(K=2 ** 31),
           dict(stride=32), dict(stride=47), dict(stride=56), dict(stride=0), dict(keys=odd)]
    for kw in bad:
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(n=264), dict(n=8), dict(n=24, mb=2), dict(n=1048576 + 8)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    # the domain is the level search's: n_bits (1 + P) <= 1 048 576
    for kw in (dict(n=524288 + 32), dict(n=349536, P=2), dict(n=262144 + 32, P=3), dict(n=209728, P=4), dict(n=1 << 21), dict(B=65536)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw
    assert call(n=264, k=9) == N.GSW_ERR_BAD_ARG and call(n=(1 << 21) + 8) == N.GSW_ERR_RAGGED
    ws = lib.gsw_key_search_soft_workspace_bytes
    for B, K, k in ((0, 5, 1), (1, 0, 1), (1, 2 ** 31, 1), (1, 5, 0), (1, 5, 9)):
        assert ws(B, K, k) == 0, (B, K, k)
    assert ws(1, 1, 1) == 8 and ws(3, 5, 2) == 3 * 5 * 2 * 8 and ws(2, 2 ** 31 - 1, 8) == ws(2, 100000, 8) > 0
    assert lib.gsw_version() == 500
    fn = lib.gsw_key_search_soft_topk
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14 and fn.argtypes[4] is ctypes.c_int64 and fn.argtypes[6] is ctypes.c_int64
    assert {"gsw_key_search_soft_topk", "gsw_key_search_soft_workspace_bytes"} <= set(N.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_key_search_soft_topk(" in hdr and "size_t gsw_key_search_soft_workspace_bytes(" in hdr
