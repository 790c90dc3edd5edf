"""CPU (no GPU): pooled evidence across the images of a set before any device is asked -- the launch policy of gsw_pool_rows and gsw_trace_keyed_pooled_topk
swept by a host-only program (tests/pool_plan_cases.cpp over csrc/gswm_pool_plan.h), the C entry points' refusals, the restatement of tests/pool_reference.py
on patterns and on the case pooling is built for (16 images under one record among 1000, sigma 13.5, fpr 1e-6: alone none is attributed, pooled the set is,
asserted on the restatement alone), the parser and the report."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pool_reference as PR
from conftest import ROOT


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, soft, trace
    assert hasattr(trace, "trace_sets_keyed") and hasattr(trace, "trace_sets") and hasattr(codec, "pool_rows") and hasattr(codec, "trace_keyed_pooled_topk")
    return codec, soft, trace


# ------------------------------------------------------------------------------------------------ the launch policy
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("pool_plan") / "pool_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pool_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """Every refusal has the status the specification gives it, in the order BAD_ARG, RAGGED, UNSUPPORTED (restated with 128-bit products), and decides
    nothing.  For every accepted pooling: Q in 1..10 holds Lmax max_set, one workgroup per set, a power of two of lanes in 64..512 that is no larger than
    the row needs, dword access only for aligned whole-dword rows, n (2^Q - 1) within int32.  For every accepted search: the tile is 1, 4 or 16, filled
    by the sets and the largest whose (1 + Q) padded rows fit 128 KiB; the LDS holds the rows and the top-k tail within the cap; the grid covers every set
    once and no record range is empty; the workspace is gsw_trace_keyed_workspace_bytes(G, U, k)."""
    words = sweep.stderr.split()
    assert int(words[0]) > 1000000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_refusal_and_every_path(sweep):
    seen = set(sweep.stderr.split()[4:])
    want = {"rows_bad_arg", "rows_unsupported", "rows_wg64", "rows_wg128", "rows_wg512", "rows_q1", "rows_q10", "rows_dwords", "rows_bytes",
            "search_bad_arg", "search_ragged", "search_unsupported", "search_t1", "search_t4", "search_t16", "search_q1", "search_q10", "search_msg4",
            "search_msg_bytes", "search_lds_at_cap", "search_tile_cut_by_lds"}
    assert seen >= want, want - seen


# ------------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_pool_rows_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd, odd8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)      # never dereferenced: every call below is refused before a launch

    def call(signs=p, planes=None, P=0, B=3, n=64, sp=p, G=1, ms=3, Q=2, os_=p, op=p, wsum=p, wsq=p):
        return lib.gsw_pool_rows(signs, planes, P, B, n, sp, G, ms, Q, os_, op, wsum, wsq, None)

    for kw in (dict(signs=None), dict(sp=None), dict(os_=None), dict(op=None), dict(wsum=None), dict(wsq=None), dict(planes=p), dict(P=2), dict(sp=odd),
               dict(wsum=odd), dict(wsq=odd8), dict(P=-1), dict(P=5, planes=p), dict(B=0), dict(G=0), dict(G=4), dict(ms=0), dict(ms=4), dict(n=0), dict(n=60),
               dict(Q=0), dict(Q=1), dict(P=4, planes=p, B=5, ms=5, Q=6)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(Q=11), dict(P=4, planes=p, B=69, ms=69, Q=10), dict(P=4, planes=p, B=69, ms=69, Q=11), dict(B=1024, ms=1024, Q=10), dict(B=1024, ms=1024, Q=11),
               dict(B=1, ms=1, Q=1, n=524296), dict(n=2 ** 21), dict(P=4, planes=p, B=68, ms=68, Q=10, n=95328)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw


def test_pooled_search_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)

    def call(signs=p, planes=p, wsum=p, Q=5, G=3, n=256, rec=p, stride=80, mb=32, U=10, k=1, idx=p, score=p, ws=p):
        return lib.gsw_trace_keyed_pooled_topk(signs, planes, wsum, Q, G, n, rec, stride, mb, U, k, idx, score, ws, None)

    for kw in (dict(signs=None), dict(planes=None), dict(wsum=None), dict(rec=None), dict(idx=None), dict(score=None), dict(ws=None), dict(wsum=odd),
               dict(rec=ctypes.c_void_p(72)), dict(Q=0), dict(G=0), dict(n=0), dict(k=0), dict(k=9), dict(U=0), dict(U=2 ** 31), dict(mb=0), dict(mb=257),
               dict(stride=64), dict(stride=88), dict(Q=0, n=264)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(n=264), dict(n=264, Q=11, G=65536), dict(mb=5, stride=64, n=256)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    for kw in (dict(Q=11), dict(Q=10, n=95488), dict(G=65536), dict(n=2 ** 21), dict(Q=10, n=95320, mb=5, stride=64, G=1)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw


def test_symbols_are_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    assert lib.gsw_version() == 500
    for name, nargs in (("gsw_pool_rows", 14), ("gsw_trace_keyed_pooled_topk", 15)):
        assert name in N.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_pool_rows(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int64_t n_bits, const int32_t* set_ptr_dev, int G, int max_set, int Q," in hdr
    assert "int gsw_trace_keyed_pooled_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, const int32_t* wsum_dev, int Q, int G, int64_t n_bits," in hdr
    import __graft_entry__ as E
    assert {"gswm_pool.inc", "gswm_pool_plan.h"} <= set(E.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert "gswm_pool.inc" in rule and "gswm_pool_plan.h" in rule
    src = open(os.path.join(csrc, "gswm_keyed.hip")).read()
    assert src.index('#include "gswm_counts_align_soft.inc"') < src.index('#include "gswm_pool.inc"')
    assert "gsw_pool_rows" in open(os.path.join(csrc, "gswm.map")).read()


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_patterns():
    """a set of one is the image itself; opposite signs at equal levels cancel to sign 0, level 0; copies multiply S and leave the bound of the best record
    where it was; the pooled score is the sum of the per-image scores"""
    rng = np.random.default_rng(3)
    n, B = 64, 6
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    lv = rng.integers(0, 4, (B, n), dtype=np.int64)
    planes = np.stack([np.packbits(((lv >> k) & 1).astype(np.uint8), axis=1) for k in range(2)], axis=1)
    one = PR.pool_rows(signs, planes, [[2]])
    assert np.array_equal(one["signs"][0] & np.packbits((lv[2] > 0).astype(np.uint8)), one["signs"][0])      # level 0: sign 0
    assert np.array_equal(one["planes"][0], planes[2]) and one["wsum"][0] == lv[2].sum() and one["wsq"][0] == (lv[2] ** 2).sum() and one["Q"] == 2
    pair_s = np.stack([signs[0], ~signs[0]])
    pair = PR.pool_rows(pair_s, np.stack([planes[0], planes[0]]), [[0, 1]])
    assert not pair["signs"].any() and not pair["planes"].any() and pair["wsum"][0] == 0 and pair["wsq"][0] == 0
    cw = rng.integers(0, 256, (9, n // 8), dtype=np.uint8)
    S = PR.signed_sums(signs, planes, [[0, 1, 2], [3], [1, 1, 1]])
    per_image = PR.scores(PR.signed_sums(signs, planes, [[b] for b in range(B)]), cw)
    assert np.array_equal(PR.scores(S, cw), np.stack([per_image[:3].sum(axis=0), per_image[3], 3 * per_image[1]]))
    s1, q1 = int(per_image[1].max()), int((PR.signed_sums(signs, planes, [[1]]) ** 2).sum())
    assert PR.bound(3 * s1, int((S[2] ** 2).sum()), 9) == pytest.approx(PR.bound(s1, q1, 9), abs=1e-12)
    packed = PR.pool_rows(signs, planes, [[0, 1, 2], [3], [1, 1, 1]])
    assert np.array_equal(PR.sums_of_rows(packed["signs"], packed["planes"], packed["wsum"]), S) and packed["Q"] == 4


def test_the_restatement_alone_meets_the_end_to_end_case(G):
    """sigma 13.5 on the oracle's latents: every single image stays at least a decade above the limit under BOTH of its bounds (Hoeffding's for a set of one,
    the exact tail of trace_latents_keyed), the pooled set lies at least a decade below; eight copies of one image have that image's own bound; 16
    unwatermarked latents name nobody; 8 + 8 images of two users with k = 2 report exactly those two.  The figures are in the README."""
    codec, S, T = G
    E = PR.E2E
    limit = math.log10(E["fpr"])
    B, U, n = E["B"], E["U"], int(np.prod(E["shape"]))
    recs, cw, u, noise = PR.e2e_setup()
    z = PR.e2e_oracle_latents(recs, u[:B], [E["owner"]] * B)
    signs = PR.sign_rows(PR.held(z, noise).numpy())
    flags = np.zeros(2 * B, dtype=np.int64)
    singles = PR.trace_sets(signs, None, flags, [[b] for b in range(B)], recs, cw, 1, E["fpr"])
    hoeffding = [r["candidates"][0][3] for r in singles]
    exact = [T.log10_p_any(T.log10_p_soft(r["candidates"][0][1], n), U) for r in singles]
    print("single images, Hoeffding:", [round(x, 2) for x in hoeffding], "exact tail:", [round(x, 2) for x in exact])
    assert min(hoeffding) >= limit + 1 and min(exact) >= limit + 1 and all(r["attributed"] is None for r in singles)
    pooled = PR.trace_sets(signs, None, flags, [list(range(B))], recs, cw, 2, E["fpr"])[0]
    print("pooled:", pooled["candidates"], "wsq", pooled["wsq"])
    assert pooled["attributed"] == E["owner"] and pooled["candidates"][0][3] <= limit - 1 and pooled["candidates"][1][3] > limit
    assert pooled["candidates"][0][2] > 0.75 * 8 * E["msg_bytes"] and pooled["size"] == B and pooled["skipped"] == 0
    # eight copies of one image: S is 8 times the image's, the bound its own
    copies = PR.trace_sets(np.repeat(signs[:1], 8, axis=0), None, flags, [list(range(8))], recs, cw, 1, E["fpr"])[0]
    assert copies["candidates"][0][0] == singles[0]["candidates"][0][0] and copies["candidates"][0][1] == 8 * singles[0]["candidates"][0][1]
    assert copies["candidates"][0][3] == pytest.approx(singles[0]["candidates"][0][3], abs=1e-9) and copies["wsq"] == 64 * n
    # unwatermarked latents (the uniforms alone) under the same noise
    blank = PR.sign_rows(PR.held(np.asarray(torch.special.ndtri(torch.from_numpy(u[:B]).clamp(1e-12, 1 - 1e-12)), dtype=np.float32), noise).numpy())
    nobody = PR.trace_sets(blank, None, flags, [list(range(B))], recs, cw, 1, E["fpr"])[0]
    assert nobody["attributed"] is None and nobody["candidates"][0][3] > limit + 1
    # two users, eight images each
    z2 = PR.e2e_oracle_latents(recs, u[:B], [E["owner"]] * 8 + [E["other"]] * 8)
    two = PR.trace_sets(PR.sign_rows(PR.held(z2, noise).numpy()), None, flags, [list(range(B))], recs, cw, 3, E["fpr"])[0]
    print("two users:", two["candidates"])
    assert {c[0] for c in two["candidates"][:2]} == {E["owner"], E["other"]} and all(c[3] <= limit for c in two["candidates"][:2])
    assert two["candidates"][2][3] > limit
    # flagged images are left out and counted; a set of flagged images alone is left empty
    flags[3] = 2
    flags[5] = 1
    part = PR.trace_sets(signs, None, flags, [list(range(B)), [3, 5]], recs, cw, 1, E["fpr"])
    assert part[0]["size"] == B - 2 and part[0]["skipped"] == 2 and part[0]["attributed"] == E["owner"] and part[1] is None


# ------------------------------------------------------------------------------------------------ the public surface
def test_parser_acceptance_and_refusals_by_name(capsys):
    from gswm_amd import trace as T
    keyed = ["--registry", "r.tsv", "--per_record_keys"]
    shared = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = T.build_parser().parse_args(shared)
    assert a.pool is None and a.pool_reliability is None
    a = T.build_parser().parse_args(keyed + ["--pool", "all", "--pool_reliability", "15", "--top", "3"])
    assert (a.pool, a.pool_reliability, a.top) == ("all", 15, 3)
    a = T.build_parser().parse_args(shared + ["--pool", "subdirs", "--is_traverse_subdirectories", "1", "--l", "4"])
    assert (a.pool, a.pool_reliability, a.l) == ("subdirs", None, 4)
    for extra, names in ((shared + ["--pool", "all", "--hard"], ("--pool", "--hard")),
                         (shared + ["--pool", "all", "--align", "d4"], ("--pool", "--align")),
                         (keyed + ["--pool", "all", "--tamper_map", "maps"], ("--pool", "--tamper_map")),
                         (keyed + ["--pool_reliability", "7"], ("--pool_reliability", "--pool")),
                         (keyed + ["--pool", "all", "--pool_reliability", "7", "--l", "2"], ("--pool_reliability", "--l 2")),
                         (shared + ["--pool", "all", "--pool_reliability", "7", "--l", "4"], ("--pool_reliability", "--l 4")),
                         (keyed + ["--pool", "subdirs"], ("--pool subdirs", "--is_traverse_subdirectories")),
                         (keyed + ["--pool", "all", "--pool_reliability", "0"], ("--pool_reliability",)),
                         (keyed + ["--pool", "all", "--pool_reliability", "16"], ("--pool_reliability",)),
                         (keyed + ["--pool", "some"], ("--pool",))):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(extra)
        err = capsys.readouterr().err
        assert all(name in err for name in names), (extra, err)


def test_the_report_header_and_set_lines(tmp_path, capsys):
    """`_report` on a made-up job: the per-image line is what it was, the set lines follow it, the header gains `pool` and `pool_reliability`"""
    from types import SimpleNamespace
    from gswm_amd import trace as T
    keyed = ["--registry", "r.tsv", "--per_record_keys"]
    reg = T.KeyedRegistry(8)
    reg.add("alice", bytes(32), bytes(16), bytes(8))
    c = T.Candidate("alice", 0, 9000, 60, -12.3456)
    job = SimpleNamespace(path=str(tmp_path), files=[str(tmp_path / "x.png")])
    sets = [T.format_set_line("leak", T.SetTraceResult([c, T.Candidate("bob", 1, 100, 30, 0.0)], "alice", 16, 2, 123456)),
            T.format_set_line("noise", T.SetTraceResult([T.Candidate("bob", 1, 100, 30, -1.5)], None, 3, 0, 99)),
            T.format_set_line("broken", ValueError("cannot convert float NaN to integer"))]
    assert sets == ["set leak, images, 16, skipped, 2, user: alice, log10 p, -12.346, score, 9000, next: bob (0.000, 100)",
                    "set noise, images, 3, skipped, 0, user: none, log10 p, -1.500, score, 100",
                    "set broken, Error: cannot convert float NaN to integer"]
    for extra, fields in ((["--pool", "all"], {"pool": "all"}), (["--pool", "all", "--pool_reliability", "15"], {"pool": "all", "pool_reliability": "15"}), ([], {})):
        a = T.build_parser().parse_args(keyed + extra)
        a.message_length = 64
        (tmp_path / "trace.txt").unlink(missing_ok=True)
        T._report(job, [T.TraceResult([c], "alice")], a, reg, False, sets if extra else ())
        out = capsys.readouterr().out
        lines = (tmp_path / "trace.txt").read_text().splitlines()
        start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
        info = dict(l.split(",", 1) for l in lines[1:start])
        assert {k: info.get(k) for k in ("pool", "pool_reliability")} == {"pool": fields.get("pool"), "pool_reliability": fields.get("pool_reliability")}
        assert lines[start + 1] == "x.png, user: alice, agreement, 0.9375, log10 p, -12.346"
        assert lines[start + 2:-1] == (sets if extra else []) and all(s in out for s in (sets if extra else []))


def test_levels_and_windows_are_refused_by_name(G):
    codec, S, T = G
    for levels, l, match in ((16, 1, "levels"), (-1, 1, "levels"), (True, 1, "levels"), (7, 2, "l = 2"), (15, 4, "l = 4"), (0, 3, "l")):
        with pytest.raises(ValueError, match=match):
            T._pool_levels(levels, l)
    assert T._pool_levels(0, 4) == (0, 4) and T._pool_levels(15, 1) == (15, 1)
    assert codec.pool_planes(0, 1) == 1 and codec.pool_planes(0, 1023) == 10 and codec.pool_planes(4, 68) == 10 and codec.pool_planes(2, 5) == 4
    with pytest.raises(ValueError, match="1023"):
        codec.pool_planes(0, 1024)
    with pytest.raises(ValueError, match="68"):
        codec.pool_planes(4, 69)


def test_host_tensors_are_refused_without_a_fallback(G):
    """there is no CPU path: the usual RuntimeError, before any launch"""
    codec, S, T = G
    with pytest.raises(RuntimeError):
        codec.pool_rows(torch.zeros(2, 8, dtype=torch.uint8), None, [2])
    rows = codec.PooledRows(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 1, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                            torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        codec.trace_keyed_pooled_topk(rows, 64, torch.zeros(3, 64, dtype=torch.uint8), 8)
    reg = T.KeyedRegistry(8)
    reg.add("alice", bytes(32), bytes(16), bytes(8))
    with pytest.raises(RuntimeError):
        T.trace_sets_keyed(torch.zeros(2, 1, 8, 8), [[0, 1]], reg)


def test_the_shared_registry_becomes_keyed_records():
    from gswm_amd import trace as T
    reg = T.Registry(4)
    reg.add("alice", b"\x01\x02\x03\x04")
    reg.add("bob", b"\xff\x00\xff\x00")
    key, nonce = bytes(range(32)), bytes(range(16))
    keyed = T.keyed_from_shared(reg, key, nonce)
    assert keyed.user_ids == ["alice", "bob"] and keyed.record_at(1) == (key, nonce, b"\xff\x00\xff\x00") and keyed.n_keys == 1
    assert T.keyed_from_shared(reg, key, nonce, 64).record_at(0)[2] == b"\x01\x02\x03\x04" * 2
