"""CPU (no GPU): the launch policy of the searches over packed sign rows is one pure function (csrc/gswm_search_plan.h: search_decide), and
tests/golden/search_plan_cases.tsv is its table -- one search per row, the inputs of search_decide and the decision the three entry points took for them (recorded
from gsw_trace_keyed_topk, gsw_trace_keyed_soft_topk, gsw_key_search_topk and the two workspace queries as they were before the policy became one function; a later
change of policy shows as a diff of the table).  tests/search_plan_cases.cpp, a host-only program, prints search_decide's answer per row; every column must be
equal, as strings.  The table must also cover the policy, and a sweep over a grid wider than the table asserts the invariants of a launch that no kernel checks."""
import collections
import csv
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "search_plan_cases.tsv")
DECISION = "status T msg4 planes sg G kpi srow copies rowbytes nblk signs_aligned grid_x grid_y wg lds ws_bytes ws_query".split()
SIGN, LEVEL, KEY = "0", "1", "2"
OK, BAD_ARG, UNSUPPORTED, RAGGED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def table():
    with open(TABLE, newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t"))
    assert 300 <= len(rows) <= 3000
    return rows


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("search_plan") / "search_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    os.path.join(ROOT, "tests", "search_plan_cases.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_search_decide_reproduces_the_recorded_decisions(table, program):
    out = subprocess.run([program, TABLE], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(table)
    bad = []
    for line, want in zip(out, table):
        got = line.split("\t")
        assert got[0] == want["tag"] and len(got) == 1 + len(DECISION)
        diff = [(c, g, want[c]) for c, g in zip(DECISION, got[1:]) if g != want[c]]
        if diff:
            bad.append((want["tag"], diff))
    assert not bad, (len(bad), bad[:10])


def test_the_table_covers_the_policy(table):
    by_tag = {r["tag"]: r for r in table}
    assert len(by_tag) == len(table)
    ok = [r for r in table if r["status"] == "0"]
    n = collections.Counter()

    def has(name, pred, rows=ok):
        n[name] = sum(1 for r in rows if pred(r))

    def tag(name, **want):
        """the row with this tag exists and its recorded decision is what the tag says"""
        r = by_tag.get(name)
        n[name] = int(r is not None and all(r[k] == str(v) for k, v in want.items()))

    i = lambda r, c: int(r[c])
    sign, level, key = ([r for r in ok if r["kind"] == kind] for kind in (SIGN, LEVEL, KEY))
    # the sign search: every tile x message form; the tile shrinking by LDS, at each edge and past it
    for T in (1, 4, 16, 64):
        for m in (0, 1):
            has(f"sign T={T} MSG4={m}", lambda r: r["T"] == str(T) and r["msg4"] == str(m), sign)
    for n_bits, T in ((16384, 64), (16640, 16), (65536, 16), (65792, 4), (262144, 4), (262400, 1), (1048576, 1)):
        tag(f"cover/sign/shrink_b64_n{n_bits}", T=T, status=OK)
    # the level search: P = 1..4, the (1 + P) shrink, the domain's edge at and one step past
    for P in (1, 2, 3, 4):
        has(f"level P={P}", lambda r: r["planes"] == str(P), level)
        for T in (16, 4, 1):
            has(f"level P={P} shrunk to T={T}", lambda r: r["planes"] == str(P) and r["B"] == "64" and r["T"] == str(T), level)
        has(f"level P={P}: a tile the sign search would not shrink", lambda r: r["planes"] == str(P) and r["B"] == "64" and i(r, "T") < 64 and 64 * i(r, "nblk") * 64 <= 131072,
            level)
        tag(f"cover/level/domain_p{P}_at", status=OK, T=1, planes=P)
        tag(f"cover/level/domain_p{P}_at_b64", status=OK, T=1, planes=P)
        tag(f"cover/level/domain_p{P}_past", status=UNSUPPORTED)
    # the key search: PL at the copies boundaries, SG at its edge, fast lost to misalignment under SG
    for copies, PL in ((15, 4), (16, 8), (255, 8), (256, 12), (4095, 12), (4096, 16)):
        tag(f"cover/key/copies{copies}_pl{PL}_b1", planes=PL, copies=copies, status=OK)
    has("PL = 0", lambda r: r["planes"] == "0" and i(r, "msg_bytes") % 4 != 0, key)
    tag("cover/key/sg_mb4_n523264_signs1_b1", sg=0, planes=16)
    tag("cover/key/sg_mb4_n523296_signs1_b1", sg=1, planes=16, T=1)
    tag("cover/key/sg_mb4_n523264_signs2_b1", sg=0, planes=16, signs_aligned=0)      # staged through LDS byte by byte: still the word path
    tag("cover/key/sg_mb4_n523296_signs2_b1", sg=1, planes=0, signs_aligned=0)       # read in place: the bit-by-bit path
    tag("cover/key/sg_mb4_n523296_signs1_b3", sg=1, T=1, grid_y=3)
    # G clipped by the units and by the tile; the bank offset; kpi clipped by LDS and by the keys
    for mb, G in ((4, 1), (8, 2), (16, 4), (32, 8), (64, 16), (128, 32), (256, 64), (1, 8), (2, 16), (3, 32), (7, 64)):
        tag(f"cover/key/g_mb{mb}_b1", G=G, T=1)
    tag("cover/key/g_by_tile_mb256_b64", G=4, T=64)
    tag("cover/key/g_by_tile_mb256_b16", G=16, T=16)
    tag("cover/key/g_by_tile_mb256_b4", G=64, T=4)
    has("bank offset taken", lambda r: r["sg"] == "0" and i(r, "G") < 32 and i(r, "srow") > 16 * i(r, "nblk") and i(r, "srow") % 32 == i(r, "G"), key)
    has("bank offset not needed", lambda r: r["sg"] == "0" and i(r, "G") < 32 and i(r, "srow") == 16 * i(r, "nblk"), key)
    has("bank offset not taken: G >= 32", lambda r: r["sg"] == "0" and i(r, "G") >= 32 and i(r, "srow") == 16 * i(r, "nblk") and i(r, "srow") % 32 != i(r, "G"), key)
    has("bank offset not taken: SG", lambda r: r["sg"] == "1" and i(r, "G") < 32 and i(r, "srow") == 16 * i(r, "nblk") and i(r, "srow") % 32 != i(r, "G"), key)
    full = lambda r: 256 // i(r, "G") // i(r, "T")
    has("kpi whole", lambda r: i(r, "kpi") == full(r), key)
    has("kpi clipped by LDS", lambda r: i(r, "kpi") < min(full(r), i(r, "n_records")), key)
    has("kpi clipped by LDS to 1", lambda r: i(r, "kpi") == 1 < min(full(r), i(r, "n_records")), key)
    has("kpi clipped by the keys", lambda r: i(r, "kpi") == i(r, "n_records") < full(r), key)
    for name, rows in (("walk", sign + level), ("key", key)):
        has(f"{name}: grid_x at its cap", lambda r: r["grid_x"] == "512", rows)
        has(f"{name}: grid_x below its cap", lambda r: 1 < i(r, "grid_x") < 512, rows)
        has(f"{name}: grid_x 1", lambda r: r["grid_x"] == "1", rows)
    has("key: grid_x below what the workspace holds", lambda r: i(r, "grid_x") * i(r, "B") * i(r, "k") * 8 < i(r, "ws_bytes"), key)
    for k in range(1, 9):
        has(f"k={k}", lambda r: r["k"] == str(k))
    # every refusal, one row per cause, in each search, and the pairs that fix which code wins
    errors = {"signs_null": BAD_ARG, "idx_null": BAD_ARG, "score_null": BAD_ARG, "workspace_null": BAD_ARG, "b_zero": BAD_ARG, "k_zero": BAD_ARG, "k_nine": BAD_ARG,
              "n_bits_zero": BAD_ARG, "records_2p31": BAD_ARG, "records_null": BAD_ARG, "records_zero": BAD_ARG, "msg_bytes_zero": BAD_ARG, "msg_bytes_257": BAD_ARG,
              "stride_short": BAD_ARG, "stride_not_16": BAD_ARG, "records_misaligned": BAD_ARG, "ragged": RAGGED, "n_bits_past_domain": UNSUPPORTED, "b_65536": UNSUPPORTED,
              "order/bad_arg_before_ragged": BAD_ARG, "order/bad_stride_before_ragged": BAD_ARG, "order/ragged_before_unsupported": RAGGED,
              "ok/signs_misaligned": OK, "ok/stride_with_room": OK}
    for name in ("sign", "level", "key"):
        for cause, status in errors.items():
            tag(f"err/{name}/{cause}", status=status)
    for cause, status in (("planes_null", BAD_ARG), ("wsum_null", BAD_ARG), ("levels_zero", BAD_ARG), ("levels_16", BAD_ARG), ("wsum_misaligned", BAD_ARG),
                          ("ok/planes_misaligned", OK), ("n_bits_past_domain_of_p4", UNSUPPORTED)):
        tag(f"err/level/{cause}", status=status)
    tag("err/level/ok/planes_misaligned", signs_aligned=0)
    tag("err/key/ok/stride_48_holds_no_message", status=OK)
    has("a refused search decides nothing", lambda r: all(r[c] == "0" for c in DECISION[1:-1]), [r for r in table if r["status"] != "0"])
    n["a refused search decides nothing"] = int(n["a refused search decides nothing"] == len(table) - len(ok))
    missing = sorted(k for k, v in n.items() if v == 0)
    print({k: v for k, v in n.items() if not k.startswith("err/")})
    assert not missing, missing


# What the sweep found in the decisions recorded from the entry points, kept as they were (this table changes no behaviour) and pinned here input by input:
# the level-weighted search sizes its tile by n_bits (1 + P) <= 1 048 576 but stages rows PADDED to whole 64-byte blocks, so with P = 2 or P = 4 -- where
# 131 072 / (1 + P) is no multiple of 64 -- the lattices whose last block is the partial one before the domain's edge ask for a little more than 128 KiB:
# 131 136 bytes (P = 2, rows of 43 649 .. 43 690 bytes) and 131 200 bytes (P = 4, rows of 26 177 .. 26 214 bytes), one image per workgroup.  The CU has 160 KiB,
# so the launch is granted; the "<= 131 072" of the design does not hold for exactly these rows.  Any other broken input, or another size for these, fails the test.
KNOWN_LDS_OVER_128K = {(2, 131136): range(43649, 43691), (4, 131200): range(26177, 26215)}


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(program):
    """LDS <= 131 072 bytes and >= what the top-k tail reuses; G a power of two <= 64 with G T kpi <= 256; kpi >= 1; srow >= 16 nblk; 1 <= grid_x <= the grid the
    workspace query sized for the same (B, n_records, k); grid_y T >= B; workspace = B x grid cap x k x 8 bytes (tests/search_plan_cases.cpp: broken)."""
    out = subprocess.run([program, "--sweep"], check=True, capture_output=True, text=True)
    swept = int(out.stderr.split()[0])
    assert swept > 1000000
    unknown, seen = [], set()
    for line in out.stdout.splitlines():
        f = line.split("\t")
        kv = dict(c.split("=") for c in f[1:])
        P = {1: 1, 2: 2, 3: 2, 4: 3, 7: 3, 8: 4, 15: 4}.get(int(kv.get("levels", 0)))
        known = KNOWN_LDS_OVER_128K.get((P, int(kv.get("lds", 0))))
        if f[0] == "lds<=131072" and kv["kind"] == LEVEL and known is not None and int(kv["n_bits"]) // 8 in known:
            seen.add(P)
        else:
            unknown.append(line)
    assert not unknown, (len(unknown), unknown[:10])
    assert seen == {2, 4}          # the sweep does reach the two findings: it would see them change
