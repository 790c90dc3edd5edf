"""CPU (no GPU): the alignment search ranked by reliability levels -- the launch policy of gsw_level_rows_align (csrc/gswm_align_soft.inc:
level_align_decide, swept by tests/level_align_plan_cases.cpp), the status codes the entry point returns before any launch, the public surface (export,
header, ctypes prototype, CLI flag and its refusals, the wrappers' errors on host tensors), `_merge_best` with the wider statistic, and the end-to-end
experiment of tests/align_soft_reference.py on the restatement alone, so that its seed is known to satisfy the conditions the GPU test relies on."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_reference as AR
import align_soft_reference as ASR
import key_search_reference as R
from conftest import ROOT

import gswm_amd
from gswm_amd import _native as N, align as AL, codec, detect as D, soft, trace as T


# ------------------------------------------------------------------------------------------------------------ the launch policy
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("level_align_plan") / "level_align_plan_cases"
    # the library's compiler on host code only, the library's optimisation level
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "level_align_plan_cases.cpp"), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


def test_a_sweep_of_inputs_keeps_the_invariants_of_a_launch(sweep):
    """LDS <= 65 536 bytes and exactly the 1 + P padded rows, or none with SG and then only when they do not fit; the chunk in 1..16 and never so large that
    the grid falls below its target; grid_x chunks cover A exactly once, grid_y = B <= 65 535; every refusal has its status and decides nothing."""
    words = sweep.stderr.split()
    assert int(words[0]) > 40000 and words[1] == "inputs,"
    assert not sweep.stdout, (words[2], sweep.stdout.splitlines()[:10])
    assert words[2] == "0"


def test_the_sweep_reaches_every_class_of_the_policy(sweep):
    seen = set(sweep.stderr.split()[4:])
    assert {"lds", "sg", "chunk1", "chunk3", "chunk16"} <= seen, seen


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_status_codes_before_any_launch():
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                          # never dereferenced: every call below is refused before a launch

    def call(signs=p, planes=p, P=2, B=1, C=4, H=8, W=8, al=p, A=1, out_s=p, out_p=p):
        return lib.gsw_level_rows_align(signs, planes, P, B, C, H, W, al, A, out_s, out_p, None)

    for kw in (dict(signs=None), dict(planes=None), dict(al=None), dict(out_s=None), dict(out_p=None), dict(al=odd), dict(P=0), dict(P=5), dict(P=-1),
               dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(A=0), dict(A=-2), dict(P=5, C=3, H=3, W=3)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    assert call(C=1, H=3, W=3) == N.GSW_ERR_RAGGED                             # 9 bits
    assert call(C=3, H=5, W=7) == N.GSW_ERR_RAGGED
    assert call(P=1, C=4, H=512, W=257) == N.GSW_ERR_UNSUPPORTED               # n (1 + P) past 1 048 576
    assert call(P=3, C=4, H=256, W=257) == N.GSW_ERR_UNSUPPORTED
    assert call(P=4, C=4, H=256, W=256) == N.GSW_ERR_UNSUPPORTED               # the top of P = 3's domain is past P = 4's
    assert call(C=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1) == N.GSW_ERR_UNSUPPORTED
    assert call(B=65536) == N.GSW_ERR_UNSUPPORTED
    assert call(B=65536, C=1, H=3, W=3) == N.GSW_ERR_UNSUPPORTED               # the order of align_decide: BAD_ARG, UNSUPPORTED, RAGGED


def test_symbol_is_exported_and_prototyped():
    lib = N.lib()
    assert "gsw_level_rows_align" in N.exported_symbols() and hasattr(lib, "gsw_level_rows_align")
    fn = lib.gsw_level_rows_align
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_level_rows_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev" in hdr
    assert lib.gsw_version() == 500                                            # additive
    for name in ("search_keys_soft", "extract_aligned_soft"):
        assert callable(getattr(AL, name))
    assert callable(codec.level_rows_align) and callable(D.detect_latents_aligned_soft)


def test_a_changed_kernel_file_rebuilds_the_library():
    import __graft_entry__ as E
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    assert "gswm_align_soft.inc" in E.HEADERS
    assert "gswm_align_soft.inc" in open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    keyed = open(os.path.join(csrc, "gswm_keyed.hip")).read()
    assert keyed.index('#include "gswm_align.inc"') < keyed.index('#include "gswm_align_soft.inc"')


# ------------------------------------------------------------------------------------------------------------ the front end
def test_cli_flag_and_its_refusals(tmp_path):
    p = D.build_parser()
    base = ["--keyring", "ring.tsv"]
    assert p.parse_args(base).align_reliability == 0                          # the default leaves every current path untouched
    a = p.parse_args(base + ["--align", "d4", "--align_shift", "2", "--align_reliability", "15"])
    assert (a.align, a.align_shift, a.align_reliability, a.reliability) == ("d4", 2, 15, 0)
    for bad in ("16", "-1", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--align", "d4", "--align_reliability", bad])
    ring = tmp_path / "ring.tsv"
    ring.write_text("k\t" + "00" * 32 + "\t" + "00" * 16 + "\n")
    common = ["--keyring", str(ring), "--message_length", "64"]
    for extra in (["--align_reliability", "4"],                                                    # without --align
                  ["--align", "flips", "--align_reliability", "4", "--l", "2"],                    # --l other than 1
                  ["--align", "d4", "--align_reliability", "4", "--reliability", "4"]):            # together with --reliability
        with pytest.raises(SystemExit) as e:
            D.main(common + extra)
        assert e.value.code not in (0, None), extra


def test_the_wrappers_refuse_before_any_launch():
    z = torch.zeros(2, 4, 8, 8, dtype=torch.float16)
    rows = codec.LevelRows(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 2, 32, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32),
                           torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.level_rows_align(rows, (4, 8, 8), [(0, 0, 0)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AL.search_keys_soft(z, torch.zeros(1, 48, dtype=torch.uint8), 8, [(0, 0, 0)])
    with pytest.raises(ValueError, match="shape must be"):
        codec.level_rows_align(rows, (8, 8), [(0, 0, 0)])
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        AL.search_keys_soft(z.view(2, -1), torch.zeros(1, 48, dtype=torch.uint8), 8, [(0, 0, 0)])
    with pytest.raises(ValueError, match="0..7"):
        AL.search_keys_soft(z, torch.zeros(1, 48, dtype=torch.uint8), 8, [(8, 0, 0)])
    with pytest.raises(ValueError, match="empty"):
        AL.search_keys_soft(z, torch.zeros(1, 48, dtype=torch.uint8), 8, [])
    ring = D.Keyring()
    ring.add("k", bytes(32), bytes(16))
    ident = [(0, 0, 0)]
    with pytest.raises(ValueError, match="levels"):
        D.detect_latents_aligned_soft(z, ring, 64, ident, levels=0)
    with pytest.raises(ValueError, match="reliability|levels"):
        D.detect_latents_aligned_soft(z, ring, 64, ident, levels=16)
    with pytest.raises(ValueError, match="k must be"):
        D.detect_latents_aligned_soft(z, ring, 64, ident, k=9)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        D.detect_latents_aligned_soft(z.view(2, -1), ring, 64, ident)
    with pytest.raises(ValueError, match="square"):
        D.detect_latents_aligned_soft(torch.zeros(1, 4, 8, 16).half(), ring, 64, [(1, 0, 0)])
    with pytest.raises(ValueError, match="message_length"):
        D.detect_latents_aligned_soft(z, ring, 60, ident)
    with pytest.raises(ValueError, match="fpr"):
        D.detect_latents_aligned_soft(z, ring, 64, ident, fpr=0.0)
    with pytest.raises(ValueError):
        D.detect_latents_aligned_soft(z, D.Keyring(), 64, ident)                                  # an empty keyring
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.detect_latents_aligned_soft(z, ring, 64, ident)
    with pytest.raises(ValueError):
        AL.extract_aligned_soft(z, bytes(31), bytes(16), 64, ident)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AL.extract_aligned_soft(z, bytes(32), bytes(16), 64, ident)
    # the existing refusals stand
    with pytest.raises(ValueError, match="cannot be combined with align"):
        D.detect_latents(z, ring, 64, align=ident, reliability=4)


def test_merge_best_holds_the_wider_statistic():
    """`_merge_best` packs (stat, key, alignment) into one int64: with 25 bits of statistic the soft search's largest value (15 x 1 048 576) keeps its order
    against `_merge`, and the default field is what `search_keys` always got."""
    g = torch.Generator().manual_seed(7)
    B, A, K = 5, 200, 4096
    stat = torch.randint(0, 15 * 1048576 + 1, (B, A), generator=g, dtype=torch.int32)
    stat[0, 3] = stat[0, 150] = 15 * 1048576                                   # a tie at the top: the lower key, then the lower alignment
    key = torch.randint(0, K, (B, A), generator=g, dtype=torch.int32)
    key[0, 3], key[0, 150] = 9, 9
    stat[1, :] = 77                                                            # all equal: the lowest key leads
    got = AL._merge_best(key, stat, K, AL.SOFT_STAT_BITS)
    want = AL._merge(key, stat, torch.arange(A, dtype=torch.int32).expand(B, A), 1)
    for g_, w_ in zip(got, want):
        assert torch.equal(g_.int(), w_.int())
    assert int(got[1][0, 0]) == 3 and int(got[2][0, 0]) == 15 * 1048576
    assert AL.SOFT_STAT_BITS >= (15 * 1048576).bit_length() + 1
    # the limits: the sign search's field by default, None past 62 bits for either caller
    assert AL._merge_best(key, stat.clamp(max=1048576), 2 ** 31 - 1) is not None                   # 21 + 31 + 8
    assert AL._merge_best(key, stat, 2 ** 31 - 1, AL.SOFT_STAT_BITS) is None                       # 25 + 31 + 8
    assert AL._merge_best(key, stat, 2 ** 29, AL.SOFT_STAT_BITS) is not None                       # 25 + 29 + 8


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restated_rows_are_rows_align_of_every_row():
    """the restatement moves LEVELS on the (C, H, W) lattice; `align_reference.rows_align` moves packed bits: the same bytes"""
    rng = np.random.default_rng(3)
    shape, B, P = (3, 5, 8), 2, 3
    signs = rng.integers(0, 256, (B, 15), dtype=np.uint8)
    planes = rng.integers(0, 256, (B, P, 15), dtype=np.uint8)
    aligns = [(0, 0, 0), (2, 1, -2), (4, 0, 3), (6, -7, 9)]
    s, p = ASR.level_rows_align(signs, planes, shape, aligns)
    assert np.array_equal(s, AR.rows_align(signs, shape, 1, aligns))
    for q in range(P):
        assert np.array_equal(p[:, :, q], AR.rows_align(planes[:, q], shape, 1, aligns))


@pytest.fixture(scope="module")
def E2E():
    E = ASR.E2E
    pairs, msgs, u, noise, blank = ASR.e2e_setup()
    clean = ASR.e2e_host_latents(pairs, msgs, u)
    z16 = ASR.e2e_attack(clean, noise)
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    ks = R.keystreams(pairs, int(np.prod(E["shape"])))
    return dict(pairs=pairs, msgs=msgs, clean=clean, z16=z16, blank=blank, cands=cands, ks=ks, noise=noise)


def test_the_setup_is_the_alignment_experiment_with_more_noise(E2E):
    pairs, msgs, clean, attacked, z1, blank = AR.e2e_setup()
    assert pairs == E2E["pairs"] and msgs == E2E["msgs"] and np.array_equal(clean, E2E["clean"]) and torch.equal(blank, E2E["blank"])
    assert torch.equal(z1, (torch.from_numpy(attacked) + 1.0 * E2E["noise"]).half())
    assert ASR.E2E["sigma"] == 4.0 and ASR.E2E["levels"] == 15 and ASR.E2E["fpr"] == 1e-6 and len(E2E["cands"]) == 200


def test_end_to_end_on_the_restatement(E2E):
    """sigma 4, 15 levels, fpr 1e-6, A = 200, K = 12 on the oracle's latents: both statistics find the key and the alignment of all six images; the soft bound
    names all six with at least 1 decade to spare, the sign bound names exactly two and every image it misses is at least 1 decade above the limit; four
    unwatermarked latents name nothing.  The device's latents differ from these by the embed's rounding, far inside those margins.  (Printed: the bounds.)"""
    E = ASR.E2E
    limit = math.log10(E["fpr"])
    z16, cands, ks = E2E["z16"], E2E["cands"], E2E["ks"]
    thr = soft.uniform_thresholds(z16, E["levels"]).numpy()
    res = ASR.detect_host(z16, thr, cands, ks, E["msg_bytes"], T.log10_p_any)
    sign = AR.detect_host(z16, cands, ks, E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    print(f"15 levels: log10 p_any {[round(float(r[3]), 2) for r in res]}\nsigns:     log10 p_any {[round(float(r[3]), 2) for r in sign]}")
    want_al = [cands.index(AL.inverse(a, 32, 32)) for a in E["attacks"]]
    for r in (res, sign):
        assert [x[0] for x in r] == list(E["rows"]) and [x[1] for x in r] == want_al
    wrong = [sum(bin(x ^ y).count("1") for x, y in zip(r[4], m)) for r, m in zip(res, E2E["msgs"])]
    print(f"wrong message bits of 64 under the soft vote: {wrong}")            # (at sigma 4 a detection is not an error-free read: nothing is asserted on it)
    assert all(x[3] <= limit - 1.0 for x in res)
    named = [x[3] <= limit for x in sign]
    assert sum(named) == 2 and all(x[3] >= limit + 1.0 for x, n in zip(sign, named) if not n)
    bz = E2E["blank"]
    none = ASR.detect_host(bz, soft.uniform_thresholds(bz, E["levels"]).numpy(), cands, ks, E["msg_bytes"], T.log10_p_any)
    none_sign = AR.detect_host(bz, cands, ks, E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    print(f"unwatermarked: 15 levels {[round(float(r[3]), 2) for r in none]}, signs {[round(float(r[3]), 2) for r in none_sign]}")
    assert all(x[3] > limit + 1.0 for x in none) and all(x[3] > limit + 1.0 for x in none_sign)
