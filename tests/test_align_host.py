"""CPU (no GPU): the alignment model of align.py (candidates, `apply` against the NumPy restatement of tests/align_reference.py, the text of an
alignment, the refusals), the merge rule of the search on host tensors, the status codes gsw_rows_align returns before any launch, and the public
surface: what `detect` prints is unchanged unless an alignment was asked for."""
import ctypes
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import key_search_reference as R
from conftest import ROOT


@pytest.fixture(scope="module")
def AL():
    import gswm_amd  # noqa: F401
    from gswm_amd import align
    return align


# ------------------------------------------------------------------------------------------------ the model
def test_alignments_counts_and_order(AL):
    assert AL.alignments("none", 0, 5, 8) == [(0, 0, 0)]
    assert AL.alignments("flips", 0, 5, 8) == [(0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0)]
    assert AL.alignments("d4", 0, 8, 8) == [(d, 0, 0) for d in range(8)]
    assert AL.alignments("none", 1, 5, 8) == [(0, 0, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, 1, 1), (0, 1, -1), (0, -1, 0), (0, -1, 1), (0, -1, -1)]
    for group, n in (("none", 1), ("flips", 4), ("d4", 8)):
        for shift in (0, 1, 2, 4):
            c = AL.alignments(group, shift, 32, 32)
            assert len(c) == n * (2 * shift + 1) ** 2 == len(set(c)) and c[0] == (0, 0, 0)
            assert [a[0] for a in c] == sorted(a[0] for a in c)                       # d ascending, a block per d
            assert {(dy, dx) for _, dy, dx in c} == {(dy, dx) for dy in range(-shift, shift + 1) for dx in range(-shift, shift + 1)}
    assert len(AL.alignments("d4", 2, 32, 32)) == 200 and len(AL.alignments("d4", 4, 64, 64)) == 648
    # no two candidates are the same permutation of the lattice
    idx = torch.arange(49).view(7, 7)
    c = AL.alignments("d4", 3, 7, 7)
    assert len({tuple(AL.apply(idx, a).reshape(-1).tolist()) for a in c}) == len(c) == 392


def test_apply_is_the_restatement(AL):
    rng = np.random.default_rng(1)
    for shape in ((3, 5, 8), (2, 4, 6, 6), (7, 7)):
        z = rng.standard_normal(shape).astype(np.float32)
        for d in range(8):
            if d & 1 and shape[-1] != shape[-2]:
                continue
            for dy, dx in ((0, 0), (1, -2), (-3, shape[-1] + 1), (shape[-2], 0)):
                got = AL.apply(torch.from_numpy(z), (d, dy, dx)).numpy()
                assert np.array_equal(got, AR.apply_np(z, (d, dy, dx))), (shape, d, dy, dx)


def test_the_eight_orientations_are_distinct_and_every_alignment_has_an_inverse(AL):
    z = torch.arange(9).view(3, 3)
    assert len({tuple(AL.apply(z, (d, 0, 0)).reshape(-1).tolist()) for d in range(8)}) == 8
    assert AL.apply(z, (4, 0, 0)).tolist() == [[2, 1, 0], [5, 4, 3], [8, 7, 6]]                # d & 4: the last axis is mirrored
    assert AL.apply(z, (1, 0, 0)).tolist() == [[2, 5, 8], [1, 4, 7], [0, 3, 6]]                # a quarter turn counterclockwise
    assert AL.apply(z, (0, 1, 0)).tolist() == [[6, 7, 8], [0, 1, 2], [3, 4, 5]]                # rows move down, cyclically
    lat = torch.randn(4, 32, 32, generator=torch.Generator().manual_seed(2))
    cands = AL.alignments("d4", 2, 32, 32)
    for a in [(0, 0, 0), (4, 0, 0), (1, 0, 0), (2, 1, -2), (7, -2, 2), (5, 2, 1), (3, -1, 2), (6, 2, 2)]:
        found = AL.inverse(a, 32, 32)
        assert found in cands                                                                # the candidates are closed under inversion
        assert torch.equal(AL.apply(AL.apply(lat, a), found), lat)
    wide = torch.randn(2, 5, 8, generator=torch.Generator().manual_seed(3))
    for a in AL.alignments("flips", 2, 5, 8):
        assert torch.equal(AL.apply(AL.apply(wide, a), AL.inverse(a, 5, 8)), wide)
    assert AL.inverse((0, 3, 0), 6, 6) == (0, 3, 0) and AL.inverse((0, 4, 0), 6, 6) == (0, 2, 0)   # shifts come back in (-H/2, H/2]


def test_describe(AL):
    want = {(0, 0, 0): "identity", (5, 1, -2): "hflip+rot90 shift (1,-2)", (4, 0, 0): "hflip", (1, 0, 0): "rot90", (2, 0, 0): "rot180", (3, 0, 0): "rot270",
            (6, 0, 0): "hflip+rot180", (7, -2, 2): "hflip+rot270 shift (-2,2)", (0, 0, 3): "shift (0,3)"}
    for a, text in want.items():
        assert AL.describe(a) == text
    assert len({AL.describe(a) for a in AL.alignments("d4", 2, 32, 32)}) == 200


def test_refusals(AL):
    z = torch.zeros(2, 5, 8)
    for d in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="square"):
            AL.apply(z, (d, 0, 0))
    for bad in ((8, 0, 0), (-1, 0, 0), (0, 0), (0.0, 0, 0), (True, 0, 0), "abc", None):
        with pytest.raises(ValueError):
            AL.apply(torch.zeros(4, 4), bad)
        with pytest.raises(ValueError):
            AL.describe(bad)
    with pytest.raises(ValueError, match="square"):
        AL.alignments("d4", 0, 5, 8)
    for shift, H, W in ((3, 6, 8), (4, 8, 8), (1, 2, 9), (-1, 8, 8)):
        with pytest.raises(ValueError, match="shift"):
            AL.alignments("flips", shift, H, W)
    assert len(AL.alignments("flips", 3, 7, 8)) == 4 * 49
    with pytest.raises(ValueError, match="group"):
        AL.alignments("rot", 0, 8, 8)
    from gswm_amd import codec
    for bad, shape in (([(8, 0, 0)], (1, 8, 8)), ([(1, 0, 0)], (1, 5, 8)), ([], (1, 8, 8)), ([(0, 0)], (1, 8, 8)), ([(0, 0, 2 ** 31)], (1, 8, 8)),
                       (torch.zeros(2, 3, dtype=torch.int64), (1, 8, 8)), ([(0, 0, 0)], (1, 0, 8))):
        with pytest.raises(ValueError):
            codec.align_table(bad, shape)
    assert codec.align_table([(7, -1, 9)], (2, 8, 8)).tolist() == [[7, -1, 9]] and codec.align_table([(6, 0, 0)], (2, 5, 8)).dtype == np.int32
    # the wrappers refuse host tensors before anything else happens
    with pytest.raises(ValueError, match="HIP device"):
        codec.rows_align(torch.zeros(1, 8, dtype=torch.uint8), (1, 8, 8), 1, [(0, 0, 0)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AL.search_keys(torch.zeros(1, 1, 8, 8), torch.zeros(1, 48, dtype=torch.uint8), 1, [(0, 0, 0)])


# ------------------------------------------------------------------------------------------------ the merge, on host tensors
@pytest.mark.parametrize("K,k", [(9, 1), (9, 3), (2, 3), (1, 8), (9, 8)])
def test_merge_rule(AL, K, k):
    """per-row top-k lists (what the key search returns for every aligned row) -> the per-image answer of the restatement; few distinct values: many ties"""
    rng = np.random.default_rng(10 * K + k)
    B, A = 5, 20
    S = rng.integers(0, 6, (B, A, K))
    idx, st = R.topk(S.reshape(B * A, K), k)
    al = torch.arange(A, dtype=torch.int32).repeat_interleave(k).expand(B, A * k)
    got = AL._merge(torch.from_numpy(idx).view(B, A * k), torch.from_numpy(st).view(B, A * k), al, k)
    for g, w, name in zip(got, AR.merge(S, k), ("key", "align", "stat")):
        assert g.dtype == torch.int32 and np.array_equal(g.numpy(), w), (name, g, w)
    # the order of the candidates does not matter: shuffled columns, the same answer
    perm = torch.from_numpy(rng.permutation(A * k))
    again = AL._merge(torch.from_numpy(idx).view(B, A * k)[:, perm], torch.from_numpy(st).view(B, A * k)[:, perm], al[:, perm], k)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("K", [1, 2, 9, 100000])
def test_merge_of_single_best_entries(AL, K):
    """k = 1 takes one maximum instead of the sorts: the same answer, and None when key x alignment x statistic do not fit one int64"""
    rng = np.random.default_rng(K)
    B, A = 5, 40
    S = rng.integers(0, 4, (B, A, min(K, 9)))
    idx, st = R.topk(S.reshape(B * A, -1), 1)
    key, stat = torch.from_numpy(idx).view(B, A), torch.from_numpy(st).view(B, A)
    got = AL._merge_best(key, stat, K)
    al = torch.arange(A, dtype=torch.int32).expand(B, A)
    for g, s, w in zip(got, AL._merge(key, stat, al, 1), AR.merge(S, 1)):
        assert g.dtype == torch.int32 and tuple(g.shape) == (B, 1) and torch.equal(g, s) and np.array_equal(g.numpy(), w)
    wide = torch.zeros(1, 65535, dtype=torch.int32)
    assert AL._merge_best(wide, wide, 2 ** 31 - 1) is None and AL._merge_best(wide, wide, 2 ** 24) is not None


def test_restatement_of_rows_align_on_a_pattern():
    """the restatement itself, on rows whose answer is known by hand: 2 x 2 lattice, l = 2, elements 0 1 / 2 3"""
    rows = np.array([[0b00011011]], dtype=np.uint8)
    out = AR.rows_align(rows, (1, 2, 2), 2, [(0, 0, 0), (4, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0)])
    assert [int(x) for x in out[0, :, 0]] == [0b00011011, 0b01001110, 0b01110010, 0b10110001, 0b11100100]


# ------------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_c_entry_point_refuses_before_any_launch():
    from gswm_amd import _native as N
    lib = N.lib()
    p, odd = ctypes.c_void_p(64), ctypes.c_void_p(66)                          # never dereferenced: every call below is refused before a launch

    def call(rows=p, B=1, C=4, H=8, W=8, l=1, al=p, A=1, out=p):
        return lib.gsw_rows_align(rows, B, C, H, W, l, al, A, out, None)

    for kw in (dict(rows=None), dict(al=None), dict(out=None), dict(al=odd), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(A=0), dict(A=-2),
               dict(l=0), dict(l=3), dict(l=8), dict(l=3, C=3, H=3, W=3)):
        assert call(**kw) == N.GSW_ERR_BAD_ARG, kw
    for kw in (dict(C=1, H=3, W=3), dict(C=3, H=5, W=5, l=2), dict(C=1, H=1, W=1, l=4)):
        assert call(**kw) == N.GSW_ERR_RAGGED, kw
    for kw in (dict(C=4, H=512, W=513), dict(C=4, H=512, W=512, l=2), dict(C=2 ** 30, H=2 ** 30, W=2 ** 30), dict(B=65536)):
        assert call(**kw) == N.GSW_ERR_UNSUPPORTED, kw


def test_symbol_is_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    assert "gsw_rows_align" in N.exported_symbols() and hasattr(lib, "gsw_rows_align")
    fn = lib.gsw_rows_align
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert "int gsw_rows_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev" in hdr
    import gswm_amd
    assert "align" in gswm_amd.__all__ and gswm_amd.align.GROUPS["flips"] == (0, 2, 4, 6)


def test_build_lists_name_the_new_include():
    """a changed gswm_align.inc rebuilds the library: it is a prerequisite in both build descriptions and is included by the keyed translation unit"""
    import __graft_entry__ as E
    assert "gswm_align.inc" in E.HEADERS
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    assert "gswm_align.inc" in open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert '#include "gswm_align.inc"' in open(os.path.join(csrc, "gswm_keyed.hip")).read()
    assert set(E.HEADERS) >= {f for f in os.listdir(csrc) if f.endswith((".inc", ".h"))}


# ------------------------------------------------------------------------------------------------ the public surface
def test_detect_lines_are_unchanged_without_align():
    from gswm_amd import detect as D
    c = [D.KeyCandidate("k7", 7, 9000, -120.5), D.KeyCandidate("k2", 2, 2100, 0.0)]
    assert c[0].alignment is None and D.DetectResult().alignment is None
    assert D.format_line("a.png", D.DetectResult(c, "k7", b"\x01\xff", 0)) == "a.png, key: k7, log10 p, -120.500, message: 01ff, next: k2 (0.000)"
    assert D.format_line("a.png", D.DetectResult(c[1:], None, None, 2)) == "a.png, key: none, log10 p, 0.000, message: none, flags 2"
    a = [D.KeyCandidate("k7", 7, 9000, -120.5, (5, 1, -2)), D.KeyCandidate("k2", 2, 2100, 0.0, (0, 0, 0))]
    assert D.format_line("a.png", D.DetectResult(a, "k7", b"\x01\xff", 0, (5, 1, -2))) == \
        "a.png, key: k7, log10 p, -120.500, message: 01ff, next: k2 (0.000), alignment: hflip+rot90 shift (1,-2)"
    assert D.format_line("a.png", D.DetectResult(a[1:], None, None, 0)).endswith(", message: none, alignment: identity")
    args = D.build_parser().parse_args(["--keyring", "x"])
    assert args.align == "none" and args.align_shift == 0
    args = D.build_parser().parse_args(["--keyring", "x", "--align", "d4", "--align_shift", "2"])
    assert (args.align, args.align_shift) == ("d4", 2)
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--keyring", "x", "--align", "rot"])


def test_extract_parser(capsys):
    from gswm_amd import extract as X
    base = ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16, "--original_message_hex", "ab"]
    a = X.build_parser().parse_args(base)
    assert a.align == "none" and a.align_shift == 0 and not X._align_wanted(a)
    a = X.build_parser().parse_args(base + ["--align", "flips", "--align_shift", "1"])
    assert X._align_wanted(a) and X._alignment_note("0101") == ""
    for extra in (["--align", "d4", "--soft", "1"], ["--align", "d4", "--robust", "1"], ["--align", "d4", "--tamper_map", "d"], ["--align_shift", "1"],
                  ["--align", "d4", "--align_shift", "-1"]):
        with pytest.raises(SystemExit):
            X.build_parser().parse_args(base + extra)
        assert "--align" in capsys.readouterr().err
    s = X._AlignedBits("0101")
    s.alignment, s.log10_p = (4, 0, 1), -12.25
    assert s == "0101" and X._alignment_note(s) == ", alignment: hflip shift (0,1), log10 p, -12.250"
