"""GPU: gsw_gemm2_ex -- a dense GEMM whose A operand lies in two column blocks [x0 | x1] with their own row strides, walked as two K segments -- against
gsw_gemm_ex on the materialised torch.cat([x0, x1], 1) with the same weight, mode and forced tiling.  Same kernel, same stage order: the results must be
BIT-identical, on every tile height (gsw_mm_config 128 / 256 / 512 = the 256 x 320 tile wherever legal), both wave layouts (split mask 0 / 15) and both
dtypes; a wrong segment switch (row stride, weight column offset, the boundary stage) cannot hide behind a tolerance.  Outputs live in the poisoned,
guard-banded buffers of tests/poison.py: PF border rows and guard rows must keep the pattern, nothing may land outside a buffer.  Shapes are the smallest at
which the walk can go wrong: one partial row tile (M = 192), several (576), a partial 160-column tile (N = 328), strided operands (ld > K)."""
import ctypes as C

import pytest
import torch

import poison

pytestmark = pytest.mark.gpu

PLAIN, GEGLU, TOK2PF = 0, 1, 3
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}          # one rounding of the storage dtype at the output magnitude (tests/test_gpu_mm_production.py)


@pytest.fixture(scope="module")
def G():
    import types
    import gswm_amd  # noqa: F401
    from gswm_amd import pf, codec, _native
    lib = _native.lib()
    yield types.SimpleNamespace(pf=pf, codec=codec, N=_native, lib=lib)
    assert lib.gsw_mm_config(0, 10) == 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _extras(G, dev, colstats=None, max_splits=0):
    ex = G.pf._extras(dev, colstats=colstats)
    ex.max_splits = max_splits
    return ex


def _gemm2(G, x0, x1, w, b, resid, y, M, N, mode, S, Wimg, ex):
    return G.lib.gsw_gemm2_ex(x0.data_ptr(), x0.stride(0), x0.shape[1], x1.data_ptr(), x1.stride(0), x1.shape[1], w.data_ptr(), w.stride(0),
                              b.data_ptr() if b is not None else None, resid.data_ptr() if resid is not None else None, N, y.data_ptr(), N, M, N, mode, S, Wimg,
                              G.codec._dt(x0.dtype), C.byref(ex) if ex is not None else None, G.codec._stream_ptr())


def _gemm1(G, x, w, b, resid, y, M, N, mode, S, Wimg, ex):
    return G.lib.gsw_gemm_ex(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), b.data_ptr() if b is not None else None,
                             resid.data_ptr() if resid is not None else None, N, y.data_ptr(), N, M, x.shape[1], N, mode, S, Wimg,
                             G.codec._dt(x.dtype), C.byref(ex) if ex is not None else None, G.codec._stream_ptr())


class Case:
    """operands of one shape, built once: tokens of B images of 8 x 8 pixels; h-like block x0 [M, K0], stream-like block x1 [M, K1], W [N, K0 + K1]"""

    def __init__(self, L, C_, B, N, dtype, pad0=0, pad1=0):
        self.H = self.W = 8
        self.B, self.N, self.K0, self.K1, self.M = B, N, 4 * C_, C_, B * 64
        g = torch.Generator().manual_seed(C_ + 7 * B + N)
        K = self.K0 + self.K1
        a0 = L.wrap(torch.randn(self.M, self.K0 + pad0, generator=g).to(dtype).cuda())
        a1 = L.wrap((torch.randn(self.M, self.K1 + pad1, generator=g) * 1.3 + 0.4).to(dtype).cuda())
        self.x0, self.x1 = a0[:, :self.K0], a1[:, :self.K1]                 # ld_i = K_i + pad_i
        self.cat = L.wrap(torch.cat([self.x0, self.x1], dim=1))
        self.w = L.wrap((torch.randn(N, K, generator=g) * K ** -0.5).to(dtype).cuda())
        self.b = L.wrap(torch.randn(N, generator=g).to(dtype).cuda())
        self.r = L.wrap(torch.randn(self.M, N, generator=g).to(dtype).cuda())
        self.ref = self.cat.float() @ self.w.float().T + self.b.float() + self.r.float()      # the shared fp32 reference

    def pf_tensor(self, G, L):
        """a PF tensor [B, 8, 8, N] in a ledger buffer: interior = the residual, border and guard rows = the pattern"""
        G_, rows = self.W + 3, self.B * (self.H + 2) * (self.W + 2)
        X = G.pf.PF(L.empty((rows + 2 * G_, self.N), self.r.dtype, "cuda"), self.B, self.H, self.W, self.N)
        X.interior.copy_(self.r.view(self.B, self.H, self.W, self.N))
        return X


def _outside_interior(X):
    gr = X.grid
    return [X.buf[: X.G], X.buf[X.G + X.M:], gr[:, 0], gr[:, -1], gr[:, 1:-1, 0], gr[:, 1:-1, -1]]


SHAPES = [
    # C, B, N, pad0, pad1
    (320, 3, 320, 0, 0),        # M = 192: one partial row tile, clamped tail rows
    (320, 9, 320, 0, 0),        # M = 576: several row tiles on every tile height, a partial last one
    (640, 4, 640, 0, 0),        # M = 256: K0 = 2560, K1 = 640; the shape on which a forced wide tile is legal for dense rows
    (320, 3, 328, 0, 0),        # a partial 160-column tile (weight rows clamped, stores masked); the wide tile is not legal: runs narrow
    (320, 3, 320, 64, 8),       # strided views: ld0 = K0 + 64, ld1 = K1 + 8 (different row strides per segment)
]


def _compare(G, L, c, dtype, what, max_splits, wide_forced):
    """one dense-row (+ residual) and one in-place token-scatter launch of each form, same extras -> (splits of the four launches)"""
    M, N, S, Wimg = c.M, c.N, 64, 8
    exs = [_extras(G, "cuda", max_splits=max_splits) for _ in range(4)]
    # ---- dense rows (+ residual)
    y1, y2 = L.empty((M, N), dtype, "cuda"), L.empty((M, N), dtype, "cuda")
    assert _gemm1(G, c.cat, c.w, c.b, c.r, y1, M, N, PLAIN, 0, 0, exs[0]) == 0
    rc = _gemm2(G, c.x0, c.x1, c.w, c.b, c.r, y2, M, N, PLAIN, 0, 0, exs[1])
    if wide_forced and M % 256 == 0 and N % 320 == 0:
        # the wide dense-row producer addresses one dense operand: forcing it on an unsplit two-block launch is refused, nothing is launched
        assert exs[0].splits == 1, what
        assert rc == G.N.GSW_ERR_UNSUPPORTED, what
        torch.cuda.synchronize()
        assert L.untouched(y2) == y2.numel(), what
        exs[1].splits = 1
    else:
        assert rc == 0, what
        assert L.untouched(y2) == 0, what + ": " + L.where(y2)
        assert torch.equal(_bits(y1), _bits(y2)), what + ": plain"
        err = (y2.float() - c.ref).abs().max().item() / c.ref.abs().max().item()
        assert err <= 2 * TOL[dtype], (what, err)
    # ---- token scatter into a PF tensor, in place (resid == out)
    X1, X2 = c.pf_tensor(G, L), c.pf_tensor(G, L)
    assert _gemm1(G, c.cat, c.w, c.b, X1.rows, X1.rows, M, N, TOK2PF, S, Wimg, exs[2]) == 0
    assert _gemm2(G, c.x0, c.x1, c.w, c.b, X2.rows, X2.rows, M, N, TOK2PF, S, Wimg, exs[3]) == 0, what
    assert torch.equal(_bits(X1.interior), _bits(X2.interior)), what + ": tok2pf"
    err = (X2.interior.reshape(M, N).float() - c.ref).abs().max().item() / c.ref.abs().max().item()
    assert err <= 2 * TOL[dtype], (what, err)
    for v in _outside_interior(X2):          # border and guard rows are not this launch's business
        assert L.untouched(v) == v.numel(), what + ": " + L.where(v, untouched=False)
    L.check()
    return [e.splits for e in exs]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("C_,B,N,pad0,pad1", SHAPES)
def test_two_segments_equal_the_concatenated_operand_bit_for_bit(G, C_, B, N, pad0, pad1, dtype):
    """Every forced tiling UNSPLIT (max_splits = 1: with a workspace the plan would split these small launches along K, and a split launch runs the split
    kernels whatever the tile knobs say) -- the 8-wave, the 12-wave and the wide producers each walk the two segments; then the automatic plan and a forced
    four-way split, whose workgroups enter the stage sequence on either side of the segment boundary."""
    L = poison.Ledger(poison.NAN)
    c = Case(L, C_, B, N, dtype, pad0, pad1)
    try:
        for tile_rows in (128, 256, 512):
            for split_mask in (0, 15):
                assert G.lib.gsw_mm_config(tile_rows, split_mask) == 0
                sp = _compare(G, L, c, dtype, f"tile_rows={tile_rows} split_mask={split_mask} unsplit", 1, tile_rows == 512)
                assert sp == [1, 1, 1, 1], sp
        assert G.lib.gsw_mm_config(0, 10) == 0
        sp = _compare(G, L, c, dtype, "automatic plan", 0, False)
        assert sp[0] == sp[1] and sp[2] == sp[3], sp            # the plan does not depend on how the operand is laid out
        sp = _compare(G, L, c, dtype, "four-way split", 4, False)
        assert min(sp) > 1 and sp[0] == sp[1] and sp[2] == sp[3], sp
    finally:
        assert G.lib.gsw_mm_config(0, 10) == 0


@pytest.mark.parametrize("tile_rows", [128, 256, 512])
def test_tok2pf_column_records_equal_the_single_segment_launch(G, tile_rows):
    """GroupNorm's column records (GswMmExtras.colstats_*) of the two-block launch: same geometry, same floats"""
    L = poison.Ledger(poison.FINITE)
    dtype = torch.float16
    c = Case(L, 320, 9, 320, dtype)
    M, N = c.M, c.N
    cap = (M + 127) // 128 * 4 * N
    try:
        assert G.lib.gsw_mm_config(tile_rows, -1) == 0
        outs = []
        for two in (False, True):
            X = c.pf_tensor(G, L)
            cs = torch.zeros(cap, dtype=torch.float32, device="cuda")
            ex = _extras(G, "cuda", colstats=cs, max_splits=1)          # unsplit: a split launch writes no records
            if two:
                assert _gemm2(G, c.x0, c.x1, c.w, c.b, X.rows, X.rows, M, N, TOK2PF, 64, 8, ex) == 0
            else:
                assert _gemm1(G, c.cat, c.w, c.b, X.rows, X.rows, M, N, TOK2PF, 64, 8, ex) == 0
            outs.append((X, cs, ex.colstats_rows_per_block, ex.colstats_blocks))
        (Xa, csa, rpa, bla), (Xb, csb, rpb, blb) = outs
        assert rpa > 0 and bla > 0 and (rpa, bla) == (rpb, blb)
        assert torch.equal(csa, csb)
        assert torch.equal(_bits(Xa.interior), _bits(Xb.interior))
        # ... and they are the statistics of what was stored: sums over all blocks against the tensor itself
        s = csb[: blb * N].view(blb, 2, N // 2).sum(0)
        v = Xb.interior.reshape(M, N // 2, 2).float()
        assert torch.allclose(s[0], v.sum((0, 2)), rtol=1e-3, atol=1e-2) and torch.allclose(s[1], (v * v).sum((0, 2)), rtol=1e-3, atol=1e-2)
        L.check()
    finally:
        assert G.lib.gsw_mm_config(0, 10) == 0


def test_pf_gemm2_wrapper(G):
    """pf.gemm2 (contiguous operands) is that launch: equal to pf.gemm on the concatenation, records handed to stats_for"""
    L = poison.Ledger(poison.NAN)
    c = Case(L, 320, 9, 320, torch.float16)
    old = G.pf.SMALL_GEMM_MAX_ROWS
    G.pf.SMALL_GEMM_MAX_ROWS = 0
    try:
        X1, X2 = c.pf_tensor(G, L), c.pf_tensor(G, L)
        G.pf.gemm(c.cat, c.w, c.b, resid=X1.rows, mode="tok2pf", tokens=64, width=8, out=X1.rows, stats_for=X1)
        G.pf.gemm2(c.x0, c.x1, c.w, c.b, resid=X2.rows, mode="tok2pf", tokens=64, width=8, out=X2.rows, stats_for=X2)
        assert torch.equal(_bits(X1.interior), _bits(X2.interior))
        assert (X1.stats is None) == (X2.stats is None)
        if X1.stats is not None:
            assert (X1.stats.rows, X1.stats.blocks) == (X2.stats.rows, X2.stats.blocks)
        for splitk_max in (0, 1):          # the automatic plan (splits this small launch), and unsplit
            G.pf.SPLITK_MAX = splitk_max
            y1 = G.pf.gemm(c.cat, c.w, c.b, resid=c.r)
            y2 = G.pf.gemm2(c.x0, c.x1, c.w, c.b, resid=c.r, mode="plain")
            assert torch.equal(_bits(y1), _bits(y2))
            assert (y2.float() - c.ref).abs().max().item() <= 2 * TOL[torch.float16] * c.ref.abs().max().item()
        with pytest.raises(ValueError):
            G.pf.gemm2(c.x0, c.x1, c.w, c.b, mode="geglu")
    finally:
        G.pf.SMALL_GEMM_MAX_ROWS = old
        G.pf.SPLITK_MAX = 0


def test_bad_arguments_return_the_documented_codes(G):
    L = poison.Ledger(poison.NAN)
    dtype = torch.float16
    c = Case(L, 320, 4, 320, dtype)          # M = 256, N = 320: a forced wide tile would be legal for dense rows
    M, N = c.M, c.N
    UNS, BAD = G.N.GSW_ERR_UNSUPPORTED, G.N.GSW_ERR_BAD_ARG
    y = L.empty((M, N), dtype, "cuda")
    X = c.pf_tensor(G, L)

    def call(x0=c.x0, x1=c.x1, mode=PLAIN, out=y, resid=None, S=0, Wimg=0, k1=None, ld1=None):
        return G.lib.gsw_gemm2_ex(x0.data_ptr(), x0.stride(0), x0.shape[1], x1.data_ptr() if x1 is not None else None, x1.stride(0) if ld1 is None else ld1,
                                  x1.shape[1] if k1 is None else k1, c.w.data_ptr(), c.w.stride(0), c.b.data_ptr(), resid, N, out.data_ptr(), N, M, N, mode, S, Wimg,
                                  G.codec._dt(dtype), None, G.codec._stream_ptr())
    try:
        assert call(k1=c.K1 - 32) == UNS                              # K1 % 64
        assert call(k1=0) == BAD
        assert call(ld1=c.K1 - 8) == UNS                              # ld1 < K1
        assert call(ld1=c.K1 + 4) == UNS                              # ld1 % 8
        assert G.lib.gsw_gemm2_ex(c.x0.data_ptr(), c.K0, c.K0, None, c.K1, c.K1, c.w.data_ptr(), c.w.stride(0), None, None, N, y.data_ptr(), N, M, N, PLAIN, 0, 0,
                                  G.codec._dt(dtype), None, None) == BAD          # no second block: that is gsw_gemm_ex
        assert call(mode=GEGLU) == UNS and call(mode=2, S=64) == UNS      # two blocks: dense rows and the token scatter only
        assert call(mode=TOK2PF, out=X.rows, S=0, Wimg=8) == BAD
        assert G.lib.gsw_mm_config(512, -1) == 0
        assert call() == UNS                                          # dense rows + two blocks + forced wide tile
        assert call(mode=TOK2PF, out=X.rows, resid=X.rows.data_ptr(), S=64, Wimg=8) == 0       # the PF-row epilogue serves it
        assert G.lib.gsw_mm_config(256, -1) == 0
        assert call() == 0
        torch.cuda.synchronize()
        assert L.untouched(y) == 0
        want = c.ref - c.r.float()                                    # (this call passes no residual)
        assert (y.float() - want).abs().max().item() <= TOL[dtype] * want.abs().max().item()
        L.check()
    finally:
        assert G.lib.gsw_mm_config(0, 10) == 0
