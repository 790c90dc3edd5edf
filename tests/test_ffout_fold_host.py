"""CPU (no GPU): the fold of a Transformer2DModel's last ff.net[2] into proj_out (unet.fold_ff_out / FOLD_FF_OUT) is algebra --
    x_pf + proj_out(x + net[2](h)) = x_pf + [h | x] [Wp W2 | Wp]^T + (Wp b2 + bp)
-- so in fp64 the two sides differ by round-off only; the folded operands are cached on the module by the four parameters; the switch is part of what
captured graphs are keyed by."""
import torch

import gswm_amd  # noqa: F401
from gswm_amd import graph, unet as U


def _transformer(dtype=torch.float64, seed=0):
    tr = U.synthetic_init_(U.Transformer2DModel(320, 1024, 5, 64), seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():           # synthetic_init_ leaves every bias at zero: the bias term of the fold would go unchecked
        tr.transformer_blocks[-1].ff.net[2].bias.copy_(0.3 * torch.randn(320, generator=g))
        tr.proj_out.bias.copy_(0.3 * torch.randn(320, generator=g))
    return tr.to(dtype).eval()


def test_fold_is_the_two_linear_maps_in_fp64():
    tr = _transformer()
    l2, po = tr.transformer_blocks[-1].ff.net[2], tr.proj_out
    g = torch.Generator().manual_seed(7)
    M = 96
    h = torch.randn(M, 1280, generator=g, dtype=torch.float64) * 1.5
    x = torch.randn(M, 320, generator=g, dtype=torch.float64) * 1.3 + 0.4
    x_pf = torch.randn(M, 320, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = x_pf + po(x + l2(h))
        w_cat, b = U.fold_ff_out(l2.weight, l2.bias, po.weight, po.bias)
        assert w_cat.shape == (320, 1600) and b.shape == (320,) and w_cat.dtype == torch.float64
        got = x_pf + torch.cat([h, x], dim=1) @ w_cat.T + b
    rel = (got - want).abs().max().item() / want.abs().max().item()
    print(f"fold vs two linear maps, fp64: max relative difference {rel:.3e}")
    assert rel <= 1e-10


def test_fold_rounds_once_to_the_model_dtype():
    tr = _transformer(torch.float16)
    l2, po = tr.transformer_blocks[-1].ff.net[2], tr.proj_out
    w_cat, b = U.fold_ff_out(l2.weight, l2.bias, po.weight, po.bias)
    assert w_cat.dtype == torch.float16 and b.dtype == torch.float16 and w_cat.is_contiguous()
    exact = po.weight.double() @ l2.weight.double()
    # the fp32 product (a K = 320 dot product: at most K 2^-24 sum |a||b|, the standard bound) and then ONE rounding to fp16: half an ulp, 2^-11 relative for
    # normal numbers, 2^-25 absolute in the subnormal range
    fp32_err = 320 * 2.0 ** -24 * (po.weight.double().abs() @ l2.weight.double().abs())
    assert ((w_cat[:, :1280].double() - exact).abs() <= exact.abs() * 2.0 ** -11 + 2.0 ** -25 + fp32_err).all()
    assert torch.equal(w_cat[:, 1280:], po.weight)


def test_cache_follows_the_four_parameters():
    tr = _transformer(torch.float32)
    l2, po = tr.transformer_blocks[-1].ff.net[2], tr.proj_out
    first = tr._ff_out_folded()
    assert tr._ff_out_folded()[0] is first[0]                    # unchanged parameters: the cached operands
    for p in (l2.weight, l2.bias, po.weight, po.bias):
        before = tr._ff_out_folded()
        with torch.no_grad():
            p.mul_(1.5)
        after = tr._ff_out_folded()
        assert after[0] is not before[0]
        w_cat, b = U.fold_ff_out(l2.weight, l2.bias, po.weight, po.bias)
        assert torch.equal(after[0], w_cat) and torch.equal(after[1], b)


def test_switch_is_part_of_the_graph_key(monkeypatch):
    on = graph._switches()
    monkeypatch.setattr(U, "FOLD_FF_OUT", not U.FOLD_FF_OUT)
    off = graph._switches()
    assert on != off
    monkeypatch.undo()
    assert graph._switches() == on
    from gswm_amd import xattn
    for name in ("ENABLED", "PRE_ENABLED", "GNPROJ_ENABLED"):    # the three one-launch switches of xattn.py decide launches too
        monkeypatch.setattr(xattn, name, not getattr(xattn, name))
        assert graph._switches() != on
        monkeypatch.undo()


def test_fold_needs_the_engine_path():
    """CPU tokens never take the fold (no engine there), whatever the switch says"""
    tr = _transformer(torch.float32)
    assert U.FOLD_FF_OUT
    assert not tr._ff_out_fold_ok(torch.zeros(2, 256, 320), False)


def test_gemm2_argument_validation_needs_no_gpu():
    """status codes of gsw_gemm2_ex that are decided before any HIP call"""
    import ctypes
    from gswm_amd import _native as N
    lib, p = N.lib(), ctypes.c_void_p(4096)
    BAD, UNS = N.GSW_ERR_BAD_ARG, N.GSW_ERR_UNSUPPORTED

    def call(x1=p, ld0=1280, K0=1280, ld1=320, K1=320, ldw=1600, mode=0, S=0, Wimg=0, M=128, N_=320):
        return lib.gsw_gemm2_ex(p, ld0, K0, x1, ld1, K1, p, ldw, None, None, N_, p, N_, M, N_, mode, S, Wimg, N.GSW_F16, None, None)
    assert call(x1=None) == BAD                        # one block: that is gsw_gemm_ex
    assert call(K1=0) == BAD and call(M=0) == BAD and call(mode=7) == BAD
    assert call(K1=288) == UNS and call(K0=1248) == UNS          # K_i % 64
    assert call(ld1=312) == UNS and call(ld0=1272) == UNS        # ld_i < K_i
    assert call(ld1=324) == UNS                        # ld_i % 8
    assert call(ldw=1280) == UNS                       # the weight rows hold K0 + K1 columns
    assert call(mode=1, N_=320) == UNS and call(mode=2, S=64) == UNS      # GEGLU / TRANS: not with two blocks
    assert call(mode=3, S=0, Wimg=8) == BAD and call(mode=3, S=60, Wimg=8) == BAD
