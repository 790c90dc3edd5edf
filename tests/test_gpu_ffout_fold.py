"""GPU: the last block's ff.net[2] folded into proj_out (unet.FOLD_FF_OUT: one two-segment launch, pf.gemm2) against the two launches it replaces and the
fp32 torch modules.  Bounds are the project's own (tests/test_gpu_xattn.py): a transformer within 1e-2 x max(1, |ref|max) of fp32 torch either way and of the
other form; whole-UNet A/B within 2e-2 x max(1, |off|max).  The folded weight is a product rounded once to the model dtype, so both dtypes are held to it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


# (channels, heads, latent side, images): at 640 / 8 x 8 with two images the transformer has 128 token rows, which is the small-batch kernel's range, so the
# fold must NOT apply there; 320 / 16 x 16 and 640 / 16 x 16 are the two narrower levels on the engine
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("C,heads,hw,B,folds", [(320, 5, 16, 2, True), (640, 10, 8, 2, False), (640, 10, 16, 2, True)])
def test_one_transformer_fold_on_and_off_vs_fp32(C, heads, hw, B, folds, dtype):
    from gswm_amd import unet as U, pf
    torch.manual_seed(C + hw)
    tr = U.synthetic_init_(U.Transformer2DModel(C, 1024, heads, 64), 1)
    with torch.no_grad():          # synthetic_init_ leaves the biases at zero: the bias term of the fold would go unchecked
        for n_, p_ in tr.named_parameters():
            if n_.endswith("bias") and "norm" not in n_:
                p_.normal_(std=0.2)
    tr = tr.cuda().to(dtype).eval()
    x = (torch.randn(B, C, hw, hw, device="cuda") * 1.2).to(dtype)
    ctx = torch.randn(B, 77, 1024, device="cuda").to(dtype)
    launches = {}
    outs = {}
    old = U.FOLD_FF_OUT
    try:
        with torch.no_grad():
            tr.forward_pf(pf.PF.from_nchw(x), ctx)          # what is computed once per context (cross-attention K / V^T) stays out of the launch counts
        for on in (True, False):
            U.FOLD_FF_OUT = on
            pf.LAUNCH_LOG = []
            with torch.no_grad():
                outs[on] = tr.forward_pf(pf.PF.from_nchw(x), ctx).to_nchw().float()
            launches[on] = len(pf.LAUNCH_LOG)
    finally:
        U.FOLD_FF_OUT = old
        pf.LAUNCH_LOG = None
    assert launches[False] - launches[True] == (1 if folds else 0)          # one engine launch less where the fold applies, the same launches where it does not
    with torch.no_grad():
        ref = tr.float()(x.float(), ctx.float())
    scale = max(1.0, ref.abs().max().item())
    e_on, e_off, e_ab = ((outs[True] - ref).abs().max().item(), (outs[False] - ref).abs().max().item(), (outs[True] - outs[False]).abs().max().item())
    print(f"C={C} {hw}x{hw} B={B} {dtype}: |on - ref| {e_on:.3e}  |off - ref| {e_off:.3e}  |on - off| {e_ab:.3e}  bound {1e-2 * scale:.3e}")
    assert torch.isfinite(outs[True]).all()
    assert e_on <= 1e-2 * scale
    assert e_off <= 1e-2 * scale
    assert e_ab <= 1e-2 * scale
    if not folds:
        assert torch.equal(outs[True], outs[False])


@pytest.mark.parametrize("hw", [16, 32])
def test_unet_forward_with_and_without_the_fold(hw, request):
    """the whole SD 2.1-shaped UNet at two images, plain and classifier-free-guidance (shared latents) forwards.  16 x 16 latents: the 320-channel transformers
    fold (256 tokens per image), the deeper ones have at most 128 rows and keep the small-batch kernel's two launches; 32 x 32: the 640-channel ones fold too."""
    from gswm_amd import unet as U
    if hw == 16:          # the mid block's 2 x 2 lattice has 4 keys, off the attention kernel's keys % 8 grid: that one attention runs torch SDPA
        request.getfixturevalue("library_kernels_allowed")
    torch.manual_seed(0)
    m = U.synthetic_init_(U.UNet2DCondition(), 0).cuda().half().eval()
    x = torch.randn(2, 4, hw, hw, device="cuda").half()
    t = torch.full((), 481, device="cuda")
    ctx = torch.randn(2, 77, 1024, device="cuda").half()
    ctx2 = torch.cat([torch.randn(1, 77, 1024, device="cuda").half().expand(2, -1, -1), ctx], dim=0)      # (uncond x 2 | text x 2)
    U.FALLBACKS.clear()
    outs = {}
    old = U.FOLD_FF_OUT
    try:
        for on in (True, False):
            U.FOLD_FF_OUT = on
            with torch.no_grad():
                outs[on] = (m(x, t, ctx).float(), m(x, t, ctx2, cfg_dup=True).float())
    finally:
        U.FOLD_FF_OUT = old
    if hw == 16:
        assert all("Sq=4 Sk=4" in why for why in U.FALLBACKS), U.FALLBACKS        # nothing but the 4-key attention left the hand-written path
    else:
        assert U.FALLBACKS == {}, U.FALLBACKS
    for a, b in zip(outs[True], outs[False]):
        assert a.shape == b.shape and torch.isfinite(a).all()
        d = (a - b).abs().max().item()
        print(f"UNet {hw}x{hw}: |on - off| {d:.3e}  bound {2e-2 * max(1.0, b.abs().max().item()):.3e}")
        assert d > 0.0                                   # the fold did run: a product rounded once is not the two roundings bit for bit
        assert d <= 2e-2 * max(1.0, b.abs().max().item())


def test_toggle_after_a_capture_captures_anew():
    """graph.GraphedEpsModel keys its entries by the switch: toggled after a capture, the next call captures the other launch sequence instead of replaying the old one"""
    from gswm_amd import unet as U, graph
    torch.manual_seed(1)
    # the product architecture at a quarter of the SD widths (tests/test_gpu_graph.py): at two 32 x 32 latents its 64- and 128-channel transformers fold
    m = U.UNet2DCondition(block_out_channels=(64, 128, 256, 256), cross_attention_dim=128, num_heads=(1, 2, 4, 4), head_dim=64)
    m = U.synthetic_init_(m, 0).cuda().half().eval()
    eps = graph.GraphedEpsModel(m, mode="always")
    x = torch.randn(2, 4, 32, 32, device="cuda").half()
    t = torch.full((), 41, dtype=torch.int64, device="cuda")
    ctx = torch.randn(2, 77, 128, device="cuda").half()
    old = U.FOLD_FF_OUT
    try:
        with torch.no_grad():
            U.FOLD_FF_OUT = True
            y_on = eps(x, t, ctx)
            assert eps.stats["captures"] == 1
            assert torch.equal(y_on, m(x, t, ctx))
            U.FOLD_FF_OUT = False
            y_off = eps(x, t, ctx)
            assert eps.stats["captures"] == 2
            assert torch.equal(y_off, m(x, t, ctx)) and not torch.equal(y_off, y_on)
            U.FOLD_FF_OUT = True
            assert torch.equal(eps(x, t, ctx), y_on) and eps.stats["captures"] == 2          # the first entry serves again
    finally:
        U.FOLD_FF_OUT = old
