"""GPU: DPM-Solver++ 2M sampling -- the one-launch scheduler step `gsw_dpm_step` against torch on poisoned, guard-banded buffers (tests/poison.py), the
loops `ddim.dpms_sample` / `dpms_invert(fused=True)` against the float64 stepwise solver of tests/dpm_reference.py, and the pipeline's `sampler="dpmpp_2m"`
on a small UNet (round trip, graph replay)."""
import types

import numpy as np
import pytest
import torch

import gs_oracle as O
import dpm_reference as R
from poison import NAN, Ledger, poisoned
from test_gpu_ddim import analytic_eps, analytic_eps_np, _bc_eps

pytestmark = pytest.mark.gpu

GSW_WG = 256                    # csrc/gswm_kernels.hip
# the margin of test_small_unet_roundtrip_with_dpmpp_2m: over seeds 5-8 the sign agreement after DPM-Solver++ 2M sampling lies 0.0155-0.0180 below
# the one after DDIM sampling (fp32 restatement of that test; mean 0.0165, standard deviation 0.0011): the largest gap plus six standard deviations
SIGN_AGREEMENT_MARGIN = 0.025


@pytest.fixture(scope="module")
def P():
    import gswm_amd
    from gswm_amd import codec, ddim, unet, pipeline, graph
    return types.SimpleNamespace(codec=codec, ddim=ddim, unet=unet, pipeline=pipeline, graph=graph)


def _grid_cap_elements():
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * GSW_WG * 8


def _sizes():
    # below one vector; one vector; vectors + tail over several blocks; a latent; past the grid cap (the stride loop's second trip) with a tail
    return [7, 8, 2053, 4 * 64 * 64, "cap+13"]


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("n", _sizes())
def test_dpm_step_vs_torch(P, dtype, n):
    """m_out is bit-equal to ddim_step[_cfg](x, e, P, Q); x_out agrees with fp32 torch A x + B m_out + C m_prev rounded once, to the tolerance of
    test_gpu_codec.py::test_ddim_step_vs_torch_fp32; in place == out of place bit for bit; no store outside a buffer, no unwritten output element, and
    no read of m_prev at first order (a NaN-filled m_prev with C = 0 changes nothing)."""
    codec = P.codec
    if n == "cap+13":
        n = _grid_cap_elements() + 13
    steps = P.ddim.DPMSolverSchedule(20).steps()
    tol = {torch.float32: 5e-7, torch.float16: 1e-3, torch.bfloat16: 8e-3}[dtype]
    g = torch.Generator(device="cuda").manual_seed(n % 100003)
    x, e, et, mp = (torch.randn(n, device="cuda", generator=g).to(dtype) for _ in range(4))
    for cfg in (False, True):
        for order2 in (False, True):
            _, pq, abc = steps[10] if order2 else steps[0]
            assert (abc[2] != 0.0) == order2
            (p32, q32), (a32, b32, c32) = ([float(np.float32(v)) for v in pq], [float(np.float32(v)) for v in abc])
            L = Ledger(NAN)
            try:
                with poisoned(L):
                    xw, ew, tw, mw = L.wrap(x), L.wrap(e), L.wrap(et), L.wrap(mp)

                    def step(xx, m_prev, **kw):
                        if cfg:
                            return codec.dpm_step_cfg(xx, ew, tw, pq, abc, 7.5, m_prev, **kw)
                        return codec.dpm_step(xx, ew, pq, abc, m_prev, **kw)

                    xo, mo = step(xw, mw if order2 else None)                              # out of place: both outputs are ledger buffers
                    assert L.untouched(xo) == 0, L.where(xo)
                    assert L.untouched(mo) == 0, L.where(mo)
                    assert torch.equal(xw, x) and torch.equal(mw, mp)                      # the inputs are inputs
                    if not order2:                                                         # first order never reads m_prev: NaN everywhere in it, same bits out
                        xo_p, mo_p = step(xw, L.empty_like(xw))
                        assert torch.equal(xo_p.view(torch.uint8), xo.view(torch.uint8)) and torch.equal(mo_p.view(torch.uint8), mo.view(torch.uint8))
                    xi, mi = L.wrap(x), L.wrap(mp)                                         # fully in place
                    r = step(xi, mi if order2 else None, out=xi, m_out=mi)
                    assert r[0] is xi and r[1] is mi
                    assert torch.equal(xi, xo), f"in place x differs in {int((xi != xo).sum())} elements"
                    assert torch.equal(mi, mo), f"in place m differs in {int((mi != mo).sum())} elements"
                torch.cuda.synchronize()
                L.check()
                m_ref = codec.ddim_step_cfg(x, e, et, pq[0], pq[1], 7.5) if cfg else codec.ddim_step(x, e, pq[0], pq[1])
                assert torch.equal(mo, m_ref), f"cfg={cfg} order2={order2}: {int((mo != m_ref).sum())} x0 predictions differ from gsw_ddim_step's"
                ref = a32 * x.float() + b32 * mo.float()
                if order2:
                    ref = ref + c32 * mp.float()
                err = (xo.float() - ref).abs().max().item()
                bound = tol * max(1.0, ref.abs().max().item())
                assert err <= bound, (cfg, order2, err, bound)
            finally:
                L.release()


def test_dpm_step_wrapper_checks(P):
    x = torch.zeros(16, device="cuda", dtype=torch.float16)
    with pytest.raises(ValueError):
        P.codec.dpm_step(x, x, (1.0, 0.0), (1.0, 0.5, 0.25))                     # second order without m_prev
    with pytest.raises(ValueError):
        P.codec.dpm_step(x, x.float(), (1.0, 0.0), (1.0, 0.5, 0.0))              # dtype
    with pytest.raises(ValueError):
        P.codec.dpm_step(x, x[:8], (1.0, 0.0), (1.0, 0.5, 0.0))                  # numel
    with pytest.raises(ValueError):
        P.codec.dpm_step(x, x, (1.0, 0.0), (1.0, 0.5, 0.0), m_out=x[::2])        # contiguity
    with pytest.raises(ValueError):
        P.codec.dpm_step_cfg(x, x, x[:8], (1.0, 0.0), (1.0, 0.5, 0.0), 7.5)


# ---------------------------------------------------------------------------------------------------------------- the loops
@pytest.fixture(scope="module")
def zT32():
    return torch.from_numpy(np.random.RandomState(11).randn(2, 4, 64, 64)).float().cuda()


def _guided_eps_np(x, t):
    """what _bc_eps gives the two halves of a guidance batch, combined at guidance 7.5"""
    eu = 0.3 * np.tanh(x) + 0.05 * np.sin(3.0 * x + 0.01 * t)
    et = eu + 0.1 * np.cos(2.0 * x - 0.003 * t)
    return eu + 7.5 * (et - eu)


def test_sampling_loop_vs_float64_solver(P, zT32):
    sched = P.ddim.DPMSolverSchedule(20)
    B = zT32.shape[0]
    x0 = P.ddim.dpms_sample(analytic_eps, zT32, torch.zeros(B, 1, 1, device="cuda"), sched, guidance_scale=1.0)
    ref = R.dpms_sample_reference(analytic_eps_np, zT32.cpu().double().numpy(), 20)
    err = np.abs(x0.cpu().numpy() - ref).max()
    print(f"dpms_sample, guidance 1: max|d| = {err:.3e} (|ref|max {np.abs(ref).max():.3f})")
    np.testing.assert_allclose(x0.cpu().numpy(), ref, rtol=0, atol=1e-3 * max(1.0, np.abs(ref).max()))
    assert x0.data_ptr() != zT32.data_ptr()


def test_guided_sampling_loop_vs_float64_solver(P, zT32):
    sched = P.ddim.DPMSolverSchedule(20)
    B = zT32.shape[0]
    x0 = P.ddim.dpms_sample(_bc_eps, zT32, torch.ones(B, 1, device="cuda"), sched, ctx_uncond=torch.zeros(B, 1, device="cuda"), guidance_scale=7.5)
    ref = R.dpms_sample_reference(_guided_eps_np, zT32.cpu().double().numpy(), 20)
    err = np.abs(x0.cpu().numpy() - ref).max()
    print(f"dpms_sample, guidance 7.5: max|d| = {err:.3e} (|ref|max {np.abs(ref).max():.3f})")
    np.testing.assert_allclose(x0.cpu().numpy(), ref, rtol=0, atol=1e-3 * max(1.0, np.abs(ref).max()))


def test_sampling_loop_is_one_launch_per_step(P, zT32, monkeypatch):
    """one codec.dpm_step[_cfg] call per step, in place on x and on ONE buffer of x0 predictions; nothing else from the step family"""
    calls = []
    real = P.codec._dpm_step

    def spy(x, eu, et, pq, abc, g, m_prev, out, m_out):
        calls.append((x.data_ptr(), out.data_ptr(), m_out.data_ptr(), None if m_prev is None else m_prev.data_ptr(), abc[2]))
        return real(x, eu, et, pq, abc, g, m_prev, out, m_out)

    monkeypatch.setattr(P.codec, "_dpm_step", spy)
    monkeypatch.setattr(P.codec, "ddim_step", lambda *a, **k: pytest.fail("ddim_step launched inside dpms_sample"))
    B = zT32.shape[0]
    P.ddim.dpms_sample(analytic_eps, zT32, torch.zeros(B, 1, 1, device="cuda"), P.ddim.DPMSolverSchedule(20), guidance_scale=1.0)
    assert len(calls) == 20
    assert len({c[2] for c in calls}) == 1 and all(c[0] == c[1] for c in calls)
    assert all((c[3] is None) == (c[4] == 0.0) and c[3] in (None, c[2]) for c in calls)


def _unfused_inversion(P, eps_model, x0, ctx, schedule):
    """the three-launch loop of ddim.dpms_invert as it stood before the fused step existed"""
    codec = P.codec
    steps = schedule.steps()
    tt = [torch.full((), s[0], dtype=torch.int64, device=x0.device) for s in steps]
    x = x0.clone()
    m_prev = None
    for (t, (Pc, Qc), (A, B, C)), t_dev in zip(steps, tt):
        m0 = codec.ddim_step(x, eps_model(x, t_dev, ctx), Pc, Qc)
        codec.ddim_step(x, m0, A, B, out=x)
        if C != 0.0:
            codec.ddim_step(x, m_prev, 1.0, C, out=x)
        m_prev = m0
    return x


def test_fused_inversion_vs_the_three_launch_loop(P, zT32):
    sched = P.ddim.DPMSolverInverseSchedule(20)
    B = zT32.shape[0]
    ctx = torch.zeros(B, 1, 1, device="cuda")
    x0 = (zT32 * 0.2).contiguous()
    plain = P.ddim.dpms_invert(analytic_eps, x0, ctx, sched)
    assert torch.equal(plain, P.ddim.dpms_invert(analytic_eps, x0, ctx, sched, fused=False))
    assert torch.equal(plain, _unfused_inversion(P, analytic_eps, x0, ctx, sched)), "the default dpms_invert no longer gives the three-launch loop's bits"
    fused = P.ddim.dpms_invert(analytic_eps, x0, ctx, sched, fused=True)
    err = (fused - plain).abs().max().item()
    print(f"dpms_invert fused vs unfused: max|d| = {err:.3e}")
    assert err <= 1e-3 * max(1.0, plain.abs().max().item())
    ref = O.dpms_invert_reference(lambda x, t: analytic_eps_np(x, t), x0.cpu().double().numpy(), 20)
    np.testing.assert_allclose(fused.cpu().numpy(), ref, rtol=0, atol=1e-3 * max(1.0, np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def _small_roundtrip(P, keys, sampler, seed=5):
    """model, contexts, seed and sizes of tests/test_gpu_ddim.py::test_small_unet_roundtrip_is_lossless"""
    key, nonce = keys
    k = O.pad_message("lthero", 32)
    torch.manual_seed(0)
    m = P.unet.UNet2DCondition(block_out_channels=(64, 128, 128, 128), cross_attention_dim=64, num_heads=(2, 4, 4, 4), head_dim=32)
    P.unet.synthetic_init_(m, 0)
    m = m.cuda().half().eval()
    g = torch.Generator().manual_seed(1)
    cu = torch.randn(1, 77, 64, generator=g).cuda().half()
    B = 4
    ct = torch.randn(B, 77, 64, generator=g).cuda().half()
    pipe = P.pipeline.GaussianShadingPipeline(m, key, nonce, k, num_inference_steps=20, ctx_uncond=cu, sampler=sampler,
                                              num_sampling_steps=20 if sampler != "ddim" else None)
    zT, x0, bits, flags = pipe.roundtrip(B, ct, seed=seed, guidance_scale=7.5)
    zi = pipe.invert(x0)
    agree = ((zi >= 0) == (zT >= 0)).float().mean().item()
    return types.SimpleNamespace(pipe=pipe, k=k, zT=zT, x0=x0, bits=bits, flags=flags, zi=zi, agree=agree)


@pytest.mark.usefixtures("library_kernels_allowed")      # small / odd shapes off the hand-written path: strict mode (the default) would raise
def test_small_unet_roundtrip_with_dpmpp_2m(P, keys):
    """embed -> 20 DPM-Solver++ 2M CFG sampling steps -> 20 DDIM inversion steps -> vote on the small UNet: every bit of every image comes back, and the
    inverted latent's signs agree with the embedded ones about as often as after DDIM sampling (both measured here; the margin: DESIGN.md 4.13)."""
    key, nonce = keys
    r = _small_roundtrip(P, keys, "dpmpp_2m")
    assert isinstance(r.pipe.sampling_schedule, P.ddim.DPMSolverSchedule) and r.pipe.sampling_schedule.num_inference_steps == 20
    assert r.zT.shape == (4, 4, 64, 64) and r.x0.shape == r.zT.shape and torch.isfinite(r.x0).all()
    assert int(r.flags.abs().sum()) == 0
    for b in range(4):
        assert P.codec.bits_to_str(r.bits[b].cpu().numpy()) == O.recover_bits(r.zi[b].cpu().numpy(), key, nonce, 256)
    d = _small_roundtrip(P, keys, "ddim")
    print(f"sign agreement zi / zT: dpmpp_2m {r.agree:.4f}, ddim {d.agree:.4f}; bits matched (min over images): "
          f"dpmpp_2m {int(P.codec.bit_matches(r.bits, 256, r.k).min())}, ddim {int(P.codec.bit_matches(d.bits, 256, d.k).min())}")
    assert torch.equal(d.zT, r.zT)
    assert int(P.codec.bit_matches(r.bits, 256, r.k).min()) == 256
    assert r.agree >= d.agree - SIGN_AGREEMENT_MARGIN, (r.agree, d.agree)


def test_dpmpp_2m_roundtrip_through_the_graph_equals_eager(P, keys):
    """batch 1 (the guidance batch: 2 rows) on the graph-replayed eps model == the same call on the ungraphed model, bit for bit: the step kernel takes
    its coefficients as arguments and sits outside the captured forward.  The small configuration of tests/test_gpu_graph.py."""
    key, nonce = keys
    m = P.unet.UNet2DCondition(block_out_channels=(64, 128, 256, 256), cross_attention_dim=128, num_heads=(1, 2, 4, 4), head_dim=64)
    m = P.unet.synthetic_init_(m, 2).cuda().half().eval()
    g = torch.Generator().manual_seed(5)
    cu = torch.randn(1, 77, 128, generator=g).cuda().half()
    ct = torch.randn(1, 77, 128, generator=g).cuda().half()
    res = []
    for mode in ("always", "never"):
        gm = P.graph.GraphedEpsModel(m, mode=mode, clone_output=False)
        pipe = P.pipeline.GaussianShadingPipeline(gm, key, nonce, P.codec.pad_message("lthero", 32), height=256, width=256, num_inference_steps=6,
                                                  ctx_uncond=cu, sampler="dpmpp_2m", num_sampling_steps=6)
        assert pipe.eps_model is gm
        res.append((pipe.roundtrip(1, ct, seed=3, guidance_scale=7.5), dict(gm.stats)))
    (a, sa), (b, sb) = res
    assert sa["replays"] >= 10 and sb["replays"] == 0, (sa, sb)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[1]).all()
