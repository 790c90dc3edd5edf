"""CPU (no GPU): the DPM-Solver++ 2M sampling schedule (`ddim.DPMSolverSchedule`) in float64 numpy -- its coefficient form against the stepwise restatement
of tests/dpm_reference.py, its order of convergence, its consistency with the inverse schedule, the Karras option, the pipeline keyword and the argument
checks of `gsw_dpm_step` that are decided before any launch."""
import ctypes

import numpy as np
import pytest

import dpm_reference as R
from test_gpu_ddim import analytic_eps_np

import gswm_amd
from gswm_amd import _native as N, ddim, pipeline


def run_coefficients(steps, eps_fn, z):
    """the loop of ddim.dpms_sample / dpms_invert on the host: m0 = P x + Q out, x' = A x + B m0 + C m_prev"""
    x = np.array(z, dtype=np.float64)
    m_prev = None
    for t, (P, Q), (A, B, C) in steps:
        m0 = P * x + Q * eps_fn(x, t)
        x = A * x + B * m0 + (C * m_prev if C != 0.0 else 0.0)
        m_prev = m0
    return x


def rms(a):
    return float(np.sqrt(np.mean(np.square(a))))


@pytest.fixture(scope="module")
def z64():
    return np.random.RandomState(0).randn(2, 4, 64, 64)


@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
@pytest.mark.parametrize("spacing", ["linspace", "leading"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 10, 20])
def test_coefficient_form_equals_the_stepwise_solver(S, order, spacing, final, prediction_type):
    z = np.random.RandomState(S).randn(2, 4, 8, 8)
    sched = ddim.DPMSolverSchedule(S, solver_order=order, timestep_spacing=spacing, final_sigmas_type=final, prediction_type=prediction_type)
    steps = sched.steps()
    assert len(steps) == S and [s[0] for s in steps] == [int(t) for t in sched.timesteps]
    got = run_coefficients(steps, analytic_eps_np, z)
    ref = R.dpms_sample_reference(analytic_eps_np, z, S, solver_order=order, timestep_spacing=spacing, final_sigmas_type=final, prediction_type=prediction_type)
    np.testing.assert_allclose(got, ref, rtol=1e-10, atol=0)          # both float64; they differ in association only
    assert all(C == 0.0 for _, _, (_, _, C) in steps) == (order == 1 or S <= 2)     # below 15 steps the first and the last step are first order


@pytest.mark.parametrize("karras", [False, True])
def test_stepwise_reference_and_schedule_agree_on_timesteps_and_sigmas(karras):
    for S in (10, 20, 50):
        sched = ddim.DPMSolverSchedule(S, use_karras_sigmas=karras)
        ts, sig = R.timesteps_and_sigmas(S, use_karras_sigmas=karras)
        assert np.array_equal(sched.timesteps, ts)
        np.testing.assert_allclose(sched.sigmas, sig, rtol=1e-12, atol=0)
        z = np.random.RandomState(S).randn(1, 4, 8, 8)
        np.testing.assert_allclose(run_coefficients(sched.steps(), analytic_eps_np, z), R.dpms_sample_reference(analytic_eps_np, z, S, use_karras_sigmas=karras),
                                   rtol=1e-10, atol=0)


def test_second_order_convergence(z64):
    """20 steps against 999 steps of the order-2 solver: the second-order result is less than half as far away as the first-order one (the numpy
    restatement gives 0.027 against 0.121).  A coefficient with the wrong sign or a wrong r0 loses the order."""
    run = lambda S, order: run_coefficients(ddim.DPMSolverSchedule(S, solver_order=order).steps(), analytic_eps_np, z64)
    fine = run(999, 2)
    d2, d1 = rms(run(20, 2) - fine), rms(run(20, 1) - fine)
    print(f"RMS distance to the 999-step result: order 2 {d2:.4f}, order 1 {d1:.4f}")
    assert d2 < 0.5 * d1, (d2, d1)


def test_sampler_and_inverse_schedule_are_mutually_consistent(z64):
    """20-step sampling (linspace, guidance 1) followed by the 20-step inverse schedule on the same eps function comes back to z"""
    x0 = run_coefficients(ddim.DPMSolverSchedule(20, timestep_spacing="linspace").steps(), analytic_eps_np, z64)
    back = run_coefficients(ddim.DPMSolverInverseSchedule(20).steps(), analytic_eps_np, x0)
    err, agree = rms(back - z64), float(np.mean((back >= 0) == (z64 >= 0)))
    print(f"sample -> invert: RMS error {err:.4f}, sign agreement {agree:.4f}")
    assert err < 0.02, err
    assert agree > 0.99, agree


@pytest.mark.parametrize("S", [10, 20, 50])
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
def test_karras_sigmas_and_timesteps(S, final):
    sched = ddim.DPMSolverSchedule(S, use_karras_sigmas=True, final_sigmas_type=final)
    sig, ts = sched.sigmas, sched.timesteps
    assert len(sig) == S + 1 and len(ts) == S
    assert np.all(np.diff(sig[:S]) < 0)                                   # the S Karras sigmas: strictly decreasing
    assert sig[S] < sig[S - 1] if final == "zero" else sig[S] == sig[S - 1]
    assert ts.dtype == np.int64 and np.all(np.diff(ts) <= 0)              # non-increasing integers; repeats at the low end are legal
    assert int(ts[0]) == 999 and int(ts.min()) >= 0 and int(ts.max()) <= 999
    if S == 50:
        assert int(np.sum(np.diff(ts) == 0)) == 1
    for t, (P, Q), (A, B, C) in sched.steps():
        assert all(np.isfinite(v) for v in (P, Q, A, B, C))


def test_final_sigma_zero_returns_the_x0_prediction():
    for S in (1, 10, 20):
        for karras in (False, True):
            assert ddim.DPMSolverSchedule(S, final_sigmas_type="zero", use_karras_sigmas=karras).steps()[-1][2] == (0.0, 1.0, 0.0)
    assert ddim.DPMSolverSchedule(20, final_sigmas_type="sigma_min").steps()[-1][2][0] > 0.0
    # lower_order_final: a first-order last step below 15 steps only
    assert ddim.DPMSolverSchedule(10, final_sigmas_type="sigma_min").steps()[-1][2][2] == 0.0
    assert ddim.DPMSolverSchedule(20, final_sigmas_type="sigma_min").steps()[-1][2][2] != 0.0
    assert ddim.DPMSolverSchedule(10, final_sigmas_type="sigma_min", lower_order_final=False).steps()[-1][2][2] != 0.0


def test_schedule_refuses_bad_arguments():
    for kw in (dict(num_inference_steps=0), dict(solver_order=3), dict(timestep_spacing="trailing"), dict(final_sigmas_type="one"), dict(prediction_type="sample")):
        with pytest.raises(ValueError):
            ddim.DPMSolverSchedule(**kw)


def _pipe(**kw):
    return pipeline.GaussianShadingPipeline(lambda x, t, c: x, bytes(32), bytes(16), b"k" * 32, **kw)


def test_pipeline_refuses_an_unknown_sampler():
    with pytest.raises(ValueError) as e:
        _pipe(sampler="euler_a")
    for name in ("ddim", "dpmpp_2m", "dpmpp_2m_karras"):
        assert repr(name) in str(e.value)


def test_pipeline_default_is_the_ddim_schedule_as_before():
    p = _pipe()
    assert p.sampler == "ddim" and isinstance(p.sampling_schedule, ddim.DDIMSchedule) and p.sampling_schedule is p.schedule
    assert p.schedule.num_inference_steps == 50
    p = _pipe(num_inference_steps=30, sampler="dpmpp_2m")
    assert isinstance(p.sampling_schedule, ddim.DPMSolverSchedule) and p.sampling_schedule.num_inference_steps == 20 and not p.sampling_schedule.use_karras_sigmas
    assert isinstance(p.schedule, ddim.DDIMSchedule) and p.schedule.num_inference_steps == 30          # inversion stays DDIM
    p = _pipe(sampler="dpmpp_2m_karras", num_sampling_steps=25, prediction_type="v_prediction")
    assert p.sampling_schedule.use_karras_sigmas and p.sampling_schedule.num_inference_steps == 25 and p.sampling_schedule.prediction_type == "v_prediction"
    p = _pipe(num_sampling_steps=20)
    assert isinstance(p.sampling_schedule, ddim.DDIMSchedule) and p.sampling_schedule.num_inference_steps == 20 and p.schedule.num_inference_steps == 50


def test_dpm_step_argument_validation_needs_no_gpu():
    """status codes of gsw_dpm_step that are decided before any launch"""
    lib = N.lib()
    p = ctypes.c_void_p(16)
    OK, BAD = N.GSW_OK, N.GSW_ERR_BAD_ARG
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, N.GSW_F32, 0, None) == OK            # n == 0: no launch
    assert lib.gsw_dpm_step(p, p, p, p, p, p, 1.0, 0.0, 1.0, 0.0, 0.5, 7.5, N.GSW_F16, 0, None) == OK
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, N.GSW_F64, 8, None) == BAD           # f64 unsupported
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, N.GSW_F64, 0, None) == BAD
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 9, 8, None) == BAD
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.5, 0.0, N.GSW_F32, 8, None) == BAD           # second order without m_prev
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.5, 0.0, N.GSW_F32, 0, None) == BAD
    assert lib.gsw_dpm_step(p, p, None, None, p, p, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, N.GSW_F32, -1, None) == BAD
    for null in range(4):                                                                                              # x, e_uncond, x_out, m_out
        a = [p, p, None, None, p, p]
        a[(0, 1, 4, 5)[null]] = None
        assert lib.gsw_dpm_step(*a, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, N.GSW_F32, 8, None) == BAD


def test_dpm_step_wrappers_refuse_cpu_tensors_and_missing_m_prev():
    import torch
    from gswm_amd import codec
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.dpm_step(z, z, (1.0, 0.0), (1.0, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.dpm_step_cfg(z, z, z, (1.0, 0.0), (1.0, 0.0, 0.0), 7.5)
