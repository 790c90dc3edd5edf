"""float64 reference for DPM-Solver++ multistep sampling (tests/test_dpm_sampler_host.py, tests/test_gpu_dpm_sampler.py).  A plain helper module, like
tests/poison.py: no pytest plugin, no settings.

The solver is written step by step, in the order it is published (Lu et al., "DPM-Solver++", Algorithm 2 with the midpoint rule; diffusers'
DPMSolverMultistepScheduler uses the same sigma parametrisation): convert the model output to the x0 prediction, form D1 = (m0 - m1) / r0, then
    x = (sigma_t / sigma_s) x - alpha_t (e^{-h} - 1) m0 - 1/2 alpha_t (e^{-h} - 1) D1.
It never forms the (A, B, C) coefficients of `ddim.DPMSolverSchedule.steps()`, and it builds its own timestep and sigma lists, so it checks both.
PARITY UNPINNED: diffusers is not available here."""
import numpy as np


def _alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012):
    return np.cumprod(1.0 - np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float64) ** 2)


def _sigma_to_t(sigma, log_sigmas):
    """the place of `sigma` in the log-sigma table by piecewise-linear interpolation, written out with explicit neighbours"""
    ls = np.log(max(sigma, 1e-10))
    low = int(np.clip(np.searchsorted(log_sigmas, ls, side="right") - 1, 0, len(log_sigmas) - 2))
    w = np.clip((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[low + 1]), 0.0, 1.0)
    return (1.0 - w) * low + w * (low + 1)


def timesteps_and_sigmas(S, *, timestep_spacing="linspace", final_sigmas_type="zero", use_karras_sigmas=False, T=1000):
    """(timesteps [S] descending int64, sigmas [S + 1])"""
    ac = _alphas_cumprod(T)
    table = np.sqrt((1.0 - ac) / ac)
    if timestep_spacing == "linspace":
        ts = np.linspace(0, T - 1, S + 1).round()[::-1][:-1].astype(np.int64)
    elif timestep_spacing == "leading":
        ts = ((np.arange(S) * (T // S)).round().astype(np.int64) + 1)[::-1]
    else:
        raise ValueError(timestep_spacing)
    if use_karras_sigmas:
        smax, smin, rho = table[-1], table[0], 7.0
        sig = np.array([(smax ** (1 / rho) + (j / (S - 1) if S > 1 else 0.0) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho for j in range(S)])
        ts = np.array([round(_sigma_to_t(s, np.log(table))) for s in sig]).astype(np.int64)
    else:
        sig = np.array([table[t] for t in ts])          # integer timesteps: the table's own entries
    last = {"zero": 0.0, "sigma_min": table[0]}[final_sigmas_type]
    return ts, np.concatenate([sig, [last]])


def _alpha_sigma(sigma):
    alpha = 1.0 / np.sqrt(sigma * sigma + 1.0)
    return alpha, sigma * alpha


def dpms_sample_reference(eps_fn, z_T, S, *, solver_order=2, timestep_spacing="linspace", final_sigmas_type="zero", prediction_type="epsilon",
                          lower_order_final=True, use_karras_sigmas=False):
    """x_T -> x_0 with `model_out = eps_fn(x, t)` (guidance, if any, is the caller's: eps_fn returns the guided output)."""
    ts, sigmas = timesteps_and_sigmas(S, timestep_spacing=timestep_spacing, final_sigmas_type=final_sigmas_type, use_karras_sigmas=use_karras_sigmas)
    x = np.array(z_T, dtype=np.float64)
    preds = []
    for i, t in enumerate(ts):
        out = eps_fn(x, int(t))
        alpha_s, sigma_s = _alpha_sigma(sigmas[i])
        # 1. the x0 prediction
        if prediction_type == "epsilon":
            m0 = (x - sigma_s * out) / alpha_s
        elif prediction_type == "v_prediction":
            m0 = alpha_s * x - sigma_s * out
        else:
            raise ValueError(prediction_type)
        preds.append(m0)
        alpha_t, sigma_t = _alpha_sigma(sigmas[i + 1])
        if sigma_t == 0.0:                       # lambda_t = +inf: h = inf, e^{-h} = 0, sigma_t / sigma_s = 0
            x = m0.copy()
            continue
        lam_t, lam_s = np.log(alpha_t) - np.log(sigma_t), np.log(alpha_s) - np.log(sigma_s)
        h = lam_t - lam_s
        final_first = i == S - 1 and lower_order_final and S < 15
        if solver_order == 1 or i == 0 or final_first or h == 0.0:
            x = (sigma_t / sigma_s) * x - alpha_t * (np.exp(-h) - 1.0) * m0
        else:
            alpha_p, sigma_p = _alpha_sigma(sigmas[i - 1])
            h_0 = lam_s - (np.log(alpha_p) - np.log(sigma_p))
            r0 = h_0 / h
            # 2. the difference quotient of the last two predictions
            D1 = (m0 - preds[-2]) / r0
            # 3. the midpoint update
            x = (sigma_t / sigma_s) * x - alpha_t * (np.exp(-h) - 1.0) * m0 - 0.5 * alpha_t * (np.exp(-h) - 1.0) * D1
    return x
