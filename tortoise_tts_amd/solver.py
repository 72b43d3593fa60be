"""Host side of the deterministic diffusion solvers (include/tortoise_mi355x_solver.h, csrc/misc.hip solver_update_kernel,
stages.DiffusionStage.solve / solve_many): DDIM (eta = 0, what the reference's `ddim_sample` computes) and DPM-Solver++(2M) (Lu et al.
2022, data prediction, multistep order 2) on the reference's 4000-step linear schedule.

With abar_t the trained schedule's cumulative product, alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = log(alpha_t / sigma_t)
and x0 the guided, clamped data prediction of a step, both solvers are one linear update per step,

    x_next = a x + b x0 + c x0_prev

    ddim      a = sigma_next / sigma_i,  b = alpha_next - sigma_next alpha_i / sigma_i,  c = 0
    dpm++2m   h = lambda_next - lambda_i,  e = -alpha_next expm1(-h),  r = (lambda_i - lambda_{i+1}) / h
              a = sigma_next / sigma_i,  b = e (1 + 1 / (2 r)),  c = -e / (2 r);  the first step run is first order (b = e, c = 0)

and the terminal step of either (alpha_next = 1, sigma_next = 0) is (0, 1, 0): the result is the clamped x0.  Spaced indices run
i = M - 1 ... 0.  Tables are float64; the engine receives float32 scalars, as with schedule.Schedule.

No trained checkpoint has been rendered with these solvers: what is verified is that they integrate the probability-flow ODE (closed-form
problems in tests/test_solver_cpu.py) and that the device does what the fp64 loop does.  The step counts they make possible are
unvalidated for audio quality; the default sampler stays the reference's.
"""
import numpy as np

from .schedule import base_alphas_cumprod, space_timesteps

KINDS = ("ddim", "dpm++2m")
SPACINGS = ("uniform", "logsnr")
DEFAULT_SPACING = {"ddim": "uniform", "dpm++2m": "logsnr"}


def logsnr_timesteps(lam, n):
    """n targets evenly spaced in lambda from lambda_{T-1} to lambda_0, each mapped to the timestep with the nearest lambda (ties: the
    smaller timestep), duplicates collapsed -> sorted distinct timesteps (at most n)."""
    targets = np.linspace(lam[-1], lam[0], n)
    d = np.abs(lam[None, :] - targets[:, None])
    return sorted(set(int(t) for t in np.argmin(d, axis=1)))  # (argmin returns the first, i.e. the smallest, index of a tie)


class SolverPlan:
    """The per-step records of one solver run.  kind: 'ddim' | 'dpm++2m'; steps: the requested N; spacing: None (the kind's default) |
    'uniform' (the p sampler's space_timesteps set) | 'logsnr'.  n_steps: the M <= N steps that actually run (logsnr collapses
    duplicates).  Arrays are indexed by the spaced index i (timesteps ascending); run order is i = M - 1 ... 0."""

    def __init__(self, kind, steps, spacing=None, trained_steps=4000, cond_free=True, cond_free_k=2.0):
        if kind not in KINDS:
            raise ValueError(f"unknown sampler {kind!r} (ddim | dpm++2m)")
        spacing = DEFAULT_SPACING[kind] if spacing is None else spacing
        if spacing not in SPACINGS:
            raise ValueError(f"unknown sampler_spacing {spacing!r} (uniform | logsnr)")
        steps = int(steps)
        if not 1 <= steps <= trained_steps:
            raise ValueError(f"diffusion_iterations={steps} must lie in 1 .. {trained_steps}")
        self.kind, self.spacing, self.requested_steps = kind, spacing, steps
        self.cond_free, self.cond_free_k = bool(cond_free), float(cond_free_k)
        abar = base_alphas_cumprod(trained_steps)
        alpha_all, sigma_all = np.sqrt(abar), np.sqrt(1.0 - abar)
        lam_all = np.log(alpha_all / sigma_all)
        ts = sorted(space_timesteps(trained_steps, [steps])) if spacing == "uniform" else logsnr_timesteps(lam_all, steps)
        self.timestep_map = np.array(ts, dtype=np.int64)
        M = self.n_steps = self.num_timesteps = len(ts)
        alpha, sigma, lam = alpha_all[ts], sigma_all[ts], lam_all[ts]
        self.cfk = self.cond_free_k * (1.0 - np.arange(M) / M)  # the p sampler's ramp
        self.sqrt_recip = 1.0 / alpha
        self.sqrt_recipm1 = sigma / alpha
        self.a, self.b, self.c = np.zeros(M), np.zeros(M), np.zeros(M)
        self.b[0] = 1.0  # terminal: the clamped x0
        for i in range(1, M):
            a_n, s_n = alpha[i - 1], sigma[i - 1]
            self.a[i] = s_n / sigma[i]
            if kind == "ddim":
                self.b[i] = a_n - s_n * alpha[i] / sigma[i]
                continue
            h = lam[i - 1] - lam[i]
            e = -a_n * np.expm1(-h)
            if i == M - 1:  # the first step run has no history: first order
                self.b[i] = e
                continue
            r = (lam[i] - lam[i + 1]) / h
            self.b[i] = e * (1.0 + 1.0 / (2.0 * r))
            self.c[i] = -e / (2.0 * r)

    @staticmethod
    def f32(arr, i):
        return float(np.float32(arr[i]))


def sampler_options(kwargs, steps, trained_steps=4000, cond_free=True, cond_free_k=2.0):
    """Takes `sampler` (None | 'p' | 'ddim' | 'dpm++2m') and `sampler_spacing` (None | 'uniform' | 'logsnr') out of a tts() call's **kwargs
    -> None (the reference's ancestral sampler: nothing is built) or the SolverPlan of `steps` diffusion iterations."""
    kind, spacing = kwargs.pop("sampler", None), kwargs.pop("sampler_spacing", None)
    if kind is None or kind == "p":
        if spacing is not None:
            raise ValueError("sampler_spacing belongs to the solvers (sampler='ddim' | 'dpm++2m'): the p sampler walks the reference's timesteps")
        return None
    return SolverPlan(kind, steps, spacing, trained_steps, cond_free, cond_free_k)


def refuse_streaming(kwargs, who):
    for key in ("sampler", "sampler_spacing"):
        if key in kwargs:
            raise ValueError(f"{who}: {key} is not available here: the HiFi-GAN path has no diffusion stage (use api.TextToSpeech)")
