"""fp64 reference of the deterministic diffusion solvers (include/tortoise_mi355x_solver.h), written from the textbook forms and
independently of tortoise_tts_amd/solver.py:

    DDIM (Song et al. 2021, eta = 0)      eps = (x - alpha_i x0) / sigma_i;  x_next = alpha_next x0 + sigma_next eps
    DPM-Solver++(2M) (Lu et al. 2022, algorithm 2, data prediction)
                                          h = lambda_next - lambda_i;  r = h_prev / h;  D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev  (first step: D = x0)
                                          x_next = (sigma_next / sigma_i) x - alpha_next (exp(-h) - 1) D

on the 4000-step linear beta schedule, x0 = clamp((x - sigma_i eps) / alpha_i, -1, 1).  The (a, b, c) of x_next = a x + b x0 + c x0_prev are
derived from these only to be compared with the product's tables; solve_loop() runs the textbook forms.

update_reference() / operand_bound(): one step of the device's update kernel in fp64 on the f32 step record, and the element-wise bound of
the f32 kernel against it, from the operation count.
"""
import math

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of f32 (round to nearest)


def gamma(n, u=U32):
    """Higham's gamma_n: n roundings compound to at most n u / (1 - n u)."""
    return n * u / (1.0 - n * u)


def alphas_cumprod(trained_steps=4000):
    scale = 1000.0 / trained_steps
    betas = np.linspace(scale * 0.0001, scale * 0.02, trained_steps, dtype=np.float64)
    return np.cumprod(1.0 - betas)


def uniform_timesteps(trained_steps, n):
    """The reference's space_timesteps(trained_steps, [n]) (utils/diffusion.py:1152-1205)."""
    stride = 1.0 if n <= 1 else (trained_steps - 1) / (n - 1)
    return sorted({int(round(j * stride)) for j in range(n)}) if n > 1 else [0]


def logsnr_timesteps(lam, n):
    out = set()
    for target in np.linspace(lam[-1], lam[0], n):
        best, best_d = 0, math.inf
        for t in range(len(lam)):  # ascending t, strict "<": a tie keeps the smaller t
            d = abs(lam[t] - target)
            if d < best_d:
                best, best_d = t, d
        out.add(best)
    return sorted(out)


class RefPlan:
    def __init__(self, kind, steps, spacing, trained_steps=4000, cond_free=True, cond_free_k=2.0):
        assert kind in ("ddim", "dpm++2m") and spacing in ("uniform", "logsnr")
        self.kind, self.spacing, self.cond_free, self.cond_free_k = kind, spacing, bool(cond_free), float(cond_free_k)
        abar = alphas_cumprod(trained_steps)
        lam_all = 0.5 * (np.log(abar) - np.log1p(-abar))  # log(alpha / sigma), written the other way round than the product does
        ts = uniform_timesteps(trained_steps, steps) if spacing == "uniform" else logsnr_timesteps(lam_all, steps)
        self.timestep_map = np.array(ts, dtype=np.int64)
        self.n_steps = M = len(ts)
        self.alpha = np.sqrt(abar[ts])
        self.sigma = np.sqrt(1.0 - abar[ts])
        self.lam = np.log(self.alpha) - np.log(self.sigma)
        self.cfk = np.array([self.cond_free_k * (1.0 - i / M) for i in range(M)])

    def nxt(self, i):
        """(alpha, sigma) the step at spaced index i lands on; the step at i = 0 lands on the data (1, 0)."""
        return (1.0, 0.0) if i == 0 else (float(self.alpha[i - 1]), float(self.sigma[i - 1]))

    def abc(self):
        """The textbook updates as x_next = a x + b x0 + c x0_prev, float64 [M] each."""
        M = self.n_steps
        a, b, c = np.zeros(M), np.zeros(M), np.zeros(M)
        for i in range(M):
            al, sg = float(self.alpha[i]), float(self.sigma[i])
            an, sn = self.nxt(i)
            if i == 0:  # both: alpha_next x0 + 0 (DPM: sigma ratio 0, -(exp(-inf) - 1) = 1)
                b[i] = 1.0
            elif self.kind == "ddim":  # alpha_next x0 + sigma_next (x - alpha x0) / sigma
                a[i], b[i] = sn / sg, an - sn * al / sg
            else:
                h = self.lam[i - 1] - self.lam[i]
                e = -an * (math.exp(-h) - 1.0)
                a[i] = sn / sg
                if i == M - 1:
                    b[i] = e
                else:
                    r = (self.lam[i] - self.lam[i + 1]) / h
                    b[i], c[i] = e * (1.0 + 0.5 / r), -e * 0.5 / r
        return a, b, c


def solve_loop(plan, model, x_T):
    """The plan's solver in fp64 from x_T (numpy, any shape) with model(x, timestep, cfk) -> the (guided) eps prediction, textbook forms.
    Lu et al.: r_i = h_{i-1} / h_i, so 1 / (2 r) = h / (2 h_prev) with h_prev the step that ran before."""
    x = np.asarray(x_T, dtype=np.float64)
    x0_prev, h_prev = None, None
    for i in reversed(range(plan.n_steps)):
        al, sg = float(plan.alpha[i]), float(plan.sigma[i])
        an, sn = plan.nxt(i)
        eps = np.asarray(model(x, int(plan.timestep_map[i]), float(plan.cfk[i])), dtype=np.float64)
        x0 = np.clip((x - sg * eps) / al, -1.0, 1.0)
        if i == 0:
            x = x0
        elif plan.kind == "ddim":
            x = an * x0 + sn * (x - al * x0) / sg
        else:
            h = plan.lam[i - 1] - plan.lam[i]
            if x0_prev is None:
                D = x0
            else:
                w = 0.5 * h / h_prev
                D = (1.0 + w) * x0 - w * x0_prev
            x = (sn / sg) * x - an * (math.exp(-h) - 1.0) * D
            h_prev = h
        x0_prev = x0
    return x


# ---------------------------------------------------------------------------------------------- one step of the device kernel
MEL_MIN32 = np.float32(-11.512925148010254)
MEL_SCALE32 = np.float32(2.3143386840820312) - MEL_MIN32  # the f32 difference the engine passes to its kernels
TINY = 4 * 2.0 ** -149                                    # products that underflow round to a subnormal: absolute, not relative
UNIT_ROUNDOFF = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}


def update_reference(x, eps_c, eps_u, hist, step):
    """fp64 on the kernel's f32 inputs.  x, eps_c, eps_u (or None), hist: float arrays [S, C]; step: dict of the record's f32 values
    (cfk, sqrt_recip, sqrt_recipm1, a, b, c).  The guidance weight 1 + cfk is the f32 sum the kernel forms once per step: a coefficient
    like the others.  hist is not touched when c == 0 (it may hold NaN).  -> dict of x0, xn, mel and their element-wise bounds."""
    f = lambda v: np.asarray(v, dtype=np.float64)
    x, ec = f(x), f(eps_c)
    cfk, sr, srm1, a, b, c = (float(np.float32(step[k])) for k in ("cfk", "sqrt_recip", "sqrt_recipm1", "a", "b", "c"))
    g2, g3 = gamma(2), gamma(3)
    if eps_u is not None:
        # guidance blend: the product cfk eu and the fused multiply-add - 2 roundings
        w1 = float(np.float32(1.0) + np.float32(cfk))
        eu = f(eps_u)
        eps = w1 * ec - cfk * eu
        d_eps = g2 * (np.abs(w1 * ec) + np.abs(cfk * eu)) + TINY
    else:
        eps, d_eps = ec, np.zeros_like(ec)
    # x0: a product and a fused multiply-add - 2 roundings - on top of what eps carries; the clamp is 1-Lipschitz
    raw = sr * x - srm1 * eps
    d_x0 = g2 * (np.abs(sr * x) + abs(srm1) * (np.abs(eps) + d_eps)) + abs(srm1) * d_eps + TINY
    x0 = np.clip(raw, -1.0, 1.0)
    # update: a x, fma(b, x0, .), fma(c, x0', .) - 3 roundings - on top of what x0 carries
    xn = a * x + b * x0
    mag = np.abs(a * x) + abs(b) * (np.abs(x0) + d_x0)
    if c != 0.0:
        h = f(hist)
        xn = xn + c * h
        mag = mag + np.abs(c * h)
    d_xn = g3 * mag + abs(b) * d_x0 + TINY
    # mel = ((xn + 1) * 0.5) * scale + shift: the sum, the (exact) halving, then a product and a sum or one fused multiply-add
    sc, sh = float(MEL_SCALE32), float(MEL_MIN32)
    mel = (xn + 1.0) * 0.5 * sc + sh
    d_mel = 0.5 * sc * d_xn * (1.0 + g3) + g3 * ((np.abs(xn) + 1.0) * 0.5 * sc + abs(sh))
    return dict(x0=x0, d_x0=d_x0, xn=xn, d_xn=d_xn, mel=mel, d_mel=d_mel)


def operand_bound(ref, name):
    """Bound of the 16-bit (or f32) operand copy of xn: the f32 result's bound plus one rounding to the operand type (fp16 values below
    its normal range round to a multiple of 2^-24)."""
    u = UNIT_ROUNDOFF[name]
    return ref["d_xn"] + u * (np.abs(ref["xn"]) + ref["d_xn"]) + (2.0 ** -25 if name == "f16" else 0.0)
