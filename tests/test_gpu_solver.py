"""Device checks of the deterministic diffusion solvers (include/tortoise_mi355x_solver.h): the update kernel alone against fp64 with
element-wise bounds from the operation count (tests/solver_reference.py), the whole loop against the oracle's denoiser at the bound the
p-loop test carries, graph capture and reuse beside the p sampler's, history isolation between runs, one- and two-step plans, padded
batches (solve_many) and tts(sampler=...) end to end.  The host side is tests/test_solver_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import make_golden as G
from oracle import tortoise_oracle as O
from tests import solver_reference as R
from tests.gpu_util import quantize_sd, rel_err, report
from tortoise_tts_amd import engine as E
from tortoise_tts_amd import stages
from tortoise_tts_amd import weights as W
from tortoise_tts_amd.config import ARConfig, CLVPConfig, DiffusionConfig, VocoderConfig
from tortoise_tts_amd.schedule import Schedule
from tortoise_tts_amd.solver import SolverPlan

pytestmark = pytest.mark.gpu

# the table of tests/test_gpu_parity_r3.py (tests/gpu_util.py): name, engine dtype, torch dtype, operand tolerance (rel-L2)
DTYPES = [("bf16", E.TT_BF16, torch.bfloat16, 2.5e-2), ("f16", E.TT_F16, torch.float16, 4e-3)]
SOLVERS = [("ddim", "uniform"), ("dpm++2m", "logsnr")]
DEV = "cuda"


def ref_plan(plan):
    return R.RefPlan(plan.kind, plan.requested_steps, plan.spacing, cond_free=plan.cond_free, cond_free_k=plan.cond_free_k)


def oracle_model(sd, cfg, emb, cond_free):
    """model(x, t, cfk) of solver_reference.solve_loop on the oracle's denoiser: the guided eps of x f64 [1, 100, S]."""
    def model(x, t, cfk):
        xt, ts = torch.from_numpy(x).float(), torch.full((1,), t, dtype=torch.long)
        eps = O.diffusion_forward(sd, cfg, xt, ts, emb, False)[:, :100].double()
        if cond_free:
            eps = (1 + cfk) * eps - cfk * O.diffusion_forward(sd, cfg, xt, ts, emb, True)[:, :100].double()
        return eps.numpy()
    return model


def reference_mel(plan, sd, cfg, emb, x):
    out = R.solve_loop(ref_plan(plan), oracle_model(sd, cfg, emb, plan.cond_free), x.double().numpy())
    return O.denormalize_tacotron_mel(torch.from_numpy(out).float())


# ------------------------------------------------------------------------------------------------ the update kernel alone
def run_update(name, dt, tdt, S, has_uncond, step, x, model, hist, ld, cpad=128):
    """-> (x', hist', x_t [rows, ld, cpad] as f32 with sentinel 7 where nothing may be written, mel, guard count)."""
    lib = E.init()
    C_ = 100
    xd, md, hd = x.to(DEV).contiguous(), model.to(DEV).contiguous(), hist.to(DEV).contiguous()
    rows = 2 if has_uncond else 1
    x_t = torch.full((rows, ld, cpad), 7.0, device=DEV, dtype=tdt)
    mel = torch.zeros(C_, S, device=DEV)
    guard = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = E.SolverStep(0, *[float(np.float32(step[k])) for k in ("cfk", "sqrt_recip", "sqrt_recipm1", "a", "b", "c")])
    torch.cuda.synchronize()
    E.check(lib.tt_op_solver_update(dt, E.ptr(xd), E.ptr(md), ld, int(has_uncond), E.ptr(hd), C.byref(st), S, C_, cpad, E.ptr(x_t), E.ptr(mel),
                                    E.ptr(guard), E.stream_ptr()))
    torch.cuda.synchronize()
    return xd.cpu(), hd.cpu(), x_t.float().cpu(), mel.cpu(), int(guard[0])


@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("S", [1, 63, 130])
def test_update_kernel_against_fp64_elementwise(S, has_uncond):
    g = torch.Generator().manual_seed(100 + S)
    C_, ld = 100, S + (3 if S == 63 else 0)  # (one shape with rows between the two blocks)
    base = dict(cfk=1.3, sqrt_recip=1.7, sqrt_recipm1=1.4, a=0.61, b=0.83)
    x = torch.randn(S, C_, generator=g)
    model = torch.randn(2 if has_uncond else 1, ld, 2 * C_, generator=g)
    model[..., C_:] = float("nan")  # the learned-variance half is never read
    good_hist = torch.randn(S, C_, generator=g).clamp(-1, 1)
    # scale x and eps together so that about a quarter of the x0 values clamp (x0 is linear in both)
    ec = model[0, :S, :C_].double()
    eps = (np.float32(1) + np.float32(1.3)).item() * ec - 1.3 * model[1, :S, :C_].double() if has_uncond else ec
    raw = 1.7 * x.double() - 1.4 * eps
    scale = float(1.0 / raw.abs().flatten().quantile(0.75))
    x, model = x * scale, model * scale
    for c, hist in ((0.0, torch.full((S, C_), float("nan"))), (-0.37, good_hist)):
        step = dict(base, c=c)
        ref = R.update_reference(x.numpy(), model[0, :S, :C_].numpy(), model[1, :S, :C_].numpy() if has_uncond else None, hist.numpy(), step)
        clamped = float(np.mean(np.abs(ref["x0"]) == 1.0))
        assert 0.12 <= clamped <= 0.4, clamped
        for name, dt, tdt, _ in DTYPES + [("f32", E.TT_F32, torch.float32, 0.0)]:
            xn, h, x_t, mel, guard = run_update(name, dt, tdt, S, has_uncond, step, x, model, hist, ld)
            tag = f"S={S} uncond={has_uncond} c={c} {name}"
            assert guard == 0 and torch.isfinite(xn).all() and torch.isfinite(h).all() and torch.isfinite(mel).all(), tag
            for what, got, want, bound in (("x", xn, ref["xn"], ref["d_xn"]), ("x0", h, ref["x0"], ref["d_x0"]), ("mel", mel.t(), ref["mel"], ref["d_mel"]),
                                           ("x_t", x_t[0, :S, :C_], ref["xn"], R.operand_bound(ref, name))):
                err = np.abs(got.double().numpy() - want)
                worst = float(np.max(err / bound))
                if name == "f32" or what == "x_t":
                    print(f"[solver] update kernel {tag} {what}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
                assert np.all(err <= bound), f"{tag} {what}: err / bound up to {worst:.3f}"
            assert torch.count_nonzero(x_t[:, :S, C_:]) == 0, tag                       # pad columns are zeros
            assert torch.all(x_t[:, S:] == 7.0), tag                                    # rows past S are not touched
            if has_uncond:
                assert torch.equal(x_t[0, :S], x_t[1, :S]), tag                         # both batch rows read the same state
    # a non-finite eps (either row) is counted: the clamp would hide it
    for row in range(2 if has_uncond else 1):
        bad = model.clone()
        bad[row, S - 1, 7] = float("inf") if row == 0 else float("nan")
        assert run_update("bf16", E.TT_BF16, torch.bfloat16, S, has_uncond, dict(base, c=0.0), x, bad, good_hist, ld)[4] >= 1


# ------------------------------------------------------------------------------------------------ the whole loop
@pytest.mark.parametrize("cond_free", [True, False])
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@torch.no_grad()
def test_solver_loops_against_the_oracles_denoiser(name, dt, tdt, tol, cond_free):
    """N = 12: st.solve() vs the fp64 textbook loop over the oracle's denoiser (weights rounded to the operand type on both sides), at the
    bound the p-loop test carries at the same N; the p loop on the same inputs beside them.  Measured on MI355X: see
    profiles/r19_solver.txt."""
    cfg = DiffusionConfig(**G.DIFF_CFG)
    sd = quantize_sd(W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=G.DIFF_SEED), tdt)
    S, latents, cond, x, _ = G.diff_inputs(cfg)
    N = 12
    step_noise = torch.randn(N, 1, 100, S, generator=torch.Generator().manual_seed(77))
    emb = O.diffusion_timestep_independent(sd, cfg, latents, cond, S)
    st = stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=128, max_codes=64, max_steps=16)
    st.condition(latents, cond, S)
    got = {}
    for kind, spacing in SOLVERS:
        plan = SolverPlan(kind, N, spacing, cond_free=cond_free)
        assert plan.n_steps == N
        got[kind] = st.solve(plan, x).cpu()
        report(f"diffusion {kind}/{spacing} cond_free={cond_free} ({N} steps) {name} vs fp64 loop over the oracle", got[kind],
               reference_mel(plan, sd, cfg, emb, x), tol * 2)
    got["p"] = st.sample(Schedule(N, 4000, cond_free, 2.0), x, step_noise).cpu()
    want = O.denormalize_tacotron_mel(O.p_sample_loop(sd, cfg, O.Schedule(N, 4000, cond_free, 2.0), emb, x.clone(), step_noise))
    report(f"diffusion p_sample_loop cond_free={cond_free} ({N} steps) {name} vs oracle", got["p"], want, tol * 2)
    assert st.guard() == 0
    st.close()
    for a, b in (("ddim", "dpm++2m"), ("ddim", "p"), ("dpm++2m", "p")):
        assert rel_err(got[a], got[b]) > 1e-3, (a, b)


# name, engine dtype, torch dtype of the weights' rounding, bar of ONE denoiser evaluation (eps rel-L2): the operand tolerances of the table
# above, and the fp32 verification mode's 1e-4 (tests/test_gpu_f32.py)
EVAL_BARS = [("fp32 mode", E.TT_F32, None, 1e-4)] + DTYPES


@pytest.mark.parametrize("name,dt,tdt,bar", EVAL_BARS)
@pytest.mark.parametrize("N", [1, 2])
@torch.no_grad()
def test_one_and_two_step_plans(N, name, dt, tdt, bar):
    """The terminal row alone, and the first-order first step in front of it (both run eagerly: a step graph is kept from three steps on;
    that the eager and the replayed step agree bit for bit is test_solver_graph_is_kept_beside_the_p_samplers).
    Every plan of two steps, and the log-SNR plan of one, starts at t = 3999, where x0 = x / alpha - (sigma / alpha) eps multiplies any
    error of eps by sigma / alpha = 153: 16-bit operand noise alone moves the clamped result by a few percent there (measured: bf16, one
    step, rel-L2 5.4e-2 - the operands' error times the gain, not the update).  So the bound is the bar of ONE denoiser evaluation in the
    mode at hand (eps rel-L2: the operand tolerance, or the fp32 verification mode's 1e-4) carried through the update: step i hands an
    eps error to the state multiplied by |b_i| sigma_i / alpha_i, the clamp is 1-Lipschitz, and what follows (here at most the terminal
    step, x0 = x / alpha_0 with alpha_0 = 0.99999) passes a state error on unamplified.  In mel units, relative:
    bar * max(1, sum_i |b_i| sigma_i / alpha_i) * (mel range / 2) * rms(eps) / rms(mel), with the largest eps the reference loop met.
    The fp32 mode is the sharp one (2.5e-2 at gain 153, 2e-4 at gain 1); the 16-bit rows are sharp only for the one-step uniform plan
    (t = 0, gain 1) and otherwise show that the eager 16-bit path runs and stays inside what its operands allow."""
    cfg = DiffusionConfig(**G.DIFF_CFG)
    sd = W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=G.DIFF_SEED)
    if tdt is not None:
        sd = quantize_sd(sd, tdt)
    S, latents, cond, x, _ = G.diff_inputs(cfg)
    emb = O.diffusion_timestep_independent(sd, cfg, latents, cond, S)
    st = stages.DiffusionStage(sd, cfg, dtype=dt, max_seq=128, max_codes=64, max_steps=16)
    st.condition(latents, cond, S)
    for kind, spacing in SOLVERS:
        plan = SolverPlan(kind, N, spacing)
        assert plan.n_steps == N
        model, eps_rms = oracle_model(sd, cfg, emb, True), []

        def recording(x_, t, cfk):
            eps = model(x_, t, cfk)
            eps_rms.append(float(np.sqrt(np.mean(eps ** 2))))
            return eps

        want = O.denormalize_tacotron_mel(torch.from_numpy(R.solve_loop(ref_plan(plan), recording, x.double().numpy())).float())
        gain = max(1.0, float(np.sum(np.abs(plan.b) * plan.sqrt_recipm1)))
        bound = bar * gain * 0.5 * float(R.MEL_SCALE32) * max(eps_rms) / float(want.pow(2).mean().sqrt())
        got = st.solve(plan, x)
        assert torch.isfinite(got).all()
        report(f"diffusion {kind}/{spacing} ({N} steps, error gain {gain:.1f}) {name} vs fp64 loop over the oracle", got, want, bound)
    assert st.solve_stat(0) == 0  # nothing was captured: the eager branch
    st.close()


# ------------------------------------------------------------------------------------------------ capture, history
@pytest.fixture(scope="module")
def small():
    cfg = DiffusionConfig(**G.DIFF_CFG)
    sd = W.synthetic_state_dict(W.diffusion_manifest(cfg), seed=G.DIFF_SEED)
    return (cfg, sd) + tuple(G.diff_inputs(cfg))


@torch.no_grad()
def test_solver_graph_is_kept_beside_the_p_samplers(small):
    cfg, sd, S, latents, cond, x, _ = small
    N = 6
    plan, sched = SolverPlan("dpm++2m", N), Schedule(N, 4000, True, 2.0)
    noise = torch.randn(N, 1, 100, S, generator=torch.Generator().manual_seed(3))
    st = stages.DiffusionStage(sd, cfg, max_seq=128, max_codes=64, max_steps=16)
    st.condition(latents, cond, S)
    assert (st.stat(0), st.solve_stat(0)) == (0, 0) and st.solve_stat(1) == -1
    first = st.solve(plan, x).clone()
    assert (st.stat(0), st.solve_stat(0)) == (0, 1)
    assert torch.equal(st.solve(plan, x), first) and st.solve_stat(0) == 1  # the same shape again: nothing is captured
    p_first = st.sample(sched, x, noise).clone()
    assert torch.equal(st.solve(plan, x), first)
    assert torch.equal(st.sample(sched, x, noise), p_first)
    assert torch.equal(st.solve(SolverPlan("ddim", N), x * 0.5), st.solve(SolverPlan("ddim", N), x * 0.5))  # other records, the same step graph
    assert (st.stat(0), st.solve_stat(0)) == (1, 1)
    E.load_library().tt_graph_replay(0)
    try:
        eager = st.solve(plan, x).clone()
    finally:
        E.load_library().tt_graph_replay(1)
    assert torch.equal(eager, first) and st.solve_stat(0) == 1
    st.close()


@torch.no_grad()
def test_a_run_does_not_see_the_history_of_the_run_before(small):
    cfg, sd, S, latents, cond, x, _ = small
    plan = SolverPlan("dpm++2m", 5)
    xb = torch.randn(1, 100, S, generator=torch.Generator().manual_seed(9))
    outs = []
    for runs in ((x * 3.0, xb), (xb,)):
        st = stages.DiffusionStage(sd, cfg, max_seq=128, max_codes=64, max_steps=16)
        st.condition(latents, cond, S)
        for x_T in runs:
            out = st.solve(plan, x_T).clone()
        outs.append(out)
        st.close()
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ padded batches
@pytest.mark.parametrize("kind,spacing", SOLVERS)
@torch.no_grad()
def test_solve_many_treats_every_utterance_as_if_it_ran_alone(small, kind, spacing):
    cfg, sd = small[:2]
    g = torch.Generator().manual_seed(5)
    items = [(torch.randn(1, M, cfg.in_latent_channels, generator=g), torch.randn(1, 2 * cfg.model_channels, generator=g) * 0.5, S,
              torch.randn(1, 100, S, generator=g), None) for M, S in ((3, 5), (30, 64), (44, 97))]
    plan = SolverPlan(kind, 6, spacing)
    st = stages.DiffusionStage(sd, cfg, max_seq=128, max_codes=64, max_steps=16, max_batch=4)
    alone = []
    for lat, cond, S, x, _ in items:
        st.condition(lat, cond, S)
        alone.append(st.solve(plan, x).clone())
    many = st.solve_many(plan, items)
    with pytest.raises(ValueError, match="condition"):  # the handle holds a batch now
        st.solve(plan, items[0][3])
    again = st.solve_many(plan, [items[2], items[0], items[1]])
    for u, (a, b) in enumerate(zip(many, alone)):
        assert a.shape == b.shape == (1, 100, items[u][2]) and torch.isfinite(a).all()
        # (the operand tolerance of tests/test_gpu_parity_r3.py's sample_many test: an utterance inside a longer batch may get another
        # attention kernel than alone)
        report(f"solve_many {kind} utterance {u} S={items[u][2]} vs solve() alone", a, b, 2.5e-2)
    for u, v in ((0, 2), (1, 0), (2, 1)):
        report(f"solve_many {kind} utterance {v} in another order of lengths vs solve() alone", again[u], alone[v], 2.5e-2)
    assert st.guard() == 0
    st.close()


# ------------------------------------------------------------------------------------------------ tts()
@torch.no_grad()
def test_tts_with_a_solver_end_to_end():
    from tortoise_tts_amd.api import TextToSpeech, calm_trim_length
    ar, clvp, diff = ARConfig(**G.AR_CFG), CLVPConfig(**G.CLVP_CFG), DiffusionConfig(**G.DIFF_CFG)
    sds = {"autoregressive": W.suppress_stop_token(W.synthetic_state_dict(W.ar_manifest(ar), seed=G.AR_SEED), ar),
           "clvp": W.synthetic_state_dict(W.clvp_manifest(clvp), seed=G.CLVP_SEED),
           "diffusion": W.synthetic_state_dict(W.diffusion_manifest(diff), seed=G.DIFF_SEED),
           "vocoder": W.fold_weight_norm(W.synthetic_state_dict(W.vocoder_manifest(VocoderConfig()), seed=G.VOC_SEED))}
    tts = TextToSpeech(state_dicts=sds, configs={"ar": ar, "clvp": clvp, "diffusion": diff}, max_candidates=8, max_mel_tokens=32)
    g = torch.Generator().manual_seed(2)
    lat = (torch.randn(1, ar.model_dim, generator=g) * 0.5, torch.randn(1, 2 * diff.model_channels, generator=g) * 0.5)
    kw = dict(conditioning_latents=lat, num_autoregressive_samples=8, diffusion_iterations=8, max_mel_tokens=24, use_deterministic_seed=3, verbose=False)
    text = list(range(10, 25))
    wav = tts.tts(text, sampler="dpm++2m", **kw)
    S = calm_trim_length(tts.last_best_codes[0]) * 4 * 24000 // 22050
    assert wav.shape == (1, 1, S * 256) and torch.isfinite(wav).all() and wav.abs().max() <= 1.0
    assert tts.diffusion.solve_stat(0) == 1 and tts.diffusion.stat(0) == 0
    assert torch.equal(tts.tts(text, sampler="dpm++2m", **kw), wav) and tts.diffusion.solve_stat(0) == 1
    p = [tts.tts(text, **kw), tts.tts(text, sampler=None, **kw), tts.tts(text, sampler="p", **kw)]
    assert torch.equal(p[0], p[1]) and torch.equal(p[0], p[2]) and tts.diffusion.stat(0) == 1
    assert p[0].shape == wav.shape and not torch.equal(p[0], wav)
    assert not tts.demotions
