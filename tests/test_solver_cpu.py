"""CPU checks of the deterministic diffusion solvers (tortoise_tts_amd/solver.py, include/tortoise_mi355x_solver.h): the coefficient tables
against an independent fp64 derivation (tests/solver_reference.py), the solvers on closed-form diffusion problems (a point mass, Gaussian
data) with the orders of convergence they must show, the log-SNR spacing, the option parser, the flow of tts() / tts_many() through the
oracle-backed stand-ins, and the new header's symbols.  The device side is tests/test_gpu_solver.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fake_stages
from tests import solver_reference as R
from tests.test_api_flow_cpu import VOCAB, small_setup, voice_latents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = list(range(10, 31))
KW = dict(num_autoregressive_samples=4, diffusion_iterations=3, max_mel_tokens=16, use_deterministic_seed=5, verbose=False)
CASES = [(kind, spacing) for kind in ("ddim", "dpm++2m") for spacing in ("uniform", "logsnr")]


def product_loop(plan, model, x_T):
    """x_next = a x + b x0 + c x0_prev over the product's tables, fp64: what the device runs, without its roundings."""
    x = np.asarray(x_T, dtype=np.float64)
    prev = np.zeros_like(x)
    for i in reversed(range(plan.n_steps)):
        eps = model(x, int(plan.timestep_map[i]), float(plan.cfk[i]))
        x0 = np.clip(plan.sqrt_recip[i] * x - plan.sqrt_recipm1[i] * eps, -1.0, 1.0)
        x = plan.a[i] * x + plan.b[i] * x0 + plan.c[i] * prev
        prev = x0
    return x


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("kind,spacing", CASES)
@pytest.mark.parametrize("N", [1, 2, 5, 12, 30])
def test_tables_equal_the_independent_derivation(kind, spacing, N):
    from tortoise_tts_amd.solver import SolverPlan
    plan, ref = SolverPlan(kind, N, spacing), R.RefPlan(kind, N, spacing)
    assert plan.n_steps == ref.n_steps and np.array_equal(plan.timestep_map, ref.timestep_map)
    a, b, c = ref.abc()
    close = lambda got, want: np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    assert close(plan.a, a) and close(plan.b, b) and close(plan.c, c)
    assert close(plan.sqrt_recip, 1.0 / ref.alpha) and close(plan.sqrt_recipm1, ref.sigma / ref.alpha) and close(plan.cfk, ref.cfk)
    assert (plan.a[0], plan.b[0], plan.c[0]) == (0.0, 1.0, 0.0)  # terminal: the clamped x0
    assert plan.c[-1] == 0.0                                      # the first step run has no history
    if kind == "ddim":
        assert not plan.c.any()
    elif plan.n_steps >= 3:
        assert plan.c[1:-1].all()


def test_default_spacing_and_the_p_samplers_timesteps():
    from tortoise_tts_amd.schedule import Schedule
    from tortoise_tts_amd.solver import SolverPlan
    assert SolverPlan("ddim", 12).spacing == "uniform" and SolverPlan("dpm++2m", 12).spacing == "logsnr"
    assert np.array_equal(SolverPlan("ddim", 12).timestep_map, Schedule(12).timestep_map)
    p = SolverPlan("dpm++2m", 7, cond_free=False, cond_free_k=3.0)
    assert p.cond_free is False and np.allclose(p.cfk, 3.0 * (1 - np.arange(7) / 7))


# ------------------------------------------------------------------------------------------------ closed-form problems
def schedule_of(t):
    abar = R.alphas_cumprod()[t]
    return abar, np.sqrt(abar), np.sqrt(1.0 - abar)


@pytest.mark.parametrize("kind,spacing", CASES)
@pytest.mark.parametrize("N", [2, 5, 30])
def test_point_mass_is_recovered_exactly(kind, spacing, N):
    """Data concentrated on m: eps(x, t) = (x - alpha_t m) / sigma_t makes every x0 equal m, so any consistent solver returns m."""
    from tortoise_tts_amd.solver import SolverPlan
    m = 0.37

    def model(x, t, cfk):
        _, al, sg = schedule_of(t)
        return (x - al * m) / sg

    x_T = np.random.default_rng(1).standard_normal(64)
    for loop, plan in ((product_loop, SolverPlan(kind, N, spacing)), (R.solve_loop, R.RefPlan(kind, N, spacing))):
        assert np.max(np.abs(loop(plan, model, x_T) - m)) <= 1e-12


def gaussian_error(loop, plan):
    """Data N(0, 0.25^2): eps(x, t) = sigma_t x / (abar_t 0.0625 + sigma_t^2); the probability-flow ODE maps x_T to
    x_T 0.25 / sqrt(abar_T 0.0625 + sigma_T^2).  -> relative max error of the solver."""
    def model(x, t, cfk):
        abar, _, sg = schedule_of(t)
        return sg * x / (abar * 0.0625 + sg * sg)

    x_T = np.random.default_rng(0).standard_normal(1000)
    abar, _, sg = schedule_of(int(plan.timestep_map[-1]))
    exact = x_T * 0.25 / np.sqrt(abar * 0.0625 + sg * sg)
    assert np.max(np.abs(exact)) < 1.0  # the clamp stays inactive
    return float(np.max(np.abs(loop(plan, model, x_T) - exact)) / np.max(np.abs(exact)))


def test_orders_of_convergence_on_gaussian_data():
    from tortoise_tts_amd.solver import SolverPlan
    dpm = {N: gaussian_error(product_loop, SolverPlan("dpm++2m", N, "logsnr")) for N in (10, 20, 40)}
    ddim = {N: gaussian_error(product_loop, SolverPlan("ddim", N, "uniform")) for N in (20, 40, 80)}
    print(f"[solver] gaussian data, relative max error: dpm++2m/logsnr {dpm}  ddim/uniform {ddim}")
    assert dpm[40] <= dpm[20] / 3      # second order in the log-SNR step
    assert ddim[40] <= ddim[20] / 1.7  # first order
    assert dpm[20] < ddim[80]
    # and the product's linear form is the textbook algorithm
    for kind, spacing, N in (("dpm++2m", "logsnr", 20), ("ddim", "uniform", 20)):
        assert abs(gaussian_error(R.solve_loop, R.RefPlan(kind, N, spacing)) - gaussian_error(product_loop, SolverPlan(kind, N, spacing))) < 1e-10


# ------------------------------------------------------------------------------------------------ spacing
def test_logsnr_spacing():
    from tortoise_tts_amd.solver import SolverPlan
    for N in (10, 15, 20, 30, 40):
        p = SolverPlan("dpm++2m", N, "logsnr")
        assert p.n_steps == N == len(set(p.timestep_map.tolist()))
        assert np.all(np.diff(p.timestep_map) > 0) and p.timestep_map[0] == 0 and p.timestep_map[-1] == 3999
    p = SolverPlan("dpm++2m", 80, "logsnr")
    assert p.n_steps < 80 and p.n_steps == len(p.timestep_map) == len(p.a) == R.RefPlan("dpm++2m", 80, "logsnr").n_steps
    assert p.requested_steps == 80 and np.all(np.diff(p.timestep_map) > 0) and p.timestep_map[0] == 0 and p.timestep_map[-1] == 3999


# ------------------------------------------------------------------------------------------------ options
def test_option_parser():
    from tortoise_tts_amd import solver
    for kw in ({}, {"sampler": None}, {"sampler": "p"}):
        kw = dict(kw, top_k=3)
        assert solver.sampler_options(kw, 30) is None and kw == {"top_k": 3}
    kw = {"sampler": "dpm++2m", "sampler_spacing": "uniform", "top_k": 3}
    p = solver.sampler_options(kw, 30, cond_free=False, cond_free_k=1.5)
    assert kw == {"top_k": 3} and (p.kind, p.spacing, p.n_steps, p.cond_free, p.cond_free_k) == ("dpm++2m", "uniform", 30, False, 1.5)
    assert solver.sampler_options({"sampler": "ddim"}, 7).spacing == "uniform"
    for bad in ({"sampler": "euler"}, {"sampler": "ddim", "sampler_spacing": "karras"}, {"sampler": "p", "sampler_spacing": "uniform"},
                {"sampler_spacing": "logsnr"}, {"sampler": "ddim", "diffusion_iterations": 0}):
        with pytest.raises(ValueError):
            solver.sampler_options(dict(bad), bad.get("diffusion_iterations", 30))


def test_fast_api_entries_refuse(monkeypatch):
    """The HiFi-GAN path has no diffusion stage: every entry that refuses speaking_rate refuses the two kwargs too, before any work."""
    from tortoise_tts_amd import api_fast, solver
    for kw in ({"sampler": "ddim"}, {"sampler_spacing": "logsnr"}, {"sampler": None}):
        with pytest.raises(ValueError, match="no diffusion stage"):
            solver.refuse_streaming(kw, "tts_stream")
    solver.refuse_streaming({"top_k": 5}, "tts_stream")
    t = object.__new__(api_fast.TextToSpeech)  # (the checks run before the instance is touched)
    with pytest.raises(ValueError, match="no diffusion stage"):
        next(t.tts_stream("x", sampler="ddim"))
    with pytest.raises(ValueError, match="no diffusion stage"):
        t.open_stream("x", sampler_spacing="uniform")
    with pytest.raises(ValueError, match="no diffusion stage"):
        next(iter(t.tts_stream_many(["x"], sampler="dpm++2m")))


# ------------------------------------------------------------------------------------------------ flow
class SolvingDiffusionStage(fake_stages.FakeDiffusionStage):
    """The stand-in diffusion stage with solve / solve_many on the oracle's denoiser, recording every stage call."""
    log = []

    def _model(self, plan):
        from oracle import tortoise_oracle as O

        def model(x, t, cfk):
            xt, ts = torch.from_numpy(x).float(), torch.full((1,), t, dtype=torch.long)
            ec = O.diffusion_forward(self.sd, self.cfg, xt, ts, self.emb, False)[:, :100].double()
            if plan.cond_free:
                eu = O.diffusion_forward(self.sd, self.cfg, xt, ts, self.emb, True)[:, :100].double()
                ec = (1 + cfk) * ec - cfk * eu
            return ec.numpy()
        return model

    def condition(self, latents, cond_latent, S):
        SolvingDiffusionStage.log.append(("condition", S))
        return super().condition(latents, cond_latent, S)

    def sample(self, sched, x_T, step_noise):
        SolvingDiffusionStage.log.append(("sample", sched.num_timesteps, tuple(step_noise.shape)))
        return super().sample(sched, x_T, step_noise)

    def sample_many(self, sched, items):
        SolvingDiffusionStage.log.append(("sample_many", len(items)))
        return super().sample_many(sched, items)

    def sample_split(self, *a, **k):
        SolvingDiffusionStage.log.append(("sample_split",))
        raise AssertionError("a solver's winner renders unsplit")

    def solve(self, plan, x_T):
        from oracle import tortoise_oracle as O
        SolvingDiffusionStage.log.append(("solve", plan.kind, plan.n_steps))
        ref = R.RefPlan(plan.kind, plan.requested_steps, plan.spacing, cond_free=plan.cond_free, cond_free_k=plan.cond_free_k)
        return O.denormalize_tacotron_mel(torch.from_numpy(R.solve_loop(ref, self._model(plan), x_T.double().cpu().numpy())).float())

    def solve_many(self, plan, items):
        assert 1 <= len(items) <= self.max_batch
        SolvingDiffusionStage.log.append(("solve_many", len(items), [it[4] for it in items]))
        out = []
        for lat, cond, S, x_T, _ in items:
            fake_stages.FakeDiffusionStage.condition(self, lat, cond, S)
            log, SolvingDiffusionStage.log = SolvingDiffusionStage.log, []
            out.append(self.solve(plan, x_T))
            SolvingDiffusionStage.log = log
        return out


def install(monkeypatch):
    fake_stages.install(monkeypatch)
    from tortoise_tts_amd import api
    monkeypatch.setattr(api.stages, "DiffusionStage", SolvingDiffusionStage)
    SolvingDiffusionStage.log = []
    return api


def make(api, **kw):
    sds, cfgs = small_setup()
    t = api.TextToSpeech(models_dir="/nonexistent", tokenizer_vocab_file=VOCAB, tokenizer_basic=True, state_dicts=sds, configs=cfgs,
                         max_candidates=8, max_mel_tokens=40, **kw)
    return t, voice_latents(cfgs)


def calls(kind=None):
    return [c for c in SolvingDiffusionStage.log if kind is None or c[0] == kind]


@torch.no_grad()
def test_tts_with_a_solver_calls_solve_and_draws_no_step_noise(monkeypatch):
    api = install(monkeypatch)
    t, lat = make(api)
    drawn = []
    randn = torch.randn
    monkeypatch.setattr(api.torch, "randn", lambda *shape, **kw: (drawn.append(shape), randn(*shape, **kw))[1])
    wav = t.tts(TEXT, conditioning_latents=lat, sampler="dpm++2m", **KW)
    assert torch.is_tensor(wav) and wav.dim() == 3 and torch.isfinite(wav).all()
    assert calls("solve") == [("solve", "dpm++2m", 3)] and not calls("sample") and not calls("sample_many") and not calls("sample_split")
    assert [len(s) for s in drawn] == [3, 3], drawn  # x_T [1, 100, S] then z [1, 64, S + 10]: no [N, 1, 100, S] tensor
    S = drawn[0][2]
    assert drawn[0] == (1, 100, S) and drawn[1][2] == S + 10
    # a supplied step_noise is ignored, x_T and z are honoured
    g = torch.Generator().manual_seed(1)
    noise = {"x_T": torch.randn(1, 100, S, generator=g), "z": torch.randn(1, 64, S + 10, generator=g)}
    a = t.tts(TEXT, conditioning_latents=lat, sampler="dpm++2m", noise_override=dict(noise), **KW)
    b = t.tts(TEXT, conditioning_latents=lat, sampler="dpm++2m", noise_override=dict(noise, step_noise=torch.full((3, 1, 100, S), float("nan"))), **KW)
    assert torch.equal(a, b) and not torch.equal(a, wav)
    # a split instance (what two ranks set up; this is its rank 0) renders the solver's winner unsplit; ddim with sampler_spacing: another clip
    t.split_diffusion = True
    SolvingDiffusionStage.log = []
    other = t.tts(TEXT, conditioning_latents=lat, sampler="ddim", sampler_spacing="logsnr", **KW)
    assert other.shape == wav.shape and not torch.equal(other, wav)
    assert SolvingDiffusionStage.log == [("condition", S), ("solve", "ddim", 3)]
    # tts_with_preset hands the caller's kwargs to tts() beside the preset's diffusion_iterations, the solver's N
    seen = []
    monkeypatch.setattr(t, "tts", lambda text, **kw: seen.append(kw))
    t.tts_with_preset(TEXT, preset="ultra_fast", sampler="ddim", sampler_spacing="uniform")
    assert seen[0]["sampler"] == "ddim" and seen[0]["sampler_spacing"] == "uniform" and seen[0]["diffusion_iterations"] == 30


@torch.no_grad()
def test_default_none_and_p_make_identical_stage_calls(monkeypatch):
    api = install(monkeypatch)
    t, lat = make(api)
    runs = []
    for kw in ({}, {"sampler": None}, {"sampler": "p"}):
        SolvingDiffusionStage.log = []
        wav = t.tts(TEXT, conditioning_latents=lat, **KW, **kw)
        runs.append((wav, list(SolvingDiffusionStage.log)))
    assert all(torch.equal(w, runs[0][0]) and log == runs[0][1] for w, log in runs)
    assert [c[0] for c in runs[0][1]] == ["condition", "sample"] and runs[0][1][1][1] == 3
    with pytest.raises(ValueError, match="sampler_spacing"):
        t.tts(TEXT, conditioning_latents=lat, sampler="p", sampler_spacing="uniform", **KW)
    with pytest.raises(ValueError, match="unknown sampler"):
        t.tts(TEXT, conditioning_latents=lat, sampler="heun", **KW)


@torch.no_grad()
def test_winner_batch_renders_the_winners_in_one_solve_many(monkeypatch):
    api = install(monkeypatch)
    serial, lat = make(api)
    want = serial.tts(TEXT, conditioning_latents=lat, k=3, sampler="dpm++2m", **KW)
    assert len(calls("solve")) == 3 and not calls("solve_many")
    batched, _ = make(api, winner_batch=3)
    SolvingDiffusionStage.log = []
    got = batched.tts(TEXT, conditioning_latents=lat, k=3, sampler="dpm++2m", **KW)
    many = calls("solve_many")
    assert len(many) == 1 and many[0][1] == 3 and many[0][2] == [None] * 3 and not calls("sample_many") and not calls("sample")
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want))


@torch.no_grad()
def test_tts_many_with_utterance_batch_goes_through_solve_many(monkeypatch):
    api = install(monkeypatch)
    t, lat = make(api, candidate_sharding=False, utterance_batch=2)
    texts = [list(range(30, 40)), list(range(41, 49))]
    kw = {k: v for k, v in KW.items() if k != "verbose"}
    want = [t.tts(x, conditioning_latents=lat, sampler="ddim", **KW) for x in texts]
    SolvingDiffusionStage.log = []
    got = t.tts_many(texts, conditioning_latents=lat, sampler="ddim", **kw)
    assert [c[1] for c in calls("solve_many")] == [2] and not calls("sample_many") and not calls("sample")
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@torch.no_grad()
def test_long_form_passes_the_kwargs_on(monkeypatch):
    api = install(monkeypatch)
    from tortoise_tts_amd import longform
    t, lat = make(api, candidate_sharding=False)
    kw = {k: v for k, v in KW.items() if k not in ("verbose", "use_deterministic_seed")}
    longform.read_long_form(t, [TEXT, list(range(30, 40))], conditioning_latents=lat, seed=5, texts_are_chunks=True, sampler="ddim", **kw)
    assert len(calls("solve")) + sum(c[1] for c in calls("solve_many")) == 2 and not calls("sample") and not calls("sample_many")


# ------------------------------------------------------------------------------------------------ ABI
def test_solver_header_symbols_are_exported_and_bound():
    from tortoise_tts_amd import engine as E
    lib = E.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tortoise_mi355x_solver.h")).read(), flags=re.S)
    names = set(re.findall(r"^(?:int|size_t|void)\s+\*?(tt_\w+)\(", src, re.M))
    assert names == set(E._SOLVER_PROTOS) == {"tt_solver_abi_version", "tt_diff_solve", "tt_diff_solve_batch", "tt_diff_solve_stat", "tt_op_solver_update"}
    for n in names:
        assert hasattr(lib, n)
    assert lib.tt_solver_abi_version() == 1 == E.SOLVER_ABI_VERSION
    import ctypes as C
    assert C.sizeof(E.SolverStep) == 28 and [f[0] for f in E.SolverStep._fields_] == ["timestep", "cfk", "sqrt_recip", "sqrt_recipm1", "a", "b", "c"]
    # the frozen drop-in header: same ABI number, same entry points
    assert lib.tt_abi_version() == 6 and not names & set(E._PROTOS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", main))
    assert declared == set(E._PROTOS)  # (tests/test_abi.py caps their number)
