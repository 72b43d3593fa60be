"""What the diffusion stage costs under the p sampler and under the deterministic solvers (include/tortoise_mi355x_solver.h).  A record,
not a gate.

    python scripts/solver_time.py [--out profiles/rNN_solver.txt]      (default: the next free round prefix)

ONE process, full-size synthetic weights (bench.synthetic_weights), one utterance of S = 870 positions (oracle/make_golden_full.py),
conditioning-free guidance on, fp16 operands as tts() runs them.  A case is condition() + sample() / solve() of one handle, device events
around the two calls, inputs resident on the device; per case 2 warm-up runs (the first captures the step graph), then the median and the
spread of 7 runs.  Cases: p at 200 and 30 steps, ddim at 30, dpm++2m at 30 and 20.  Per-step time of a sampler's graph = the slope between
its two step counts (the fixed part - conditioning, the timestep tables, the first chunk of the integrator pre-pass - cancels); ddim and
dpm++2m replay the same captured step, so the solver's slope is taken from dpm++2m.

Then, unless --no-parity, a child process runs tests/test_gpu_solver.py with -s under its own time limit and the figures it prints
([solver]: the update kernel against its fp64 bounds; [parity]: the loops against the oracle's denoiser, the p loop beside them) are
appended with its result line, so that the record's timing and parity parts come from one run.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPEATS = 2, 7
CASES = (("p", 200), ("p", 30), ("ddim", 30), ("dpm++2m", 30), ("dpm++2m", 20))


def next_round_prefix():
    rounds = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return "r%02d" % (max(rounds) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", next_round_prefix() + "_solver.txt")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")

    import torch
    import bench
    from oracle import make_golden_full as GF
    from tortoise_tts_amd import engine as E
    from tortoise_tts_amd import stages
    from tortoise_tts_amd.config import DiffusionConfig
    from tortoise_tts_amd.schedule import Schedule
    from tortoise_tts_amd.solver import SolverPlan

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cfg = DiffusionConfig()
    sd = bench.synthetic_weights()["diffusion"]
    _, _, cond = GF.prompt()
    N_max = max(n for _, n in CASES)
    S, latents, x, step_noise = GF.diff_inputs(cfg, M=GF.DIFF_M, seed=1, steps=N_max)
    latents, cond, x, step_noise = latents.cuda(), cond.cuda(), x.cuda(), step_noise.cuda()
    st = stages.DiffusionStage(sd, cfg, dtype=E.TT_F16, max_seq=S + 8, max_codes=GF.DIFF_M + 8, max_steps=N_max)
    log("# diffusion stage, one utterance, S = %d, cond_free=True, fp16 operands, full-size synthetic weights: condition() + sample() / solve()" % S)
    log("# one process; %d warm-up runs, then %d timed runs per case (device events); step-noise tensor of the p sampler: 100 x S x 4 bytes per step" % (WARM, REPEATS))
    med = {}
    for kind, n in CASES:
        if kind == "p":
            sched, noise = Schedule(n, cfg.trained_steps, True, 2.0), step_noise[:n].contiguous()
            run = lambda: st.sample(sched, x, noise)
            steps = n
        else:
            plan = SolverPlan(kind, n, cond_free=True)
            run = lambda: st.solve(plan, x)
            steps = plan.n_steps
        ms = []
        for r in range(WARM + REPEATS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            st.condition(latents, cond, S)
            mel = run()
            t1.record()
            t1.synchronize()
            assert torch.isfinite(mel).all() and st.guard() == 0
            if r >= WARM:
                ms.append(t0.elapsed_time(t1))
        med[(kind, n)] = statistics.median(ms)
        log("%-8s @ %3d steps (%3d run)   stage ms: median %8.2f  min %8.2f  max %8.2f   noise drawn after x_T: %5.1f MB" % (
            kind, n, steps, med[(kind, n)], min(ms), max(ms), (steps * 100 * S * 4 / 1e6) if kind == "p" else 0.0))
    log("per-step ms, p graph       (p @ 200 - p @ 30) / 170              %.4f" % ((med[("p", 200)] - med[("p", 30)]) / 170))
    log("per-step ms, solver graph  (dpm++2m @ 30 - dpm++2m @ 20) / 10    %.4f" % ((med[("dpm++2m", 30)] - med[("dpm++2m", 20)]) / 10))
    log("graph captures: p %d, solver %d (one per step count each sampler ran)" % (st.stat(0), st.solve_stat(0)))
    st.close()
    if a.no_parity:
        return
    log("")
    log("# python -m pytest -m gpu -s -q tests/test_gpu_solver.py: the figures it prints")
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "pytest", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider", "tests/test_gpu_solver.py"],
                       capture_output=True, text=True, cwd=ROOT)
    rows = [re.sub(r"^[.F]*", "", row) for row in r.stdout.splitlines()]
    for row in rows:
        if row.startswith(("[solver]", "[parity]")) or re.search(r"\d+ (passed|failed)", row):
            log(row)
    if r.returncode != 0:
        log("pytest exit status %d" % r.returncode)
        sys.exit(1)


if __name__ == "__main__":
    main()
