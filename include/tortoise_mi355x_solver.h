/*
 * Deterministic diffusion solvers on a tt_diff handle: DDIM (eta = 0) and DPM-Solver++(2M) (Lu et al. 2022, data prediction, multistep
 * order 2).  Both walk the probability-flow ODE of the trained 4000-step schedule in N denoiser evaluations and draw no noise after x_T.
 *
 *   step      with eps the model's first C output columns (the learned-variance half is not read), guided as in the p sampler,
 *               eps  = (1 + cfk) eps_c - cfk eps_u                      (cond_free; else eps = eps_c)
 *               x0   = clamp(sqrt_recip x - sqrt_recipm1 eps, -1, 1)
 *               x'   = fma(c, x0_prev, fma(b, x0, a x))
 *             x0_prev is the x0 of the step before, kept in f32 on the handle.  A step with c == 0 does not read it, so the first step of a
 *             run never sees what an earlier run left there.  Every step stores its x0 as the next step's x0_prev.
 *   records   the host computes (a, b, c) per step in fp64 (tortoise_tts_amd/solver.py) and hands them over as f32, in the order the
 *             steps run; the last record of a run is the terminal step (0, 1, 0), whose result is the clamped x0
 *   output    mel_out as tt_diff_sample writes it: the state of the last step, denormalised, channels first [C][S]
 *
 * The denoiser, the conditioning pre-pass, the step counter, the overflow guard (tt_diff_guard) and the handling of a padded batch are
 * the ones of tt_diff_sample / tt_diff_sample_batch; the preconditions are theirs too (tt_diff_condition, or tt_diff_batch_begin and
 * tt_diff_condition_slot for every utterance, first).  The captured solver step is kept on the handle beside the p sampler's, each
 * under its own key: alternating the two on one handle re-captures neither.  tt_diff_stat(h, 0) counts the p sampler's captures only.
 * The split path (tt_diff_split_*) has no solver form.
 *
 * Its own header and version; exported from the same library as tortoise_mi355x.h.  Errors are reported through tt_last_error(); every
 * argument and capacity check happens before any device work.
 */
#ifndef TORTOISE_MI355X_SOLVER_H
#define TORTOISE_MI355X_SOLVER_H
#include "tortoise_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int tt_solver_abi_version(void);

typedef struct tt_solver_step {
  int timestep;                  /* trained-schedule timestep the denoiser is evaluated at */
  float cfk;                     /* conditioning-free weight of this step */
  float sqrt_recip, sqrt_recipm1;/* 1 / alpha_t, sigma_t / alpha_t */
  float a, b, c;                 /* x' = a x + b x0 + c x0_prev */
} tt_solver_step;

/* x_T f32 [C][S] (device), steps_host: n_steps records in run order (host), mel_out f32 [C][S] (device).  1 <= n_steps <= max_steps. */
int tt_diff_solve(tt_diff* h, const float* x_T, const tt_solver_step* steps_host, int n_steps, int cond_free, float* mel_out, void* stream);

/* The U utterances of the current batch (tt_diff_batch_begin): x_T[u] f32 [C][S_u], mel_out[u] f32 [C][S_u] (host arrays of device
 * pointers).  All utterances walk the same records. */
int tt_diff_solve_batch(tt_diff* h, int U, const float* const* x_T, const tt_solver_step* steps_host, int n_steps, int cond_free,
                        float* const* mel_out, void* stream);

/* which = 0: solver-step graph captures so far (tests: the kept graph is reused); anything else: -1 */
int tt_diff_solve_stat(tt_diff* h, int which);

/* The update kernel alone (tests).  Device pointers except `step`:
 *   dtype      TT_BF16 | TT_F16 | TT_F32: the element type of x_t
 *   x          f32 [S][C]                 state, updated in place
 *   model      f32 [1 or 2][ld_rows][2C]  model output rows, token major: row block 0 conditioned, block 1 (has_uncond) conditioning-free;
 *                                         ld_rows >= S rows lie between the two blocks
 *   hist       f32 [S][C]                 x0 of the step before: read only when step->c != 0, always written
 *   step       one record (host)
 *   x_t        [1 or 2][ld_rows][cpad]    optional operand copy of the new state for both blocks, zeros in columns C .. cpad - 1
 *   mel_out    f32 [C][S]                 optional denormalised copy of the new state, channels first
 *   guard      i32 [1]                    optional counter: += 1 per wave that read a non-finite model value
 * Synchronous: returns after the kernel has run. */
int tt_op_solver_update(int dtype, float* x, const float* model, int ld_rows, int has_uncond, float* hist, const tt_solver_step* step, int S,
                        int C, int cpad, void* x_t, float* mel_out, int* guard, void* stream);

#ifdef __cplusplus
}
#endif
#endif
