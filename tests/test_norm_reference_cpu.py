"""CPU: the element-wise bounds of tests/norm_reference.py can fail, and their constants have margin.  Every mutation below puts at least one
element outside the bound at D = 1024 and at D = 4096 (C = 1024, S = 77 for GroupNorm); the plain fp32 emulations of the kernels' algorithms
stay at or below 0.5 of the bound on every input family tests/test_gpu_norm_forms.py uses (the kernels have to stay at or below 1)."""
import pytest
import torch

from tests import norm_reference as N

M, NSLAB, EPS = 7, 3, 1e-5
HALF = 0.5


@pytest.fixture(scope="module", params=[1024, 4096])
def row(request):
    """double LayerNorm on bias + three slabs; row 2 has a spread of 1e-3 around 1"""
    D = request.param
    d = N.rownorm_inputs(D, M, D, NSLAB)
    d["x"][2] = N.rownorm_edge_rows(D, EPS)[2]
    d["slabs"][:, 2] *= 1e-4
    d["bias"] = d["bias"] * 0.25
    d["t"] = N.updated_row(d["x"], None, d["bias"], d["slabs"])
    d["one"] = N.rownorm_reference(d["t"], N.NORM_LAYER, d["g1"], d["b1"], EPS)
    d["two"] = N.rownorm_reference(d["t"], N.NORM_LAYER, d["g1"], d["b1"], EPS, d["g2"], d["b2"], 1e-6)
    return d


def emu(d, t=None, **kw):
    args = dict(g1=d["g1"], b1=d["b1"], eps1=EPS)
    args.update(kw)
    return N.rownorm_emulate(d["t"] if t is None else t, N.NORM_LAYER, **args)


def rejects(got, ref, out="f32"):
    with pytest.raises(AssertionError):
        N.assert_within_bound("mutated", got, ref, out, quiet=True)


def test_row_emulation_is_inside_half_the_bound(row):
    assert N.assert_within_bound("LayerNorm", emu(row), row["one"], "f32") <= HALF
    assert N.assert_within_bound("double LayerNorm", emu(row, g2=row["g2"], b2=row["b2"], eps2=1e-6), row["two"], "f32") <= HALF


def test_one_slab_dropped(row):
    rejects(emu(row, N.updated_row(row["x"], None, row["bias"], row["slabs"][:2])), row["one"])


def test_bias_added_twice_on_one_quad(row):
    b = row["bias"].clone()
    b[8:12] *= 2.0
    rejects(emu(row, N.updated_row(row["x"], None, b, row["slabs"])), row["one"])


def test_gamma_shifted_by_four_channels(row):
    rejects(emu(row, g1=row["g1"].roll(4)), row["one"])


def test_variance_divided_by_d_minus_1(row):
    rejects(emu(row, unbiased=True), row["one"])


def test_eps_left_out_on_a_row_of_small_spread(row):
    got = emu(row, eps1=0.0)
    ratio = N.worst_ratio(got, row["one"], "f32")
    assert ratio[2].max() > 1.0  # the row of spread 1e-3: var ~ 1e-6 against eps 1e-5
    rejects(got, row["one"])


def test_row_normalised_with_its_neighbours_statistics(row):
    rejects(emu(row, neighbour=True), row["one"])


def test_second_layernorm_skipped(row):
    rejects(emu(row), row["two"])


@pytest.mark.parametrize("out,tdt", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_t_output_rounded_toward_zero(row, out, tdt):
    y = emu(row)
    assert N.assert_within_bound("round to nearest", y.to(tdt), row["one"], out) <= 1.0
    rejects(N.round_toward_zero(y, tdt), row["one"], out)


# ------------------------------------------------------------------------------------------------- GroupNorm32
@pytest.fixture(scope="module")
def gn():
    """C = 1024, S = 77, four samples of 77 / 9 valid rows, scale / shift blocks shared by pairs of samples (ss_batch_div = 2), SiLU"""
    B, S, C = 4, 77, 1024
    d = N.groupnorm_inputs(11, B, S, C)
    d["vlen"] = [77, 9]
    d["ss2"] = N.ss_per_sample(d["ss"], B, C, 2, 2 * C)
    d["ref"], d["kappa"] = N.groupnorm_reference(d["x"], d["gamma"], d["beta"], EPS, d["vlen"], d["ss2"], N.ACT_SILU)
    return d


def gn_emu(d, **kw):
    args = dict(eps=EPS, vlen=d["vlen"], ss=d["ss2"], act=N.ACT_SILU)
    args.update(kw)
    return N.groupnorm_emulate(d["x"], d["gamma"], d["beta"], **args)


def test_groupnorm_emulation_is_inside_half_the_bound(gn):
    assert float(gn["kappa"].max()) <= N.KAPPA_MAX
    got = gn_emu(gn)
    assert N.assert_within_bound("GroupNorm", got, gn["ref"], "f32") <= HALF
    assert (got[1, 9:] == 0).all() and (gn["ref"].value[1, 9:] == 0).all()


def test_group_boundaries_shifted_by_four_channels(gn):
    rejects(gn_emu(gn, group_shift=4), gn["ref"])


def test_padded_rows_counted_in_the_statistics(gn):
    rejects(gn_emu(gn, count_pad=True), gn["ref"])


def test_nonzero_padded_row_is_rejected(gn):
    got = gn_emu(gn)
    got[1, 40, 3] = 1e-30
    rejects(got, gn["ref"])


def test_scale_shift_block_of_the_wrong_sample(gn):
    """ss_batch_div ignored: sample b reads block b instead of block b / 2"""
    rejects(gn_emu(gn, ss=N.ss_per_sample(gn["ss"], 4, 1024, 1, 2 * 1024)), gn["ref"])


@pytest.mark.parametrize("out,tdt", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_groupnorm_t_output_rounded_toward_zero(gn, out, tdt):
    y = gn_emu(gn)
    assert N.assert_within_bound("round to nearest", y.to(tdt), gn["ref"], out) <= 1.0
    rejects(N.round_toward_zero(y, tdt), gn["ref"], out)


# ------------------------------------------------------------------------------------------------- the input families of the GPU tests
@pytest.mark.parametrize("D", [4, 132, 512, 1020, 1024, 1028, 2048, 4096])
def test_row_emulation_on_the_gpu_test_inputs(D):
    """LayerNorm, RMSNorm, the double LayerNorm and LayerNorm + activation on x / x_in + bias + 0, 3 and 8 slabs, M = 5 and M = 1027"""
    worst = {}
    for M_ in (5, 1027):
        for nslab in (0, 3, 8):
            d = N.rownorm_inputs(D * 16 + nslab, M_, D, nslab)
            t = N.updated_row(d["x"], d["x_in"] if nslab == 3 else None, d["bias"] if nslab else None, d["slabs"])
            forms = {"LayerNorm": dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=1e-5),
                     "RMSNorm": dict(mode=N.NORM_RMS, g1=d["g1"], eps1=1e-8),
                     "double LayerNorm": dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=1e-5, g2=d["g2"], b2=d["b2"], eps2=1e-6),
                     "LayerNorm + GELU": dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=1e-5, act=N.ACT_GELU_ERF),
                     "LayerNorm + SiLU": dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=1e-5, act=N.ACT_SILU)}
            for name, kw in forms.items():
                w = N.assert_within_bound(f"{name} D={D} M={M_} nslab={nslab}", N.rownorm_emulate(t, **kw), N.rownorm_reference(t, **kw), "f32", quiet=True)
                worst[name] = max(worst.get(name, 0.0), w)
    print(f"[bound] fp32 emulation D={D}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= HALF, worst


@pytest.mark.parametrize("D", [4, 1024, 4096])
def test_row_emulation_on_the_edge_rows(D):
    for eps in (1e-5, 1e-8):
        t = N.rownorm_edge_rows(D, eps)
        d = N.rownorm_inputs(D, 6, D)
        for kw in (dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=eps), dict(mode=N.NORM_RMS, g1=d["g1"], eps1=eps),
                   dict(mode=N.NORM_LAYER, g1=d["g1"], b1=d["b1"], eps1=eps, g2=d["g2"], b2=d["b2"], eps2=1e-6)):
            ref = N.rownorm_reference(t, **kw)
            assert torch.isfinite(ref.value).all()
            assert N.assert_within_bound(f"edge rows D={D} eps={eps} {kw['mode']}", N.rownorm_emulate(t, **kw), ref, "f32") <= HALF


@pytest.mark.parametrize("C,B,S", N.gn_cases())
def test_groupnorm_emulation_on_the_gpu_test_inputs(C, B, S):
    d = N.groupnorm_inputs(N.gn_seed(C, B, S), B, S, C)
    ss = N.ss_per_sample(d["ss"], B, C, 1, 2 * C)
    ref, kappa = N.groupnorm_reference(d["x"], d["gamma"], d["beta"], EPS, None, ss, N.ACT_SILU)
    assert float(kappa.max()) <= N.KAPPA_MAX, float(kappa.max())
    assert N.assert_within_bound(f"GroupNorm C={C} B={B} S={S}", N.groupnorm_emulate(d["x"], d["gamma"], d["beta"], EPS, None, ss, N.ACT_SILU), ref, "f32") <= HALF
    ref, _ = N.groupnorm_reference(d["x"], d["gamma"], d["beta"], EPS)
    assert N.assert_within_bound(f"GroupNorm C={C} B={B} S={S} plain", N.groupnorm_emulate(d["x"], d["gamma"], d["beta"], EPS), ref, "f32") <= HALF


@pytest.mark.parametrize("C", N.GN_CHANNELS)
def test_groupnorm_reference_at_a_large_mean(C):
    """kappa ~ 1e4 (mean / spread = 100): the bound is wide but finite, and the emulation is inside it"""
    d = N.groupnorm_inputs(C, 2, 77, C)
    x = torch.randn(2, 77, C, generator=torch.Generator().manual_seed(C)) + 100.0
    ref, kappa = N.groupnorm_reference(x, d["gamma"], d["beta"], EPS)
    assert 5e3 < float(kappa.min()) and float(kappa.max()) < 2e4
    assert N.assert_within_bound(f"GroupNorm C={C} kappa 1e4", N.groupnorm_emulate(x, d["gamma"], d["beta"], EPS), ref, "f32") <= 1.0


@pytest.mark.parametrize("B,S,vlen", [(4, 77, [77, 9]), (3, 333, [1, 333, 200])])
def test_groupnorm_emulation_on_padded_batches(B, S, vlen):
    C = 1024
    d = N.groupnorm_inputs(N.gn_seed(C, B, S) + 1, B, S, C)
    ref, kappa = N.groupnorm_reference(d["x"], d["gamma"], d["beta"], EPS, vlen)
    assert float(kappa.max()) <= N.KAPPA_MAX
    got = N.groupnorm_emulate(d["x"], d["gamma"], d["beta"], EPS, vlen)
    assert N.assert_within_bound(f"GroupNorm vlen={vlen}", got, ref, "f32") <= HALF
    for b in range(B):
        assert (ref.value[b, vlen[b % len(vlen)]:] == 0).all()
