"""No GPU: the fp64 references of tests/univnet_reference.py against torch's own operators and the oracle's LVC in fp64, the one-hot family's
bit-exact property, and plain fp32 emulations of every kernel's summation order, which must stay at or below 0.5 of the element-wise bound on
every input family tests/test_gpu_univnet_forms.py uses (the kernels must stay at or below 1)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import tortoise_oracle as O
from tests import univnet_reference as R

EMU_LIMIT = 0.5
WORST = {}


def _note(form, worst):
    WORST[form] = max(WORST.get(form, 0.0), worst)
    print(f"[bound] emulation {form}: worst |err|/bound={worst:.3f}")


def _close64(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_conv1d_reference_is_torch_conv1d(fam):
    for Cin, Cout, k, d, reflect, T in ((32, 32, 3, 1, 0, 40), (32, 32, 3, 9, 0, 26), (32, 32, 3, 27, 0, 26), (32, 32, 3, 28, 0, 1), (64, 32, 7, 1, 1, 4),
                                        (64, 32, 7, 1, 1, 11), (32, 1, 7, 1, 1, 40)):
        i = R.conv1d_inputs(fam, Cin, Cout, k, T)
        x, w, b = i["x"][0], i["w"], i["bias"]
        for in_slope in (0.2, -1.0):
            ref = R.conv1d_reference(x, w, b, k, d, reflect, in_slope)
            xa = R.lrelu32(x, in_slope).double()[None]
            half = (k // 2) * d
            xa = F.pad(xa, (half, half), mode="reflect") if reflect else F.pad(xa, (half, half))
            want = F.conv1d(xa, w.double(), b.double(), dilation=d)[0]
            assert _close64(ref.value, want), (fam, Cin, Cout, k, d, reflect, T)
            assert bool((ref.bound > 0).all()) or fam == "onehot"


def test_conv1d_reference_activations():
    i = R.conv1d_inputs("gauss", 32, 32, 3, 50)
    x, w, b = i["x"][0], i["w"], i["bias"]
    pre = R.conv1d_reference(x, w, b, 3, 2, 0, 0.2).value
    assert _close64(R.conv1d_reference(x, w, b, 3, 2, 0, 0.2, R.ACT_LRELU, 0.2).value, torch.where(pre > 0, pre, pre * float(torch.tensor(0.2, dtype=torch.float32))))
    assert _close64(R.conv1d_reference(x, w, b, 3, 2, 0, 0.2, R.ACT_TANH).value, torch.tanh(pre))


def test_reflect_reference_refuses_what_torch_refuses():
    i = R.conv1d_inputs("gauss", 64, 32, 7, 3)
    with pytest.raises(AssertionError):
        R.conv1d_reference(i["x"][0], i["w"], i["bias"], 7, 1, 1, -1.0)
    with pytest.raises(RuntimeError):
        F.pad(i["x"], (3, 3), mode="reflect")


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("stride", [8, 4, 2])
def test_convt1d_reference_is_torch_conv_transpose1d(fam, stride):
    for Tin in (1, 2, 37):
        i = R.convt1d_inputs(fam, stride, Tin)
        x, w, b = i["x"][0], i["w"], i["bias"]
        ref = R.convt1d_reference(x, w, b, stride, 0.2)
        want = F.conv_transpose1d(R.lrelu32(x, 0.2).double()[None], w.double(), b.double(), stride=stride, padding=stride // 2 + stride % 2,
                                  output_padding=stride % 2)[0]
        assert ref.value.shape == (32, Tin * stride)
        assert _close64(ref.value, want), (fam, stride, Tin)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("kname", ["f32", "f16", "bf16"])
def test_lvc_reference_is_the_oracle(fam, kname):
    for L, hop in ((1, 8), (2, 64), (5, 8)):
        i = R.lvc_inputs(fam, kname, L, hop)
        x_in, kern, bias, x_res = i["x_in"][0], i["kern"][0], i["bias"][0], i["x_res"][0]
        ref = R.lvc_reference(x_in, kern, bias, x_res, hop, -1.0)
        kk = kern.float().double().permute(1, 2, 3, 0)[None]  # [1, i, o, k, L]
        o = O.location_variable_convolution(x_in.double()[None], kk, bias.double().t()[None], hop)
        want = x_res.double() + (torch.sigmoid(o[:, :32]) * torch.tanh(o[:, 32:]))[0]
        assert _close64(ref.value, want), (fam, kname, L, hop)


def test_onehot_selects_one_input_element_exactly():
    """one unit weight per output channel and zero bias: the fp32 emulations give the selected, LeakyReLU'd element bit for bit"""
    i = R.conv1d_inputs("onehot", 32, 32, 3, 60)
    x, w, b = i["x"][0], i["w"], i["bias"]
    ref = R.conv1d_reference(x, w, b, 3, 9, 0, 0.2)
    for got in (R.emulate_conv1d_direct(x, w, b, 3, 9, 0, 0.2), R.emulate_conv1d_mfma(x, w, b, 9, 0.2)):
        assert torch.equal(got.double(), ref.value)
    sel = R.lrelu32(x, 0.2)
    co = torch.arange(32)
    t = torch.arange(60)
    src = t[None, :] + ((co % 3) - 1)[:, None] * 9
    want = torch.where((src >= 0) & (src < 60), sel[((5 * co + 3) % 32)[:, None], src.clamp(0, 59)], torch.zeros(()))
    assert torch.equal(ref.value, want.double())
    i = R.convt1d_inputs("onehot", 4, 9)
    ref = R.convt1d_reference(i["x"][0], i["w"], i["bias"], 4, 0.2)
    assert torch.equal(R.emulate_convt1d(i["x"][0], i["w"], i["bias"], 4, 0.2).double(), ref.value)


def test_a_permuted_channel_or_tap_fails_the_bound():
    """every channel has its own scale and offset: a kernel that swapped two input channels or two taps is outside the bound"""
    for fam in ("gauss", "offset"):
        i = R.conv1d_inputs(fam, 32, 32, 3, 200)
        x, w, b = i["x"][0], i["w"], i["bias"]
        ref = R.conv1d_reference(x, w, b, 3, 2, 0, 0.2)
        xs = x.clone()
        xs[[3, 4]] = x[[4, 3]]
        ws = w.clone()
        ws[:, :, [0, 2]] = w[:, :, [2, 0]]
        for wrong in (R.emulate_conv1d_mfma(xs, w, b, 2, 0.2), R.emulate_conv1d_mfma(x, ws, b, 2, 0.2), R.emulate_conv1d_mfma(x, w, b, 3, 0.2)):
            assert float(R.ratio(wrong, ref).max()) > 100.0


def test_ulps():
    w = torch.tensor([1.0, 0.75, -3.0], dtype=torch.float64)
    got = torch.tensor([1.0 + 2.0 ** -23, 0.75, -3.0 - 2.0 ** -21], dtype=torch.float32)
    assert R.ulps(got, w).tolist() == [1.0, 0.0, 2.0]


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_conv1d_emulations_within_half_the_bound(fam):
    for d in (1, 2, 3, 9, 26, 27, 28):
        for T in (1, 26, 127, 129, 300):
            i = R.conv1d_inputs(fam, 32, 32, 3, T)
            x, w, b = i["x"][0], i["w"], i["bias"]
            for in_slope, out_act in ((0.2, R.ACT_LRELU), (-1.0, R.ACT_NONE)):
                ref = R.conv1d_reference(x, w, b, 3, d, 0, in_slope, out_act, 0.2)
                _note("conv1d_direct_kernel<32> k3", R.assert_within_bound(f"direct {fam} d={d} T={T}", R.emulate_conv1d_direct(x, w, b, 3, d, 0, in_slope, out_act, 0.2), ref, EMU_LIMIT))
                if d <= 27:
                    _note("conv1d_mfma_kernel", R.assert_within_bound(f"mfma {fam} d={d} T={T}", R.emulate_conv1d_mfma(x, w, b, d, in_slope, out_act, 0.2), ref, EMU_LIMIT))
    for T in (4, 11, 255, 257):
        i = R.conv1d_inputs(fam, 64, 32, 7, T)
        ref = R.conv1d_reference(i["x"][0], i["w"], i["bias"], 7, 1, 1, -1.0)
        _note("conv1d_direct_kernel<32> k7 reflect", R.assert_within_bound(f"conv_pre {fam} T={T}", R.emulate_conv1d_direct(i["x"][0], i["w"], i["bias"], 7, 1, 1, -1.0), ref, EMU_LIMIT))
        i = R.conv1d_inputs(fam, 32, 1, 7, T)
        ref = R.conv1d_reference(i["x"][0], i["w"], i["bias"], 7, 1, 1, 0.2, R.ACT_TANH)
        _note("conv1d_direct_kernel<1> k7 reflect tanh", R.assert_within_bound(f"conv_post {fam} T={T}", R.emulate_conv1d_direct(i["x"][0], i["w"], i["bias"], 7, 1, 1, 0.2, R.ACT_TANH), ref, EMU_LIMIT))


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_convt1d_emulation_within_half_the_bound(fam):
    for stride in (8, 4, 2):
        for Tin in (1, 2, 255, 257):
            i = R.convt1d_inputs(fam, stride, Tin)
            x, w, b = i["x"][0], i["w"], i["bias"]
            ref = R.convt1d_reference(x, w, b, stride, 0.2)
            _note("convt1d_kernel", R.assert_within_bound(f"convt {fam} s={stride} Tin={Tin}", R.emulate_convt1d(x, w, b, stride, 0.2), ref, EMU_LIMIT))


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("kname", ["f32", "f16", "bf16"])
def test_lvc_emulations_within_half_the_bound(fam, kname):
    for L, hop in ((1, 8), (5, 8), (2, 64), (5, 64), (1, 256), (2, 256)):
        i = R.lvc_inputs(fam, kname, L, hop)
        x_in, kern, bias, x_res = i["x_in"][0], i["kern"][0], i["bias"][0], i["x_res"][0]
        for in_slope in (-1.0, 0.2):
            ref = R.lvc_reference(x_in, kern, bias, x_res, hop, in_slope)
            _note("lvc_kernel", R.assert_within_bound(f"lvc {fam} {kname} L={L} hop={hop}", R.emulate_lvc(x_in, kern, bias, x_res, hop, in_slope), ref, EMU_LIMIT))
            if hop != 8:
                _note("lvc_mfma_kernel", R.assert_within_bound(f"lvc mfma {fam} {kname} L={L} hop={hop}", R.emulate_lvc_mfma(x_in, kern, bias, x_res, hop, in_slope), ref, EMU_LIMIT))


def test_activation_probe_takes_the_arithmetic_out():
    p = R.activation_probe(2, 64)
    o, S = R.lvc_preact(p["x_in"], p["kern"], p["bias"], 64, -1.0)
    grid = p["x_in"][0].double()
    assert torch.equal(o[0], grid) and torch.equal(o[33], grid) and bool((o[32] == 30).all()) and bool((o[1] == 88).all())
    assert float(torch.tanh(torch.tensor(30.0))) == 1.0 and float(1.0 / (1.0 + torch.exp(torch.tensor(-88.0)))) == 1.0
    assert float(grid.min()) == -12.0 and float(grid.max()) == 12.0
