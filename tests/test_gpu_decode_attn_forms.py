"""-m gpu: the three forms of the decode attention agree IN BITS (csrc/decode_attention.hip).

decode_attn_lds_kernel<4> (variant 0), decode_attn_lds_kernel<16> (variant 2) and the per-wave decode_attn_kernel (variant 1) are built from
one set of wave-level steps (dec_*): per (sequence, head) the same products in the same order, whatever the workgroup geometry and wherever
the prefix is read from.  tests/test_gpu_qkv_attn.py holds the fused QKV + attention launch to the bits of the two-launch path; this test
holds the other forms to one another, and each to the float reference of tests/test_gpu_r6.py at its tolerances.
"""
import pytest
import torch

from tortoise_tts_amd import engine as E
from tests.gpu_util import DTYPES, report
from tests.test_gpu_r6 import _decode_attention_reference

pytestmark = pytest.mark.gpu
FORMS = {0: "LDS prefix, 4 sequences per workgroup", 2: "LDS prefix, 16 sequences per workgroup", 1: "one wave per (sequence, head)"}


@pytest.fixture(scope="module")
def lib():
    return E.init()


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("B,P1,tgen,tmax", [(7, 33, 3, 16), (20, 65, 65, 72), (16, 1, 1, 8)])
def test_decode_attention_forms_agree_in_bits(lib, name, dt, tdt, tol, B, P1, tgen, tmax):
    """(7, 33, 3, 16): surplus waves in the last workgroup and one partial prefix slot; (20, 65, 65, 72): two prefix slots, two own slots with
    the second nearly empty, an odd number of PV iterations; (16, 1, 1, 8): the smallest legal prefix and a single own key.  Cache slots at
    and beyond tgen hold +-1e4: a form that reads one of them into a sum shows at once."""
    H = 16
    g = torch.Generator().manual_seed(B * 1000 + tgen)
    q = (torch.randn(B, H, 64, generator=g) * 0.125 * 2).to(tdt)
    kp = (torch.randn(H, P1, 64, generator=g) * 2).to(tdt)
    vp = torch.randn(H, P1, 64, generator=g).to(tdt)
    k_own = (torch.randn(B, H, tgen, 64, generator=g) * 2).to(tdt)
    v_own = torch.randn(B, H, tgen, 64, generator=g).to(tdt)
    # cache layouts (include/tortoise_mi355x.h): keys [B][H][8 chunks][tmax][8], values [B][H][tmax][64]
    kc = torch.full((B, H, 8, tmax, 8), 1e4).to(tdt)
    kc[:, :, :, :tgen] = k_own.reshape(B, H, tgen, 8, 8).permute(0, 1, 3, 2, 4)
    vc = torch.full((B, H, tmax, 64), -1e4).to(tdt)
    vc[:, :, :tgen] = v_own
    want = _decode_attention_reference(q.float(), kp.float(), vp.float(), k_own.float(), v_own.float()).reshape(B, H * 64)
    dq, dkp, dvp, dkc, dvc = (t.cuda().contiguous() for t in (q.reshape(B, H * 64), kp, vp, kc, vc))
    outs = {}
    for variant in FORMS:
        out = torch.zeros(B, H * 64, device="cuda", dtype=tdt)
        E.check(lib.tt_op_decode_attention(dt, E.ptr(dq), E.ptr(dkp), E.ptr(dvp), P1, E.ptr(dkc), E.ptr(dvc), tmax, tgen, E.ptr(out), B, H, variant, None))
        torch.cuda.synchronize()
        outs[variant] = out.cpu()
        report(f"decode attention forms {name} B={B} P1={P1} own keys={tgen}: {FORMS[variant]}", outs[variant].float(), want, {"bf16": 4e-3, "f16": 6e-4}[name])
    for variant in (2, 1):
        differ = int((outs[variant].view(torch.int16) != outs[0].view(torch.int16)).sum())
        print(f"[parity] decode attention forms {name} B={B} P1={P1} own keys={tgen}: '{FORMS[variant]}' vs '{FORMS[0]}': {differ} of {outs[0].numel()} elements differ")
    assert torch.equal(outs[2], outs[0]), f"{FORMS[2]} differs in bits from {FORMS[0]}"
    assert torch.equal(outs[1], outs[0]), f"{FORMS[1]} differs in bits from {FORMS[0]}"
