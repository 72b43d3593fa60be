"""CPU-only checks of the drop-in boundary: the C-ABI library builds/loads, exports every symbol that
include/tortoise_mi355x.h declares, the ctypes mirrors have the library's struct sizes, and a call
without a GPU fails loudly through tt_last_error (never silently falls back)."""
import ctypes as C
import os
import re

import pytest

from tortoise_tts_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        from tortoise_tts_amd.build import build
        build(verbose=False)
    return E.load_library()


def declared_symbols(header="tortoise_mi355x.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ttx?_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    """Both headers under include/: the drop-in boundary and the operator-level test entries."""
    names = declared_symbols()
    assert 30 <= len(names) <= 60, len(names)  # the boundary a maintainer binds stays small: experiments and test hooks live elsewhere
    assert not [n for n in names if n.startswith(("tt_op_", "ttx_"))], "test / experiment entries belong in tortoise_mi355x_test.h"
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in the header but not exported: {missing}"
    assert set(names) == set(E._PROTOS), set(names) ^ set(E._PROTOS)
    tnames = declared_symbols("tortoise_mi355x_test.h")
    missing = [n for n in tnames if not hasattr(lib, n)]
    assert not missing, f"declared in the test header but not exported: {missing}"
    assert set(tnames) == set(E._TEST_PROTOS), set(tnames) ^ set(E._TEST_PROTOS)


def test_struct_mirrors_match(lib):
    for i, st in enumerate(E.BOUNDARY_STRUCTS):
        assert C.sizeof(st) == lib.tt_struct_size(i), st.__name__
    assert lib.tt_abi_version() == 6
    # the operator-level descriptors of the test header (tt_op_gemm_ex, tt_op_rownorm_ex, tt_op_groupnorm_ex, tt_op_conv1d_ex, tt_op_convt1d_ex,
    # tt_op_lvc_ex), field by field: a reordered field keeps the size
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x_test.h")).read()
    for cname, mirror, size in (("tt_op_gemm_desc", E.GemmDesc, lib.tt_op_gemm_desc_size()), ("tt_op_rownorm_desc", E.RowNormDesc, lib.tt_op_rownorm_desc_size()),
                                ("tt_op_groupnorm_desc", E.GroupNormDesc, lib.tt_op_groupnorm_desc_size()),
                                ("tt_op_conv1d_desc", E.Conv1dDesc, lib.tt_op_conv1d_desc_size()), ("tt_op_convt1d_desc", E.ConvT1dDesc, lib.tt_op_convt1d_desc_size()),
                                ("tt_op_lvc_desc", E.LvcDesc, lib.tt_op_lvc_desc_size())):
        assert C.sizeof(mirror) == size, cname
        names = [f[0] for f in mirror._fields_]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            rest = re.match(r"^(?:const\s+)?\w+\s*\**\s*(.*)$", decl, flags=re.S).group(1)
            declared += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in rest.split(",")]
        assert declared == names, (cname, declared, names)


def test_reflect_padding_the_kernel_cannot_index_is_refused_on_the_host(lib):
    """conv1d_direct_kernel reflects an index once: conv1d_direct_launch refuses a sequence of no more than (k / 2) * dilation columns before
    anything is launched (no device is touched: the pointers are never read), for the n = 0 form and for one short sequence of a batch"""
    for T, n, mul, frames, k, d in ((3, 0, 0, (), 7, 1), (64, 2, 1, (64, 3), 7, 1), (64, 2, 3, (21, 1), 7, 1), (18, 0, 0, (), 7, 6), (1, 0, 0, (), 3, 1)):
        desc = E.Conv1dDesc(Cin=32, Cout=32, T=T, k=k, dilation=d, reflect=1, in_slope=-1.0, seq_n=n, seq_mul=mul)
        for i, f in enumerate(frames):
            desc.seq_frames[i] = f
        ran = (C.c_int * 4)(-2, -2, -2, -2)
        rc = lib.tt_op_conv1d_ex(C.byref(desc), ran, None)
        assert rc < 0 and b"reflect" in lib.tt_last_error(), (rc, lib.tt_last_error())
        assert tuple(ran) == (-1, 0, 0, 0)


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc = lib.tt_init()
    assert rc != 0
    assert b"hip" in lib.tt_last_error().lower() or b"device" in lib.tt_last_error().lower()
    with pytest.raises(E.EngineError):
        E.check(rc)


def test_header_constants_match_the_host_mirror():
    """Every integer `#define TT_*` of the header that the ctypes host names too has the header's value (dtype codes, option ids)."""
    src = open(os.path.join(ROOT, "include", "tortoise_mi355x.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(TT_[A-Z0-9_]+)\s+(-?\d+)\s*$", src, flags=re.M)}
    assert {"TT_BF16", "TT_F16", "TT_F32", "TT_AR_OPT_LOOKAHEAD", "TT_DIFF_OPT_OVERLAP_PREPASS", "TT_DIFF_OPT_FUSED_GN"} <= set(defines)
    mirrored = [k for k in defines if hasattr(E, k)]
    assert len(mirrored) >= 6
    for k in mirrored:
        assert getattr(E, k) == defines[k], k
