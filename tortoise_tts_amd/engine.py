"""ctypes binding of include/tortoise_mi355x.h (the drop-in boundary), include/tortoise_mi355x_align.h (the redaction aligner) and
include/tortoise_mi355x_test.h (operator-level test entries).

The library is the product: there is no PyTorch/CPU fallback.  If the shared object is missing
or the device is not gfx950, loading fails loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TORTOISE_MI355X_LIB") or os.path.join(HERE, "lib", "libtortoise_mi355x.so")  # env: an alternative build of the same ABI

TT_BF16, TT_F16, TT_F32 = 0, 1, 2  # TT_F32: the slow fp32-operand VERIFICATION mode of the AR / CLVP / diffusion / vocoder stages (tests)
DTYPE_NAMES = {TT_BF16: "bf16", TT_F16: "fp16", TT_F32: "fp32"}
TT_AR_OPT_LOOKAHEAD = 4
TT_AR_OPT_SESSIONS = 5
TT_AR_OPT_SESSION_CLOSE = 6
TT_AR_OPT_SESSION_SAMPLING = 7
TT_AR_OPT_FUSED_QKV_ATTN = 8
TT_DIFF_OPT_OVERLAP_PREPASS = 1
TT_DIFF_OPT_FUSED_GN = 2
TTX_FLASH32, TTX_GEMM_P8, TTX_VOC_MFMA, TTX_GEMM_SKINNY, TTX_AR_GEMV, TTX_NR_SELECT_LONG = 0, 1, 2, 3, 4, 5  # ttx_kernel_variant families (include/tortoise_mi355x_test.h)


def dtype_code(name):
    """'bf16' | 'fp16' | 'f16' (or an engine code) -> engine dtype code."""
    if isinstance(name, int):
        return name
    try:
        return {"bf16": TT_BF16, "fp16": TT_F16, "f16": TT_F16, "fp32": TT_F32, "f32": TT_F32}[name]
    except KeyError:
        raise ValueError(f"unknown operand type {name!r} (bf16 | fp16; fp32 = the slow verification mode)") from None
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SILU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3, 4, 5

vp, fp, ip = C.c_void_p, C.c_void_p, C.c_void_p  # device pointers are passed as integers


class EngineError(RuntimeError):
    pass


class GptLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("ln1_g", "ln1_b", "w_qkv", "b_qkv", "w_proj", "b_proj", "ln2_g", "ln2_b",
                                  "w_fc", "b_fc", "w_proj2", "b_proj2")]


class ArConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "layers", "model_dim", "heads", "vocab", "start_mel_token", "stop_mel_token",
                                       "mel_pos_len", "max_batch", "max_prefix", "max_new_tokens", "max_full_rows",
                                       "mel_pos_offset", "max_groups")]


class ArWeights(C.Structure):
    _fields_ = [("layers_host", C.POINTER(GptLayer))] + [(n, vp) for n in (
        "lnf_g", "lnf_b", "final_norm_g", "final_norm_b", "w_mel_head", "b_mel_head", "mel_emb", "mel_pos")]


class Sampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float), ("top_k", C.c_int),
                ("seed", C.c_ulonglong), ("row_offset", C.c_int), ("exp_noise", vp), ("group_seeds", C.POINTER(C.c_ulonglong)),
                ("typical_mass", C.c_float)]


class ClvpLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("attn_norm_g", "w_qkv", "w_out", "b_out", "ff_norm_g", "w_ff1", "b_ff1", "w_ff2", "b_ff2")]


class ClvpTower(C.Structure):
    _fields_ = [("layers_host", C.POINTER(ClvpLayer))] + [(n, vp) for n in ("emb", "inv_freq", "norm_g", "norm_b", "w_latent")]


class ClvpConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "dim", "latent_dim", "depth", "heads", "ff_inner", "rot_dim", "max_rows")]


class AttnBlock(C.Structure):
    _fields_ = [(n, vp) for n in ("norm_g", "norm_b", "w_qkv", "b_qkv", "w_proj", "b_proj", "relpos")]


class ResBlock(C.Structure):
    _fields_ = [(n, vp) for n in ("gn1_g", "gn1_b", "w_in", "b_in", "gn2_g", "gn2_b", "w_out", "b_out")]


class DiffConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "channels", "heads", "num_layers", "in_channels", "in_pad", "out_channels",
                                       "latent_channels", "max_seq", "max_codes", "max_steps", "max_batch")]


class DiffWeights(C.Structure):
    _fields_ = [("w_latent_conv", vp), ("b_latent_conv", vp), ("latent_attn_host", C.POINTER(AttnBlock)),
                ("code_norm_g", vp), ("code_norm_b", vp), ("uncond_emb", vp),
                ("w_time1", vp), ("b_time1", vp), ("w_time2", vp), ("b_time2", vp), ("w_emb_all", vp), ("b_emb_all", vp),
                ("res_host", C.POINTER(ResBlock)), ("attn_host", C.POINTER(AttnBlock)),
                ("w_inp", vp), ("b_inp", vp), ("w_integ", vp), ("b_integ", vp), ("out_gn_g", vp), ("out_gn_b", vp),
                ("w_final", vp), ("b_final", vp)]


class DiffStep(C.Structure):
    _fields_ = [("timestep", C.c_int)] + [(n, C.c_float) for n in (
        "min_log", "max_log", "cfk", "sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "nonzero")]


class SolverStep(C.Structure):  # tt_solver_step (include/tortoise_mi355x_solver.h)
    _fields_ = [("timestep", C.c_int)] + [(n, C.c_float) for n in ("cfk", "sqrt_recip", "sqrt_recipm1", "a", "b", "c")]


class VocBlock(C.Structure):
    _fields_ = [("w_convt", vp), ("b_convt", vp), ("w_kp_in", vp), ("b_kp_in", vp),
                ("w_kp_res", vp * 6), ("b_kp_res", vp * 6), ("w_kp_kernel", vp), ("b_kp_kernel", vp),
                ("w_kp_bias", vp), ("b_kp_bias", vp), ("w_conv", vp * 4), ("b_conv", vp * 4), ("stride", C.c_int)]


class VocConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "max_frames", "mel_channels", "mel_pad")]


class VocWeights(C.Structure):
    _fields_ = [("w_pre", vp), ("b_pre", vp), ("blocks_host", C.POINTER(VocBlock)), ("w_post", vp), ("b_post", vp)]


class CondConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "ar_dim", "ar_heads", "ar_blocks", "ar_mel", "ar_mel_pad", "diff_channels", "diff_heads",
                                       "diff_blocks", "diff_mel", "diff_mel_pad", "max_frames")]


class CondWeights(C.Structure):
    _fields_ = [("ar_w_init", vp), ("ar_b_init", vp), ("ar_attn_host", C.POINTER(AttnBlock)),
                ("diff_w_c0", vp), ("diff_b_c0", vp), ("diff_w_c1", vp), ("diff_b_c1", vp), ("diff_attn_host", C.POINTER(AttnBlock))]


class CvvpTower(C.Structure):
    _fields_ = [("layers_host", C.POINTER(ClvpLayer)), ("inv_freq", vp), ("norm_g", vp), ("norm_b", vp), ("w_pre0", vp), ("b_pre0", vp),
                ("attn", AttnBlock), ("w_pre2", vp), ("b_pre2", vp), ("w_latent", vp)]


class CvvpConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "dim", "heads", "depth", "rot_dim", "mel_channels", "mel_pad", "max_rows", "max_cond_frames")]


class CvvpWeights(C.Structure):
    _fields_ = [("cond", CvvpTower), ("speech", CvvpTower), ("w_cond0", vp), ("b_cond0", vp), ("w_cond1", vp), ("b_cond1", vp),
                ("speech_emb", vp), ("temperature", vp)]


HIFI_MAX_STAGES = 6


class HifiResBlock(C.Structure):
    _fields_ = [("w1", vp * 3), ("b1", vp * 3), ("w2", vp * 3), ("b2", vp * 3)]


class HifiConfig(C.Structure):
    _fields_ = [("dtype", C.c_int), ("in_channels", C.c_int), ("cond_channels", C.c_int), ("initial_channel", C.c_int),
                ("num_stages", C.c_int), ("up_factor", C.c_int * HIFI_MAX_STAGES), ("num_kernels", C.c_int), ("kernel_size", C.c_int * 3),
                ("num_dilations", C.c_int), ("dilation", C.c_int * 3), ("lrelu_slope", C.c_float), ("max_latents", C.c_int)]


class HifiWeights(C.Structure):
    _fields_ = [("w_pre", vp), ("b_pre", vp), ("w_cond", vp), ("b_cond", vp), ("w_up", vp * HIFI_MAX_STAGES), ("b_up", vp * HIFI_MAX_STAGES),
                ("res_host", C.POINTER(HifiResBlock)), ("w_post", vp), ("b_post", vp)]


W2V_CONV_LAYERS = 7


class W2vConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "dim", "heads", "layers", "ff_dim", "conv_dim")] + [
        ("conv_kernel", C.c_int * W2V_CONV_LAYERS), ("conv_stride", C.c_int * W2V_CONV_LAYERS)] + [
        (n, C.c_int) for n in ("pos_kernel", "pos_groups", "vocab", "vocab_pad", "max_samples")] + [("eps", C.c_float)]


class W2vWeights(C.Structure):
    _fields_ = [("resample_taps", vp), ("w_conv0", vp), ("b_conv0", vp), ("w_conv", vp * W2V_CONV_LAYERS), ("b_conv", vp * W2V_CONV_LAYERS),
                ("ln_conv_g", vp * W2V_CONV_LAYERS), ("ln_conv_b", vp * W2V_CONV_LAYERS), ("fp_ln_g", vp), ("fp_ln_b", vp), ("w_fp", vp),
                ("b_fp", vp), ("w_pos", vp), ("b_pos", vp), ("layers_host", C.POINTER(GptLayer)), ("lnf_g", vp), ("lnf_b", vp),
                ("w_head", vp), ("b_head", vp)]


CLS_DEPTH, CLS_RES_BLOCKS, CLS_ATTN_BLOCKS = 5, 2, 4


class ClsConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "spec_dim", "base_channels", "depth", "resnet_blocks", "kernel_size", "downsample_factor",
                                       "embedding_dim", "attn_blocks", "heads", "classes", "max_samples")]


class ClsResBlock(C.Structure):
    _fields_ = [(n, vp) for n in ("gn1_g", "gn1_b", "w1", "b1", "gn2_g", "gn2_b", "w2", "b2")]


class ClsAttn(C.Structure):
    _fields_ = [(n, vp) for n in ("norm_g", "norm_b", "w_qkv", "b_qkv", "w_proj", "b_proj")]


class ClsWeights(C.Structure):
    _fields_ = [("w_init", vp), ("b_init", vp), ("res", (ClsResBlock * CLS_RES_BLOCKS) * CLS_DEPTH), ("w_down", vp * CLS_DEPTH),
                ("b_down", vp * CLS_DEPTH), ("final_g", vp), ("final_b", vp), ("w_final", vp), ("b_final", vp),
                ("attn", ClsAttn * CLS_ATTN_BLOCKS), ("w_head", vp), ("b_head", vp)]


# include/tortoise_mi355x_classify.h, order == tt_cls_struct_size(which)
CLASSIFY_STRUCTS = [ClsConfig, ClsWeights]

MEL_MAX_CLIPS = 16


class MelConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_fft", "hop", "n_mels", "bins_pad", "power", "clamp_input")] + [("floor", C.c_float)] + [
        (n, C.c_int) for n in ("max_samples", "max_clips")]


class MelTables(C.Structure):
    _fields_ = [(n, vp) for n in ("basis", "fb", "scale")]


# include/tortoise_mi355x_mel.h, order == tt_mel_struct_size(which)
MEL_STRUCTS = [MelConfig, MelTables]

FMT_MAX_CLIPS, FMT_MAX_WARPS, FMT_Q_PAD = 16, 16, 64  # TT_FMT_MAX_CLIPS, TT_FMT_MAX_WARPS, TT_FMT_Q_PAD


class FmtConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_fft", "hop", "bins_pad", "q")] + [("max_gain_db", C.c_float)] + [
        (n, C.c_int) for n in ("max_samples", "max_clips", "n_warps")]


class FmtTables(C.Structure):
    _fields_ = [(n, vp) for n in ("basis", "inverse", "cepstrum", "warps")]


# include/tortoise_mi355x_fmt.h, order == tt_fmt_struct_size(which)
FMT_STRUCTS = [FmtConfig, FmtTables]
FMT_ABI_VERSION = 1

# include/tortoise_mi355x_nr.h: TT_NR_MAX_CLIPS, TT_NR_MAX_SAMPLES, TT_NR_MIN_FRAMES, TT_NR_MIN_REGION, TT_NR_QUANTILE_DEN, TT_NR_MAX_SMOOTH, TT_NR_REG_FRAMES
NR_MAX_CLIPS, NR_MAX_SAMPLES, NR_MIN_FRAMES, NR_MIN_REGION, NR_QUANTILE_DEN, NR_MAX_SMOOTH, NR_REG_FRAMES = 16, 4194304, 32, 8, 10000, 4, 1024
NR_OK, NR_SHORT, NR_REFUSED = 0, 1, 2  # TT_NR_OK, TT_NR_SHORT, TT_NR_REFUSED


class NrConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_fft", "hop", "bins_pad", "max_samples", "max_clips")]


class NrTables(C.Structure):
    _fields_ = [(n, vp) for n in ("basis", "inverse")]


class NrParams(C.Structure):
    _fields_ = [("quantile_num", C.c_int), ("quantile_scale", C.c_float), ("beta", C.c_float), ("g_min", C.c_float), ("smooth_frames", C.c_int),
                ("smooth_bins", C.c_int)]


# include/tortoise_mi355x_nr.h, order == tt_nr_struct_size(which)
NR_STRUCTS = [NrConfig, NrTables, NrParams]
NR_ABI_VERSION = 1

class GemmDesc(C.Structure):
    """tt_op_gemm_desc (include/tortoise_mi355x_test.h): every GEMM form of the operator-level test entry tt_op_gemm_ex."""
    _fields_ = [("A", vp), ("W", vp), ("A2", vp), ("a2_slot", vp), ("a2_slot_stride", C.c_size_t)] + [
        (n, C.c_int) for n in ("lda", "ldw", "lda2", "k_split", "M", "N", "K", "taps", "dilation", "seq_len", "splitk", "serial_k")] + [
        ("seq_vlen", vp), ("bias", vp), ("res", vp), ("out_f32", vp), ("out_t", vp)] + [
        (n, C.c_int) for n in ("act", "ldres", "ldo32", "ldot")] + [("slope", C.c_float), ("act_t", C.c_int), ("slope_t", C.c_float),
        ("gn_part", vp), ("gn_seq", C.c_int), ("gn_vperiod", C.c_int), ("gn_vlen", C.c_int * 32)] + [
        (n, C.c_int) for n in ("dmodel", "heads", "seq_pad", "tmax")] + [("q_scale", C.c_float)] + [
        (n, vp) for n in ("q", "k", "v", "vt", "step", "qbuf", "kc", "vc")]


class RowNormDesc(C.Structure):
    """tt_op_rownorm_desc (include/tortoise_mi355x_test.h): every row-norm form of the operator-level test entry tt_op_rownorm_ex."""
    _fields_ = [("x", vp), ("ldx", C.c_int), ("x_in", vp), ("ldxin", C.c_int), ("M", C.c_int), ("D", C.c_int), ("add_bias", vp), ("add_slabs", vp),
                ("nslab", C.c_int), ("slab_stride", C.c_size_t), ("ldslab", C.c_int), ("write_x", C.c_int), ("mode", C.c_int), ("g1", vp), ("b1", vp),
                ("eps1", C.c_float), ("g2", vp), ("b2", vp), ("eps2", C.c_float), ("out_t", vp), ("ldot", C.c_int), ("out_f32", vp), ("ldo32", C.c_int),
                ("f32_slot", vp), ("f32_slot_base", C.c_int), ("f32_slot_stride", C.c_size_t), ("f32_row_slot", vp), ("row_blocks", C.c_int),
                ("guard", vp), ("act", C.c_int)]


class GroupNormDesc(C.Structure):
    """tt_op_groupnorm_desc (include/tortoise_mi355x_test.h): every GroupNorm32 form of the operator-level test entry tt_op_groupnorm_ex."""
    _fields_ = [("x", vp), ("B", C.c_int), ("S", C.c_int), ("C", C.c_int), ("gamma", vp), ("beta", vp), ("eps", C.c_float), ("scale_shift", vp),
                ("ss_batch_stride", C.c_size_t), ("ss_batch_div", C.c_int), ("act", C.c_int), ("out_t", vp), ("ldot", C.c_int), ("out_f32", vp),
                ("ldo32", C.c_int), ("partial", vp), ("gemm_part", vp), ("part_rows", C.c_int), ("vperiod", C.c_int), ("vlen", C.c_int * 32),
                ("guard", vp)]


class Conv1dDesc(C.Structure):
    """tt_op_conv1d_desc (include/tortoise_mi355x_test.h): every argument of the audio-rate conv1d launch, the ragged batch included."""
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("y", vp)] + [(n, C.c_int) for n in ("Cin", "Cout", "T", "k", "dilation", "seq_n", "seq_mul")] + [
        ("seq_frames", C.c_int * 32), ("reflect", C.c_int), ("in_slope", C.c_float), ("out_act", C.c_int), ("out_slope", C.c_float)]


class ConvT1dDesc(C.Structure):
    """tt_op_convt1d_desc (include/tortoise_mi355x_test.h)"""
    _fields_ = [("x", vp), ("w", vp), ("bias", vp), ("y", vp), ("C", C.c_int), ("Tin", C.c_int), ("stride", C.c_int), ("in_slope", C.c_float),
                ("seq_n", C.c_int), ("seq_mul", C.c_int), ("seq_frames", C.c_int * 32)]


class LvcDesc(C.Structure):
    """tt_op_lvc_desc (include/tortoise_mi355x_test.h)"""
    _fields_ = [("x_in", vp), ("kernels", vp), ("ldk", C.c_int), ("koff", C.c_int), ("dtype", C.c_int), ("bias", vp), ("ldb", C.c_int),
                ("boff", C.c_int), ("x", vp), ("L", C.c_int), ("hop", C.c_int), ("seq_n", C.c_int), ("seq_mul", C.c_int),
                ("seq_frames", C.c_int * 32), ("in_slope", C.c_float), ("guard", vp)]


# tt_op_conv1d_ex / tt_op_lvc_ex `ran` records (csrc/ops.h VocRan)
CONV1D_KERNELS = {-1: "-", 0: "conv1d_direct_kernel<32>", 1: "conv1d_direct_kernel<1>", 2: "conv1d_mfma_kernel"}
LVC_KERNELS = {-1: "-", 0: "lvc_kernel", 1: "lvc_mfma_kernel"}
LVC_ELEM = {"f32": 0, "bf16": 1, "f16": 2}

# tt_op_rownorm_ex / tt_op_groupnorm_ex `ran` records (csrc/ops.h RowNormRan, GroupNormRan)
NORM_NONE, NORM_LAYER, NORM_RMS = 0, 1, 2
ROWNORM_KERNELS = {0: "generic", 1: "narrow", 2: "wave"}
GROUPNORM_APPLY = {0: "generic", 1: "c1024"}

# tt_op_gemm_ex `ran` record: tiles (gemm_impl.h Tile) and standard-epilogue variants (StdVariant)
GEMM_TILES = {0: "64x64", 1: "128x64", 2: "128x128", 3: "256x256", 4: "32x16", 5: "64x16"}
GEMM_VARIANTS = {-1: "-", 0: "V_GEN", 1: "V_NONE", 2: "V_SLAB", 3: "V_GELU_T", 4: "V_ST_F32", 5: "V_ST_RES", 6: "V_ST_A2", 7: "V_BIAS_T", 8: "V_SERIAL"}
EPI_STD, EPI_QKV_HEADS, EPI_QKV_DECODE, EPI_GEGLU = 0, 1, 2, 3

# tt_op_flash_ran record {kernel, NQ, KS} (csrc/ops.h FlashRan)
FLASH_KERNELS = {-1: "-", 0: "flash_kernel", 1: "flash_lds_kernel", 2: "flash32_kernel", 3: "flash_f32_kernel"}

# include/tortoise_mi355x_hifi.h, order == tt_hifi_batch_struct_size(which)
HIFI_BATCH_STRUCTS = [HifiConfig, HifiWeights, HifiResBlock]
HIFI_MAX_BATCH = 64  # TT_HIFI_MAX_BATCH

# include/tortoise_mi355x_univnet.h, order == tt_voc_batch_struct_size(which)
VOC_BATCH_STRUCTS = [VocConfig, VocWeights, VocBlock]
VOC_MAX_BATCH = 32  # TT_VOC_MAX_BATCH

# include/tortoise_mi355x_align.h, order == tt_align_struct_size(which)
ALIGN_STRUCTS = [W2vConfig, W2vWeights]

# order == tt_struct_size(which)
BOUNDARY_STRUCTS = [GptLayer, ArConfig, ArWeights, Sampling, ClvpLayer, ClvpTower, ClvpConfig, AttnBlock, ResBlock, DiffConfig,
                    DiffWeights, DiffStep, VocBlock, VocConfig, VocWeights, CondConfig, CondWeights, HifiResBlock, HifiConfig, HifiWeights,
                    CvvpTower, CvvpConfig, CvvpWeights]

_i, _f, _sz = C.c_int, C.c_float, C.c_size_t
_PROTOS = {
    "tt_last_error": (C.c_char_p, []),
    "tt_init": (_i, []),
    "tt_abi_version": (_i, []),
    "tt_struct_size": (_sz, [_i]),
    "tt_ar_create": (_i, [C.POINTER(ArConfig), C.POINTER(ArWeights), C.POINTER(vp)]),
    "tt_ar_destroy": (None, [vp]),
    "tt_ar_prefill": (_i, [vp, vp, _i, vp]),
    "tt_ar_prefill_group": (_i, [vp, _i, _i, vp, _i, vp]),
    "tt_ar_get_logits": (_i, [vp, vp, _i, vp]),
    "tt_ar_generate": (_i, [vp, _i, _i, C.POINTER(Sampling), vp, C.POINTER(_i), vp]),
    "tt_ar_generate_chunk": (_i, [vp, _i, _i, _i, _i, C.POINTER(Sampling), vp, C.POINTER(_i), C.POINTER(_i), vp]),
    "tt_ar_begin": (_i, [vp, _i, vp]),
    "tt_ar_decode_step": (_i, [vp, vp, vp]),
    "tt_ar_latents": (_i, [vp, vp, _i, _i, vp, vp]),
    "tt_ar_stream_latents": (_i, [vp, _i, _i, vp, vp]),
    "tt_ar_set_option": (_i, [vp, _i, _i]),
    "tt_ar_guard": (_i, [vp, _i]),
    "tt_ar_stat": (_i, [vp, _i]),
    "tt_diff_stat": (_i, [vp, _i]),
    "tt_diff_set_option": (_i, [vp, _i, _i]),
    "tt_clvp_guard": (_i, [vp, _i]),
    "tt_diff_guard": (_i, [vp, _i]),
    "tt_clvp_create": (_i, [C.POINTER(ClvpConfig), C.POINTER(ClvpTower), C.POINTER(ClvpTower), vp, C.POINTER(vp)]),
    "tt_clvp_destroy": (None, [vp]),
    "tt_clvp_score": (_i, [vp, vp, _i, vp, _i, _i, vp, vp]),
    "tt_clvp_score_groups": (_i, [vp, vp, C.POINTER(_i), _i, vp, _i, _i, vp, vp]),
    "tt_diff_create": (_i, [C.POINTER(DiffConfig), C.POINTER(DiffWeights), C.POINTER(vp)]),
    "tt_diff_destroy": (None, [vp]),
    "tt_diff_condition": (_i, [vp, vp, _i, vp, vp, _i, vp]),
    "tt_diff_get_code_emb": (_i, [vp, vp, vp]),
    "tt_diff_forward": (_i, [vp, vp, _i, _i, vp, vp]),
    "tt_diff_sample": (_i, [vp, vp, vp, C.POINTER(DiffStep), _i, _i, vp, vp]),
    "tt_diff_batch_begin": (_i, [vp, _i, _i, vp]),
    "tt_diff_condition_slot": (_i, [vp, _i, vp, _i, vp, vp, _i, vp]),
    "tt_diff_sample_batch": (_i, [vp, _i, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(DiffStep), _i, _i, C.POINTER(C.c_void_p), vp]),
    "tt_diff_split_begin": (_i, [vp, vp, C.POINTER(DiffStep), _i, _i, vp]),
    "tt_diff_split_forward": (_i, [vp, vp, vp]),
    "tt_diff_split_update": (_i, [vp, vp, vp, vp, vp]),
    "tt_diff_split_end": (_i, [vp]),
    "tt_cond_create": (_i, [C.POINTER(CondConfig), C.POINTER(CondWeights), C.POINTER(vp)]),
    "tt_cond_destroy": (None, [vp]),
    "tt_cond_ar_clip": (_i, [vp, vp, _i, vp, vp]),
    "tt_cond_diff_clip": (_i, [vp, vp, _i, vp, C.POINTER(_i), vp]),
    "tt_hifi_create": (_i, [C.POINTER(HifiConfig), C.POINTER(HifiWeights), C.POINTER(vp)]),
    "tt_hifi_destroy": (None, [vp]),
    "tt_hifi_output_frames": (_i, [_i]),
    "tt_hifi_run": (_i, [vp, vp, _i, vp, vp, C.POINTER(_i), vp]),
    "tt_voc_create": (_i, [C.POINTER(VocConfig), C.POINTER(VocWeights), C.POINTER(vp)]),
    "tt_voc_destroy": (None, [vp]),
    "tt_voc_run": (_i, [vp, vp, _i, vp, vp, vp]),
    "tt_voc_guard": (_i, [vp, _i]),
    "tt_cvvp_create": (_i, [C.POINTER(CvvpConfig), C.POINTER(CvvpWeights), C.POINTER(vp)]),
    "tt_cvvp_destroy": (None, [vp]),
    "tt_cvvp_score": (_i, [vp, vp, _i, _i, vp, _i, _i, vp, vp]),
    "tt_cvvp_guard": (_i, [vp, _i]),
    "tt_prof_enable": (_i, [_i]),
    "tt_graph_replay": (_i, [_i]),
    "tt_prof_classes": (_i, []),
    "tt_prof_class_name": (C.c_char_p, [_i]),
    "tt_prof_read": (_i, [_i, C.POINTER(C.c_double)]),
}
# include/tortoise_mi355x_align.h: the wav2vec2 aligner of the redaction path (its own header and version, same library)
_ALIGN_PROTOS = {
    "tt_align_abi_version": (_i, []),
    "tt_align_struct_size": (_sz, [_i]),
    "tt_w2v_create": (_i, [C.POINTER(W2vConfig), C.POINTER(W2vWeights), C.POINTER(vp)]),
    "tt_w2v_destroy": (None, [vp]),
    "tt_w2v_frames": (_i, [vp, _i]),
    "tt_w2v_run": (_i, [vp, vp, _i, vp, vp, vp]),
    "tt_w2v_guard": (_i, [vp, _i]),
}
# include/tortoise_mi355x_classify.h: the Tortoise detector (classify_audio_clip; its own header and version, same library)
_CLASSIFY_PROTOS = {
    "tt_cls_abi_version": (_i, []),
    "tt_cls_struct_size": (_sz, [_i]),
    "tt_cls_max_samples": (_i, []),
    "tt_cls_create": (_i, [C.POINTER(ClsConfig), C.POINTER(ClsWeights), C.POINTER(vp)]),
    "tt_cls_destroy": (None, [vp]),
    "tt_cls_run": (_i, [vp, vp, _i, vp, vp, vp]),
    "tt_cls_guard": (_i, [vp, _i]),
}
# include/tortoise_mi355x_mel.h: the mel front-end of the voice_samples path (its own header and version, same library)
_ll = C.c_longlong
_MEL_PROTOS = {
    "tt_mel_abi_version": (_i, []),
    "tt_mel_struct_size": (_sz, [_i]),
    "tt_mel_create": (_i, [C.POINTER(MelConfig), C.POINTER(MelTables), C.POINTER(vp)]),
    "tt_mel_destroy": (None, [vp]),
    "tt_mel_frames": (_i, [vp, _i]),
    "tt_mel_run": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), _i, vp, C.POINTER(_ll), vp]),
    "tt_mel_spectrum": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), _i, vp, C.POINTER(_ll), vp]),
    "tt_mel_resampler_create": (_i, [vp, _i, _i, _i, _i, C.POINTER(vp)]),
    "tt_mel_resampler_destroy": (None, [vp]),
    "tt_mel_resampled_length": (_i, [vp, _i]),
    "tt_mel_resample": (_i, [vp, vp, _i, vp, vp]),
}
# include/tortoise_mi355x_ctc.h: CTC forced alignment over the aligner's logits (its own header and version, same library)
_CTC_PROTOS = {
    "tt_ctc_abi_version": (_i, []),
    "tt_ctc_create": (_i, [_i, _i, _i, _i, _i, C.POINTER(vp)]),
    "tt_ctc_destroy": (None, [vp]),
    "tt_ctc_align": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
CTC_ABI_VERSION = 1
CTC_MAX_TOKENS = 511  # TT_CTC_MAX_TOKENS
CTC_OK, CTC_INFEASIBLE, CTC_EMPTY, CTC_REFUSED = 0, 1, 2, 3
# include/tortoise_mi355x_tsm.h: WSOLA time-stretch of rendered clips (its own header and version, same library)
_TSM_PROTOS = {
    "tt_tsm_abi_version": (_i, []),
    "tt_tsm_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_tsm_destroy": (None, [vp]),
    "tt_tsm_out_samples": (_i, [_i, _i]),
    "tt_tsm_frames": (_i, [_i, _i]),
    "tt_tsm_stretch": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
TSM_ABI_VERSION = 1
TSM_WINDOW, TSM_HOP, TSM_SEARCH = 768, 384, 256  # TT_TSM_WINDOW, TT_TSM_HOP, TT_TSM_SEARCH
TSM_RATE_ONE, TSM_RATE_MIN, TSM_RATE_MAX = 65536, 32768, 131072  # TT_TSM_RATE_*: 16.16 fixed point, rates 0.5 .. 2.0
TSM_SAMPLE_RATE = 24000
TSM_MAX_SAMPLES, TSM_MAX_CLIPS = 8388608, 64
TSM_OK, TSM_EMPTY, TSM_REFUSED = 0, 1, 2
# include/tortoise_mi355x_loud.h: loudness measurement, normalisation and true-peak limiting of rendered clips (its own header and version)
_LOUD_PROTOS = {
    "tt_loud_abi_version": (_i, []),
    "tt_loud_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_loud_destroy": (None, [vp]),
    "tt_loud_hops": (_i, [_i]),
    "tt_loud_blocks": (_i, [_i]),
    "tt_loud_measure": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tt_loud_normalize": (_i, [vp, _i, vp, vp, vp, vp, vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
LOUD_ABI_VERSION = 1
LOUD_HOP, LOUD_BLOCK, LOUD_SEGMENT, LOUD_LOOKAHEAD = 2400, 9600, 150, 120  # TT_LOUD_HOP, TT_LOUD_BLOCK, TT_LOUD_SEGMENT, TT_LOUD_LOOKAHEAD
LOUD_OVERSAMPLE, LOUD_TAPS = 4, 16
LOUD_SAMPLE_RATE = 24000
LOUD_MAX_SAMPLES, LOUD_MAX_CLIPS = 268435456, 64
LOUD_NONE, LOUD_SCALE, LOUD_LOOKAHEAD_MODE = 0, 1, 2
LOUD_OK, LOUD_SHORT, LOUD_SILENT, LOUD_EMPTY, LOUD_REFUSED = 0, 1, 2, 3, 4
# include/tortoise_mi355x_rs.h: arbitrary-ratio band-limited resampler of rendered clips: pitch and output sample rate (its own header and version)
_RS_PROTOS = {
    "tt_rs_abi_version": (_i, []),
    "tt_rs_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_rs_destroy": (None, [vp]),
    "tt_rs_out_samples": (_i, [_i, _i, _i]),
    "tt_rs_resample": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
RS_ABI_VERSION = 1
RS_ZEROS, RS_PER_ZERO, RS_TABLE, RS_BETA = 32, 512, 16385, 10  # TT_RS_ZEROS, TT_RS_PER_ZERO, TT_RS_TABLE, TT_RS_BETA
RS_RHO_NUM, RS_RHO_DEN = 9, 10
RS_PITCH_ONE = 65536
RS_MAX_TERM, RS_MAX_RATIO = 1048576, 8
RS_MAX_SAMPLES, RS_MAX_CLIPS = 8388608, 64
RS_OK, RS_EMPTY, RS_REFUSED = 0, 1, 2
# include/tortoise_mi355x_rss.h: the resampler fed in chunks, for streams at another sample rate (its own header and version)
_ip = C.POINTER(_i)
_RSS_PROTOS = {
    "tt_rss_abi_version": (_i, []),
    "tt_rss_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_rss_destroy": (None, [vp]),
    "tt_rss_open": (_i, [vp, _i, _i, _i, vp]),
    "tt_rss_close": (_i, [vp, _i]),
    "tt_rss_state": (_i, [vp, _i, _ip, _ip, _ip, _ip]),
    "tt_rss_ready": (_i, [_i, _i, _i, _i, _i]),
    "tt_rss_push": (_i, [vp, _i, _ip, _ip, _ip, vp, vp, vp]),
}
RSS_ABI_VERSION = 1
RSS_HIST, RSS_MAX_STREAMS, RSS_BANK_MAX, RSS_AUTO_MAX_Q = 576, 64, 16384, 16  # TT_RSS_HIST, TT_RSS_MAX_STREAMS, TT_RSS_BANK_MAX, TT_RSS_AUTO_MAX_Q
RSS_AUTO, RSS_TABLE, RSS_BANK = 0, 1, 2
# include/tortoise_mi355x_lvs.h: the streaming leveler - causal loudness, a slew-limited gain, the look-ahead limiter (its own header and version)
_fl = C.c_float
_LVS_PROTOS = {
    "tt_lvs_abi_version": (_i, []),
    "tt_lvs_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_lvs_destroy": (None, [vp]),
    "tt_lvs_open": (_i, [vp, _i, _i, _i, _fl, _fl, _fl, _fl, _fl, _fl, _fl]),
    "tt_lvs_close": (_i, [vp, _i]),
    "tt_lvs_state": (_i, [vp, _i, _ip, _ip, _ip, _ip]),
    "tt_lvs_ready": (_i, [_i, _i, _i, _i]),
    "tt_lvs_push": (_i, [vp, _i, _ip, _ip, _ip, vp, vp, vp]),
    "tt_lvs_read": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tt_lvs_trace": (_i, [vp, _i, _i, _i, vp, vp, vp, vp, vp, vp, vp]),
}
LVS_ABI_VERSION = 1
LVS_MAX_STREAMS, LVS_DELAY, LVS_HIST, LVS_TILE = 64, 248, 512, 1024  # TT_LVS_MAX_STREAMS, TT_LVS_DELAY, TT_LVS_HIST, TT_LVS_TILE
LVS_DEFAULT_HOPS, LVS_MAX_HOPS = 36000, 864000
LVS_ADAPT, LVS_FIXED = 0, 1
LVS_NONE, LVS_LOOKAHEAD = 0, 1
# include/tortoise_mi355x_rsw.h: the resampler along a pitch map, a pitch that changes inside the clip (its own header and version)
_RSW_PROTOS = {
    "tt_rsw_abi_version": (_i, []),
    "tt_rsw_plan": (_i, [_i, _i, _ip, _ip, _ip]),
    "tt_rsw_out_samples": (_i, [_i, _i, _ip]),
    "tt_rsw_create": (_i, [_i, _i, _i, C.POINTER(vp)]),
    "tt_rsw_destroy": (None, [vp]),
    "tt_rsw_resample": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
RSW_ABI_VERSION = 1
RSW_MAX_SEGMENTS, RSW_MIN_SEGMENT = 64, 2  # TT_RSW_MAX_SEGMENTS, TT_RSW_MIN_SEGMENT
RSW_P_MIN, RSW_P_MAX = 32768, 131072       # TT_RSW_P_MIN, TT_RSW_P_MAX
RSW_OK, RSW_EMPTY, RSW_REFUSED = 0, 1, 2

# include/tortoise_mi355x_tss.h: the time-stretch fed in chunks, for streams at another speaking rate and pitch (its own header and version)
_TSS_PROTOS = {
    "tt_tss_abi_version": (_i, []),
    "tt_tss_create": (_i, [_i, C.POINTER(vp)]),
    "tt_tss_destroy": (None, [vp]),
    "tt_tss_open": (_i, [vp, _i, _i]),
    "tt_tss_close": (_i, [vp, _i]),
    "tt_tss_state": (_i, [vp, _i, _ip, _ip, _ip, _ip]),
    "tt_tss_frames_done": (_i, [_i, _i]),
    "tt_tss_ready": (_i, [_i, _i, _i, _i]),
    "tt_tss_push": (_i, [vp, _i, _ip, _ip, _ip, vp, vp, vp, vp]),
}
TSS_ABI_VERSION = 1
TSS_LOOK, TSS_HIST, TSS_MAX_STREAMS = 1407, 1664, 64  # TT_TSS_LOOK, TT_TSS_HIST, TT_TSS_MAX_STREAMS
# include/tortoise_mi355x_tsw.h: the time-stretch along a rate map, a speaking rate that changes inside the clip (its own header and version)
_TSW_PROTOS = {
    "tt_tsw_abi_version": (_i, []),
    "tt_tsw_plan": (_i, [_i, _i, _ip, _ip, _ip]),
    "tt_tsw_out_samples": (_i, [_i, _i, _ip]),
    "tt_tsw_frames": (_i, [_i, _i, _ip]),
    "tt_tsw_create": (_i, [_i, _i, _i, C.POINTER(vp)]),
    "tt_tsw_destroy": (None, [vp]),
    "tt_tsw_stretch": (_i, [vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
TSW_ABI_VERSION = 1
TSW_MAX_SEGMENTS, TSW_MIN_SEGMENT = 64, 2  # TT_TSW_MAX_SEGMENTS, TT_TSW_MIN_SEGMENT
TSW_OK, TSW_EMPTY, TSW_REFUSED = 0, 1, 2
# include/tortoise_mi355x_sil.h: speech regions, edge trimming and pause capping of rendered clips (its own header and version)
_SIL_PROTOS = {
    "tt_sil_abi_version": (_i, []),
    "tt_sil_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_sil_destroy": (None, [vp]),
    "tt_sil_frames": (_i, [_i]),
    "tt_sil_max_regions": (_i, [_i]),
    "tt_sil_find": (_i, [vp, _i] + [vp] * 12),
    "tt_sil_trim": (_i, [vp, _i] + [vp] * 15),
}
SIL_ABI_VERSION = 1
SIL_SLOT, SIL_HOP, SIL_FRAME, SIL_FADE = 120, 240, 480, 120  # TT_SIL_SLOT, TT_SIL_HOP, TT_SIL_FRAME, TT_SIL_FADE
SIL_SAMPLE_RATE = 24000
SIL_MAX_SAMPLES, SIL_MAX_CLIPS = 8388608, 64
SIL_MAX_FRAMES_PARAM = 6000
SIL_OK, SIL_UNCHANGED, SIL_SILENT, SIL_EMPTY, SIL_REFUSED = 0, 1, 2, 3, 4
# include/tortoise_mi355x_f0.h: the YIN fundamental-frequency tracker over ragged batches (its own header and version)
_F0_PROTOS = {
    "tt_f0_abi_version": (_i, []),
    "tt_f0_create": (_i, [_i, _i, C.POINTER(vp)]),
    "tt_f0_destroy": (None, [vp]),
    "tt_f0_frames": (_i, [_i]),
    "tt_f0_lags": (_i, [C.c_double, C.c_double, _ip, _ip]),
    "tt_f0_track": (_i, [vp, _i] + [vp] * 11),
}
F0_ABI_VERSION = 1
F0_HOP, F0_WINDOW, F0_LEAD, F0_LAG_MIN, F0_LAG_MAX = 240, 960, 720, 24, 480  # TT_F0_HOP, TT_F0_WINDOW, TT_F0_LEAD, TT_F0_LAG_MIN, TT_F0_LAG_MAX
F0_SAMPLE_RATE = 24000
F0_MAX_SAMPLES, F0_MAX_CLIPS = 8388608, 64
F0_OK, F0_EMPTY, F0_REFUSED = 0, 1, 2
# include/tortoise_mi355x_f0v.h: the Viterbi path over YIN candidates (its own header and version, same library)
_F0V_PROTOS = {
    "tt_f0v_abi_version": (_i, []),
    "tt_f0v_create": (_i, [_i, _i, C.POINTER(C.c_double), C.POINTER(vp)]),
    "tt_f0v_destroy": (None, [vp]),
    "tt_f0v_track": (_i, [vp, _i] + [vp] * 14),
}
F0V_ABI_VERSION = 1
F0V_STATES, F0V_UNVOICED, F0V_TABLE = 8, 7, 481  # TT_F0V_STATES, TT_F0V_UNVOICED, TT_F0V_TABLE
# include/tortoise_mi355x_nr.h: the spectral-subtraction denoiser of voice clips (its own header and version, same library)
_NR_PROTOS = {
    "tt_nr_abi_version": (_i, []),
    "tt_nr_struct_size": (_sz, [_i]),
    "tt_nr_create": (_i, [C.POINTER(NrConfig), C.POINTER(NrTables), C.POINTER(vp)]),
    "tt_nr_destroy": (None, [vp]),
    "tt_nr_frames": (_i, [vp, _i]),
    "tt_nr_rank": (_i, [_i, _i]),
    "tt_nr_region": (_i, [_ll, _ll, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "tt_nr_run": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(NrParams), _i, vp, C.POINTER(_ll), vp, C.POINTER(_i), vp]),
}

# include/tortoise_mi355x_fmt.h: formant-preserving pitch, the cepstral envelope correction (its own header and version, same library)
_FMT_PROTOS = {
    "tt_fmt_abi_version": (_i, []),
    "tt_fmt_struct_size": (_sz, [_i]),
    "tt_fmt_create": (_i, [C.POINTER(FmtConfig), C.POINTER(FmtTables), C.POINTER(vp)]),
    "tt_fmt_destroy": (None, [vp]),
    "tt_fmt_frames": (_i, [vp, _i]),
    "tt_fmt_run": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), _i, vp, C.POINTER(_ll), vp]),
}
# include/tortoise_mi355x_solver.h: DDIM / DPM-Solver++(2M) on a tt_diff handle (its own header and version, same library)
_SOLVER_PROTOS = {
    "tt_solver_abi_version": (_i, []),
    "tt_diff_solve": (_i, [vp, vp, C.POINTER(SolverStep), _i, _i, vp, vp]),
    "tt_diff_solve_batch": (_i, [vp, _i, C.POINTER(C.c_void_p), C.POINTER(SolverStep), _i, _i, C.POINTER(C.c_void_p), vp]),
    "tt_diff_solve_stat": (_i, [vp, _i]),
    "tt_op_solver_update": (_i, [_i, vp, vp, _i, _i, vp, C.POINTER(SolverStep), _i, _i, _i, vp, vp, vp, vp]),
}
SOLVER_ABI_VERSION = 1
# include/tortoise_mi355x_hifi.h: ragged batches of the HiFi-GAN decoder (its own header and version, same library)
_HIFI_PROTOS = {
    "tt_hifi_batch_abi_version": (_i, []),
    "tt_hifi_batch_struct_size": (_sz, [_i]),
    "tt_hifi_batch_capacity": (_i, [vp]),
    "tt_hifi_run_batch": (_i, [vp, _i, vp, C.POINTER(_i), vp, vp, vp]),
}
# include/tortoise_mi355x_univnet.h: ragged batches of the UnivNet vocoder (its own header and version, same library)
_UNIVNET_PROTOS = {
    "tt_voc_batch_abi_version": (_i, []),
    "tt_voc_batch_struct_size": (_sz, [_i]),
    "tt_voc_batch_capacity": (_i, [vp]),
    "tt_voc_run_batch": (_i, [vp, _i, C.POINTER(C.c_void_p), C.POINTER(_i), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), vp]),
}
# include/tortoise_mi355x_test.h: operator-level TEST entries + the A/B switch (not part of the boundary a maintainer binds)
_TEST_PROTOS = {
    "ttx_kernel_variant": (_i, [_i, _i]),
    "tt_op_gemm": (_i, [_i, vp, _i, vp, _i, _i, _i, _i, _i, _i, _i, vp, _i, vp, vp, vp, vp]),
    "tt_op_gemm_segv": (_i, [_i, vp, _i, vp, _i, _i, _i, _i, _i, _i, _i, vp, vp, _i, vp, vp, vp, vp]),
    "tt_op_gemm_desc_size": (_sz, []),
    "tt_op_gemm_ex": (_i, [_i, _i, C.POINTER(GemmDesc), C.POINTER(_i), vp]),
    "tt_op_gemm_stat_rows": (_i, [_i, C.POINTER(GemmDesc)]),
    "tt_op_rownorm_desc_size": (_sz, []),
    "tt_op_rownorm_ex": (_i, [_i, C.POINTER(RowNormDesc), C.POINTER(_i), vp]),
    "tt_op_groupnorm_desc_size": (_sz, []),
    "tt_op_groupnorm_ex": (_i, [_i, C.POINTER(GroupNormDesc), C.POINTER(_i), vp]),
    "tt_op_groupnorm_part": (_i, [_i, vp, _i, _i, _i, vp, vp, vp, _i, vp, _i, _i, C.POINTER(_i), vp, vp, vp, vp]),
    "tt_op_layernorm": (_i, [_i, vp, _i, _i, vp, vp, _f, _i, vp, vp, vp]),
    "tt_op_groupnorm": (_i, [_i, vp, _i, _i, _i, vp, vp, vp, _i, vp, vp, vp, vp]),
    "tt_op_groupnorm_workspace": (_sz, [_i, _i]),
    "tt_op_gn_gemm": (_i, [_i, vp, _i, _i, vp, vp, _i, vp, vp, _i, vp, vp, vp]),
    "tt_op_gn_gemm_workspace": (_sz, [_i, _i]),
    "tt_op_flash_attention": (_i, [_i, vp, vp, vp, vp, _i, _i, _i, _i, _i, vp, vp]),
    "tt_op_flash_attention_rows": (_i, [_i, vp, vp, vp, vp, _i, _i, _i, _i, _i, vp, vp, _i, _i, vp]),
    "tt_op_flash_ran": (_i, [C.POINTER(_i)]),
    "tt_op_decode_attention": (_i, [_i, vp, vp, vp, _i, vp, vp, _i, _i, vp, _i, _i, _i, vp]),
    "tt_op_decode_qkv_attention": (_i, [_i, vp, vp, vp, C.c_float, vp, vp, _i, vp, vp, _i, _i, vp, vp, _i, _i, vp]),
    "tt_op_decode_attention_rows": (_i, [_i, vp, vp, vp, C.c_longlong, vp, _i, vp, vp, _i, vp, vp, _i, _i, vp]),
    "tt_op_gemv": (_i, [_i, vp, vp, _i, _i, _i, vp, _i, vp, vp, vp]),
    "tt_op_gemv_ln": (_i, [_i, vp, vp, vp, _f, vp, _i, _i, vp, vp, vp]),
    "tt_op_sample": (_i, [vp, _i, _i, _i, vp, C.POINTER(Sampling), _i, vp, _i, vp, _i, vp]),
    "tt_op_typical_mask": (_i, [vp, _i, _i, _i, vp, _f, _f, vp, vp]),
    "tt_op_conv1d": (_i, [vp, vp, vp, vp, _i, _i, _i, _i, _i, _i, _f, _i, _f, vp]),
    "tt_op_convt1d": (_i, [vp, vp, vp, vp, _i, _i, _i, _f, vp]),
    "tt_op_lvc": (_i, [_i, vp, vp, _i, _i, vp, _i, _i, vp, _i, _i, vp]),
    "tt_op_conv1d_desc_size": (_sz, []),
    "tt_op_conv1d_ex": (_i, [C.POINTER(Conv1dDesc), C.POINTER(_i), vp]),
    "tt_op_convt1d_desc_size": (_sz, []),
    "tt_op_convt1d_ex": (_i, [C.POINTER(ConvT1dDesc), C.POINTER(_i), vp]),
    "tt_op_lvc_desc_size": (_sz, []),
    "tt_op_lvc_ex": (_i, [C.POINTER(LvcDesc), C.POINTER(_i), vp]),
    "tt_op_w2v_resample_workspace": (_sz, [_i]),
    "tt_op_w2v_resample": (_i, [vp, _i, vp, vp, vp, vp, vp]),
    "tt_op_w2v_conv0": (_i, [_i, vp, vp, _i, _i, _i, vp, vp, vp, vp, vp, vp, vp]),
    "tt_op_layernorm_act": (_i, [_i, vp, _i, _i, vp, vp, _f, _i, vp, vp, vp]),
    "tt_op_w2v_argmax": (_i, [vp, _i, _i, _i, vp, vp, vp]),
    "tt_op_cls_workspace": (_sz, [_i]),
    "tt_op_cls_init": (_i, [vp, _i, vp, vp, vp, vp, vp]),
    "tt_op_cls_stats": (_i, [vp, _i, _i, _i, vp, vp]),
    "tt_op_cls_conv": (_i, [_i, _i, _i, _i, vp, _i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "tt_op_cls_attention": (_i, [_i, vp, _i, _i, vp, vp]),
    "tt_op_cls_head": (_i, [vp, vp, vp, vp, vp, vp]),
    "tt_op_fmt_run": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), _i, vp, C.POINTER(_ll), vp, vp, vp, C.POINTER(_ll), vp]),
    "tt_op_fmt_synth": (_i, [vp, vp, vp, C.POINTER(_ll), C.POINTER(_i), _i, vp, C.POINTER(_ll), vp]),
    "tt_op_nr_run": (_i, [vp, vp, C.POINTER(_ll), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(NrParams), _i, vp, C.POINTER(_ll), vp, C.POINTER(_i),
                          vp, vp, vp, C.POINTER(_ll), vp]),
    "tt_op_f0_track": (_i, [vp, _i] + [vp] * 12),
    "tt_op_f0_group": (_i, []),
    "tt_op_f0v_candidates": (_i, [vp, _i] + [vp] * 10),
    "tt_op_f0v_path": (_i, [vp, _i] + [vp] * 15),
}

_lib = None
_initialised = False


def load_library():
    """dlopen the engine and declare every prototype.  Needs no GPU (ABI checks run on CPU)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError("MI355X engine library not built: %s is missing. Run `python -m tortoise_tts_amd.build` "
                          "(hipcc, gfx950). There is no fallback path." % LIB_PATH)
    # torch must be loaded first: the engine shares device pointers and streams with PyTorch-ROCm, so
    # both have to bind to the ONE HIP runtime that torch ships (libamdhip64.so.7, resolved by SONAME).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(_PROTOS.items()) + list(_TEST_PROTOS.items()) + list(_ALIGN_PROTOS.items()) + list(_CLASSIFY_PROTOS.items()) + \
            list(_MEL_PROTOS.items()) + list(_CTC_PROTOS.items()) + list(_TSM_PROTOS.items()) + list(_LOUD_PROTOS.items()) + list(_LVS_PROTOS.items()) + list(_RS_PROTOS.items()) + list(_RSS_PROTOS.items()) + list(_RSW_PROTOS.items()) + list(_TSS_PROTOS.items()) + list(_TSW_PROTOS.items()) + list(_SIL_PROTOS.items()) + list(_F0_PROTOS.items()) + list(_F0V_PROTOS.items()) + list(_FMT_PROTOS.items()) + list(_NR_PROTOS.items()) + list(_SOLVER_PROTOS.items()) + list(_HIFI_PROTOS.items()) + list(_UNIVNET_PROTOS.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for i, st in enumerate(BOUNDARY_STRUCTS):
        want = lib.tt_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(ALIGN_STRUCTS):
        want = lib.tt_align_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(HIFI_BATCH_STRUCTS):
        want = lib.tt_hifi_batch_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(VOC_BATCH_STRUCTS):
        want = lib.tt_voc_batch_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(CLASSIFY_STRUCTS):
        want = lib.tt_cls_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(MEL_STRUCTS):
        want = lib.tt_mel_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    for i, st in enumerate(FMT_STRUCTS):
        want = lib.tt_fmt_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    if lib.tt_fmt_abi_version() != FMT_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_fmt.h is version %d in the library, %d in Python" % (lib.tt_fmt_abi_version(), FMT_ABI_VERSION))
    for i, st in enumerate(NR_STRUCTS):
        want = lib.tt_nr_struct_size(i)
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    if lib.tt_nr_abi_version() != NR_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_nr.h is version %d in the library, %d in Python" % (lib.tt_nr_abi_version(), NR_ABI_VERSION))
    if lib.tt_ctc_abi_version() != CTC_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_ctc.h is version %d in the library, %d in Python" % (lib.tt_ctc_abi_version(), CTC_ABI_VERSION))
    if lib.tt_tsm_abi_version() != TSM_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_tsm.h is version %d in the library, %d in Python" % (lib.tt_tsm_abi_version(), TSM_ABI_VERSION))
    if lib.tt_loud_abi_version() != LOUD_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_loud.h is version %d in the library, %d in Python" % (lib.tt_loud_abi_version(), LOUD_ABI_VERSION))
    if lib.tt_rs_abi_version() != RS_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_rs.h is version %d in the library, %d in Python" % (lib.tt_rs_abi_version(), RS_ABI_VERSION))
    if lib.tt_lvs_abi_version() != LVS_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_lvs.h is version %d in the library, %d in Python" % (lib.tt_lvs_abi_version(), LVS_ABI_VERSION))
    if lib.tt_rss_abi_version() != RSS_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_rss.h is version %d in the library, %d in Python" % (lib.tt_rss_abi_version(), RSS_ABI_VERSION))
    if lib.tt_rsw_abi_version() != RSW_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_rsw.h is version %d in the library, %d in Python" % (lib.tt_rsw_abi_version(), RSW_ABI_VERSION))
    if lib.tt_tss_abi_version() != TSS_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_tss.h is version %d in the library, %d in Python" % (lib.tt_tss_abi_version(), TSS_ABI_VERSION))
    if lib.tt_tsw_abi_version() != TSW_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_tsw.h is version %d in the library, %d in Python" % (lib.tt_tsw_abi_version(), TSW_ABI_VERSION))
    if lib.tt_sil_abi_version() != SIL_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_sil.h is version %d in the library, %d in Python" % (lib.tt_sil_abi_version(), SIL_ABI_VERSION))
    if lib.tt_f0_abi_version() != F0_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_f0.h is version %d in the library, %d in Python" % (lib.tt_f0_abi_version(), F0_ABI_VERSION))
    if lib.tt_f0v_abi_version() != F0V_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_f0v.h is version %d in the library, %d in Python" % (lib.tt_f0v_abi_version(), F0V_ABI_VERSION))
    if lib.tt_solver_abi_version() != SOLVER_ABI_VERSION:
        raise EngineError("ABI mismatch: tortoise_mi355x_solver.h is version %d in the library, %d in Python" % (lib.tt_solver_abi_version(), SOLVER_ABI_VERSION))
    for st, want in ((GemmDesc, lib.tt_op_gemm_desc_size()), (RowNormDesc, lib.tt_op_rownorm_desc_size()), (GroupNormDesc, lib.tt_op_groupnorm_desc_size())):
        if C.sizeof(st) != want:
            raise EngineError("ABI mismatch: %s is %d bytes in Python, %d in the library" % (st.__name__, C.sizeof(st), want))
    _lib = lib
    return lib


def init():
    """Load the library and initialise it on the current HIP device (must be gfx950)."""
    global _initialised
    lib = load_library()
    if not _initialised:
        check(lib.tt_init())
        # process-wide kernel A/B switches (diagnostics; the defaults are the measured winners)
        for env, which in (("TT_GEMM_VARIANT", TTX_GEMM_P8), ("TT_FLASH_VARIANT", TTX_FLASH32), ("TT_VOC_VARIANT", TTX_VOC_MFMA), ("TT_GEMM_SKINNY", TTX_GEMM_SKINNY), ("TT_AR_GEMV", TTX_AR_GEMV)):
            if os.environ.get(env, "") != "":
                lib.ttx_kernel_variant(which, int(os.environ[env]))
        _initialised = True
    return lib


def require_gpu(device=None):
    """The torch.device the engine will run on; raises EngineError unless it is a HIP/ROCm GPU (there is no CPU path)."""
    import torch
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise EngineError("TextToSpeech needs an MI355X (gfx950) device; the engine has no CPU path")
    return torch.device(device)


class OperandOverflow(EngineError):
    """A stage's overflow guard tripped: non-finite values downstream of an MFMA operand cast (fp16 saturates at 65504)."""


def guard_count(rc):
    """Return value of a tt_*_guard call: >= 0 is the count, negative an error."""
    if rc < 0:
        check(rc)
    return rc


def check(rc):
    if rc != 0:
        msg = load_library().tt_last_error()
        raise EngineError("tortoise_mi355x error %d: %s" % (rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "engine tensors must be contiguous"
    return t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream
