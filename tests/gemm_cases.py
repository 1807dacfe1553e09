"""The cases of the bf16 GEMM sweep (tests/test_gpu_gemm_sweep.py), their inputs and their float64 references: plain torch, no GPU, and
no threshold of the library -- which kernel a case runs on is asked of the library (tests/test_gemm_cases_host.py), never restated here.

Exact-grid data ("grid"): A, B and resid are integers in [-3, 3], aux in [-2, 2] (eighths in [-4, 4] for EPI_DGELU_BF16, whose output is
bounded, not exact); row i of A and column j of B are multiplied by a power
of two from a short cycle (A_CYCLE, B_CYCLE), so that rows and columns differ in exponent as well as in value; bias is a multiple of 1/8;
`shift` multiplies A by 2^shift on top (the GELU cases: pre-activations of order 1).  Every product and every partial sum, in any order
and any K partition, is then a multiple of the grid's least bit lsb(case) of magnitude below 2^24 lsb -- exactly representable in
float32 (test_gemm_cases_host.py checks this from the data) -- so the float64 result IS the answer and no tolerance enters.

Random data ("rand"): N(0, 1) x N(0, 0.05) operands rounded to bf16; ("big"): the same with A times 2^20 and B times 2^-20.
"""
import math

import numpy as np
import torch

NT, NN, TN = 0, 1, 2                                                      # CAREL_GEMM_*
BIAS_BF16, BIAS_GELU, BIAS_DROP_RESID, DGELU_BF16, ADD_F32, SLAB_F32, BIAS_GELU_DG, MUL_BF16 = range(8)      # CAREL_EPI_*
EPI_OF_FORM = {NT: (BIAS_BF16, BIAS_GELU, BIAS_GELU_DG, BIAS_DROP_RESID, ADD_F32), NN: (BIAS_BF16, DGELU_BF16, MUL_BF16, ADD_F32), TN: (SLAB_F32,)}
EPI_NAME = {BIAS_BF16: "bias", BIAS_GELU: "gelu", BIAS_DROP_RESID: "drop", DGELU_BF16: "dgelu", ADD_F32: "add", SLAB_F32: "slab",
            BIAS_GELU_DG: "geludg", MUL_BF16: "mul"}
FORM_NAME = {NT: "NT", NN: "NN", TN: "TN"}
PP, K128, BIG, PP_SLABS, K128_SLABS = 1, 2, 3, 4, 5                        # CAREL_PLAN_* (include/carel_hip_experiments.h)
F32_OUT = (BIAS_DROP_RESID, ADD_F32, SLAB_F32)
A_CYCLE, B_CYCLE = (0, 1, 2), (0, 1)                                       # exponents of the row / column scales
WRAP = (1 << 32) - 1000                                                    # a dropout offset that wraps 2^32 inside the first tile

CASES = []


def case(name, form, epi, M, N, K, splits=1, plan=None, **opt):
    """plan: the (slabs, family, npn) the experiments build reported when the case was written (the host test asserts it).
    opt: ws_bytes; ld = (lda, ldb, ldc) each a delta in elements or "x3"; off = operand offset in elements; drop = (seed, site, off, p);
    row_map; resid_ln; colsum_part; colsum_a; null = names among bias / resid / out_bf16; data = grid | rand | big; shift."""
    known = {"ws_bytes", "ld", "off", "drop", "row_map", "resid_ln", "colsum_part", "colsum_a", "null", "data", "shift"}
    assert set(opt) <= known, set(opt) - known
    c = dict(name=name, form=form, epi=epi, M=M, N=N, K=K, splits=splits, plan=plan, ws_bytes=0, ld=(0, 0, 0), off=0, drop=(0, 0, 0, 0.0),
             row_map=False, resid_ln=False, colsum_part=False, colsum_a=False, null=(), data="grid", shift=0)
    c.update(opt)
    if epi in (BIAS_GELU, BIAS_GELU_DG) and "shift" not in opt and c["data"] == "grid":
        c["shift"] = -4 - int(round(math.log2(K) / 2))                    # pre-activations of order 1: the erf and the table at work
    assert all(o["name"] != name for o in CASES), name
    CASES.append(c)


def planes(n, M, N, delta=0):
    return n * M * N * 4 + delta


D5 = (7, 5, 0, 0.5)
# ---- 128x128 kernel, single pass ----------------------------------------------------------------------------------------------------
case("k128_one_tile_one_step", NT, ADD_F32, 128, 128, 64, plan=(1, K128, 0))
case("k128_nine_tiles", NT, BIAS_BF16, 384, 384, 128, plan=(1, K128, 0))                       # the chunk map with a remainder
case("k128_nine_tiles_nn", NN, ADD_F32, 384, 384, 128, plan=(1, K128, 0))
case("k128_640x256", NT, BIAS_DROP_RESID, 640, 256, 192, plan=(1, K128, 0), drop=D5)
case("k128_below_pp_floor", NT, BIAS_BF16, 1280, 1536, 1024, plan=(1, K128, 0))
case("pp_above_pp_floor", NT, BIAS_BF16, 1536, 1536, 1024, plan=(1, PP, 1))
# ---- big tile -------------------------------------------------------------------------------------------------------------------------
case("big_one_tile_one_step", NT, ADD_F32, 256, 192, 64, plan=(1, BIG, 0))
case("big_six_tiles", NT, BIAS_BF16, 512, 576, 192, plan=(1, BIG, 0))
case("big_six_tiles_nn", NN, ADD_F32, 512, 576, 192, plan=(1, BIG, 0))
case("big_k256", NT, BIAS_DROP_RESID, 256, 192, 256, plan=(1, BIG, 0), drop=D5)
case("big_leaves_for_pp", NT, BIAS_BF16, 4096, 192, 256, plan=(1, PP, 1))
# ---- ping-pong npn 1: ragged M makes the plan take it at any grid -------------------------------------------------------------------
case("pp1_8x1", NT, BIAS_BF16, 2047, 96, 256, plan=(1, PP, 1))
case("pp1_4x2", NT, ADD_F32, 1000, 192, 256, plan=(1, PP, 1), null=("resid",))
case("pp1_4x2_nn", NN, ADD_F32, 1000, 192, 256)
case("pp1_2x4_k320", NT, BIAS_DROP_RESID, 300, 384, 320, plan=(1, PP, 1), drop=D5)
case("pp1_1x8", NT, BIAS_BF16, 37, 768, 256, plan=(1, PP, 1))
case("pp1_3x3_no_rectangle", NT, ADD_F32, 700, 288, 256, plan=(1, PP, 1))
case("pp1_3x3_no_rectangle_nn", NN, BIAS_BF16, 700, 288, 256, plan=(1, PP, 1))
case("pp1_5x1", NT, BIAS_DROP_RESID, 1153, 96, 256, plan=(1, PP, 1), drop=(7, 5, 0, 0.0))
case("pp1_one_row", NT, ADD_F32, 1, 96, 256, plan=(1, PP, 1))
case("pp1_one_row_nn", NN, BIAS_BF16, 1, 96, 256, plan=(1, PP, 1))
case("pp1_k768", NT, BIAS_BF16, 300, 96, 768, plan=(1, PP, 1))
case("pp1_k3072", NN, ADD_F32, 300, 96, 3072, plan=(1, PP, 1))
# ---- ping-pong npn 2 / 3 ------------------------------------------------------------------------------------------------------------
case("pp2_full", NT, BIAS_BF16, 2304, 3072, 256, plan=(1, PP, 2))
case("pp2_ragged", NT, ADD_F32, 2050, 3072, 256, plan=(1, PP, 2))
case("pp2_ragged_nn", NN, BIAS_BF16, 2050, 3072, 256, plan=(1, PP, 2))
case("pp3_full", NT, BIAS_BF16, 8192, 2304, 256, plan=(1, PP, 3))
case("pp3_ragged", NT, ADD_F32, 7937, 2304, 256, plan=(1, PP, 3))
# ---- 128x128 slabs, workspace given -------------------------------------------------------------------------------------------------
case("k128s_4", NT, BIAS_DROP_RESID, 128, 128, 1536, plan=(4, K128_SLABS, 0), ws_bytes=planes(8, 128, 128), drop=D5)
case("k128s_8", NT, ADD_F32, 128, 128, 3072, plan=(8, K128_SLABS, 0), ws_bytes=planes(8, 128, 128))
case("k128s_2_by_k", NT, BIAS_BF16, 128, 128, 1664, plan=(2, K128_SLABS, 0), ws_bytes=planes(8, 128, 128))
case("k128s_none_by_k", NT, BIAS_BF16, 128, 128, 1600, plan=(1, K128, 0), ws_bytes=planes(8, 128, 128))
case("k128s_2_by_workspace", NN, ADD_F32, 128, 128, 1536, plan=(2, K128_SLABS, 0), ws_bytes=planes(2, 128, 128))
case("k128s_none_by_workspace", NN, ADD_F32, 128, 128, 1536, plan=(1, K128, 0), ws_bytes=planes(2, 128, 128, -16))
case("k128s_2_wide", NT, BIAS_BF16, 8192, 256, 1536, plan=(2, K128_SLABS, 0), ws_bytes=planes(2, 8192, 256))
# ---- ping-pong slabs ----------------------------------------------------------------------------------------------------------------
case("pps1_4", NT, BIAS_DROP_RESID, 256, 384, 1536, plan=(4, PP_SLABS, 1), ws_bytes=planes(8, 256, 384), drop=D5)
case("pps1_8", NN, ADD_F32, 256, 384, 3072, plan=(8, PP_SLABS, 1), ws_bytes=planes(8, 256, 384))
case("pps2_4", NT, BIAS_BF16, 640, 2304, 1536, plan=(4, PP_SLABS, 2), ws_bytes=planes(8, 640, 2304))
case("pps2_8", NN, ADD_F32, 640, 1152, 3072, plan=(8, PP_SLABS, 2), ws_bytes=planes(8, 640, 1152))
case("pps1_4_colsum_single_pass", NN, MUL_BF16, 256, 384, 1536, ws_bytes=planes(8, 256, 384), colsum_part=True)
case("pps1_4_ldc_single_pass", NT, ADD_F32, 256, 384, 1536, ws_bytes=planes(8, 256, 384), ld=(0, 0, 8))
case("pps2_4_colsum_single_pass", NN, MUL_BF16, 640, 2304, 1536, ws_bytes=planes(8, 640, 2304), colsum_part=True)
case("pps2_8_ldc_single_pass", NN, ADD_F32, 640, 1152, 3072, ws_bytes=planes(8, 640, 1152), ld=(0, 0, 4))
# ---- TN (weight gradients), each with and without colsum_a --------------------------------------------------------------------------
for cs in (False, True):
    t = "_colsum_a" if cs else ""
    case("tn_k128_s1" + t, TN, SLAB_F32, 128, 128, 256, 1, plan=(1, K128, 0), colsum_a=cs)
    case("tn_k128_s3" + t, TN, SLAB_F32, 384, 128, 576, 3, plan=(1, K128, 0), colsum_a=cs)
    case("tn_big_s2" + t, TN, SLAB_F32, 256, 192, 256, 2, plan=(1, BIG, 0), colsum_a=cs)
    case("tn_pp1_s8" + t, TN, SLAB_F32, 256, 768, 2048, 8, plan=(1, PP, 1), colsum_a=cs)
    case("tn_pp1_s8_uneven" + t, TN, SLAB_F32, 256, 768, 2112, 8, plan=(1, PP, 1), colsum_a=cs)
    case("tn_pp1_s8_tall" + t, TN, SLAB_F32, 1024, 192, 2048, 8, plan=(1, PP, 1), colsum_a=cs)
    case("tn_pp2_s8" + t, TN, SLAB_F32, 2304, 384, 2048, 8, plan=(1, PP, 2), colsum_a=cs)
    # shapes only the ping-pong kernel takes, below its 64-workgroup floor, with the split carel_gemm_wgrad_splits returns (the host
    # test asserts that `splits` is that value): refused before the plan's weight-gradient branch learned to take them.  T = 512 with 2
    # slices is four K tiles per slice, the kernel's stated minimum: its prologue stages K tiles 0 and 1 of the slice, the steady loop
    # runs tiles 0 .. nk - 3 and issues tile t + 2 <= nk - 1, the two tail tiles issue nothing past the slice -- any nk >= 3 is in bounds
    case("tn_pp_only_256x96_t512" + t, TN, SLAB_F32, 256, 96, 512, 2, plan=(1, PP, 1), colsum_a=cs)
    case("tn_pp_only_256x96_t1024" + t, TN, SLAB_F32, 256, 96, 1024, 4, plan=(1, PP, 1), colsum_a=cs)
    case("tn_pp_only_512x288_t1024" + t, TN, SLAB_F32, 512, 288, 1024, 4, plan=(1, PP, 1), colsum_a=cs)
WGRAD_SPLIT_CASES = ("tn_pp_only_256x96_t512", "tn_pp_only_256x96_t1024", "tn_pp_only_512x288_t1024")

# ---- every epilogue of a form on every family; (M, N, K, workspace planes) ---------------------------------------------------------------
FAMILY_SHAPES = (("k128", 384, 384, 128, 0), ("big", 512, 576, 192, 0), ("pp1", 300, 384, 320, 0), ("pp2", 2050, 3072, 256, 0),
                 ("k128s", 128, 128, 1536, 8), ("pps1", 256, 384, 1536, 8))
for fam, M_, N_, K_, ws_ in FAMILY_SHAPES:
    for form_ in (NT, NN):
        for epi_ in EPI_OF_FORM[form_]:
            case("epi_%s_%s_%s" % (fam, FORM_NAME[form_], EPI_NAME[epi_]), form_, epi_, M_, N_, K_, ws_bytes=planes(ws_, M_, N_),
                 drop=(11, 8, 0, 0.5 if epi_ == BIAS_DROP_RESID else 0.0))
case("epi_pp3_NT_gelu", NT, BIAS_GELU, 7937, 2304, 256, plan=(1, PP, 3))
case("epi_pp3_NT_geludg", NT, BIAS_GELU_DG, 7937, 2304, 256, plan=(1, PP, 3))
# (pre-activations up to ~40: finite |u| >= 16 leaves the ping-pong kernel's GELU table by its table-free words)
case("gelu_wide_range_pp1", NT, BIAS_GELU_DG, 300, 384, 320, shift=-5)
case("gelu_wide_range_pp2", NT, BIAS_GELU, 2050, 3072, 256, shift=-5)
case("gelu_wide_range_k128", NT, BIAS_GELU_DG, 384, 384, 128, shift=-4)
case("epi_pp3_NT_drop", NT, BIAS_DROP_RESID, 7937, 2304, 256, plan=(1, PP, 3), drop=(11, 8, 0, 0.5))

# ---- options, on at least one case per family that accepts them ------------------------------------------------------------------------
for fam, M_, N_, K_, ws_ in FAMILY_SHAPES[:3]:
    case("opt_%s_ldc8_bf16" % fam, NT, BIAS_BF16, M_, N_, K_, ld=(0, 0, 8))
    case("opt_%s_ldc4_f32" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, ld=(0, 0, 4), drop=(3, 2, 1, 0.5))
    case("opt_%s_ldc8_f32_nn" % fam, NN, ADD_F32, M_, N_, K_, ld=(0, 0, 8))
    case("opt_%s_ld8" % fam, NT, ADD_F32, M_, N_, K_, ld=(8, 8, 0))
    case("opt_%s_ld8_nn" % fam, NN, ADD_F32, M_, N_, K_, ld=(8, 8, 0))
    case("opt_%s_ldx3" % fam, NT, BIAS_BF16, M_, N_, K_, ld=("x3", "x3", 0))
    case("opt_%s_ldx3_nn" % fam, NN, BIAS_BF16, M_, N_, K_, ld=("x3", "x3", 0))
    case("opt_%s_offset" % fam, NT, ADD_F32, M_, N_, K_, off=8)
    case("opt_%s_offset_nn" % fam, NN, ADD_F32, M_, N_, K_, off=8)
    case("opt_%s_row_map" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, drop=(5, 11, 0, 0.5), row_map=True)
    case("opt_%s_drop_odd" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, drop=(5, 11, 12345, 0.5))
    case("opt_%s_drop_wraps" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, drop=(5, 11, WRAP, 0.5))
    case("opt_%s_null_bias" % fam, NT, BIAS_BF16, M_, N_, K_, null=("bias",))
    case("opt_%s_null_bias_drop" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, null=("bias",), drop=(5, 11, 0, 0.5))
    case("opt_%s_add_no_resid" % fam, NT, ADD_F32, M_, N_, K_, null=("resid",))
    case("opt_%s_gelu_no_u" % fam, NT, BIAS_GELU, M_, N_, K_, null=("out_bf16",))
fam, M_, N_, K_, ws_ = FAMILY_SHAPES[3]          # (the 2050 x 3072 outputs: one case per option)
case("opt_pp2_ldc8_bf16", NT, BIAS_BF16, M_, N_, K_, ld=(0, 0, 8))
case("opt_pp2_ldc4_f32", NT, BIAS_DROP_RESID, M_, N_, K_, ld=(0, 0, 4), drop=(3, 2, 1, 0.5))
case("opt_pp2_ld8_offset", NT, ADD_F32, M_, N_, K_, ld=(8, 8, 0), off=8)
case("opt_pp2_ldx3_nn", NN, BIAS_BF16, M_, N_, K_, ld=("x3", "x3", 0))
case("opt_pp2_row_map_wraps", NT, BIAS_DROP_RESID, M_, N_, K_, drop=(5, 11, WRAP, 0.5), row_map=True, null=("bias",))
case("opt_pp2_gelu_no_u", NT, BIAS_GELU, M_, N_, K_, null=("out_bf16",))
for fam, M_, N_, K_, ws_ in FAMILY_SHAPES[4:]:
    case("opt_%s_row_map" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, ws_bytes=planes(ws_, M_, N_), drop=(5, 11, 0, 0.5), row_map=True)
    case("opt_%s_drop_wraps" % fam, NT, BIAS_DROP_RESID, M_, N_, K_, ws_bytes=planes(ws_, M_, N_), drop=(5, 11, WRAP, 0.5))
    case("opt_%s_ld8_offset" % fam, NN, ADD_F32, M_, N_, K_, ws_bytes=planes(ws_, M_, N_), ld=(8, 8, 0), off=8)
    case("opt_%s_null_bias" % fam, NT, BIAS_BF16, M_, N_, K_, ws_bytes=planes(ws_, M_, N_), null=("bias",))
    case("opt_%s_gelu_no_u" % fam, NT, BIAS_GELU, M_, N_, K_, ws_bytes=planes(ws_, M_, N_), null=("out_bf16",))
case("opt_tn_k128_ld8_offset", TN, SLAB_F32, 384, 128, 576, 3, ld=(8, 8, 8), off=8, colsum_a=True)
case("opt_tn_big_ld8_offset", TN, SLAB_F32, 256, 192, 256, 2, ld=(8, "x3", 4), off=8, colsum_a=True)
case("opt_tn_pp_ld8_offset", TN, SLAB_F32, 256, 768, 2112, 8, ld=("x3", 8, 4), off=8, colsum_a=True)
# colsum_part on DGELU and MUL: ragged M on N = 192 (ping-pong npn 2: the fused sums need fragment pairs), the 128x128 kernel, the big tile
for epi_ in (DGELU_BF16, MUL_BF16):
    case("colsum_pp2_ragged_" + EPI_NAME[epi_], NN, epi_, 300, 192, 256, plan=(1, PP, 2), colsum_part=True)
    case("colsum_pp2_ragged_two_tiles_" + EPI_NAME[epi_], NN, epi_, 129, 192, 256, plan=(1, PP, 2), colsum_part=True)
    case("colsum_k128_" + EPI_NAME[epi_], NN, epi_, 384, 384, 128, plan=(1, K128, 0), colsum_part=True)
    case("colsum_big_" + EPI_NAME[epi_], NN, epi_, 512, 576, 192, plan=(1, BIG, 0), colsum_part=True)
    case("colsum_pp2_ldc8_" + EPI_NAME[epi_], NN, epi_, 300, 192, 256, colsum_part=True, ld=(0, 0, 8))

# ---- random data: a few per family, and magnitudes near 2^+-20 --------------------------------------------------------------------------
case("rand_k128", NT, BIAS_BF16, 384, 384, 128, data="rand")
case("rand_k128_f32", NN, ADD_F32, 384, 384, 128, data="rand")
case("rand_big", NT, BIAS_DROP_RESID, 512, 576, 192, data="rand", drop=(9, 4, 0, 0.1))
case("rand_pp1", NN, ADD_F32, 300, 384, 320, data="rand")
case("rand_pp2", NT, BIAS_BF16, 2050, 3072, 256, data="rand")
case("rand_pp3", NT, ADD_F32, 7937, 2304, 256, data="rand")
case("rand_k128s", NT, BIAS_DROP_RESID, 128, 128, 3072, data="rand", ws_bytes=planes(8, 128, 128), drop=(9, 4, 0, 0.1))
case("rand_pps2", NN, ADD_F32, 640, 1152, 3072, data="rand", ws_bytes=planes(8, 640, 1152))
case("rand_tn_pp", TN, SLAB_F32, 256, 768, 2112, 8, data="rand", colsum_a=True)
case("rand_tn_k128", TN, SLAB_F32, 384, 128, 576, 3, data="rand", colsum_a=True)
case("rand_big_magnitudes_pp", NT, ADD_F32, 300, 384, 320, data="big")
case("rand_big_magnitudes_k128", NN, BIAS_BF16, 384, 384, 128, data="big")
case("rand_gelu_pp1", NT, BIAS_GELU, 300, 384, 320, data="rand")
case("rand_dgelu_pp2", NN, DGELU_BF16, 300, 192, 256, data="rand", colsum_part=True)
# ---- the recomputed LayerNorm residual (rows of 768, the width of carel_layernorm_fwd): the 96-wide ping-pong tile, the 128x128 kernel,
# and the slab epilogue behind both (the big tile never gets an N = 768 GEMM: a (256, 192)-multiple with N = 768 is a (128, 128)-multiple)
case("resid_ln_pp1", NT, BIAS_DROP_RESID, 300, 768, 320, plan=(1, PP, 1), resid_ln=True, drop=(5, 11, 0, 0.5))
case("resid_ln_k128", NT, BIAS_DROP_RESID, 384, 768, 128, plan=(1, K128, 0), resid_ln=True, drop=(5, 11, 0, 0.5))
case("resid_ln_k128s", NT, BIAS_DROP_RESID, 128, 768, 1536, plan=(4, K128_SLABS, 0), resid_ln=True, ws_bytes=planes(8, 128, 768))
case("resid_ln_pps1", NT, BIAS_DROP_RESID, 256, 768, 1536, plan=(4, PP_SLABS, 1), resid_ln=True, ws_bytes=planes(8, 256, 768), drop=(5, 11, 0, 0.5))

BY_NAME = {c["name"]: c for c in CASES}
EXACT = [c for c in CASES if c["data"] == "grid"]


# ------------------------------------------------------------------------------------------------ geometry
def a_shape(c):
    return (c["K"], c["M"]) if c["form"] == TN else (c["M"], c["K"])


def b_shape(c):
    return (c["N"], c["K"]) if c["form"] == NT else (c["K"], c["N"])


def lds(c):
    """(lda, ldb, ldc) in elements."""
    dense = (a_shape(c)[1], b_shape(c)[1], c["N"])
    return tuple(3 * d if x == "x3" else d + x for d, x in zip(dense, c["ld"]))


def lsb(c):
    """The least bit of the case's exact grid."""
    return 2.0 ** min(-3, c["shift"])


def k_slices(c):
    """[(k0, k1)] of the case's `splits` K slices: slice z is K tiles [z nk / s, (z + 1) nk / s) of 64 (equal slices where s divides nk)."""
    nk, s = c["K"] // 64, c["splits"]
    return [(64 * (z * nk // s), 64 * ((z + 1) * nk // s)) for z in range(s)]


# ------------------------------------------------------------------------------------------------ inputs
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _strided(t, ld, off, pad=float("nan")):
    """-> (flat buffer holding t at element offset `off` with row pitch ld -- exactly t's rows long --, the view of t inside it)."""
    rows, cols = t.shape
    buf = torch.full((off + (rows - 1) * ld + cols,), pad, dtype=t.dtype)
    view = buf[off:].as_strided((rows, cols), (ld, 1))
    view.copy_(t)
    return buf, view


def make_inputs(c, seed=None):
    """CPU tensors of the case: A / B (bf16 values [rows, cols]) with their flat buffers A_buf / B_buf (NaN between and around the rows),
    bias [N] f32, resid / aux [M, N] (f32 / bf16), row_map int32 [M] or None, and for resid_ln the pre-LayerNorm rows h [M, N] with
    gamma / beta [N]."""
    g = torch.Generator().manual_seed(seed if seed is not None else 1000 + CASES.index(c))
    M, N, K = c["M"], c["N"], c["K"]
    ash, bsh = a_shape(c), b_shape(c)
    if c["data"] == "grid":
        A, B = _ints(g, ash, -3, 3), _ints(g, bsh, -3, 3)
        sa = 2.0 ** (torch.tensor(A_CYCLE, dtype=torch.float32)[torch.arange(M) % len(A_CYCLE)] + c["shift"])
        sb = 2.0 ** torch.tensor(B_CYCLE, dtype=torch.float32)[torch.arange(N) % len(B_CYCLE)]
        A = A * (sa[None, :] if c["form"] == TN else sa[:, None])
        B = B * (sb[:, None] if c["form"] == NT else sb[None, :])
        bias = _ints(g, (N,), -24, 24) / 8
        resid = _ints(g, (M, N), -3, 3)
        aux = _ints(g, (M, N), -32, 32) / 8 if c["epi"] == DGELU_BF16 else _ints(g, (M, N), -2, 2)
    else:
        A, B = torch.randn(ash, generator=g), torch.randn(bsh, generator=g) * 0.05
        if c["data"] == "big":
            A, B = A * 2.0 ** 20, B * 2.0 ** -20
        bias, resid = torch.randn((N,), generator=g) * 0.1, torch.randn((M, N), generator=g)
        aux = torch.randn((M, N), generator=g) * 1.5
    lda, ldb, ldc = lds(c)
    d = {"bias": None if "bias" in c["null"] else bias, "resid": None if "resid" in c["null"] else resid,
         "aux": aux.bfloat16(), "row_map": None}
    d["A_buf"], d["A"] = _strided(A.bfloat16(), lda, c["off"])
    d["B_buf"], d["B"] = _strided(B.bfloat16(), ldb, c["off"])
    if c["row_map"]:
        d["row_map"] = torch.randperm(M, generator=g).to(torch.int32)
    if c["resid_ln"]:
        d["h"] = torch.randn((M, N), generator=g) * 2 + 0.3
        d["gamma"], d["beta"] = 1 + 0.1 * torch.randn((ldc,), generator=g), 0.1 * torch.randn((ldc,), generator=g)
    return d


# ------------------------------------------------------------------------------------------------ float64 references
def gelu64(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2)))


def dgelu64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def keep_mult(c, row_map, device="cpu"):
    """[M, N] float64 dropout multipliers (0 or 1 / (1 - p)) of element map[row] * ldc + col + off (uint32, wrapping); None at p = 0."""
    from oracle import carel_oracle as O
    seed, site, off, p = c["drop"]
    if p <= 0:
        return None
    rows = np.arange(c["M"], dtype=np.uint64) if row_map is None else row_map.cpu().numpy().astype(np.uint64)
    idx = (rows[:, None] * np.uint64(lds(c)[2]) + np.arange(c["N"], dtype=np.uint64)[None, :] + np.uint64(off)).astype(np.uint32)
    return torch.from_numpy(O.dropout_keep(seed, site, idx, p).astype(np.float64) / (1 - p)).to(device)


def product64(c, A, B, k0=0, k1=None):
    """float64 product of the K range [k0, k1) on the operands' own bf16 values."""
    k1 = c["K"] if k1 is None else k1
    A, B = A.double(), B.double()
    if c["form"] == TN:
        return A[k0:k1].t() @ B[k0:k1]
    return A[:, k0:k1] @ (B[:, k0:k1].t() if c["form"] == NT else B[k0:k1])


def absprod64(c, A, B):
    """sum over k of |a||b| per output: the scale of the order-free dot-product bound, and of the exactness claim."""
    return product64(c, A.double().abs(), B.double().abs())


def tile_sums(x, M):
    """[ceil(M / 128), N]: column sums over each 128-row tile."""
    nt = (M + 127) // 128
    pad = torch.zeros((nt * 128, x.shape[1]), dtype=x.dtype, device=x.device)
    pad[:M] = x
    return pad.view(nt, 128, -1).sum(1)


def reference(c, d, resid_rows=None):
    """float64 references of every output of the case from the inputs d (make_inputs; on any device):
    acc (the product), pre (acc + bias where the epilogue has one), and per epilogue out_f32 / out_bf16 / out2_bf16 (before the bf16 rounding),
    u (the bf16-rounded pre-activation, float64), colsum_part, slabs [s, M, N], colsum_a [s, M].  resid_rows: the residual to add where the
    case recomputes it (resid_ln)."""
    epi, M = c["epi"], c["M"]
    r = {}
    if epi == SLAB_F32:
        sl = k_slices(c)
        r["slabs"] = torch.stack([product64(c, d["A"], d["B"], k0, k1) for k0, k1 in sl])
        if c["colsum_a"]:
            r["colsum_a"] = torch.stack([d["A"][k0:k1].double().sum(0) for k0, k1 in sl])
        return r
    acc = product64(c, d["A"], d["B"])
    r["acc"] = acc
    pre = acc if (d["bias"] is None or epi in (DGELU_BF16, MUL_BF16, ADD_F32)) else acc + d["bias"].double()
    r["pre"] = pre
    if epi == BIAS_BF16:
        r["out_bf16"] = pre
    elif epi in (BIAS_GELU, BIAS_GELU_DG):
        u = pre.float().bfloat16().double()                 # (exact-grid data: pre is a float32 value, so this is the kernel's own rounding)
        r["u"] = u
        r["out2_bf16"] = gelu64(u)
        r["out_bf16"] = pre if epi == BIAS_GELU else dgelu64(u)
    elif epi == BIAS_DROP_RESID:
        km = keep_mult(c, d["row_map"], pre.device)
        y = pre if km is None else pre * km
        res = resid_rows if resid_rows is not None else d["resid"]
        r["dropped"] = y
        r["out_f32"] = y + res.double()
    elif epi == ADD_F32:
        r["out_f32"] = acc if d["resid"] is None else acc + d["resid"].double()
    elif epi in (DGELU_BF16, MUL_BF16):
        aux = d["aux"].double()
        r["factor"] = dgelu64(aux) if epi == DGELU_BF16 else aux
        r["out_bf16"] = acc * r["factor"]
        if c["colsum_part"]:
            r["colsum_part"] = tile_sums(r["out_bf16"], M)
    return r


# ------------------------------------------------------------------------------------------------ derived bounds
U24 = 2.0 ** -24
# Random data: per element |got - ref| <= K 2^-24 sum_k |a||b| (dot_bound), the order-free bound of an fp32 dot product of length K
# (Higham, Accuracy and Stability of Numerical Algorithms, (3.5): gamma_K = K u / (1 - K u) with u = 2^-24, the products of two bf16
# values being exact in fp32): it holds for every order of the additions and every K partition, so for every kernel and slab count.
BF16_RND = 2.0 ** -8                                                # one bf16 rounding of the reference, relative (the issue's constant)
# erf: Abramowitz & Stegun 7.1.26 (the five-term rational approximation), |error| <= 1.5e-7 in exact arithmetic (A&S p. 299;
# test_gemm_cases_host.py evaluates the formula in float64 and confirms it).  The fp32 chain of carel_common.h erf_as around it:
# t = rcp(fma) 2 roundings, four fma of the Horner chain + 2 products 6 roundings of values <= 1.5 (poly t ez <= 1), the fast
# exponential exp(-z^2): the argument's rounding (relative 2^-24 of z^2, i.e. z^2 2^-24 relative in ez) and ~2 ulp of its own
# -- ez (z^2 + 2) 2^-23 <= 1.3 x 2^-23 since z^2 exp(-z^2) <= 1 / e --, the final 1 - x one rounding of a value <= 1: at most
# (2 + 6) 1.5 + 2.6 + 0.5 < 16 units of 2^-24.  Two more for x / sqrt 2 entering erf (|d erf| <= 1.13 |dz|, relative 2^-24 of z with
# z exp(-z^2) <= 0.43).
E_ERF = 1.5e-7 + 18 * U24


def gelu_bound(u, ref, rnd=BF16_RND):
    """|bf16 gelu output - ref|: gelu = 0.5 u (1 + erf): 0.5 |u| E_ERF, three roundings of the result (1 + erf, the two products), and the
    bf16 rounding of the result (2^-9 relative of the computed value, within BF16_RND of the reference with room for the terms before)."""
    return rnd * ref.abs() + 1.01 * (0.5 * u.abs() * E_ERF + 3 * U24 * ref.abs())


def dgelu_bound(u, ref, rnd=BF16_RND):
    """|bf16 gelu' output - ref|: gelu' = 0.5 (1 + erf) + u phi(u): 0.5 E_ERF, the error of ez = exp(-u^2 / 2) carried by u phi(u)
    (relative (u^2 / 2 + 2) 2^-23, and |u| phi(u) (u^2 / 2 + 2) <= 0.8), four roundings of values <= 1.13."""
    return rnd * ref.abs() + 1.01 * (0.5 * E_ERF + (1.6 + 4 * 1.13) * U24)


E_DGELU = 0.5 * E_ERF + (1.6 + 4 * 1.13) * U24                      # the absolute error of the fp32 gelu' before its bf16 rounding


def dot_bound(c, d):
    """K 2^-24 sum_k |a||b| per output (of the whole contraction: a slab's own bound is that of its K range)."""
    return c["K"] * U24 * absprod64(c, d["A"], d["B"])


def exact_outputs(c):
    """The outputs of the case that must equal the float64 reference bit for bit (after its rounding to the output's type)."""
    if c["data"] != "grid":
        return ()
    return {SLAB_F32: ("slabs", "colsum_a"), ADD_F32: ("out_f32",), BIAS_BF16: ("out_bf16",), BIAS_GELU: ("out_bf16",), BIAS_GELU_DG: (),
            DGELU_BF16: (), MUL_BF16: ("out_bf16", "colsum_part"), BIAS_DROP_RESID: () if c["resid_ln"] else ("out_f32",)}[c["epi"]]


def bounds(c, d, r, u=None, rounding=True):
    """{output: per-element bound on |got - reference|} of the case's outputs that are not exact (exact_outputs), from the float64
    references r = reference(c, d).  u: the pre-activation the GELU outputs of `r` were taken at, when it is not r's own (random data:
    the kernel's own bf16 pre-activation).  Random data: dot_bound; one 2^-24 relative rounding per further fp32 operation; one bf16
    rounding for a bf16 output; GELU outputs: gelu_bound / dgelu_bound.  rounding=False: the bounds of the fp32 values BEFORE the bf16 rounding
    of the output, i.e. the derived part alone (one bf16 rounding is 2^-8 relative at worst whatever is rounded: the host test's float32
    yardstick is judged before it)."""
    epi, grid = c["epi"], c["data"] == "grid"
    rnd = BF16_RND if rounding else 0.0
    b = {}
    if epi == SLAB_F32:
        if not grid:
            sl = k_slices(c)
            A, B = d["A"].double().abs(), d["B"].double().abs()
            b["slabs"] = torch.stack([(k1 - k0) * U24 * (A[k0:k1].t() @ B[k0:k1]) for k0, k1 in sl])
            if c["colsum_a"]:
                b["colsum_a"] = torch.stack([(k1 - k0) * U24 * A[k0:k1].sum(0) for k0, k1 in sl])
        return b
    dot = 0.0 if grid else dot_bound(c, d)
    if epi == BIAS_BF16 and not grid:
        b["out_bf16"] = dot + U24 * r["pre"].abs() + rnd * r["out_bf16"].abs()
    elif epi == ADD_F32 and not grid:
        b["out_f32"] = dot + U24 * r["out_f32"].abs()
    elif epi == BIAS_DROP_RESID and not grid:
        m = 1.0 / (1.0 - c["drop"][3])
        b["out_f32"] = m * (dot + U24 * r["pre"].abs()) + 2 * U24 * (r["dropped"].abs() + r["out_f32"].abs())
    elif epi in (BIAS_GELU, BIAS_GELU_DG):
        uu = r["u"] if u is None else u
        if epi == BIAS_GELU:
            if not grid:
                b["out_bf16"] = dot + U24 * r["pre"].abs() + rnd * r["pre"].abs()
        else:
            b["out_bf16"] = dgelu_bound(uu, dgelu64(uu), rnd)
        b["out2_bf16"] = gelu_bound(uu, gelu64(uu), rnd)
    elif epi == DGELU_BF16:
        f = r["factor"].abs()
        pre_round = 1.01 * (r["acc"].abs() * E_DGELU + dot * f + 2 * U24 * r["out_bf16"].abs())
        b["out_bf16"] = rnd * r["out_bf16"].abs() + pre_round
        if c["colsum_part"]:
            b["colsum_part"] = tile_sums(pre_round, c["M"]) + 128 * U24 * tile_sums(r["out_bf16"].abs(), c["M"])
    return b


def resid_ln_rows64(d, stats):
    """The residual rows of a resid_ln case in float64: LayerNorm of the given rows h from the GIVEN statistics [M, 2] = (mean, rstd)."""
    st = stats.double()
    return (d["h"].double() - st[:, :1]) * st[:, 1:] * d["gamma"].double() + d["beta"].double()


LN_ROW_REL = 1e-6          # ||got - ref|| / ||ref|| per row of the LayerNorm forward's x_f32 (tests/test_gpu_rowops_sweep.py)


def resid_ln_row_bound(res, out):
    """Per row, on ||got - ref||: the LayerNorm forward bound on the residual term, and the one rounding of the epilogue's last addition
    (the dropped term is exact on the grid)."""
    return LN_ROW_REL * res.norm(dim=1) + 2 * U24 * out.norm(dim=1)


def worst_fractions(c, d, got, r, u=None, rounding=True):
    """{output: max |got - ref| / bound} over the case's bounded outputs (a zero difference counts as 0 whatever the bound).  u: the
    pre-activation the GELU outputs in `got` were computed from, when it is not the reference's own (random data)."""
    out = {}
    if u is not None:
        r = dict(r, out2_bf16=gelu64(u))
        if c["epi"] == BIAS_GELU_DG:
            r["out_bf16"] = dgelu64(u)
    for k, b in bounds(c, d, r, u, rounding).items():
        if got.get(k) is None:
            continue
        diff = (got[k].double() - r[k]).abs()
        out[k] = float(torch.where(diff == 0, torch.zeros_like(diff), diff / b).max())
    return out
