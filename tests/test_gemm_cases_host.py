"""The GEMM sweep's cases (tests/gemm_cases.py) judged without a GPU: the exact-grid claim from the data alone, the coverage of every
kernel family / tile width / slab count / epilogue the plan can choose -- asked of the experiments library through carel_gemm_split_plan,
as tests/test_packed_dispatch.py does, not restated in Python --, stock torch float32 against the derived bounds, the intrinsic error of
the erf formula, and carel_gemm_wgrad_splits against the plan over a grid of weight-gradient shapes."""
import ctypes as C
import math

import pytest
import torch

from carel_vae_amd import _lib as L
from tests import gemm_cases as G

_BIG = 1 << 40              # a fake, aligned address: the plan checks the operands' alignment but never reads them


@pytest.fixture(scope="module")
def exp_lib():
    from carel_vae_amd import build
    build.build(verbose=False)
    return L.load_experiments()


def plan_args(c):
    a = L.GemmArgs()
    a.A = a.B = _BIG + 2 * c["off"]
    a.lda, a.ldb, a.ldc = G.lds(c)
    a.M, a.N, a.K, a.form, a.epilogue, a.splits = c["M"], c["N"], c["K"], c["form"], c["epi"], c["splits"]
    a.out_bf16 = a.out2_bf16 = a.out_f32 = a.bias = a.resid_f32 = a.aux_bf16 = _BIG
    for name in c["null"]:
        setattr(a, {"bias": "bias", "resid": "resid_f32", "out_bf16": "out_bf16"}[name], None)
    if c["ws_bytes"]:
        a.splitk_ws, a.splitk_ws_bytes = _BIG, c["ws_bytes"]
    if c["colsum_part"]:
        a.colsum_part = _BIG
    if c["colsum_a"]:
        a.colsum_a = _BIG
    if c["row_map"]:
        a.drop_row_map = _BIG
    if c["resid_ln"]:
        a.resid_ln_stats = a.resid_ln_gamma = a.resid_ln_beta = _BIG
    a.drop_seed, a.drop_site, a.drop_idx_offset, a.drop_p = c["drop"]
    return a


def plan_of(lib, c):
    out = (C.c_int32 * 3)()
    L.check(lib.carel_gemm_split_plan(C.byref(plan_args(c)), 1, out), "carel_gemm_split_plan(%s)" % c["name"])
    return tuple(out)


# ------------------------------------------------------------------------------------------------ coverage
# (form, family, npn, slabs) the product library can choose -- the issue's list; NN has no npn 3 (gemm_pp_launch)
WANTED_PLANS = ([(f, G.K128, 0, 1) for f in (G.NT, G.NN, G.TN)] + [(f, G.BIG, 0, 1) for f in (G.NT, G.NN, G.TN)] +
                [(G.NT, G.PP, n, 1) for n in (1, 2, 3)] + [(G.NN, G.PP, n, 1) for n in (1, 2)] + [(G.TN, G.PP, n, 1) for n in (1, 2)] +
                [(G.NT, G.K128_SLABS, 0, s) for s in (2, 4, 8)] + [(G.NN, G.K128_SLABS, 0, s) for s in (2, 4)] +
                [(f, G.PP_SLABS, n, s) for f, n, s in ((G.NT, 1, 4), (G.NN, 1, 8), (G.NT, 2, 4), (G.NN, 2, 8))])


def test_every_case_is_planned_as_its_row_says(exp_lib):
    wrong = {c["name"]: (plan_of(exp_lib, c), c["plan"]) for c in G.CASES if c["plan"] is not None and plan_of(exp_lib, c) != c["plan"]}
    assert not wrong, "cases whose plan (slabs, family, npn) has moved (now, table): %r" % wrong


def test_the_table_covers_every_family_width_slab_count_and_epilogue(exp_lib):
    plans = {c["name"]: plan_of(exp_lib, c) for c in G.CASES}
    have = {(c["form"], plans[c["name"]][1], plans[c["name"]][2], plans[c["name"]][0]) for c in G.CASES}
    missing = [w for w in WANTED_PLANS if w not in have]
    assert not missing, "(form, family, npn, slabs) without a case in tests/gemm_cases.py: %r" % missing
    # every epilogue launch_instance offers for the form, on every family (and ping-pong width) the plan gives it; exact-grid cases only
    have_epi = {(c["form"], c["epi"], plans[c["name"]][1], plans[c["name"]][2]) for c in G.EXACT}
    fams = {(p[1], p[2]) for p in plans.values()}
    want = []
    for form in (G.NT, G.NN):
        for epi in G.EPI_OF_FORM[form]:
            for fam, npn in sorted(fams):
                if form == G.NN and npn == 3:
                    continue
                if fam == G.PP_SLABS and npn == 2:
                    continue                                      # (the slab epilogue kernel is one for both widths: npn 1 carries the epilogues)
                want.append((form, epi, fam, npn))
    missing = [w for w in want if w not in have_epi]
    assert not missing, "(form, epilogue, family, npn) without an exact-grid case: %r" % missing
    # the options: what forces the single pass does
    for name in ("pps1_4_colsum_single_pass", "pps1_4_ldc_single_pass", "pps2_4_colsum_single_pass", "pps2_8_ldc_single_pass"):
        assert plans[name][0] == 1, (name, plans[name])
    # colsum_part on all three single-pass kernels, ragged M on the ping-pong one
    for epi in (G.DGELU_BF16, G.MUL_BF16):
        got = {plans[c["name"]][1] for c in G.CASES if c["epi"] == epi and c["colsum_part"]}
        assert {G.PP, G.K128, G.BIG} <= got, (epi, got)
        assert any(c["epi"] == epi and c["colsum_part"] and c["M"] % 128 and plans[c["name"]][1] == G.PP for c in G.CASES)
    # colsum_a, row_map, resid_ln, offsets and pitches each reach every family that accepts them
    for key, fams_wanted in (("colsum_a", {G.PP, G.K128, G.BIG}), ("row_map", {G.PP, G.K128, G.BIG, G.PP_SLABS, G.K128_SLABS}),
                             ("resid_ln", {G.PP, G.K128, G.PP_SLABS, G.K128_SLABS}), ("off", {G.PP, G.K128, G.BIG, G.PP_SLABS, G.K128_SLABS})):
        got = {plans[c["name"]][1] for c in G.CASES if c[key]}
        assert fams_wanted <= got, (key, got)
    for i in range(3):
        got = {plans[c["name"]][1] for c in G.CASES if c["ld"][i] != 0}
        assert {G.PP, G.K128, G.BIG} <= got, (i, got)


def test_weight_gradient_split_cases_use_the_split_the_library_proposes(exp_lib):
    for name in G.WGRAD_SPLIT_CASES:
        c = G.BY_NAME[name]
        assert exp_lib.carel_gemm_wgrad_splits(c["M"], c["N"], c["K"]) == c["splits"], name


def test_wgrad_splits_proposes_only_what_the_gemm_accepts(exp_lib):
    """For every weight-gradient shape the header admits -- (M, N) multiples of (128, 128), (256, 192) or (256, 96), T a multiple of 64
    from 256 -- carel_gemm_wgrad_splits returns a split that carel_gemm_bf16 plans.  Before the fix 131 of the 240 (256, 96)-multiple
    shapes below were refused: the weight-gradient branch of gemm_plan took the ping-pong kernel only from 64 workgroups on."""
    refused = []
    shapes = [(m, n) for m in (256, 512, 768, 1024, 2304, 3072) for n in (96, 288, 480, 672, 864)]
    shapes += [(128, 128), (384, 128), (128, 768), (768, 768), (256, 192), (512, 576), (2304, 768), (768, 3072), (3072, 768)]
    for M, N in shapes:
        for T in (256, 320, 512, 576, 1024, 1088, 2048, 2112, 4096, 8192):
            s = exp_lib.carel_gemm_wgrad_splits(M, N, T)
            c = dict(G.BY_NAME["tn_k128_s1"], M=M, N=N, K=T, splits=s)
            out = (C.c_int32 * 3)()
            if s < 1 or exp_lib.carel_gemm_split_plan(C.byref(plan_args(c)), 1, out) != 0 or out[1] not in (G.PP, G.K128, G.BIG):
                refused.append((M, N, T, s))
    assert not refused, "carel_gemm_wgrad_splits proposes what carel_gemm_bf16 refuses (M, N, T, splits): %r" % refused


def test_bf16_outputs_refuse_a_row_pitch_of_8k_plus_4(exp_lib):
    out = (C.c_int32 * 3)()
    for name in ("k128_nine_tiles", "epi_pp1_NT_gelu", "epi_big_NT_geludg", "epi_k128_NN_dgelu", "epi_pp1_NN_mul"):
        c = dict(G.BY_NAME[name], ld=(0, 0, 4))
        assert exp_lib.carel_gemm_split_plan(C.byref(plan_args(c)), 1, out) == -1, name          # CAREL_ERR_ARG
        assert b"ldc a multiple of 8" in exp_lib.carel_last_error(), name
    for name in ("k128_nine_tiles_nn", "k128_640x256", "tn_k128_s3"):              # f32 outputs: a multiple of 4 will do
        c = dict(G.BY_NAME[name], ld=(0, 0, 4))
        assert exp_lib.carel_gemm_split_plan(C.byref(plan_args(c)), 1, out) == 0, name


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("c", G.EXACT, ids=lambda c: c["name"])
def test_exact_grid_cases_are_exact_in_float32(c):
    """Every partial sum of an exact-grid case, in any order and any K partition, is a multiple of the grid's least bit below 2^24 of it:
    max over outputs of sum_k |a||b| (+ |bias|, times the dropout multiplier, + |resid|), the same times |aux| for EPI_MUL_BF16, and the sum
    of the 128 terms of every colsum_part entry.  A case that breaks this is the case to change."""
    d = G.make_inputs(c)
    lsb, lim = G.lsb(c), 2.0 ** 24
    for t in (d["A"], d["B"]):
        v = t.double() / lsb
        assert bool((v == v.round()).all())
    s = G.absprod64(c, d["A"], d["B"])
    if c["epi"] == G.SLAB_F32:
        assert float(s.max()) / lsb < lim
        assert float(d["A"].double().abs().sum(0).max()) / lsb < lim
        return
    if d["bias"] is not None and c["epi"] in (G.BIAS_BF16, G.BIAS_GELU, G.BIAS_GELU_DG, G.BIAS_DROP_RESID):
        assert bool(((d["bias"].double() / lsb) == (d["bias"].double() / lsb).round()).all())
        s = s + d["bias"].double().abs()
    if c["epi"] == G.BIAS_DROP_RESID:
        p = c["drop"][3]
        assert p in (0.0, 0.5)
        s = s / (1 - p)
        if not c["resid_ln"]:
            s = s + d["resid"].double().abs()
    if c["epi"] == G.ADD_F32 and d["resid"] is not None:
        s = s + d["resid"].double().abs()
    if c["epi"] == G.MUL_BF16:
        s = s * d["aux"].double().abs()
        if c["colsum_part"]:
            r = G.reference(c, d)
            assert float(G.tile_sums(r["out_bf16"].abs(), c["M"]).max()) / lsb < lim
    assert float(s.max()) / lsb < lim, float(s.max()) / lsb


def test_gelu_cases_exercise_the_table_and_both_ways_out_of_it():
    """The exact-grid GELU cases hold pre-activations inside the lookup table's range (2^-16 <= |u| < 16), zeros (below it: the arithmetic
    path) and |u| >= 16 (the table-free words)."""
    u = torch.cat([G.reference(c, G.make_inputs(c))["u"].flatten() for c in G.EXACT if c["epi"] in (G.BIAS_GELU, G.BIAS_GELU_DG) and c["M"] <= 512])
    a = u.abs()
    assert bool((a == 0).any()) and bool((a >= 16).any()) and float(((a >= 2.0 ** -16) & (a < 16)).double().mean()) > 0.9
    assert bool(((a > 0.25) & (a < 4)).double().mean() > 0.3)


# ------------------------------------------------------------------------------------------------ yardsticks
def test_the_erf_formula_is_within_its_published_bound():
    """Abramowitz & Stegun 7.1.26, the formula of carel_common.h erf_as, in float64 against erf: |error| <= 1.5e-7 (what E_ERF starts from)."""
    z = torch.linspace(0, 6, 600001, dtype=torch.float64)
    t = 1 / (1 + 0.3275911 * z)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    err = float((1 - poly * torch.exp(-z * z) - torch.erf(z)).abs().max())
    assert 0.5e-7 < err <= 1.5e-7, err


def _torch_f32(c, d):
    """The case by stock torch float32 on the CPU; bf16 outputs before their rounding (the pre-activation u of the GELU epilogues rounded)."""
    A, B = d["A"].float(), d["B"].float()
    o = {}
    if c["epi"] == G.SLAB_F32:
        o["slabs"] = torch.stack([A[k0:k1].t() @ B[k0:k1] for k0, k1 in G.k_slices(c)])
        if c["colsum_a"]:
            o["colsum_a"] = torch.stack([A[k0:k1].sum(0) for k0, k1 in G.k_slices(c)])
        return o
    acc = A @ (B.t() if c["form"] == G.NT else B)
    pre = acc + d["bias"] if (d["bias"] is not None and c["epi"] in (G.BIAS_BF16, G.BIAS_GELU, G.BIAS_GELU_DG, G.BIAS_DROP_RESID)) else acc
    epi = c["epi"]
    if epi == G.BIAS_BF16:
        o["out_bf16"] = pre
    elif epi in (G.BIAS_GELU, G.BIAS_GELU_DG):
        u = pre.bfloat16().float()
        o["u"] = u
        o["out2_bf16"] = torch.nn.functional.gelu(u)
        phi = torch.exp(-0.5 * u * u) * (1 / math.sqrt(2 * math.pi))
        o["out_bf16"] = pre if epi == G.BIAS_GELU else 0.5 * (1 + torch.erf(u * (1 / math.sqrt(2)))) + u * phi
    elif epi == G.BIAS_DROP_RESID:
        km = G.keep_mult(c, d["row_map"])
        y = pre if km is None else pre * km.float()
        o["out_f32"] = y + d["resid"]
    elif epi == G.ADD_F32:
        o["out_f32"] = acc if d["resid"] is None else acc + d["resid"]
    else:
        aux = d["aux"].float()
        f = aux if epi == G.MUL_BF16 else 0.5 * (1 + torch.erf(aux * (1 / math.sqrt(2)))) + aux * torch.exp(-0.5 * aux * aux) * (1 / math.sqrt(2 * math.pi))
        v = acc * f
        o["out_bf16"] = v
        if c["colsum_part"]:
            o["colsum_part"] = G.tile_sums(v, c["M"])
    return o


BOUNDED = [c for c in G.CASES if not c["resid_ln"] and (c["data"] != "grid" or c["epi"] in (G.BIAS_GELU, G.BIAS_GELU_DG, G.DGELU_BF16))
           and c["M"] * c["N"] <= 640 * 1152]


def test_torch_fp32_within_half_of_every_bound():
    """Stock torch float32 on the CPU stays within half of every derived bound of the sweep, on every case that has one (the 2050 x 3072
    and 7937 x 2304 outputs left to their smaller twins: the same bounds at the same K).  bf16 outputs are judged before their rounding,
    against the bound without its bf16-rounding term: that term is the format's half unit in the last place, 2^-8 relative at worst,
    which one rounding of anything reaches."""
    worst = {}
    for c in BOUNDED:
        d = G.make_inputs(c)
        r = G.reference(c, d)
        got = _torch_f32(c, d)
        u = got["u"].double() if (c["data"] != "grid" and "u" in got) else None
        for k, f in G.worst_fractions(c, d, got, r, u, rounding=False).items():
            key = "%s/%s" % (G.EPI_NAME[c["epi"]] + ("" if c["data"] == "grid" else "_rand"), k)
            if f > worst.get(key, (0.0, ""))[0] or key not in worst:
                worst[key] = (f, c["name"])
    print("torch float32, worst fraction of each bound: " + "  ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(worst.items())))
    over = {k: v for k, v in worst.items() if not v[0] <= 0.5}
    assert not over, over
    assert len(worst) >= 10


def test_torch_fp32_layernorm_residual_within_half_of_its_row_bound():
    for c in (x for x in G.CASES if x["resid_ln"]):
        d = G.make_inputs(c)
        h = d["h"]
        mean = h.mean(1)
        stats = torch.stack([mean, 1 / torch.sqrt(h.var(1, unbiased=False) + 1e-12)], 1)
        res = G.resid_ln_rows64(d, stats)
        r = G.reference(c, d, resid_rows=res)
        x32 = torch.nn.functional.layer_norm(h, (c["N"],), d["gamma"], d["beta"], 1e-12)
        km = G.keep_mult(c, d["row_map"])
        pre = (d["A"].float() @ d["B"].float().t()) + d["bias"]
        got = (pre if km is None else pre * km.float()) + x32
        frac = (got.double() - r["out_f32"]).norm(dim=1) / G.resid_ln_row_bound(res, r["out_f32"])
        print("torch float32, %s: worst row %.3f of its bound" % (c["name"], float(frac.max())))
        assert float(frac.max()) <= 0.5, (c["name"], float(frac.max()))
