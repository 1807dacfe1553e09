"""Coverage of the packed-step sweep (tests/test_gpu_packed_sweep.py), without a GPU.

A packed ECPE batch reaches the encoder with its own token count T (a multiple of 128, drl_classifier.py `_pack_info`), and several
kernel choices of the library are functions of T.  This test enumerates T = 128 k <= 8192, asks the library -- not a Python copy of its
thresholds -- what it decides at each T, and asserts that the sweep's T list holds a representative of every distinct decision tuple,
so that retuning a constant that moves a regime boundary makes this test name the T the sweep is missing.

Decisions in the tuple, for the three-layer packed step the sweep runs (full layers 0 and 1, [CLS]-only layer 2):
  * every forward / data-gradient GEMM with M = T rows, as the encoder issues it (encoder.hip forward_layers /
    carel_encoder_backward_layer: same form, epilogue, N, K, residual-LayerNorm inputs, chain count and split-K workspace bytes):
    (fp32 slabs of the internal split-K path, kernel family, ping-pong tile width npn) from carel_gemm_split_plan, the plan
    the encoder itself asks for and every launch executes (gemm.hip gemm_plan: auto_splits, split_pp_npn, gemm_pp_pick with
    g_pp_min_tiles / g_pp_min_tiles_k768, resid_split, big_auto).  A slab count > 1 on the FFN1 / QKV data gradient or the out-projection / FFN2 forward is also the
    decision to defer the slab epilogue into the LayerNorm behind it, and the next layer's `dx_in_slabs`;
  * the weight gradients: whether the grouped launch runs (carel_gemm_wgrad_group_ws_bytes against the encoder's slab area,
    carel_encoder_workspace_bytes) and its workspace (the grouped launch's K-split factor), else the split factor of each
    weight gradient (carel_gemm_wgrad_splits) and its kernel (carel_gemm_split_plan on the TN form); the [CLS]-only layer's QKV
    weight gradient (T rows, never grouped) likewise;
  * the LayerNorm backward's rows per wave, from carel_layernorm_bwd_blocks (ln.hip ln_bwd_rpw).
Not in the tuple, covered by the explicit T values of the sweep instead:
  * the row-band GEMM + LayerNorm kernel (gemm.hip gemm_rowln_wanted, encoder.hip:298 / :317): the experiments build only, never on
    the product path the sweep runs;
  * the [CLS]-only layer's row-wise GEMMs: M = 128 whatever T (GEMM_EX_FIXED_ROWS), one plan for every T;
  * the embedding backward (ln.hip embed_ln_bwd_ex) and the attention kernels: per sample / per row, no T-dependent dispatch."""
import ctypes as C

import pytest

from carel_vae_amd import _lib as L

EH, EI = 768, 3072
B, S = 64, 128
T_ALL = list(range(128, B * S + 1, 128))
_BIG = 1 << 40              # a fake, aligned address: the plan checks the operands' alignment but never reads them


def _plan(lib, form, epi, M, N, K, flags=1, ws_bytes=0, lnres=False, splits=1):
    a = L.GemmArgs()
    a.A = a.B = _BIG
    a.lda = K if form != L.GEMM_TN else M
    a.ldb = N if form != L.GEMM_NT else K
    a.ldc = N
    a.M, a.N, a.K, a.form, a.epilogue, a.splits = M, N, K, form, epi, splits
    a.out_bf16 = a.out2_bf16 = a.out_f32 = a.bias = a.resid_f32 = a.aux_bf16 = _BIG
    if ws_bytes:
        a.splitk_ws, a.splitk_ws_bytes = _BIG, ws_bytes
        a.splitk_ws_zeroed = 1 if (flags & 0xff) == 1 else 0           # encoder.hip gemm_call
    if lnres:
        a.resid_ln_stats = a.resid_ln_gamma = a.resid_ln_beta = _BIG
    out = (C.c_int32 * 3)()
    L.check(lib.carel_gemm_split_plan(C.byref(a), flags, out), "carel_gemm_split_plan")
    return tuple(out)


def _wgrad_group_bytes(lib, T):
    ga = L.WgradGroupArgs()
    for i, (m, n) in enumerate(((EH, EI), (EI, EH), (3 * EH, EH), (EH, EH))):       # encoder.hip carel_encoder_backward_layer: ga.prob
        ga.prob[i] = L.WgradProblem(_BIG, _BIG, _BIG, _BIG, m, n)
    ga.n_prob, ga.T = 4, T
    return lib.carel_gemm_wgrad_group_ws_bytes(C.byref(ga))


def decisions(lib, T):
    """The tuple of row-count-dependent decisions of the packed step at T rows (module docstring)."""
    ws = lib.carel_encoder_workspace_bytes(B, S, 0)
    slab = lib.carel_encoder_workspace_bytes(B, S, 1)
    NT, NN, TN = L.GEMM_NT, L.GEMM_NN, L.GEMM_TN
    d = {
        "fwd_qkv": _plan(lib, NT, L.EPI_BIAS_BF16, T, 3 * EH, EH, ws_bytes=ws),
        "fwd_out_l0": _plan(lib, NT, L.EPI_BIAS_DROP_RESID, T, EH, EH, ws_bytes=ws),                  # residual = the embedding output rows
        "fwd_out": _plan(lib, NT, L.EPI_BIAS_DROP_RESID, T, EH, EH, ws_bytes=ws, lnres=True),          # residual recomputed from LayerNorm 2 below
        "fwd_ffn1": _plan(lib, NT, L.EPI_BIAS_GELU_DG, T, EI, EH, ws_bytes=ws),
        "fwd_ffn2": _plan(lib, NT, L.EPI_BIAS_DROP_RESID, T, EH, EI, ws_bytes=ws, lnres=True),
        "bwd_qkv": _plan(lib, NN, L.EPI_ADD_F32, T, EH, 3 * EH, ws_bytes=ws),
        "bwd_ffn2": _plan(lib, NN, L.EPI_MUL_BF16, T, EI, EH),
        "bwd_ffn1": _plan(lib, NN, L.EPI_ADD_F32, T, EH, EI, ws_bytes=ws),
        "bwd_out": _plan(lib, NN, L.EPI_BIAS_BF16, T, EH, EH, ws_bytes=ws),
        "ln_bwd_rows_per_wave": T // (4 * lib.carel_layernorm_bwd_blocks(T)),
    }
    need = _wgrad_group_bytes(lib, T)
    grouped = 0 <= need <= slab
    d["wgrad_group"] = need if grouped else None
    for name, (m, n) in (("wgrad_ffn2", (EH, EI)), ("wgrad_ffn1", (EI, EH)), ("wgrad_qkv", (3 * EH, EH)), ("wgrad_out", (EH, EH))):
        if grouped and name != "wgrad_qkv":          # (the [CLS]-only layer's QKV weight gradient is never grouped)
            continue
        s = lib.carel_gemm_wgrad_splits(m, n, T)
        d[name] = (s, _plan(lib, TN, L.EPI_SLAB_F32, m, n, T, splits=s))
    return d


def regimes(lib):
    """{decision tuple: [every T = 128 k <= 8192 that makes it]}"""
    groups = {}
    for T in T_ALL:
        groups.setdefault(tuple(sorted(decisions(lib, T).items())), []).append(T)
    return groups


@pytest.fixture(scope="module")
def exp_lib():
    from carel_vae_amd import build
    build.build(verbose=False)
    return L.load_experiments()


def test_the_sweep_has_a_token_count_in_every_dispatch_regime(exp_lib):
    from tests.test_gpu_packed_sweep import SWEEP_T
    assert set(SWEEP_T) <= set(T_ALL) and len(set(SWEEP_T)) == len(SWEEP_T)
    groups = regimes(exp_lib)
    missing = {tuple(ts): dict(key) for key, ts in groups.items() if not set(ts) & set(SWEEP_T)}
    assert not missing, "regimes without a T in tests/test_gpu_packed_sweep.py SWEEP_T (T values that would cover them -> decisions): %r" % missing
    # (the regimes the sweep is documented to cross, so that a tuple that stopped moving at all is noticed too)
    assert len(groups) >= 12, len(groups)


def test_the_plan_sees_the_regime_boundaries_the_encoder_is_tuned_for(exp_lib):
    """Spot checks of the plan wrapper against the packed step as DESIGN.md describes it: at the bench's ~1.8 k packed rows the
    K = 3072 / 2304 data-gradient GEMMs and the FFN2 forward run as 4 K slices on the ping-pong kernel (slab epilogue deferred into the
    LayerNorm behind them), at 8192 rows everything runs in one pass; the LayerNorm backward has 1 / 2 / 4 rows per wave below 2048 /
    4096 / above."""
    d = decisions(exp_lib, 1792)
    assert d["bwd_ffn1"] == (4, 4, 1) and d["bwd_qkv"][:2] == (4, 4) and d["fwd_ffn2"][:2] == (4, 4), d
    d = decisions(exp_lib, 8192)
    assert all(d[k][0] == 1 and d[k][1] == 1 for k in d if k.startswith(("fwd_", "bwd_"))), d
    assert d["wgrad_group"] is not None and d["wgrad_group"] <= exp_lib.carel_encoder_workspace_bytes(B, S, 1)
    assert [decisions(exp_lib, T)["ln_bwd_rows_per_wave"] for T in (2048, 2176, 4096, 4224)] == [1, 2, 2, 4]


def test_the_plan_is_true_under_hooks(exp_lib):
    """carel_gemm_split_plan reports what carel_gemm_bf16 launches when a kernel is forced (carel_gemm_set_variant 1 / 2 / 3), not
    "not planned": 1792 x 2304 are multiples of the 128 x 128 and of the 256 x 192 tile, and no forced variant splits along K."""
    PLAN_PP, PLAN_128, PLAN_BIG = 1, 2, 3          # CAREL_PLAN_* (include/carel_hip_experiments.h)

    def plan():
        return _plan(exp_lib, L.GEMM_NT, L.EPI_BIAS_BF16, 1792, 2304, 768, ws_bytes=1 << 26)

    before = plan()
    try:
        L.check(exp_lib.carel_gemm_set_variant(1))
        assert plan() == (1, PLAN_128, 0)
        L.check(exp_lib.carel_gemm_set_variant(2))
        assert plan() == (1, PLAN_BIG, 0)
        L.check(exp_lib.carel_gemm_set_variant(3))
        forced_pp = plan()
        assert forced_pp[:2] == (1, PLAN_PP) and 1 <= forced_pp[2] <= 3, forced_pp
    finally:
        L.check(exp_lib.carel_gemm_set_variant(0))
    assert plan() == before


def test_split_plan_refuses_launch_flags(exp_lib):
    a = L.GemmArgs()
    out = (C.c_int32 * 3)()
    assert exp_lib.carel_gemm_split_plan(C.byref(a), 1, None) == -1
    assert exp_lib.carel_gemm_split_plan(C.byref(a), 0x200, out) == -1            # (GEMM_EX_DEFER_EPILOGUE is not a plan input)
    assert exp_lib.carel_encoder_workspace_bytes(B, S, 2) == -1
