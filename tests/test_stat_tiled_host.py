"""The host side of the tiled differentiable statistics (carel_hsic_tiled_fwd/bwd, carel_rbf_mmd_tiled_fwd/bwd), without a GPU: the
symbols are exported and bound, the workspace functions return what include/carel_hip.h states, every refusal comes back with its code
and the entry point's name before anything could be launched, the Python dispatch threshold is the single-workgroup LDS limit, the
cases of tests/test_gpu_stat_tiled.py meet the input conditions of tests/stats_restate.py, the chain lengths of the tile plan are what
tests/stat_tiled_restate.py says of them, and stock torch float32 on the CPU stays within HALF of the bounds the kernels are held to
on those cases (the condition that keeps the bounds' constants honest, as in tests/test_stats_restate_host.py).  Run with -s for the
worst fractions.

torch float32 on the CPU, worst fraction of the bound over the cases of the GPU test: see DESIGN.md 4.17."""
import ctypes as C

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests import stat_tiled_restate as T
from tests import stats_restate as R
from tests.test_stats_restate_host import _sign_margin

NEW = ("carel_hsic_tiled_workspace_bytes", "carel_hsic_tiled_fwd", "carel_hsic_tiled_bwd", "carel_rbf_mmd_tiled_workspace_bytes",
       "carel_rbf_mmd_tiled_fwd", "carel_rbf_mmd_tiled_bwd")


def test_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    for n in NEW:
        assert n in L.SIGNATURES and hasattr(lib, n)
    assert lib.carel_abi_version() == L.ABI_VERSION == 9
    for n in ("hsic_tiled", "hsic_tiled_backward", "rbf_mmd_tiled", "rbf_mmd_tiled_backward"):
        assert callable(getattr(ops, n))


def test_workspace_functions_follow_the_header():
    lib = L.load()
    for m in (2, 3, 63, 64, 65, 129, 757, 800, 1938, 2049, 4097, 8191, 8192):
        for d in (1, 16, 24, 64):
            assert lib.carel_hsic_tiled_workspace_bytes(m, d) == T.hsic_workspace_bytes(m, d) > 0, (m, d)
    for n1, n2 in ((2, 2), (2, 63), (65, 64), (800, 800), (1938, 1938), (4096, 4096), (2, 8190)):
        for d in (1, 24, 64):
            assert lib.carel_rbf_mmd_tiled_workspace_bytes(n1, n2, d) == T.mmd_workspace_bytes(n1, n2, d) > 0, (n1, n2, d)
    for m, d in ((1, 24), (0, 24), (-5, 24), (8193, 24), (64, 0), (64, 65)):
        assert lib.carel_hsic_tiled_workspace_bytes(m, d) == 0
    for n1, n2, d in ((1, 8, 24), (8, 1, 24), (4097, 4096, 24), (8, 8, 0), (8, 8, 65), (2 ** 31 - 1, 2 ** 31 - 1, 24)):
        assert lib.carel_rbf_mmd_tiled_workspace_bytes(n1, n2, d) == 0
    # O(m * tiles) floats for the partials, never O(m^2 d): the largest shape stays below 64 MB
    assert lib.carel_hsic_tiled_workspace_bytes(8192, 64) < 64 << 20 and lib.carel_rbf_mmd_tiled_workspace_bytes(4096, 4096, 64) < 64 << 20


def test_the_split_plan():
    assert [T.split(t) for t in (1, 2, 13, 31, 32, 33, 64, 128)] == [(1, 1), (1, 2), (1, 13), (1, 31), (1, 32), (2, 17), (4, 16), (16, 8)]
    for rows in range(2, T.MAX_ROWS + 1, 37):
        t = T.tiles(rows)
        per, S = T.split(t)
        assert per * S >= t > per * (S - 1) and S * t <= 1024 + t           # every tile in one run, no empty run, about 1024 workgroups


# ------------------------------------------------------------------------------------------------ refusals, with a NULL stream and no GPU
_FAKE = 0x1000          # a non-NULL, 8-byte aligned address that a refused call never touches


def _hsic_call(p):
    a = L.HsicArgs()
    d = p.get("d", 24)
    a.x, a.y, a.ldx, a.ldy, a.m, a.d = _FAKE, _FAKE, p.get("ldx", max(d, 1)), max(d, 1), p.get("m", 8), d
    a.s_x, a.s_y = p.get("s", (1.0, 1.0))
    a.hsic_out, a.gx, a.gy = _FAKE, _FAKE, _FAKE
    work = _FAKE
    null = p.get("null")
    if null in ("x", "y"):
        setattr(a, null, None)
    elif null == "out":
        a.hsic_out, a.gx = None, None
    elif null == "work":
        work = None
    return a, work


def _mmd_call(p):
    a = L.MmdArgs()
    d = p.get("d", 24)
    a.s1, a.s2, a.ld1, a.ld2 = _FAKE, _FAKE, p.get("ld1", max(d, 1)), max(d, 1)
    a.n1, a.n2, a.d, a.n_alphas, a.eps = p.get("n1", 8), p.get("n2", 8), d, p.get("n_alphas", 1), 1e-5
    a.alphas[0] = 0.1
    a.mmd_out, a.g1, a.g2 = _FAKE, _FAKE, _FAKE
    work = _FAKE
    null = p.get("null")
    if null in ("s1", "s2"):
        setattr(a, null, None)
    elif null == "out":
        a.mmd_out, a.g1 = None, None
    elif null == "work":
        work = None
    return a, work


@pytest.mark.parametrize("r", T.REFUSALS, ids=T.refusal_id)
def test_every_refusal_names_its_entry_point(r):
    op, p, want = r
    lib = L.load()
    a, work = (_hsic_call if op == "hsic" else _mmd_call)(p)
    names = ("carel_hsic_tiled_fwd", "carel_hsic_tiled_bwd") if op == "hsic" else ("carel_rbf_mmd_tiled_fwd", "carel_rbf_mmd_tiled_bwd")
    for n in names:
        assert getattr(lib, n)(C.byref(a), work, None) == want, (n, p)
        assert lib.carel_last_error().startswith(n.encode() + b":"), lib.carel_last_error()


def test_null_struct_and_misaligned_workspace_are_refused():
    lib = L.load()
    for n in NEW:
        if n.endswith("_bytes"):
            continue
        assert getattr(lib, n)(None, _FAKE, None) == T.ERR_ARG and lib.carel_last_error().startswith(n.encode())
    a, _ = _hsic_call({})
    assert lib.carel_hsic_tiled_fwd(C.byref(a), _FAKE + 4, None) == T.ERR_ARG and b"aligned" in lib.carel_last_error()
    b, _ = _mmd_call({})
    assert lib.carel_rbf_mmd_tiled_bwd(C.byref(b), _FAKE + 4, None) == T.ERR_ARG and b"aligned" in lib.carel_last_error()
    # the single-workgroup entries keep their refusals one past the LDS limit
    for op, p, want in R.REFUSALS:
        if op == "hsic" and p["m"] > 700:
            a, _ = _hsic_call(dict(m=p["m"], d=p["d"]))
            assert lib.carel_hsic_fwd(C.byref(a), None) == want == T.ERR_SHAPE


# ------------------------------------------------------------------------------------------------ the dispatch threshold
def test_dispatch_threshold_is_the_single_workgroup_lds_limit():
    for d in (16, 24, 64):
        assert ops.hsic_single_limit(d) == R.largest_accepted(R.hsic_lds_floats, d)
        assert ops.mmd_single_limit(d) == R.largest_accepted(R.mmd_lds_floats, d)
    assert ops.hsic_single_limit(24) == 757 and ops.mmd_single_limit(24) == 1572 and ops.mmd_single_limit(64) == 619
    on_cpu = lambda *shape: torch.zeros(shape)
    assert not ops._hsic_goes_tiled(on_cpu(757, 24)) and ops._hsic_goes_tiled(on_cpu(758, 24)) and ops._hsic_goes_tiled(on_cpu(8192, 24))
    assert not ops._hsic_goes_tiled(on_cpu(8193, 24)) and not ops._hsic_goes_tiled(on_cpu(800, 65))      # those keep the old refusal
    assert not ops._mmd_goes_tiled(on_cpu(700, 24), on_cpu(872, 24)) and ops._mmd_goes_tiled(on_cpu(700, 24), on_cpu(873, 24))
    assert not ops._mmd_goes_tiled(on_cpu(1, 24), on_cpu(2000, 24)) and not ops._mmd_goes_tiled(on_cpu(4097, 24), on_cpu(4096, 24))


# ------------------------------------------------------------------------------------------------ the cases and the chains
def test_every_case_meets_the_input_conditions():
    for c in T.MMD_CASES:
        s1, s2 = R.mmd_inputs(c)
        assert s1.shape == (c["n1"], c["d"]) and s2.shape == (c["n2"], c["d"]) and s1.dtype == s2.dtype == np.float32
        z = np.concatenate((s1, s2), 0)
        allow = (c["dup"][0], c["n1"] + c["dup"][1]) if c.get("dup") else None
        assert _sign_margin(z, allow=allow) >= R.SIGN_MARGIN, c["name"]
        d2, _ = R.pair_terms(z.astype(np.float64))
        arg = max(R.f32_scalars(c["alphas"])) * (R.f32_scalars([c["eps"]])[0] + np.abs(d2).max())
        assert 1.0 <= arg <= 20.0, (c["name"], arg)
    for c in T.HSIC_CASES:
        x, y = R.hsic_inputs(c)
        assert x.shape == y.shape == (c["m"], c["d"])
        args = [R.pair_terms(t.astype(np.float64))[0] / s for t, s in zip((x, y), c["s"])]
        assert all(a.min() >= 0.0 and a.max() <= 20.0 for a in args), c["name"]
    assert R.hsic_lds_floats(T.HSIC_ABOVE["m"], T.HSIC_ABOVE["d"]) > R.LDS_FLOATS
    assert R.mmd_lds_floats(T.MMD_ABOVE["n1"] + T.MMD_ABOVE["n2"], T.MMD_ABOVE["d"]) > R.LDS_FLOATS
    assert {c["m"] for c in T.HSIC_SMALL} == {2, 3, 63, 64, 65, 129} and {1, 24, 63, 64} <= {c["d"] for c in T.HSIC_SMALL}
    assert {(c["n1"], c["n2"]) for c in T.MMD_SMALL} == {(2, 2), (2, 63), (33, 31), (64, 64), (65, 64)}
    assert {1, 63, 64} <= {c["d"] for c in T.MMD_SMALL} and {len(c["alphas"]) for c in T.MMD_SMALL} == {1, 3, 8}
    assert any(c.get("strided") for c in T.HSIC_SMALL) and any(c["gs"] is None for c in T.HSIC_SMALL) and any(c["corr"] for c in T.HSIC_SMALL)
    assert any(c.get("strided") for c in T.MMD_SMALL) and any(c["gs"] is None for c in T.MMD_SMALL) and any(c.get("dup") for c in T.MMD_SMALL)


def test_tiled_chains_against_the_single_workgroup_ones():
    """HSIC and the MMD value keep the bounds of stats_restate (every tiled chain is at most the chain it stands for, at EVERY size the
    tiled entries accept); the MMD gradient is the one that had to be restated, and only below 1025 rows is its chain the longer one."""
    for m in range(2, T.MAX_ROWS + 1):
        assert min(m, T.SUM_CHAIN) <= R.chain_hsic_row(m) and T.grad_chain(m) <= R.chain_hsic_row(m), m
        assert T.TOTAL_CHAIN <= R.chain_block(m) and T.SUM_CHAIN <= R.chain_mmd_fwd(max(m, 4))
    assert (T.grad_chain(4), R.chain_mmd_bwd(4)) == (4, 4) and (T.grad_chain(128), R.chain_mmd_bwd(128)) == (65, 19)
    assert (T.grad_chain(1572), R.chain_mmd_bwd(1572)) == (88, 1572) and T.grad_chain(8192) == 64 * 16 + 7
    assert all(T.grad_chain(n) < R.chain_mmd_bwd(n) for n in range(1025, 1573))
    keep = R.chain_mmd_bwd
    T.mmd_reference("t_2_2")
    assert R.chain_mmd_bwd is keep                                                # the restated bound leaves stats_restate as it found it


def test_blocked_float64_restatement_equals_hsic_closed():
    """hsic_rows_closed (the m = 8192 reference of the GPU test) against stats_restate.hsic_closed on a case of three row blocks"""
    c, x, y, gs, ref, bound = T.hsic_reference("t_129_d33")
    rows = (0, 1, 64, 127, 128)
    r2, b2 = T.hsic_rows_closed(x, y, *c["s"], gs, rows, block=50)
    assert abs(r2["hsic"] - ref["hsic"]) <= 1e-12 * sum(ref["terms"]) and abs(b2["hsic"] - bound["hsic"]) <= 1e-9 * bound["hsic"]
    for k in ("gx", "gy"):
        np.testing.assert_allclose(r2[k], ref[k][list(rows)], rtol=0, atol=1e-12 * np.abs(ref[k]).max())
        np.testing.assert_allclose(b2[k], bound[k][list(rows)], rtol=1e-9)
    assert b2["perm"] > 0


# ------------------------------------------------------------------------------------------------ torch float32 within half of every bound
def _report(tag, worst):
    print("torch float32, worst fraction of the tiled bound, %s: " % tag + ", ".join("%s %.3f" % kv for kv in worst.items()))
    assert all(v <= 0.5 for v in worst.values()), (tag, worst)


def test_torch_fp32_within_half_of_every_tiled_bound_mmd():
    worst = {}
    for c in T.MMD_CASES:
        _, s1, s2, gs, ref, b = T.mmd_reference(c["name"])
        got = R.mmd_literal(s1, s2, c["alphas"], c["eps"], gs, dtype=torch.float32)
        for k in ("mmd", "g1", "g2"):
            worst[k] = max(worst.get(k, 0.0), R.frac(got[k], ref[k], b[k]))
    _report("MMD", worst)


def test_torch_fp32_within_half_of_every_tiled_bound_hsic():
    for tag, form in (("matrix form", R.hsic_formula), ("three sums", R.hsic_three_sum_formula)):
        worst = {}
        for c in T.HSIC_CASES:
            _, x, y, gs, ref, b = T.hsic_reference(c["name"])
            got = R.hsic_literal(x, y, *c["s"], gs, dtype=torch.float32, form=form)
            for k in ("hsic", "gx", "gy"):
                worst[k] = max(worst.get(k, 0.0), R.frac(got[k], ref[k], b[k]))
        _report("HSIC " + tag, worst)
