"""The restatements of tests/pdist_select_restate.py agree with each other, every float case meets the honesty condition (the same
selection in float32 numpy stays within half the bound of float64), the exact cases are exact, the designed cases hold what they are
designed for, and the host side of carel_pdist_select: ABI 9 unchanged, the symbols declared, bound and exported, the struct laid out as
the header says, the workspace size, every refusal before a launch (they need no GPU), the public names, and the refusal of a width
word other than "median".  The inputs of the case that pins the reason for the feature are checked against the float64 permutation
test here.  No GPU is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from tests import hsic_perm_restate as HR
from tests import pdist_select_restate as PS
from tests.test_hsic_perm_restate_host import _header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("carel_pdist_select_workspace_bytes", "carel_pdist_select")
SMALL = [c["name"] for c in PS.CASES if c["m"] <= PS.BIG]


@pytest.fixture(scope="module")
def lib():
    from carel_vae_amd import build
    build.build(verbose=False)
    return L.load()


def test_partition_sort_and_bincount_agree():
    for name in ("e_m3_d24", "e_m65_d1", "e_m129_d63", "e_m1000_d24"):
        c, x, ranks = PS.case_inputs(name)
        v, b, e = PS.select64(x, ranks)
        ref = PS.case_reference(name)
        assert np.array_equal(v, ref["values"]) and np.array_equal(b, ref["below"]) and np.array_equal(e, ref["equal"])
        assert np.array_equal(PS.upper32(x).astype(np.float64), PS.upper64(x)[0])              # float32 is exact on integers below 2^24
        assert np.array_equal(np.sort(PS.upper64(x)[0])[np.asarray(ranks)], v)
    c, x, _ = PS.case_inputs("f_m129_d24")
    D = PS.upper64(x)[0]
    assert D.shape == (PS.n_pairs(129),) and PS.quantile64(x, 0.5) == np.median(D)
    for q in (0.0, 0.3, 1.0):
        pos = (D.size - 1) * q
        lo = int(np.floor(pos))
        v = np.sort(D)[[lo, min(lo + 1, D.size - 1)]]
        assert abs(PS.quantile64(x, q) - (v[0] + (v[1] - v[0]) * (pos - lo))) <= 1e-15 * abs(v[1])


@pytest.mark.parametrize("name", SMALL)
def test_case_is_what_it_says_and_float32_numpy_is_within_half_the_bound(name):
    c, x, ranks = PS.case_inputs(name)
    m, d, N = c["m"], c["d"], PS.n_pairs(c["m"])
    assert x.shape == (m, d) and x.dtype == np.float32 and len(ranks) in (4, 8) and all(0 <= r < N for r in ranks)
    assert {0, N - 1, (N - 1) // 2, N // 2} <= set(ranks) and (c["ranks"] == "edges" or len(set(ranks)) < len(ranks) or N < 8)
    ref = PS.case_reference(name)
    assert (ref["below"] <= ranks).all() and (np.asarray(ranks) < ref["below"] + ref["equal"]).all()
    v32 = PS.select32(x, ranks)
    if c["kind"] == "exact":
        assert ref["bound"] == 0.0 and np.array_equal(v32.astype(np.float64), ref["values"])
        assert N < 8 or ref["equal"].max() > 1                                                 # ties are massive
        return
    worst = float(np.abs(v32.astype(np.float64) - ref["values"]).max() / ref["bound"])
    print("CASE %s bound %.3e float32 numpy at %.3f of it" % (name, ref["bound"], worst))
    assert ref["bound"] > 0 and worst <= 0.5
    if c["kind"] == "dup":
        z = PS.coinciding_pairs(x)
        D = np.sort(PS.upper64(x)[0])                    # (float64 sums in another order: its zeros are 1e-14, the device's are +0)
        assert z > 20 and np.abs(D[:z]).max() < 1e-12 and D[z] > 1.0 and abs(ref["values"][0]) < 1e-12
    if c["kind"] == "offset":
        D32 = PS.upper32(x)
        assert PS.upper64(x)[0].min() > 0 and (D32 < 0).sum() > 0.1 * N and np.abs(D32).max() <= ref["bound"]


def test_the_big_case_is_exact_and_the_list_covers_the_edges():
    c, x, ranks = PS.case_inputs("e_m8192_d24")
    ref = PS.case_reference("e_m8192_d24")
    N = PS.n_pairs(8192)
    assert N == 33550336 and ranks == [0, N - 1, (N - 1) // 2, N // 2] and ref["bound"] == 0.0
    assert (ref["below"] <= ranks).all() and (np.asarray(ranks) < ref["below"] + ref["equal"]).all() and ref["equal"].min() >= 1
    assert ref["values"][0] < ref["values"][2] <= ref["values"][3] < ref["values"][1]
    ms = {c["m"] for c in PS.CASES}
    assert {2, 3, PS.TILE - 1, PS.TILE, PS.TILE + 1, 2 * PS.TILE, 2 * PS.TILE + 1, 1000, PS.MAX_M} <= ms
    assert [c["m"] for c in PS.CASES].count(PS.MAX_M) == 1 and PS.by_name("e_m8192_d24")["kind"] == "exact"
    assert {1, 24, 63, 64} <= {c["d"] for c in PS.CASES} and any(c["pad"] for c in PS.CASES)
    assert {"float", "exact", "dup", "offset"} == {c["kind"] for c in PS.CASES} and {"edges", "eight"} == {c["ranks"] for c in PS.CASES}


def test_the_power_case_is_decided_at_the_median_widths():
    """the input condition of test_gpu_pdist_select.test_the_reason_for_the_feature: in float64, at the median widths, every
    permutation is decided (outside its rounding interval, with a margin of 100 bounds for the rounding of the widths themselves)
    and none reaches the observed statistic; at the default widths the off-diagonal of both Gram matrices underflows to exactly 0."""
    x, y, perms = PS.power_inputs()
    sx, sy = PS.quantile64(x, 0.5), PS.quantile64(y, 0.5)
    assert sx > 1000 and sy > 1000
    ref = HR.reference(HR.gram32(x, sx), HR.gram32(y, sy), perms)
    assert ref["decided"][1:].all() and ref["lo"] == ref["hi"] == 0
    gap = ref["stats"][0] - ref["stats"][1:].max()
    assert gap > 100 * (ref["bound"][0] + ref["bound"][1:].max())
    for s in (x, y):
        K = HR.gram32(s, 1.0)
        assert np.array_equal(K, np.eye(200, dtype=np.float32)) and PS.upper64(s)[0].min() > 200     # exp(-200) is far below float32


def test_abi_and_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    assert "#define CAREL_ABI_VERSION 9" in hdr and L.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    assert hdr.count("parity unpinned") >= 3
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name), name
    import carel_vae_amd as pkg
    for name in ("pdist_quantile", "median_heuristic", "median_alphas"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    from carel_vae_amd import ops
    assert callable(ops.pdist_select)


def test_struct_layout_matches_the_header():
    T = L.PdistSelectArgs
    want = dict(x=0, ldx=8, m=16, d=20, n_ranks=24, ranks=32, values=96, counts=104, workspace=112, workspace_bytes=120)
    assert {f[0]: getattr(T, f[0]).offset for f in T._fields_} == want and C.sizeof(T) == 128
    assert [n.split("[")[0] for n in _header_fields("carel_pdist_select_args")] == list(want)


def test_workspace_size(lib):
    f = lib.carel_pdist_select_workspace_bytes
    for m in (2, 3, 64, 1938, 8192):
        for n in range(1, 9):
            assert f(m, n) == PS.workspace_bytes(m, n) > 0 and f(m, n) % 16 == 0
    assert f(8192, 8) < 1 << 20
    for m, n in ((1, 2), (8193, 2), (100, 0), (100, 9), (-5, 2), (100, -1)):
        assert f(m, n) == 0 == PS.workspace_bytes(m, n)


def _valid_args(keep):
    """a call that would be accepted (m = 16, d = 24, ranks 0 and 119); the pointers are host buffers that a refused call never touches"""
    bufs = {k: C.create_string_buffer(80) for k in ("x", "values", "counts", "workspace")}
    keep.append(bufs)
    a = L.PdistSelectArgs()
    for k, b in bufs.items():
        setattr(a, k, (C.addressof(b) + 15) & ~15)
    a.ldx, a.m, a.d, a.n_ranks = 24, 16, 24, 2
    a.ranks[0], a.ranks[1] = 0, 119
    a.workspace_bytes = PS.workspace_bytes(16, 2)
    return a, bufs


def apply_refusal(a, what):
    """makes the valid call `a` wrong in the way `what` names"""
    if "null" in what:
        setattr(a, what["null"], None)
    for k in ("m", "d", "ldx", "n_ranks"):
        if k in what:
            setattr(a, k, what[k])
    if "rank" in what:
        a.ranks[1] = what["rank"]
    if what.get("short_workspace"):
        a.workspace_bytes -= 1
    if what.get("misaligned_workspace"):
        a.workspace += 8


@pytest.mark.parametrize("what,code", PS.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in PS.REFUSALS])
def test_refusals_need_no_gpu(lib, what, code):
    keep = []
    a, bufs = _valid_args(keep)
    apply_refusal(a, what)
    before = {k: bytes(b.raw) for k, b in bufs.items()}
    assert lib.carel_pdist_select(C.byref(a), None) == code
    assert lib.carel_last_error().startswith(b"carel_pdist_select")
    assert {k: bytes(b.raw) for k, b in bufs.items()} == before
    assert lib.carel_pdist_select(None, None) == PS.ERR_ARG and lib.carel_last_error().startswith(b"carel_pdist_select")


def test_a_width_word_other_than_median_is_refused_by_name():
    from carel_vae_amd import drl_classifier as M
    x = torch.zeros(8, 3)
    model = M.DrlClassifier(M.make_opt(pair_bow_dim=50), M.encoder_config("zh", vocab_size=100, layers=1))
    lat = torch.zeros(8, 4 * model.opt.ec_dim)
    for call in (lambda: M.hsic_independence_test(x, x, "mean", 1.0), lambda: M.hsic_independence_test(x, x, 1.0, "Median"),
                 lambda: M.mmd_two_sample_test(x, x, "medians"), lambda: model.latent_independence_test(lat, 10, s_c="auto"),
                 lambda: model.latent_two_sample_test(lat, 10, alphas="mean")):
        with pytest.raises(L.CarelError, match='"median"'):
            call()


def test_without_a_gpu_the_public_names_are_refused_not_computed():
    from carel_vae_amd import drl_classifier as M
    x = torch.rand(8, 3)
    if torch.cuda.is_available():
        assert M.median_heuristic(x) == M.pdist_quantile(x, 0.5) > 0.0
        return
    model = M.DrlClassifier(M.make_opt(pair_bow_dim=50), M.encoder_config("zh", vocab_size=100, layers=1))
    lat = torch.zeros(8, 4 * model.opt.ec_dim)
    for call in (lambda: M.pdist_quantile(x, 0.25), lambda: M.median_heuristic(x), lambda: M.median_alphas(x, x, (1.0, 2.0)),
                 lambda: M.hsic_independence_test(x, x, "median", "median", 5), lambda: M.mmd_two_sample_test(x, x, "median", 5),
                 lambda: model.latent_independence_test(lat, 5, s_e="median", s_c="median"),
                 lambda: model.latent_two_sample_test(lat, 5, alphas="median")):
        with pytest.raises(L.CarelError, match="GPU|CUDA|cuda"):
            call()
