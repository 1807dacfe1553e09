"""The float64 restatements of the permutation test (tests/perm_restate.py) agree with each other, every committed case meets the input
condition (at most 5 % of its labellings undecided against the bound, three cases with a count away from 0 and P), and the host side
of the new entry points: ABI 9 unchanged, the symbols declared, bound and exported, the struct laid out as the header says, and every
refusal of carel_mmd_perm_test / carel_rbf_gram / carel_sample_latents before a launch (they need no GPU).  No GPU is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from tests import perm_restate as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("carel_rbf_gram", "carel_mmd_perm_workspace_bytes", "carel_mmd_perm_test", "carel_sample_latents")


@pytest.fixture(scope="module")
def lib():
    from carel_vae_amd import build
    build.build(verbose=False)
    return L.load()


def test_the_two_restatements_agree():
    rs = np.random.RandomState(3)
    for n1, n2 in ((2, 2), (2, 5), (7, 6), (17, 20)):
        n = n1 + n2
        M = rs.uniform(0.1, 1.0, size=(n, n)).astype(np.float32)          # not symmetric
        M[np.diag_indices(n)] = rs.uniform(5.0, 9.0, size=n)              # a diagonal that would show if it were used
        labels = PR.random_labels(n1, n2, 6, 10 + n)
        for coef in (PR.mmd_coefficients(n1, n2), (1.0, 0.0, 1.0), (0.3, -1.1, 0.7)):
            quad = PR.stats_quadratic(M, labels, coef)
            scale = sum(abs(c) for c in coef) * np.abs(M).sum()
            for p in range(labels.shape[0]):
                assert abs(PR.stat_loop(M, labels[p], coef) - quad[p]) <= 1e-13 * scale
        S00, S11, S01 = PR.three_sums(M, labels)
        off = M.astype(np.float64).sum() - np.trace(M.astype(np.float64))
        assert np.allclose(S00 + S11 + S01, off, rtol=1e-13)
    # the observed labelling with MMDStatistic's coefficients is the MMD statistic
    from tests import stats_restate as R
    c, s1, s2, _, ref, _ = R.mmd_reference("g8_64_64_equal")
    got = PR.stats_quadratic(ref["kern"], PR.observed(64, 64)[None], PR.mmd_coefficients(64, 64))[0]
    assert abs(got - ref["mmd"]) <= 1e-12 * abs(ref["mmd"]) + 1e-15


@pytest.mark.parametrize("name", [c["name"] for c in PR.CASES])
def test_case_meets_the_input_condition(name):
    c, s1, s2, M, labels, coef = PR.case_inputs(name)
    n, P = c["n1"] + c["n2"], c["P"]
    assert M.shape == (n, n) and M.dtype == np.float32 and labels.shape == (P + 1, n) and labels.dtype == np.uint8
    assert np.array_equal(labels[0], PR.observed(c["n1"], c["n2"])) and (labels.sum(1) == c["n2"]).all() and labels.max() == 1
    if c["kind"] == "nonsym":
        assert np.abs(M - M.T).max() > 0.01 * np.abs(M).max()
    ref = PR.case_reference(name)
    undecided = int((~ref["decided"])[1:].sum())
    print("CASE %s undecided %d / %d count %d..%d" % (name, undecided, P, ref["lo"], ref["hi"]))
    assert undecided <= PR.MAX_UNDECIDED * P
    assert (ref["bound"] > 0).all() and ref["bound"].max() < 1e-3 * np.abs(ref["stats"]).max() + 1e-4


def test_three_cases_have_a_count_away_from_the_ends():
    mid = [c["name"] for c in PR.CASES if 0.1 * c["P"] <= PR.case_reference(c["name"])["lo"]
           and PR.case_reference(c["name"])["hi"] <= 0.9 * c["P"]]
    assert len(mid) >= 3, mid


def test_case_list_covers_the_tile_edges():
    ns = {c["n1"] + c["n2"] for c in PR.CASES}
    assert {4, 31, 32, 33, 64, 65, 129, 257} <= ns and {PR.CHUNK - 1, PR.CHUNK, PR.CHUNK + 1, 2 * PR.CHUNK + 1} <= ns
    assert {2, 32, 33, 65, 1001, PR.LABS_WG, PR.LABS_WG + 1} <= {c["P"] + 1 for c in PR.CASES}
    assert any(c["n1"] == 2 for c in PR.CASES) and any(c["n1"] != c["n2"] for c in PR.CASES)
    assert {len(c["alphas"]) for c in PR.CASES if c["kind"] == "gram"} == {1, 3, 8}


def test_abi_and_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    assert "#define CAREL_ABI_VERSION 9" in hdr and L.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name), name
    import carel_vae_amd as pkg
    for name in ("permutation_test_mat", "mmd_two_sample_test", "random_labellings", "MMDStatistic"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.DrlClassifier.latent_two_sample_test)


def test_struct_layout_matches_the_header():
    T = L.MmdPermArgs
    want = dict(matrix=0, ldm=8, labels=16, n1=24, n2=28, n_permutations=32, a00=40, a01=48, a11=56, stats=64, count=72, workspace=80,
                workspace_bytes=88)
    assert {f[0]: getattr(T, f[0]).offset for f in T._fields_} == want and C.sizeof(T) == 96
    body = re.search(r"typedef struct carel_mmd_perm_args \{(.*?)\} carel_mmd_perm_args;", open(os.path.join(ROOT, "include", "carel_hip.h")).read(),
                     flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:                                         # "type a, b": the first name follows the type, the others stand alone
            parts = decl.split(",")
            names += [parts[0].split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in parts[1:]]
    assert names == list(want), names                    # the same fields in the same order


def test_workspace_size(lib):
    f = lib.carel_mmd_perm_workspace_bytes
    for n, P in ((4, 1), (31, 31), (32, 1000), (33, 1), (3876, 1000), (8192, 65535)):
        assert f(n, P) == PR.workspace_bytes(n, P) > 0
    for n, P in ((3, 10), (8193, 10), (100, 0), (100, 65536)):
        assert f(n, P) == 0


def _valid_args(keep, n1=8, n2=8, P=4):
    """a call that would be accepted; the pointers are host buffers that a refused call never touches"""
    n = n1 + n2
    need = max(PR.workspace_bytes(n, P), 8) if 4 <= n <= PR.MAX_N and 1 <= P <= PR.MAX_P else 64
    bufs = dict(matrix=C.create_string_buffer(64), labels=C.create_string_buffer(64), stats=C.create_string_buffer(64),
                count=C.create_string_buffer(64), workspace=C.create_string_buffer(64))
    keep.append(bufs)
    a = L.MmdPermArgs()
    for k, b in bufs.items():
        setattr(a, k, C.addressof(b))
    a.ldm, a.n1, a.n2, a.n_permutations = n, n1, n2, P
    a.a00, a.a01, a.a11 = PR.mmd_coefficients(n1, n2) if n1 > 1 and n2 > 1 else (1.0, 0.0, 1.0)
    a.workspace_bytes = need
    return a, bufs


@pytest.mark.parametrize("what,code", PR.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in PR.REFUSALS])
def test_perm_test_refusals_need_no_gpu(lib, what, code):
    keep = []
    a, bufs = _valid_args(keep, n1=what.get("n1", 8), n2=what.get("n2", 8), P=what.get("P", 4))
    if "null" in what:
        setattr(a, what["null"], None)
    if what.get("short_workspace"):
        a.workspace_bytes -= 1
    if "ldm" in what:
        a.ldm = what["ldm"]
    before = {k: bytes(b.raw) for k, b in bufs.items()}
    assert lib.carel_mmd_perm_test(C.byref(a), None) == code
    assert lib.carel_last_error().startswith(b"carel_mmd_perm_test")
    assert {k: bytes(b.raw) for k, b in bufs.items()} == before
    assert lib.carel_mmd_perm_test(None, None) == PR.ERR_ARG


def test_gram_and_sample_refusals_need_no_gpu(lib):
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def gram(**kw):
        a = L.MmdArgs()
        a.s1, a.s2, a.kernels_out, a.ld1, a.ld2, a.n1, a.n2, a.d, a.n_alphas, a.eps = p, p, p, 24, 24, 8, 8, 24, 1, 1e-5
        a.alphas[0] = 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.carel_rbf_gram(C.byref(a), None)
    assert lib.carel_rbf_gram(None, None) == PR.ERR_ARG
    for kw, code in ((dict(s1=None), PR.ERR_ARG), (dict(s2=None), PR.ERR_ARG), (dict(kernels_out=None), PR.ERR_ARG), (dict(n_alphas=0), PR.ERR_ARG),
                     (dict(n_alphas=9), PR.ERR_ARG), (dict(ld1=23), PR.ERR_ARG), (dict(ld2=3), PR.ERR_ARG), (dict(n1=0), PR.ERR_SHAPE),
                     (dict(n2=0), PR.ERR_SHAPE), (dict(n1=4097, n2=4096), PR.ERR_SHAPE), (dict(d=0), PR.ERR_SHAPE), (dict(d=65, ld1=65, ld2=65), PR.ERR_SHAPE)):
        assert gram(**kw) == code, kw
        assert lib.carel_last_error().startswith(b"carel_rbf_gram")
    s = lib.carel_sample_latents
    assert s(None, p, p, 4, 24, p, None) == PR.ERR_ARG and s(p, None, p, 4, 24, p, None) == PR.ERR_ARG
    assert s(p, p, None, 4, 24, p, None) == PR.ERR_ARG and s(p, p, p, 4, 24, None, None) == PR.ERR_ARG
    assert s(p, p, p, 0, 24, p, None) == PR.ERR_SHAPE and s(p, p, p, 4, 0, p, None) == PR.ERR_SHAPE and s(p, p, p, 4, 33, p, None) == PR.ERR_SHAPE
    assert bytes(buf.raw) == bytes(64)


def test_pval_without_a_gpu_is_refused_not_computed():
    """the drop-in surface has no CPU path: on a machine without a GPU the call raises; with one, a CPU matrix goes to the device"""
    from carel_vae_amd import drl_classifier as M
    K = torch.full((8, 8), 0.5)
    labels = torch.from_numpy(PR.random_labels(4, 4, 5, 1)[1:])
    if not torch.cuda.is_available():
        for call in (lambda: M.MMDStatistic(4, 4).pval(K, 5), lambda: M.permutation_test_mat(K.numpy(), 4, 4, 5, labels=labels),
                     lambda: M.mmd_two_sample_test(torch.zeros(4, 3), torch.ones(4, 3), [0.1], 5)):
            with pytest.raises(L.CarelError):
                call()
    else:
        assert M.MMDStatistic(4, 4).pval(K, 5, labels=labels) == 1.0
    for bad in (lambda: M.permutation_test_mat(K, 1, 7, 5), lambda: M.permutation_test_mat(K, 4, 4, 0)):
        with pytest.raises(L.CarelError):
            bad()
