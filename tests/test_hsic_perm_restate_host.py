"""The float64 restatements of the permutation independence test (tests/hsic_perm_restate.py) agree with each other, every committed
case meets the input condition (at most 5 % of its permutations undecided against the bound, every exp argument in [-20, 0]), the case
list holds the edges it names, and the host side of the new entry points: ABI 9 unchanged, the symbols declared, bound and exported,
the structs laid out as the header says, the workspace size, and every refusal of carel_hsic_perm_test / carel_hsic_gram before a
launch (they need no GPU).  random_permutations with a CPU generator.  No GPU is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from tests import hsic_perm_restate as HR
from tests import stats_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("carel_hsic_gram", "carel_hsic_perm_workspace_bytes", "carel_hsic_perm_test")


@pytest.fixture(scope="module")
def lib():
    from carel_vae_amd import build
    build.build(verbose=False)
    return L.load()


def test_the_literal_loop_and_the_vectorised_form_agree():
    rs = np.random.RandomState(3)
    for m in (2, 3, 7, 18):
        K = rs.uniform(0.1, 1.0, size=(m, m)).astype(np.float32)          # not symmetric, an arbitrary diagonal
        Lm = rs.uniform(0.1, 1.0, size=(m, m)).astype(np.float32)
        perms = HR.random_perms(m, 6, 10 + m)
        vec, mag = HR.stats_centred(K, Lm, perms)
        for p in range(perms.shape[0]):
            assert abs(HR.stat_loop(K, Lm, perms[p]) - vec[p]) <= 1e-13 * mag[p]
        assert (mag >= np.abs(vec)).all()
    # the identity on the Gram matrices of x and y is the HSIC statistic
    c, x, y, _, ref, _ = R.hsic_reference("h_65")
    got = HR.stats_centred(HR.gram64(x, c["s"][0])[0], HR.gram64(y, c["s"][1])[0], np.arange(65)[None])[0][0]
    assert abs(got - ref["hsic"]) <= 1e-12 * sum(ref["terms"])
    # ... and the Gram restatement is the kernel matrix of that closed form, bound included
    K, b = HR.gram64(x, c["s"][0])
    K2, b2 = HR.gram64(x, c["s"][0], np.arange(10, 20))
    assert np.array_equal(K[10:20], K2) and np.array_equal(b[10:20], b2) and (np.diag(K) == 1.0).all()
    assert np.abs(HR.gram32(x, c["s"][0]) - K).max() <= HR.U


@pytest.mark.parametrize("name", [c["name"] for c in HR.CASES])
def test_case_meets_the_input_condition_and_the_restatements_agree(name):
    c, x, y, K, Lm, perms = HR.case_inputs(name)
    m, P = c["m"], c["P"]
    assert x.shape == (m, c["dx"]) and y.shape == (m, c["dy"]) and x.dtype == y.dtype == np.float32
    assert K.shape == Lm.shape == (m, m) and K.dtype == Lm.dtype == np.float32 and perms.shape == (P + 1, m) and perms.dtype == np.int32
    assert np.array_equal(perms[0], np.arange(m)) and np.array_equal(np.sort(perms, 1), np.broadcast_to(np.arange(m), perms.shape))
    assert HR.max_arg(x, c["s"][0]) <= HR.MAX_ARG and HR.max_arg(y, c["s"][1]) <= HR.MAX_ARG
    if c.get("nonsym"):
        assert np.abs(K - K.T).max() > 0.01 * np.abs(K).max()
    ref = HR.case_reference(name)
    exp, exp_mag = HR.stats_expanded(K, Lm, perms)
    worst = float(np.abs(exp - ref["stats"]).max() / exp_mag.max())
    undecided = int((~ref["decided"])[1:].sum())
    print("CASE %s undecided %d / %d count %d..%d expanded - centred %.1e of the expansion's terms" % (name, undecided, P, ref["lo"], ref["hi"], worst))
    assert worst <= 1e-13                                    # (the expansion's own cancellation, in float64)
    assert (ref["bound"] > 0).all() and ref["bound"].max() < 1e-5 * np.abs(ref["stats"]).max() + 1e-9
    if c.get("tie"):
        assert m == 2 and undecided == P
    else:
        assert undecided <= HR.MAX_UNDECIDED * P


def test_three_cases_have_a_count_away_from_the_ends():
    mid = [c["name"] for c in HR.CASES if 0.1 * c["P"] <= HR.case_reference(c["name"])["lo"]
           and HR.case_reference(c["name"])["hi"] <= 0.9 * c["P"]]
    assert len(mid) >= 3, mid


def test_case_list_covers_the_edges():
    ms = {c["m"] for c in HR.CASES}
    assert {2, 3, 31, 32, 33, 63, 64, 65, 129, 257, 1025} <= ms
    assert {HR.SLAB - 1, HR.SLAB, HR.SLAB + 1, 2 * HR.SLAB, 2 * HR.SLAB + 1, HR.THREADS, HR.THREADS + 1, 4 * HR.THREADS, 4 * HR.THREADS + 1,
            HR.GROUP_M, HR.GROUP_M + 1, HR.MAX_M} <= ms and {m % 4 for m in ms} == {0, 1, 2, 3}
    np1 = {c["P"] + 1 for c in HR.CASES}
    assert {2, 3, 64, 65, 129, 1001, HR.GROUP, HR.GROUP + 1} <= np1
    assert any(c["m"] == HR.MAX_M and c["P"] == 2 for c in HR.CASES)
    assert {1, 24, 64} <= {c["dx"] for c in HR.CASES} and any(c["dx"] != c["dy"] for c in HR.CASES)
    assert {1.0, 4.0} <= {s for c in HR.CASES for s in c["s"]} and any(c.get("nonsym") for c in HR.CASES)
    assert {0.0, 0.15, 1.0} <= {c["dep"] for c in HR.CASES}


def test_abi_and_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "carel_hip.h")).read()
    assert "#define CAREL_ABI_VERSION 9" in hdr and L.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    assert hdr.count("parity unpinned") >= 2
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name), name
    import carel_vae_amd as pkg
    for name in ("hsic_permutation_test", "hsic_independence_test", "random_permutations"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert callable(pkg.DrlClassifier.latent_independence_test) and callable(pkg.drl_classifier_en.DrlClassifier.latent_independence_test)
    from carel_vae_amd import ops
    assert callable(ops.hsic_gram) and callable(ops.hsic_perm_test)


def _header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), open(os.path.join(ROOT, "include", "carel_hip.h")).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:                                         # "type a, b": the first name follows the type, the others stand alone
            parts = decl.split(",")
            names += [parts[0].split()[-1].lstrip("*")] + [x.strip().lstrip("*") for x in parts[1:]]
    return names


def test_struct_layouts_match_the_header():
    T = L.HsicPermArgs
    want = dict(k=0, ldk=8, l=16, ldl=24, perms=32, m=40, n_permutations=44, stats=48, count=56, workspace=64, workspace_bytes=72)
    assert {f[0]: getattr(T, f[0]).offset for f in T._fields_} == want and C.sizeof(T) == 80
    assert _header_fields("carel_hsic_perm_args") == list(want)
    G = L.HsicGramArgs
    want = dict(x=0, ldx=8, m=16, d=20, s=24, k_out=32, ldk=40)
    assert {f[0]: getattr(G, f[0]).offset for f in G._fields_} == want and C.sizeof(G) == 48
    assert _header_fields("carel_hsic_gram_args") == list(want)


def test_workspace_size(lib):
    f = lib.carel_hsic_perm_workspace_bytes
    for c in HR.CASES:
        assert f(c["m"], c["P"]) == HR.workspace_bytes(c["m"], c["P"]) > 0 and f(c["m"], c["P"]) % 8 == 0
    for m, P in ((2, 1), (1938, 1000), (8192, 65535)):
        assert f(m, P) == HR.workspace_bytes(m, P) > 0
    for m, P in ((1, 10), (8193, 10), (100, 0), (100, 65536), (-5, 10)):
        assert f(m, P) == 0 == HR.workspace_bytes(m, P)


def _valid_args(keep, m=16, P=4):
    """a call that would be accepted; the pointers are host buffers that a refused call never touches"""
    bufs = {k: C.create_string_buffer(80) for k in ("k", "l", "perms", "stats", "count", "workspace")}
    keep.append(bufs)
    a = L.HsicPermArgs()
    for k, b in bufs.items():
        setattr(a, k, (C.addressof(b) + 15) & ~15)
    a.ldk, a.ldl, a.m, a.n_permutations = m, m, m, P
    a.workspace_bytes = max(HR.workspace_bytes(m, P), 64)
    return a, bufs


@pytest.mark.parametrize("what,code", HR.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in HR.REFUSALS])
def test_perm_test_refusals_need_no_gpu(lib, what, code):
    keep = []
    a, bufs = _valid_args(keep, m=what.get("m", 16), P=what.get("P", 4))
    if "null" in what:
        setattr(a, what["null"], None)
    if what.get("short_workspace"):
        a.workspace_bytes = HR.workspace_bytes(16, 4) - 1
    if what.get("misaligned_workspace"):
        a.workspace += 8
    for k in ("ldk", "ldl"):
        if k in what:
            setattr(a, k, what[k])
    before = {k: bytes(b.raw) for k, b in bufs.items()}
    assert lib.carel_hsic_perm_test(C.byref(a), None) == code
    assert lib.carel_last_error().startswith(b"carel_hsic_perm_test")
    assert {k: bytes(b.raw) for k, b in bufs.items()} == before
    assert lib.carel_hsic_perm_test(None, None) == HR.ERR_ARG and lib.carel_last_error().startswith(b"carel_hsic_perm_test")


@pytest.mark.parametrize("what,code", HR.GRAM_REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in HR.GRAM_REFUSALS])
def test_gram_refusals_need_no_gpu(lib, what, code):
    buf = C.create_string_buffer(64)
    a = L.HsicGramArgs()
    a.x, a.k_out, a.ldx, a.m, a.d, a.s, a.ldk = C.addressof(buf), C.addressof(buf), 24, 16, 24, 1.0, 16
    for k, v in what.items():
        setattr(a, k, v)
    assert lib.carel_hsic_gram(C.byref(a), None) == code
    assert lib.carel_last_error().startswith(b"carel_hsic_gram")
    assert bytes(buf.raw) == bytes(64)
    assert lib.carel_hsic_gram(None, None) == HR.ERR_ARG


def test_random_permutations_with_a_cpu_generator():
    from carel_vae_amd import random_permutations
    a = random_permutations(37, 50, "cpu", torch.Generator().manual_seed(5))
    b = random_permutations(37, 50, "cpu", torch.Generator().manual_seed(5))
    c = random_permutations(37, 50, "cpu", torch.Generator().manual_seed(6))
    assert a.dtype == torch.int32 and tuple(a.shape) == (51, 37) and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a[0], torch.arange(37, dtype=torch.int32))
    assert torch.equal(torch.sort(a, dim=1).values, torch.arange(37, dtype=torch.int32).expand(51, 37))
    assert len({tuple(r.tolist()) for r in a[1:]}) == 50


def test_without_a_gpu_the_tests_are_refused_not_computed():
    """no CPU path: on a machine without a GPU the calls raise; bad shapes raise everywhere"""
    from carel_vae_amd import drl_classifier as M
    K = torch.full((8, 8), 0.5)
    if not torch.cuda.is_available():
        for call in (lambda: M.hsic_permutation_test(K, K, 5), lambda: M.hsic_independence_test(torch.zeros(8, 3), torch.ones(8, 2), n_permutations=5)):
            with pytest.raises(L.CarelError):
                call()
    else:
        assert M.hsic_permutation_test(K, K.numpy(), 5) == 1.0                 # a constant L: every permutation ties
        for bad in (lambda: M.hsic_permutation_test(K, K[:7, :7], 5), lambda: M.hsic_permutation_test(K, K, 0),
                    lambda: M.hsic_permutation_test(K[:1, :1], K[:1, :1], 5)):
            with pytest.raises(L.CarelError):
                bad()
