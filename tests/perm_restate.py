"""The permutation two-sample test -- carel_mmd_perm_test (csrc/mmd_perm.hip), behind permutation_test_mat / MMDStatistic.pval --
restated twice in float64: TEST INFRASTRUCTURE for tests/test_perm_restate_host.py and tests/test_gpu_perm_test.py, in the manner of
tests/stats_restate.py.  The definition is the project's own (include/carel_hip.h; the reference's function is a stub).

  (i)  stat_loop: the literal loop over i < j of c(g_i, g_j) (M_ij + M_ji), one labelling at a time;
  (ii) three_sums / stats_quadratic: with M' = M without its diagonal, R / C its row / column sums, T its total, q = g^T M' g and
       l = g . (R + C):  S11 = q, S01 = l - 2 q, S00 = T - q - S01, stat = a00 S00 + a11 S11 + a01 S01, for all labellings at once.

Bound.  |stats[p] - stat64_p| <= FACTOR * 2^-24 * (|a00| A00 + |a11| A11 + |a01| A01), A.. = the three sums of |M'| for labelling p.
The kernel forms S_ij = M_ij + M_ji in float32 (1 rounding of |M_ij| + |M_ji|) and sums S_ij over the partners j of one label in
chunks of CHUNK on the exact f32 MFMA: a k-ordered fmaf chain from zero whose weights are 0.0 / 1.0, so every product is exact, the
first addition is exact and a chunk sum carries at most CHUNK - 1 roundings of the magnitude it holds.  Each chunk sum is converted
to double; the sum over a lane's rows, over the chunks, over the two lane halves and over the row tiles (at most n * 16 / CHUNK + 1
+ n / 32 < 4 400 additions at n = 8 192) and the combination with the coefficients are double: below 2^-40 relative, which with the
second-order terms of (1 + 2^-24)^CHUNK (below 2^-39) is far inside one more unit.  Every one of the three sums is a sum of the
chunk sums that belong to it -- none is obtained as a difference -- so FACTOR = (CHUNK - 1) + 1 + 1 = CHUNK + 1 = 33.

Judge.  Labelling p >= 1 is DECIDED when |stat64_p - stat64_0| > bound_p + bound_0: then every pair of values inside the two bounds
compares like the float64 pair.  The device's stats must lie inside the bound everywhere, its comparison must agree with float64 on
every decided labelling, and its count must be the count of its own comparisons.
Input condition (asserted on every case by tests/test_perm_restate_host.py): at most MAX_UNDECIDED of a case's labellings are
undecided; at least three cases have a count between 0.1 P and 0.9 P.
Nothing here touches the GPU or the library."""
import functools

import numpy as np

from tests import stats_restate as R

U = 2.0 ** -24
ROWS, LABS, CHUNK = 32, 32, 32          # perm_tile_kernel: rows per workgroup, labellings per wave (128 per workgroup), partners per f32 chain
LABS_WG = 128
FACTOR = CHUNK + 1
MAX_UNDECIDED = 0.05
MAX_N, MAX_P = 8192, 65535
ERR_ARG, ERR_SHAPE = -1, -2


def workspace_bytes(n, P):
    """carel_mmd_perm_workspace_bytes: three doubles and one 32-bit label word per row tile and labelling, a multiple of 8 bytes"""
    if n < 4 or n > MAX_N or P < 1 or P > MAX_P:
        return 0
    cells = -(-n // ROWS) * (P + 1)
    return 8 * (3 * cells + (cells + 1) // 2)


def mmd_coefficients(n1, n2):
    """(a00, a01, a11) of MMDStatistic(n1, n2)"""
    return 1.0 / (n1 * (n1 - 1)), -1.0 / (n1 * n2), 1.0 / (n2 * (n2 - 1))


# ------------------------------------------------------------------------------------------------ (i) the literal loop
def stat_loop(M, g, coef):
    a00, a01, a11 = coef
    M = np.asarray(M, np.float64)
    n = M.shape[0]
    s = 0.0
    for i in range(n):
        for j in range(i + 1, n):
            c = a01 if g[i] != g[j] else (a11 if g[i] else a00)
            s += c * (M[i, j] + M[j, i])
    return s


# ------------------------------------------------------------------------------------------------ (ii) the quadratic form
def three_sums(M, labels):
    """-> (S00, S11, S01), float64 [rows of labels] each, of the off-diagonal part of M"""
    Mz = np.array(M, np.float64)
    np.fill_diagonal(Mz, 0.0)
    G = (np.asarray(labels) != 0).astype(np.float64)
    rc = Mz.sum(1) + Mz.sum(0)
    q = ((G @ Mz) * G).sum(1)
    l = G @ rc
    S01 = l - 2.0 * q
    return Mz.sum() - q - S01, q, S01


def stats_quadratic(M, labels, coef):
    a00, a01, a11 = coef
    S00, S11, S01 = three_sums(M, labels)
    return a00 * S00 + a11 * S11 + a01 * S01


def stats_bound(M, labels, coef):
    a00, a01, a11 = coef
    A00, A11, A01 = three_sums(np.abs(np.asarray(M, np.float64)), labels)
    return FACTOR * U * (abs(a00) * A00 + abs(a11) * A11 + abs(a01) * A01)


def reference(M, labels, coef):
    """-> dict(stats, bound, decided [P+1] bool (entry 0 False), ge [P+1] bool, lo, hi): lo / hi = the counts with every undecided
    labelling counted out / in."""
    stats = stats_quadratic(M, labels, coef)
    bound = stats_bound(M, labels, coef)
    decided = np.abs(stats - stats[0]) > bound + bound[0]
    decided[0] = False
    ge = stats >= stats[0]
    lo = int((ge & decided)[1:].sum())
    return dict(stats=stats, bound=bound, decided=decided, ge=ge, lo=lo, hi=lo + int((~decided)[1:].sum()))


def judge(got_stats, got_count, ref):
    """-> the worst |error| / bound; asserts the comparisons and the count"""
    got_stats = np.asarray(got_stats, np.float64)
    assert np.isfinite(got_stats).all()
    fr = R.frac(got_stats, ref["stats"], ref["bound"])
    own = got_stats >= got_stats[0]
    d = ref["decided"]
    assert np.array_equal(own[d], ref["ge"][d]), "the device's comparison differs from float64 on a decided labelling"
    assert int(got_count) == int(own[1:].sum()), (int(got_count), int(own[1:].sum()))
    assert ref["lo"] <= int(got_count) <= ref["hi"]
    assert fr <= 1.0, fr
    return fr


# ------------------------------------------------------------------------------------------------ inputs
def observed(n1, n2):
    return np.concatenate((np.zeros(n1, np.uint8), np.ones(n2, np.uint8)))


def random_labels(n1, n2, P, seed):
    """uint8 [P+1, n]: the observed labelling, then P uniformly random ones with n2 ones each"""
    rs = np.random.RandomState(seed)
    out = np.empty((P + 1, n1 + n2), np.uint8)
    out[0] = observed(n1, n2)
    for p in range(1, P + 1):
        out[p] = out[0][rs.permutation(n1 + n2)]
    return out


def rbf_matrix(z, alphas, eps=1e-5):
    """float32 [n, n]: the float64 kernel matrix of the rows of z, rounded"""
    d2, _ = R.pair_terms(np.asarray(z, np.float64))
    ad = eps + np.abs(d2)
    return sum(np.exp(-a * ad) for a in R.f32_scalars(alphas)).astype(np.float32)


def _case(name, n1, n2, P, d=24, alphas=R.A1, kind="rbf", **kw):
    return dict(name=name, n1=n1, n2=n2, P=P, d=d, alphas=alphas, kind=kind, eps=1e-5, seed=500 + 7 * n1 + n2 + 3 * P, **kw)


# n: the edges of the 32-row tile and of the chunk (CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1), several row tiles; P + 1: the edges of a
# wave's 32 labellings and of a workgroup's 128; unequal sides, n1 = 2.  kind "rbf": N(0, 1) samples, both sides alike (the null);
# "nonsym": the same matrix times (1 + 0.2 u_ij), u uniform, so that M_ij != M_ji; "gram": the samples of stats_restate.mmd_inputs
# (equal sides), whose matrix the GPU test takes from carel_rbf_gram.
CASES = [
    _case("n4_p1", 2, 2, 1, explicit=((0, 1, 0, 1),)),
    _case("n31_p31", 15, 16, 31), _case("n32_p32", 16, 16, 32), _case("n33_p64_n1_2", 2, 31, 64),
    _case("n64_p127", 32, 32, 127), _case("n65_p128", 40, 25, 128), _case("n129_p1000", 64, 65, 1000),
    _case("n257_p200", 150, 107, 200), _case("n384_p1000", 192, 192, 1000), _case("n384_unequal_p1000", 150, 234, 1000),
    _case("nonsym_n97_p300", 50, 47, 300, kind="nonsym"),
    _case("gram_a1_n131", 70, 61, 100, kind="gram"), _case("gram_a3_n73_d7", 33, 40, 100, d=7, alphas=R.A3, kind="gram"),
    _case("gram_a8_n128_d64", 64, 64, 100, d=64, alphas=R.A8, kind="gram"),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def case_samples(c):
    """float32 (s1, s2)"""
    if c["kind"] == "gram":
        return R.mmd_inputs(dict(c, equal=True))
    z = np.random.RandomState(c["seed"]).randn(c["n1"] + c["n2"], c["d"]).astype(np.float32)
    return np.ascontiguousarray(z[:c["n1"]]), np.ascontiguousarray(z[c["n1"]:])


def case_labels(c):
    if c.get("explicit"):
        return np.concatenate((observed(c["n1"], c["n2"])[None], np.asarray(c["explicit"], np.uint8)), 0)
    return random_labels(c["n1"], c["n2"], c["P"], c["seed"] + 1)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (case, s1, s2, M float32 [n, n] built on the host, labels uint8 [P+1, n], (a00, a01, a11))"""
    c = by_name(name)
    s1, s2 = case_samples(c)
    M = rbf_matrix(np.concatenate((s1, s2), 0), c["alphas"], c["eps"])
    if c["kind"] == "nonsym":
        M = (M * (1.0 + 0.2 * np.random.RandomState(c["seed"] + 2).uniform(size=M.shape))).astype(np.float32)
    return c, s1, s2, M, case_labels(c), mmd_coefficients(c["n1"], c["n2"])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the float64 reference of the case on its host-built matrix"""
    c, _, _, M, labels, coef = case_inputs(name)
    return reference(M, labels, coef)


# every refused call: (what is wrong, expected return code); the fields not named are those of a valid call with n1 = n2 = 8, P = 4
REFUSALS = [
    (dict(null="matrix"), ERR_ARG), (dict(null="labels"), ERR_ARG), (dict(null="stats"), ERR_ARG), (dict(null="count"), ERR_ARG),
    (dict(null="workspace"), ERR_ARG), (dict(n1=1), ERR_SHAPE), (dict(n2=1), ERR_SHAPE), (dict(n1=4097, n2=4096), ERR_SHAPE),
    (dict(P=0), ERR_SHAPE), (dict(P=65536), ERR_SHAPE), (dict(short_workspace=True), ERR_ARG), (dict(ldm=15), ERR_ARG),
]
