"""carel_pdist_select (csrc/pdist_select.hip) -- the exact order statistics of the squared pairwise distances of one sample, behind
ops.pdist_select / pdist_quantile / median_heuristic and the "median" widths of the two permutation tests -- restated in float64: TEST
INFRASTRUCTURE for tests/test_pdist_select_host.py and tests/test_gpu_pdist_select.py, in the manner of tests/hsic_perm_restate.py.
The definition is the project's own (include/carel_hip.h; the reference has no such function).

  select64: D64 = |xi|^2 + |xj|^2 - 2 xi.xj of stats_restate.pair_terms on the float32 sample, the upper triangle i < j, np.partition
            at the ranks; `below` / `equal` by comparison.
  select32: the same selection on a float32 numpy evaluation (norms and products summed by numpy in float32): the honesty condition.
  exact_expected: for integer-valued samples with entries in [-8, 8] every norm and dot product is an integer below 2^24, float32 is
            exact, D32 == D64, and (value, below, equal) of a rank come from np.bincount cumulatives -- by row chunks, so that m = 8 192
            is judged without 33.5 M doubles.

Bound.  If every element of a multiset moves by at most e, every order statistic moves by at most e (the r-th smallest of the moved
set lies between the r-th smallest minus e and plus e).  The device's D_ij is the argument of hsic_kern, for which
tests/hsic_perm_restate.gram64 (and stats_restate.hsic_closed) use (d + 2) roundings of the magnitude S_ij = |xi|^2 + |xj|^2 +
2 sum_k |xik xjk| that pair_terms returns; hence  |v_r - v64_r| <= max_{i<j} (d + 2) * 2^-24 * S_ij.  No new constant.
Honesty condition (tests/test_pdist_select_host.py, every float case): select32 stays within HALF that bound of select64.
Nothing here touches the GPU or the library."""
import functools

import numpy as np

from tests import stats_restate as R

U = 2.0 ** -24
TILE = 64               # ps_sweep_kernel: rows and columns of a tile (ST_TILE of stat_tile_device.h)
MAX_M, MAX_D, MAX_RANKS = 8192, 64, 8
STATE_BYTES, BINS = 256, (2048, 2048, 1024)
ERR_ARG, ERR_SHAPE = -1, -2
CHUNK_ROWS = 1024


def workspace_bytes(m, n_ranks):
    """carel_pdist_select_workspace_bytes: the state, then u32 histograms [2048], [n_ranks][2048], [n_ranks][1024]"""
    if m < 2 or m > MAX_M or n_ranks < 1 or n_ranks > MAX_RANKS:
        return 0
    return STATE_BYTES + 4 * (BINS[0] + n_ranks * (BINS[1] + BINS[2]))


def n_pairs(m):
    return m * (m - 1) // 2


def ranks_of(m, which):
    """"edges": rank 0, N - 1 and the two median ranks; "eight": eight ranks at once, duplicates included"""
    N = n_pairs(m)
    edges = [0, N - 1, (N - 1) // 2, N // 2]
    return edges if which == "edges" else edges + [N // 2, N // 4, 0, (3 * N) // 4]


# ------------------------------------------------------------------------------------------------ the selection
def upper64(x):
    """-> (D64 [N], S [N]) of the pairs i < j of float32 x, row-major"""
    d2, S = R.pair_terms(np.asarray(x, np.float64))
    iu = np.triu_indices(x.shape[0], 1)
    return d2[iu], S[iu]


def bound_of(x):
    return float((x.shape[1] + 2) * U * upper64(x)[1].max())


def _select(D, ranks):
    ranks = np.asarray(ranks, np.int64)
    v = np.partition(D, np.unique(ranks))[ranks]
    below = np.array([(D < a).sum() for a in v], np.int64)
    equal = np.array([(D == a).sum() for a in v], np.int64)
    return v, below, equal


def select64(x, ranks):
    """-> (values float64 [n], below int64 [n], equal int64 [n])"""
    return _select(upper64(x)[0], ranks)


def upper32(x):
    """the float32 numpy evaluation: n_i + n_j - 2 (x x^T)_ij, every operation in float32"""
    x = np.asarray(x, np.float32)
    n = (x * x).sum(1, dtype=np.float32)
    D = (n[:, None] + n[None, :]) - np.float32(2.0) * (x @ x.T)
    assert D.dtype == np.float32
    return D[np.triu_indices(x.shape[0], 1)]


def select32(x, ranks):
    return _select(upper32(x), ranks)[0]


def quantile64(x, q):
    """numpy's default ("linear") quantile of D64 over i < j"""
    return float(np.quantile(upper64(x)[0], q))


def exact_hist(x):
    """-> counts int64 [max D + 1] of { D_ij : i < j } for an integer-valued sample: D is a non-negative integer"""
    xi = np.asarray(x, np.float64)
    assert np.array_equal(xi, np.rint(xi)) and np.abs(xi).max() <= 8
    m, d = xi.shape
    n = (xi * xi).sum(1)
    full = np.zeros(4 * 64 * d + 1, np.int64)
    for a in range(0, m, CHUNK_ROWS):
        D = n[a:a + CHUNK_ROWS, None] + n[None, :] - 2.0 * (xi[a:a + CHUNK_ROWS] @ xi.T)
        full += np.bincount(D.astype(np.int64).ravel(), minlength=full.size)
    full[0] -= m                                     # the diagonal
    assert (full % 2 == 0).all()
    return full // 2


def exact_expected(x, ranks):
    """-> (values, below, equal) from the bincount cumulatives"""
    h = exact_hist(x)
    cum = np.cumsum(h)
    assert cum[-1] == n_pairs(x.shape[0])
    ranks = np.asarray(ranks, np.int64)
    v = np.searchsorted(cum, ranks, side="right")
    return v.astype(np.float64), (cum[v] - h[v]).astype(np.int64), h[v].astype(np.int64)


# ------------------------------------------------------------------------------------------------ inputs
def _case(name, m, d, kind="float", pad=0, ranks="edges", scale=1.0):
    return dict(name=name, m=m, d=d, kind=kind, pad=pad, ranks=ranks, scale=scale, seed=900 + 11 * m + d)


# m: 2, 3 (one tile, N = 1 and 3), the edges of a 64-row tile (63, 64, 65: a diagonal-only grid, then three tiles), 128 / 129 and 1000
# (136 tiles, the last one partial); m = 8192 once, exact only.  d: 1, 24, 63, 64 (row strides 1, 25, 63, 65 in LDS).  pad: ldx = d + pad.
# kinds: "float" N(0, scale^2); "exact" integers in [-8, 8]; "dup" 65 rows drawn from 20 distinct ones (ties at exactly +0);
# "offset" rows 100 + 1e-3 N(0, 1): true distances 5e-5 under roundings of 0.03, so that some D_ij come out negative.
CASES = [
    _case("f_m2_d24", 2, 24), _case("f_m3_d1", 3, 1, pad=2), _case("f_m63_d64", 63, 64, ranks="eight"), _case("f_m64_d24", 64, 24, pad=7),
    _case("f_m65_d63", 65, 63, scale=8.0), _case("f_m128_d1", 128, 1, ranks="eight"), _case("f_m129_d24", 129, 24, pad=1, ranks="eight", scale=0.3),
    _case("f_m1000_d24", 1000, 24, scale=8.0),
    _case("e_m2_d1", 2, 1, "exact"), _case("e_m3_d24", 3, 24, "exact", ranks="eight"), _case("e_m64_d64", 64, 64, "exact", pad=3),
    _case("e_m65_d1", 65, 1, "exact", ranks="eight"), _case("e_m129_d63", 129, 63, "exact"), _case("e_m1000_d24", 1000, 24, "exact", ranks="eight"),
    _case("e_m8192_d24", 8192, 24, "exact"),
    _case("dup_m65_d24", 65, 24, "dup", ranks="eight"), _case("offset_m129_d24", 129, 24, "offset", pad=4),
]
BIG = 2048          # above this only the exact restatement is used


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (case, x float32 [m, d], ranks list)"""
    c = by_name(name)
    rs = np.random.RandomState(c["seed"])
    m, d = c["m"], c["d"]
    if c["kind"] == "exact":
        x = rs.randint(-8, 9, size=(m, d)).astype(np.float32)
    elif c["kind"] == "dup":
        x = (c["scale"] * rs.randn(20, d)).astype(np.float32)[rs.randint(0, 20, size=m)]
    elif c["kind"] == "offset":
        x = (100.0 + 1e-3 * rs.randn(m, d)).astype(np.float32)
    else:
        x = (c["scale"] * rs.randn(m, d)).astype(np.float32)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return c, x, ranks_of(m, c["ranks"])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """-> dict(values, below, equal, bound): exact cases from the bincount (bound 0), the others from select64"""
    c, x, ranks = case_inputs(name)
    if c["kind"] == "exact":
        v, b, e = exact_expected(x, ranks)
        return dict(values=v, below=b, equal=e, bound=0.0)
    v, b, e = select64(x, ranks)
    return dict(values=v, below=b, equal=e, bound=bound_of(x))


def coinciding_pairs(x):
    """the number of pairs i < j of bitwise equal rows"""
    _, cnt = np.unique(np.asarray(x), axis=0, return_counts=True)
    return int((cnt * (cnt - 1) // 2).sum())


# the case that pins the reason for the feature: a strongly dependent sample whose distances are in the thousands
POWER = dict(m=200, d=24, P=200, seed=4242)


@functools.lru_cache(maxsize=None)
def power_inputs():
    """-> (x, y float32 [200, 24], perms int32 [P + 1, m]): x = 8 N(0, 1), y a noisy copy of x"""
    from tests import hsic_perm_restate as HR
    rs = np.random.RandomState(POWER["seed"])
    x = (8.0 * rs.randn(POWER["m"], POWER["d"])).astype(np.float32)
    y = (x + 2.0 * rs.randn(POWER["m"], POWER["d"])).astype(np.float32)
    return x, y, HR.random_perms(POWER["m"], POWER["P"], POWER["seed"] + 1)


# every refused call of carel_pdist_select: (what is wrong, expected return code); the fields not named are those of a valid call with
# m = 16, d = 24, ldx = 24, ranks (0, 119)
REFUSALS = [
    (dict(null="x"), ERR_ARG), (dict(null="values"), ERR_ARG), (dict(null="workspace"), ERR_ARG), (dict(m=1), ERR_SHAPE),
    (dict(m=8193), ERR_SHAPE), (dict(d=0), ERR_SHAPE), (dict(d=65, ldx=65), ERR_SHAPE), (dict(ldx=23), ERR_ARG), (dict(n_ranks=0), ERR_SHAPE),
    (dict(n_ranks=9), ERR_SHAPE), (dict(rank=-1), ERR_ARG), (dict(rank=120), ERR_ARG), (dict(short_workspace=True), ERR_ARG),
    (dict(misaligned_workspace=True), ERR_ARG),
]
