"""The permutation independence test -- carel_hsic_perm_test and carel_hsic_gram (csrc/hsic_perm.hip), behind hsic_permutation_test /
hsic_independence_test / DrlClassifier.latent_independence_test -- restated in float64: TEST INFRASTRUCTURE for
tests/test_hsic_perm_restate_host.py and tests/test_gpu_hsic_perm_test.py, in the manner of tests/perm_restate.py.  The definition is
the project's own (include/carel_hip.h; the reference has no such function); the statistic is the reference's HSIC.

  (i)   stat_loop: the literal double loop  sum_ij Kc_ij L[pi_i][pi_j] / (m-1)^2  with Kc_ij = K_ij - R_i/m - C_j/m + T/m^2 (small m);
  (ii)  stats_centred: the same, vectorised over row chunks of CHUNK_ROWS rows (m = 8 192 needs no [m, m] float64 temporary), together
        with the magnitude  sum_ij |Kc_ij| |L[pi_i][pi_j]| / (m-1)^2  the bound is made of;
  (iii) stats_expanded: sum K.Lp - (1/m) sum_i R_i RL[pi_i] - (1/m) sum_j C_j CL[pi_j] + T TL / m^2 (Lp = L[pi][:, pi]; RL, CL, TL the
        row sums, column sums and total of L), used ONLY to cross-check (ii): at m = 8 192 it is a small difference of large sums, which
        is why the kernel does not use it.

Bound.  |stats[p] - float64| <= FACTOR * 2^-24 * sum_ij |Kc_ij| |L[pi_i][pi_j]| / (m-1)^2.  The kernels take R, C, T in double, form
Kc_ij in double and round it to float32 ONCE: 1 rounding of |Kc_ij|.  hsic_gather_kernel then accumulates
fma((double)kc, (double)l, acc): the product of two float32 values is exact in double, so there is NO float32 chain (0 roundings).
Everything else -- the m^2 double additions of a statistic (m^2 * 2^-53 <= 2^-27 relative to the magnitude at m = 8 192), the double
errors of R, C, T inside Kc, the division -- is far inside one more unit.  FACTOR = 0 + 1 + 1 = 2 (the two-sample test: 33).

Judge (perm_restate.judge).  Permutation p >= 1 is DECIDED when |stat64_p - stat64_0| > bound_p + bound_0; the device's comparison
must agree with float64 on every decided permutation and its count must lie in [#decided >=, #decided >= + #undecided].
Input condition (asserted on every case by tests/test_hsic_perm_restate_host.py): at most MAX_UNDECIDED of a case's permutations are
undecided, and every exp argument of a Gram matrix lies in [-20, 0].
Nothing here touches the GPU or the library."""
import functools

import numpy as np

from tests import perm_restate as PR
from tests import stats_restate as R

U = 2.0 ** -24
SLAB = 64               # hsic_gather_kernel: rows i per workgroup (HG_SLAB)
GROUP, GROUP_M = 4, 3072    # permutations per workgroup up to m = GROUP_M (HG_M4), one above
COLPART = 64            # rows per column-sum part (HC_ROWS)
THREADS = 256           # the staging loop's stride; the gather loop's is 4 * THREADS columns
FACTOR = 2
MAX_UNDECIDED = 0.05
MAX_M, MAX_P = 8192, 65535
MAX_ARG = 20.0
ERR_ARG, ERR_SHAPE = -1, -2
CHUNK_ROWS = 256

judge = PR.judge


def workspace_bytes(m, P):
    """carel_hsic_perm_workspace_bytes: Kc f32 [m][m4], idx u16 [P+1][m4], then doubles: part [slabs][P+1], R [m], C [m], T, parts [.][m]"""
    if m < 2 or m > MAX_M or P < 1 or P > MAX_P:
        return 0
    m4 = (m + 3) // 4 * 4
    return 4 * m * m4 + 2 * (P + 1) * m4 + 8 * (-(-m // SLAB) * (P + 1) + 2 * m + 1 + -(-m // COLPART) * m)


# ------------------------------------------------------------------------------------------------ the statistic
def sums(K):
    """-> (R [m], C [m], T) of K in float64, by row chunks"""
    m = K.shape[0]
    Rs, Cs = np.empty(m), np.zeros(m)
    for a in range(0, m, CHUNK_ROWS):
        blk = np.asarray(K[a:a + CHUNK_ROWS], np.float64)
        Rs[a:a + CHUNK_ROWS] = blk.sum(1)
        Cs += blk.sum(0)
    return Rs, Cs, float(Rs.sum())


def stat_loop(K, L, perm):
    """(i): the literal loop, one permutation"""
    K, L = np.asarray(K, np.float64), np.asarray(L, np.float64)
    m = K.shape[0]
    Rs = [sum(K[i, j] for j in range(m)) for i in range(m)]
    Cs = [sum(K[i, j] for i in range(m)) for j in range(m)]
    T = sum(Rs)
    s = 0.0
    for i in range(m):
        for j in range(m):
            s += (K[i, j] - Rs[i] / m - Cs[j] / m + T / (m * m)) * L[perm[i], perm[j]]
    return s / ((m - 1) ** 2)


def stats_centred(K, L, perms):
    """(ii) -> (stats, magnitude) float64 [rows of perms]"""
    m = K.shape[0]
    perms = np.asarray(perms, np.int64)
    Rs, Cs, T = sums(K)
    out, mag = np.zeros(perms.shape[0]), np.zeros(perms.shape[0])
    for a in range(0, m, CHUNK_ROWS):
        b = min(a + CHUNK_ROWS, m)
        Kc = np.asarray(K[a:b], np.float64) - Rs[a:b, None] / m - Cs[None, :] / m + T / (m * m)
        aKc = np.abs(Kc)
        Kc, aKc = Kc.ravel(), aKc.ravel()
        for p, pi in enumerate(perms):
            Lp = np.take(L[pi[a:b]], pi, axis=1).astype(np.float64).ravel()
            out[p] += np.dot(Kc, Lp)
            mag[p] += np.dot(aKc, np.abs(Lp, out=Lp))
    den = (m - 1.0) ** 2
    return out / den, mag / den


def stats_expanded(K, L, perms):
    """(iii) -> (stats, the sum of the magnitudes of its four terms) float64 [rows of perms]"""
    m = K.shape[0]
    perms = np.asarray(perms, np.int64)
    Rs, Cs, T = sums(K)
    RL, CL, TL = sums(L)
    t1 = np.zeros(perms.shape[0])
    for a in range(0, m, CHUNK_ROWS):
        Kb = np.asarray(K[a:a + CHUNK_ROWS], np.float64).ravel()
        for p, pi in enumerate(perms):
            t1[p] += np.dot(Kb, np.take(L[pi[a:a + CHUNK_ROWS]], pi, axis=1).astype(np.float64).ravel())
    t2 = np.array([(Rs * RL[pi]).sum() for pi in perms]) / m
    t3 = np.array([(Cs * CL[pi]).sum() for pi in perms]) / m
    t4 = T * TL / (m * m)
    den = (m - 1.0) ** 2
    return (t1 - t2 - t3 + t4) / den, (np.abs(t1) + np.abs(t2) + np.abs(t3) + abs(t4)) / den


def reference(K, L, perms):
    """-> dict(stats, bound, decided [P+1] bool (entry 0 False), ge [P+1] bool, lo, hi): lo / hi = the counts with every undecided
    permutation counted out / in (the layout perm_restate.judge takes)."""
    stats, mag = stats_centred(K, L, perms)
    bound = FACTOR * U * mag
    decided = np.abs(stats - stats[0]) > bound + bound[0]
    decided[0] = False
    ge = stats >= stats[0]
    lo = int((ge & decided)[1:].sum())
    return dict(stats=stats, bound=bound, decided=decided, ge=ge, lo=lo, hi=lo + int((~decided)[1:].sum()))


# ------------------------------------------------------------------------------------------------ the Gram matrix
def gram64(x, s, rows=None):
    """-> (K float64 [rows, m], bound [rows, m]) of carel_hsic_gram on float32 x: exp(-D / s) with the float32 1 / s the kernel
    multiplies by, and the bound the HSIC cases of stats_restate.hsic_closed use for hsic_kern: (d + 2) roundings of the magnitude of
    the argument, |arg| + 2 for __expf."""
    x = np.asarray(x, np.float64)
    a = x if rows is None else x[rows]
    inv = float(np.float32(1.0) / np.float32(s))
    d2, S = R.pair_terms(a, x)
    if rows is None:
        np.fill_diagonal(d2, 0.0)
    else:
        d2[np.arange(len(rows)), rows] = 0.0
    K = np.exp(-d2 * inv)
    return K, U * K * (inv * (x.shape[1] + 2) * S + np.abs(d2 * inv) + 2.0)


def gram32(x, s):
    """float32 [m, m]: the float64 Gram matrix rounded, built by row chunks"""
    m = x.shape[0]
    out = np.empty((m, m), np.float32)
    x64 = np.asarray(x, np.float64)
    n = (x64 * x64).sum(1)
    inv = float(np.float32(1.0) / np.float32(s))
    for a in range(0, m, 1024):
        b = min(a + 1024, m)
        d2 = n[a:b, None] + n[None, :] - 2.0 * (x64[a:b] @ x64.T)
        d2[np.arange(b - a), np.arange(a, b)] = 0.0
        out[a:b] = np.exp(-d2 * inv)
    return out


def max_arg(x, s):
    """the largest |exp argument| of the Gram matrix"""
    x = np.asarray(x, np.float64)
    n = (x * x).sum(1)
    return max(float((n[a:a + 1024, None] + n[None, :] - 2.0 * x[a:a + 1024] @ x.T).max()) for a in range(0, x.shape[0], 1024)) / s


# ------------------------------------------------------------------------------------------------ inputs
def random_perms(m, P, seed):
    """int32 [P+1, m]: the identity, then P uniformly random permutations"""
    rs = np.random.RandomState(seed)
    out = np.empty((P + 1, m), np.int32)
    out[0] = np.arange(m)
    for p in range(1, P + 1):
        out[p] = rs.permutation(m)
    return out


def samples(m, dx, dy, dep, scale, seed):
    """float32 x [m, dx], y [m, dy]: N(0, scale^2) draws; y = dep * (x spread over dy columns) + sqrt(1 - dep^2) * its own noise"""
    rs = np.random.RandomState(seed)
    x = scale * rs.randn(m, dx)
    xs = x[:, np.arange(dy) % dx]
    y = dep * xs + np.sqrt(1.0 - dep * dep) * scale * rs.randn(m, dy)
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y.astype(np.float32))


def _case(name, m, P, dx=24, dy=None, dep=0.15, s=(1.0, 1.0), scale=0.3, **kw):
    dy = dx if dy is None else dy
    return dict(name=name, m=m, P=P, dx=dx, dy=dy, dep=dep, s=s, scale=scale, seed=700 + 7 * m + 3 * P + dx, **kw)


# m: 2, 3 and the edges of the 4-column vector (m mod 4 = 0 .. 3), of a slab of SLAB rows (63, 64, 65; 128 / 129: two slabs / a third),
# of the staging stride (256, 257), of the gather loop's 1024 columns (1024, 1025), of the group regime (GROUP_M, GROUP_M + 1) and the
# row limit; P + 1: 2, 3, the edges of a group of GROUP permutations (4, 5; 64, 65; 129; 1001 = 250 groups and one), of the stats kernel's
# 256 (1001 > 256); d: 1, 24, 64 and d_x != d_y; s: 1, 4 (and 48 at scale 1); dep: 0 (the null), 0.15, 1.
# scale: 0.3, and 0.18 at d = 64 (at 0.3 the off-diagonal of K is 1e-5, K = I, H K H = H and every permutation ties).
# "nonsym": K times (1 + 0.2 u_ij), u uniform, so that K_ij != K_ji.  "tie": m = 2, where H K H = c [[1, -1], [-1, 1]] for every K and the
# swap has the statistic of the identity: a designed tie, outside the input condition.
CASES = [
    _case("m2_p1", 2, 1, explicit=((1, 0),), tie=True), _case("m3_p2", 3, 2, dx=1, explicit=((2, 0, 1), (1, 0, 2))),
    _case("m31_p3", 31, 3, dep=0.0), _case("m32_p4", 32, 4, dx=1, dy=3, dep=1.0), _case("m33_p63", 33, 63, s=(4.0, 1.0)),
    _case("m63_p64", 63, 64, dx=64, dy=24, dep=0.0, scale=0.18), _case("m64_p128", 64, 128, dep=1.0, s=(1.0, 4.0)), _case("m65_p300", 65, 300, dx=8, dy=3),
    _case("m128_p5", 128, 5, dx=64, scale=0.18), _case("m129_p1000", 129, 1000, dep=0.0), _case("m256_p7", 256, 7, dx=3, dy=8, s=(4.0, 4.0)),
    _case("m257_p300", 257, 300), _case("m257_wide_p100", 257, 100, scale=1.0, s=(48.0, 48.0), dep=0.0),
    _case("nonsym_m97_p300", 97, 300, dx=8, nonsym=True),
    _case("m1024_p3", 1024, 3, dx=8), _case("m1025_p8", 1025, 8, dx=8, dy=24, dep=0.0),
    _case("m3072_p4", 3072, 4, dx=8), _case("m3073_p2", 3073, 2, dx=8), _case("m8192_p2", 8192, 2, dx=8),
]
BIG = 2048          # cases above this are built and judged once, by row chunks


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (case, x, y float32 samples, K, L float32 [m, m] built on the host, perms int32 [P+1, m])"""
    c = by_name(name)
    x, y = samples(c["m"], c["dx"], c["dy"], c["dep"], c["scale"], c["seed"])
    K, L = gram32(x, c["s"][0]), gram32(y, c["s"][1])
    if c.get("nonsym"):
        K = (K * (1.0 + 0.2 * np.random.RandomState(c["seed"] + 2).uniform(size=K.shape))).astype(np.float32)
    if c.get("explicit"):
        perms = np.concatenate((np.arange(c["m"], dtype=np.int32)[None], np.asarray(c["explicit"], np.int32)), 0)
    else:
        perms = random_perms(c["m"], c["P"], c["seed"] + 1)
    return c, x, y, K, L, perms


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the float64 reference of the case on its host-built matrices"""
    _, _, _, K, L, perms = case_inputs(name)
    return reference(K, L, perms)


# every refused call of carel_hsic_perm_test: (what is wrong, expected return code); the fields not named are those of a valid call
# with m = 16, P = 4
REFUSALS = [
    (dict(null="k"), ERR_ARG), (dict(null="l"), ERR_ARG), (dict(null="perms"), ERR_ARG), (dict(null="stats"), ERR_ARG),
    (dict(null="count"), ERR_ARG), (dict(null="workspace"), ERR_ARG), (dict(m=1), ERR_SHAPE), (dict(m=8193), ERR_SHAPE),
    (dict(P=0), ERR_SHAPE), (dict(P=65536), ERR_SHAPE), (dict(ldk=15), ERR_ARG), (dict(ldl=15), ERR_ARG),
    (dict(short_workspace=True), ERR_ARG), (dict(misaligned_workspace=True), ERR_ARG),
]
# ... and of carel_hsic_gram; a valid call has m = 16, d = 24, s = 1, ldx = 24, ldk = 16
GRAM_REFUSALS = [
    (dict(x=None), ERR_ARG), (dict(k_out=None), ERR_ARG), (dict(d=0), ERR_SHAPE), (dict(d=65, ldx=65), ERR_SHAPE), (dict(s=0.0), ERR_ARG),
    (dict(s=-1.0), ERR_ARG), (dict(m=1), ERR_SHAPE), (dict(m=8193, ldk=8193), ERR_SHAPE), (dict(ldx=23), ERR_ARG), (dict(ldk=15), ERR_ARG),
]
