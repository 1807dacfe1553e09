"""The tiled differentiable statistics -- carel_hsic_tiled_fwd/bwd, carel_rbf_mmd_tiled_fwd/bwd (csrc/stat_tiled.hip, stat_tiled_device.h)
-- restated: TEST INFRASTRUCTURE for tests/test_stat_tiled_host.py and tests/test_gpu_stat_tiled.py.  The float64 references, the
bounds' form and the input builders are those of tests/stats_restate.py (hsic_closed, mmd_closed, hsic_inputs, mmd_inputs); what is
restated here is the tile plan the host code picks and the chain lengths that follow from it.

The plan (stat_tiled.hip: st_split, the workspace functions).  T = ceil(rows / 64) tiles a side; the gradient sweeps cut the T partner
tiles of a row tile into S runs of `per` tiles: want = min(T, max(1, 1024 // T)), per = ceil(T / want), S = ceil(T / per).

Chains (the L of the bounds: the sequential float additions a term passes through).  A masked pair or an absent run enters a sum as an
exact 0, so no sum of r terms has a term pass through more than r additions, whatever the plan says.
  sums          a thread adds 16 kernel values in turn, the four threads of a row by a two-level butterfly; everything after that is
                double, rounded to float once: SUM_CHAIN = 16 + 2 + 1.  This covers the row sums RK_i, RL_i, sum K.L and the three MMD
                block sums; TK, TL and sum RK.RL are double sums of floats and exact products, rounded once (TOTAL_CHAIN = 1).
  gradients     a thread adds the partners of its run in turn, 64 * per of them, then the S runs are added in turn:
                grad_chain(rows) = min(rows, 64 * per + S - 1).
HSIC: SUM_CHAIN <= 19 and grad_chain(m) <= m = chain_hsic_row(m) for every m >= 2 (min(m, .) for m < 19; 64 + T - 1 <= m from T = 2 on),
and TOTAL_CHAIN <= chain_block(m): the bounds of stats_restate.hsic_closed, which count the single-workgroup chains, hold for the
tiled kernels AS THEY ARE, and the tests use them unchanged.  MMD value: SUM_CHAIN <= 24 <= chain_mmd_fwd(n): unchanged too.
MMD gradient: the single-workgroup backward splits a row's partners over 8 or 2 lanes for n <= 512, so its chain (19 at n = 128) is
SHORTER than the tiled one (65): the one bound that has to be restated.  mmd_closed_tiled is mmd_closed with chain_mmd_bwd replaced by
grad_chain, nothing else; where grad_chain is the shorter one (n > 1024: 88 against 1572 at the LDS limit) the restated bound is the
tighter one, and it is used there all the same.
Nothing here touches the library; hsic_rows_closed alone can be told to do its float64 arithmetic on the GPU (the m = 8192 case)."""
import functools

import numpy as np

from tests import stats_restate as R

TILE = 64
MAX_ROWS = 8192
SUM_CHAIN = 16 + 2 + 1
TOTAL_CHAIN = 1


def tiles(rows):
    return -(-rows // TILE)


def split(T):
    """-> (per, S): partner tiles per gradient workgroup and the number of such runs"""
    want = min(T, max(1, 1024 // T))
    per = -(-T // want)
    return per, -(-T // per)


def grad_chain(rows):
    per, S = split(tiles(rows))
    return min(rows, TILE * per + S - 1)


def hsic_workspace_bytes(m, d):
    if not (2 <= m <= MAX_ROWS and 1 <= d <= 64):
        return 0
    T = tiles(m)
    _, S = split(T)
    return 8 * (T * T + 3 * -(-m // 256)) + 4 * (4 + 2 * TILE * T + 2 * T * TILE * T + 2 * S * m * d)


def mmd_workspace_bytes(n1, n2, d):
    if not (n1 >= 2 and n2 >= 2 and n1 + n2 <= MAX_ROWS and 1 <= d <= 64):
        return 0
    T = tiles(n1 + n2)
    _, S = split(T)
    return 8 * 3 * T * T + 4 * S * (n1 + n2) * d


def mmd_closed_tiled(s1, s2, alphas, eps, gs):
    """stats_restate.mmd_closed with the gradient chain of the tiled plan in the place of chain_mmd_bwd; the value's bound keeps
    chain_mmd_fwd (SUM_CHAIN is the shorter one for every n)."""
    n = len(s1) + len(s2)
    assert SUM_CHAIN <= R.chain_mmd_fwd(n)
    keep = R.chain_mmd_bwd
    R.chain_mmd_bwd = grad_chain
    try:
        return R.mmd_closed(s1, s2, alphas, eps, gs)
    finally:
        R.chain_mmd_bwd = keep


def hsic_closed_tiled(x, y, s_x, s_y, gs):
    """stats_restate.hsic_closed as it is: every tiled chain is at most the single-workgroup one it stands for (asserted here)."""
    m = len(x)
    assert min(m, SUM_CHAIN) <= R.chain_hsic_row(m) and grad_chain(m) <= R.chain_hsic_row(m) and TOTAL_CHAIN <= R.chain_block(m)
    return R.hsic_closed(x, y, s_x, s_y, gs)


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
A1, A3, A8 = R.A1, R.A3, R.A8


def _hs(name, m, d, **kw):
    c = R._hs(name, m, d, **kw)
    c["seed"] += 50000
    return c


def _mmd(name, n1, n2, **kw):
    c = R._mmd(name, n1, n2, **kw)
    c["seed"] += 50000
    return c


# one tile (2, 3, 63, 64), the tile edge + 1 (65: 2 x 2 tiles, 63 masked rows), 129 (3 x 3 tiles, a last tile of one row); d = 1, 24, 63, 64
# (DQ = 4 / 8 / 16 accumulators); strided rows, a NULL upstream gradient, dependent and independent samples
HSIC_SMALL = [
    _hs("t_2", 2, 24, corr=True), _hs("t_3_d1", 3, 1, s=(0.5, 2.0)), _hs("t_63_d63", 63, 63, s=(0.5, 2.0), corr=True), _hs("t_64_d64", 64, 64),
    _hs("t_64_d1", 64, 1, corr=True), _hs("t_65_strided", 65, 24, corr=True, strided=True), _hs("t_65_d16", 65, 16, s=(0.5, 2.0)),
    _hs("t_129_grad_null", 129, 24, gs=None, corr=True), _hs("t_129_d64", 129, 64, s=(0.5, 2.0)), _hs("t_129_d33", 129, 33),
]
HSIC_ABOVE = _hs("t_800_above_the_lds_limit", 800, 24, s=(0.5, 2.0), corr=True)
HSIC_TOP = _hs("t_8192_row_limit", 8192, 24, corr=True, gs=0.75)

# the sample boundary inside a tile (2 | 2, 2 | 63, 33 | 31), on a tile edge (64 | 64) and one past it (65 | 64); a duplicate row across
# the samples; (1, .) is refused
MMD_SMALL = [
    _mmd("t_2_2", 2, 2), _mmd("t_2_63_d1", 2, 63, d=1, alphas=A3), _mmd("t_33_31_d63_strided", 33, 31, d=63, alphas=A8, strided=True),
    _mmd("t_33_31_duplicate", 33, 31, alphas=A3, dup=(5, 3), gs=0.75), _mmd("t_64_64_d64_equal", 64, 64, d=64, alphas=A3, eps=0.0, equal=True),
    _mmd("t_64_64_d2", 64, 64, d=2, alphas=A8, eps=1e-2), _mmd("t_65_64_grad_null", 65, 64, gs=None, alphas=A3), _mmd("t_65_64_d17", 65, 64, d=17),
]
MMD_ABOVE = _mmd("t_800_800_above_the_lds_limit", 800, 800, gs=0.75)

HSIC_CASES = HSIC_SMALL + [HSIC_ABOVE]
MMD_CASES = MMD_SMALL + [MMD_ABOVE]

ERR_ARG, ERR_SHAPE = R.ERR_ARG, R.ERR_SHAPE
# every refused call: (operator, what differs from a valid call, expected code).  "null": the pointer field set to NULL.
REFUSALS = [
    ("hsic", dict(m=1), ERR_SHAPE), ("hsic", dict(m=8193), ERR_SHAPE), ("hsic", dict(d=0), ERR_SHAPE), ("hsic", dict(d=65), ERR_SHAPE),
    ("hsic", dict(s=(0.0, 1.0)), ERR_ARG), ("hsic", dict(s=(1.0, -2.0)), ERR_ARG), ("hsic", dict(null="x"), ERR_ARG), ("hsic", dict(null="y"), ERR_ARG),
    ("hsic", dict(null="out"), ERR_ARG), ("hsic", dict(null="work"), ERR_ARG), ("hsic", dict(ldx=23), ERR_ARG),
    ("mmd", dict(n1=1), ERR_SHAPE), ("mmd", dict(n2=1), ERR_SHAPE), ("mmd", dict(n1=4097, n2=4096), ERR_SHAPE), ("mmd", dict(d=0), ERR_SHAPE),
    ("mmd", dict(d=65), ERR_SHAPE), ("mmd", dict(n_alphas=0), ERR_ARG), ("mmd", dict(n_alphas=9), ERR_ARG), ("mmd", dict(null="s1"), ERR_ARG),
    ("mmd", dict(null="s2"), ERR_ARG), ("mmd", dict(null="out"), ERR_ARG), ("mmd", dict(null="work"), ERR_ARG), ("mmd", dict(ld1=23), ERR_ARG),
]


def refusal_id(r):
    return "%s-%s" % (r[0], "-".join("%s_%s" % kv for kv in r[1].items()).replace(" ", ""))


@functools.lru_cache(maxsize=None)
def hsic_reference(name):
    """-> (case, x, y, gs, ref, bound) of a case of HSIC_CASES here or of stats_restate.HSIC_CASES, computed once"""
    if not name.startswith("t_"):
        return R.hsic_reference(name)
    c = R.by_name(HSIC_CASES, name)
    x, y = R.hsic_inputs(c)
    gs = 1.0 if c["gs"] is None else c["gs"]
    return (c, x, y, gs) + hsic_closed_tiled(x, y, *c["s"], gs)


@functools.lru_cache(maxsize=None)
def mmd_reference(name):
    """-> (case, s1, s2, gs, ref, bound), the gradient bounds with the tiled chain"""
    c = R.by_name(MMD_CASES + R.MMD_CASES, name)
    s1, s2 = R.mmd_inputs(c)
    gs = 1.0 if c["gs"] is None else c["gs"]
    return (c, s1, s2, gs) + mmd_closed_tiled(s1, s2, c["alphas"], c["eps"], gs)


# ------------------------------------------------------------------------------------------------ the row limit: m = 8192 in row blocks
def hsic_top_inputs():
    """stats_restate.hsic_inputs for HSIC_TOP without its m x m float64 scan: at std = 0.15 no exp argument comes near ARG_CLAMP
    (hsic_rows_closed asserts it block by block), so the draws are used as they are."""
    c = HSIC_TOP
    rs = np.random.RandomState(c["seed"])
    std = c["std"] / np.sqrt(c["d"] / 24.0)
    x = rs.randn(c["m"], c["d"]) * std
    y = 0.8 * x + 0.6 * std * rs.randn(c["m"], c["d"])
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y.astype(np.float32))


def hsic_rows_closed(x, y, s_x, s_y, gs, rows, device="cpu", block=1024):
    """stats_restate.hsic_closed restricted: the value and its bound, and the gradients and their bounds for the rows `rows` only, the
    m x m matrices visited in row blocks, in torch float64 on `device` (the CPU for the cross-check against hsic_closed on a small
    case, tests/test_stat_tiled_host.py; the GPU for m = 8192, where NumPy would take a minute).  Term by term the expressions and the
    roundings counted are those of hsic_closed.  Also returns perm_bound: the bound of the permutation test's observed statistic on
    the device's own Gram matrices (tests/test_gpu_hsic_perm_test.py: FACTOR * 2^-24 * sum |Kc| |L| plus what the hsic_kern errors
    of K and L move it by, 1 % for the second order), over (m-1)^2."""
    import torch
    from tests import hsic_perm_restate as HR
    x, y = (torch.from_numpy(np.asarray(t, np.float64)).to(device) for t in (x, y))
    m, d = x.shape
    U = R.U
    isx, isy = float(np.float32(1.0) / np.float32(s_x)), float(np.float32(1.0) / np.float32(s_y))
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    ax, ay = x.abs(), y.abs()
    row, blk = R.chain_hsic_row(m), R.chain_block(m)

    def block_of(idx):
        """K, L, EK, EL of the rows idx against every row"""
        out = []
        for z, nz, az, inv in ((x, nx, ax, isx), (y, ny, ay, isy)):
            d2 = nz[idx, None] + nz[None, :] - 2.0 * (z[idx] @ z.T)
            d2[torch.arange(len(idx), device=device), idx] = 0.0
            assert float(d2.max()) * inv <= R.ARG_CLAMP + 1.0
            S = nz[idx, None] + nz[None, :] + 2.0 * (az[idx] @ az.T)
            out += [torch.exp(-d2 * inv), inv * (d + 2) * S + (d2 * inv).abs() + 2.0]
        return out[0], out[2], out[1], out[3]

    rk, rl, e_rk, e_rl = (torch.empty(m, dtype=torch.float64, device=device) for _ in range(4))
    T1 = e1 = 0.0
    blocks = [torch.arange(b0, min(b0 + block, m), device=device) for b0 in range(0, m, block)]
    for idx in blocks:
        K, L, EK, EL = block_of(idx)
        rk[idx], rl[idx] = K.sum(1), L.sum(1)
        e_rk[idx], e_rl[idx] = (K * (EK + row)).sum(1), (L * (EL + row)).sum(1)
        T1 += float((K * L).sum())
        e1 += float((K * L * (EK + EL + 1 + row + blk)).sum())
    tk, tl = float(rk.sum()), float(rl.sum())
    T2, T3 = 2.0 / m * float((rk * rl).sum()), tk * tl / (m * m)
    den = (m - 1.0) ** 2
    e_tk, e_tl = float((e_rk + rk * blk).sum()), float((e_rl + rl * blk).sum())
    e2 = 2.0 / m * float((rl * e_rk + rk * e_rl + rk * rl * (1 + blk)).sum()) + 3.0 * T2
    e3 = (tl * e_tk + tk * e_tl) / (m * m) + 4.0 * T3
    b_hsic = U * (e1 + e2 + e3 + 4.0 * (T1 + T2 + T3)) / den

    def centred(K, L, idx):
        return (L - (rl[idx, None] + rl[None, :]) / m + tl / (m * m), K - (rk[idx, None] + rk[None, :]) / m + tk / (m * m))

    perm = 0.0
    for idx in blocks:
        K, L, EK, EL = block_of(idx)
        Lc, Kc = centred(K, L, idx)
        perm += HR.FACTOR * U * float((Kc.abs() * L).sum()) + 1.01 * U * float((Kc.abs() * L * EL).sum() + (Lc.abs() * K * EK).sum())
    idx = torch.as_tensor(np.asarray(rows), device=device)
    K, L, EK, EL = block_of(idx)
    inv = abs(gs) / den
    off = torch.ones((len(idx), m), dtype=torch.float64, device=device)
    off[torch.arange(len(idx), device=device), idx] = 0.0
    Lc, Kc = centred(K, L, idx)
    Cx, Cy = 2.0 * Lc * K * (-2.0 * isx) * gs / den * off, 2.0 * Kc * L * (-2.0 * isy) * gs / den * off
    gx = Cx.sum(1)[:, None] * x[idx] - Cx @ x
    gy = Cy.sum(1)[:, None] * y[idx] - Cy @ y
    mag_l = L + (rl[idx, None] + rl[None, :]) / m + tl / (m * m)
    mag_k = K + (rk[idx, None] + rk[None, :]) / m + tk / (m * m)
    e_lc = L * EL + (e_rl[idx, None] + e_rl[None, :]) / m + e_tl / (m * m) + 5.0 * mag_l
    e_kc = K * EK + (e_rk[idx, None] + e_rk[None, :]) / m + e_tk / (m * m) + 5.0 * mag_k
    Wx = 4.0 * isx * inv * K * (e_lc + Lc.abs() * (EK + 6 + row))
    Wy = 4.0 * isy * inv * L * (e_kc + Kc.abs() * (EL + 6 + row))
    b_gx, b_gy = (torch.empty((len(idx), d), dtype=torch.float64, device=device) for _ in range(2))
    for k in range(d):
        b_gx[:, k] = U * (Wx * (x[idx, k][:, None] - x[None, :, k]).abs()).sum(1)
        b_gy[:, k] = U * (Wy * (y[idx, k][:, None] - y[None, :, k]).abs()).sum(1)
    host = lambda t: t.cpu().numpy()
    return (dict(hsic=(T1 - T2 + T3) / den, gx=host(gx), gy=host(gy), terms=(T1 / den, T2 / den, T3 / den)),
            dict(hsic=b_hsic, gx=host(b_gx), gy=host(b_gy), perm=perm / den))


TOP_ROWS = tuple(range(70)) + tuple(range(8192 - 70, 8192))
