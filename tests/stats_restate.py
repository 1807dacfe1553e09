"""The stand-alone statistic operators -- carel_rbf_mmd_fwd/bwd, carel_pdist_fwd/bwd, carel_hsic_fwd/bwd, carel_vi_aprx/upper
(csrc/mmd.hip, mmd_device.h, hsic.hip, hsic_device.h, vi.hip) -- restated twice in float64: TEST INFRASTRUCTURE for
tests/test_stats_restate_host.py and tests/test_gpu_stats_sweep.py.

  (i)  *_formula(...): the formulas of oracle.carel_oracle.mmd_statistic / pdist / hsic_statistic / vi_aprx_loss / vi_upper_loss, line
       for line on torch tensors of any dtype (eps and the kernel widths are arguments here), so autograd gives the gradients: on
       .double() inputs the literal reference, on float32 inputs "stock torch float32".
  (ii) *_closed(...): value and gradients written out in NumPy without autograd (HSIC by the expansion of hsic_device.h:
       sum K.L - (2/m) sum RK.RL + TK.TL/m^2, gradients through (HLH) and (HKH); the VI nets by hand-written back-propagation).

Bounds.  Every bound is   |got - ref| <= 2^-24 * sum over terms of |term| * (L + E):
  L  the longest chain of sequential additions a term passes through, read off the kernel (chain_* below);
  E  the rounding budget of the term itself in units of 2^-24.  A kernel value exp(-a (eps + |d2|)) carries the error of its argument,
     a (d + 2) roundings of S = |zi|^2 + |zj|^2 + 2 sum_k |zik zjk| (d for the three fma chains, one each for the sum of the norms and the
     subtraction), plus the exponential's own: 2 for expf, |arg| + 2 for the __expf of hsic_kern (exp2(arg log2 e): the rounding of
     the scaled argument grows with |arg|).
The scalars are differences, so their "terms" are the positive magnitudes they are the difference of: MMD 2|a01| s12 + a00 s11 + a11 s22,
HSIC the three sums over (m-1)^2, VI-upper both squared-residual terms.  Gradients are bounded per element over the partner sum
sum_j |coef_ij| |z_ik - z_jk|.  pdist is bounded on dist^2 (PDIST_ROUND roundings of S + eps), |dist error| <= bound / (2 dist).
The kernels subtract z_ik - z_jk first; autograd of the reference's Gram form instead rounds c_ij z_ik and c_ij z_jk apart (the partner
j = i included) and subtracts afterwards, so where that cancellation is not averaged out over many partners stock torch float32 cannot
meet a bound in |z_ik - z_jk|: a pdist side whose rows have ONE partner (torch float32: up to 125 times the bound) and the HSIC case at
the goldens' scale, where the diagonal K_ii = 1 outweighs every off-diagonal value by 1e5 (up to 350 times).  For those alone the host
measurement takes the "*_operands" bounds, which add OPERANDS_ROUND (+ the row chain) roundings of sum_j |coef_ij| (|z_ik| + |z_jk|);
the kernels are held to the plain bounds on every case.
The VI bounds push an absolute error (in units of 2^-24) through the two small nets operation by operation (_vi_forward).

Input conditions (enforced by the builders, asserted by tests/test_stats_restate_host.py on every case):
  MMD, pdist  sign(d2) is decided: every pair of distinct rows has d2 >= 256 * 2^-24 * S (d <= 2: a jittered grid, plain draws fail it);
  VI          every hidden pre-activation of both nets is >= 1e-4 from 0, so the ReLU mask is decided (offending rows are redrawn);
  MMD, HSIC   every exp argument lies in [-20, 0] (the samples are scaled down where a draw would exceed it).
Nothing here touches the GPU or the library."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
LDS_FLOATS = 160 * 1024 // 4          # 40 960: what the three host checks accept


# ------------------------------------------------------------------------------------------------ what the host code picks, restated
def align4(n):
    return (n + 3) & ~3


def mmd_lds_floats(n, d):
    return 64 + align4(n) + n * (d | 1)


def hsic_lds_floats(m, d):
    return 64 + 4 * align4(m) + 2 * m * (d | 1)


def vi_lds_floats(B, D):
    return 16 + 6 * B * D


def largest_accepted(lds_floats, d):
    """the largest row count n with lds_floats(n, d) <= LDS_FLOATS"""
    n = 1
    while lds_floats(n + 1, d) <= LDS_FLOATS:
        n += 1
    return n


def mmd_bwd_group(n):
    """lanes per row of mmd_bwd_kernel<G>: 8 for n <= 128, 2 for n <= 512, else 1"""
    return 8 if n * 8 <= 1024 else (2 if n * 2 <= 1024 else 1)


def mmd_bwd_row_trips(n):
    return -(-n // (1024 // mmd_bwd_group(n)))


def chain_mmd_fwd(n):
    """mmd_forward_block: a thread adds every 1024th of the n*n kernel values, six butterfly levels, 16 wave sums in turn, the double
    combination rounded once."""
    return -(-n * n // 1024) + 6 + 16 + 1


def chain_mmd_bwd(n):
    """mmd_backward_row: a lane adds every G-th partner, log2(G) shuffle levels."""
    G = mmd_bwd_group(n)
    return -(-n // G) + int(math.log2(G))


def chain_block(rows, threads=1024):
    """a per-thread partial over ceil(rows / threads) rows, then block_sum: six butterfly levels and the wave sums in turn"""
    return -(-rows // threads) + 6 + threads // 64


def chain_hsic_row(m):
    return m                       # one thread adds the m partners of its row in turn


PDIST_ROUND = 6 + 1 + 3 + 2        # wave_sum butterfly, the product, (nx + ny, - 2 dot, + eps), sqrtf (1 ulp of dist = 2 of dist^2)
PDIST_COEF = 4                     # up * sg / dist (division 2), x - y, the fma
OPERANDS_ROUND = 3                 # autograd of the Gram form: c_ij z_ik and c_ij z_jk rounded apart, then subtracted (see *_operands)


# ------------------------------------------------------------------------------------------------ (i) the reference's formulas, torch
def pdist_formula(s1, s2, eps):
    n1 = (s1 * s1).sum(dim=1, keepdim=True)
    n2 = (s2 * s2).sum(dim=1, keepdim=True)
    d2 = n1 + n2.t() - 2.0 * (s1 @ s2.t())
    return torch.sqrt(eps + d2.abs())


def mmd_formula(s1, s2, alphas, eps, ret_matrix=False):
    n1, n2 = s1.shape[0], s2.shape[0]
    a00 = 1.0 / (n1 * (n1 - 1))
    a11 = 1.0 / (n2 * (n2 - 1))
    a01 = -1.0 / (n1 * n2)
    z = torch.cat((s1, s2), dim=0)
    if eps > 0:
        dsq = pdist_formula(z, z, eps) ** 2
    else:                          # sqrt(0) on the diagonal has no autograd: the reference's sqrt-then-square folded, as in the kernel
        nz = (z * z).sum(dim=1, keepdim=True)
        dsq = (nz + nz.t() - 2.0 * (z @ z.t())).abs()
    kern = None
    for a in alphas:
        ka = torch.exp(-a * dsq)
        kern = ka if kern is None else kern + ka
    k1, k2, k12 = kern[:n1, :n1], kern[n1:, n1:], kern[:n1, n1:]
    mmd = 2 * a01 * k12.sum() + a00 * (k1.sum() - torch.trace(k1)) + a11 * (k2.sum() - torch.trace(k2))
    return (mmd, kern) if ret_matrix else mmd


def _pairwise(t):
    inst = (t * t).sum(dim=-1).reshape(-1, 1)
    return -2 * (t @ t.t()) + inst + inst.t()


def hsic_formula(x, y, s_x, s_y):
    """the matrix form tr(L H K H) / (m-1)^2"""
    m = x.shape[0]
    K = torch.exp(-_pairwise(x) / s_x)
    L = torch.exp(-_pairwise(y) / s_y)
    Hm = torch.eye(m, dtype=x.dtype) - (1.0 / m) * torch.ones((m, m), dtype=x.dtype)
    return torch.trace(L @ (Hm @ (K @ Hm))) / ((m - 1) ** 2)


def hsic_three_sum_formula(x, y, s_x, s_y):
    """the same statistic by the expansion the kernel uses, in torch (for the float32 measurement)"""
    m = x.shape[0]
    K = torch.exp(-_pairwise(x) / s_x)
    L = torch.exp(-_pairwise(y) / s_y)
    rk, rl = K.sum(1), L.sum(1)
    return ((K * L).sum() - 2.0 / m * (rk * rl).sum() + rk.sum() * rl.sum() / (m * m)) / ((m - 1) ** 2)


def vi_net_formula(net, c):
    """net: 8 tensors (w1, b1, w2, b2) x (mu, log_var)"""
    def mlp(w1, b1, w2, b2):
        h = torch.relu(c @ w1.t() + b1)
        return h @ w2.t() + b2
    return mlp(*net[:4]), torch.tanh(mlp(*net[4:]))


def vi_aprx_formula(net, z_e, z_c):
    mu, lv = vi_net_formula(net, z_c.detach())
    return -((-(mu - z_e) ** 2 / lv.exp() - lv).sum(dim=1).mean(dim=0))


def vi_upper_formula(net, z_e, z_c, perm):
    mu, lv = vi_net_formula(net, z_c)
    positive = -(mu - z_e) ** 2 / lv.exp()
    negative = -(mu - z_e[perm.long()]) ** 2 / lv.exp()
    return (positive.sum(dim=-1) - negative.sum(dim=-1)).mean() / 2.


def f32_scalars(vals):
    """the float32 roundings of host scalars (alphas, eps), as Python floats: what the kernels receive"""
    return [float(np.float32(v)) for v in vals]


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(grad)


def mmd_literal(s1, s2, alphas, eps, gs, dtype=torch.float64):
    """-> dict(mmd, kern [n, n], g1, g2 = gs * d mmd / d s), NumPy float64, from mmd_formula in `dtype` under autograd."""
    a, b = _t(s1, dtype, True), _t(s2, dtype, True)
    al, (e,) = f32_scalars(alphas), f32_scalars([eps])
    mmd, kern = mmd_formula(a, b, al, e, ret_matrix=True)
    (mmd * gs).backward()
    return dict(mmd=float(mmd.detach().double()), kern=kern.detach().double().numpy(), g1=a.grad.double().numpy(), g2=b.grad.double().numpy())


def pdist_literal(s1, s2, eps, w, dtype=torch.float64):
    a, b = _t(s1, dtype, True), _t(s2, dtype, True)
    dist = pdist_formula(a, b, f32_scalars([eps])[0])
    (dist * _t(w, dtype)).sum().backward()
    return dict(dist=dist.detach().double().numpy(), g1=a.grad.double().numpy(), g2=b.grad.double().numpy())


def hsic_literal(x, y, s_x, s_y, gs, dtype=torch.float64, form=hsic_formula):
    a, b = _t(x, dtype, True), _t(y, dtype, True)
    h = form(a, b, s_x, s_y)
    (h * gs).backward()
    return dict(hsic=float(h.detach().double()), gx=a.grad.double().numpy(), gy=b.grad.double().numpy())


def vi_aprx_literal(net, z, dtype=torch.float64):
    D = z.shape[1] // 2
    leaf = [_t(w, dtype, True) for w in net]
    zt = _t(z, dtype)
    loss = vi_aprx_formula(leaf, zt[:, :D], zt[:, D:])
    loss.backward()
    return dict(loss=float(loss.detach().double()), grads=[w.grad.double().numpy() for w in leaf])


def vi_upper_literal(net, z, perm, dtype=torch.float64):
    D = z.shape[1] // 2
    ws = [_t(w, dtype) for w in net]
    ze, zc = _t(z[:, :D], dtype, True), _t(z[:, D:], dtype, True)
    loss = vi_upper_formula(ws, ze, zc, torch.from_numpy(np.asarray(perm)))
    loss.backward()
    return dict(loss=float(loss.detach().double()), dz=torch.cat((ze.grad, zc.grad), 1).double().numpy())


# ------------------------------------------------------------------------------------------------ (ii) closed forms and bounds, NumPy
def pair_terms(a, b=None):
    """-> (d2, S) of the row pairs of float64 a [n, d] and b (default a): d2 = |ai|^2 + |bj|^2 - 2 ai.bj and the magnitude it is the
    difference of, S = |ai|^2 + |bj|^2 + 2 sum_k |aik bjk|."""
    b = a if b is None else b
    na, nb = (a * a).sum(1), (b * b).sum(1)
    d2 = na[:, None] + nb[None, :] - 2.0 * (a @ b.T)
    S = na[:, None] + nb[None, :] + 2.0 * (np.abs(a) @ np.abs(b).T)
    if b is a:
        np.fill_diagonal(d2, 0.0)
    return d2, S


def _partner_sum(W, z):
    """out[i, k] = sum_j W[i, j] |z[i, k] - z[j, k]|"""
    out = np.empty(z.shape)
    for k in range(z.shape[1]):
        out[:, k] = (W * np.abs(z[:, k][:, None] - z[:, k][None, :])).sum(1)
    return out


def mmd_closed(s1, s2, alphas, eps, gs):
    """-> (result dict as mmd_literal, bound dict(mmd, kern [n, n], g1, g2))."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    n1, n2, d = s1.shape[0], s2.shape[0], s1.shape[1]
    n, na = n1 + n2, len(alphas)
    al, (e,) = f32_scalars(alphas), f32_scalars([eps])
    z = np.concatenate((s1, s2), 0)
    d2, S = pair_terms(z)
    ad = e + np.abs(d2)
    w = np.empty((n, n))
    w[:n1, :n1], w[n1:, n1:] = 1.0 / (n1 * (n1 - 1)), 1.0 / (n2 * (n2 - 1))
    w[:n1, n1:] = w[n1:, :n1] = -1.0 / (n1 * n2)
    off = 1.0 - np.eye(n)
    kern, dc = np.zeros((n, n)), np.zeros((n, n))
    kern_e, dc_e = np.zeros((n, n)), np.zeros((n, n))              # sum_a K_a E_a and sum_a a K_a E_a
    for a in al:
        ka = np.exp(-a * ad)
        E = a * (d + 2) * S + 2.0                                   # expf: 2
        kern += ka
        dc += a * ka
        kern_e += ka * E
        dc_e += a * ka * E
    mmd = float((w * kern * off).sum())
    C = -4.0 * w * dc * np.sign(d2) * gs * off                      # coef_ij; d mmd / d z_i = sum_j coef_ij (z_i - z_j)
    g = C.sum(1)[:, None] * z - C @ z
    Lf, Lb = chain_mmd_fwd(n), chain_mmd_bwd(n)
    b_mmd = U * float((np.abs(w) * off * (kern * Lf + kern_e)).sum())
    b_kern = U * (kern * na + kern_e)                               # kv += e: n_alphas additions
    Wc = 4.0 * np.abs(w) * abs(gs) * off * (dc * (Lb + na + 5) + dc_e)    # fma chain of dc, w as a float, two products, zi - zj, the fma
    b_g = U * _partner_sum(Wc, z)
    return (dict(mmd=mmd, kern=kern, g1=g[:n1], g2=g[n1:]), dict(mmd=b_mmd, kern=b_kern, g1=b_g[:n1], g2=b_g[n1:]))


def pdist_closed(s1, s2, eps, w):
    s1, s2, w = np.asarray(s1, np.float64), np.asarray(s2, np.float64), np.asarray(w, np.float64)
    (e,) = f32_scalars([eps])
    d2, S = pair_terms(s1, s2)
    dist = np.sqrt(e + np.abs(d2))
    C = w * np.sign(d2) / dist                                      # d dist_ij / d s1_i = sign (s1_i - s2_j) / dist
    g1 = C.sum(1)[:, None] * s1 - C @ s2
    g2 = C.sum(0)[:, None] * s2 - C.T @ s1
    b_d2 = U * PDIST_ROUND * (S + e)
    rel = b_d2 / (2.0 * dist * dist) / U                            # relative error of dist, in units of 2^-24
    b_g1, b_g2 = np.empty(s1.shape), np.empty(s2.shape)
    for k in range(s1.shape[1]):
        diff = np.abs(s1[:, k][:, None] - s2[:, k][None, :])
        b_g1[:, k] = U * (np.abs(C) * diff * (s2.shape[0] + PDIST_COEF + rel)).sum(1)     # one lane adds all partners in turn
        b_g2[:, k] = U * (np.abs(C) * diff * (s1.shape[0] + PDIST_COEF + rel)).sum(0)
    aC = np.abs(C)
    o_g1 = U * OPERANDS_ROUND * (aC.sum(1)[:, None] * np.abs(s1) + aC @ np.abs(s2))
    o_g2 = U * OPERANDS_ROUND * (aC.sum(0)[:, None] * np.abs(s2) + aC.T @ np.abs(s1))
    return (dict(dist=dist, g1=g1, g2=g2),
            dict(dist=b_d2 / (2.0 * dist), g1=b_g1, g2=b_g2, g1_operands=b_g1 + o_g1, g2_operands=b_g2 + o_g2))


def hsic_closed(x, y, s_x, s_y, gs):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m, d = x.shape
    isx, isy = float(np.float32(1.0) / np.float32(s_x)), float(np.float32(1.0) / np.float32(s_y))
    dx, Sx = pair_terms(x)
    dy, Sy = pair_terms(y)
    K, L = np.exp(-dx * isx), np.exp(-dy * isy)
    EK = isx * (d + 2) * Sx + np.abs(dx * isx) + 2.0               # __expf: |arg| + 2
    EL = isy * (d + 2) * Sy + np.abs(dy * isy) + 2.0
    rk, rl = K.sum(1), L.sum(1)
    tk, tl = rk.sum(), rl.sum()
    T1, T2, T3 = (K * L).sum(), 2.0 / m * (rk * rl).sum(), tk * tl / (m * m)
    den = (m - 1.0) ** 2
    hsic = (T1 - T2 + T3) / den
    Lc = L - (rl[:, None] + rl[None, :]) / m + tl / (m * m)         # (H L H)
    Kc = K - (rk[:, None] + rk[None, :]) / m + tk / (m * m)
    off = 1.0 - np.eye(m)                                           # the partner j = i contributes c_ii (x_i - x_i) = 0
    Cx, Cy = 2.0 * Lc * K * (-2.0 * isx) * gs / den * off, 2.0 * Kc * L * (-2.0 * isy) * gs / den * off
    gx = Cx.sum(1)[:, None] * x - Cx @ x
    gy = Cy.sum(1)[:, None] * y - Cy @ y
    # errors in units of 2^-24
    row, blk = chain_hsic_row(m), chain_block(m)
    e_rk, e_rl = (K * (EK + row)).sum(1), (L * (EL + row)).sum(1)  # of the row sums
    e_tk, e_tl = (e_rk + rk * blk).sum(), (e_rl + rl * blk).sum()
    e1 = (K * L * (EK + EL + 1 + row + blk)).sum()
    e2 = 2.0 / m * (rl * e_rk + rk * e_rl + rk * rl * (1 + blk)).sum() + 3.0 * T2
    e3 = (tl * e_tk + tk * e_tl) / (m * m) + 4.0 * T3
    b_hsic = U * (e1 + e2 + e3 + 4.0 * (T1 + T2 + T3)) / den
    inv = abs(gs) / den
    mag_l = L + (rl[:, None] + rl[None, :]) / m + tl / (m * m)      # what (H L H)_ij is the difference of
    mag_k = K + (rk[:, None] + rk[None, :]) / m + tk / (m * m)
    e_lc = L * EL + (e_rl[:, None] + e_rl[None, :]) / m + e_tl / (m * m) + 5.0 * mag_l
    e_kc = K * EK + (e_rk[:, None] + e_rk[None, :]) / m + e_tk / (m * m) + 5.0 * mag_k
    Wx = 4.0 * isx * inv * K * (e_lc + np.abs(Lc) * (EK + 6 + row))      # four products, xi - xj, the fma; m partners in turn
    Wy = 4.0 * isy * inv * L * (e_kc + np.abs(Kc) * (EL + 6 + row))
    b_gx, b_gy = U * _partner_sum(Wx, x), U * _partner_sum(Wy, y)
    aCx, aCy = 4.0 * isx * inv * K * np.abs(Lc), 4.0 * isy * inv * L * np.abs(Kc)       # the diagonal (K_ii = 1) included
    o_gx = U * (OPERANDS_ROUND + row) * (aCx.sum(1)[:, None] * np.abs(x) + aCx @ np.abs(x))
    o_gy = U * (OPERANDS_ROUND + row) * (aCy.sum(1)[:, None] * np.abs(y) + aCy @ np.abs(y))
    return (dict(hsic=hsic, gx=gx, gy=gy, terms=(T1 / den, T2 / den, T3 / den)),
            dict(hsic=b_hsic, gx=b_gx, gy=b_gy, gx_operands=b_gx + o_gx, gy_operands=b_gy + o_gy))


def _vi_mlp(w1, b1, w2, b2, c):
    """-> pre, h, out and the error bounds (units of 2^-24) of h and out: each output is a bias plus D fmas in turn."""
    D = c.shape[1]
    pre = c @ w1.T + b1
    h = np.maximum(pre, 0.0)
    out = h @ w2.T + b2
    e_h = D * (np.abs(c) @ np.abs(w1).T + np.abs(b1)) * (pre > 0)
    e_out = e_h @ np.abs(w2).T + D * (h @ np.abs(w2).T + np.abs(b2))
    return pre, h, out, e_h, e_out


def _vi_mlp_bwd(w1, w2, pre, dout, e_dout):
    D = pre.shape[1]
    mask = pre > 0
    dh = (dout @ w2) * mask
    e_dh = (e_dout @ np.abs(w2) + D * (np.abs(dout) @ np.abs(w2))) * mask
    dc = dh @ w1
    e_dc = e_dh @ np.abs(w1) + D * (np.abs(dh) @ np.abs(w1))
    return dh, e_dh, dc, e_dc


def _vi_forward(net, z):
    net = [np.asarray(w, np.float64) for w in net]
    z = np.asarray(z, np.float64)
    D = z.shape[1] // 2
    e, c = z[:, :D], z[:, D:]
    f = dict(net=net, e=e, c=c, B=z.shape[0], D=D)
    f["pm"], f["hm"], mu, f["e_hm"], e_mu = _vi_mlp(*net[:4], c)
    f["pl"], f["hl"], lp, f["e_hl"], e_lp = _vi_mlp(*net[4:], c)
    lv = np.tanh(lp)
    e_lv = e_lp * (1.0 - lv * lv) + 2.0 * np.abs(lv)               # tanhf: 2
    s = np.exp(-lv)
    f.update(mu=mu, e_mu=e_mu, lv=lv, e_lv=e_lv, s=s, e_s=s * (e_lv + 2.0))     # expf: 2
    f["chain"] = D * -(-f["B"] // 256) + 6 + 4 + 2                 # a thread's samples and features in turn, block_sum of 256, the scale
    return f


def _vi_through_tanh(f, dlv, e_dlv):
    lv, e_lv = f["lv"], f["e_lv"]
    dol = dlv * (1.0 - lv * lv)
    e_dol = e_dlv * (1.0 - lv * lv) + np.abs(dlv) * (2.0 * np.abs(lv) * e_lv + 2.0 * (1.0 + lv * lv)) + np.abs(dol)
    return dol, e_dol


def vi_aprx_closed(net, z):
    """-> (dict(loss, grads [8]), dict(loss, grads [8]) of bounds)."""
    f = _vi_forward(net, z)
    B, s, e_s, lv = f["B"], f["s"], f["e_s"], f["lv"]
    r = f["mu"] - f["e"]
    e_r = f["e_mu"] + np.abs(r)
    loss = float((r * r * s + lv).sum() / B)
    e_t = 2.0 * np.abs(r) * e_r * s + r * r * e_s + 3.0 * r * r * s + f["e_lv"]
    b_loss = U * float((e_t + f["chain"] * (r * r * s + np.abs(lv))).sum() / B)
    dom = 2.0 * r * s / B
    e_dom = (2.0 / B) * (e_r * s + np.abs(r) * e_s + 3.0 * np.abs(r) * s)
    dlv = (-r * r * s + 1.0) / B
    e_dlv = (2.0 * np.abs(r) * e_r * s + r * r * e_s + 3.0 * r * r * s + 2.0 * (r * r * s + 1.0)) / B
    dol, e_dol = _vi_through_tanh(f, dlv, e_dlv)
    grads, bounds = [], []
    for (w1, b1, w2, b2), pre, h, e_h, dout, e_dout in ((f["net"][:4], f["pm"], f["hm"], f["e_hm"], dom, e_dom),
                                                        (f["net"][4:], f["pl"], f["hl"], f["e_hl"], dol, e_dol)):
        dh, e_dh, _, _ = _vi_mlp_bwd(w1, w2, pre, dout, e_dout)
        c = f["c"]
        grads += [dh.T @ c, dh.sum(0), dout.T @ h, dout.sum(0)]   # a thread per weight adds the B samples in turn
        bounds += [U * (e_dh.T @ np.abs(c) + B * (np.abs(dh).T @ np.abs(c))), U * (e_dh.sum(0) + B * np.abs(dh).sum(0)),
                   U * (e_dout.T @ h + np.abs(dout).T @ e_h + B * (np.abs(dout).T @ h)), U * (e_dout.sum(0) + B * np.abs(dout).sum(0))]
    return dict(loss=loss, grads=grads), dict(loss=b_loss, grads=bounds)


def vi_upper_closed(net, z, perm):
    """-> (dict(loss, dz [B, 2D], terms), dict(loss, dz) of bounds); terms = sum of both squared-residual terms / (2B)."""
    f = _vi_forward(net, z)
    perm = np.asarray(perm).astype(np.int64)
    B, D, s, e_s = f["B"], f["D"], f["s"], f["e_s"]
    k = 0.5 / B
    r, r2 = f["mu"] - f["e"], f["mu"] - f["e"][perm]
    e_r, e_r2 = f["e_mu"] + np.abs(r), f["e_mu"] + np.abs(r2)
    sq = (r * r + r2 * r2) * s
    loss = float(k * ((-r * r + r2 * r2) * s).sum())
    e_t = 2.0 * (np.abs(r) * e_r + np.abs(r2) * e_r2) * s + (r * r + r2 * r2) * e_s + 3.0 * sq
    b_loss = U * k * float((e_t + f["chain"] * sq).sum())
    a1 = np.abs(r) + np.abs(r2)
    dom = k * (-2.0 * r + 2.0 * r2) * s
    e_dom = 2.0 * k * s * (e_r + e_r2) + 2.0 * k * a1 * (e_s + 5.0 * s)
    dlv = k * (r * r - r2 * r2) * s
    e_dlv = 2.0 * k * s * (np.abs(r) * e_r + np.abs(r2) * e_r2) + k * (r * r + r2 * r2) * (e_s + 5.0 * s)
    dol, e_dol = _vi_through_tanh(f, dlv, e_dlv)
    own, neg = 2.0 * k * r * s, -2.0 * k * r2 * s                   # added at row b and at row perm[b]
    e_own = 2.0 * k * (e_r * s + np.abs(r) * e_s + 3.0 * np.abs(r) * s)
    e_neg = 2.0 * k * (e_r2 * s + np.abs(r2) * e_s + 3.0 * np.abs(r2) * s)
    dze, b_dze = own.copy(), e_own + np.abs(own)
    np.add.at(dze, perm, neg)
    np.add.at(b_dze, perm, e_neg + np.abs(neg))
    _, _, dcm, e_dcm = _vi_mlp_bwd(f["net"][0], f["net"][2], f["pm"], dom, e_dom)
    _, _, dcl, e_dcl = _vi_mlp_bwd(f["net"][4], f["net"][6], f["pl"], dol, e_dol)
    dzc, b_dzc = dcm + dcl, e_dcm + e_dcl + 2.0 * (np.abs(dcm) + np.abs(dcl))
    return (dict(loss=loss, dz=np.concatenate((dze, dzc), 1), terms=float(k * sq.sum())),
            dict(loss=b_loss, dz=U * np.concatenate((b_dze, b_dzc), 1)))


# ------------------------------------------------------------------------------------------------ input builders
ARG_TARGET = 12.0        # the MMD samples are scaled so that the largest |exp argument| is this
ARG_CLAMP = 19.0         # the HSIC samples are scaled down to this where a draw exceeds it
SIGN_MARGIN = 256.0      # d2 >= SIGN_MARGIN * 2^-24 * S for every pair of distinct rows
RELU_MARGIN = 1e-4


def _grid(rs, n, d):
    """n distinct points of a unit grid in d <= 2 dimensions, centred, each moved by at most 0.15 per coordinate"""
    if d == 1:
        p = rs.permutation(n).astype(np.float64)[:, None] - (n - 1) / 2.0
    else:
        side = int(math.ceil(math.sqrt(n)))
        cell = rs.permutation(side * side)[:n]
        p = np.stack((cell // side, cell % side), 1).astype(np.float64) - (side - 1) / 2.0
    return p + rs.uniform(-0.15, 0.15, size=p.shape)


def mmd_inputs(case):
    """-> (s1, s2) float32.  Normal draws (d <= 2: the jittered grid); sample 2 has another mean and spread unless case["equal"];
    case["dup"] = (i, j) copies row i of sample 1 over row j of sample 2; both are then scaled so that the largest exp argument is
    ARG_TARGET."""
    rs = np.random.RandomState(case["seed"])
    n1, n2, d = case["n1"], case["n2"], case["d"]
    z = _grid(rs, n1 + n2, d) if d <= 2 else rs.randn(n1 + n2, d)
    if d > 2 and not case.get("equal"):
        z[n1:] = z[n1:] * 1.2 + 0.5
    if case.get("dup"):
        z[n1 + case["dup"][1]] = z[case["dup"][0]]
    d2, _ = pair_terms(z)
    z *= math.sqrt(ARG_TARGET / (max(case["alphas"]) * (case["eps"] + d2.max())))
    z = z.astype(np.float32)
    return np.ascontiguousarray(z[:n1]), np.ascontiguousarray(z[n1:])


def pdist_inputs(case):
    """-> (s1, s2, w) float32; w: the upstream gradient.  case["far"]: sample 2 moved by +30 per coordinate; case["dup"]: s2[0] = s1[0],
    with upstream weight 0 (the sign of that pair's gradient is undefined)."""
    rs = np.random.RandomState(case["seed"])
    n1, n2, d = case["n1"], case["n2"], case["d"]
    z = _grid(rs, n1 + n2, d) if d <= 2 else rs.randn(n1 + n2, d)
    if case.get("far"):
        z[n1:] += 30.0
    w = rs.randn(n1, n2)
    if case.get("dup"):
        z[n1] = z[0]
        w[0, 0] = 0.0
    z = z.astype(np.float32)
    return np.ascontiguousarray(z[:n1]), np.ascontiguousarray(z[n1:]), w.astype(np.float32)


def hsic_inputs(case):
    """-> (x, y) float32 of standard deviation case["std"] / sqrt(d / 24) (off-diagonal kernel values of 0.1 .. 0.9 at 0.15);
    case["corr"]: y = 0.8 x + 0.6 noise, else independent; scaled down where an exp argument would pass ARG_CLAMP."""
    rs = np.random.RandomState(case["seed"])
    m, d = case["m"], case["d"]
    std = case["std"] / math.sqrt(d / 24.0)
    x = rs.randn(m, d) * std
    y = 0.8 * x + 0.6 * std * rs.randn(m, d) if case["corr"] else rs.randn(m, d) * std
    worst = max(pair_terms(x)[0].max() / case["s"][0], pair_terms(y)[0].max() / case["s"][1])
    if worst > ARG_CLAMP:
        x, y = x * math.sqrt(ARG_CLAMP / worst), y * math.sqrt(ARG_CLAMP / worst)
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y.astype(np.float32))


def vi_hidden_margin(net, z):
    """the smallest |hidden pre-activation| of either net, per sample"""
    D = z.shape[1] // 2
    c = np.asarray(z, np.float64)[:, D:]
    pre = [c @ np.asarray(net[i], np.float64).T + np.asarray(net[i + 1], np.float64) for i in (0, 4)]
    return np.minimum(np.abs(pre[0]).min(1), np.abs(pre[1]).min(1))


def vi_inputs(case):
    """-> (net: 8 float32 arrays, nn.Linear-style uniform(+-1/sqrt(D)); z float32 [B, 2D], N(0, 0.8)); rows with a hidden pre-activation
    within RELU_MARGIN of 0 are drawn again."""
    rs = np.random.RandomState(case["seed"])
    B, D = case["B"], case["D"]
    bound = 1.0 / math.sqrt(D)
    net = [rs.uniform(-bound, bound, size=sh).astype(np.float32) for sh in [(D, D), (D,), (D, D), (D,)] * 2]
    z = (rs.standard_normal((B, 2 * D)) * 0.8).astype(np.float32)
    for _ in range(1000):
        bad = np.nonzero(vi_hidden_margin(net, z) < RELU_MARGIN)[0]
        if bad.size == 0:
            return net, z
        z[bad] = (rs.standard_normal((bad.size, 2 * D)) * 0.8).astype(np.float32)
    raise AssertionError("vi_inputs: no draw clears the ReLU margin")


PERM_KINDS = ("random", "identity", "fixed")


def vi_perm(case, kind):
    """int32 [B]: a random permutation, the identity, or a permutation that leaves every third index (and maybe more) in place"""
    rs = np.random.RandomState(case["seed"] + 7919)
    B = case["B"]
    if kind == "random":
        p = rs.permutation(B)
    else:
        p = np.arange(B)
        if kind == "fixed":
            moving = np.nonzero(p % 3 != 0)[0]
            p[moving] = moving[rs.permutation(moving.size)]
    return p.astype(np.int32)


# ------------------------------------------------------------------------------------------------ the cases of the GPU sweep
A1, A3, A8 = (0.1,), (0.1, 0.5, 2.0), (0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0)


def _mmd(name, n1, n2, d=24, alphas=A1, eps=1e-5, gs=-1.0, **kw):
    return dict(name=name, n1=n1, n2=n2, d=d, alphas=alphas, eps=eps, gs=gs, seed=1000 + 7 * n1 + n2 + 131 * d, **kw)


MMD_CASES = [
    # mmd_bwd_kernel<8>: n1 + n2 <= 128
    _mmd("g8_2_2", 2, 2), _mmd("g8_64_64_equal", 64, 64, alphas=A3, eps=0.0, equal=True), _mmd("g8_2_126", 2, 126, eps=1e-2, gs=0.75),
    _mmd("g8_126_2", 126, 2, alphas=A8),
    _mmd("g8_d1", 9, 8, d=1, alphas=A3), _mmd("g8_d2", 9, 8, d=2, alphas=A3), _mmd("g8_d63", 9, 8, d=63, alphas=A3),
    _mmd("g8_d64", 9, 8, d=64, alphas=A3, eps=1e-2),
    _mmd("g8_strided", 40, 56, alphas=A3, strided=True), _mmd("g8_grad_null", 33, 30, alphas=A3, gs=None),
    _mmd("g8_duplicate", 20, 20, alphas=A3, dup=(5, 3)),
    # mmd_bwd_kernel<2>: 128 < n1 + n2 <= 512
    _mmd("g2_65_64", 65, 64), _mmd("g2_100_156", 100, 156, alphas=A3, eps=1e-2, gs=0.75), _mmd("g2_256_256_equal", 256, 256, alphas=A8, eps=0.0, equal=True),
    _mmd("g2_d1", 65, 64, d=1), _mmd("g2_d63", 70, 61, d=63, alphas=A3),
    # mmd_bwd_kernel<1>: n1 + n2 > 512; one row trip up to 1024 rows, two above
    _mmd("g1_257_256_matrix", 257, 256, kern=True), _mmd("g1_d2", 257, 256, d=2, alphas=A3), _mmd("g1_500_600_two_trips", 500, 600, alphas=A3, gs=0.75),
    _mmd("g1_700_872_lds_top", 700, 872), _mmd("g1_300_319_d64_lds_top", 300, 319, d=64, eps=0.0),
]


def _pd(name, n1, n2, d, eps=1e-5, **kw):
    return dict(name=name, n1=n1, n2=n2, d=d, eps=eps, seed=2000 + 7 * n1 + n2 + 131 * d, **kw)


# pdist_fwd_kernel / pdist_bwd_kernel<0>, <1>: one wave per row, lane = feature (d = 63, 64: the last lane idle / every lane live)
PDIST_CASES = ([_pd("p_%d_%d_d%d" % (n1, n2, d), n1, n2, d) for d in (1, 24, 63, 64) for n1, n2 in ((1, 1), (1, 70), (70, 1), (40, 56))]
               + [_pd("p_130_65_d%d" % d, 130, 65, d) for d in (24, 63, 64)]
               + [_pd("p_strided", 40, 56, 24, strided=True), _pd("p_far", 40, 56, 24, far=True), _pd("p_coincident", 40, 56, 24, far=True, dup=True),
                  _pd("p_eps0", 40, 56, 24, eps=0.0)])


def _hs(name, m, d, s=(1.0, 1.0), corr=False, std=0.15, gs=3.0, **kw):
    return dict(name=name, m=m, d=d, s=s, corr=corr, std=std, gs=gs, seed=3000 + 7 * m + 131 * d, **kw)


HSIC_CASES = [
    # one row per thread, LDS <= 64 KB
    _hs("h_2", 2, 24, corr=True), _hs("h_3", 3, 24, s=(0.5, 2.0)), _hs("h_17", 17, 24, corr=True), _hs("h_64", 64, 24, s=(0.5, 2.0)),
    _hs("h_65", 65, 24, corr=True), _hs("h_17_d1", 17, 1), _hs("h_64_d1", 64, 1, s=(0.5, 2.0)), _hs("h_33_d16", 33, 16),
    _hs("h_40_d64", 40, 64, corr=True, s=(0.5, 2.0)), _hs("h_strided", 50, 24, corr=True, strided=True), _hs("h_grad_null", 30, 24, gs=None),
    _hs("h_golden_scale", 17, 24, std=0.5, corr=True),
    # LDS above 64 KB (hipFuncSetAttribute), up to the largest accepted m
    _hs("h_300", 300, 24), _hs("h_757_lds_top", 757, 24, s=(0.5, 2.0), corr=True),
    # m > 1024: two rows per thread
    _hs("h_1025_d16", 1025, 16), _hs("h_1076_d16_lds_top", 1076, 16, corr=True),
]

# vi_kernel<0>, <1>: 256 threads, a sample per thread: a second trip from B = 257, eight at 2000; LDS top at (284, 24) and (213, 32)
VI_CASES = [dict(name="v_%d_%d" % (B, D), B=B, D=D, seed=4000 + 7 * B + 131 * D)
            for B, D in ((1, 1), (1, 32), (255, 24), (256, 24), (257, 24), (284, 24), (213, 32), (300, 16), (2000, 3))]

ERR_ARG, ERR_SHAPE = -1, -2
# every refused call: (operator, arguments, expected return code); nothing may be launched
REFUSALS = [
    ("mmd", dict(n1=700, n2=873, d=24, n_alphas=1), ERR_SHAPE), ("mmd", dict(n1=8, n2=8, d=0, n_alphas=1), ERR_SHAPE),
    ("mmd", dict(n1=8, n2=8, d=65, n_alphas=1), ERR_SHAPE), ("mmd", dict(n1=1, n2=8, d=24, n_alphas=1), ERR_SHAPE),
    ("mmd", dict(n1=127, n2=1, d=24, n_alphas=1), ERR_SHAPE), ("mmd", dict(n1=8, n2=8, d=24, n_alphas=0), ERR_ARG),
    ("mmd", dict(n1=8, n2=8, d=24, n_alphas=9), ERR_ARG),
    ("pdist", dict(n1=4, n2=4, d=0), ERR_SHAPE), ("pdist", dict(n1=4, n2=4, d=65), ERR_SHAPE), ("pdist", dict(n1=0, n2=4, d=24), ERR_SHAPE),
    ("hsic", dict(m=758, d=24, s=(1.0, 1.0)), ERR_SHAPE), ("hsic", dict(m=1077, d=16, s=(1.0, 1.0)), ERR_SHAPE),
    ("hsic", dict(m=8, d=0, s=(1.0, 1.0)), ERR_SHAPE), ("hsic", dict(m=8, d=65, s=(1.0, 1.0)), ERR_SHAPE),
    ("hsic", dict(m=1, d=24, s=(1.0, 1.0)), ERR_SHAPE), ("hsic", dict(m=8, d=24, s=(0.0, 1.0)), ERR_ARG),
    ("hsic", dict(m=8, d=24, s=(1.0, -2.0)), ERR_ARG),
    ("vi", dict(B=285, D=24), ERR_SHAPE), ("vi", dict(B=214, D=32), ERR_SHAPE), ("vi", dict(B=8, D=0), ERR_SHAPE), ("vi", dict(B=8, D=33), ERR_SHAPE),
    ("vi", dict(B=0, D=24), ERR_SHAPE),
]


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


# ------------------------------------------------------------------------------------------------ each case's inputs, reference and bounds, computed once
@functools.lru_cache(maxsize=None)
def mmd_reference(name):
    c = by_name(MMD_CASES, name)
    s1, s2 = mmd_inputs(c)
    gs = 1.0 if c["gs"] is None else c["gs"]
    return (c, s1, s2, gs) + mmd_closed(s1, s2, c["alphas"], c["eps"], gs)


@functools.lru_cache(maxsize=None)
def pdist_reference(name):
    c = by_name(PDIST_CASES, name)
    s1, s2, w = pdist_inputs(c)
    return (c, s1, s2, w) + pdist_closed(s1, s2, c["eps"], w)


@functools.lru_cache(maxsize=None)
def hsic_reference(name):
    c = by_name(HSIC_CASES, name)
    x, y = hsic_inputs(c)
    gs = 1.0 if c["gs"] is None else c["gs"]
    return (c, x, y, gs) + hsic_closed(x, y, *c["s"], gs)


@functools.lru_cache(maxsize=None)
def vi_reference(name):
    c = by_name(VI_CASES, name)
    net, z = vi_inputs(c)
    perms = {k: vi_perm(c, k) for k in PERM_KINDS}
    return c, net, z, perms, vi_aprx_closed(net, z), {k: vi_upper_closed(net, z, p) for k, p in perms.items()}


def frac(got, ref, bound):
    """the worst |got - ref| / bound over the elements (0 / 0 counts as 0, x / 0 as inf)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bound)
    return float(np.max(f)) if f.size else 0.0
