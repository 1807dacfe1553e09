"""The stand-alone statistic operators through the C ABI -- carel_rbf_mmd_fwd/bwd, carel_pdist_fwd/bwd, carel_hsic_fwd/bwd, carel_vi_aprx,
carel_vi_upper -- against the float64 restatements of tests/stats_restate.py, over every launch form the host code picks:
mmd_bwd_kernel<8>, <2>, <1> (one and two row trips), LDS below and above 64 KB up to the largest accepted size, one and two rows per
thread of hsic_kernel, one to eight sample trips of vi_kernel, d = 1 .. 64, strided rows, NULL upstream gradients, 1 / 3 / 8 alphas.
Every output starts as NaN between guard regions at exactly the size the header states, the guards must be intact afterwards, a second
identical call must give the same bits (carel_vi_upper too: with a permutation every dz address gets at most two atomic adds onto a
zeroed buffer), and every refused call must leave every output NaN.  The bounds (L + E roundings of the magnitudes a result is made of)
and the cases are those of tests/stats_restate.py; tests/test_stats_restate_host.py holds stock torch float32 on the CPU to half of them.
Run with -s: every case prints its worst fraction of each bound.

Worst fractions of the bound over all cases, torch float32 on the CPU | the kernels on an MI355X:
    MMD    value, g1, g2, kernel matrix (n = 513)      0.175, 0.097, 0.128, 0.167 | 0.013, 0.055, 0.088, 0.151
    pdist  dist, g1, g2                                0.412, 0.052, 0.067        | 0.324, 0.234, 0.235
    HSIC   value, gx, gy   matrix form                 0.002, 0.148, 0.300        | 0.005, 0.017, 0.023
                           three sums                  0.006, 0.189, 0.159
    VI     aprx loss, aprx gradients                   0.051, 0.113               | 0.030, 0.113
           upper bound, dz                             0.001, 0.205               | 0.001, 0.208
torch float32 is held to the wider "operands" bounds on the pdist sides with one partner per row and on the HSIC case at the goldens'
scale (0.260 and 0.140 of those; 125 and 350 times the plain bounds, see tests/stats_restate.py); the kernels' figures above are against
the plain bounds on every case, those included (0.235 and 0.012 there).  The __expf of hsic_kern and the three-sum cancellation cost
nothing that shows: HSIC is at 0.005 of a bound that torch's matrix form meets at 0.002 and its three-sum form at 0.006.  With the
identity permutation carel_vi_upper returns exactly 0 and an exactly zero e-half of dz.  The sweep found no fault in a kernel; the host
wrapper ops._mmd_args let samples of different feature width through (the kernel then read past the rows of the narrower one) and
overran its alpha array at nine alphas: both are refused now (the last test).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from tests import stats_restate as R
from tests.gpu_util import Arena, bits

pytestmark = pytest.mark.gpu


def _names(cases):
    return [c["name"] for c in cases]


def _put(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slice_of_wider(a, left, right):
    """a [n, d] as a column slice of a wider device matrix whose other columns are NaN -> (view, row stride)"""
    n, d = a.shape
    wide = torch.full((n, left + d + right), float("nan"), device="cuda")
    wide[:, left:left + d] = _put(a)
    return wide[:, left:left + d], wide.stride(0)


def _sample(a, strided, left, right):
    if strided:
        return _slice_of_wider(a, left, right)
    t = _put(a)
    return t, t.stride(0)


def _snapshot(ar):
    return [bits(b.t) for b in ar.all]


def _refill(ar):
    for b in ar.all:
        b.t.fill_(float("nan"))


def _twice(ar, call):
    """run `call` on NaN outputs, then again on NaN outputs: same bits, guards intact"""
    call()
    torch.cuda.synchronize()
    first = _snapshot(ar)
    _refill(ar)
    call()
    torch.cuda.synchronize()
    assert ar.intact()
    for a, b in zip(first, _snapshot(ar)):
        assert torch.equal(a, b)


def _np(buf):
    return buf.t.detach().cpu().double().numpy()


def _check(tag, name, fracs):
    print("FRAC %s %s " % (tag, name) + " ".join("%s=%.3f" % kv for kv in fracs.items()))
    assert all(v <= 1.0 for v in fracs.values()), (tag, name, fracs)


def _ok(rc, what):
    L.check(rc, what)


# ------------------------------------------------------------------------------------------------ MMD
def _mmd_args(s1, ld1, s2, ld2, n1, n2, d, alphas, eps):
    a = L.MmdArgs()
    a.s1, a.s2, a.ld1, a.ld2 = s1.data_ptr(), s2.data_ptr(), ld1, ld2
    a.n1, a.n2, a.d, a.n_alphas, a.eps = n1, n2, d, len(alphas), eps
    for i, v in enumerate(alphas):
        a.alphas[i] = v
    return a


@pytest.mark.parametrize("name", _names(R.MMD_CASES))
def test_mmd_forward_and_backward(name):
    """MMD_CASES names the form each case reaches: g8_ / g2_ / g1_ = mmd_bwd_kernel<8> / <2> / <1>."""
    c, s1, s2, gs, ref, bound = R.mmd_reference(name)
    n1, n2, d = c["n1"], c["n2"], c["d"]
    n = n1 + n2
    lib = L.load()
    t1, ld1 = _sample(s1, c.get("strided"), 5, 8)
    t2, ld2 = _sample(s2, c.get("strided"), 26, 0)
    ar = Arena(seed=n)
    out, g1, g2 = ar.nan((1,)), ar.nan((n1, d)), ar.nan((n2, d))
    kern = ar.nan((n * n,)) if c.get("kern") else None
    grad = None if c["gs"] is None else torch.tensor([gs], device="cuda", dtype=torch.float32)
    a = _mmd_args(t1, ld1, t2, ld2, n1, n2, d, c["alphas"], c["eps"])
    a.mmd_out, a.kernels_out = out.ptr, None if kern is None else kern.ptr
    a.grad_mmd, a.g1, a.g2 = None if grad is None else grad.data_ptr(), g1.ptr, g2.ptr

    def call():
        _ok(lib.carel_rbf_mmd_fwd(C.byref(a), L.current_stream()), "mmd fwd")
        _ok(lib.carel_rbf_mmd_bwd(C.byref(a), L.current_stream()), "mmd bwd")
    _twice(ar, call)
    got = dict(mmd=_np(out)[0], g1=_np(g1), g2=_np(g2))
    assert all(np.isfinite(v).all() for v in got.values())
    fr = {k: R.frac(got[k], ref[k], bound[k]) for k in ("mmd", "g1", "g2")}
    if kern is not None:
        K = kern.t.view(n, n)
        assert torch.equal(bits(K), bits(K.t()))                                  # the same fma chain with the operands swapped
        fr["kern"] = R.frac(_np(kern).reshape(n, n), ref["kern"], bound["kern"])
    if c["gs"] is None:                                                           # grad_mmd == NULL is an upstream gradient of 1
        one = torch.ones(1, device="cuda")
        h1, h2 = ar.nan((n1, d)), ar.nan((n2, d))
        a.grad_mmd, a.g1, a.g2 = one.data_ptr(), h1.ptr, h2.ptr
        _ok(lib.carel_rbf_mmd_bwd(C.byref(a), L.current_stream()), "mmd bwd")
        torch.cuda.synchronize()
        assert ar.intact() and torch.equal(bits(h1.t), bits(g1.t)) and torch.equal(bits(h2.t), bits(g2.t))
    _check("mmd", name, fr)


# ------------------------------------------------------------------------------------------------ pdist
@pytest.mark.parametrize("name", _names(R.PDIST_CASES))
def test_pdist_forward_and_backward(name):
    """pdist_fwd_kernel, pdist_bwd_kernel<0> (grid n1) and <1> (grid n2): one wave per row, lane = feature."""
    c, s1, s2, w, ref, bound = R.pdist_reference(name)
    n1, n2, d = c["n1"], c["n2"], c["d"]
    lib = L.load()
    t1, ld1 = _sample(s1, c.get("strided"), 3, 2)
    t2, ld2 = _sample(s2, c.get("strided"), 0, 40)
    up = _put(w)
    ar = Arena(seed=n1 + n2)
    dist, g1, g2 = ar.nan((n1, n2)), ar.nan((n1, d)), ar.nan((n2, d))
    a = L.PdistArgs()
    a.s1, a.s2, a.ld1, a.ld2 = t1.data_ptr(), t2.data_ptr(), ld1, ld2
    a.n1, a.n2, a.d, a.eps = n1, n2, d, c["eps"]
    a.dist_out, a.grad_dist, a.g1, a.g2 = dist.ptr, up.data_ptr(), g1.ptr, g2.ptr

    def call():
        _ok(lib.carel_pdist_fwd(C.byref(a), L.current_stream()), "pdist fwd")
        _ok(lib.carel_pdist_bwd(C.byref(a), L.current_stream()), "pdist bwd")
    _twice(ar, call)
    got = dict(dist=_np(dist), g1=_np(g1), g2=_np(g2))
    assert all(np.isfinite(v).all() for v in got.values())
    if c.get("far"):
        assert got["dist"].max() > 100.0
    _check("pdist", name, {k: R.frac(got[k], ref[k], bound[k]) for k in ("dist", "g1", "g2")})


# ------------------------------------------------------------------------------------------------ HSIC
@pytest.mark.parametrize("name", _names(R.HSIC_CASES))
def test_hsic_forward_and_backward(name):
    """hsic_kernel: one row per thread up to m = 1024, two above; hipFuncSetAttribute from 64 KB of LDS (m = 300 at d = 24) on."""
    c, x, y, gs, ref, bound = R.hsic_reference(name)
    m, d = c["m"], c["d"]
    lib = L.load()
    tx, ldx = _sample(x, c.get("strided"), 7, 1)
    ty, ldy = _sample(y, c.get("strided"), 0, 9)
    ar = Arena(seed=m)
    out, gx, gy = ar.nan((1,)), ar.nan((m, d)), ar.nan((m, d))
    grad = None if c["gs"] is None else torch.tensor([gs], device="cuda", dtype=torch.float32)
    a = L.HsicArgs()
    a.x, a.y, a.ldx, a.ldy, a.m, a.d, a.s_x, a.s_y = tx.data_ptr(), ty.data_ptr(), ldx, ldy, m, d, c["s"][0], c["s"][1]
    a.hsic_out, a.grad_hsic, a.gx, a.gy = out.ptr, None if grad is None else grad.data_ptr(), gx.ptr, gy.ptr

    def call():
        _ok(lib.carel_hsic_fwd(C.byref(a), L.current_stream()), "hsic fwd")
        _ok(lib.carel_hsic_bwd(C.byref(a), L.current_stream()), "hsic bwd")
    _twice(ar, call)
    got = dict(hsic=_np(out)[0], gx=_np(gx), gy=_np(gy))
    assert all(np.isfinite(v).all() for v in got.values())
    if c["gs"] is None:
        one = torch.ones(1, device="cuda")
        hx, hy = ar.nan((m, d)), ar.nan((m, d))
        a.grad_hsic, a.gx, a.gy = one.data_ptr(), hx.ptr, hy.ptr
        _ok(lib.carel_hsic_bwd(C.byref(a), L.current_stream()), "hsic bwd")
        torch.cuda.synchronize()
        assert ar.intact() and torch.equal(bits(hx.t), bits(gx.t)) and torch.equal(bits(hy.t), bits(gy.t))
    _check("hsic", name, {k: R.frac(got[k], ref[k], bound[k]) for k in ("hsic", "gx", "gy")})


# ------------------------------------------------------------------------------------------------ VI
def _vi_args(z, net, B, D):
    a = L.ViArgs()
    a.z, a.batch, a.ec_dim = z.data_ptr(), B, D
    for i, w in enumerate(net):
        a.net[i] = w.data_ptr()
    return a


@pytest.mark.parametrize("name", _names(R.VI_CASES))
def test_vi_aprx_and_upper(name):
    """vi_kernel<0> and <1>: 256 threads, a sample per thread and trip (B = 257: two trips, 2000: eight); LDS above 64 KB from
    B * D = 2728 on, the largest accepted at (284, 24) and (213, 32)."""
    c, net, z, perms, (aprx, b_aprx), upper = R.vi_reference(name)
    B, D = c["B"], c["D"]
    lib = L.load()
    zt, nt = _put(z), [_put(w) for w in net]
    ar = Arena(seed=B)
    loss = ar.nan((1,))
    grads = [ar.nan(w.shape) for w in net]
    a = _vi_args(zt, nt, B, D)
    a.loss_out = loss.ptr
    for i, g in enumerate(grads):
        a.d_net[i] = g.ptr
    _twice(ar, lambda: _ok(lib.carel_vi_aprx(C.byref(a), L.current_stream()), "vi aprx"))
    fr = dict(aprx_loss=R.frac(_np(loss)[0], aprx["loss"], b_aprx["loss"]),
              aprx_grads=max(R.frac(_np(g), r, b) for g, r, b in zip(grads, aprx["grads"], b_aprx["grads"])))
    assert all(np.isfinite(_np(g)).all() for g in grads)
    for kind in R.PERM_KINDS:
        ref, bound = upper[kind]
        pt = _put(perms[kind])
        ar = Arena(seed=B + 1)
        loss, dz = ar.nan((1,)), ar.nan((B, 2 * D))
        a = _vi_args(zt, nt, B, D)
        a.perm, a.loss_out, a.dz = pt.data_ptr(), loss.ptr, dz.ptr
        _twice(ar, lambda: _ok(lib.carel_vi_upper(C.byref(a), L.current_stream()), "vi upper"))
        got_loss, got_dz = _np(loss)[0], _np(dz)
        assert np.isfinite(got_dz).all()
        if kind == "identity" or B == 1:                 # both residuals are the same number: the bound and d / d e vanish exactly
            assert got_loss == 0.0 and not got_dz[:, :D].any()
        fr["upper_loss_" + kind] = R.frac(got_loss, ref["loss"], bound["loss"])
        fr["upper_dz_" + kind] = R.frac(got_dz, ref["dz"], bound["dz"])
    _check("vi", name, fr)


# ------------------------------------------------------------------------------------------------ refusals: the error, and nothing launched
def _all_nan(ar):
    torch.cuda.synchronize()
    return ar.intact() and all(bool(torch.isnan(b.t).all()) for b in ar.all)


@pytest.mark.parametrize("i", range(len(R.REFUSALS)), ids=["%s-%s" % (op, "-".join("%s" % (v,) for v in a.values())) for op, a, _ in R.REFUSALS])
def test_refused_calls_return_the_error_and_launch_nothing(i):
    """One past each LDS limit, d = 0 and 65, one-row samples, 0 and 9 alphas, non-positive kernel widths.  The inputs are allocated at
    the size the arguments claim, the outputs start as NaN and must all still be NaN."""
    op, p, want = R.REFUSALS[i]
    lib = L.load()
    ar = Arena(seed=i)
    if op == "mmd":
        n1, n2, d = p["n1"], p["n2"], p["d"]
        s1, s2 = torch.ones((n1, max(d, 1)), device="cuda"), torch.ones((n2, max(d, 1)), device="cuda")
        a = _mmd_args(s1, s1.stride(0), s2, s2.stride(0), n1, n2, d, [0.1] * min(p["n_alphas"], 8), 1e-5)
        a.n_alphas = p["n_alphas"]
        out, kern, g1, g2 = ar.nan((1,)), ar.nan(((n1 + n2) ** 2,)), ar.nan((n1, max(d, 1))), ar.nan((n2, max(d, 1)))
        a.mmd_out, a.kernels_out, a.g1, a.g2 = out.ptr, kern.ptr, g1.ptr, g2.ptr
        calls = (lib.carel_rbf_mmd_fwd, lib.carel_rbf_mmd_bwd)
    elif op == "pdist":
        n1, n2, d = p["n1"], p["n2"], p["d"]
        s1, s2 = torch.ones((max(n1, 1), max(d, 1)), device="cuda"), torch.ones((max(n2, 1), max(d, 1)), device="cuda")
        up = torch.ones((max(n1, 1), max(n2, 1)), device="cuda")
        a = L.PdistArgs()
        a.s1, a.s2, a.ld1, a.ld2 = s1.data_ptr(), s2.data_ptr(), s1.stride(0), s2.stride(0)
        a.n1, a.n2, a.d, a.eps = n1, n2, d, 1e-5
        dist, g1, g2 = ar.nan(up.shape), ar.nan(s1.shape), ar.nan(s2.shape)
        a.dist_out, a.grad_dist, a.g1, a.g2 = dist.ptr, up.data_ptr(), g1.ptr, g2.ptr
        calls = (lib.carel_pdist_fwd, lib.carel_pdist_bwd)
    elif op == "hsic":
        m, d = p["m"], p["d"]
        x, y = torch.ones((m, max(d, 1)), device="cuda"), torch.ones((m, max(d, 1)), device="cuda")
        a = L.HsicArgs()
        a.x, a.y, a.ldx, a.ldy, a.m, a.d, a.s_x, a.s_y = x.data_ptr(), y.data_ptr(), x.stride(0), y.stride(0), m, d, p["s"][0], p["s"][1]
        out, gx, gy = ar.nan((1,)), ar.nan(x.shape), ar.nan(x.shape)
        a.hsic_out, a.gx, a.gy = out.ptr, gx.ptr, gy.ptr
        calls = (lib.carel_hsic_fwd, lib.carel_hsic_bwd)
    else:
        B, D = p["B"], p["D"]
        Da = max(D, 1)
        z = torch.ones((max(B, 1), 2 * Da), device="cuda")
        net = [torch.ones(sh, device="cuda") for sh in [(Da, Da), (Da,), (Da, Da), (Da,)] * 2]
        perm = torch.zeros(max(B, 1), dtype=torch.int32, device="cuda")
        a = _vi_args(z, net, B, D)
        loss, dz = ar.nan((1,)), ar.nan(z.shape)
        grads = [ar.nan(w.shape) for w in net]
        a.perm, a.loss_out, a.dz = perm.data_ptr(), loss.ptr, dz.ptr
        for k, g in enumerate(grads):
            a.d_net[k] = g.ptr
        calls = (lib.carel_vi_aprx, lib.carel_vi_upper)
    for fn in calls:
        assert fn(C.byref(a), L.current_stream()) == want
        assert lib.carel_last_error()
    assert _all_nan(ar)


def test_mmdstatistic_refuses_mismatched_widths_and_too_many_alphas():
    """ops._mmd_args: samples of different feature width would let the kernel read past the rows of the narrower one, and a ninth alpha
    overran the ctypes array; both are a CarelError before any launch."""
    import carel_vae_amd as M
    s = torch.ones((8, 24), device="cuda")
    stat = M.MMDStatistic(8, 8)
    with pytest.raises(L.CarelError, match="feature width"):
        stat(s, s[:, :16], [0.1])
    with pytest.raises(L.CarelError, match="feature width"):
        stat(s[:, :16], s, [0.1])
    with pytest.raises(L.CarelError, match="at most 8 alphas"):
        stat(s, s, [0.1] * 9)
    assert float(stat(s, s.clone(), [0.1] * 8)) == float(stat(s, s.clone(), [0.1] * 8))       # eight are accepted
