"""The tiled differentiable statistics through the C ABI -- carel_hsic_tiled_fwd/bwd, carel_rbf_mmd_tiled_fwd/bwd (csrc/stat_tiled.hip) --
and the public paths on top of them (ops.hsic / ops.rbf_mmd above the single-workgroup LDS limit, HSIC, MMDStatistic), against the
float64 restatements of tests/stats_restate.py with the chains of tests/stat_tiled_restate.py, in the manner of
tests/test_gpu_stats_sweep.py: every output and the workspace start as NaN between guard regions at exactly the size the header
states, the guards must be intact afterwards, a second identical call must give the same bits, a refused call must leave everything
NaN.  One tile, the tile edge and one past it, 3 x 3 tiles with a last tile of one row; the sample boundary of the MMD inside a tile,
on a tile edge and past it; d = 1 .. 64 (4 / 8 / 16 gradient accumulators); strided rows, NULL upstream gradients, 1 / 3 / 8 alphas,
a duplicate row; every case of the single-workgroup sweep, where both families must lie within their own bound of the same float64
value; m = 800 and n1 = n2 = 800 (above the old limits: HSIC(x, y) and MMDStatistic(800, 800) raised CarelError there before); m =
8192 against the permutation test's statistic and a float64 restatement of the first and last 70 rows.
tests/test_stat_tiled_host.py holds stock torch float32 on the CPU to half of the same bounds.  Run with -s for the worst fractions.

Worst fractions of the bound on an MI355X: DESIGN.md 4.17."""
import ctypes as C

import numpy as np
import pytest
import torch

import carel_vae_amd as M
from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests import stat_tiled_restate as T
from tests import stats_restate as R
from tests.gpu_util import Arena, bits
from tests.test_gpu_stats_sweep import _check, _np, _ok, _put, _refill, _sample, _snapshot, _twice

pytestmark = pytest.mark.gpu


def _names(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------ one call of each family on guarded NaN buffers
class HsicCall:
    def __init__(self, c, x, y, gs, seed=0):
        m, d = c["m"], c["d"]
        self.keep = [_sample(x, c.get("strided"), 7, 1), _sample(y, c.get("strided"), 0, 9)]
        (tx, ldx), (ty, ldy) = self.keep
        self.ar = Arena(seed=m + seed)
        nbytes = int(L.load().carel_hsic_tiled_workspace_bytes(m, d))
        assert nbytes == T.hsic_workspace_bytes(m, d) and nbytes % 4 == 0
        self.out, self.gx, self.gy, self.work = self.ar.nan((1,)), self.ar.nan((m, d)), self.ar.nan((m, d)), self.ar.nan((nbytes // 4,))
        assert self.work.ptr % 8 == 0
        self.grad = None if c["gs"] is None else torch.tensor([gs], device="cuda", dtype=torch.float32)
        a = self.a = L.HsicArgs()
        a.x, a.y, a.ldx, a.ldy, a.m, a.d, a.s_x, a.s_y = tx.data_ptr(), ty.data_ptr(), ldx, ldy, m, d, c["s"][0], c["s"][1]
        a.hsic_out, a.grad_hsic, a.gx, a.gy = self.out.ptr, None if self.grad is None else self.grad.data_ptr(), self.gx.ptr, self.gy.ptr

    def codes(self):
        lib = L.load()
        return (lib.carel_hsic_tiled_fwd(C.byref(self.a), self.work.ptr, L.current_stream()),
                lib.carel_hsic_tiled_bwd(C.byref(self.a), self.work.ptr, L.current_stream()))

    def __call__(self):
        fwd, bwd = self.codes()
        _ok(fwd, "hsic tiled fwd")
        _ok(bwd, "hsic tiled bwd")

    def got(self):
        return dict(hsic=_np(self.out)[0], gx=_np(self.gx), gy=_np(self.gy))


class MmdCall:
    def __init__(self, c, s1, s2, gs, seed=0):
        n1, n2, d = c["n1"], c["n2"], c["d"]
        self.keep = [_sample(s1, c.get("strided"), 5, 8), _sample(s2, c.get("strided"), 26, 0)]
        (t1, ld1), (t2, ld2) = self.keep
        self.ar = Arena(seed=n1 + n2 + seed)
        nbytes = int(L.load().carel_rbf_mmd_tiled_workspace_bytes(n1, n2, d))
        assert nbytes == T.mmd_workspace_bytes(n1, n2, d) and nbytes % 4 == 0
        self.out, self.g1, self.g2, self.work = self.ar.nan((1,)), self.ar.nan((n1, d)), self.ar.nan((n2, d)), self.ar.nan((nbytes // 4,))
        self.kern = self.ar.nan((16,))              # kernels_out is not read by the tiled entries: it stays NaN
        assert self.work.ptr % 8 == 0
        self.grad = None if c["gs"] is None else torch.tensor([gs], device="cuda", dtype=torch.float32)
        a = self.a = L.MmdArgs()
        a.s1, a.s2, a.ld1, a.ld2 = t1.data_ptr(), t2.data_ptr(), ld1, ld2
        a.n1, a.n2, a.d, a.n_alphas, a.eps = n1, n2, d, len(c["alphas"]), c["eps"]
        for i, v in enumerate(c["alphas"]):
            a.alphas[i] = v
        a.mmd_out, a.kernels_out = self.out.ptr, self.kern.ptr
        a.grad_mmd, a.g1, a.g2 = None if self.grad is None else self.grad.data_ptr(), self.g1.ptr, self.g2.ptr

    def codes(self):
        lib = L.load()
        return (lib.carel_rbf_mmd_tiled_fwd(C.byref(self.a), self.work.ptr, L.current_stream()),
                lib.carel_rbf_mmd_tiled_bwd(C.byref(self.a), self.work.ptr, L.current_stream()))

    def __call__(self):
        fwd, bwd = self.codes()
        _ok(fwd, "mmd tiled fwd")
        _ok(bwd, "mmd tiled bwd")

    def got(self):
        assert bool(torch.isnan(self.kern.t).all())
        return dict(mmd=_np(self.out)[0], g1=_np(self.g1), g2=_np(self.g2))


def _finite(got):
    assert all(np.isfinite(v).all() for v in got.values())
    return got


def _null_gradient_is_one(call, outs, field):
    """with the upstream gradient NULL the backward gives the bits of an upstream gradient of 1"""
    first = [bits(o.t) for o in outs]
    one = torch.ones(1, device="cuda")
    setattr(call.a, field, one.data_ptr())
    for o in outs:
        o.t.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    assert call.ar.intact() and all(torch.equal(a, bits(o.t)) for a, o in zip(first, outs))


# ------------------------------------------------------------------------------------------------ the smallest shapes that can go wrong, and one above each old limit
@pytest.mark.parametrize("name", _names(T.HSIC_CASES))
def test_hsic_tiled_forward_and_backward(name):
    """t_800_above_the_lds_limit is refused by carel_hsic_fwd (CAREL_ERR_SHAPE from m = 758 on at d = 24)."""
    c, x, y, gs, ref, bound = T.hsic_reference(name)
    call = HsicCall(c, x, y, gs)
    _twice(call.ar, call)
    got = _finite(call.got())
    if c["gs"] is None:
        _null_gradient_is_one(call, (call.gx, call.gy), "grad_hsic")
    _check("hsic_tiled", name, {k: R.frac(got[k], ref[k], bound[k]) for k in ("hsic", "gx", "gy")})


@pytest.mark.parametrize("name", _names(T.MMD_CASES))
def test_mmd_tiled_forward_and_backward(name):
    """t_800_800_above_the_lds_limit is refused by carel_rbf_mmd_fwd (CAREL_ERR_SHAPE from n1 + n2 = 1573 on at d = 24)."""
    c, s1, s2, gs, ref, bound = T.mmd_reference(name)
    call = MmdCall(c, s1, s2, gs)
    _twice(call.ar, call)
    got = _finite(call.got())
    if c["gs"] is None:
        _null_gradient_is_one(call, (call.g1, call.g2), "grad_mmd")
    if c.get("dup"):                                  # the duplicate pair has d2 = 0 exactly: no gradient between the two rows
        assert np.array_equal(s1[c["dup"][0]], s2[c["dup"][1]])
    _check("mmd_tiled", name, {k: R.frac(got[k], ref[k], bound[k]) for k in ("mmd", "g1", "g2")})


# ------------------------------------------------------------------------------------------------ agreement with the single-workgroup operators
@pytest.mark.parametrize("name", _names(R.HSIC_CASES))
def test_hsic_tiled_agrees_with_the_single_workgroup_operator(name):
    """both within the bound of stats_restate.hsic_closed of the same float64 value (the tiled chains are the shorter ones)"""
    c, x, y, gs, ref, bound = R.hsic_reference(name)
    call = HsicCall(c, x, y, gs)
    call()
    got = _finite(call.got())
    grad = torch.tensor([gs], device="cuda", dtype=torch.float32)
    tx, ty = _put(x), _put(y)
    gx, gy = ops.hsic_backward(tx, ty, grad, *c["s"])
    one = dict(hsic=ops.hsic(tx, ty, *c["s"]).double().cpu().numpy()[0], gx=gx.double().cpu().numpy(), gy=gy.double().cpu().numpy())
    fr = {k: R.frac(got[k], ref[k], bound[k]) for k in ("hsic", "gx", "gy")}
    fr.update({"single_" + k: R.frac(one[k], ref[k], bound[k]) for k in ("hsic", "gx", "gy")})
    assert call.ar.intact()
    _check("hsic_tiled_vs_single", name, fr)


@pytest.mark.parametrize("name", _names(R.MMD_CASES))
def test_mmd_tiled_agrees_with_the_single_workgroup_operator(name):
    """each within its OWN bound of the same float64 value: the gradient of the tiled entries with the chain of the tile plan"""
    c, s1, s2, gs, ref, bound = R.mmd_reference(name)
    tiled_bound = T.mmd_reference(name)[5]
    call = MmdCall(c, s1, s2, gs)
    call()
    got = _finite(call.got())
    grad = torch.tensor([gs], device="cuda", dtype=torch.float32)
    t1, t2 = _put(s1), _put(s2)
    g1, g2 = ops.rbf_mmd_backward(t1, t2, c["alphas"], grad, eps=c["eps"])
    one = dict(mmd=ops.rbf_mmd(t1, t2, c["alphas"], eps=c["eps"])[0].double().cpu().numpy()[0], g1=g1.double().cpu().numpy(),
               g2=g2.double().cpu().numpy())
    fr = {k: R.frac(got[k], ref[k], tiled_bound[k]) for k in ("mmd", "g1", "g2")}
    fr.update({"single_" + k: R.frac(one[k], ref[k], bound[k]) for k in ("mmd", "g1", "g2")})
    assert call.ar.intact()
    _check("mmd_tiled_vs_single", name, fr)


# ------------------------------------------------------------------------------------------------ the row limit
def test_hsic_tiled_at_the_row_limit():
    """m = 8192, d = 24.  The value against the permutation test's observed statistic (other kernels: the stored Gram matrices, centred
    and summed in double), each within its own bound of the float64 value; the first and last 70 rows of both gradients against the
    float64 restatement restricted to those rows (the float64 arithmetic itself runs on the GPU, in row blocks)."""
    c = T.HSIC_TOP
    x, y = T.hsic_top_inputs()
    rows = list(T.TOP_ROWS)
    ref, bound = T.hsic_rows_closed(x, y, *c["s"], c["gs"], rows, device="cuda")
    call = HsicCall(c, x, y, c["gs"])
    _twice(call.ar, call)
    got = _finite(call.got())
    perms = torch.stack([torch.roll(torch.arange(c["m"], dtype=torch.int32), k) for k in (1, 2)]).cuda()
    perm_stat, _ = M.hsic_independence_test(call.keep[0][0], call.keep[1][0], c["s"][0], c["s"][1], 2, permutations=perms)
    fr = dict(hsic=R.frac(got["hsic"], ref["hsic"], bound["hsic"]), perm=R.frac(perm_stat, ref["hsic"], bound["perm"]),
              both=abs(got["hsic"] - perm_stat) / (bound["hsic"] + bound["perm"]),
              gx=R.frac(got["gx"][rows], ref["gx"], bound["gx"]), gy=R.frac(got["gy"][rows], ref["gy"], bound["gy"]))
    print("HSIC m = 8192: tiled %.9e permutation test %.9e float64 %.9e terms %s" % (got["hsic"], perm_stat, ref["hsic"], ref["terms"]))
    _check("hsic_tiled", c["name"], fr)


# ------------------------------------------------------------------------------------------------ refusals on the device: nothing written, nothing left behind
def _all_nan(ar):
    torch.cuda.synchronize()
    return ar.intact() and all(bool(torch.isnan(b.t).all()) for b in ar.all)


def test_refused_calls_write_nothing_and_the_next_valid_call_reproduces_its_bits():
    c, x, y, gs, _, _ = T.hsic_reference("t_65_d16")
    call = HsicCall(c, x, y, gs)
    call()
    torch.cuda.synchronize()
    first = _snapshot(call.ar)
    for field, bad, want in (("m", 1, T.ERR_SHAPE), ("m", 8193, T.ERR_SHAPE), ("d", 0, T.ERR_SHAPE), ("d", 65, T.ERR_SHAPE), ("s_x", 0.0, T.ERR_ARG),
                             ("s_y", -1.0, T.ERR_ARG), ("ldx", 15, T.ERR_ARG)):
        good = getattr(call.a, field)
        setattr(call.a, field, bad)
        _refill(call.ar)
        assert call.codes() == (want, want) and L.load().carel_last_error().startswith(b"carel_hsic_tiled_bwd")
        assert _all_nan(call.ar), field
        setattr(call.a, field, good)
    call()
    torch.cuda.synchronize()
    assert call.ar.intact() and all(torch.equal(a, b) for a, b in zip(first, _snapshot(call.ar)))

    c, s1, s2, gs, _, _ = T.mmd_reference("t_65_64_d17")
    call = MmdCall(c, s1, s2, gs)
    call()
    torch.cuda.synchronize()
    first = _snapshot(call.ar)
    for field, bad, want in (("n1", 1, T.ERR_SHAPE), ("n2", 1, T.ERR_SHAPE), ("n2", 8192, T.ERR_SHAPE), ("d", 0, T.ERR_SHAPE), ("d", 65, T.ERR_SHAPE),
                             ("n_alphas", 0, T.ERR_ARG), ("n_alphas", 9, T.ERR_ARG), ("ld2", 16, T.ERR_ARG)):
        good = getattr(call.a, field)
        setattr(call.a, field, bad)
        _refill(call.ar)
        assert call.codes() == (want, want) and L.load().carel_last_error().startswith(b"carel_rbf_mmd_tiled_bwd")
        assert _all_nan(call.ar), field
        setattr(call.a, field, good)
    call()
    torch.cuda.synchronize()
    assert call.ar.intact() and all(torch.equal(a, b) for a, b in zip(first, _snapshot(call.ar)))


# ------------------------------------------------------------------------------------------------ the autograd surface
def test_hsic_autograd_above_the_old_limit():
    """M.HSIC(x, y) with m = 800 raised CarelError ("too large for one LDS") before the tiled entries existed."""
    c, x, y, _, _, _ = T.hsic_reference(T.HSIC_ABOVE["name"])
    up = -1.75
    ref, bound = T.hsic_closed_tiled(x, y, *c["s"], up)
    tx, ty = _put(x).requires_grad_(True), _put(y).requires_grad_(True)
    h = M.HSIC(tx, ty, *c["s"])
    gx, gy = torch.autograd.grad(h * up, (tx, ty))
    assert tx.grad is None and h.shape == ()
    got = dict(hsic=float(h.detach()), gx=gx.double().cpu().numpy(), gy=gy.double().cpu().numpy())
    _check("HSIC autograd", c["name"], {k: R.frac(got[k], ref[k], bound[k]) for k in ("hsic", "gx", "gy")})
    h2 = M.HSIC(tx, ty, *c["s"])
    h2.backward()
    assert float(h2.detach()) == float(h.detach()) and torch.equal(bits(tx.grad), bits(ops.hsic_tiled_backward(tx.detach(), ty.detach(), None, *c["s"])[0]))


def test_mmdstatistic_autograd_and_matrix_above_the_old_limit():
    """M.MMDStatistic(800, 800)(s1, s2, [0.1]) raised CarelError before; ret_matrix=True returns the matrix of ops.rbf_gram."""
    c, s1, s2, _, _, _ = T.mmd_reference(T.MMD_ABOVE["name"])
    up = 2.5
    ref, bound = T.mmd_closed_tiled(s1, s2, c["alphas"], c["eps"], up)
    t1, t2 = _put(s1).requires_grad_(True), _put(s2).requires_grad_(True)
    stat = M.MMDStatistic(c["n1"], c["n2"])
    mmd, kern = stat(t1, t2, list(c["alphas"]), ret_matrix=True)
    g1, g2 = torch.autograd.grad(mmd * up, (t1, t2))
    assert not kern.requires_grad and torch.equal(bits(kern), bits(ops.rbf_gram(t1.detach(), t2.detach(), list(c["alphas"]))))
    got = dict(mmd=float(mmd.detach()), g1=g1.double().cpu().numpy(), g2=g2.double().cpu().numpy())
    _check("MMDStatistic autograd", c["name"], {k: R.frac(got[k], ref[k], bound[k]) for k in ("mmd", "g1", "g2")})
    again = stat(t1, t2, list(c["alphas"]))
    again.backward()
    assert float(again.detach()) == float(mmd.detach()) and t1.grad.shape == t1.shape and bool(torch.isfinite(t2.grad).all())


class _Counting:
    """the library with every statistic entry point that is looked up written down"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith(("carel_hsic", "carel_rbf")) and not name.endswith("_bytes"):
            self.calls.append(name)
        return getattr(self.lib, name)


def test_below_the_limit_the_single_workgroup_entries_are_still_the_ones_called(monkeypatch):
    lib = _Counting(L.load())
    monkeypatch.setattr(L, "load", lambda: lib)
    c, x, y, _, _, _ = R.hsic_reference("h_757_lds_top")
    tx, ty = _put(x).requires_grad_(True), _put(y).requires_grad_(True)
    M.HSIC(tx, ty, *c["s"]).backward()
    assert lib.calls == ["carel_hsic_fwd", "carel_hsic_bwd"]
    del lib.calls[:]
    c, s1, s2, _, _, _ = R.mmd_reference("g1_700_872_lds_top")
    t1, t2 = _put(s1).requires_grad_(True), _put(s2).requires_grad_(True)
    M.MMDStatistic(c["n1"], c["n2"])(t1, t2, list(c["alphas"])).backward()
    assert lib.calls == ["carel_rbf_mmd_fwd", "carel_rbf_mmd_bwd"]
    del lib.calls[:]
    z = torch.zeros((758, 24), device="cuda").normal_(0.0, 0.15, generator=torch.Generator(device="cuda").manual_seed(3)).requires_grad_(True)
    M.HSIC(z, z.detach() * 0.5).backward()
    assert lib.calls == ["carel_hsic_tiled_fwd", "carel_hsic_tiled_bwd"]
