"""The sentence adapters (csrc/adapter.hip) through the C ABI against float64, at designed supports and at the edges of their
dispatch: every length 32 / 64 / 96 / 128, supports on both sides of the lane / +64 boundary of wave_normalise (63, 64, 65), S - 1 and S,
tie blocks, every AD_NV_SWITCH instantiation (raw heads 1, 2, 3, 4, 6, 8, 12), the batch remainders of the 4- and 8-sample trips, padded
and unpadded batches.  The table, the layout of x that makes each kernel observable, the references and the derivation of every bound are
in tests/adapter_cases.py; tests/test_adapter_cases_host.py judges them without a device.

Every case: x, u, out, d_out, dx and both workspaces in guarded buffers (tests.gpu_util.Arena); the filler samples of x, and out, dx and
the workspaces, NaN before the call; afterwards the guards are intact, out and every row of dx are finite, the filler rows of dx are
exactly zero, and a second launch gives the same bits.  No sample is left out of any check.

Designed cases (sparsemax / entmax-1.5, u = unit vectors): {p > 0} equals the float64 support exactly and p is exactly zero off it;
the dyadic rows equal float64 bit for bit; every other p, the weighted sums, dz (read from dx[:, 0:2]; exactly zero off the support)
and the p * d_out columns are held element by element to their kernel's own bound.  Raw cases: out and dx per sample.  Weight
gradients: per destination, repeat and accumulate bit rules, on designed cases (u built by carel_adapter_build_u) and every raw head
count.

Worst fraction of each bound, float32 torch on the CPU | the kernels on an MI355X:
  designed   p sparsemax 0.323 | 0.323   p entmax 0.245 | 0.245   out 0.307 | 0.307   dx (p d_out) 0.482 | 0.482
             dz sparsemax 0.016 | 0.011   dz entmax 0.018 | 0.017   (dp alone, CPU: 0.035 of its 18 u bound)
  raw        per sample, of max(fixed, 4 x float32 torch): out 0.25 | 0.916   dx 0.25 | 0.184   (the CPU figure is 1/4 at most by construction)
  weights    of max(1e-4, 4 x float32 torch): 0.25 | 0.487
The dyadic rows equalled float64 bit for bit, and p, out and the p d_out columns of every designed case reproduce the figures of the
float32 chains written out in tests/adapter_cases.py to three digits: the kernels round where the derivation says they do.

Faults this sweep found, fixed with it:
  * softmax backward (adapter_dzdh_kernel, adapter_wgrad_dz_kernel), raw_G1_S64_k40: with one head and kscale 40 four of the emotion
    side's five softmax rows are one-hot to 1 - p_max = 6e-10 .. 4e-3, and dz = p (dp - sum p dp), evaluated as written, lost the
    dominant token to the rounding of sum p: d_q_w, d_q_b and d_k_w were 1.74e-4 off float64 where float32 torch is 2.9e-5 off and the
    rule allows 1.15e-4.  (In float64 on the case's inputs, rounding p alone to float32 moves du by 2.5e-5; the expression in plain
    float32 torch is 4.0e-4 off.)  The kernels now shift dp by its value at the largest p, dz = p ((dp - c) - sum p (dp - c)): the
    dominant term of the sum is an exact zero.  Measured after: 1.84e-5 on that case; F32_LIMITED of
    tests/test_gpu_adapter_train.py, 8.2e-4 before, 6.4e-7.  Raw-mode dx and q / k gradients change in their last bits; sparsemax and
    entmax are untouched.
  * preconditions the kernels rely on that nothing checked, now refused before any launch (test_refusals; never run): u, work, x, out,
    d_out, dx, query or a weight matrix that is not 16-byte aligned (every kernel moves them as float4), and batch_padded > 65535 (the
    sample index is a grid y coordinate).
"""
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests import adapter_cases as AC
from tests import test_gpu_adapter as A
from tests import test_gpu_adapter_train as TR
from tests.gpu_util import Arena, bits

pytestmark = pytest.mark.gpu
H = AC.H
WORST = {}                   # {bound name: (fraction, case)} over the run; test_report prints it
DESIGNED, DESIGNED_WG, RAW = AC.designed_cases(), AC.designed_wgrad_cases(), AC.raw_cases()
ids = lambda cs: [c["name"] for c in cs]                     # noqa: E731


def _record(name, case, got, ref, bound):
    """Hold got to ref element by element; -> the worst fraction of the bound (recorded, printed by test_report)."""
    err = (got.double().cpu() - ref).abs()
    fr = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    f = float(fr.max())
    if name not in WORST or f > WORST[name][0]:
        WORST[name] = (f, case)
    print("SWEEP %s %s: %.3f of the bound" % (case, name, f))
    return f


class _Buf:
    """What ops.adapter_args / adapter_wgrad_args expect of ops.AdapterBuffers, in guarded NaN-filled storage."""

    def __init__(self, ar, B, S, G, wgrad):
        lib = L.load()
        self.B, self.S, self.heads = B, S, G
        self.g_out, self.g_d_out = ar.nan((2, B, H)), ar.nan((2, B, H))
        self.g_work = ar.nan((lib.carel_adapter_workspace_floats(B, S, G),))
        self.out, self.d_out, self.work = self.g_out.t, self.g_d_out.t, self.g_work.t
        self.wgrad_work = ar.nan((lib.carel_adapter_wgrad_workspace_floats(B, G),)).t if wgrad else None


class Run:
    """One case on the device."""

    def __init__(self, c, d, mode_weights=None, u=None):
        """d: the case's inputs (CPU).  u: a float64 [2, G, 768] to pass as it is, or None to build it from the weights."""
        self.c = c
        B, Bp, S, G = c["B"], c["Bp"], c["S"], c["G"]
        ar = self.arena = Arena(seed=11)
        x = torch.full((Bp * S, H), float("nan"))
        x[:B * S] = d["Hs"].reshape(B * S, H).float()
        self.x, self.dx = ar.put(x), ar.nan((Bp * S, H))
        self.buf = _Buf(ar, B, S, G, c["wgrad"])
        self.u = ar.nan((2, G, H)) if u is None else ar.put(u.float())
        self.build = u is None
        ws = mode_weights or [dict(q_w=None, q_b=None, k_w=None) for _ in range(2)]
        qd = [q.float().cuda().contiguous() for q in d["qs"]] if "qs" in d else [torch.zeros(H, device="cuda") for _ in range(2)]
        self.a = ops.adapter_args(c["mode"], G, qd, ws, self.u.t, self.buf, Bp, x=self.x.t, dx=self.dx.t)
        self.d_out = d["d_out"].float().cuda()

    def launch(self):
        self.buf.out.fill_(float("nan"))
        self.dx.t.fill_(float("nan"))
        self.buf.work.fill_(float("nan"))
        if self.build:
            ops.adapter_build_u(self.a)
        ops.adapter_forward(self.a)
        self.buf.d_out.copy_(self.d_out)
        ops.adapter_backward(self.a)
        torch.cuda.synchronize()
        return self.buf.out.clone(), self.dx.t.clone()

    def every_case(self):
        """-> (out [2, B, 768], dx [B, S, 768]) on the CPU as float64, after the checks every case gets."""
        c = self.c
        B, S = c["B"], c["S"]
        out, dx = self.launch()
        out2, dx2 = self.launch()
        assert self.arena.intact(), "guard bytes overwritten"
        assert bool(torch.isfinite(out).all()), "out not fully written"
        assert bool(torch.isfinite(dx).all()), "a row of dx was not written"
        assert bool((dx[B * S:] == 0).all()), "filler samples must be exactly zero"
        assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(dx), bits(dx2)), "repeat launch not bitwise identical"
        return out.double().cpu(), dx[:B * S].view(B, S, H).double().cpu()


@pytest.mark.parametrize("c", DESIGNED, ids=ids(DESIGNED))
def test_designed_supports(c):
    d = AC.designed_inputs(c)
    mode, S, z, Hs, d_out = c["mode"], c["S"], d["z"], d["Hs"], d["d_out"]
    out, dx = Run(c, d, u=d["u"]).every_case()
    # ---- forward: p is out[:, :, 2 : 2 + S] bit for bit
    p = out[:, :, 2:2 + S]
    ref = AC.normalise(z, mode)
    assert torch.equal(p > 0, ref > 0), "support differs from float64"
    assert [tuple(int(k) for k in pair) for pair in (p > 0).sum(-1).T] == [tuple(pair) for pair in c["ks"]]
    assert bool((p[ref == 0] == 0).all()), "p must be exactly zero off the support"
    if c["rows"] == "dyadic":
        assert torch.equal(p, ref), "dyadic rows: p must equal float64 bit for bit"
    fr = [_record("p/" + mode, c["name"], p, ref, AC.p_bound(z, mode))]
    want, scale = AC.combine_ref(p, Hs)                               # the weighted sums, on the kernel's own p
    fr.append(_record("out", c["name"], out, want, AC.combine_bound(S, scale)))
    # ---- backward: dz is dx[:, :, 0:2] bit for bit
    dz = dx[:, :, 0:2].permute(2, 0, 1)
    assert bool((dz[p == 0] == 0).all()), "dz must be exactly zero off the support"
    dp, dscale = AC.dp_ref(Hs, d_out)
    fr.append(_record("dz/" + mode, c["name"], dz, AC.normalise_backward(p, dp, mode), AC.dz_bound(p, dp, AC.dp_bound(dscale), mode)))
    want, bound = AC.dx_cols_ref(p, d_out)
    fr.append(_record("dx", c["name"], dx[:, :, 2:], want[:, :, 2:], bound[:, :, 2:]))
    assert max(fr) <= 1.0, fr


def _device_weights(c, d):
    return [A._kernel_weights(w, c["mode"]) for w in d["ws"]]


def _weight_gradients(c, d, run):
    """carel_adapter_backward_weights after run's forward / backward: per destination against float64 autograd, repeat and accumulate."""
    bounds, ref, _ = AC.wgrad_bounds(c["mode"], c["G"], d)
    assert TR.conditioned(ref, d["d_out"])
    out0, dx0 = run.buf.out.clone(), run.dx.t.clone()
    dests = TR._dests()
    ops.adapter_backward_weights(run.a, ops.adapter_wgrad_args(run.buf, dests))
    first = TR._snapshot(dests)
    ops.adapter_backward_weights(run.a, ops.adapter_wgrad_args(run.buf, dests))
    second = TR._snapshot(dests)
    ops.adapter_backward_weights(run.a, ops.adapter_wgrad_args(run.buf, dests, accumulate=True))
    torch.cuda.synchronize()
    assert run.arena.intact()
    assert torch.equal(bits(run.buf.out), bits(out0)) and torch.equal(bits(run.dx.t), bits(dx0)), "the call must leave out and dx alone"
    written = TR.DESTS if c["mode"] == "raw" else TR.DESTS[:4]
    worst, missed = 0.0, []
    for side in range(2):
        for k in TR.DESTS:
            f, s, acc = first[side][k], second[side][k], dests[side][k]
            if k not in written:
                assert bool(torch.isnan(f).all()) and bool(torch.isnan(acc).all()), k
                continue
            assert bool(torch.isfinite(f).all()), k
            assert torch.equal(f, s), "repeat call not bitwise identical: " + k
            assert torch.equal(acc, f + f), "accumulate = 1 must give first + first: " + k
            if k == "d_k_b":
                assert float(f.abs().max()) == 0.0
                continue
            e, bound = A.relnorm(f, ref[side][k]), bounds.get((side, k), AC.WGRAD_BOUND)
            print("SWEEP %s side %d %s: %.3g (bound %.3g)" % (c["name"], side, k, e, bound))
            worst = max(worst, e / bound)
            if e > bound:
                missed.append((side, k, e, bound))
    if "wgrad" not in WORST or worst > WORST["wgrad"][0]:
        WORST["wgrad"] = (worst, c["name"])
    assert not missed, (c["name"], missed)


@pytest.mark.parametrize("c", DESIGNED_WG, ids=ids(DESIGNED_WG))
def test_designed_weight_gradients(c):
    d = AC.designed_wgrad_inputs(c)
    run = Run(c, d, mode_weights=_device_weights(c, d))
    out, dx = run.every_case()
    for side in range(2):                                            # build_u gave the unit vector up to one rounding
        u = run.u.t[side, 0].double().cpu()
        assert abs(float(u[side]) - 1.0) <= 2.0 ** -23 and float(u.abs().sum() - u[side].abs()) == 0.0
    p = out[:, :, 2:2 + c["S"]]                                      # the one-hot columns still show p bit for bit
    assert [tuple(int(k) for k in pair) for pair in (p > 0).sum(-1).T] == [tuple(pair) for pair in c["ks"]]
    _weight_gradients(c, d, run)


@pytest.mark.parametrize("c", RAW, ids=ids(RAW))
def test_raw_heads_and_batches(c):
    d = AC.raw_inputs(c)
    run = Run(c, d, mode_weights=_device_weights(c, d))
    out, dx = run.every_case()
    ref = AC.raw_reference(c, d)
    (b_out, b_dx), _ = AC.raw_bounds(c, d, ref)
    e_out, e_dx = AC.sample_err(out, ref[0], (-1,)), AC.sample_err(dx, ref[1], (-2, -1))
    for name, e, b in (("raw out", e_out, b_out), ("raw dx", e_dx, b_dx)):
        f = float((e / b).max())
        if name not in WORST or f > WORST[name][0]:
            WORST[name] = (f, c["name"])
        print("SWEEP %s %s per sample: worst %.3g, %.3f of its bound" % (c["name"], name, float(e.max()), f))
        assert bool((e <= b).all()), (c["name"], name, e, b)
    if c["wgrad"]:
        _weight_gradients(c, d, run)


# ------------------------------------------------------------------------------------------------ refusals
def _valid(mode, G=1, B=2, Bp=3, S=32):
    ar = Arena(seed=3)
    g = torch.Generator().manual_seed(0)
    kind = "raw" if mode == "raw" else "entmax"
    ws = [A._kernel_weights(A._weights(kind, g, 1.0), kind) for _ in range(2)]
    qd = [torch.randn(H, generator=g).cuda() for _ in range(2)]
    buf = _Buf(ar, B, S, G, True)
    x, dx, u = ar.put(torch.randn(Bp * S, H, generator=g)), ar.nan((Bp * S, H)), ar.nan((2, G, H))
    mk = lambda: ops.adapter_args(mode, G, qd, ws, u.t, buf, Bp, x=x.t, dx=dx.t)      # noqa: E731
    return ar, buf, mk, [buf.g_out, buf.g_work, dx, u, buf.g_d_out]


def _all_nan(bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b.t).all()) for b in bufs)


CALLS = {"build_u": ops.adapter_build_u, "forward": ops.adapter_forward, "backward": ops.adapter_backward}
EVERY = ("build_u", "forward", "backward", "weights")


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _null(field, i=None):
    def f(a):
        if i is None:
            setattr(a, field, None)
        else:
            getattr(a, field)[i] = None
    return f


def _shift(field):
    def f(a):
        setattr(a, field, getattr(a, field) + 4)
    return f


REFUSALS = [("seq_len_%d" % s, "entmax", _set(seq_len=s), EVERY, "seq_len") for s in (0, 16, 48, 160)]
REFUSALS += [("heads_%d" % g, "raw", _set(heads=g), EVERY, "heads") for g in (0, 5, 13, 16)]
REFUSALS += [("mode_%d" % m, "entmax", _set(mode=m), EVERY, "mode") for m in (-1, 3)]
REFUSALS += [("sparse_heads_4", "sparsemax", _set(heads=4), EVERY, "heads = 1"),
             ("batch_0", "entmax", _set(batch=0), EVERY, "batch"),
             ("padded_below_batch", "entmax", _set(batch_padded=1), EVERY, "batch"),
             ("padded_above_grid", "entmax", _set(batch_padded=65536), EVERY, "65535"),
             ("null_u", "entmax", _null("u"), EVERY, "null u"),
             ("null_work", "entmax", _null("work"), EVERY, "null u"),
             ("null_x", "entmax", _null("x_f32"), ("forward", "backward", "weights"), "null x"),
             ("null_out", "entmax", _null("out_f32"), ("forward",), "null x / out"),
             ("null_d_out", "entmax", _null("d_out_f32"), ("backward",), "d_out"),
             ("null_dx", "entmax", _null("dx_f32"), ("backward",), "dx"),
             ("raw_null_v_w", "raw", _null("v_w", 1), ("forward", "backward"), "raw mode needs"),
             ("raw_null_v_b", "raw", _null("v_b", 0), ("forward",), "raw mode needs"),
             ("raw_null_o_w", "raw", _null("o_w", 0), ("forward", "backward"), "raw mode needs"),
             ("raw_null_o_b", "raw", _null("o_b", 1), ("forward",), "raw mode needs"),
             ("raw_null_d_out_weights", "raw", _null("d_out_f32"), ("weights",), "d_out")]
REFUSALS += [("misaligned_" + f, "entmax", _shift(f), EVERY, "16-byte") for f in ("u", "work", "x_f32", "out_f32", "d_out_f32", "dx_f32")]


@pytest.mark.parametrize("name,mode,spoil,calls,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, mode, spoil, calls, match):
    """Each call that ad_check and the entry points do not admit returns its error and touches nothing; the next valid call succeeds."""
    G = 4 if mode == "raw" else 1
    ar, buf, mk, nans = _valid(mode, G)
    dests = TR._dests()
    for call in calls:
        a = mk()
        spoil(a)
        with pytest.raises(L.CarelError, match=match):
            if call == "weights":
                ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests))
            else:
                CALLS[call](a)
        assert _all_nan(nans) and all(bool(torch.isnan(v).all()) for dd in dests for v in dd.values()), (name, call)
    assert ar.intact()
    a = mk()
    ops.adapter_build_u(a)
    ops.adapter_forward(a)
    buf.d_out.fill_(0.5)
    ops.adapter_backward(a)
    ops.adapter_backward_weights(a, ops.adapter_wgrad_args(buf, dests))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf.out).all()) and bool(torch.isfinite(nans[2].t).all()) and ar.intact()


def test_report():
    """The worst fraction of every bound over the run (the figures in the module docstring)."""
    for k in sorted(WORST):
        print("SWEEP WORST %-14s %.3f  (%s)" % (k, WORST[k][0], WORST[k][1]))
    assert WORST                                                     # each figure is asserted where it is measured
