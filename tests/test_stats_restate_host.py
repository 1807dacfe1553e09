"""tests/stats_restate.py on the CPU: the two float64 forms agree, the input conditions hold on every case of the GPU sweep, stock
torch float32 stays within half of every bound (the measurement the bounds rest on), and the LDS limits follow from the formulas.
No GPU.  Run with -s for the worst fraction of each quantity."""
import numpy as np
import pytest
import torch

from tests import stats_restate as R

AGREE = 1e-12


def _close(a, b, scale=None):
    """|a - b| <= 1e-12 * max|b| (or `scale`: the magnitude a scalar is the difference of)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = float(np.abs(b).max()) if scale is None else scale
    return float(np.abs(a - b).max()) <= AGREE * s if a.size else True


mmd_ref, pdist_ref, hsic_ref, vi_ref = R.mmd_reference, R.pdist_reference, R.hsic_reference, R.vi_reference


def _names(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------ 1. the two float64 forms agree
@pytest.mark.parametrize("name", _names(R.MMD_CASES))
def test_mmd_forms_agree(name):
    c, s1, s2, gs, ref, _ = mmd_ref(name)
    lit = R.mmd_literal(s1, s2, c["alphas"], c["eps"], gs)
    n1, n2 = c["n1"], c["n2"]
    k = ref["kern"]
    off = k.sum() - np.trace(k)
    scale = 2.0 * k[:n1, n1:].sum() / (n1 * n2) + (k[:n1, :n1].sum() - np.trace(k[:n1, :n1])) / (n1 * (n1 - 1)) + (k[n1:, n1:].sum() - np.trace(k[n1:, n1:])) / (n2 * (n2 - 1))
    assert off > 0 and _close(lit["mmd"], ref["mmd"], scale)
    assert _close(lit["kern"], ref["kern"])
    assert _close(lit["g1"], ref["g1"]) and _close(lit["g2"], ref["g2"])
    assert np.abs(ref["g1"]).max() > 0 and np.abs(ref["g2"]).max() > 0


@pytest.mark.parametrize("name", _names(R.PDIST_CASES))
def test_pdist_forms_agree(name):
    c, s1, s2, w, ref, _ = pdist_ref(name)
    lit = R.pdist_literal(s1, s2, c["eps"], w)
    if c.get("dup"):                                   # float64 rounding of a d2 that is 0 in exact arithmetic, under sqrt(eps + .)
        assert abs(lit["dist"][0, 0] - ref["dist"][0, 0]) <= 1e-9
        lit["dist"][0, 0] = ref["dist"][0, 0]
    assert _close(lit["dist"], ref["dist"])
    assert _close(lit["g1"], ref["g1"], max(np.abs(ref["g1"]).max(), 1e-300)) and _close(lit["g2"], ref["g2"], max(np.abs(ref["g2"]).max(), 1e-300))


@pytest.mark.parametrize("name", _names(R.HSIC_CASES))
def test_hsic_forms_agree(name):
    c, x, y, gs, ref, _ = hsic_ref(name)
    for form in (R.hsic_formula, R.hsic_three_sum_formula):
        lit = R.hsic_literal(x, y, *c["s"], gs, form=form)
        assert _close(lit["hsic"], ref["hsic"], sum(ref["terms"]))
        assert _close(lit["gx"], ref["gx"]) and _close(lit["gy"], ref["gy"])
    assert np.abs(ref["gx"]).max() > 0 and np.abs(ref["gy"]).max() > 0


@pytest.mark.parametrize("name", _names(R.VI_CASES))
def test_vi_forms_agree(name):
    c, net, z, perms, (aprx, _), upper = vi_ref(name)
    lit = R.vi_aprx_literal(net, z)
    assert _close(lit["loss"], aprx["loss"])
    for a, b in zip(lit["grads"], aprx["grads"]):
        assert a.shape == b.shape and _close(a, b, max(np.abs(b).max(), 1e-300))
    for kind, p in perms.items():
        ref, _ = upper[kind]
        lit = R.vi_upper_literal(net, z, p)
        assert _close(lit["loss"], ref["loss"], ref["terms"])
        assert _close(lit["dz"], ref["dz"], max(np.abs(ref["dz"]).max(), 1e-300))
        if kind == "identity" or c["B"] == 1:
            assert ref["loss"] == 0.0 and not ref["dz"][:, :c["D"]].any()


# ------------------------------------------------------------------------------------------------ 2. the input conditions, nothing left out
def _sign_margin(a, b=None, allow=None):
    """the smallest d2 / (2^-24 S) over the pairs of distinct rows (`allow`: the one planted coincident pair, which must be exactly equal)"""
    d2, S = R.pair_terms(a.astype(np.float64), None if b is None else b.astype(np.float64))
    ratio = d2 / (R.U * S)
    if b is None:
        np.fill_diagonal(ratio, np.inf)
    if allow is not None:
        i, j = allow
        assert np.array_equal(a[i], (a if b is None else b)[j])
        ratio[i, j] = np.inf
        if b is None:
            ratio[j, i] = np.inf
    return float(ratio.min())


def test_every_case_meets_its_input_conditions():
    for c in R.MMD_CASES:
        s1, s2 = R.mmd_inputs(c)
        assert s1.shape == (c["n1"], c["d"]) and s2.shape == (c["n2"], c["d"]) and s1.dtype == s2.dtype == np.float32
        z = np.concatenate((s1, s2), 0)
        allow = (c["dup"][0], c["n1"] + c["dup"][1]) if c.get("dup") else None
        assert _sign_margin(z, allow=allow) >= R.SIGN_MARGIN, c["name"]
        d2, _ = R.pair_terms(z.astype(np.float64))
        arg = max(R.f32_scalars(c["alphas"])) * (R.f32_scalars([c["eps"]])[0] + np.abs(d2).max())
        assert 1.0 <= arg <= 20.0, (c["name"], arg)
        assert R.mmd_lds_floats(c["n1"] + c["n2"], c["d"]) <= R.LDS_FLOATS
    for c in R.PDIST_CASES:
        s1, s2, w = R.pdist_inputs(c)
        assert _sign_margin(s1, s2, allow=(0, 0) if c.get("dup") else None) >= R.SIGN_MARGIN, c["name"]
        assert not c.get("dup") or w[0, 0] == 0.0
    for c in R.HSIC_CASES:
        x, y = R.hsic_inputs(c)
        assert x.shape == y.shape == (c["m"], c["d"])
        args = [R.pair_terms(t.astype(np.float64))[0] / s for t, s in zip((x, y), c["s"])]
        assert all(a.min() >= 0.0 and a.max() <= 20.0 for a in args), c["name"]
        if c["std"] == 0.15 and c["m"] >= 17:                        # the regime the sweep is about: kernel mass off the diagonal
            off = np.exp(-args[0])[~np.eye(c["m"], dtype=bool)]
            assert 0.05 <= np.median(off) <= 0.95, (c["name"], float(np.median(off)))
        assert R.hsic_lds_floats(c["m"], c["d"]) <= R.LDS_FLOATS
    for c in R.VI_CASES:
        net, z = R.vi_inputs(c)
        assert float(R.vi_hidden_margin(net, z).min()) >= R.RELU_MARGIN, c["name"]
        assert R.vi_lds_floats(c["B"], c["D"]) <= R.LDS_FLOATS
        ident, fixed, rnd = R.vi_perm(c, "identity"), R.vi_perm(c, "fixed"), R.vi_perm(c, "random")
        for p in (ident, fixed, rnd):
            assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(c["B"]))
        assert np.array_equal(ident, np.arange(c["B"]))
        if c["B"] >= 200:
            nfix = int((fixed == np.arange(c["B"])).sum())
            assert c["B"] // 3 <= nfix < c["B"] - 10 and int((rnd == np.arange(c["B"])).sum()) < 10


def test_plain_draws_would_fail_the_conditions():
    """why the builders do more than draw: d = 1 normal draws leave sign(d2) undecided, plain VI draws leave pre-activations at 0"""
    rs = np.random.RandomState(0)
    assert _sign_margin(rs.randn(129, 1).astype(np.float32)) < R.SIGN_MARGIN
    worst = []
    for B, D in ((257, 24), (300, 16)):
        c = R.by_name(R.VI_CASES, "v_%d_%d" % (B, D))
        rs = np.random.RandomState(c["seed"])
        bound = 1.0 / np.sqrt(D)
        net = [rs.uniform(-bound, bound, size=sh).astype(np.float32) for sh in [(D, D), (D,), (D, D), (D,)] * 2]
        z = (rs.standard_normal((B, 2 * D)) * 0.8).astype(np.float32)
        worst.append(float(R.vi_hidden_margin(net, z).min()))
    assert min(worst) < R.RELU_MARGIN, worst


def test_cases_reach_the_forms_they_name():
    for c in R.MMD_CASES:
        n = c["n1"] + c["n2"]
        assert c["name"].startswith("g%d_" % R.mmd_bwd_group(n)), c["name"]
    assert R.mmd_bwd_row_trips(1024) == 1 and R.mmd_bwd_row_trips(1100) == 2 and R.mmd_bwd_row_trips(1572) == 2
    assert [R.mmd_bwd_group(n) for n in (128, 129, 512, 513)] == [8, 2, 2, 1]
    have = {(R.mmd_bwd_group(c["n1"] + c["n2"]), c["d"]) for c in R.MMD_CASES}
    assert {(8, 1), (8, 2), (8, 63), (8, 64), (2, 1), (2, 63), (1, 2), (1, 64)} <= have
    assert {len(c["alphas"]) for c in R.MMD_CASES} == {1, 3, 8} and {c["eps"] for c in R.MMD_CASES} == {0.0, 1e-5, 1e-2}
    assert any(R.hsic_lds_floats(c["m"], c["d"]) * 4 > 65536 for c in R.HSIC_CASES) and any(c["m"] > 1024 for c in R.HSIC_CASES)
    assert sum(c["corr"] for c in R.HSIC_CASES) * 2 == len(R.HSIC_CASES)
    assert any(R.vi_lds_floats(c["B"], c["D"]) * 4 > 65536 for c in R.VI_CASES)


# ------------------------------------------------------------------------------------------------ 3. torch float32 within half of every bound
def _report(tag, worst):
    print("torch float32, worst fraction of the bound, %s: " % tag + ", ".join("%s %.3f" % kv for kv in worst.items()))
    assert all(v <= 0.5 for v in worst.values()), (tag, worst)


def _upd(worst, key, v):
    worst[key] = max(worst.get(key, 0.0), v)


def test_torch_fp32_within_half_of_every_bound_mmd():
    worst = {}
    for c in R.MMD_CASES:
        _, s1, s2, gs, ref, b = mmd_ref(c["name"])
        got = R.mmd_literal(s1, s2, c["alphas"], c["eps"], gs, dtype=torch.float32)
        for k in ("mmd", "g1", "g2") + (("kern",) if c.get("kern") else ()):      # kern: where the sweep compares the matrix
            _upd(worst, k, R.frac(got[k], ref[k], b[k]))
    _report("MMD", worst)


def test_torch_fp32_within_half_of_every_bound_pdist():
    worst = {}
    for c in R.PDIST_CASES:
        _, s1, s2, w, ref, b = pdist_ref(c["name"])
        got = R.pdist_literal(s1, s2, c["eps"], w, dtype=torch.float32)
        _upd(worst, "dist", R.frac(got["dist"], ref["dist"], b["dist"]))
        for k, partners in (("g1", c["n2"]), ("g2", c["n1"])):              # one partner: the operands form (tests/stats_restate.py)
            if partners == 1:
                _upd(worst, "g (operands)", R.frac(got[k], ref[k], b[k + "_operands"]))
            else:
                _upd(worst, k, R.frac(got[k], ref[k], b[k]))
    _report("pdist", worst)


def test_torch_fp32_within_half_of_every_bound_hsic():
    for tag, form in (("matrix form", R.hsic_formula), ("three sums", R.hsic_three_sum_formula)):
        worst = {}
        for c in R.HSIC_CASES:
            _, x, y, gs, ref, b = hsic_ref(c["name"])
            got = R.hsic_literal(x, y, *c["s"], gs, dtype=torch.float32, form=form)
            _upd(worst, "hsic", R.frac(got["hsic"], ref["hsic"], b["hsic"]))
            for k in ("gx", "gy"):                                          # the goldens' scale: the operands form
                if c["std"] != 0.15:
                    _upd(worst, "g (operands)", R.frac(got[k], ref[k], b[k + "_operands"]))
                else:
                    _upd(worst, k, R.frac(got[k], ref[k], b[k]))
        _report("HSIC " + tag, worst)


def test_torch_fp32_within_half_of_every_bound_vi():
    worst = {}
    for c in R.VI_CASES:
        _, net, z, perms, (aprx, b_aprx), upper = vi_ref(c["name"])
        got = R.vi_aprx_literal(net, z, dtype=torch.float32)
        _upd(worst, "aprx loss", R.frac(got["loss"], aprx["loss"], b_aprx["loss"]))
        for g, r, b in zip(got["grads"], aprx["grads"], b_aprx["grads"]):
            _upd(worst, "aprx grads", R.frac(g, r, b))
        for kind, p in perms.items():
            ref, b = upper[kind]
            got = R.vi_upper_literal(net, z, p, dtype=torch.float32)
            _upd(worst, "upper loss", R.frac(got["loss"], ref["loss"], b["loss"]))
            _upd(worst, "upper dz", R.frac(got["dz"], ref["dz"], b["dz"]))
    _report("VI", worst)


# ------------------------------------------------------------------------------------------------ 4. the LDS limits
def test_lds_limits_follow_from_the_formulas():
    assert R.LDS_FLOATS == 40960
    assert R.largest_accepted(R.mmd_lds_floats, 24) == 1572 and R.largest_accepted(R.mmd_lds_floats, 64) == 619
    assert R.largest_accepted(R.hsic_lds_floats, 24) == 757 and R.largest_accepted(R.hsic_lds_floats, 16) == 1076
    assert R.largest_accepted(R.vi_lds_floats, 24) == 284 and R.largest_accepted(R.vi_lds_floats, 32) == 213
    for fn, n, d in ((R.mmd_lds_floats, 1572, 24), (R.mmd_lds_floats, 619, 64), (R.hsic_lds_floats, 757, 24), (R.hsic_lds_floats, 1076, 16),
                     (R.vi_lds_floats, 284, 24), (R.vi_lds_floats, 213, 32)):
        assert fn(n, d) <= R.LDS_FLOATS < fn(n + 1, d)
    # the sweep's top cases sit on the limit and its refusals one past it
    tops = {(c["n1"] + c["n2"], c["d"]) for c in R.MMD_CASES}
    assert (1572, 24) in tops and (619, 64) in tops
    assert {(757, 24), (1076, 16)} <= {(c["m"], c["d"]) for c in R.HSIC_CASES}
    assert {(284, 24), (213, 32)} <= {(c["B"], c["D"]) for c in R.VI_CASES}
    past = {(op, tuple(sorted(a.items()))) for op, a, _ in R.REFUSALS}
    assert ("mmd", tuple(sorted(dict(n1=700, n2=873, d=24, n_alphas=1).items()))) in past
    for m, d in ((758, 24), (1077, 16)):
        assert any(op == "hsic" and a["m"] == m and a["d"] == d for op, a, _ in R.REFUSALS)
    for B, D in ((285, 24), (214, 32)):
        assert any(op == "vi" and a["B"] == B and a["D"] == D for op, a, _ in R.REFUSALS)
