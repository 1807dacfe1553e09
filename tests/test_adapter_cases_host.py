"""The sentence-adapter sweep's case table (tests/adapter_cases.py) judged without a device, on the references alone: every designed
row has the support it names in float64 and in float32 with every deciding comparison far from its threshold, the dyadic rows are exact
in float32, the table reaches every template instantiation, length, lane-boundary support and batch remainder, no case leaves a sample
out, and float32 torch (the two fmaf chains in the kernels' own order) sits within half of every derived bound."""
import functools

import pytest
import torch

from tests import adapter_cases as AC
from tests import test_gpu_adapter_train as TR

F32, F64 = torch.float32, torch.float64
DESIGNED = AC.designed_cases() + AC.designed_wgrad_cases()
ids = lambda cs: [c["name"] for c in cs]                     # noqa: E731
DROPPED_SAMPLES_CAP = 0


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = next(c for c in DESIGNED if c["name"] == name)
    return c, AC.designed_inputs(c)


def test_names_are_unique_and_cases_are_small():
    cs = AC.all_cases()
    assert len(set(c["name"] for c in cs)) == len(cs)
    for c in cs:
        assert 1 <= c["B"] <= 16 and c["B"] <= c["Bp"] and c["S"] in AC.S_ALL, c["name"]


@pytest.mark.parametrize("c", DESIGNED, ids=ids(DESIGNED))
def test_designed_rows_have_their_support_with_margin_in_both_precisions(c):
    z = _inputs(c["name"])[1]["z"]
    want = torch.tensor(c["ks"]).T                                   # [2, B]
    bar = AC.P_MARGIN if c["mode"] == "sparsemax" else AC.X_MARGIN
    for dtype in (F64, F32):
        k, margin = AC.decisions(z, c["mode"], dtype)
        assert torch.equal(k, want), (c["name"], dtype)
        assert float(margin.min()) >= bar, (c["name"], dtype, float(margin.min()))
        p = AC.normalise(z, c["mode"], dtype)
        assert torch.equal((p > 0).sum(-1), want)
        assert float((p.sum(-1) - 1).abs().max()) <= (1e-12 if dtype == F64 else 2e-6)
    # the two adapters of a sample differ, and the float32 restatement stays within 6e-8 of float64
    assert all(a != b for a, b in c["ks"])
    assert float((AC.normalise(z, c["mode"], F32).double() - AC.normalise(z, c["mode"])).abs().max()) <= 6e-8


def test_dyadic_rows_are_bit_equal_between_float32_and_float64():
    cs = [c for c in DESIGNED if c["rows"] == "dyadic"]
    assert sorted(c["S"] for c in cs) == list(AC.S_ALL)
    for c in cs:
        z = _inputs(c["name"])[1]["z"]
        assert all(k & (k - 1) == 0 for pair in c["ks"] for k in pair)
        p64, p32 = AC.normalise(z, "sparsemax"), AC.normalise(z, "sparsemax", F32)
        assert torch.equal(p32.double(), p64), c["name"]
        assert torch.equal(p64.float().double(), p64)                # representable: the kernel can be held to the bits


def test_the_table_covers_every_instantiation_length_boundary_and_remainder():
    cs = AC.all_cases()
    raw = [c for c in cs if c["kind"] == "raw"]
    assert {2 * c["G"] for c in cs} == set(AC.NV_ALL)
    for S in (64, 128):
        assert {c["G"] for c in raw if c["S"] == S} == set(AC.HEADS)
    assert {c["G"] for c in raw if c["wgrad"]} == set(AC.HEADS)
    for mode in ("raw", "sparsemax", "entmax"):
        assert {c["S"] for c in cs if c["mode"] == mode} == set(AC.S_ALL), mode
    untested = [G for G in (2, 3, 6, 8) if {c["S"] for c in raw if c["G"] == G} == set(AC.S_ALL)]
    assert untested
    for mode in ("sparsemax", "entmax"):
        for rows in ("spaced", "tied"):
            for S in (96, 128):
                ks = {k for c in cs if c["mode"] == mode and c["S"] == S and c["rows"] == rows for pair in c["ks"] for k in pair}
                assert {63, 64, 65, S - 1, S} <= ks, (mode, rows, S)
        for S in AC.S_ALL:
            ks = {k for c in cs if c["mode"] == mode and c["S"] == S for pair in c["ks"] for k in pair}
            assert set(AC.supports(S)) <= ks
        assert any(c["mode"] == mode and c["B"] == 1 for c in cs)
        assert any(c["mode"] == mode and c["wgrad"] for c in cs)
    # gemv walks the samples four at a time, gemvT_part eight: every remainder class that B <= 9 can show, padded and not
    one = [c for c in raw if c["G"] == 6 and c["S"] == 32]
    assert {c["B"] for c in one} == {1, 3, 4, 5, 8, 9}
    assert {c["B"] % 4 for c in one} == {0, 1, 3} and {c["B"] % 8 for c in one} >= {0, 1, 3, 4, 5}
    for B in (1, 3, 4, 5, 8, 9):
        assert {c["Bp"] - c["B"] for c in one if c["B"] == B} == {0, 3}
    assert {c["kscale"] for c in raw} == {1.0, 40.0} and {c["Bp"] - c["B"] for c in raw} == {0, 3}
    assert all(c["Bp"] == c["B"] + 3 for c in cs if c["kind"] == "designed")
    # the tied, constant and dominant samples of _inputs() are present wherever B allows
    assert all(c["B"] >= 4 for c in raw if c["name"].startswith("raw_G") and "_B" not in c["name"])


def test_no_sample_is_ever_left_out():
    """Designed rows keep every decision away from its threshold (asserted above), raw mode has no threshold: the sweep has no keep
    mask at all, and the table carries nothing that could ask for one."""
    for c in AC.all_cases():
        assert "keep" not in c and "drop" not in c
    assert DROPPED_SAMPLES_CAP == 0


@pytest.mark.parametrize("c", DESIGNED, ids=ids(DESIGNED))
def test_torch_fp32_within_half_of_every_bound(c):
    """The float32 restatement (torch on the CPU, the reference alone; combine_chain32 / dx_chain32 for the two fmaf chains) against
    float64, per bound of tests/adapter_cases.py."""
    c, d = _inputs(c["name"])
    mode, S, z, Hs, d_out = c["mode"], c["S"], d["z"], d["Hs"], d["d_out"]
    worst = {}

    def hold(name, got, ref, bound):
        fr = ((got.double() - ref).abs() / bound.clamp(min=1e-300))
        fr = torch.where((bound == 0) & (got.double() == ref), torch.zeros_like(fr), fr)
        worst[name] = float(fr.max())

    p32 = AC.normalise(z, mode, F32)
    hold("p", p32, AC.normalise(z, mode), AC.p_bound(z, mode))
    # every later stage on the float32 p, as the sweep judges the kernels on theirs
    p = p32.double()
    ref, scale = AC.combine_ref(p, Hs)
    hold("out", AC.combine_chain32(p32, Hs), ref, AC.combine_bound(S, scale))
    dp, dscale = AC.dp_ref(Hs, d_out)
    dp32 = AC.dp_ref(Hs.float(), d_out.float())[0]
    hold("dp", dp32, dp, AC.dp_bound(dscale))
    hold("dz", AC.normalise_backward(p32, dp32, mode), AC.normalise_backward(p, dp, mode), AC.dz_bound(p, dp, AC.dp_bound(dscale), mode))
    ref, bound = AC.dx_cols_ref(p, d_out)
    hold("dx", AC.dx_chain32(p32, d_out), ref, bound)
    print("HOST %s: %s" % (c["name"], "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 0.5, (c["name"], worst)


def test_built_u_is_the_unit_vector_up_to_one_rounding():
    """carel_adapter_build_u from designed_weights(): e_side (1 +- 2^-23), far inside the margins of rows whose values are below 17."""
    for side in range(2):
        u = AC.built_u32(side).double()
        assert float((u[side] - 1).abs()) <= 2.0 ** -23 and float(u.abs().sum() - u[side].abs()) == 0.0
        assert (AC.OFFSET + AC.DROP) * 2.0 ** -22 < AC.P_MARGIN / 100


WG = [c for c in AC.all_cases() if c["wgrad"]]


@pytest.mark.parametrize("c", WG, ids=ids(WG))
def test_weight_gradient_cases_carry_signal_and_float32_sits_within_half(c):
    d = AC.designed_wgrad_inputs(c) if c["kind"] == "designed" else AC.raw_inputs(c)
    bounds, ref, e32 = AC.wgrad_bounds(c["mode"], c["G"], d)
    assert TR.conditioned(ref, d["d_out"]), c["name"]
    for k, e in e32.items():
        assert e <= bounds[k] / 2, (c["name"], k, e)
    if c["kind"] == "designed":                  # the float64 reference sees the designed supports
        for side in range(2):
            w = d["ws"][side]
            sc = (d["Hs"] @ w["k_proj.weight"].T) @ w["q_proj.bias"] / AC.math.sqrt(AC.H)
            assert [int(k) for k in (AC.normalise(sc, c["mode"]) > 0).sum(-1)] == [pair[side] for pair in c["ks"]]
            sc32 = d["Hs"][:, :, side].float() * AC.built_u32(side)[side]          # what the kernels' rowdot sees
            assert [int(k) for k in (AC.normalise(sc32, c["mode"], F32) > 0).sum(-1)] == [pair[side] for pair in c["ks"]]


RAWS = AC.raw_cases()


@pytest.mark.parametrize("c", [c for c in RAWS if c["S"] == 32], ids=ids([c for c in RAWS if c["S"] == 32]))
def test_raw_bounds_are_per_sample_and_keep_float32_within_half(c):
    d = AC.raw_inputs(c)
    (b_out, b_dx), (e_out, e_dx) = AC.raw_bounds(c, d)
    assert b_out.shape == (2, c["B"]) and b_dx.shape == (c["B"],)
    assert bool((e_out <= b_out / 2).all()) and bool((e_dx <= b_dx / 2).all())
    assert bool((b_out >= AC.OUT_BOUND).all()) and bool((b_dx >= AC.DX_BOUND).all())
