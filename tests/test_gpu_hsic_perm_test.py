"""carel_hsic_perm_test and carel_hsic_gram through the C ABI, and the public paths on top of them (hsic_permutation_test,
hsic_independence_test, DrlClassifier.latent_independence_test), against the float64 restatements of tests/hsic_perm_restate.py: m at
the edges of the 4-column vector, the 64-row slab, the 256 / 1024-column strides, the group regime (3072 / 3073) and the row limit,
P + 1 at the edges of a group of four permutations, d in 1 / 24 / 64 with d_x != d_y, widths 1 / 4 / 48, a non-symmetric K, strides above
m.  The device's stats must lie within the bound (2 roundings of the magnitude a statistic is made of), its comparison must agree with
float64 on every decided permutation, two runs must give the same bits, and the NaN regions around every output must stay NaN.
Run with -s: every case prints its worst fraction of the bound.

Worst fractions of the bound on an MI355X: stats 0.064 (m3_p2; 0.000 .. 0.036 elsewhere), the Gram matrix 0.534 of the hsic_kern bound of
tests/stats_restate.py (h_64_d1; 0.381 over the cases of this file, 0.294 at m = 8 192); every count inside the float64 interval.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import data as D
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import drl_classifier_en as ME
from carel_vae_amd import ops
from tests import hsic_perm_restate as HR
from tests import stats_restate as R
from tests.gpu_util import bits
from tests.test_gpu_perm_test import NanBuf, _put          # the NaN-sentinel helpers of the two-sample suite

pytestmark = pytest.mark.gpu


class HsicCall:
    """one carel_hsic_perm_test call on NaN outputs of exactly the stated sizes"""

    def __init__(self, Kt, Lt, perms):
        self.Kt, self.Lt, self.perms = Kt, Lt, perms
        m, P = Kt.shape[0], perms.shape[0] - 1
        self.P = P
        self.stats, self.count = NanBuf(P + 1, torch.float64), NanBuf(1, torch.float32)
        nbytes = int(L.load().carel_hsic_perm_workspace_bytes(m, P))
        assert nbytes == HR.workspace_bytes(m, P) > 0
        self.work = NanBuf(nbytes // 8, torch.float64)
        a = L.HsicPermArgs()
        a.k, a.ldk, a.l, a.ldl, a.perms = Kt.data_ptr(), Kt.stride(0), Lt.data_ptr(), Lt.stride(0), perms.data_ptr()
        a.m, a.n_permutations = m, P
        a.stats, a.count, a.workspace, a.workspace_bytes = self.stats.ptr, self.count.ptr, self.work.ptr, nbytes
        self.a = a

    def run(self):
        rc = L.load().carel_hsic_perm_test(C.byref(self.a), L.current_stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        """(stats float64 ndarray, count int) and the guards checked"""
        assert self.stats.guards_nan() and self.count.guards_nan() and self.work.guards_nan()
        return self.stats.t.cpu().numpy().copy(), int(self.count.t.view(torch.int32).cpu()[0])

    def snap(self):
        return [bits(self.stats.t), bits(self.count.t), bits(self.work.t)]

    def refill(self):
        for b in (self.stats, self.count, self.work):
            b.buf.fill_(float("nan"))


def _twice(call):
    """-> (stats, count) of a run; a second run on NaN outputs gives the same bits (the workspace too: it is fully rewritten)"""
    L.check(call.run(), "carel_hsic_perm_test")
    stats, count = call.out()
    snap = call.snap()
    call.refill()
    L.check(call.run(), "carel_hsic_perm_test")
    call.out()
    for a, b in zip(snap, call.snap()):
        assert torch.equal(a, b)
    return stats, count


def _gram(x, s, pad=0, strided=False):
    """carel_hsic_gram on a NaN output of m * (m + pad) floats between NaN guards -> the [m, m] device view; the padding stays NaN"""
    m, d = x.shape
    if strided:
        w = torch.full((m, d + 13), float("nan"), device="cuda")
        w[:, 5:5 + d] = _put(x)
        t = w[:, 5:5 + d]
    else:
        t = _put(x)
    ld = m + pad
    out = NanBuf(m * ld, torch.float32)
    a = L.HsicGramArgs()
    a.x, a.ldx, a.m, a.d, a.s, a.k_out, a.ldk = t.data_ptr(), t.stride(0), m, d, s, out.ptr, ld
    L.check(L.load().carel_hsic_gram(C.byref(a), L.current_stream()), "carel_hsic_gram")
    torch.cuda.synchronize()
    assert out.guards_nan()
    full = out.t.view(m, ld)
    assert pad == 0 or bool(torch.isnan(full[:, m:]).all())
    K = full[:, :m]
    Ki = K.view(torch.int32)                             # bitwise symmetric (compared on the device: 256 MB at the row limit)
    assert torch.equal(Ki, Ki.t()) and torch.equal(K, K.t()) and bool((torch.diagonal(K) == 1.0).all())
    return K


def _gram_frac(K, x, s):
    """the worst fraction of the hsic_kern bound; above HR.BIG rows only the first and the last 70 rows (every column tile) are compared"""
    m = x.shape[0]
    rows = None if m <= HR.BIG else np.concatenate((np.arange(70), np.arange(m - 70, m)))
    ref, bound = HR.gram64(x, s, rows)
    got = (K if rows is None else K[torch.from_numpy(rows).cuda()]).cpu().double().numpy()
    assert np.isfinite(got).all()
    return R.frac(got, ref, bound)


# ------------------------------------------------------------------------------------------------ the Gram matrix
@pytest.mark.parametrize("name", [c["name"] for c in HR.CASES])
def test_gram_against_float64(name):
    c, x, y, _, _, _ = HR.case_inputs(name)
    pad = 5 if c["m"] % 2 else 0
    fx = _gram_frac(_gram(x, c["s"][0], pad=pad, strided=c["dx"] == 24), x, c["s"][0])
    fy = _gram_frac(_gram(y, c["s"][1], pad=pad), y, c["s"][1])
    print("FRAC gram %s x=%.3f y=%.3f" % (name, fx, fy))
    assert fx <= 1.0 and fy <= 1.0


@pytest.mark.parametrize("name", ["h_3", "h_64_d1", "h_40_d64", "h_golden_scale", "h_300"])
def test_gram_on_the_hsic_cases_of_the_operator_sweep(name):
    """the inputs tests/stats_restate.py holds hsic_kern to (widths 0.5 / 2, exp arguments up to 19), the same bound"""
    c, x, y, _, _, _ = R.hsic_reference(name)
    fx, fy = _gram_frac(_gram(x, c["s"][0]), x, c["s"][0]), _gram_frac(_gram(y, c["s"][1], pad=3), y, c["s"][1])
    print("FRAC gram %s x=%.3f y=%.3f" % (name, fx, fy))
    assert fx <= 1.0 and fy <= 1.0


# ------------------------------------------------------------------------------------------------ the statistic
@pytest.mark.parametrize("name", [c["name"] for c in HR.CASES])
def test_case_against_float64(name):
    c, _, _, K, Lm, perms = HR.case_inputs(name)
    stats, count = _twice(HsicCall(_put(K), _put(Lm), _put(perms)))
    fr = HR.judge(stats, count, HR.case_reference(name))
    print("FRAC hsic perm %s stats=%.3f count=%d of %d" % (name, fr, count, c["P"]))


@pytest.mark.parametrize("name", ["m65_p300", "nonsym_m97_p300"])
def test_matrices_inside_wider_ones(name):
    """ldk, ldl > m: each matrix as a block of a NaN-filled wider one"""
    c, _, _, K, Lm, perms = HR.case_inputs(name)
    m = c["m"]
    wk, wl = torch.full((m, m + 11), float("nan"), device="cuda"), torch.full((m, m + 6), float("nan"), device="cuda")
    wk[:, 3:3 + m], wl[:, 5:5 + m] = _put(K), _put(Lm)
    stats, count = _twice(HsicCall(wk[:, 3:3 + m], wl[:, 5:5 + m], _put(perms)))
    HR.judge(stats, count, HR.case_reference(name))
    plain = HsicCall(_put(K), _put(Lm), _put(perms))
    L.check(plain.run(), "hsic perm")
    assert np.array_equal(plain.out()[0].view(np.int64), stats.view(np.int64)) and plain.out()[1] == count


def _magnitude(K, Lm):
    """float64 (Kc, sum |Kc| |L| / (m-1)^2) of float64 matrices, for the bounds of the comparisons below"""
    m = K.shape[0]
    Rs, Cs, T = HR.sums(K)
    Kc = K - Rs[:, None] / m - Cs[None, :] / m + T / (m * m)
    return Kc, float((np.abs(Kc) * np.abs(Lm)).sum()) / (m - 1.0) ** 2


@pytest.mark.parametrize("name", ["h_3", "h_65", "h_300", "h_757_lds_top"])
def test_observed_statistic_against_the_existing_operator(name):
    """m <= 757 (d = 24): stats[0] and ops.hsic(x, y) each lie within their OWN bound of the same float64 value, the HSIC of the
    float32 samples.  The operator's bound is that of tests/stats_restate.py.  stats[0] carries the test's bound on the device's own
    Gram matrices, FACTOR * 2^-24 * magnitude, plus what the errors bK, bL of those matrices (the hsic_kern bound) move it by:
    tr(L H K H) = tr(K H L H), so to first order sum |(H K H)_ij| bL_ij + sum |(H L H)_ij| bK_ij over (m-1)^2 (1 % for the second order)."""
    c, x, y, _, ref, bound = R.hsic_reference(name)
    m = c["m"]
    perms = _put(HR.random_perms(m, 3, 5)[1:])
    hsic, pval, stats, count = M.hsic_independence_test(_put(x), _put(y), c["s"][0], c["s"][1], 3, permutations=perms, return_stats=True)
    K64, bK = HR.gram64(x, c["s"][0])
    L64, bL = HR.gram64(y, c["s"][1])
    Kc, mag = _magnitude(K64, L64)
    Lc, _ = _magnitude(L64, K64)
    own = HR.FACTOR * HR.U * mag + 1.01 * float((np.abs(Kc) * bL).sum() + (np.abs(Lc) * bK).sum()) / (m - 1.0) ** 2
    op = float(ops.hsic(_put(x), _put(y), *c["s"]).item())
    print("HSIC %s test %.9e operator %.9e float64 %.9e bounds %.2e / %.2e" % (name, hsic, op, ref["hsic"], own, bound["hsic"]))
    assert abs(hsic - ref["hsic"]) <= own and abs(op - ref["hsic"]) <= bound["hsic"]
    assert hsic == float(stats[0]) and pval == count / 3


def test_reference_values_of_the_golden_file(golden_dir):
    z = np.load(os.path.join(golden_dir, "statistics.npz"), allow_pickle=False)
    for tag in "ab":
        hsic, pval = M.hsic_independence_test(z[f"h{tag}_x"], torch.from_numpy(z[f"h{tag}_y"]).cuda(), n_permutations=20)
        np.testing.assert_allclose(hsic, float(z[f"h{tag}_hsic"]), rtol=2e-4, atol=1e-7)
        assert isinstance(hsic, float) and isinstance(pval, float) and 0.0 <= pval <= 1.0


# ------------------------------------------------------------------------------------------------ designed inputs
def test_identity_everywhere_ties_bit_for_bit():
    c, _, _, K, Lm, perms = HR.case_inputs("nonsym_m97_p300")
    P = 41
    ident = np.broadcast_to(np.arange(c["m"], dtype=np.int32), (P + 1, c["m"])).copy()
    stats, count = _twice(HsicCall(_put(K), _put(Lm), _put(ident)))
    assert (stats.view(np.int64) == stats.view(np.int64)[0]).all() and count == P
    pval = M.hsic_permutation_test(K, torch.from_numpy(Lm), P, permutations=ident[1:])
    assert isinstance(pval, float) and pval == 1.0


def test_constant_l_every_permutation_ties():
    _, x, _, _, _, _ = HR.case_inputs("m65_p300")
    y = np.broadcast_to(np.float32([0.25, -0.5, 0.125]), (65, 3)).copy()                 # all rows of y equal: L = 1 everywhere
    hsic, pval, stats, count = M.hsic_independence_test(x, y, n_permutations=40, generator=torch.Generator(device="cuda").manual_seed(1),
                                                        return_stats=True)
    b = bits(stats)
    assert bool((b == b[0]).all()) and count == 40 and pval == 1.0
    mag = _magnitude(HR.gram64(x, 1.0)[0], np.ones((65, 65)))[1]
    assert abs(hsic) <= HR.FACTOR * HR.U * mag                      # the sum of H K H is 0 up to the roundings of Kc


def test_y_equal_x_counts_zero():
    """y = x with distinct rows: by Cauchy-Schwarz the observed pairing is the strict maximum"""
    c, x, _, _, _, perms = HR.case_inputs("m65_p300")
    K = _gram(x, 1.0)
    stats, count = _twice(HsicCall(K, K, _put(perms)))
    ref = HR.reference(K.cpu().numpy(), K.cpu().numpy(), perms)
    HR.judge(stats, count, ref)
    assert ref["decided"][1:].all() and count == 0 and stats[0] > stats[1:].max()


def test_copies_of_a_permutation_have_equal_bits_wherever_they_stand():
    c, _, _, K, Lm, perms = HR.case_inputs("nonsym_m97_p300")
    perms = perms.copy()
    at = (1, 3, 4, 5, 7, 8, 150, 299, 300)            # first / last rows, first / last slots of the groups of four, the lone last group
    perms[list(at)] = perms[9]
    stats, count = _twice(HsicCall(_put(K), _put(Lm), _put(perms)))
    HR.judge(stats, count, HR.reference(K, Lm, perms))
    b = stats.view(np.int64)
    assert all(b[p] == b[9] for p in at) and b[9] != b[0] and b[9] != b[10]
    # the one-permutation-per-workgroup regime (m > 3072): rows 1 and 2 alike
    c, _, _, K, Lm, perms = HR.case_inputs("m3073_p2")
    perms = perms.copy()
    perms[2] = perms[1]
    call = HsicCall(_put(K), _put(Lm), _put(perms))
    L.check(call.run(), "hsic perm")
    b = call.out()[0].view(np.int64)
    assert b[1] == b[2] and b[1] != b[0]


def test_permuted_l_observed_equals_l_permuted():
    """without the restatement: stats[p] on (K, L) and stats[0] on (K, L[pi_p][:, pi_p]) agree within the sum of their bounds"""
    c, _, _, K, Lm, perms = HR.case_inputs("m257_p300")
    perms = perms[:6]
    Kt, ident = _put(K), _put(perms[:1].repeat(2, 0))
    call = HsicCall(Kt, _put(Lm), _put(perms))
    L.check(call.run(), "hsic perm")
    stats = call.out()[0]
    Kc = _magnitude(K.astype(np.float64), Lm.astype(np.float64))[0]
    for p in range(1, 6):
        Lp = np.ascontiguousarray(Lm[perms[p]][:, perms[p]])
        one = HsicCall(Kt, _put(Lp), ident)
        L.check(one.run(), "hsic perm")
        s0 = one.out()[0][0]
        bound = HR.FACTOR * HR.U * float((np.abs(Kc) * np.abs(Lp)).sum()) / (c["m"] - 1.0) ** 2
        assert abs(s0 - stats[p]) <= 2 * bound and s0 != 0.0, (p, s0, stats[p], bound)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what,code", HR.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in HR.REFUSALS])
def test_refused_calls_write_nothing(what, code):
    Kt, Lt = torch.rand((16, 16), device="cuda"), torch.rand((16, 16), device="cuda")
    call = HsicCall(Kt, Lt, _put(HR.random_perms(16, 4, 1)))
    L.check(call.run(), "hsic perm")
    call.out()
    before = call.snap()
    call.refill()
    good = (call.a.m, call.a.n_permutations, call.a.ldk, call.a.ldl, call.a.workspace, call.a.workspace_bytes)
    call.a.m, call.a.n_permutations = what.get("m", 16), what.get("P", 4)
    saved = {}
    if "null" in what:
        saved[what["null"]] = getattr(call.a, what["null"])
        setattr(call.a, what["null"], None)
    if what.get("short_workspace"):
        call.a.workspace_bytes -= 1
    if what.get("misaligned_workspace"):
        call.a.workspace += 8
    for k in ("ldk", "ldl"):
        if k in what:
            setattr(call.a, k, what[k])
    assert call.run() == code
    assert call.stats.all_nan() and call.count.all_nan() and call.work.all_nan()
    call.a.m, call.a.n_permutations, call.a.ldk, call.a.ldl, call.a.workspace, call.a.workspace_bytes = good
    for k, v in saved.items():
        setattr(call.a, k, v)
    L.check(call.run(), "hsic perm")                     # the same valid call after the refusal: the bits of the one before it
    call.out()
    for a, b in zip(before, call.snap()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what,code", HR.GRAM_REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in HR.GRAM_REFUSALS])
def test_refused_gram_calls_write_nothing(what, code):
    x = torch.rand((16, 24), device="cuda")
    out = NanBuf(16 * 16, torch.float32)
    a = L.HsicGramArgs()
    a.x, a.ldx, a.m, a.d, a.s, a.k_out, a.ldk = x.data_ptr(), 24, 16, 24, 1.0, out.ptr, 16
    for k, v in what.items():
        setattr(a, k, v)
    assert L.load().carel_hsic_gram(C.byref(a), L.current_stream()) == code
    torch.cuda.synchronize()
    assert out.all_nan()


# ------------------------------------------------------------------------------------------------ the public paths
def test_permutation_test_equals_the_restatement():
    c, _, _, K, Lm, perms = HR.case_inputs("m65_p300")
    P = 200
    ref = HR.reference(K, Lm, perms[:P + 1])
    assert ref["lo"] == ref["hi"]
    for Km, Ll in ((_put(K), _put(Lm)), (torch.from_numpy(K), Lm), (K, _put(Lm))):      # CUDA tensors, CPU tensor / ndarray, mixed
        pval = M.hsic_permutation_test(Km, Ll, P, permutations=torch.from_numpy(perms[1:P + 1]))
        assert isinstance(pval, float) and pval == ref["lo"] / P
    pval, stats, count = M.hsic_permutation_test(K, Lm, P, permutations=_put(perms[1:P + 1]).long(), return_stats=True)
    assert pval == ref["lo"] / P and count == ref["lo"] and stats.dtype == torch.float64 and stats.is_cuda
    HR.judge(stats.cpu().numpy(), count, ref)


def test_bad_permutations_are_refused_before_any_launch(monkeypatch):
    c, x, y, K, Lm, perms = HR.case_inputs("m33_p63")
    calls = []
    real_perm, real_gram = ops.hsic_perm_test, ops.hsic_gram
    monkeypatch.setattr(ops, "hsic_perm_test", lambda *a, **k: calls.append("perm") or real_perm(*a, **k))
    monkeypatch.setattr(ops, "hsic_gram", lambda *a, **k: calls.append("gram") or real_gram(*a, **k))
    repeated = perms[1:].copy()
    repeated[5, 0] = repeated[5, 1]
    out_of_range = perms[1:].copy()
    out_of_range[0, 3] = 33
    for wrong in (repeated, out_of_range, perms[1:-1].copy(), perms[1:, :-1].copy(), perms[1:].astype(np.float32), perms[1:].astype(np.uint8)):
        with pytest.raises(L.CarelError):
            M.hsic_permutation_test(K, Lm, 63, permutations=torch.from_numpy(wrong))
        with pytest.raises(L.CarelError):
            M.hsic_independence_test(x, y, n_permutations=63, permutations=wrong)
    assert calls == []
    assert M.hsic_permutation_test(K, Lm, 63, permutations=perms[1:]) == HR.case_reference("m33_p63")["lo"] / 63 and calls == ["perm"]


def test_seeded_generator_repeats_itself():
    c, x, y, _, _, _ = HR.case_inputs("m129_p1000")
    xt, yt = _put(x), _put(y)
    runs = [M.hsic_independence_test(xt, yt, n_permutations=500, generator=torch.Generator(device="cuda").manual_seed(5), return_stats=True)
            for _ in range(2)]
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][3] == runs[1][3] and torch.equal(bits(runs[0][2]), bits(runs[1][2]))
    other = M.hsic_independence_test(xt, yt, n_permutations=500, generator=torch.Generator(device="cuda").manual_seed(6), return_stats=True)
    assert not torch.equal(bits(other[2]), bits(runs[0][2])) and torch.equal(bits(other[2][:1]), bits(runs[0][2][:1]))
    cpu = [M.hsic_independence_test(x, y, n_permutations=50, generator=torch.Generator().manual_seed(5)) for _ in range(2)]
    assert cpu[0] == cpu[1] and cpu[0][0] == runs[0][0]                                  # a CPU generator draws on the CPU
    pm = M.random_permutations(129, 300, "cuda", torch.Generator(device="cuda").manual_seed(1))
    assert pm.dtype == torch.int32 and tuple(pm.shape) == (301, 129) and pm.is_cuda
    assert torch.equal(torch.sort(pm, dim=1).values.cpu(), torch.arange(129, dtype=torch.int32).expand(301, 129))
    assert torch.equal(pm[0].cpu(), torch.arange(129, dtype=torch.int32)) and len({tuple(r.tolist()) for r in pm.cpu()}) == 301
    assert 0.0 <= runs[0][1] <= 1.0 and runs[0][1] == runs[0][3] / 500


def test_dependent_samples_are_found_dependent_and_independent_ones_are_not():
    c, x, y, _, _, _ = HR.case_inputs("m64_p128")                                        # dep = 1: y = x
    assert M.hsic_independence_test(x, y, 1.0, 4.0, 200, generator=torch.Generator(device="cuda").manual_seed(2))[1] == 0.0
    c, x, y, _, _, _ = HR.case_inputs("m129_p1000")                                      # dep = 0
    assert M.hsic_independence_test(x, y, n_permutations=200, generator=torch.Generator(device="cuda").manual_seed(2))[1] > 0.02


def test_latent_independence_test_on_a_small_model():
    N, S, VOCAB, V, D_ = 130, 32, 600, 64, 24
    m = M.DrlClassifier(M.make_opt(pair_bow_dim=V, ec_dim=D_), M.encoder_config("zh", vocab_size=VOCAB, layers=2), seed=9).to("cuda").eval()
    b = D.synthetic_ecpe_batch(N, S, VOCAB, V, seed=230, shape="B")
    lat = m.pair_latents(*(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids")))
    g = torch.Generator().manual_seed(2)
    noise = (torch.randn(D_, generator=g), torch.randn(D_, generator=g))
    gen = lambda: torch.Generator(device="cuda").manual_seed(4)          # noqa: E731
    hsic, pval, stats, count = m.latent_independence_test(lat, 100, noise=noise, s_e=2.0, s_c=0.5, generator=gen(), return_stats=True)
    assert isinstance(hsic, float) and np.isfinite(hsic) and isinstance(pval, float) and pval == count / 100 and stats.shape == (101,)
    z = ops.sample_latents(lat, noise[0].cuda(), noise[1].cuda(), D_)
    want = M.hsic_independence_test(z[:, :D_], z[:, D_:], 2.0, 0.5, 100, generator=gen(), return_stats=True)
    assert want[0] == hsic and want[1] == pval and want[3] == count and torch.equal(bits(want[2]), bits(stats))
    assert m.latent_independence_test(lat, 100, noise=noise, s_e=2.0, s_c=0.5, generator=gen()) == (hsic, pval)
    assert 0.0 <= m.latent_independence_test(lat, 20)[1] <= 1.0          # noise drawn like a forward call's, permutations from the default generator


def test_three_space_model_refuses_by_name():
    m = ME.DrlClassifier(ME.make_zh_opt(pair_bow_dim=64), M.encoder_config("zh", vocab_size=600, layers=1))
    with pytest.raises(L.CarelError, match="latent_independence_test"):
        m.latent_independence_test(torch.zeros((8, 96), device="cuda"), 10)
    with pytest.raises(L.CarelError, match="pair_latents"):
        m.pair_latents(None, None, None)
