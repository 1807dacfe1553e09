"""carel_mmd_perm_test, carel_rbf_gram and carel_sample_latents through the C ABI, and the public paths on top of them
(permutation_test_mat, MMDStatistic.pval, mmd_two_sample_test, DrlClassifier.latent_two_sample_test), against the float64 restatements
of tests/perm_restate.py: n at the edges of the 32-row tile and of the 32-partner chunk, P + 1 at the edges of a wave's 32 and a
workgroup's 128 labellings, unequal sides, n_1 = 2, a non-symmetric matrix, 1 / 3 / 8 alphas through the Gram kernel.  The device's
stats must lie within the bound (33 roundings of the magnitudes a statistic is made of), its comparison must agree with float64 on
every decided labelling, two runs must give the same bits, and the NaN regions around every output must stay NaN.
Run with -s: every case prints its worst fraction of the bound.

Worst fractions of the bound on an MI355X: stats 0.015 (n32_p32; 0.001 .. 0.011 elsewhere), the Gram matrix 0.283 of the kernel bound of
tests/stats_restate.py (g8_d1; 0.268 at the corners of n = 8 192); every count inside the float64 interval.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import data as D
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import ops
from tests import perm_restate as PR
from tests import stats_restate as R
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

PAD = 4096          # NaN elements before and after every output


class NanBuf:
    """`count` elements of `dtype` (float32 / float64) between two regions of PAD NaNs, all NaN to begin with"""

    def __init__(self, count, dtype):
        self.count = int(count)
        self.buf = torch.full((2 * PAD + self.count,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + self.count]
        self.ptr = self.t.data_ptr() if self.count else self.buf.data_ptr() + PAD * self.buf.element_size()

    def guards_nan(self):
        return bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.count:]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


def _put(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class PermCall:
    """one carel_mmd_perm_test call on NaN outputs of exactly the stated sizes"""

    def __init__(self, Mt, labels, n1, n2, coef, ldm=None):
        self.Mt, self.labels = Mt, labels
        n, P = n1 + n2, labels.shape[0] - 1
        self.P = P
        self.stats, self.count = NanBuf(P + 1, torch.float64), NanBuf(1, torch.float32)
        nbytes = int(L.load().carel_mmd_perm_workspace_bytes(n, P))
        assert nbytes == PR.workspace_bytes(n, P) > 0
        self.work = NanBuf(nbytes // 8, torch.float64)
        a = L.MmdPermArgs()
        a.matrix, a.ldm, a.labels = Mt.data_ptr(), Mt.stride(0) if ldm is None else ldm, labels.data_ptr()
        a.n1, a.n2, a.n_permutations = n1, n2, P
        a.a00, a.a01, a.a11 = coef
        a.stats, a.count, a.workspace, a.workspace_bytes = self.stats.ptr, self.count.ptr, self.work.ptr, nbytes
        self.a = a

    def run(self):
        rc = L.load().carel_mmd_perm_test(C.byref(self.a), L.current_stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        """(stats float64 ndarray, count int) and the guards checked"""
        assert self.stats.guards_nan() and self.count.guards_nan() and self.work.guards_nan()
        return self.stats.t.cpu().numpy().copy(), int(self.count.t.view(torch.int32).cpu()[0])

    def refill(self):
        for b in (self.stats, self.count, self.work):
            b.buf.fill_(float("nan"))


def _twice(call):
    """-> (stats, count) of a run; a second run on NaN outputs gives the same bits (the workspace too)"""
    L.check(call.run(), "carel_mmd_perm_test")
    stats, count = call.out()
    snap = [bits(call.stats.t), bits(call.count.t), bits(call.work.t)]
    call.refill()
    L.check(call.run(), "carel_mmd_perm_test")
    call.out()
    for a, b in zip(snap, [bits(call.stats.t), bits(call.count.t), bits(call.work.t)]):
        assert torch.equal(a, b)
    return stats, count


def _gram(s1, s2, alphas, eps, strided=False):
    """carel_rbf_gram on a NaN output of n * n floats between NaN guards -> the [n, n] device view"""
    n1, n2, d = s1.shape[0], s2.shape[0], s1.shape[1]
    n = n1 + n2
    if strided:
        w1, w2 = torch.full((n1, d + 13), float("nan"), device="cuda"), torch.full((n2, d + 26), float("nan"), device="cuda")
        w1[:, 5:5 + d], w2[:, 26:] = _put(s1), _put(s2)
        t1, t2 = w1[:, 5:5 + d], w2[:, 26:]
    else:
        t1, t2 = _put(s1), _put(s2)
    out = NanBuf(n * n, torch.float32)
    a = L.MmdArgs()
    a.s1, a.s2, a.ld1, a.ld2 = t1.data_ptr(), t2.data_ptr(), t1.stride(0), t2.stride(0)
    a.n1, a.n2, a.d, a.n_alphas, a.eps = n1, n2, d, len(alphas), eps
    for i, v in enumerate(alphas):
        a.alphas[i] = v
    a.kernels_out = out.ptr
    L.check(L.load().carel_rbf_gram(C.byref(a), L.current_stream()), "carel_rbf_gram")
    torch.cuda.synchronize()
    assert out.guards_nan()
    K = out.t.view(n, n)
    assert torch.equal(bits(K), bits(K.t()))
    return K


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", [c["name"] for c in PR.CASES])
def test_case_against_float64(name):
    c, s1, s2, M_host, labels, coef = PR.case_inputs(name)
    if c["kind"] == "gram":          # the matrix comes from carel_rbf_gram; the reference is float64 on exactly that matrix
        Mt = _gram(s1, s2, c["alphas"], c["eps"], strided=len(c["alphas"]) == 3)
        kref, kb = R.mmd_closed(s1, s2, c["alphas"], c["eps"], 1.0)
        fk = R.frac(Mt.cpu().double().numpy(), kref["kern"], kb["kern"])
        print("FRAC gram %s kern=%.3f" % (name, fk))
        assert fk <= 1.0
        ref = PR.reference(Mt.cpu().numpy(), labels, coef)
        assert int((~ref["decided"])[1:].sum()) <= PR.MAX_UNDECIDED * c["P"]
    else:
        Mt, ref = _put(M_host), PR.case_reference(name)
    stats, count = _twice(PermCall(Mt, _put(labels), c["n1"], c["n2"], coef))
    fr = PR.judge(stats, count, ref)
    print("FRAC perm %s stats=%.3f count=%d of %d (float64 %d..%d)" % (name, fr, count, c["P"], ref["lo"], ref["hi"]))


def test_matrix_inside_a_wider_one():
    """ldm > n: the matrix as a block of a NaN-filled wider one"""
    c, _, _, M_host, labels, coef = PR.case_inputs("n65_p128")
    n = M_host.shape[0]
    wide = torch.full((n, n + 11), float("nan"), device="cuda")
    wide[:, 3:3 + n] = _put(M_host)
    call = PermCall(wide[:, 3:3 + n], _put(labels), c["n1"], c["n2"], coef)
    stats, count = _twice(call)
    PR.judge(stats, count, PR.case_reference("n65_p128"))
    plain = PermCall(_put(M_host), _put(labels), c["n1"], c["n2"], coef)
    L.check(plain.run(), "perm")
    assert np.array_equal(plain.out()[0].view(np.int64), stats.view(np.int64))


# ------------------------------------------------------------------------------------------------ designed inputs
def test_nan_on_the_diagonal_changes_no_bit():
    c, _, _, M_host, labels, coef = PR.case_inputs("nonsym_n97_p300")
    a = PermCall(_put(M_host), _put(labels), c["n1"], c["n2"], coef)
    L.check(a.run(), "perm")
    Mn = M_host.copy()
    np.fill_diagonal(Mn, np.nan)
    b = PermCall(_put(Mn), _put(labels), c["n1"], c["n2"], coef)
    L.check(b.run(), "perm")
    (sa, ca), (sb, cb) = a.out(), b.out()
    assert np.isfinite(sb).all() and np.array_equal(sa.view(np.int64), sb.view(np.int64)) and ca == cb


def test_constant_matrix_every_labelling_ties():
    n1, n2, P = 5, 7, 40
    Mc = np.full((n1 + n2, n1 + n2), 0.5, np.float32)
    np.fill_diagonal(Mc, 123.0)
    labels = PR.random_labels(n1, n2, P, 77)
    call = PermCall(_put(Mc), _put(labels), n1, n2, PR.mmd_coefficients(n1, n2))
    L.check(call.run(), "perm")
    stats, count = call.out()
    assert (stats.view(np.int64) == stats.view(np.int64)[0]).all() and count == P
    assert abs(stats[0]) <= 1e-15                                            # 0.5 * (1 + 1 - 2) up to the coefficients' rounding
    pval = M.MMDStatistic(n1, n2).pval(torch.from_numpy(Mc), P, labels=torch.from_numpy(labels[1:]))
    assert isinstance(pval, float) and pval == 1.0


def test_two_far_apart_clusters_count_zero():
    rs = np.random.RandomState(5)
    n1, n2, P = 40, 41, 200
    s1 = (0.3 * rs.randn(n1, 24)).astype(np.float32)
    s2 = (0.3 * rs.randn(n2, 24) + 2.0).astype(np.float32)
    K = _gram(s1, s2, R.A1, 1e-5)
    labels = PR.random_labels(n1, n2, P, 78)
    coef = PR.mmd_coefficients(n1, n2)
    stats, count = _twice(PermCall(K, _put(labels), n1, n2, coef))
    ref = PR.reference(K.cpu().numpy(), labels, coef)
    PR.judge(stats, count, ref)
    assert ref["decided"][1:].all() and count == 0 and stats[0] > stats[1:].max()


def test_copies_of_a_labelling_have_equal_bits_wherever_they_stand():
    c, _, _, M_host, labels, coef = PR.case_inputs("nonsym_n97_p300")
    labels = labels.copy()
    at_g0, at_x = (1, 31, 32, 33, 127, 128, 129, 255, 300), (2, 64, 130, 299)        # first / last columns of waves and workgroups
    labels[list(at_g0)] = labels[0]
    labels[list(at_x)] = labels[7]
    stats, count = _twice(PermCall(_put(M_host), _put(labels), c["n1"], c["n2"], coef))
    ref = PR.reference(M_host, labels, coef)
    PR.judge(stats, count, ref)
    b = stats.view(np.int64)
    assert all(b[p] == b[0] for p in at_g0) and all(b[p] == b[7] for p in at_x) and b[7] != b[0]
    assert count >= len(at_g0) and count == int((stats[1:] >= stats[0]).sum())   # every copy of g_0 is counted (>=)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what,code", PR.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in PR.REFUSALS])
def test_refused_calls_write_nothing(what, code):
    n1, n2, P = what.get("n1", 8), what.get("n2", 8), what.get("P", 4)
    Mt = torch.rand((16, 16), device="cuda")
    labels = _put(PR.random_labels(8, 8, 4, 1))
    call = PermCall(Mt, labels, 8, 8, (1.0, 0.0, 1.0))
    call.a.n1, call.a.n2, call.a.n_permutations = n1, n2, P
    if "null" in what:
        setattr(call.a, what["null"], None)
    if what.get("short_workspace"):
        call.a.workspace_bytes -= 1
    if "ldm" in what:
        call.a.ldm = what["ldm"]
    assert call.run() == code
    assert call.stats.all_nan() and call.count.all_nan() and call.work.all_nan()


# ------------------------------------------------------------------------------------------------ the Gram matrix
@pytest.mark.parametrize("name", ["g8_2_2", "g8_126_2", "g8_d1", "g8_d2", "g8_d63", "g8_d64", "g8_strided", "g8_duplicate", "g2_65_64",
                                  "g1_257_256_matrix"])
def test_gram_against_float64(name):
    """the MMD cases of tests/stats_restate.py (n = 4 .. 513: inside one 64-tile, at its edge, nine by nine tiles), the same bound"""
    c, s1, s2, _, ref, bound = R.mmd_reference(name)
    K = _gram(s1, s2, c["alphas"], c["eps"], strided=bool(c.get("strided")))
    fk = R.frac(K.cpu().double().numpy(), ref["kern"], bound["kern"])
    print("FRAC gram %s kern=%.3f" % (name, fk))
    assert fk <= 1.0


def test_gram_at_the_row_limit():
    """n = 8 192: bitwise symmetric, and its four corner blocks against float64 (an element depends on its two rows only)"""
    rs = np.random.RandomState(11)
    n1, n2, d = 4000, 4192, 8
    s1, s2 = (0.7 * rs.randn(n1, d)).astype(np.float32), (0.7 * rs.randn(n2, d)).astype(np.float32)
    K = ops.rbf_gram(_put(s1), _put(s2), list(R.A3), 1e-5)
    assert K.shape == (n1 + n2, n1 + n2) and torch.equal(K, K.t().contiguous())
    ref, bound = R.mmd_closed(s1[:64], s2[-64:], R.A3, 1e-5, 1.0)
    idx = torch.cat((torch.arange(64), torch.arange(n1 + n2 - 64, n1 + n2))).cuda()
    got = K[idx][:, idx].cpu().double().numpy()
    fk = R.frac(got, ref["kern"], bound["kern"])
    print("FRAC gram n8192 corners kern=%.3f" % fk)
    assert np.isfinite(got).all() and fk <= 1.0
    with pytest.raises(L.CarelError):
        ops.rbf_gram(_put(s1), torch.zeros((4193, d), device="cuda"), list(R.A3))


# ------------------------------------------------------------------------------------------------ the public paths
def test_pval_equals_the_restatement():
    """MMDStatistic.pval returned None before carel_mmd_perm_test existed"""
    c, _, _, M_host, labels, coef = PR.case_inputs("nonsym_n97_p300")
    P = 200
    ref = PR.reference(M_host, labels[:P + 1], coef)
    assert ref["lo"] == ref["hi"]
    stat = M.MMDStatistic(c["n1"], c["n2"])
    for matrix in (_put(M_host), torch.from_numpy(M_host), M_host):           # CUDA tensor, CPU tensor, ndarray
        pval = stat.pval(matrix, P, labels=torch.from_numpy(labels[1:P + 1]))
        assert isinstance(pval, float) and pval == ref["lo"] / P
    pval, stats, count = M.permutation_test_mat(M_host, c["n1"], c["n2"], P, *(coef[0], coef[1], coef[2]), labels=_put(labels[1:P + 1]),
                                                return_stats=True)
    assert pval == ref["lo"] / P and count == ref["lo"] and stats.dtype == torch.float64 and stats.is_cuda
    PR.judge(stats.cpu().numpy(), count, ref)
    bad = labels[1:P + 1].copy()
    bad[3, np.nonzero(bad[3] == 0)[0][0]] = 1                                 # one row with n_2 + 1 ones
    for wrong in (bad, labels[1:P].copy(), labels[1:P + 1].astype(np.int32)):
        with pytest.raises(L.CarelError):
            stat.pval(M_host, P, labels=torch.from_numpy(wrong))


def test_seeded_generator_repeats_itself():
    c, _, _, M_host, _, coef = PR.case_inputs("n129_p1000")
    stat, Kt = M.MMDStatistic(c["n1"], c["n2"]), _put(M_host)
    runs = [stat.pval(Kt, 500, generator=torch.Generator(device="cuda").manual_seed(5), return_stats=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    other = stat.pval(Kt, 500, generator=torch.Generator(device="cuda").manual_seed(6), return_stats=True)
    assert not torch.equal(bits(other[1]), bits(runs[0][1])) and torch.equal(bits(other[1][:1]), bits(runs[0][1][:1]))
    cpu = [stat.pval(Kt, 50, generator=torch.Generator().manual_seed(5)) for _ in range(2)]      # a CPU generator draws on the CPU
    assert cpu[0] == cpu[1]
    lab = M.random_labellings(c["n1"], c["n2"], 300, "cuda", torch.Generator(device="cuda").manual_seed(1))
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (301, 129) and bool((lab.sum(1) == c["n2"]).all()) and int(lab.max()) == 1
    assert torch.equal(lab[0].cpu(), torch.from_numpy(PR.observed(c["n1"], c["n2"]))) and len({bytes(r.tolist()) for r in lab.cpu()}) > 290
    # the statistic of the null: the p-value of like samples is not extreme
    assert 0.02 < runs[0][0] <= 1.0


def test_two_sample_test_agrees_with_the_mmd_operator():
    c, s1, s2, _, ref, bound = R.mmd_reference("g2_256_256_equal")
    t1, t2 = _put(s1), _put(s2)
    gen = torch.Generator(device="cuda").manual_seed(3)
    mmd, pval, stats, count = M.mmd_two_sample_test(t1, t2, c["alphas"], 100, eps=c["eps"], generator=gen, return_stats=True)
    call = float(M.MMDStatistic(256, 256)(t1, t2, c["alphas"]))
    print("MMD two-sample %.9e operator %.9e float64 %.9e bound %.2e" % (mmd, call, ref["mmd"], bound["mmd"]))
    assert isinstance(mmd, float) and isinstance(pval, float) and 0.0 <= pval <= 1.0 and pval == count / 100
    assert abs(mmd - ref["mmd"]) <= bound["mmd"] and abs(call - ref["mmd"]) <= bound["mmd"]
    assert M.mmd_two_sample_test(s1, s2, c["alphas"], 100, eps=c["eps"], generator=torch.Generator(device="cuda").manual_seed(3)) == (mmd, pval)


def test_latent_two_sample_test_on_a_small_model():
    N, S, VOCAB, V, D_ = 130, 32, 600, 64, 24
    m = M.DrlClassifier(M.make_opt(pair_bow_dim=V, ec_dim=D_), M.encoder_config("zh", vocab_size=VOCAB, layers=2), seed=9).to("cuda").eval()
    b = D.synthetic_ecpe_batch(N, S, VOCAB, V, seed=230, shape="B")
    lat = m.pair_latents(*(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids")))
    g = torch.Generator().manual_seed(2)
    noise = (torch.randn(D_, generator=g), torch.randn(D_, generator=g))
    res = [m.latent_two_sample_test(lat, 100, noise=noise, generator=torch.Generator(device="cuda").manual_seed(4), return_stats=True)
           for _ in range(2)]
    mmd, pval, stats, count = res[0]
    assert isinstance(mmd, float) and np.isfinite(mmd) and isinstance(pval, float) and pval == count / 100 and stats.shape == (101,)
    assert res[1][0] == mmd and res[1][1] == pval and torch.equal(bits(res[1][2]), bits(stats))
    # the samples are draw 0's: mu + eps * exp(log_var) per side, and the observed statistic is the MMD operator's on them
    z = ops.sample_latents(lat, noise[0].cuda(), noise[1].cuda(), D_)
    l64 = lat.double().cpu()
    want = torch.cat((l64[:, :D_] + noise[0].double() * l64[:, D_:2 * D_].exp(), l64[:, 2 * D_:3 * D_] + noise[1].double() * l64[:, 3 * D_:].exp()), 1)
    assert float((z.double().cpu() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max() + 1.0)
    ze, zc = z[:, :D_].cpu().numpy(), z[:, D_:].cpu().numpy()
    ref, bound = R.mmd_closed(ze, zc, ops.MODEL_MMD_ALPHAS, 1e-5, 1.0)
    assert abs(mmd - ref["mmd"]) <= bound["mmd"]
    assert m.latent_two_sample_test(lat, 20) [1] >= 0.0                        # noise drawn like a forward call's, labels from the default generator
