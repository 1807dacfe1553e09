"""carel_pdist_select through the C ABI, and the public paths on top of it (ops.pdist_select, pdist_quantile, median_heuristic,
median_alphas, the "median" widths of hsic_independence_test / mmd_two_sample_test / DrlClassifier.latent_independence_test /
latent_two_sample_test), against tests/pdist_select_restate.py: m at 2, 3, the edges of a 64-row tile, 1000 and the row limit, d in
1 / 24 / 63 / 64, ldx > d, ranks 0, N - 1, the two median ranks and eight at once with duplicates, duplicated rows, rows far from the
origin whose distances round below zero.  Float cases are held to the bound (d + 2 roundings of the magnitude a distance is made of,
the hsic_kern bound), integer cases to equality on the value and both counts; below <= r < below + equal everywhere; two runs give the
same bits, workspace included; the NaN / -1 regions around every output stay as they were.  Run with -s: every float case prints its
worst fraction of the bound.

Worst fraction of the bound on an MI355X: 0.311 (f_m3_d1; 0.002 .. 0.046 on the other plain cases, 0.022 with duplicated rows, 0.105
with rows at 100 + 1e-3 noise); every integer case equal, m = 8 192 included (median 1135 with 47 935 ties).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import data as D
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import ops
from tests import hsic_perm_restate as HR
from tests import pdist_select_restate as PS
from tests.gpu_util import bits
from tests.test_gpu_perm_test import PAD, NanBuf, _put          # the NaN-sentinel helpers of the two-sample suite
from tests.test_pdist_select_host import apply_refusal

pytestmark = pytest.mark.gpu


class MinusBuf:
    """`count` int64 between two regions of PAD values -1, all -1 to begin with"""

    def __init__(self, count):
        self.count = int(count)
        self.buf = torch.full((2 * PAD + self.count,), -1, dtype=torch.int64, device="cuda")
        self.t = self.buf[PAD:PAD + self.count]
        self.ptr = self.t.data_ptr()

    def guards_ok(self):
        return bool((self.buf[:PAD] == -1).all()) and bool((self.buf[PAD + self.count:] == -1).all())

    def untouched(self):
        return bool((self.buf == -1).all())


class SelCall:
    """one carel_pdist_select call on NaN / -1 outputs and a NaN workspace of exactly the stated sizes"""

    def __init__(self, xt, ranks):
        self.xt, n = xt, len(ranks)
        m, d = xt.shape
        self.values, self.counts = NanBuf(n, torch.float32), MinusBuf(2 * n)
        nbytes = int(L.load().carel_pdist_select_workspace_bytes(m, n))
        assert nbytes == PS.workspace_bytes(m, n) > 0 and nbytes % 16 == 0
        self.work = NanBuf(nbytes // 8, torch.float64)
        assert self.work.ptr % 16 == 0
        a = L.PdistSelectArgs()
        a.x, a.ldx, a.m, a.d, a.n_ranks = xt.data_ptr(), xt.stride(0), m, d, n
        for q, r in enumerate(ranks):
            a.ranks[q] = r
        a.values, a.counts, a.workspace, a.workspace_bytes = self.values.ptr, self.counts.ptr, self.work.ptr, nbytes
        self.a = a

    def run(self):
        rc = L.load().carel_pdist_select(C.byref(self.a), L.current_stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        """(values float32 ndarray, below, equal int64 ndarrays) and the guards checked"""
        assert self.values.guards_nan() and self.counts.guards_ok() and self.work.guards_nan()
        c = self.counts.t.cpu().numpy().reshape(-1, 2)
        return self.values.t.cpu().numpy().copy(), c[:, 0].copy(), c[:, 1].copy()

    def snap(self):
        return [bits(self.values.t), self.counts.t.clone(), bits(self.work.t)]

    def refill(self):
        for b in (self.values, self.work):
            b.buf.fill_(float("nan"))
        self.counts.buf.fill_(-1)

    def untouched(self):
        return self.values.all_nan() and self.work.all_nan() and self.counts.untouched()


def _twice(call):
    """-> (values, below, equal) of a run; a second run on fresh sentinels gives the same bits (the workspace too: it is fully rewritten)"""
    L.check(call.run(), "carel_pdist_select")
    got = call.out()
    snap = call.snap()
    call.refill()
    L.check(call.run(), "carel_pdist_select")
    call.out()
    for a, b in zip(snap, call.snap()):
        assert torch.equal(a, b)
    return got


def _device_sample(x, pad):
    """x on the device, as columns 2 .. 2 + d of a NaN-filled [m, d + pad] matrix when pad > 0 (ldx = d + pad)"""
    if not pad:
        return _put(x)
    m, d = x.shape
    w = torch.full((m, d + pad), float("nan"), device="cuda")
    lo = min(2, pad)
    w[:, lo:lo + d] = _put(x)
    return w[:, lo:lo + d]


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", [c["name"] for c in PS.CASES])
def test_case(name):
    c, x, ranks = PS.case_inputs(name)
    ref = PS.case_reference(name)
    xt = _device_sample(x, c["pad"])
    assert xt.stride(0) == c["d"] + c["pad"]
    v, below, equal = _twice(SelCall(xt, ranks))
    r = np.asarray(ranks, np.int64)
    assert np.isfinite(v).all() and (below >= 0).all() and (equal >= 1).all()
    assert (below <= r).all() and (r < below + equal).all()
    for q in range(len(ranks)):                                  # equal ranks get equal answers, larger ranks no smaller ones
        for p in range(len(ranks)):
            assert (v[q] <= v[p]) if ranks[q] <= ranks[p] else True
            assert ranks[q] != ranks[p] or (v[q].view(np.int32) == v[p].view(np.int32) and below[q] == below[p] and equal[q] == equal[p])
    if c["kind"] == "exact":
        assert np.array_equal(v.astype(np.float64), ref["values"]) and np.array_equal(below, ref["below"]) and np.array_equal(equal, ref["equal"])
        print("EXACT pdist_select %s values %s below %s equal %s" % (name, v.tolist(), below.tolist(), equal.tolist()))
        return
    frac = float(np.abs(v.astype(np.float64) - ref["values"]).max() / ref["bound"])
    print("FRAC pdist_select %s %.3f of the bound %.3e" % (name, frac, ref["bound"]))
    assert frac <= 1.0
    if c["kind"] == "dup":                                       # ties at exactly +0: as many as there are coinciding pairs of rows
        z = PS.coinciding_pairs(x)
        assert v[0].view(np.int32) == 0 and below[0] == 0 and equal[0] == z
    if c["kind"] == "offset":
        # the case's own precondition, on the device: the Gram matrix of the same distances has an off-diagonal entry above 1 ...
        K = ops.hsic_gram(xt, 1.0)
        K.fill_diagonal_(0.0)
        kmax = float(K.max())
        assert kmax > 1.0
        # ... so rank 0 is negative, and it is that entry's argument: log kmax = -v_0 up to the rounding of __expf (|arg| + 2 units
        # of K, the exp part of hsic_perm_restate.gram64), twice over for the logarithm taken here in double of a float32 value
        assert v[0] < 0.0 and abs(math.log(kmax) + float(v[0])) <= 2 * PS.U * (abs(float(v[0])) + 2.0)
        # ... and as many distances are negative as the matrix has entries above 1, pair by pair (the negative values here are
        # multiples of 2^-6, far from where __expf rounds to 1): the ranks on either side of that count straddle zero
        neg = int((K > 1.0).sum()) // 2
        assert below[0] == 0 and 0 < neg < PS.n_pairs(c["m"]) and int((K > 1.0).sum()) == 2 * neg
        edge, cnt = ops.pdist_select(xt, [neg - 1, neg])
        assert float(edge[0]) < 0.0 <= float(edge[1]) and int(cnt[1, 0]) == neg


def test_ops_layer_returns_what_the_abi_returns():
    c, x, ranks = PS.case_inputs("f_m129_d24")
    xt = _device_sample(x, 3)
    v, below, equal = _twice(SelCall(xt, ranks))
    values, counts = ops.pdist_select(xt, ranks)
    assert values.dtype == torch.float32 and counts.dtype == torch.int64 and tuple(values.shape) == (8,) and tuple(counts.shape) == (8, 2)
    assert np.array_equal(values.cpu().numpy().view(np.int32), v.view(np.int32))
    assert np.array_equal(counts.cpu().numpy(), np.stack((below, equal), 1))
    one = ops.pdist_select(_put(x), ranks[2:3])                  # contiguous rows, one rank: the same element
    assert bits(one[0]).item() == bits(values[2:3]).item() and torch.equal(one[1][0], counts[2])
    for bad in (lambda: ops.pdist_select(xt, []), lambda: ops.pdist_select(xt, list(range(9))), lambda: ops.pdist_select(xt.double(), [0]),
                lambda: ops.pdist_select(xt, [PS.n_pairs(129)]), lambda: ops.pdist_select(xt, [-1]), lambda: ops.pdist_select(xt.t(), [0])):
        with pytest.raises(L.CarelError):
            bad()


@pytest.mark.parametrize("what,code", PS.REFUSALS, ids=[",".join("%s=%s" % kv for kv in w.items()) for w, _ in PS.REFUSALS])
def test_refused_calls_write_nothing(what, code):
    call = SelCall(torch.rand((16, 24), device="cuda"), [0, 119])
    L.check(call.run(), "pdist select")
    call.out()
    before = call.snap()
    call.refill()
    names = ("x", "values", "workspace", "m", "d", "ldx", "n_ranks", "workspace_bytes")
    good = {k: getattr(call.a, k) for k in names}
    apply_refusal(call.a, what)
    assert call.run() == code
    assert L.load().carel_last_error().startswith(b"carel_pdist_select")
    assert call.untouched()
    for k, v in good.items():
        setattr(call.a, k, v)
    call.a.ranks[1] = 119
    L.check(call.run(), "pdist select")                          # the same valid call after the refusal: the bits of the one before it
    call.out()
    for a, b in zip(before, call.snap()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the public layer
@pytest.mark.parametrize("name", ["f_m3_d1", "f_m129_d24", "f_m1000_d24", "offset_m129_d24"])
def test_quantile_against_numpy(name):
    c, x, _ = PS.case_inputs(name)
    bound = PS.bound_of(x)                                       # a convex combination of two order statistics moves by no more
    for q, src in ((0.0, x), (0.5, _put(x)), (0.3, torch.from_numpy(x)), (0.999, x), (1.0, _device_sample(x, 5))):
        got = M.pdist_quantile(src, q)
        assert isinstance(got, float) and abs(got - PS.quantile64(x, q)) <= bound, (q, got)
    assert M.median_heuristic(x) == M.pdist_quantile(x, 0.5) == M.pdist_quantile(_put(x), 0.5)
    for bad in (lambda: M.pdist_quantile(x, 1.5), lambda: M.pdist_quantile(x, -0.1), lambda: M.pdist_quantile(x[:1], 0.5),
                lambda: M.pdist_quantile(x[0], 0.5)):
        with pytest.raises(L.CarelError):
            bad()


def test_median_of_an_even_population_is_the_mean_of_the_two_middle_values():
    c, x, _ = PS.case_inputs("e_m64_d64")                        # N = 2016; integer distances: everything is exact
    h = PS.exact_hist(x)
    sorted_d = np.repeat(np.arange(h.size), h)
    assert M.median_heuristic(x) == 0.5 * (sorted_d[1007] + sorted_d[1008]) == float(np.median(sorted_d))
    c, x, _ = PS.case_inputs("e_m3_d24")                         # N = 3: the middle one
    assert M.median_heuristic(x) == float(np.median(PS.upper64(x)[0]))


def _same(a, b):
    """two results of a test with return_stats: every number and every bit"""
    return a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and torch.equal(bits(a[2]), bits(b[2]))


def test_median_widths_equal_the_same_call_with_the_numbers():
    c, x, y, _, _, perms = HR.case_inputs("m129_p1000")
    xt, yt, pm = _put(8.0 * x), _put(3.0 * y), _put(perms[1:101])
    out = M.hsic_independence_test(xt, yt, "median", "median", 100, permutations=pm, return_stats=True, return_widths=True)
    w = out[4]
    assert len(out) == 5 and set(w) == {"s_x", "s_y"} and w["s_x"] == M.median_heuristic(xt) and w["s_y"] == M.median_heuristic(yt)
    assert _same(out, M.hsic_independence_test(xt, yt, w["s_x"], w["s_y"], 100, permutations=pm, return_stats=True))
    mixed = M.hsic_independence_test(xt, yt, 2.0, "median", 100, permutations=pm, return_widths=True)
    assert len(mixed) == 3 and mixed[2] == dict(s_x=2.0, s_y=w["s_y"])
    assert mixed[:2] == M.hsic_independence_test(xt, yt, 2.0, w["s_y"], 100, permutations=pm)
    # the two-sample test: the pooled sample's median, and the multi-scale helper
    labels = M.random_labellings(129, 129, 60, "cuda", torch.Generator(device="cuda").manual_seed(3))[1:]
    out = M.mmd_two_sample_test(xt, yt, "median", 60, labels=labels, return_stats=True, return_widths=True)
    med = M.median_heuristic(torch.cat((xt, yt), 0))
    assert len(out) == 5 and out[4] == dict(alphas=[1.0 / med]) == dict(alphas=M.median_alphas(xt, yt))
    assert _same(out, M.mmd_two_sample_test(xt, yt, out[4]["alphas"], 60, labels=labels, return_stats=True))
    assert M.median_alphas(x, yt, (0.5, 1.0, 2.0)) == [1.0 / (s * M.median_heuristic(np.concatenate((x, 3.0 * y), 0))) for s in (0.5, 1.0, 2.0)]
    stat = M.MMDStatistic(129, 129)                              # the helper's list goes into the statistic as any list does
    assert np.isfinite(float(stat(xt, yt, M.median_alphas(xt, yt, (0.5, 1.0, 2.0)))))


def test_default_calls_return_what_they_returned():
    c, x, y, _, _, perms = HR.case_inputs("m33_p63")
    pm = perms[1:]
    assert len(M.hsic_independence_test(x, y, n_permutations=63, permutations=pm)) == 2
    assert len(M.hsic_independence_test(x, y, 1.0, 1.0, 63, permutations=pm, return_stats=True)) == 4
    assert len(M.mmd_two_sample_test(x, y, [0.1], 20)) == 2 and len(M.mmd_two_sample_test(x, y, [0.1], 20, return_stats=True)) == 4
    assert len(M.hsic_independence_test(x, y, n_permutations=63, permutations=pm, return_widths=True)) == 3
    assert M.hsic_independence_test(x, y, n_permutations=63, permutations=pm, return_widths=True)[2] == dict(s_x=1.0, s_y=1.0)


def test_a_median_that_is_not_positive_is_refused():
    x = np.zeros((9, 4), np.float32)
    x[0] = 1.0                                                   # 8 of 9 rows coincide: 28 of 36 distances are 0
    assert M.median_heuristic(x) == 0.0
    with pytest.raises(L.CarelError, match="not > 0"):
        M.hsic_independence_test(x, np.arange(36, dtype=np.float32).reshape(9, 4), "median", 1.0, 5)
    with pytest.raises(L.CarelError, match="not > 0"):
        M.mmd_two_sample_test(x, x, "median", 5)
    with pytest.raises(L.CarelError, match='"median"'):
        M.hsic_independence_test(x, x, "mean", 1.0, 5)


def test_model_methods_take_the_widths_from_the_z_they_test():
    N, S, VOCAB, V, D_ = 130, 32, 600, 64, 24
    m = M.DrlClassifier(M.make_opt(pair_bow_dim=V, ec_dim=D_), M.encoder_config("zh", vocab_size=VOCAB, layers=2), seed=9).to("cuda").eval()
    b = D.synthetic_ecpe_batch(N, S, VOCAB, V, seed=230, shape="B")
    lat = m.pair_latents(*(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids")))
    g = torch.Generator().manual_seed(2)
    noise = (torch.randn(D_, generator=g), torch.randn(D_, generator=g))
    gen = lambda: torch.Generator(device="cuda").manual_seed(4)          # noqa: E731
    z = ops.sample_latents(lat, noise[0].cuda(), noise[1].cuda(), D_)
    out = m.latent_independence_test(lat, 100, noise=noise, s_e="median", s_c="median", generator=gen(), return_stats=True, return_widths=True)
    assert len(out) == 5 and out[4] == dict(s_e=M.median_heuristic(z[:, :D_]), s_c=M.median_heuristic(z[:, D_:]))
    assert _same(out, m.latent_independence_test(lat, 100, noise=noise, s_e=out[4]["s_e"], s_c=out[4]["s_c"], generator=gen(), return_stats=True))
    assert len(m.latent_independence_test(lat, 20, noise=noise)) == 2 and len(m.latent_independence_test(lat, 20, return_stats=True)) == 4
    out = m.latent_two_sample_test(lat, 100, noise=noise, alphas="median", generator=gen(), return_stats=True, return_widths=True)
    assert len(out) == 5 and out[4] == dict(alphas=M.median_alphas(z[:, :D_], z[:, D_:]))
    assert _same(out, m.latent_two_sample_test(lat, 100, noise=noise, alphas=out[4]["alphas"], generator=gen(), return_stats=True))
    assert len(m.latent_two_sample_test(lat, 20, noise=noise)) == 2
    assert m.latent_two_sample_test(lat, 20, noise=noise, return_widths=True)[2] == dict(alphas=[float(a) for a in ops.MODEL_MMD_ALPHAS])


# ------------------------------------------------------------------------------------------------ the reason for the feature
def test_the_reason_for_the_feature():
    """m = 200, d = 24, x = 8 N(0, 1), y a noisy copy: strongly dependent, distances in the thousands.  At the default widths K and L are
    the identity to the bit, every re-pairing ties with the observed one and p = 1.0 whatever the data are; at the median widths, on
    the same permutations, no re-pairing reaches the observed statistic.  (tests/test_pdist_select_host.py checks in float64 that
    every permutation is decided at the median widths.)"""
    x, y, perms = PS.power_inputs()
    pm = _put(perms[1:])
    P = perms.shape[0] - 1
    eye = torch.eye(200, device="cuda")
    assert torch.equal(ops.hsic_gram(_put(x), 1.0), eye) and torch.equal(ops.hsic_gram(_put(y), 1.0), eye)
    hsic, pval, stats, count = M.hsic_independence_test(x, y, n_permutations=P, permutations=pm, return_stats=True)
    assert pval == 1.0 and count == P
    hsic, pval, stats, count, w = M.hsic_independence_test(x, y, "median", "median", P, permutations=pm, return_stats=True, return_widths=True)
    assert count == 0 and pval == 0.0 and w["s_x"] > 1000 and w["s_y"] > 1000
