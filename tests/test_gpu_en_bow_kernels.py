"""carel_en_tail_losses_bow (the element-weighted content losses of drl_classifier_bow_loss.py) driven directly from given latents
and noise, no encoder: the three content row statistics and the images g_cdisc_*[0..2], d_ccls_* and d lat against the float64
restatement tests/en_bow_restate.py.

Tolerance: the same harness first measures the existing UNWEIGHTED instantiation (carel_en_tail_losses against the restatement
with every weight 1) on the same inputs; the weighted path may be at most twice that error per quantity -- it adds one sigmoid
value and one multiply per element.  Both errors sit at a few fp32 roundings (1e-7), where the figure of ONE shape is noise:
measured shape by shape, the ratio weighted / unweighted is 0.65-1.4 for the vectors and images (1.8 and 2.2 at B = 1, V = 70, 70
numbers per image) and anything from 0.03 to 40 for a scalar term, which lands within 1e-9 of float64 by chance.  So "the error
of a quantity" is its worst figure over the sweep, for both columns alike (measured: DESIGN.md section 7).
"""
from types import SimpleNamespace

import pytest
import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import en_bow_restate as R
from tests.en_tail_restate import run_kernel          # the ctypes driver, shared with tests/test_gpu_en_tail_sweep.py

pytestmark = pytest.mark.gpu

D = 24
HEADS = dict(content_disc=lambda V, Cd: (V, D), content_classifier=lambda V, Cd: (V, Cd), decoder=lambda V, Cd: (V, 2 * D + Cd),
             emotion_disc=lambda V, Cd: (1, Cd), cause_disc=lambda V, Cd: (1, Cd), ec_disc=lambda V, Cd: (1, D), ce_disc=lambda V, Cd: (1, D),
             emotion_classifier=lambda V, Cd: (1, D), cause_classifier=lambda V, Cd: (1, D), pair_classifier=lambda V, Cd: (1, 2 * D))
IMAGES = ["g_cdisc_w0", "g_cdisc_b0", "g_cdisc_w1", "g_cdisc_b1", "g_cdisc_w2", "g_cdisc_b2", "d_ccls_w", "d_ccls_b", "dlat"]
# what neither entry point weights: every term but the three content losses and the total, and every image below
UNWEIGHTED_TERMS = [2, 3, 4, 5] + list(range(7, 15)) + list(range(16, 21))
UNWEIGHTED_IMAGES = ["g_cdisc_w2", "g_cdisc_b2", "d_dec_w", "d_dec_b", "d_emo_w", "d_cau_w", "d_pair_w", "d_pair_b"] + \
    ["g_sdisc_w%d" % i for i in range(4)] + ["g_sdisc_ent_w%d" % i for i in range(4)] + ["g_sdisc_b%d" % i for i in range(4)]


def make_case(B, V, Cd, seed, drop_p=0.0, edit=None):
    g = torch.Generator().manual_seed(seed)
    opt = OE.OptEn(pair_bow_dim=V, con_dim=Cd, ec_dim=D, dropout=drop_p)
    P = {}
    for name, shp in HEADS.items():
        s = shp(V, Cd)
        bound = 1.0 / s[1] ** 0.5
        P[name + ".weight"] = (torch.rand(s, generator=g) * 2 - 1) * bound
        P[name + ".bias"] = (torch.rand(s[0], generator=g) * 2 - 1) * bound
    lat = torch.randn(B, 2 * Cd + 4 * D, generator=g) * 0.3
    eps = torch.randn(2 * D + Cd, generator=g)
    bow = (torch.rand(B, V, generator=g) < 0.05).float()
    emo, cau = (torch.rand(B, generator=g) < 0.5).float(), (torch.rand(B, generator=g) < 0.5).float()
    pair = (torch.rand(B, generator=g) < 0.4).float()
    pair[0] = 1.0
    c = SimpleNamespace(B=B, V=V, Cd=Cd, opt=opt, P=P, lat=lat, eps=eps, bow=bow, emo=emo, cau=cau, pair=pair, drop_p=drop_p, seed=1234 + seed,
                        kl=(0.013, 0.021))
    if edit is not None:
        edit(c)
    return c


def reference(c, weighting):
    """float64 restatement: terms, row statistics and the same images by autograd."""
    f64 = torch.float64
    P = {k: v.to(f64).requires_grad_(True) for k, v in c.P.items()}
    lat = c.lat.to(f64).requires_grad_(True)
    o = c.opt
    eps = dict(e=c.eps[:D].to(f64), c=c.eps[D:2 * D].to(f64), con=c.eps[2 * D:].to(f64))
    out = R.tail_from_latents(P, R.split_lat(lat, o), c.emo, c.cau, c.pair, c.bow.to(f64), c.kl[0], c.kl[1], o, eps, weighting=weighting,
                              train=c.drop_p > 0, seed=c.seed)
    ref = dict(t0=out["content_disc_emo"].detach(), t1=out["content_disc_cau"].detach(), t15=out["con_mul"].detach())
    gw = lambda loss, k: torch.autograd.grad(loss, P[k], retain_graph=True)[0]      # noqa: E731
    for i, n in enumerate(("content_disc_emo", "content_disc_cau")):
        ref["g_cdisc_w%d" % i], ref["g_cdisc_b%d" % i] = gw(out[n], "content_disc.weight"), gw(out[n], "content_disc.bias")
    ref["g_cdisc_w2"], ref["g_cdisc_b2"] = gw(out["vae"], "content_disc.weight"), gw(out["vae"], "content_disc.bias")
    ref["d_ccls_w"], ref["d_ccls_b"] = gw(out["vae"], "content_classifier.weight"), gw(out["vae"], "content_classifier.bias")
    ref["dlat"] = torch.autograd.grad(out["vae"], lat, retain_graph=True)[0]
    # row statistics: sum_j omega_j bce_j per sample, recomputed from the pieces the restatement exposes
    with torch.no_grad():
        ls, V = o.label_smoothing, c.V
        bow_t = c.bow.to(f64) * (1 - ls) + ls / V
        z = out["z"]
        drop = lambda t, site: t if c.drop_p <= 0 else t * O.dropout_scale_mask(c.seed, site, tuple(t.shape), c.drop_p).to(f64)      # noqa: E731
        lin = lambda x, n: x @ P[n + ".weight"].t() + P[n + ".bias"]      # noqa: E731
        cw = out["con_w"]
        ecw = 1 - cw if weighting == "bow" else cw          # "plain": every weight is 1
        rows = []
        for x, site, head, om in ((z[:, :D], OE.SITE_CDISC_E, "content_disc", ecw), (z[:, D:2 * D], OE.SITE_CDISC_C, "content_disc", ecw),
                                  (z[:, 2 * D:], OE.SITE_CMUL, "content_classifier", cw)):
            rows.append((om * O.bce_prob(torch.softmax(lin(drop(x, site), head), dim=1), bow_t)).sum(dim=1))
        ref["rowstat"] = torch.stack(rows)
        ref["con_w"] = cw if weighting == "bow" else None
    return ref


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def errors(got, ref):
    e = {k: rel(got[k], ref[k]) for k in IMAGES + ["rowstat"]}
    for i in (0, 1, 15):
        e["t%d" % i] = abs(float(got["terms"][i]) - float(ref["t%d" % i])) / abs(float(ref["t%d" % i]))
    return e


SHAPES = [(1, 70, 4), (5, 211, 384), (16, 2048, 4), (65, 2049, 384), (5, 4100, 4), (65, 4100, 384), (1, 2049, 384), (16, 70, 384),
          (16, 211, 4), (65, 2048, 4), (5, 2048, 384), (1, 4100, 4)]
_cache = {}


def results(shape):
    if shape not in _cache:
        B, V, Cd = shape
        c = make_case(B, V, Cd, seed=B * 7 + V + Cd)
        _cache[shape] = (c, run_kernel(c, False), run_kernel(c, True), run_kernel(c, True), reference(c, "plain"), reference(c, "bow"))
    return _cache[shape]


def test_weighted_error_is_at_most_twice_the_unweighted_error():
    """Per quantity, over the whole sweep: the worst error of the weighted entry point against float64 is at most twice the worst error
    of the unweighted one against float64 on the same inputs (every figure is printed; DESIGN.md section 7 has the table)."""
    worst_plain, worst_bow = {}, {}
    for shape in SHAPES:
        c, plain, bow, bow2, ref_plain, ref_bow = results(shape)
        e_plain, e_bow = errors(plain, ref_plain), errors(bow, ref_bow)
        for k in sorted(e_plain):
            print("%-12s B=%d V=%d Cd=%d  unweighted %.3e  weighted %.3e" % ((k,) + shape + (e_plain[k], e_bow[k])))
            worst_plain[k], worst_bow[k] = max(worst_plain.get(k, 0.0), e_plain[k]), max(worst_bow.get(k, 0.0), e_bow[k])
        assert rel(bow["con_w"], ref_bow["con_w"]) < 1e-6, shape            # sigmoid of an fp32 GEMM row of length con_dim
        for r in (plain, bow):
            assert all(bool(torch.isfinite(v).all()) for v in r.values()), shape
    for k in sorted(worst_plain):
        print("WORST %-12s unweighted %.3e  weighted %.3e" % (k, worst_plain[k], worst_bow[k]))
    for k in sorted(worst_plain):
        assert worst_bow[k] <= 2 * worst_plain[k], (k, worst_bow[k], worst_plain[k])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-V%d-Cd%d" % s)
def test_repeat_is_bitwise_and_unweighted_outputs_do_not_move(shape):
    c, plain, bow, bow2, _, _ = results(shape)
    for k in bow:
        assert torch.equal(bow[k], bow2[k]), k
    assert torch.equal(bow["terms"][UNWEIGHTED_TERMS], plain["terms"][UNWEIGHTED_TERMS])
    for k in UNWEIGHTED_IMAGES + ["z"]:
        assert torch.equal(bow[k], plain[k]), k
    assert not torch.equal(bow["terms"][:2], plain["terms"][:2]) and not torch.equal(bow["g_cdisc_w0"], plain["g_cdisc_w0"])


def _saturate_weights(c):          # content-classifier logits of +-40: the weights saturate at 0 and 1
    c.P["content_classifier.weight"].zero_()
    c.P["content_classifier.bias"] = torch.where(torch.arange(c.V) % 2 == 0, 40.0, -40.0)


def _saturate_softmax(c):          # one content-discriminator logit far above the rest: a softmax row with p -> 1
    c.P["content_disc.bias"][3] = 80.0
    c.P["content_classifier.bias"][5] = 80.0


@pytest.mark.parametrize("edit", [_saturate_weights, _saturate_softmax], ids=["weights_0_1", "softmax_p_1"])
def test_saturated_inputs_stay_finite(edit):
    c = make_case(5, 2049, 384, seed=17, edit=edit)
    got = run_kernel(c, True)
    if edit is _saturate_weights:
        assert float(got["con_w"].min()) < 1e-15 and float(got["con_w"].max()) == 1.0
    for k, v in got.items():
        assert bool(torch.isfinite(v[:21] if k == "terms" else v).all()), k


def test_half_weights_halve_the_content_terms_at_real_width():
    """B = 64, V = 23 771, dropout 0.5, content-classifier weight and bias zero: omega = sigmoid(0) = 0.5 = 1 - omega exactly.
    The kernel multiplies each element by omega BEFORE summing, and a multiplication by 0.5 commutes with every fp32 rounding
    (no value here is near the denormal range), so the equality with half of the unweighted call is BITWISE."""
    def zero_ccls(c):
        c.P["content_classifier.weight"].zero_()
        c.P["content_classifier.bias"].zero_()
    c = make_case(64, 23771, 384, seed=5, drop_p=0.5, edit=zero_ccls)
    plain, bow = run_kernel(c, False), run_kernel(c, True)
    assert torch.equal(bow["con_w"], torch.full_like(bow["con_w"], 0.5))
    keep = (bow["xw"] != 0).float().mean()
    assert abs(float(keep) - 0.5) < 0.02
    for i in (0, 1, 15):
        assert float(bow["terms"][i]) == 0.5 * float(plain["terms"][i]), i
    for k in ("g_cdisc_w0", "g_cdisc_b0", "g_cdisc_w1", "g_cdisc_b1", "d_ccls_w", "d_ccls_b", "rowstat"):
        assert torch.equal(bow[k], 0.5 * plain[k]), k
    assert float(plain["g_cdisc_w0"].abs().max()) > 0 and float(plain["d_ccls_b"].abs().max()) > 0
