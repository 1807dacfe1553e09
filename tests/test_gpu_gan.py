"""carel_gan_disc (csrc/gan.hip): the two adversaries of drl_classifier_ec_gan.py in one launch -- the four scalars and the four
gradient images against the float64 restatement (tests/gan_restate.py), with dropout masks from the same counter-based hash."""
import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests import gan_restate as R

pytestmark = pytest.mark.gpu

# the constants tests/test_gpu_tail.py uses for the fp32 tail kernels against their oracle (test_tail_matches_oracle)
RTOL, ATOL = 1e-4, 1e-5
IMAGES = ("g_loss", "g_ent")


def make_inputs(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 2 * D, generator=g) * 1.5
    emo = (torch.rand(B, generator=g) < 0.5).float()
    cau = (torch.rand(B, generator=g) < 0.4).float()
    if B >= 2:
        emo[0], emo[1], cau[0], cau[1] = 1.0, 0.0, 0.0, 1.0           # both labels present
    P = R.init_gan_params(D, seed=seed + 1)
    return z, emo, cau, P


def run_kernel(z, emo, cau, P, opt, drop=(0.0, 0, 0), vae_in=None):
    dev = "cuda"
    D = z.shape[1] // 2
    out = dict(terms=torch.full((8,), float("nan"), device=dev))
    for n in IMAGES:
        out[n + "_w"] = [torch.full((D,), float("nan"), device=dev) for _ in range(2)]
        out[n + "_b"] = [torch.full((1,), float("nan"), device=dev) for _ in range(2)]
    w = [P["ec_disc.weight"].reshape(-1).cuda().contiguous(), P["ce_disc.weight"].reshape(-1).cuda().contiguous()]
    b = [P["ec_disc.bias"].cuda(), P["ce_disc.bias"].cuda()]
    ops.gan_disc(z.cuda().contiguous(), emo.cuda(), cau.cuda(), w, b, opt, out["terms"], out["g_loss_w"], out["g_loss_b"],
                 out["g_ent_w"], out["g_ent_b"], drop=drop, vae_loss_in=vae_in)
    torch.cuda.synchronize()
    return out


def restated(z, emo, cau, P, opt, drop):
    """float64 terms and the four images by autograd."""
    D = z.shape[1] // 2
    p, seed, row_offset = drop
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    zd = z.double()
    t = R.disc_terms(leaf, zd[:, :D], zd[:, D:], emo.double(), cau.double(), opt.label_smoothing, opt.epsilon, p, seed if p > 0 else None,
                     row_offset)
    img = {}
    for i, name in enumerate(("ec", "ce")):
        for n, term in (("g_loss", name + "_disc_loss"), ("g_ent", name + "_entropy")):
            gw, gb = torch.autograd.grad(t[term], [leaf[name + "_disc.weight"], leaf[name + "_disc.bias"]], retain_graph=True)
            img[(n + "_w", i)], img[(n + "_b", i)] = gw.reshape(-1), gb.reshape(-1)
    return {k: float(v.detach()) for k, v in t.items()}, img


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("D", [24, 32])
@pytest.mark.parametrize("B", [2, 8, 64, 65, 512, 1024])
def test_terms_and_images_vs_float64_restatement(B, D, p_drop):
    opt = R.gan_opt(ec_dim=D)
    z, emo, cau, P = make_inputs(B, D, seed=1000 * B + D)
    drop = (p_drop, 0xC0FFEE + B, 0)
    out = run_kernel(z, emo, cau, P, opt, drop)
    terms, img = restated(z, emo, cau, P, opt, drop)
    got = out["terms"].cpu().numpy()
    for i, n in enumerate(ops.GAN_TERM_NAMES):
        print("term", B, D, p_drop, n, got[i], terms[n])
        np.testing.assert_allclose(got[i], terms[n], rtol=RTOL, atol=ATOL, err_msg=n)
    assert np.isnan(got[4])                                   # no vae_loss_in: the total is not written
    for (n, i), ref in img.items():
        g = out[n][i].cpu().double()
        print("image", B, D, p_drop, n, i, float((g - ref).abs().max()), float(ref.abs().max()))
        np.testing.assert_allclose(g.numpy(), ref.numpy(), rtol=RTOL, atol=ATOL, err_msg="%s[%d]" % (n, i))
    # two runs: identical bits (fixed summation order, no atomics)
    again = run_kernel(z, emo, cau, P, opt, drop)
    assert torch.equal(again["terms"][:4], out["terms"][:4])
    for n in IMAGES:
        for s in ("_w", "_b"):
            for i in range(2):
                assert torch.equal(again[n + s][i], out[n + s][i]), (n, s, i)


def test_total_takes_the_vae_loss_and_the_weighted_entropies():
    opt = R.gan_opt(ec_dim=24, ecce_adv_loss_weight=3.0)
    z, emo, cau, P = make_inputs(16, 24, seed=5)
    vae = torch.tensor([12.5], device="cuda")
    out = run_kernel(z, emo, cau, P, opt, vae_in=vae)
    t = out["terms"].cpu()
    want = np.float32(12.5) + np.float32(3.0) * (t[2].numpy() + t[3].numpy())
    assert abs(float(t[4]) - float(want)) <= 2e-6 * abs(float(want))


def test_row_offset_shifts_the_masks_like_a_shard():
    """drop_row_offset = first global sample index of a shard: rows 8..15 of a 16-row call see the masks of an 8-row call at offset 8."""
    opt = R.gan_opt(ec_dim=24)
    z, emo, cau, P = make_inputs(16, 24, seed=9)
    drop = (0.5, 77, 0)
    lo = run_kernel(z[:8], emo[:8], cau[:8], P, opt, (0.5, 77, 0))
    hi = run_kernel(z[8:], emo[8:], cau[8:], P, opt, (0.5, 77, 8))
    full = run_kernel(z, emo, cau, P, opt, drop)
    for i in range(4):
        assert abs(float(full["terms"][i]) - 0.5 * (float(lo["terms"][i]) + float(hi["terms"][i]))) <= 1e-5
    terms, _ = restated(z[8:], emo[8:], cau[8:], P, opt, (0.5, 77, 8))
    np.testing.assert_allclose(float(hi["terms"][0]), terms["ec_disc_loss"], rtol=RTOL, atol=ATOL)


def test_wrapper_refuses_bad_tensors():
    opt = R.gan_opt(ec_dim=24)
    z, emo, cau, P = make_inputs(4, 24, seed=3)
    with pytest.raises(L.CarelError):
        run_kernel(z.double(), emo, cau, P, opt)
    with pytest.raises(L.CarelError):
        run_kernel(z, emo[:3], cau, P, opt)
    with pytest.raises(L.CarelError):                         # CPU tensors: no fallback
        ops.gan_disc(z, emo, cau, [P["ec_disc.weight"]] * 2, [P["ec_disc.bias"]] * 2, opt, torch.zeros(8), *[[torch.zeros(24)] * 2] * 4)
