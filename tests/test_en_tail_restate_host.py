"""Host-side checks of tests/en_tail_restate.py, the float64 yardstick of the three-space tail's sweep: that it IS the oracle's tail
(forward to 1e-12, gradients on the en_adv_small fixture inputs), that every case of the GPU sweep meets its input conditions, that
float32 torch stays within half of every bound (what keeps the bound constants honest), and that the limits restated from the host code
of csrc/en_tail.hip hold.  No GPU."""
import os

import numpy as np
import torch

from oracle import carel_oracle as O
from oracle import carel_oracle_en as OE
from tests import en_bow_restate as R
from tests import en_tail_restate as T


def test_float64_plain_is_the_oracle_tail_forward():
    """tail_from_latents behind `reference`, fed the latents of given pooled rows, against OE.tail_forward on the same float64 inputs;
    also with the data-parallel override, which the restatement takes as an explicit pos_weight."""
    f64 = torch.float64
    opt = OE.OptEn(pair_bow_dim=70, con_dim=8, ec_dim=4, dropout=0.5)
    cfg = O.EncoderConfig(layers=1, vocab_size=50)
    P = {k: v.to(f64) for k, v in OE.init_params(cfg, opt, seed=3).items() if not k.startswith("encoder.")}
    g = torch.Generator().manual_seed(1)
    pooled = torch.randn(5, 768, generator=g, dtype=f64)
    batch = OE.synthetic_batch(5, 16, cfg, 70, seed=2)
    batch["labels"][0], batch["labels"][1] = 1.0, 0.0
    eps = dict(con=torch.randn(8, generator=g, dtype=f64), e=torch.randn(4, generator=g, dtype=f64), c=torch.randn(4, generator=g, dtype=f64))
    args = (P, pooled, batch["emo_labels"], batch["cau_labels"], batch["labels"], batch["bow_reps"].to(f64), 11, opt, eps)
    for kw, okw in ((dict(), dict()), (dict(pos_weight=(15 - 5.0) / 5.0), dict(global_label_sum=5.0, global_n=15))):
        want = OE.tail_forward(*args, train=True, seed=77, row_offset=3, **okw)
        got = R.tail_forward(*args, weighting="plain", train=True, seed=77, row_offset=3, **kw)
        for k in T.TERM_NAMES + ("z", "pair_logit") + R.LAT_NAMES:
            assert got[k].dtype == f64
            np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol=1e-12, err_msg=k)
    assert float(got["pair"]) != float(R.tail_forward(*args, weighting="plain", train=True, seed=77, row_offset=3)["pair"])


def test_autograd_images_are_the_oracle_tail_gradients(golden_dir):
    """On the en_adv_small fixture inputs (B = 16, V = 211, the widths of the model): the latents of the oracle's own forward pass go
    through `reference`; own + entropy-share images (own + second + entropy-share for content_disc) are the gradients
    OE.loss_and_grads hands the discriminator optimisers, the classifier / decoder images those of the last group, and d lat pulled back
    through the six heads is its gradient of the latent heads' weights."""
    z = np.load(os.path.join(golden_dir, "en_adv_small.npz"), allow_pickle=False)
    batch = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    B, S, Lr, vocab, V, wseed, bseed, steps = (int(v) for v in z["meta"])
    cfg = O.EncoderConfig(layers=2, vocab_size=900, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1)
    opt = OE.OptEn(pair_bow_dim=V, dropout=0.0)
    f64 = torch.float64
    P = {k: (v.to(f64) if v.is_floating_point() else v) for k, v in OE.init_params(cfg, opt, seed=wseed).items()}
    eps = dict(con=torch.from_numpy(z["eps_con_0"]).to(f64), e=torch.from_numpy(z["eps_e_0"]).to(f64), c=torch.from_numpy(z["eps_c_0"]).to(f64))
    batch["bow_reps"] = batch["bow_reps"].to(f64)
    it = 7
    out, grads = OE.loss_and_grads(P, batch, it, cfg, opt, eps)
    D, Cd = opt.ec_dim, opt.con_dim
    c = T.make_case(B, V, Cd, D)
    c.P = {k: v for k, v in P.items() if k.split(".")[0] in T.head_shapes(V, Cd, D)}
    c.lat = torch.cat([out[n] for n in R.LAT_NAMES], dim=1)
    c.eps = torch.cat((eps["e"], eps["c"], eps["con"]))
    c.bow, c.emo, c.cau, c.pair = batch["bow_reps"], batch["emo_labels"].reshape(-1), batch["cau_labels"].reshape(-1), batch["labels"].reshape(-1)
    c.kl = R.kl_weights(it, opt)
    ref, _ = T.reference(c, "plain")
    for i, n in enumerate(T.TERM_NAMES):
        np.testing.assert_allclose(float(ref["terms"][i]), float(out[n]), rtol=1e-12, err_msg=n)
    close = lambda a, b, k: np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-9, atol=1e-12 * float(b.abs().max()), err_msg=k)      # noqa: E731
    for s, key in (("w", ".weight"), ("b", ".bias")):
        close(ref["g_cdisc_%s0" % s] + ref["g_cdisc_%s1" % s] + ref["g_cdisc_%s2" % s], grads["content_disc" + key], "content_disc" + key)
        for i, h in enumerate(T.SMALL):
            close((ref["g_sdisc_%s%d" % (s, i)] + ref["g_sdisc_ent_%s%d" % (s, i)]).reshape(grads[h + key].shape), grads[h + key], h + key)
        for n, h in (("d_ccls", "content_classifier"), ("d_emo", "emotion_classifier"), ("d_cau", "cause_classifier"), ("d_pair", "pair_classifier"),
                     ("d_dec", "decoder")):
            close(ref["%s_%s" % (n, s)].reshape(grads[h + key].shape), grads[h + key], h + key)
    # the latent heads are in no optimiser group, so the oracle returns no gradient for them: d lat is checked through the encoder's
    # last parameter instead, d vae / d pooler.dense.bias = sum_b (1 - pooled^2) (d lat W_heads)
    Wh = torch.cat([P[h + ".weight"] for h in OE.LATENT_HEADS], dim=0)
    dpre = (ref["dlat"] @ Wh) * (1 - out["pooled"] ** 2)
    close(dpre.sum(dim=0), grads["encoder.pooler.dense.bias"], "encoder.pooler.dense.bias")


def test_every_case_meets_its_input_conditions():
    f64 = torch.float64
    for spec, wt in T.ALL_CASES:
        c = T.case_of(spec)
        assert spec.D % 2 == 0 and spec.Cd % 4 == 0 and 1 <= spec.B <= 1024 and spec.D <= 64 and spec.Cd <= 1024, spec
        pw = (c.B - c.pair.sum()) / c.pair.sum()
        assert bool(torch.isfinite(pw)) and (float(pw) > 0 or c.B == 1), spec
        z = T.latents_to_z(c.lat.to(f64), c.eps.to(f64), c.D, c.Cd)
        for x, head in ((z[:, :c.D], "content_disc"), (z[:, c.D:2 * c.D], "content_disc"), (z[:, 2 * c.D:], "content_classifier"), (z, "decoder")):
            lg = x @ c.P[head + ".weight"].to(f64).t() + c.P[head + ".bias"].to(f64)
            if c.V > 1:
                top = lg.topk(2, dim=1).values
                assert bool((top[:, 0] > top[:, 1]).all()), (spec, head)           # no exactly tied maximum
            p = torch.softmax(lg, dim=1).max(dim=1).values
            if spec.peaked and head != "content_classifier":
                assert float(p.min()) > 0.9 and float((1 - p).min()) >= 1e-3, (spec, head)
        ref, scale = T.reference_of(spec, wt)
        for n, r, s in T.quantities(ref, scale):
            assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(torch.as_tensor(s)).all()), (spec, n)


def test_float32_torch_stays_within_half_of_every_bound():
    """The condition that keeps the bound constants honest: the same restatement in float32 (stock torch on the CPU) against float64,
    every case of the sweep, every quantity: at most half of c * 2^-24 * scale -- and the worst fraction of each quantity is above a
    quarter, i.e. c is the smallest such power of two (printed with -s)."""
    worst = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # one summation order for the float32 figures, whatever machine runs this
    try:
        for spec, wt in T.ALL_CASES:
            r64, s = T.reference_of(spec, wt)
            r32, _ = T.reference(T.case_of(spec), wt, torch.float32)
            for (n, ref, sc), (_, got, _) in zip(T.quantities(r64, s), T.quantities(r32, s)):
                f = T.fraction(got, ref, T.bound(n, sc))
                worst[T.family(n)] = max(worst.get(T.family(n), 0.0), f)
                assert f <= 0.5, (spec.id, wt, n, f)
        for shape in T.FRONT_CASES + [T.FRONT_ODD]:
            f = T.front_case(*shape)
            p64, l64 = T.front(f)
            p32, l32 = T.front(f, torch.float32)
            rows = lambda r: r.abs().max(dim=1, keepdim=True).values      # noqa: E731
            cmp = [("pooled", p32, p64, rows(p64)), ("lat", l32, l64, rows(l64))]
            for go in (None, 2.5):
                b64, b32 = T.back(f, go), T.back(f, go, torch.float32)
                cmp += [(n, b32[n], b64[n], rows(b64[n]) if n == "dx_last" else float(b64[n].abs().max())) for n in b64]
                assert bool((b64["dx_last"].abs().sum(dim=1) == 0)[[r for r in range(f.n_rows) if r not in set(f.rows.tolist())]].all())
            for n, got, ref, sc in cmp:
                fr = T.fraction(got, ref, T.bound(n, sc, T.C_FRONT))
                worst[n] = max(worst.get(n, 0.0), fr)
                assert fr <= 0.5, (shape, n, fr)
    finally:
        torch.set_num_threads(threads)
    print("float32 torch, worst fraction of the bound: " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert set(worst) == set(T.C_BOUND) | set(T.C_FRONT)
    assert all(v > 0.25 for v in worst.values()), {k: v for k, v in worst.items() if v <= 0.25}


def test_front_cases_cover_the_cls_stride_and_the_row_index():
    """Per shape: a dense case with seq_len 2 (no cls_rows, n_rows = B * seq_len: every use of the [CLS] stride matters) and a case with
    irregular, increasing cls_rows and n_rows past the last of them."""
    shapes = {(B, Cd) for B, Cd, _ in T.FRONT_CASES}
    assert len(shapes) == 21
    for B, Cd in shapes:
        assert (B, Cd, "dense2") in T.FRONT_CASES and (B, Cd, "rows") in T.FRONT_CASES
        f = T.front_case(B, Cd, "dense2")
        assert not f.irregular and f.seq_len == 2 and f.n_rows == B * f.seq_len and f.rows.tolist() == [2 * b for b in range(B)]
        f = T.front_case(B, Cd, "rows")
        r = f.rows.tolist()
        assert f.irregular and all(a < b for a, b in zip(r, r[1:])) and f.n_rows > r[-1] + 1 and r != [f.seq_len * b for b in range(B)] \
            and (B < 5 or r != [r[0] + k * (r[1] - r[0]) for k in range(B)])
    assert any(m == "dense1" for _, _, m in T.FRONT_CASES)
    f = T.front_case(*T.FRONT_ODD)
    assert f.D % 2 == 1 and f.Cd % 4 == 2


def test_restated_limits():
    assert (T.heads_lds_bytes(909), T.heads_lds_bytes(910)) == (65512, 65584) and T.heads_lds_bytes(909) <= 65536 < T.heads_lds_bytes(910)
    assert [T.split_plan(V) for V in (2048, 2049, 16384, 16385, 23771)] == [(8, 256, 8), (9, 256, 9), (64, 256, 64), (64, 288, 57), (64, 384, 62)]
    assert all(T.split_plan(V)[2] == T.split_plan(V)[0] for V in range(1, 16385))        # inside the tail the empty-slab branch starts at 16 385
    assert T.split_plan(70, 7) == (7, 32, 3)


def test_restated_workspace_carving_is_the_librarys():
    from carel_vae_amd import _lib as L
    lib = L.load()
    shapes = {(s.B, s.D, s.Cd, s.V) for s, _ in T.ALL_CASES} | {(64, 24, 384, 23771), (1024, 64, 1024, 23771)}
    for B, D, Cd, V in sorted(shapes):
        w = T.carve(B, D, Cd, V)
        assert w["total"] == lib.carel_en_tail_workspace_floats(B, D, Cd, V), (B, D, Cd, V)
        if D == 24:
            assert T.work_offsets(B, Cd, V) == (w["rowstat"], w["dlat"]), (B, Cd, V)
        assert T.work_offsets(B, Cd, V, D) == (w["rowstat"], w["dlat"])
    assert T.carve(64, 24, 384, 23771)["total"] == 6489088
