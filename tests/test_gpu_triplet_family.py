"""carel_triplet_loss (csrc/triplet_family.hip) and the four losses of carel_vae_amd.sentence_transformer.losses on the GPU against
the float64 restatement tests/triplet_restate.py (PARITY UNPINNED: the `sentence_transformers` package is absent).  Tolerances are
those of tests/test_gpu_triplet.py: loss 2e-5 * max(1, |loss|), gradient relative norm 2e-4; counts are exact.  The inputs
(triplet_restate.CASES) keep every deciding comparison >= 5e-5 / 1e-4 apart (tests/test_triplet_family_host.py), so no selection or
hinge can flip in fp32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import sentence_transformer as S
from tests import triplet_restate as R
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu

MODE_NO = {m: i for i, m in enumerate(R.MODES)}
LOSS_TOL, GRAD_TOL = 2e-5, 2e-4


def relnorm(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@functools.lru_cache(maxsize=None)
def inputs(name):
    return R.case_inputs(R.case_by_name(name))


@functools.lru_cache(maxsize=None)
def reference(name, mode, dist, margin):
    emb, labels = inputs(name)
    return R.restate(mode, dist, emb, labels, margin)


def entry(emb, labels, mode, dist, margin, with_grad=True, work=None):
    """One carel_triplet_loss call on device tensors -> (loss [1], demb or None, stats int32 [3], work)."""
    B, H = emb.shape
    lib = L.load()
    if work is None:
        work = torch.full((lib.carel_triplet_workspace_floats(B),), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    demb = torch.full((B, H), float("nan"), device="cuda") if with_grad else None
    stats = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    a = L.TripletArgs()
    a.emb, a.labels, a.batch, a.hidden = emb.data_ptr(), labels.data_ptr(), B, H
    a.mode, a.distance, a.margin = MODE_NO[mode], (0 if dist == R.EUCLIDEAN else 1), margin
    a.loss_out, a.demb, a.stats_out, a.work = loss.data_ptr(), (demb.data_ptr() if with_grad else None), stats.data_ptr(), work.data_ptr()
    L.check(lib.carel_triplet_loss(C.byref(a), L.current_stream()), "carel_triplet_loss")
    return loss, demb, stats, work


GRID = [c["name"] for c in R.CASES if c["kind"] == "grid"]


@pytest.mark.parametrize("name", GRID)
def test_entry_point_on_the_integer_grid(name):
    case = R.case_by_name(name)
    emb_np, lab_np = inputs(name)
    B = case["B"]
    emb, labels = torch.from_numpy(emb_np).cuda(), torch.from_numpy(lab_np).to(torch.int32).cuda()
    for mode, dist, margin in R.case_runs(case):
        ref = reference(name, mode, dist, margin)
        what = (name, mode, dist, margin)
        loss, demb, stats, work = entry(emb, labels, mode, dist, margin)
        got_loss, got_stats = float(loss), tuple(int(v) for v in stats.cpu())
        D = work[:B * B].reshape(B, B).clone()
        W = work[B * B:2 * B * B].reshape(B, B).clone()
        rel = relnorm(demb, ref["grad"]) if float(np.linalg.norm(ref["grad"])) > 0 else float(demb.double().norm())
        print(what, "loss %.7g want %.7g" % (got_loss, ref["loss"]), "stats", got_stats, "grad err %.3g" % rel)
        assert got_stats == tuple(ref["counts"]), what
        assert abs(got_loss - ref["loss"]) <= LOSS_TOL * max(1.0, abs(ref["loss"])), what
        assert rel < GRAD_TOL, what
        assert torch.equal(bits(D), bits(D.t().contiguous())), what                      # bitwise symmetric
        assert relnorm(D, ref["D"]) < 1e-6, what
        if mode != "hard_soft":                                                          # the hinge modes leave integer counts
            assert torch.equal(W, W.round()), what
        # a second launch into fresh buffers: the same bits
        loss2, demb2, stats2, work2 = entry(emb, labels, mode, dist, margin)
        assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(demb), bits(demb2)) and torch.equal(stats, stats2), what
        assert torch.equal(bits(W), bits(work2[B * B:2 * B * B].reshape(B, B))), what
        # without the gradient launch: the same loss
        loss3, _, stats3, _ = entry(emb, labels, mode, dist, margin, with_grad=False)
        assert torch.equal(bits(loss), bits(loss3)) and torch.equal(stats, stats3), what


def make_loss(mode, dist, margin):
    F = S.losses.BatchHardTripletLossDistanceFunction
    metric = F.eucledian_distance if dist == R.EUCLIDEAN else F.cosine_distance
    if mode == "semihard":
        return S.losses.BatchSemiHardTripletLoss(None, margin, distance_metric=metric), "batch_semi_hard_triplet_loss"
    if mode == "all":
        return S.losses.BatchAllTripletLoss(None, metric, margin), "batch_all_triplet_loss"
    if mode == "hard":
        return S.losses.BatchHardTripletLoss(None, metric, margin), "batch_hard_triplet_loss"
    return S.losses.BatchHardSoftMarginTripletLoss(None, metric), "batch_hard_triplet_soft_margin_loss"


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["kind"] == "float"])
def test_python_classes_on_random_floats(name):
    """H = 768 through the loss classes; the cosine metric goes through Normalize (carel_l2_normalize_fwd / _bwd) and back."""
    case = R.case_by_name(name)
    emb_np, lab_np = inputs(name)
    labels = torch.from_numpy(lab_np)
    for mode, dist, margin in R.case_runs(case):
        ref = reference(name, mode, dist, margin)
        mod, method = make_loss(mode, dist, margin)
        e = torch.from_numpy(emb_np).cuda().requires_grad_(True)
        got = getattr(mod, method)(labels, e)
        (2.5 * got).backward()
        rel = relnorm(e.grad, 2.5 * ref["grad"])
        print((name, mode, dist, margin), "loss %.7g want %.7g" % (got.item(), ref["loss"]), "grad err %.3g" % rel)
        assert abs(got.item() - ref["loss"]) <= LOSS_TOL * max(1.0, abs(ref["loss"])), (mode, dist, margin)
        assert rel < GRAD_TOL, (mode, dist, margin)
        if mode == "semihard" and dist == R.EUCLIDEAN and case["B"] <= 64:
            assert mod._work == {}                                                        # the old one-workgroup kernel: no workspace
            continue
        assert list(mod._work) == [(case["B"], e.device)]                                 # the workspace is cached per batch size
        w = mod._work[(case["B"], e.device)]
        getattr(mod, method)(labels, e.detach())
        assert mod._work[(case["B"], e.device)] is w


@pytest.mark.parametrize("B", [16, 64])
def test_semihard_euclidean_up_to_64_keeps_the_old_kernel_and_its_bits(B):
    g = torch.Generator().manual_seed(B)
    emb = torch.randn((B, 768), generator=g).cuda()
    labels = torch.randint(0, 5, (B,), generator=g)
    mod = S.losses.BatchSemiHardTripletLoss(None, 4.45)
    e = emb.clone().requires_grad_(True)
    got = mod.batch_semi_hard_triplet_loss(labels, e)
    got.backward()
    loss = torch.empty(1, device="cuda")
    demb = torch.empty_like(emb)
    L.check(L.load().carel_triplet_semihard(emb.data_ptr(), labels.to(torch.int32).cuda().data_ptr(), B, 768, 4.45, loss.data_ptr(), demb.data_ptr(),
                                            L.current_stream()), "carel_triplet_semihard")
    assert torch.equal(bits(got.reshape(1)), bits(loss)) and torch.equal(bits(e.grad), bits(demb))
    assert mod._work == {}                                                                # the new entry point was not involved


def test_new_entry_point_agrees_with_the_old_kernel_at_64():
    emb_np, lab_np = inputs("b64")
    emb, labels = torch.from_numpy(emb_np).cuda(), torch.from_numpy(lab_np).to(torch.int32).cuda()
    for margin in R.GRID_MARGINS[R.EUCLIDEAN]:
        loss, demb, _, _ = entry(emb, labels, "semihard", R.EUCLIDEAN, margin)
        old_loss, old_demb = torch.empty(1, device="cuda"), torch.empty_like(emb)
        L.check(L.load().carel_triplet_semihard(emb.data_ptr(), labels.data_ptr(), 64, emb.shape[1], margin, old_loss.data_ptr(), old_demb.data_ptr(),
                                                L.current_stream()), "carel_triplet_semihard")
        assert abs(float(loss) - float(old_loss)) <= LOSS_TOL * max(1.0, abs(float(old_loss))), margin
        assert relnorm(demb, old_demb) < GRAD_TOL, margin


def test_semihard_past_64_runs_through_the_class():
    """65 sentences: a CarelError before this loss family existed."""
    emb_np, lab_np = inputs("b65")
    for margin in R.GRID_MARGINS[R.EUCLIDEAN]:
        ref = reference("b65", "semihard", R.EUCLIDEAN, margin)
        e = torch.from_numpy(emb_np).cuda().requires_grad_(True)
        got = S.losses.BatchSemiHardTripletLoss(None, margin).batch_semi_hard_triplet_loss(torch.from_numpy(lab_np), e)
        got.backward()
        assert abs(got.item() - ref["loss"]) <= LOSS_TOL * max(1.0, abs(ref["loss"])), margin
        assert relnorm(e.grad, ref["grad"]) < GRAD_TOL, margin


def test_batch_all_on_the_model_72_sentences_and_two_fit_steps():
    """chi_sentence_transformer_old.py:33 -- losses.BatchAllTripletLoss(model=..., margin=...) -- on the two-layer model of
    tests/test_gpu_triplet.py, 72 sentences (S = 32) in one batch: more than the old loss kernel could take."""
    from tests.test_gpu_triplet import _setup
    cfg, P, model, _, _ = _setup()
    rs = np.random.RandomState(17)
    sents = ["".join(chr(0x4E00 + int(c)) for c in rs.randint(0, 200, size=rs.randint(2, 29))) for _ in range(72)]
    labels = rs.randint(0, 4, size=72)
    margin = 100.0
    loss_mod = S.losses.BatchAllTripletLoss(model=model, margin=margin)
    model.train(True)
    emb = model(model.tokenize(sents))["sentence_embedding"]
    assert emb.shape == (72, 768)
    loss = loss_mod.batch_all_triplet_loss(torch.from_numpy(labels), emb)
    ref = R.restate("all", R.EUCLIDEAN, emb.detach().cpu().numpy(), labels, margin)
    assert margin > ref["D"].max() and ref["counts"][2] == ref["counts"][1] > 0           # above every distance: every valid triplet is active
    # "within 2e-5" is taken in the relative form every other loss check here uses, 2e-5 * max(1, |loss|): with the margin above every
    # distance the loss is ~100, where one fp32 ulp is already 7.6e-6, so an absolute 2e-5 would ask for under three ulps of the result
    assert abs(loss.item() - ref["loss"]) <= LOSS_TOL * max(1.0, abs(ref["loss"])), (loss.item(), ref["loss"])
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert any(float(p.grad.abs().max()) > 0 for _, p in model.named_parameters())
    for p in model.parameters():
        p.grad = None
    examples = [S.InputExample(texts=[s], label=int(l)) for s, l in zip(sents, labels)]
    loader = torch.utils.data.DataLoader(examples, shuffle=False, batch_size=72)
    model.fit(train_objectives=[(loader, loss_mod)], epochs=1, steps_per_epoch=2, warmup_steps=0, optimizer_params={"lr": 1e-3}, output_path=None)
    l1, l2 = model.last_fit.losses
    assert abs(l1 - loss.item()) <= 1e-6 * abs(l1)                                        # the same batch, the same weights
    assert np.isfinite(l2) and l2 != l1                                                   # the same batch again after one update
