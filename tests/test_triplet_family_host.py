"""The batch triplet loss family without a GPU: the two float64 restatements of tests/triplet_restate.py agree with each other, the
GPU inputs keep every deciding comparison far from fp32 rounding, and the C ABI / Python surface of carel_triplet_loss
(include/carel_hip.h, carel_vae_amd/sentence_transformer.py) is what the header says.  No kernel is launched here."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests import triplet_restate as R


# ------------------------------------------------------------------------------------------------ (ii) == (i)
@pytest.mark.parametrize("distance", [R.EUCLIDEAN, R.COSINE])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("B", [2, 5, 16, 33])
def test_definitions_equal_the_published_form(B, mode, distance):
    for classes in (1, 2, 4, B):
        rs = np.random.RandomState(1000 * B + classes)
        emb = rs.randn(B, 12)
        labels = rs.permutation(B) if classes == B else rs.randint(0, classes, size=B)
        for margin in (0.3, 9.0):
            e = torch.from_numpy(emb).requires_grad_(True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = R.published(mode, distance, e, torch.from_numpy(labels), margin)
            got = R.restate(mode, distance, emb, labels, margin)
            if not torch.isfinite(want):                 # semi-hard without a positive pair: 0 / 0 in the package, 0 here
                assert mode == "semihard" and got["counts"][0] == 0 and got["loss"] == 0.0
                continue
            assert abs(got["loss"] - want.item()) <= 1e-12, (classes, margin, got["loss"], want.item())
            if want.requires_grad:
                want.backward()
                ref = e.grad.numpy()
            else:
                ref = np.zeros_like(emb)
            # relative to the gradient; where the exact gradient is 0 (cosine distance, one class of two rows: the Normalize
            # projection g - n (n.g) cancels completely) both sides hold float64 rounding residue of ~1e-17, so the
            # denominator has a floor of 1e-3, far below the 0.01 .. 1 of every non-zero gradient here
            err = np.linalg.norm(got["grad"] - ref)
            assert err <= 1e-10 * max(np.linalg.norm(ref), 1e-3), (classes, margin, err, np.linalg.norm(ref))


def test_counts_and_tie_rule_of_the_restatement():
    # four points on a line, labels 0 0 1 1: anchor 0 has positive 1 (distance 1) and negatives 2, 3 at the SAME distance 2
    emb = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [0.0, -2.0]])
    labels = np.array([0, 0, 1, 1])
    r = R.restate("semihard", R.EUCLIDEAN, emb, labels, 5.0)
    assert r["counts"][:2] == (4, 8)
    assert r["W"][0, 2] < 0 and r["W"][0, 3] == 0            # the lower index takes the tie
    r = R.restate("all", R.EUCLIDEAN, emb, labels, 5.0)
    assert r["counts"] == (4, 8, 8)
    r = R.restate("hard", R.EUCLIDEAN, emb, labels, 5.0)
    assert r["counts"] == (4, 8, 4) and r["W"][0, 2] < 0 and r["W"][0, 3] == 0
    assert R.restate("hard_soft", R.EUCLIDEAN, emb, labels)["counts"] == (4, 8, 4)


# ------------------------------------------------------------------------------------------------ the input condition
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_gpu_inputs_keep_every_comparison_away_from_fp32_rounding(case):
    """A property of the inputs alone: no comparison that decides a selection or a hinge is closer than 5e-5 (integer grid) /
    1e-4 (random floats), ~20x the fp32 rounding of these distances; and the large margin really is above every distance
    difference (no hinge cuts)."""
    emb, labels = R.case_inputs(case)
    bar = 5e-5 if case["kind"] == "grid" else 1e-4
    assert emb.dtype == np.float32 and emb.shape == (case["B"], case["H"])
    if case["kind"] == "grid":
        assert np.array_equal(emb, np.round(emb)) and np.abs(emb).max() <= 3
    for mode, dist, margin in R.case_runs(case):
        r = R.restate(mode, dist, emb, labels, margin)
        assert r["min_gap"] >= bar, (case["name"], mode, dist, margin, r["min_gap"])
        if margin == case["margins"][dist][-1]:
            assert margin > r["D"].max() - r["D"].min() and margin > r["D"].max()
            if mode in ("semihard", "all"):
                assert r["counts"][2] == r["counts"][0 if mode == "semihard" else 1]


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from carel_vae_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_abi_version_symbols_and_struct_layout(lib):
    from carel_vae_amd import _lib, build
    assert _lib.ABI_VERSION == 9 and lib.carel_abi_version() == 9
    raw = C.CDLL(build.lib_path())
    for name in ("carel_triplet_loss", "carel_triplet_workspace_floats"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    T = _lib.TripletArgs
    assert C.sizeof(T) == 72
    offs = {n: getattr(T, n).offset for n, _ in T._fields_}
    assert offs == dict(emb=0, labels=8, batch=16, hidden=20, mode=24, distance=28, margin=32, loss_out=40, demb=48, stats_out=56, work=64)
    assert (_lib.TRIPLET_SEMIHARD, _lib.TRIPLET_ALL, _lib.TRIPLET_HARD, _lib.TRIPLET_HARD_SOFT) == (0, 1, 2, 3)
    assert (_lib.TRIPLET_EUCLIDEAN, _lib.TRIPLET_DOT) == (0, 1)


def test_argument_errors_come_before_any_launch(lib):
    from carel_vae_amd import _lib
    assert lib.carel_triplet_loss(None, None) == -1
    assert b"carel_triplet_loss" in lib.carel_last_error()
    buf = (C.c_float * 16)()                              # host memory: a call that got past the checks would fail differently (-3)
    p = C.addressof(buf)

    def args(**kw):
        a = _lib.TripletArgs()
        a.emb, a.labels, a.loss_out, a.work = p, p, p, p
        a.batch, a.hidden, a.mode, a.distance, a.margin = 2, 4, 0, 0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, code, word in ((dict(emb=None), -1, b"null"), (dict(labels=None), -1, b"null"), (dict(loss_out=None), -1, b"null"),
                           (dict(work=None), -1, b"null"), (dict(batch=0), -2, b"512"), (dict(batch=513), -2, b"512"),
                           (dict(batch=-1), -2, b"512"), (dict(hidden=0), -2, b"hidden"), (dict(mode=4), -1, b"mode"),
                           (dict(mode=-1), -1, b"mode"), (dict(distance=2), -1, b"distance")):
        assert lib.carel_triplet_loss(C.byref(args(**kw)), None) == code, kw
        assert word in lib.carel_last_error(), (kw, lib.carel_last_error())


def test_workspace_size(lib):
    f = lib.carel_triplet_workspace_floats
    prev = 0
    for B in (1, 2, 16, 64, 65, 160, 511, 512):
        n = f(B)
        assert n >= 2 * B * B + 4 * B + 1                 # D, W, the partial losses, three counts per anchor, the scale
        assert n > prev
        prev = n
    assert f(512) * 4 < 4 << 20                           # ~2 MiB at the largest batch
    assert f(0) == 0 and f(513) == 0


# ------------------------------------------------------------------------------------------------ Python surface
def test_losses_surface():
    from carel_vae_amd import sentence_transformer as S
    from carel_vae_amd._lib import CarelError
    F = S.losses.BatchHardTripletLossDistanceFunction
    assert callable(F.eucledian_distance) and callable(F.cosine_distance)
    for name in ("BatchSemiHardTripletLoss", "BatchAllTripletLoss", "BatchHardTripletLoss", "BatchHardSoftMarginTripletLoss"):
        assert issubclass(getattr(S.losses, name), torch.nn.Module)
    assert S.losses.BatchAllTripletLoss(model=None).triplet_margin == 5
    assert S.losses.BatchHardTripletLoss(model=None).triplet_margin == 5
    assert S.losses.BatchSemiHardTripletLoss(model=None).triplet_margin == 5
    assert S.losses.BatchSemiHardTripletLoss(None, 4.45).triplet_margin == 4.45
    assert S.losses.BatchAllTripletLoss(None, F.cosine_distance, 10).triplet_margin == 10         # the package's positional order
    assert S.losses.BatchAllTripletLoss(model=None, margin=10).distance_metric is F.eucledian_distance      # chi_sentence_transformer_old.py:33
    assert S.losses.BatchSemiHardTripletLoss(None, distance_metric=F.cosine_distance).distance_metric is F.cosine_distance
    with pytest.raises(TypeError):
        S.losses.BatchSemiHardTripletLoss(None, 5.0, F.cosine_distance)                           # keyword-only: (model, margin) stays positional
    with pytest.raises(TypeError):
        S.losses.BatchHardSoftMarginTripletLoss(None, F.eucledian_distance, 5)                    # no margin in the soft-margin loss
    for name, method in (("BatchSemiHardTripletLoss", "batch_semi_hard_triplet_loss"), ("BatchAllTripletLoss", "batch_all_triplet_loss"),
                         ("BatchHardTripletLoss", "batch_hard_triplet_loss"), ("BatchHardSoftMarginTripletLoss", "batch_hard_triplet_soft_margin_loss")):
        assert callable(getattr(getattr(S.losses, name), method)) and callable(getattr(S.losses, name).forward)
    for bad in (lambda e: e @ e.t(), torch.cdist, None, "cosine"):
        with pytest.raises(CarelError):
            S.losses.BatchAllTripletLoss(None, distance_metric=bad)
        with pytest.raises(CarelError):
            S.losses.BatchSemiHardTripletLoss(None, distance_metric=bad)
    with pytest.raises(CarelError):                        # selectors, not an eager implementation
        F.eucledian_distance(torch.zeros(2, 4))


def test_oversize_batches_and_cpu_tensors_are_refused():
    from carel_vae_amd import sentence_transformer as S
    from carel_vae_amd._lib import CarelError
    F = S.losses.BatchHardTripletLossDistanceFunction
    mods = [(S.losses.BatchSemiHardTripletLoss(None), "batch_semi_hard_triplet_loss"),
            (S.losses.BatchSemiHardTripletLoss(None, distance_metric=F.cosine_distance), "batch_semi_hard_triplet_loss"),
            (S.losses.BatchAllTripletLoss(None), "batch_all_triplet_loss"), (S.losses.BatchHardTripletLoss(None), "batch_hard_triplet_loss"),
            (S.losses.BatchHardSoftMarginTripletLoss(None), "batch_hard_triplet_soft_margin_loss")]
    for mod, method in mods:
        with pytest.raises(CarelError, match="512"):       # named before anything is launched (there is no GPU here to launch on)
            getattr(mod, method)(torch.zeros(513, dtype=torch.long), torch.zeros(513, 8))
        for B in (4, 65, 512):
            with pytest.raises(CarelError, match="CPU"):
                getattr(mod, method)(torch.zeros(B, dtype=torch.long), torch.zeros(B, 8))
        for n in (3, 5):                                   # one label per sentence: the kernels read labels[0 .. sentences)
            with pytest.raises(CarelError, match="labels"):
                getattr(mod, method)(torch.zeros(n, dtype=torch.long), torch.zeros(4, 8))
