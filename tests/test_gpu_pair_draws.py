"""Many noise draws per encoder pass (carel_pair_probs_draws; DrlClassifier.pair_latents / pair_probabilities_from / draw_counts) and the
new-split driver end to end, on a two-layer encoder at S = 32.  The probabilities must have the BITS of sequential pair_probabilities
calls (same generator state); the counts are integers and must equal numpy's counts of those probabilities exactly."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import data as D
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import ops
from carel_vae_amd import training as T
from tests.test_host_data import FakeTokenizer, char_segmenter

pytestmark = pytest.mark.gpu

S, VOCAB, V = 32, 600, 64
CHUNK = 256                      # N = 300 then spans two chunks
NS = (1, 255, 256, 257, 300)
KS = (1, 3, 64, 65)
_models, _batches, _sequential = {}, {}, {}


def model_of(D_, adapter="false"):
    key = (D_, adapter)
    if key not in _models:
        opt = M.make_opt(pair_bow_dim=V, ec_dim=D_, adapter=adapter)
        m = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=VOCAB, layers=2), seed=4 + D_)
        with torch.no_grad():     # probabilities on both sides of 0.5
            m.pair_classifier.weight.mul_(8.0)
        _models[key] = m.to("cuda").eval()
    return _models[key]


def batch_of(N):
    if N not in _batches:
        b = D.synthetic_ecpe_batch(N, S, VOCAB, V, seed=100 + N, shape="B")
        _batches[N] = tuple(b[k].cuda() for k in ("input_ids", "attention_masks", "token_type_ids"))
    return _batches[N]


def sequential(D_, N, adapter="false"):
    """max(KS) sequential pair_probabilities calls from seed 1234, computed once per (ec_dim, N) and never modified."""
    key = (D_, N, adapter)
    if key not in _sequential:
        m = model_of(D_, adapter)
        torch.manual_seed(1234)
        _sequential[key] = torch.stack([m.pair_probabilities(*batch_of(N), chunk=CHUNK) for _ in range(max(KS))])
    return _sequential[key]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D_", [8, 24, 32])
def test_draws_have_the_bits_of_sequential_calls(D_, N, K):
    want = sequential(D_, N)[:K]
    m = model_of(D_)
    lat = m.pair_latents(*batch_of(N), chunk=CHUNK)
    assert lat.shape == (N, 4 * D_) and lat.dtype == torch.float32 and lat.is_cuda
    torch.manual_seed(1234)
    got, noise = m.pair_probabilities_from(lat, K, return_noise=True)
    assert got.shape == (K, N) and torch.equal(got, want)
    torch.manual_seed(1234)                                    # it drew what K _draw_noise calls draw: emotion then cause, per draw
    for k in range(K):
        assert torch.equal(noise[0][k], torch.randn(D_, device="cuda")) and torch.equal(noise[1][k], torch.randn(D_, device="cuda"))
    again = m.pair_probabilities_from(lat, noise=noise)        # replay of chosen draws
    assert torch.equal(again, want)


def test_draws_with_an_entmax_adapter():
    N, K = 257, 3
    want = sequential(24, N, "entmax")[:K]
    m = model_of(24, "entmax")
    lat = m.pair_latents(*batch_of(N), chunk=CHUNK)
    torch.manual_seed(1234)
    assert torch.equal(m.pair_probabilities_from(lat, K), want)
    assert not torch.equal(lat, model_of(24).pair_latents(*batch_of(N), chunk=CHUNK))      # the latents do come from the adapters


def test_get_pair_preds_round_flag():
    m, b = model_of(24), batch_of(257)
    torch.manual_seed(7)
    prob = m.pair_probabilities(*b).cpu().numpy()
    torch.manual_seed(7)
    raw = m.get_pair_preds(*b, round=False)
    assert isinstance(raw, list) and len(raw) == 257 and all(isinstance(r, list) and len(r) == 1 for r in raw)
    assert np.array_equal(np.array(raw, dtype=np.float32).reshape(-1), prob)
    torch.manual_seed(7)
    default = m.get_pair_preds(*b)
    torch.manual_seed(7)
    assert default == m.get_pair_preds(*b, True) == prob.reshape(-1, 1).round().tolist()
    assert set(np.array(default).reshape(-1).tolist()) <= {0.0, 1.0}


def numpy_counts(prob, labels, groups, G):
    pred = prob.cpu().numpy().round() == 1                     # ref :282
    assert np.array_equal(pred, prob.cpu().numpy() > 0.5)
    pos = labels.cpu().numpy().reshape(-1) == 1
    grp = np.zeros(len(pos), dtype=np.int64) if groups is None else groups.cpu().numpy()
    out = np.zeros((prob.shape[0], G, 3), dtype=np.int64)
    for g in range(G):
        sel = grp == g
        out[:, g, 0] = (pred & pos & sel).sum(1)
        out[:, g, 1] = (pred & ~pos & sel).sum(1)
        out[:, g, 2] = (~pred & pos & sel).sum(1)
    return out


@pytest.mark.parametrize("N,K,D_,grouping", [(1000, 70, 24, "none"), (1000, 70, 24, "three"), (515, 33, 32, "empty"), (257, 5, 8, "eight"),
                                             (100, 2, 24, "allneg"), (512, 64, 24, "three")])
def test_draw_counts_equal_numpy_counts(N, K, D_, grouping):
    m = model_of(D_)
    g = torch.Generator().manual_seed(N + K)
    lat = (torch.randn(N, 4 * D_, generator=g) * 0.7).cuda()
    labels = (torch.rand(N, 1, generator=g) < 0.4).float().cuda()
    groups, G = None, 1
    if grouping == "three":
        groups, G = torch.randint(0, 3, (N,), generator=g), 3
    elif grouping == "empty":                                  # group 1 and the last group (3) have no row
        groups, G = torch.randint(0, 2, (N,), generator=g) * 2, 4
    elif grouping == "eight":
        groups, G = torch.randint(0, 8, (N,), generator=g), 8
        groups[0] = 7
    elif grouping == "allneg":
        labels.zero_()
    torch.manual_seed(5)
    prob, noise = m.pair_probabilities_from(lat, K, return_noise=True)
    want = numpy_counts(prob, labels, groups, G)
    counts = m.draw_counts(lat, labels, K, groups=groups, noise=noise, n_groups=G)
    assert counts.dtype == torch.int64 and counts.shape == (K, G, 3) and counts.is_cuda
    assert np.array_equal(counts.cpu().numpy(), want)
    if grouping == "none":
        assert want[:, 0, :2].sum() > 0 and want[:, 0, 2].sum() > 0          # the case does predict both classes
    if grouping == "empty":
        assert not want[:, 1].any() and not want[:, 3].any() and want[:, 2].any()
    if grouping == "allneg":
        assert not want[:, :, 0].any() and not want[:, :, 2].any()
    torch.manual_seed(5)                                       # without `noise`: the same draws from the same generator state
    assert torch.equal(m.draw_counts(lat, labels, K, groups=groups, n_groups=G), counts)
    # the wrapper underneath: garbage in `counts` is overwritten, a second launch gives the same bits, prob = NULL changes nothing
    W = m._tail_weights()[0]
    args = (lat, noise[0], noise[1], W["pair_classifier.weight"], W["pair_classifier.bias"], D_)
    g32 = None if groups is None else groups.to("cuda", torch.int32)
    lab = labels.reshape(-1).contiguous()
    garbage = torch.full((K, G, 3), -123456, device="cuda", dtype=torch.int32)
    p1, c1 = ops.pair_probs_draws(*args, labels=lab, groups=g32, n_groups=G, counts_out=garbage)
    assert c1 is garbage and np.array_equal(c1.cpu().numpy(), want) and torch.equal(p1, prob)
    p2, c2 = ops.pair_probs_draws(*args, labels=lab, groups=g32, n_groups=G, counts_out=garbage)
    assert np.array_equal(c2.cpu().numpy(), want) and torch.equal(p2, prob)
    p3, c3 = ops.pair_probs_draws(*args, labels=lab, groups=g32, n_groups=G, want_prob=False)
    assert p3 is None and np.array_equal(c3.cpu().numpy(), want)
    prf = T.prf_from_counts(counts.sum(1))
    assert all(t.shape == (K,) for t in prf)


def test_probability_one_half_predicts_zero():
    opt = M.make_opt(pair_bow_dim=V)
    m = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=VOCAB, layers=2), seed=1)
    with torch.no_grad():
        m.pair_classifier.weight.zero_()
        m.pair_classifier.bias.zero_()
    m = m.to("cuda").eval()
    N, K = 300, 4
    lat = torch.randn(N, 96, generator=torch.Generator().manual_seed(0)).cuda()
    labels = (torch.arange(N) % 3 == 0).float()
    prob = m.pair_probabilities_from(lat, K)
    assert bool((prob == 0.5).all())
    counts = m.draw_counts(lat, labels, K).cpu()
    assert counts.tolist() == [[[0, 0, int(labels.sum())]]] * K


def test_refusals_leave_the_outputs_untouched():
    lib = L.load()
    N, D_, K, G = 10, 24, 3, 2
    z = lambda *s: torch.zeros(*s, device="cuda")
    lat, ee, ec, w, b, lab = z(N, 4 * D_), z(K, D_), z(K, D_), z(2 * D_), z(1), z(N)
    grp = torch.zeros(N, device="cuda", dtype=torch.int32)
    prob = torch.full((K, N), 7.0, device="cuda")
    counts = torch.full((K, G, 3), -77, device="cuda", dtype=torch.int32)
    p = lambda t: t.data_ptr()
    good = dict(lat=p(lat), eps_e=p(ee), eps_c=p(ec), pair_w=p(w), pair_b=p(b), n=N, ec_dim=D_, n_draws=K, prob=p(prob), labels=p(lab),
                groups=p(grp), n_groups=G, counts=p(counts))
    bad = [dict(lat=None), dict(eps_e=None), dict(eps_c=None), dict(pair_w=None), dict(pair_b=None), dict(n=0), dict(n=-1), dict(n_draws=0),
           dict(n_groups=0), dict(n_groups=9), dict(prob=None, counts=None), dict(ec_dim=0), dict(ec_dim=33), dict(labels=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.carel_pair_probs_draws(a["lat"], a["eps_e"], a["eps_c"], a["pair_w"], a["pair_b"], a["n"], a["ec_dim"], a["n_draws"], a["prob"],
                                        a["labels"], a["groups"], a["n_groups"], a["counts"], L.current_stream())
        assert rc < 0, change
        assert b"carel_pair_probs_draws" in lib.carel_last_error(), change
    torch.cuda.synchronize()
    assert bool((prob == 7.0).all()) and bool((counts == -77).all())
    m = model_of(24)
    for groups, kw in ((torch.tensor([0, 1, 2, 9] + [0] * 6), {}), (torch.tensor([-1] + [0] * 9), {}), (torch.tensor([0, 3] + [0] * 8), dict(n_groups=3)),
                       (torch.zeros(9, dtype=torch.long), {}), (torch.zeros(10), {})):
        with pytest.raises(L.CarelError):                      # group ids are validated on the host before any launch
            m.draw_counts(lat, lab, K, groups=groups, **kw)
    with pytest.raises(L.CarelError):
        m.draw_counts(lat, lab[:5], K)
    with pytest.raises(L.CarelError):
        m.pair_probabilities_from(lat, 0)


def _six_documents(path):
    """Six ECPE-format documents of 3-5 clauses; one true pair each, causes before, at and after the emotion clause."""
    rs = random.Random(3)
    chars = "天地人和山水风云日月星火木金土春夏秋冬东西南北"
    lines = []
    for d in range(6):
        n = 3 + d % 3
        emo = 1 + (d * 2 + 1) % n
        cause = emo if d == 4 else 1 + (emo + d) % n
        lines += ["%d %d" % (50 + d, n), "(%d,%d)" % (emo, cause)]
        for i in range(1, n + 1):
            text = " ".join(rs.choice(chars) for _ in range(rs.randint(3, 7)))
            lines.append("%d,%d,null,%s" % (i, (d % 6) if i == emo else 6, text))
    with open(path, "w", encoding="utf8") as f:
        f.write("\n".join(lines) + "\n")


def test_newsplit_self_training_iteration_end_to_end(tmp_path):
    path = str(tmp_path / "six.txt")
    _six_documents(path)
    random.seed(42)
    torch.manual_seed(0)
    test_df, sizes, unpred = D.read_ECPE_data(path, test=True, language="zh", newsplit=True)
    assert len(sizes) == 6 and list(test_df.columns) == ["pair", "label", "emotion", "temporal_order"]
    bow = D.get_bow_zh(path, segmenter=char_segmenter)
    opt = M.make_newsplit_opt(pair_bow_dim=len(bow), max_len=S, self_epochs=1, batch_size=4, best_model_path=str(tmp_path / "ckpt"),
                              model_id="newsplit", vae_lr=1e-4)
    assert opt.self_strategy == "temporal_order_modification"
    tok = FakeTokenizer()
    te = D.ECPEDataset(test_df, tokenizer=tok, bow=bow, max_len=S, segmenter=char_segmenter, language=opt.language, bow_optimize=opt.bow_optimize)
    test_loader = torch.utils.data.DataLoader(te, batch_size=len(te), shuffle=False, num_workers=0)
    model = M.DrlClassifier(opt, M.encoder_config("zh", vocab_size=1300, layers=2), seed=1).to("cuda")
    self_df = T.generate_self_train_data(sizes, test_df, test_loader, model, strategy=opt.self_strategy, self_training_iteration=0,
                                         r_flag=opt.round_up)
    assert list(self_df.columns) == ["pair", "label", "emotion"] and len(self_df) >= 4 and len(self_df) % 2 == 0
    assert list(self_df["label"]) == [1, 0] * (len(self_df) // 2)              # rows alternate positive / negative
    ordered = set(test_df["pair"][test_df["temporal_order"]])
    assert all(p in ordered for p in self_df["pair"][self_df["label"] == 1])
    assert all(p in set(test_df["pair"]) for p in self_df["pair"])
    ds = D.ECPEDataset(self_df, tokenizer=tok, bow=bow, max_len=S, segmenter=char_segmenter)
    assert len(ds) > 0                                                          # (the driver's `continue` on an empty set)
    loader = torch.utils.data.DataLoader(ds, batch_size=opt.batch_size, shuffle=True, num_workers=0, drop_last=True)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    logs = []
    best, p, r, f1 = T.train(loader, test_loader, model, [M.FusedAdam(model, lr=opt.vae_lr)], "cuda", unpred, self_metrics=[0.0, 0.0, 0.0],
                             self_train=True, opt=opt, log=logs.append)
    torch.cuda.synchronize()
    after = model.state_dict()
    assert best is model and 0.0 <= f1 <= 1.0 and sum("f1 socre" in str(l) for l in logs) == 1
    assert any(not torch.equal(before[k], after[k]) for k in before) and all(torch.isfinite(v).all() for v in after.values())
