"""What tests/test_gpu_eval_paths.py and tests/test_gpu_pool_sweep.py rely on, checked without a GPU (tests/eval_restate.py):

  * the ORACLE alone gives the evaluation cases probabilities on both sides of 0.5 and away from it, and the case lengths hold every edge;
  * stock float32 torch stays within half of every bound of the float64 restatement of the four row kernels;
  * the per-row tolerances are three times a figure measured here, oracle against oracle -- never from the kernels;
  * the packing arrays of DrlClassifier._pack_info equal a plain loop on the cases' lengths.

Measured on the CPU (oracle fp32 against oracle bf16_round, worst row): latents 2.438e-3 on one host and 2.489e-3 on another, sentence
embeddings 2.374e-3, probabilities 2.528e-3 at pair-head scale 8.  TOL_ROW_LATENT = 7.5e-3 is tighter per row than TOL_LATENT_BF16 =
1e-2 is for a whole tensor.

The kernels' worst fraction of each tolerance, measured on an MI355X (pytest -s tests/test_gpu_eval_paths.py tests/test_gpu_pool_sweep.py):
  TOL_ROW_LATENT  pair_latents, every case and chunk          0.369 (against fp32)  0.334 (against bf16_round): worst rows 2.77e-3 / 2.51e-3
  TOL_PROB        pair_probabilities / get_pair_preds        0.340
  TOL_ROW_EMBED   encode, both variants, every batch size    0.365 (against fp32)  0.308 (against bf16_round)
  row kernels     mean pool forward 0.250, backward 0.857 (two roundings of two budgeted); normalise y 0.491, norm 0.205, dx 0.444
The slice, neighbour, padding-content and length-rounding properties and forward_terms == pair_latents all held bit for bit."""
import numpy as np
import pytest
import torch

from carel_vae_amd import drl_classifier as M
from tests import eval_restate as R


# ------------------------------------------------------------------------------------------------ oracle conditions
@pytest.mark.parametrize("name", list(R.EVAL_CASES))
def test_oracle_puts_both_classes_far_from_one_half(name):
    """From 9 rows on: at least a quarter of the rows in each class and three quarters far; a smaller case has both classes (one row: one)."""
    N = R.EVAL_CASES[name][1]
    p = R.oracle_prob(name)
    ones, far = float((p > 0.5).double().mean()), float(((p - 0.5).abs() > R.FAR).double().mean())
    assert far >= 0.75, (name, far)
    if N >= 9:
        assert 0.25 <= ones <= 0.75, (name, ones)
    elif N > 1:
        assert 0.0 < ones < 1.0, (name, ones)
    assert 3 * R.YARD_PROB < R.FAR            # a far row cannot change class within the probability tolerance


def test_case_lengths_contain_every_edge():
    E, L_ = R.EVAL_CASES, R.case_lengths
    assert {E[n][1] for n in E if E[n][0] == "zh24" and E[n][3] == "B"} == {1, 5, 127, 128, 129, 300}
    assert R.chunks_of(5) == [1, 5, 8, 128] and R.chunks_of(300) == [8, 128, 300] and R.chunks_of(128) == [8, 128]
    assert set(L_("zh24_two")) == {2} and set(L_("zh24_full")) == {32}
    mix = L_("zh24_mix")
    assert {2, 3, 31, 32} <= set(mix) and {2, 63, 64} <= set(L_("zh24_s64_mix"))
    last = L_("zh24_lastfull")
    assert len(last) == 129 and max(last[:128]) < 32 and last[128:] == [32]
    for c in (128, 8):                       # the last chunk is all full-length (dense), every earlier chunk has padding (packed)
        starts = list(range(0, 129, c))
        assert all(sum(last[s:s + c]) < 32 * len(last[s:s + c]) for s in starts[:-1]) and set(last[starts[-1]:]) == {32}
    b = L_("zh24_B_300")
    assert min(b) >= 4 and max(b) == 32 and 0.1 < sum(v == 32 for v in b) / 300 < 0.9
    assert {"zh32", "en24"} <= {E[n][0] for n in E}
    for n in E:                              # prefix masks, pad_id under mask 0, the lengths the mask says
        bt = R.case_batch(n)
        att = bt["attention_masks"]
        assert att.sum(1).tolist() == L_(n)
        assert bool(((torch.arange(att.shape[1])[None, :] < att.sum(1)[:, None]).long() == att).all())
        assert bool((bt["input_ids"][att == 0] == R.MODELS[E[n][0]][0].pad_id).all())
    st = R.st_lengths()
    assert len(st) == 37 and {2, R.ST_S} <= set(st) and 37 % 16 and 37 % 5
    assert set(R.POOL_LENS) == {0, 1, 2, 31, 32, 33, 128, 512} and all((h * r // 4) % 256 for h, r in R.POOL_BWD)
    for v in R.ST_VARIANTS:
        for kind in ("left", "hole"):
            att = R.st_non_prefix(v, kind)["attention_mask"]
            assert not bool(((torch.arange(att.shape[1])[None, :] < att.sum(1)[:, None]).long() == att).all())


# ------------------------------------------------------------------------------------------------ float32 torch against the bounds
def _frac(got, ref, bound):
    d = (got.double() - ref).abs()
    assert bool((d[bound == 0] == 0).all())
    return float((d / bound.clamp(min=1e-300)).max())


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("H", R.POOL_H)
def test_float32_torch_within_half_of_the_mean_pool_bounds(H, packed):
    lens = list(R.POOL_LENS)
    x, row0, rs = R.pool_lengths_case(lens, H, packed, seed=H)
    ref, bound = R.mean_pool_fwd_ref(x, row0, lens)
    got = torch.stack([x[r:r + n].mean(0) if n else torch.zeros(H) for r, n in zip(row0, lens)])
    assert _frac(got, ref, bound) <= 0.5
    assert bool((ref[0] == 0).all()) and bool((bound[0] == 0).all())            # length 0: exactly zero
    if H % 4 == 0:
        g = torch.randn((len(lens), H), generator=torch.Generator().manual_seed(H + 1))
        dref, dbound = R.mean_pool_bwd_ref(g, rs, lens)
        n = torch.tensor(lens, dtype=torch.float32).clamp(min=1)
        dgot = torch.where((rs >= 0)[:, None], g[rs.long().clamp(min=0)] / n[rs.long().clamp(min=0)][:, None], torch.zeros(()))
        assert _frac(dgot, dref, dbound) <= 0.5


@pytest.mark.parametrize("hidden", R.NORM_HIDDEN)
@pytest.mark.parametrize("rows", R.NORM_ROWS)
def test_float32_torch_within_half_of_the_normalise_bounds(rows, hidden):
    x, g, where = R.normalize_case(rows, hidden, seed=rows * 10000 + hidden)
    y, norm, by, bn = R.l2_normalize_fwd_ref(x)
    xr = x.clone().requires_grad_(True)
    yt = torch.nn.functional.normalize(xr, p=2, dim=1)
    nt = x.norm(dim=1).clamp(min=1e-12)
    assert torch.isfinite(yt).all() and _frac(yt.detach(), y, by) <= 0.5
    assert _frac(nt, norm, bn) <= 0.5                       # (exact where the norm is clamped: _frac wants equality at bound 0)
    # the backward on float32 y and norm, as the kernel gets them: its formula in float32
    d = (g * yt.detach()).sum(1, keepdim=True)
    dx = (g - yt.detach() * d) / nt[:, None]
    dref, dbound = R.l2_normalize_bwd_ref(g, yt.detach(), nt)
    assert _frac(dx, dref, dbound) <= 0.5
    if "zero" in where:
        r = where["zero"]
        assert bool((y[r] == 0).all()) and float(norm[r]) == R.NORM_EPS and torch.equal(dref[r], g[r].double() / R.NORM_EPS)
    if "tiny" in where:
        assert float(norm[where["tiny"]]) == R.NORM_EPS and float(x[where["tiny"]].double().norm()) < 1e-12
    if "huge" in where:
        r = where["huge"]
        assert np.isfinite(np.float32((x[r] * x[r]).sum().item())) and float((x[r].double() ** 2).sum()) > 0.99 * R.FLT_MAX
    if "parallel" in where and hidden > 1:
        r = where["parallel"]
        assert float(dref[r].abs().max()) <= 1e-6 * float((g[r].double() / norm[r]).abs().max())       # a cancellation


# ------------------------------------------------------------------------------------------------ the yardsticks
def _held(measured, recorded, what):
    assert measured <= 1.05 * recorded, (what, measured, recorded)      # (5 %: the fp32 oracle's sums differ from host to host)
    assert measured >= 0.5 * recorded, (what, measured, recorded)      # the constant follows its measurement, not the other way round


def test_row_tolerances_are_three_times_the_measured_oracle_gap():
    lat = max(float(R.row_rel(R.oracle_latents(n, True), R.oracle_latents(n, False)).max()) for n in R.EVAL_CASES)
    prob = max(float((R.oracle_prob(n, True) - R.oracle_prob(n, False)).abs().max()) for n in R.EVAL_CASES)
    emb = max(float(R.row_rel(R.st_oracle(v, True), R.st_oracle(v, False)).max()) for v in R.ST_VARIANTS)
    print("\nmeasured: row latent %.4g  row embedding %.4g  probability %.4g" % (lat, emb, prob))
    _held(lat, R.YARD_ROW_LATENT, "latent")
    _held(emb, R.YARD_ROW_EMBED, "embedding")
    _held(prob, R.YARD_PROB, "probability")
    assert R.TOL_ROW_LATENT == 3 * R.YARD_ROW_LATENT and R.TOL_ROW_EMBED == 3 * R.YARD_ROW_EMBED and R.TOL_PROB == 3 * R.YARD_PROB


def test_oracle_pair_preds_goes_through_pair_latents():
    from oracle import carel_oracle as O
    name = "zh24_two"
    cfg, opt, _ = R.MODELS["zh24"]
    P, b = R.params("zh24"), R.case_batch(name)
    with torch.no_grad():
        p = O.pair_preds(P, b["input_ids"], b["attention_masks"], b["token_type_ids"], cfg, opt, *R.noise("zh24")).reshape(-1)
    assert float((p.double() - R.oracle_prob(name)).abs().max()) < 1e-5          # float32 head and sigmoid against the float64 ones


# ------------------------------------------------------------------------------------------------ packing arrays
@pytest.mark.parametrize("name", [n for n in R.EVAL_CASES if R.EVAL_CASES[n][0] != "zh32"])
def test_packing_arrays_equal_a_plain_loop(name):
    model, N, S, kind = R.EVAL_CASES[name]
    cfg = R.MODELS[model][0]
    m = M.DrlClassifier(M.make_opt(pair_bow_dim=8), M.encoder_config("en" if cfg.variant == "roberta" else "zh", vocab_size=cfg.vocab_size, layers=1), seed=1)
    b, lens = R.case_batch(name), R.case_lengths(name)
    for chunk in R.chunks_of(N):
        for s in range(0, N, chunk):
            ln = lens[s:s + chunk]
            c = m._prepare_inputs(b["input_ids"][s:s + chunk], b["attention_masks"][s:s + chunk], b["token_type_ids"][s:s + chunk], ln)
            assert c.B == len(ln) and c.S == S and (c.Bp * S) % 128 == 0
            if sum(ln) == len(ln) * S:
                assert c.pack is None            # nothing to skip: dense
                continue
            cu, tok = R.pack_arrays_loop(ln, c.Bp, S)
            assert c.pack.cu.tolist() == cu and c.pack.tok_row.tolist() == tok and (c.pack.t_eff, c.pack.n_tokens) == (sum(ln), len(tok))
