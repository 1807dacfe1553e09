"""The sentence-embedding evaluation path on the GPU: the four row kernels under SentenceTransformer.encode -- carel_mean_pool_fwd / _bwd,
carel_l2_normalize_fwd / _bwd (csrc/triplet.hip) -- against their float64 restatement, element by element, within the rounding-count
bounds of tests/eval_restate.py; `encode` with a batch loop that splits, against the oracle row by row (oracle/carel_oracle_st.py) and
against itself bitwise (slice and neighbour properties); attention masks that are not right-padded.

`pytest -s` prints the worst fraction of each bound / tolerance."""
import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import drl_classifier as M
from carel_vae_amd import sentence_transformer as S
from tests import eval_restate as R
from tests.gpu_util import bits

pytestmark = pytest.mark.gpu


def _frac(got, ref, bound):
    """worst |got - ref| / bound; where the bound is 0 the value must be exact"""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all())
    d = (got - ref).abs()
    assert bool((d[bound == 0] == 0).all())
    return float((d / bound.clamp(min=1e-300)).max())


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------ C.1 the row kernels against float64
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("H", R.POOL_H)
def test_mean_pool_forward_against_float64(H, packed):
    lens = list(R.POOL_LENS)
    x, row0, _ = R.pool_lengths_case(lens, H, packed, seed=H)
    assert all(r + n <= x.shape[0] for r, n in zip(row0, lens))                   # every read is inside x
    ref, bound = R.mean_pool_fwd_ref(x, row0, lens)
    out = torch.full((len(lens), H), float("nan"), device="cuda")
    xd, r0d, lnd = x.cuda(), _i32(row0), _i32(lens)                               # (held until the result is read)
    L.check(L.load().carel_mean_pool_fwd(xd.data_ptr(), r0d.data_ptr(), lnd.data_ptr(), len(lens), H, out.data_ptr(), L.current_stream()),
            "carel_mean_pool_fwd")
    f = _frac(out, ref, bound)
    print("\nmean_pool_fwd H=%d %s: %.3f of the bound" % (H, "packed" if packed else "dense", f))
    assert f <= 1.0
    assert bool((out[0] == 0).all())                                              # length 0: an all-zero row


@pytest.mark.parametrize("H,rows", R.POOL_BWD)
def test_mean_pool_backward_against_float64(H, rows):
    assert (rows * H // 4) % 256 != 0                                             # the last workgroup is partial
    gen = torch.Generator().manual_seed(H + rows)
    lens, left = [], rows - max(1, rows // 5)                                      # samples back to back, then filler rows (-1)
    while left > 0:
        lens.append(min(left, 1 + len(lens) * 3))
        left -= lens[-1]
    rs = torch.full((rows,), -1, dtype=torch.int32)
    o = 0
    for b, n in enumerate(lens):
        rs[o:o + n] = b
        o += n
    assert o < rows
    g = torch.randn((len(lens), H), generator=gen)
    ref, bound = R.mean_pool_bwd_ref(g, rs, lens)
    dx = torch.full((rows, H), float("nan"), device="cuda")
    gd, rsd, lnd = g.cuda(), rs.cuda(), _i32(lens)                                # (held until the result is read)
    L.check(L.load().carel_mean_pool_bwd(gd.data_ptr(), rsd.data_ptr(), lnd.data_ptr(), rows, H, dx.data_ptr(), L.current_stream()),
            "carel_mean_pool_bwd")
    assert not bool(torch.isnan(dx).any())                                        # every element was written
    assert bool((dx[o:] == 0).all())                                              # filler rows: exactly 0
    f = _frac(dx, ref, bound)
    print("\nmean_pool_bwd H=%d rows=%d: %.3f of the bound" % (H, rows, f))
    assert f <= 1.0


@pytest.mark.parametrize("hidden", R.NORM_HIDDEN)
@pytest.mark.parametrize("rows", R.NORM_ROWS)
def test_l2_normalize_forward_and_backward_against_float64(rows, hidden):
    lib = L.load()
    x, g, where = R.normalize_case(rows, hidden, seed=rows * 10000 + hidden)
    yr, nr, by, bn = R.l2_normalize_fwd_ref(x)
    xd, gd = x.cuda(), g.cuda()
    y = torch.full((rows, hidden), float("nan"), device="cuda")
    norm = torch.full((rows,), float("nan"), device="cuda")
    L.check(lib.carel_l2_normalize_fwd(xd.data_ptr(), rows, hidden, y.data_ptr(), norm.data_ptr(), L.current_stream()), "carel_l2_normalize_fwd")
    fy, fn = _frac(y, yr, by), _frac(norm, nr, bn)
    # the backward is judged on the y and norm it is given: the forward kernel's float32 outputs
    dr, bd = R.l2_normalize_bwd_ref(g, y.cpu(), norm.cpu())
    dx = torch.full((rows, hidden), float("nan"), device="cuda")
    L.check(lib.carel_l2_normalize_bwd(gd.data_ptr(), y.data_ptr(), norm.data_ptr(), rows, hidden, dx.data_ptr(), L.current_stream()), "carel_l2_normalize_bwd")
    fd = _frac(dx, dr, bd)
    print("\nl2_normalize rows=%d hidden=%d %s: y %.3f  norm %.3f  dx %.3f of the bound" % (rows, hidden, sorted(where), fy, fn, fd))
    assert fy <= 1.0 and fn <= 1.0 and fd <= 1.0
    yc, nc, dc = y.cpu(), norm.cpu(), dx.cpu()
    if "zero" in where:                    # torch.nn.functional.normalize: y = 0 / 1e-12, dx = g / 1e-12
        r = where["zero"]
        assert bool((yc[r] == 0).all()) and float(nc[r]) == R.NORM_EPS
        assert float(((dc[r].double() - g[r].double() / R.NORM_EPS).abs() / (g[r].double().abs() / R.NORM_EPS * 2 * R.U + R.DENORM)).max()) <= 1.0
    if "tiny" in where:
        assert float(nc[where["tiny"]]) == R.NORM_EPS
    if "huge" in where:
        assert bool(torch.isfinite(nc[where["huge"]])) and float(nc[where["huge"]]) > 1e19 / 1.01
    if "parallel" in where and hidden > 1:  # a cancellation: what is left is rounding, on the scale of g / norm
        r = where["parallel"]
        assert float(dc[r].abs().max()) <= 1e-5 * float((g[r] / nc[r]).abs().max())


# ------------------------------------------------------------------------------------------------ C.2 encode with a splitting batch loop
_st = {}


def st_model(variant):
    """(model, embeddings at batch_size 37) per variant, built once: oracle weights (init_params) in a 2-layer encoder, max_seq_length 32."""
    if variant not in _st:
        cfg = R.ST_VARIANTS[variant]
        mcfg = M.encoder_config("mpnet" if variant == "mpnet" else "zh", vocab_size=cfg.vocab_size, layers=cfg.layers, hidden_dropout=0.0, attn_dropout=0.0)
        model = S.SentenceTransformer(mcfg, max_seq_length=R.ST_S)
        model.load_state_dict({model._to_public(k[len("encoder."):]): v for k, v in R.st_params(variant).items()
                               if k.startswith("encoder.") and not (variant == "mpnet" and "token_type" in k)})
        model.to("cuda")
        _st[variant] = (model, model.encode(dict(R.st_features(variant)), batch_size=R.ST_N, convert_to_numpy=False).clone())
    return _st[variant]


@pytest.mark.parametrize("batch_size", R.ST_BATCH_SIZES)
@pytest.mark.parametrize("variant", list(R.ST_VARIANTS))
def test_encode_rows_against_the_oracle_at_every_batch_size(variant, batch_size):
    model, _ = st_model(variant)
    feats = R.st_features(variant)
    got = model.encode(dict(feats), batch_size=batch_size, convert_to_numpy=False)
    assert got.shape == (R.ST_N, 768) and model.normalize == (variant == "mpnet")
    worst = {}
    for emu in (False, True):
        rel = R.row_rel(got, R.st_oracle(variant, emu))
        worst[emu] = float(rel.max())
        assert worst[emu] <= R.TOL_ROW_EMBED, (variant, batch_size, emu, int(rel.argmax()), worst[emu])
    print("\nencode %s batch_size=%d: worst row %.3f (fp32) %.3f (bf16_round) of TOL_ROW_EMBED" % (
        variant, batch_size, worst[False] / R.TOL_ROW_EMBED, worst[True] / R.TOL_ROW_EMBED))
    if variant == "mpnet":
        assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-6
    # slice: rows [s, s + batch_size) of the whole call are the call on that slice alone -- same launch shapes, bit for bit
    for s in range(0, R.ST_N, batch_size):
        alone = model.encode({k: v[s:s + batch_size] for k, v in feats.items()}, batch_size=batch_size, convert_to_numpy=False)
        assert torch.equal(bits(got[s:s + batch_size]), bits(alone)), (variant, batch_size, s)


@pytest.mark.parametrize("batch_size", (37, 5))
@pytest.mark.parametrize("variant", list(R.ST_VARIANTS))
def test_encode_rows_do_not_depend_on_their_neighbours(variant, batch_size):
    """Every second sentence replaced by another of the same length: the untouched sentences' embeddings keep their bits."""
    model, _ = st_model(variant)
    feats = {k: v.clone() for k, v in R.st_features(variant).items()}
    base = model.encode(dict(feats), batch_size=batch_size, convert_to_numpy=False)
    cfg = R.ST_VARIANTS[variant]
    rs = np.random.RandomState(77)
    for b in range(1, R.ST_N, 2):
        n = int(feats["attention_mask"][b].sum())
        feats["input_ids"][b, :n] = torch.from_numpy(rs.randint(2, cfg.vocab_size, size=n))
    got = model.encode(feats, batch_size=batch_size, convert_to_numpy=False)
    assert torch.equal(bits(got[0::2]), bits(base[0::2]))
    assert not torch.equal(got[1::2], base[1::2])                                # (the replaced ones did change)


# ------------------------------------------------------------------------------------------------ C.3 masks that are not prefixes
@pytest.mark.parametrize("kind", ["left", "hole"])
@pytest.mark.parametrize("variant", list(R.ST_VARIANTS))
def test_encode_with_a_mask_that_is_no_prefix_is_exact_or_refused(variant, kind):
    """Packing and the pooling kernel read the FIRST sum(mask) tokens of a sentence.  A left-padded mask or one with a hole must either
    give the masked mean of the oracle (ST.mean_pool weights by the mask) or be refused; this build refuses."""
    model, _ = st_model(variant)
    feats = R.st_non_prefix(variant, kind)
    try:
        got = model.encode(dict(feats), batch_size=8, convert_to_numpy=False)
    except L.CarelError as e:
        assert "right-padded" in str(e)
    else:
        rel = R.row_rel(got, R.st_encode(variant, feats, True))
        assert float(rel.max()) <= R.TOL_ROW_EMBED, (variant, kind, float(rel.max()))
    # the same sentences right-padded are accepted, and lengths given by the caller are taken at their word (documented: no read-back)
    ok = {k: v[:8] for k, v in R.st_features(variant).items()}
    assert model.encode(ok, batch_size=8, convert_to_numpy=False).shape == (8, 768)
