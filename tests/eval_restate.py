"""The evaluation paths -- DrlClassifier.pair_latents / pair_probabilities / get_pair_preds, the three-space pair_logits and
SentenceTransformer.encode -- and the four row kernels under encode (carel_mean_pool_fwd / _bwd, carel_l2_normalize_fwd / _bwd,
csrc/triplet.hip): TEST INFRASTRUCTURE shared by tests/test_eval_restate_host.py (CPU), tests/test_gpu_eval_paths.py and
tests/test_gpu_pool_sweep.py.  Nothing here touches the GPU or the library.

(1) The row kernels restated in float64, with a bound per element.  Every bound is a count of roundings x 2^-24 x the scale of the
    sum the rounding happens on (U = 2^-24 is the unit round-off of float32):
      mean pool forward   s = x_0 + ... + x_{n-1} one column at a time, then s * (1 / n): n additions, the reciprocal, one multiply
                          -> (n + 2) U sum_t |x_t| / n.  n = 0: the row is exactly 0.
      mean pool backward  g * (1 / n): the reciprocal and one multiply -> 2 U |g| / n; rows of no sample are exactly 0.
      normalise forward   s = sum x^2: one product, ceil(hidden / 256) additions in a thread, 6 butterfly levels, 4 wave sums: NORM_CHAIN
                          roundings, all terms positive, so relative to s; the square root halves that and adds its own:
                          norm (NORM_CHAIN / 2 + 2) U norm, y = x / norm two more (below).  norm is clamped at float32(1e-12), where it is
                          exact.
      normalise backward  d = sum g y has NORM_CHAIN roundings of sum |g y|; dx = (g - y d) / norm adds the product, the subtraction
                          and the division: (|y| NORM_CHAIN sum|g y| + 2 |y d| + 4 |g - y d|) U / norm.  Where g is parallel to y the
                          exact dx is a cancellation and this bound stays on the scale of g / norm, which is what is meant.
    Outside a summation chain an elementary operation is budgeted TWO roundings: its own, and one for the ways it may be evaluated (a / b
    as a * (1 / b), which the mean pool itself does; a square root through a reciprocal square root; a product and a difference fused or
    not).  Stock float32 torch, which evaluates each of them once, therefore stays within half of every bound, and the host test says so.
    Below the float32 normal range (|value| < 2^-126) nothing relative holds: every bound adds 2^-149, one denormal step.

(2) The cases of the evaluation paths (EVAL_CASES, ST_VARIANTS), their parameters (oracle init_params; the pair head rescaled by
    `calibrate` so that the ORACLE's probabilities fall on both sides of 0.5) and the oracle outputs, computed once per process.

(3) The per-row tolerances.  YARD_* are MEASURED on the CPU, oracle against oracle (tests/test_eval_restate_host.py measures them
    again and holds the constants to the measurement): the worst row of |fp32 oracle - bf16_round oracle| / |fp32 oracle| over all
    cases.  TOL_* = 3 x YARD_*: the kernels round at the storage points the emulation rounds at, but sum in other orders (the
    whole-tensor constants of test_gpu_model.py sit 1.5 to 8 times above their measured values for the same reason).
"""
import functools
import math

import numpy as np
import torch

from carel_vae_amd import data as D
from oracle import carel_oracle as O
from oracle import carel_oracle_st as ST

U = 2.0 ** -24
DENORM = 2.0 ** -149
NORM_EPS = float(np.float32(1e-12))          # what fmaxf(sqrtf(s), 1e-12f) clamps at
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------ (1) the row kernels in float64
def mean_pool_fwd_ref(x, row0, lens):
    """x [rows, H] -> (out [B, H], bound [B, H]) float64: the mean of rows row0[b] .. row0[b] + lens[b] - 1 (0 for an empty sample)."""
    x = x.double()
    out = torch.zeros((len(lens), x.shape[1]), dtype=torch.float64)
    bound = torch.zeros_like(out)
    for b, (r, n) in enumerate(zip(row0, lens)):
        if n > 0:
            out[b] = x[r:r + n].sum(0) / n
            bound[b] = (n + 2) * U * x[r:r + n].abs().sum(0) / n + DENORM
    return out, bound


def mean_pool_bwd_ref(g, row_sample, lens):
    """g [B, H], row_sample [rows] (-1: a row of no sample) -> (dx [rows, H], bound) float64: g[b] / lens[b] on the rows of sample b."""
    g = g.double()
    rs = torch.as_tensor(row_sample, dtype=torch.long)
    n = torch.as_tensor(lens, dtype=torch.float64).clamp(min=1.0)
    live = (rs >= 0).to(torch.float64)[:, None]
    idx = rs.clamp(min=0)
    dx = g[idx] / n[idx][:, None] * live
    return dx, (2 * U * dx.abs() + DENORM) * live


def norm_chain(hidden):
    return -(-hidden // 256) + 1 + 6 + 4


def l2_normalize_fwd_ref(x):
    """x [rows, hidden] -> (y, norm, bound_y, bound_norm) float64: torch.nn.functional.normalize(p=2, dim=1, eps=1e-12) and the norm it
    divides by."""
    x = x.double()
    k = norm_chain(x.shape[1])
    raw = (x * x).sum(1).sqrt()
    norm = raw.clamp(min=NORM_EPS)
    rel = torch.where(raw < NORM_EPS * (1 - k * U), torch.zeros_like(raw), torch.full_like(raw, (k / 2 + 2) * U))     # clamped: exact
    y = x / norm[:, None]
    return y, norm, (rel[:, None] + 2 * U) * y.abs() + DENORM, rel * norm


def l2_normalize_bwd_ref(g, y, norm):
    """dx = (g - y (y . g)) / norm from the float32 y and norm the forward kernel left (so the backward is judged on its own inputs)."""
    g, y, norm = g.double(), y.double(), norm.double()[:, None]
    k = norm_chain(g.shape[1])
    d = (g * y).sum(1, keepdim=True)
    r = g - y * d
    bound = (y.abs() * k * (g * y).abs().sum(1, keepdim=True) + 2 * (y * d).abs() + 4 * r.abs()) * U / norm + DENORM
    return r / norm, bound


def largest_finite_row(hidden, gen):
    """A normal draw scaled to the largest magnitude at which its float32 sum of squares stays finite: sum x^2 = FLT_MAX (1 - 2^-10), well
    outside the NORM_CHAIN roundings of the sum."""
    r = torch.randn(hidden, generator=gen).double()
    r = torch.where(r.abs() < 1e-3, torch.ones_like(r), r)
    return (r * math.sqrt(FLT_MAX * (1 - 2.0 ** -10) / float((r * r).sum()))).float()


def pool_lengths_case(lens, H, packed, seed):
    """x, row0, row_sample of a mean-pool case: packed = samples back to back (row0 the running sums) then filler rows; dense = sample b
    at row b * S with S = max(lens) rounded up to 32."""
    g = torch.Generator().manual_seed(seed)
    S = max(32, (max(lens) + 31) // 32 * 32)
    if packed:
        row0 = [int(v) for v in np.cumsum([0] + list(lens[:-1]))]
        rows = (sum(lens) + 127) // 128 * 128
    else:
        row0 = [b * S for b in range(len(lens))]
        rows = len(lens) * S
    rows = max(rows, 1)
    x = torch.randn((rows, H), generator=g) * torch.rand((rows, 1), generator=g).mul(3).exp()
    rs = torch.full((rows,), -1, dtype=torch.int32)
    for b, (r, n) in enumerate(zip(row0, lens)):
        rs[r:r + n] = b
    return x, row0, rs


POOL_H = (1, 4, 260, 768, 1028)
POOL_LENS = (0, 1, 2, 31, 32, 33, 128, 512)
POOL_BWD = ((4, 37), (260, 5), (768, 3), (768, 131))          # (H, rows): rows * H / 4 is no multiple of 256
NORM_ROWS = (1, 3, 65)
NORM_HIDDEN = (1, 63, 64, 65, 256, 257, 768, 1025)


def normalize_case(rows, hidden, seed):
    """x, g [rows, hidden] and the names of the designed rows.  Every case has the four edge rows where it has the rows for them (the
    one-row case cycles through them by hidden): zero, tiny (norm < 1e-12), huge (largest finite sum of squares), parallel (g = 3 y)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, hidden), generator=gen) * torch.rand((rows, 1), generator=gen).mul(4).sub(2).exp()
    g = torch.randn((rows, hidden), generator=gen)
    kinds = ["zero", "tiny", "huge", "parallel"]
    where = {}
    if rows == 1:
        where[kinds[NORM_HIDDEN.index(hidden) % 4]] = 0
    elif rows == 3:
        where = {kinds[(NORM_HIDDEN.index(hidden) + i) % 4]: i for i in range(3)}
    else:
        where = {"zero": 1, "tiny": 7, "huge": 63, "parallel": 64}
    for kind, r in where.items():
        if kind == "zero":
            x[r] = 0.0
        elif kind == "tiny":
            x[r] = torch.randn(hidden, generator=gen) * 1e-14
        elif kind == "huge":
            x[r] = largest_finite_row(hidden, gen)
        else:
            g[r] = 3.0 * x[r] / x[r].double().norm().clamp(min=1e-30).float()
    return x, g, where


# ------------------------------------------------------------------------------------------------ (2) the evaluation cases
VOCAB, V = 300, 64
MODELS = {
    "zh24": (O.EncoderConfig(layers=2, vocab_size=VOCAB), O.Opt(pair_bow_dim=V, ec_dim=24, dropout=0.0), 21),
    "zh32": (O.EncoderConfig(layers=2, vocab_size=VOCAB), O.Opt(pair_bow_dim=V, ec_dim=32, dropout=0.0), 22),
    "en24": (O.EncoderConfig(layers=2, vocab_size=VOCAB, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="roberta", pad_id=1),
             O.Opt(language="en", pair_bow_dim=V, ec_dim=24, dropout=0.0), 23),
}
NS = (1, 5, 127, 128, 129, 300)
PAIR_SCALE = 8.0           # what `calibrate` multiplies pair_classifier.weight by
FAR = 2e-2                 # a row is "far" when |p - 0.5| > FAR (test_get_pair_preds_and_cpu_refusal)


def chunks_of(N):
    return sorted({N, 128, 8} | ({1} if N == 5 else set()))


def _first_id(cfg):
    return 2 if cfg.pad_id == 1 else 1


def batch_with_lengths(lens, S, cfg, seed):
    """ids / mask / token types [len(lens), S] with the given attended prefix lengths: [CLS]-like id first, random ids, pad_id after."""
    rs = np.random.RandomState(seed)
    n = len(lens)
    ids = rs.randint(_first_id(cfg), cfg.vocab_size, size=(n, S)).astype(np.int64)
    att = (np.arange(S)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)
    ids[att == 0] = cfg.pad_id
    tt = np.zeros((n, S), dtype=np.int64)
    if cfg.type_vocab > 1:                                # the second half of every sentence is segment 1
        for b, ln in enumerate(lens):
            tt[b, ln // 2:ln] = 1
    t = torch.from_numpy
    return dict(input_ids=t(ids), attention_masks=t(att), token_type_ids=t(tt))


def _mix_lengths(N, S):
    cyc = [2, S, 3, S - 1, 17, S, 2, 9, S // 2, S - 2, 5]
    return [cyc[i % len(cyc)] for i in range(N)]


# name -> (model, N, S, kind).  "B": the first N rows of ONE 300-row D.synthetic_ecpe_batch(shape="B") per (model, S), so the oracle runs
# once; the others are hand-set lengths.
EVAL_CASES = {}
for _n in NS:
    EVAL_CASES["zh24_B_%d" % _n] = ("zh24", _n, 32, "B")
EVAL_CASES.update({
    "zh24_two": ("zh24", 5, 32, "two"),                  # only [CLS] and [SEP]
    "zh24_full": ("zh24", 5, 32, "full"),                # exactly S: nothing to pack
    "zh24_mix": ("zh24", 129, 32, "mix"),
    "zh24_lastfull": ("zh24", 129, 32, "lastfull"),      # row 128 (the last chunk at chunk 128 and at chunk 8) is full-length: dense after packed chunks
    "zh24_s64_mix": ("zh24", 9, 64, "mix"),
    "zh32_B_129": ("zh32", 129, 32, "B"),
    "en24_B_129": ("en24", 129, 32, "B"),
    "en24_mix": ("en24", 5, 32, "mix"),
})


def case_lengths(name):
    model, N, S, kind = EVAL_CASES[name]
    if kind == "B":
        return [int(v) for v in case_batch(name)["attention_masks"].sum(1)]
    if kind == "two":
        return [2] * N
    if kind == "full":
        return [S] * N
    if kind == "mix":
        return _mix_lengths(N, S)
    lens = [3 + (7 * i) % (S - 4) for i in range(N)]     # lastfull: everything before the last chunk is shorter than S
    lens[128:] = [S] * (N - 128)
    return lens


@functools.lru_cache(maxsize=None)
def _base_batch(model, S):
    cfg = MODELS[model][0]
    return D.synthetic_ecpe_batch(max(NS), S, cfg.vocab_size, V, seed=100 + S + MODELS[model][2], shape="B", pad_id=cfg.pad_id, first_id=_first_id(cfg))


@functools.lru_cache(maxsize=None)
def case_batch(name):
    """dict of CPU tensors (ids, mask, token types; for "B" cases the labels and bag of words too)."""
    model, N, S, kind = EVAL_CASES[name]
    if kind == "B":
        return {k: v[:N] for k, v in _base_batch(model, S).items()}
    return batch_with_lengths(case_lengths(name), S, MODELS[model][0], seed=7 + len(name) + N)


def _ids(b):
    return b["input_ids"], b["attention_masks"], b["token_type_ids"]


@functools.lru_cache(maxsize=None)
def noise(model):
    g = torch.Generator().manual_seed(1000 + MODELS[model][2])
    d = MODELS[model][1].ec_dim
    return torch.randn(d, generator=g), torch.randn(d, generator=g)


def _raw_latents(P, name, quant):
    model, N, S, kind = EVAL_CASES[name]
    cfg, opt, _ = MODELS[model]
    with torch.no_grad():
        if kind == "B":                                    # one oracle pass over the 300 rows serves every N
            return _base_latents(model, S, quant is not None)[:N]
        return O.pair_latents(P, *_ids(case_batch(name)), cfg, opt, quant=quant)


@functools.lru_cache(maxsize=None)
def _base_latents(model, S, emu):
    cfg, opt, seed = MODELS[model]
    with torch.no_grad():
        return O.pair_latents(O.init_params(cfg, opt, seed=seed), *_ids(_base_batch(model, S)), cfg, opt, quant=O.bf16_round if emu else None)


def pair_logit(lat, P, eps_e, eps_c):
    """float64 logits of the pair head on latents [N, 4 D] (reference :277-281: z = mu + eps * exp(log_var), no 1/2)."""
    mu_e, lv_e, mu_c, lv_c = lat.double().split(lat.shape[1] // 4, dim=1)
    z = torch.cat((mu_e + eps_e.double() * lv_e.exp(), mu_c + eps_c.double() * lv_c.exp()), dim=1)
    return (z @ P["pair_classifier.weight"].double().t() + P["pair_classifier.bias"].double()).reshape(-1)


def pair_prob(lat, P, eps_e, eps_c):
    return torch.sigmoid(pair_logit(lat, P, eps_e, eps_c))


def calibrate(P, lat, eps_e, eps_c, scale=PAIR_SCALE):
    """pair_classifier.weight *= scale, bias = -(median logit of `lat` under the scaled weight): from the ORACLE's latents alone, so
    that its probabilities fall on both sides of 0.5 and away from it.  Returns a new parameter dict."""
    Q = dict(P)
    Q["pair_classifier.weight"] = P["pair_classifier.weight"] * scale
    Q["pair_classifier.bias"] = torch.zeros_like(P["pair_classifier.bias"])
    med = pair_logit(lat, Q, eps_e, eps_c).median()
    Q["pair_classifier.bias"] = torch.full_like(P["pair_classifier.bias"], -float(med))
    return Q


@functools.lru_cache(maxsize=None)
def params(model):
    """init_params with the pair head calibrated on the fp32 oracle's latents of the model's 300-row batch at S = 32."""
    cfg, opt, seed = MODELS[model]
    return calibrate(O.init_params(cfg, opt, seed=seed), _base_latents(model, 32, False), *noise(model))


@functools.lru_cache(maxsize=None)
def oracle_latents(name, emu):
    """[N, 4 D] float32 of the fp32 oracle (emu False) or the oracle that rounds to bf16 where the kernels store bf16 (emu True)."""
    return _raw_latents(params(EVAL_CASES[name][0]), name, O.bf16_round if emu else None)


def oracle_prob(name, emu=False):
    model = EVAL_CASES[name][0]
    return pair_prob(oracle_latents(name, emu), params(model), *noise(model))


def row_rel(got, ref):
    """per row: |got - ref| / |ref| (float64, CPU)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).norm(dim=1) / ref.norm(dim=1).clamp(min=1e-30)


# ---- sentence embeddings: N = 37 sentences, max_seq_length 32, lengths 2 and 32 among them
ST_N, ST_S = 37, 32
ST_BATCH_SIZES = (37, 16, 5, 1)
ST_VARIANTS = {
    "bert": O.EncoderConfig(layers=2, vocab_size=VOCAB),
    "mpnet": O.EncoderConfig(layers=2, vocab_size=VOCAB, max_pos=514, type_vocab=1, ln_eps=1e-5, variant="mpnet", pad_id=1, rel_pos=True),
}
ST_SEED = 5


def st_lengths():
    rs = np.random.RandomState(11)
    lens = [int(v) for v in rs.randint(2, ST_S + 1, size=ST_N)]
    lens[0], lens[1], lens[17], lens[36] = 2, ST_S, ST_S, 2
    return lens


@functools.lru_cache(maxsize=None)
def st_params(variant):
    return O.init_params(ST_VARIANTS[variant], O.Opt(pair_bow_dim=8), seed=ST_SEED)


@functools.lru_cache(maxsize=None)
def st_features(variant):
    b = batch_with_lengths(st_lengths(), ST_S, ST_VARIANTS[variant], seed=31)
    tt = b["token_type_ids"] if variant == "bert" else torch.zeros_like(b["token_type_ids"])
    return {"input_ids": b["input_ids"], "attention_mask": b["attention_masks"], "token_type_ids": tt}


def st_encode(variant, feats, emu):
    with torch.no_grad():
        return ST.encode(st_params(variant), feats["input_ids"], feats["attention_mask"], feats["token_type_ids"], ST_VARIANTS[variant],
                         quant=O.bf16_round if emu else None)


@functools.lru_cache(maxsize=None)
def st_oracle(variant, emu):
    return st_encode(variant, st_features(variant), emu)


def st_non_prefix(variant, kind):
    """The features of the first 8 sentences with a mask that is no prefix: "left" = the attended tokens moved to the right end
    (left padding), "hole" = position 1 of every sentence of 4 or more tokens masked out."""
    f = {k: v[:8].clone() for k, v in st_features(variant).items()}
    pad = ST_VARIANTS[variant].pad_id
    if kind == "left":
        for b, n in enumerate(st_lengths()[:8]):
            for k, fill in (("input_ids", pad), ("attention_mask", 0), ("token_type_ids", 0)):
                row = f[k][b].clone()
                f[k][b] = fill
                f[k][b, ST_S - n:] = row[:n]
    else:
        for b, n in enumerate(st_lengths()[:8]):
            if n >= 4:
                f["attention_mask"][b, 1] = 0
    return f


# ------------------------------------------------------------------------------------------------ (3) measured yardsticks, tolerances
# worst row of |fp32 oracle - bf16_round oracle| / |fp32 oracle| over EVAL_CASES (latents) and ST_VARIANTS (embeddings), and the worst
# |p_fp32 - p_bf16emu| over EVAL_CASES under the calibrated pair heads: measured by tests/test_eval_restate_host.py, which fails when a
# figure here is more than 5 % below its measurement or more than twice above it.
# The fp32 oracle's own sums depend on the host's BLAS: two hosts gave 2.438e-3 and 2.489e-3 for the latents (the other two figures
# agreed to four digits), so the host test allows a measurement 5 % above the figure recorded here.
YARD_ROW_LATENT = 2.50e-3        # measured 2.438e-3 / 2.489e-3 (zh24_lastfull); the other cases 1.73e-3 .. 2.44e-3
YARD_ROW_EMBED = 2.40e-3         # measured 2.374e-3 (mpnet), 2.328e-3 (bert)
YARD_PROB = 2.55e-3              # measured 2.528e-3 (zh24_two) at PAIR_SCALE 8; 3 x this stays below FAR
# TOL_ROW_LATENT (7.5e-3) is tighter per row than TOL_LATENT_BF16 (1e-2) of test_gpu_model.py is for a whole tensor.
TOL_ROW_LATENT = 3 * YARD_ROW_LATENT
TOL_ROW_EMBED = 3 * YARD_ROW_EMBED
TOL_PROB = 3 * YARD_PROB


# ------------------------------------------------------------------------------------------------ packing arrays, as a plain loop
def pack_arrays_loop(lens, Bp, S):
    """cu [Bp + 1] and tok_row [tokens rounded up to 128] of DrlClassifier._pack_info, written as a loop: sample b's tokens are rows
    cu[b] .. cu[b + 1] - 1 and row r holds position tok_row[r] = b * S + t of the padded batch; filler samples are empty, filler rows -1."""
    cu, tok = [0], []
    for b, n in enumerate(lens):
        for t in range(n):
            tok.append(b * S + t)
        cu.append(cu[-1] + n)
    while len(cu) < Bp + 1:
        cu.append(cu[-1])
    while len(tok) % 128:
        tok.append(-1)
    return cu, tok
