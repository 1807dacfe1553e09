"""The batch triplet loss family of the `sentence_transformers` package (2.x: losses.BatchSemiHardTripletLoss, BatchAllTripletLoss,
BatchHardTripletLoss, BatchHardSoftMarginTripletLoss with BatchHardTripletLossDistanceFunction) restated twice in float64 -- TEST
INFRASTRUCTURE for tests/test_triplet_family_host.py and tests/test_gpu_triplet_family.py.  PARITY UNPINNED: the package is not
installed; what follows restates its published algorithm.

  (i)  published(...): the four losses vectorised the way the package writes them, on torch tensors, so autograd gives the gradient.
  (ii) restate(...): the same losses from their definitions (include/carel_hip.h), one anchor at a time in NumPy, with the
       lowest-index tie rule, an analytic gradient, the three counts and `min_gap`: the smallest non-zero |lhs - rhs| over the
       comparisons that decide the result -- a distance against the distance it is selected against or over, and a hinge argument l
       against 0 (batch-all: also against 1e-16).  A selection or hinge flip in fp32 moves a gradient by whole triplets without any
       kernel being wrong, so the GPU inputs (CASES) are chosen so that min_gap is far above fp32 rounding.
"""
import numpy as np
import torch

MODES = ("semihard", "all", "hard", "hard_soft")           # the kernel's mode numbers 0..3
EUCLIDEAN, DOT, COSINE = "euclidean", "dot", "cosine"       # DOT = 1 - e_i.e_j on the rows as given (the kernel's distance 1)


# ------------------------------------------------------------------------------------------------ (i) as published, torch
def euclidean_distance(emb):
    dot = emb @ emb.t()
    sq = torch.diag(dot)
    d = sq.unsqueeze(0) - 2.0 * dot + sq.unsqueeze(1)
    d = torch.where(d < 0, torch.zeros_like(d), d)
    mask = d.eq(0).to(d.dtype)
    return (1.0 - mask) * torch.sqrt(d + mask * 1e-16)


def cosine_distance(emb):
    n = torch.nn.functional.normalize(emb, p=2, dim=1)
    return 1 - n @ n.t()


def dot_distance(emb):
    return 1 - emb @ emb.t()


DISTANCES = {EUCLIDEAN: euclidean_distance, DOT: dot_distance, COSINE: cosine_distance}


def _anchor_positive_mask(labels):
    return (labels.unsqueeze(0) == labels.unsqueeze(1)) & ~torch.eye(labels.numel(), dtype=torch.bool)


def _anchor_negative_mask(labels):
    return ~(labels.unsqueeze(0) == labels.unsqueeze(1))


def _triplet_mask(labels):
    ne = ~torch.eye(labels.numel(), dtype=torch.bool)
    distinct = ne.unsqueeze(2) & ne.unsqueeze(1) & ne.unsqueeze(0)
    eq = labels.unsqueeze(0) == labels.unsqueeze(1)
    return (eq.unsqueeze(2) & ~eq.unsqueeze(1)) & distinct


def _masked_minimum(data, mask, dim=1):
    axis_max = data.max(dim, keepdim=True)[0]
    return ((data - axis_max) * mask).min(dim, keepdim=True)[0] + axis_max


def _masked_maximum(data, mask, dim=1):
    axis_min = data.min(dim, keepdim=True)[0]
    return ((data - axis_min) * mask).max(dim, keepdim=True)[0] + axis_min


def _published_semihard(pd, labels, margin):
    labels = labels.reshape(-1, 1)
    adj = labels == labels.t()
    adj_not = ~adj
    B = labels.numel()
    tile = pd.repeat([B, 1])
    mask = adj_not.repeat([B, 1]) & (tile > pd.t().reshape(-1, 1))
    mask_final = (mask.to(pd.dtype).sum(1, keepdim=True) > 0.0).reshape(B, B).t()
    neg_outside = _masked_minimum(tile, mask.to(pd.dtype)).reshape(B, B).t()
    neg_inside = _masked_maximum(pd, adj_not.to(pd.dtype)).repeat([1, B])
    semi_hard = torch.where(mask_final, neg_outside, neg_inside)
    loss_mat = (pd - semi_hard) + margin
    mask_pos = adj.to(pd.dtype) - torch.eye(B, dtype=pd.dtype)
    return torch.clamp(loss_mat * mask_pos, min=0.0).sum() / mask_pos.sum()


def _published_all(pd, labels, margin):
    tl = pd.unsqueeze(2) - pd.unsqueeze(1) + margin
    tl = _triplet_mask(labels).to(pd.dtype) * tl
    tl = torch.where(tl < 0, torch.zeros_like(tl), tl)
    num_positive = int((tl > 1e-16).sum())
    return tl.sum() / (num_positive + 1e-16)


def _published_hard_terms(pd, labels):
    ap = _anchor_positive_mask(labels).to(pd.dtype)
    hardest_positive = (ap * pd).max(1, keepdim=True)[0]
    an = _anchor_negative_mask(labels).to(pd.dtype)
    max_dist = pd.max(1, keepdim=True)[0]
    hardest_negative = (pd + max_dist * (1.0 - an)).min(1, keepdim=True)[0]
    return hardest_positive, hardest_negative


def _published_hard(pd, labels, margin):
    hp, hn = _published_hard_terms(pd, labels)
    tl = hp - hn + margin
    return torch.where(tl < 0, torch.zeros_like(tl), tl).mean()


def _published_hard_soft(pd, labels, margin):
    hp, hn = _published_hard_terms(pd, labels)
    return torch.log1p(torch.exp(hp - hn)).mean()


_PUBLISHED = {"semihard": _published_semihard, "all": _published_all, "hard": _published_hard, "hard_soft": _published_hard_soft}


def published(mode, distance, emb, labels, margin):
    """emb: torch [B, H] (float64 in the tests; may require grad), labels: torch int [B] -> the loss, a 0-dim tensor."""
    return _PUBLISHED[mode](DISTANCES[distance](emb), labels.reshape(-1), margin)


# ------------------------------------------------------------------------------------------------ (ii) from the definitions, NumPy
class _Gap:
    """the smallest non-zero |lhs - rhs| seen"""

    def __init__(self):
        self.v = np.inf

    def see(self, diff):
        d = np.abs(np.asarray(diff, dtype=np.float64)).ravel()
        d = d[d > 0]
        if d.size:
            self.v = min(self.v, float(d.min()))


def distance_matrix(distance, e):
    """e float64 [B, H] -> (D, n, norm): n, norm = the normalised rows and clamped norms for COSINE (else None)."""
    if distance == EUCLIDEAN:
        sq = (e * e).sum(1)
        d2 = sq[:, None] - 2.0 * (e @ e.T) + sq[None, :]
        D = np.where(d2 <= 0, 0.0, np.sqrt(np.maximum(d2, 0.0)))
        np.fill_diagonal(D, 0.0)
        return D, None, None
    if distance == DOT:
        return 1.0 - e @ e.T, None, None
    norm = np.maximum(np.sqrt((e * e).sum(1)), 1e-12)
    n = e / norm[:, None]
    return 1.0 - n @ n.T, n, norm


def restate(mode, distance, emb, labels, margin=0.0):
    """-> dict(loss, grad [B, H], counts (positive pairs, valid triplets, active terms), min_gap, D, W): float64 throughout; W is
    d loss / d D (normalised).  active: hinge terms > 0 (semihard: pairs, hard: anchors), the package's P (all), B (hard_soft)."""
    e = np.asarray(emb, dtype=np.float64)
    lab = np.asarray(labels).reshape(-1)
    B = e.shape[0]
    D, n_rows, norm = distance_matrix(distance, e)
    Wc = np.zeros((B, B))                  # d (sum of the terms) / d D
    gap = _Gap()
    total, n_pairs, n_valid, n_active = 0.0, 0, 0, 0
    idx = np.arange(B)
    for a in range(B):
        row = D[a]
        neg_m = lab != lab[a]
        pos_m = ~neg_m & (idx != a)
        pos, neg = idx[pos_m], idx[neg_m]
        n_pairs += pos.size
        n_valid += pos.size * neg.size
        if mode == "semihard":
            if pos.size == 0:
                continue
            dap, dn = row[pos], row[neg]
            if neg.size == 0:
                dneg, sel = np.zeros(pos.size), np.full(pos.size, -1)
            else:
                out = dn[None, :] > dap[:, None]
                gap.see(dn[None, :] - dap[:, None])
                masked = np.where(out, dn[None, :], np.inf)
                kmin = masked.argmin(1)                       # first occurrence = lowest index (neg is ascending)
                kmax = int(dn.argmax())
                has = out.any(1)
                vmin = masked[np.arange(pos.size), kmin]
                gap.see(np.where(out, dn[None, :] - np.where(has, vmin, 0.0)[:, None], 0.0))
                if (~has).any():
                    gap.see(dn - dn[kmax])
                dneg = np.where(has, vmin, dn[kmax])
                sel = np.where(has, neg[kmin], neg[kmax])
            l = dap - dneg + margin
            gap.see(l)
            act = l > 0
            total += float(l[act].sum())
            n_active += int(act.sum())
            np.add.at(Wc[a], pos[act], 1.0)
            s = sel[act]
            np.add.at(Wc[a], s[s >= 0], -1.0)
        elif mode == "all":
            if pos.size == 0 or neg.size == 0:
                continue
            Lm = row[pos][:, None] - row[neg][None, :] + margin
            gap.see(Lm)
            gap.see(Lm - 1e-16)
            act = Lm > 0
            total += float(Lm[act].sum())
            n_active += int((Lm > 1e-16).sum())
            Wc[a, pos] += act.sum(1)
            Wc[a, neg] -= act.sum(0)
        else:
            kmax = int(row.argmax())
            mx = row[kmax]
            vp = np.where(pos_m, row, 0.0)
            jp = int(vp.argmax())
            vn = row + np.where(neg_m, 0.0, mx)
            jn = int(vn.argmin())
            gap.see(row - mx)
            gap.see(vp - vp[jp])
            gap.see(vn - vn[jn])
            x = vp[jp] - vn[jn]
            if mode == "hard":
                l = x + margin
                gap.see(l)
                w = 1.0 if l > 0 else 0.0
                if l > 0:
                    total += l
                    n_active += 1
            else:
                total += max(x, 0.0) + np.log1p(np.exp(-abs(x)))
                w = 1.0 / (1.0 + np.exp(-x)) if x >= 0 else np.exp(x) / (1.0 + np.exp(x))
                n_active += 1
            if w != 0.0:
                if pos_m[jp]:
                    Wc[a, jp] += w
                Wc[a, jn] -= w
                if not neg_m[jn]:
                    Wc[a, kmax] -= w
    if mode == "semihard":
        inv = 1.0 / n_pairs if n_pairs > 0 else 0.0          # the package's 0 / 0 is reported as 0
    elif mode == "all":
        inv = 1.0 / (n_active + 1e-16)
    else:
        inv = 1.0 / B
    W = Wc * inv
    S = W + W.T
    if distance == EUCLIDEAN:
        with np.errstate(divide="ignore", invalid="ignore"):
            Cm = np.where(D > 0, S / np.where(D > 0, D, 1.0), 0.0)
        grad = Cm.sum(1)[:, None] * e - Cm @ e
    elif distance == DOT:
        grad = -S @ e
    else:
        gn = -S @ n_rows
        grad = (gn - n_rows * (n_rows * gn).sum(1, keepdims=True)) / norm[:, None]
    return dict(loss=total * inv, grad=grad, counts=(n_pairs, n_valid, n_active), min_gap=gap.v, D=D, W=W)


# ------------------------------------------------------------------------------------------------ the GPU inputs
# kind "grid": coordinates drawn from {-3 .. 3}: every squared distance and every dot product is a small integer, exact in f32; run on
#   the entry point with distances EUCLIDEAN and DOT.  kind "float": N(0, 1) * scale; run through the Python classes with
#   EUCLIDEAN and COSINE.  classes == B: every label distinct.  margins[distance] = (one that cuts the hinge, one above every
#   distance difference so that no hinge cuts).  modes: which of the four run the case.  min_gap (tests/test_triplet_family_host.py):
#   >= 5e-5 on the grid cases, >= 1e-4 on the float cases, for every (mode, distance, margin) the GPU test runs.
GRID_MARGINS = {EUCLIDEAN: (0.7183, 30.0), DOT: (0.7183, 400.0)}
CASES = [
    dict(name="b1", kind="grid", seed=101, B=1, H=16, classes=1, margins=GRID_MARGINS, modes=MODES),
    dict(name="b2_same", kind="grid", seed=102, B=2, H=16, classes=1, margins=GRID_MARGINS, modes=MODES),
    dict(name="b2_diff", kind="grid", seed=103, B=2, H=16, classes=2, margins=GRID_MARGINS, modes=MODES),
    dict(name="b33", kind="grid", seed=104, B=33, H=5, classes=3, margins=GRID_MARGINS, modes=MODES),
    dict(name="b64", kind="grid", seed=105, B=64, H=16, classes=4, margins=GRID_MARGINS, modes=MODES),
    dict(name="b65", kind="grid", seed=106, B=65, H=16, classes=4, margins=GRID_MARGINS, modes=MODES),
    dict(name="b65_one_class", kind="grid", seed=107, B=65, H=16, classes=1, margins=GRID_MARGINS, modes=MODES),
    dict(name="b65_distinct", kind="grid", seed=108, B=65, H=16, classes=65, margins=GRID_MARGINS, modes=MODES),
    dict(name="b160", kind="grid", seed=109, B=160, H=16, classes=5, margins=GRID_MARGINS, modes=MODES),
    dict(name="b512", kind="grid", seed=110, B=512, H=16, classes=8, margins=GRID_MARGINS, modes=MODES),
    dict(name="f16", kind="float", seed=215, B=16, H=768, classes=4, scale=1.0, margins={EUCLIDEAN: (0.5, 80.0), COSINE: (0.02, 5.0)}, modes=MODES),
    # 96 random rows.  Semi-hard compares every (positive, negative) pair of a row: ~1e5 distance pairs drawn from a range of ~3 cannot all
    # be 1e-4 apart (measured min_gap 3e-7 Euclidean, 5e-8 cosine), so it is covered past B = 16 on the integer grid only.  Batch-all
    # compares no distance with another, and above every distance no hinge is near 0 either (a cutting margin would put ~1e5 hinge
    # arguments near 0).  The two hard modes compare each row's extremes with the runners-up only: a seed that keeps those 1e-4 apart.
    dict(name="f96", kind="float", seed=202, B=96, H=768, classes=6, scale=1.0, margins={EUCLIDEAN: (None, 80.0), COSINE: (None, 5.0)}, modes=("all",)),
    dict(name="f96_hard", kind="float", seed=305, B=96, H=768, classes=6, scale=1.0, margins={EUCLIDEAN: (0.5, 80.0), COSINE: (0.02, 5.0)},
         modes=("hard", "hard_soft")),
]


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def case_distances(case):
    return (EUCLIDEAN, DOT) if case["kind"] == "grid" else (EUCLIDEAN, COSINE)


def case_inputs(case):
    """-> (emb float32 [B, H], labels int64 [B]) as NumPy arrays."""
    rs = np.random.RandomState(case["seed"])
    B, H = case["B"], case["H"]
    if case["kind"] == "grid":
        emb = rs.randint(-3, 4, size=(B, H)).astype(np.float32)
    else:
        emb = (rs.randn(B, H) * case["scale"]).astype(np.float32)
    labels = rs.permutation(B) if case["classes"] == B else rs.randint(0, case["classes"], size=B)
    return emb, labels.astype(np.int64)


def case_runs(case):
    """every (mode, distance, margin) the GPU test runs for this case"""
    for dist in case_distances(case):
        for mode in case["modes"]:
            for margin in case["margins"][dist]:
                if margin is None:
                    continue
                if mode == "hard_soft" and margin != case["margins"][dist][-1]:
                    continue                                  # no margin in the soft-margin loss: one run
                yield mode, dist, margin
