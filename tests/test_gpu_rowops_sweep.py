"""The stand-alone row kernels (csrc/ln.hip, ln_device.h, reduce_device.h) through carel_layernorm_fwd, carel_layernorm_bwd,
carel_layernorm_bwd_packed, carel_colsum_bf16 and carel_partial_reduce_f32, against torch.nn.functional.layer_norm in float64 on the
kernels' own float32 inputs (and its autograd backward), dropout multipliers from oracle.carel_oracle.dropout_keep.  Outputs start as
NaN, every written buffer (the partials included, at exactly the size the header states) sits between guard regions, and a second
identical run must give the same bits.

Metrics are per row and per column, never per tensor:
  x_f32, dh      ||got - ref|| / ||ref|| of each row: 1e-6 forward, 1e-5 backward (tests/test_gpu_rowops.py)
  stats          mean: rtol 1e-5, atol 1e-6 (as there); rstd: relative 1e-5 against the float64 1 / sqrt(var + eps)
  x_bf16         == x_f32.to(bfloat16) bit for bit
  dy_bf16        exactly 0 where the oracle drops the element, elsewhere within one bf16 rounding (relative 2^-8) of the kernel's own
                 dh * keep / (1 - p), element by element; with p = 0 it is dh.to(bfloat16) bit for bit
  dgamma, dbeta, dbias, column sums, per column:  |got - ref| <= L * 2^-24 * sum over rows of |term|
                 L = the longest chain of sequential additions a term passes through, from the code (chain_ln / chain_colsum /
                 chain_reduce below): rows per wave, the 4-wave combine (two levels), the parts of one part-lane of
                 partial_colsum16 (four accumulators, then two levels), its 8-way combine
For dbeta, the bf16 column sums and the partial reduction a term is an input.  A term of dgamma (dy * xhat) or dbias (dh * keep) is
itself computed, as a difference: xhat = (h - mean) rstd, dh = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)), and the error it carries
does not shrink with its value.  The bound is taken with |term| the term's own value ("values") wherever stock torch float32 on the CPU
stays within half of it: every case from 2047 rows on and the 17-row cases of the normal and small inputs (literal_form).  It cannot be
met by any float32 code at fewer rows, where a column's xhat or dh lies near 0 in some column out of 768 (torch float32: 2.6 / 17 times
the bound on dgamma / dbias at one N(0.3, 2) row, 22 / 3.6 at three mixed rows, 1.26 on dbias at five, 1.5 on dgamma at 17 mixed rows),
nor with rows of mean 20 among 17 or fewer (10.6 / 5.3 at five, 1.8 / 0.63 at 17).  Only those cases take the "operands" form: |term|
the sum of the magnitudes the term is the difference of -- |dy| (|h| + |mean|) rstd for dgamma, keep * rstd (|dy g| + mean|dy g| +
|xhat| mean|dy g xhat|) for dbias -- and L plus the ROUND roundings of forming it (for dbias also the ROW_CHAIN additions of the row
sums inside dh).  No column bound carries the conditioning factor below.
Rows of mean 20 and standard deviation 1 get their per-ROW bounds multiplied by 1 + |mean| rstd, the conditioning of h - mean; no other
row gets any allowance.  test_torch_fp32_within_half_of_every_bound checks on the CPU that stock torch float32 LayerNorm stays within
half of every one of these bounds on every row and column; worst fractions, torch float32 on the CPU | the kernels on an MI355X:
    x, mean, rstd, dh                          0.159, 0.017, 0.012, 0.017 | 0.146, 0.014, 0.015, 0.015
    dbeta                                      0.139 | 0.116
    dgamma, dbias, "values" cases              0.186, 0.328 | 0.159, 0.295
    dgamma, dbias, "operands" cases            0.126, 0.103 | 0.140, 0.074
    dy_bf16 0.996 (a bf16 rounding is up to 2^-8), carel_colsum_bf16 0.048, carel_partial_reduce_f32 0.173
(run with -s: every case prints its own).  The sweep found one fault: the pair branch of dropout_mult_n (carel_common.h) added the pair
index without wrapping it at 2^31, so that an even offset which takes the element index past 2^32 inside a group of four gave the
second pair the hash of pair 0x80000000 instead of pair 0, unlike dropout_mult and the oracle; fixed there, and the last of OFFSETS
is its case.
"""
import math

import pytest
import torch

from carel_vae_amd import _lib as L
from oracle import carel_oracle as O
from tests.gpu_util import Arena, bits, keep_mask, one_thread

H = 768
U = 2.0 ** -24
ROUND = 8                      # roundings of forming one dgamma / dbias term, on top of the row sums it contains (ROW_CHAIN)
ROW_CHAIN = 12 + 6             # a 768-wide row sum: 12 sequential additions per lane, six butterfly levels
ROWS = (1, 2, 3, 4, 5, 17, 2047, 2048, 2049, 4095, 4096, 4097, 8193)
SEED, SITE = 99, O.site_attn_out(1)
WRAP = 2 ** 32


# ------------------------------------------------------------------------------------------------ what the host code picks, restated
def rpw(rows):
    return 1 if rows <= 2048 else (2 if rows <= 4096 else 4)


def blocks(rows):
    return -(-rows // (4 * rpw(rows)))


def chain_reduce(nparts):
    """partial_colsum16: part-lane rl takes parts rl, rl + 8, ...: four at a time into s0 .. s3 while p + 24 < nparts, the rest into s0;
    (s0 + s1) + (s2 + s3); then the 8 part-lanes one after the other."""
    worst = 0
    for rl in range(8):
        p, c = rl, [0, 0, 0, 0]
        while p + 24 < nparts:
            c = [v + 1 for v in c]
            p += 32
        while p < nparts:
            c[0] += 1
            p += 8
        worst = max(worst, max(c) + 2)
    return worst + 8


def chain_ln(rows):
    return rpw(rows) + 2 + chain_reduce(blocks(rows))


def chain_colsum(rows, accumulate):
    """colsum_bf16_kernel: one thread adds every 8th row of a 256-row chunk, 8 such sums are added in turn, then the chunks' partials."""
    return -(-min(rows, 256) // 8) + 8 + chain_reduce(-(-rows // 256)) + (1 if accumulate else 0)


def test_chains():
    assert [rpw(r) for r in (2048, 2049, 4096, 4097)] == [1, 2, 2, 4]
    assert [blocks(r) for r in (1, 5, 2048, 2049, 4096, 4097, 8193)] == [1, 2, 512, 257, 512, 257, 513]
    assert [chain_reduce(n) for n in (1, 8, 9, 32, 33, 57, 512, 513)] == [11, 11, 12, 11, 12, 14, 26, 27]


# ------------------------------------------------------------------------------------------------ inputs
def make_rows(rows, kind, seed):
    """-> (h [rows, 768] float32, cond [rows] float64 or None).  kind: "normal" N(0.3, 2); "small" standard deviation 3e-3 (eps 1e-5
    decides rstd); "offset" mean 20, standard deviation 1; "mixed": the three in turn, row rows // 2 all zero (from two rows on)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((rows, H), generator=g)
    which = {"normal": 0, "small": 1, "offset": 2}.get(kind)
    k = torch.arange(rows) % 3 if which is None else torch.full((rows,), which)
    h = torch.where((k == 0)[:, None], z * 2.0 + 0.3, torch.where((k == 1)[:, None], z * 3e-3, z + 20.0))
    if kind == "mixed" and rows >= 2:
        h[rows // 2] = 0.0
    return h.contiguous(), k == 2


def make_affine(seed):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    gamma[5], gamma[300], gamma[17] = 0.0, 0.0, -0.7                      # zeros and a negative entry
    return gamma, beta


def make_map(rows, seed):
    """A permutation with gaps: `rows` distinct original rows out of 3 * rows + 7, in random order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(3 * rows + 7, generator=g)[:rows].to(torch.int32)


def drop_mult(rows, drop, row_map, device):
    """[rows, 768] float64 multipliers (0 or 1 / (1 - p)) at element map[row] * 768 + col + offset (uint32, wrapping)."""
    seed, site, off, p = drop
    if row_map is None:
        return keep_mask(seed, site, rows * H, p, off, device).view(rows, H)
    import numpy as np
    idx = (row_map.cpu().numpy().astype(np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :] + np.uint64(off)).astype(np.uint32)
    return torch.from_numpy(O.dropout_keep(seed, site, idx.reshape(-1), p).astype(np.float64) / (1 - p)).view(rows, H).to(device)


# ------------------------------------------------------------------------------------------------ reference and bounds
def literal_form(rows, kind):
    """Which cases take the column bound with |term| the term's own value: those where stock torch float32 stays within half of it
    (test_torch_fp32_within_half_of_every_bound) -- every case from 2047 rows on, and 17 rows of the normal and small inputs."""
    return rows >= 2047 or (rows >= 17 and kind in ("normal", "small"))


def reference(h, gamma, beta, eps, dy, mult, offset_rows, literal):
    """Everything in float64 on h's device.  -> dict of references and of the per-row / per-column scales of the bounds."""
    hd = h.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    x = torch.nn.functional.layer_norm(hd, (H,), gd, bd, eps)
    x.backward(dy.double())
    mean, var = h.double().mean(1), h.double().var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    cond = torch.where(offset_rows.to(h.device), 1.0 + mean.abs() * rstd, torch.ones_like(mean))
    xhat = (h.double() - mean[:, None]) * rstd[:, None]
    dxh = dy.double() * gamma.double()
    dh = hd.grad
    r = dict(x=x.detach(), mean=mean, rstd=rstd, cond=cond, dh=dh, dgamma=gd.grad, dbeta=bd.grad, dbias=(dh * mult).sum(0), mult=mult)
    rows = h.shape[0]
    Lc = chain_ln(rows)
    r["lim_dbeta"] = Lc * U * dy.double().abs().sum(0)
    r["form"] = "values" if literal else "operands"
    if literal:
        r["lim_dgamma"] = Lc * U * (dy.double() * xhat).abs().sum(0)
        r["lim_dbias"] = Lc * U * (dh * mult).abs().sum(0)
        return r
    mag_g = dy.double().abs() * (h.double().abs() + mean.abs()[:, None]) * rstd[:, None]
    r["lim_dgamma"] = (Lc + ROUND) * U * mag_g.sum(0)
    mag_h = rstd[:, None] * (dxh.abs() + dxh.abs().mean(1, keepdim=True) + xhat.abs() * (dxh * xhat).abs().mean(1, keepdim=True))
    r["lim_dbias"] = (Lc + ROUND + ROW_CHAIN) * U * (mag_h * mult).sum(0)
    return r


def row_err(got, ref, cond=None):
    e = (got.double() - ref).norm(dim=1) / ref.norm(dim=1)
    return e if cond is None else e / cond


def col_frac(got, ref, lim):
    d = (got.double() - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / lim)                  # (a column nothing is added to has lim 0 and must be exact)


class Worst:
    """The worst fraction of its bound per quantity; done() fails on those above `limit`."""

    def __init__(self, tag, limit=1.0):
        self.tag, self.limit, self.rows = tag, limit, {}

    def add(self, name, frac):
        f = float(torch.as_tensor(frac).double().max())
        assert not math.isnan(f), (self.tag, name)
        self.rows[name] = max(self.rows.get(name, 0.0), f)

    def done(self):
        print("%-44s " % self.tag + "  ".join("%s %.3f" % kv for kv in self.rows.items()))
        bad = {k: v for k, v in self.rows.items() if not v <= self.limit}
        assert not bad, (self.tag, bad)


def judge_fwd(w, got, r):
    if got.get("xf") is not None:
        w.add("x", row_err(got["xf"], r["x"], r["cond"]) / 1e-6)
    if got.get("st") is not None:
        st = got["st"].double()
        w.add("mean", (st[:, 0] - r["mean"]).abs() / (1e-6 + 1e-5 * r["mean"].abs()))
        w.add("rstd", (st[:, 1] - r["rstd"]).abs() / (1e-5 * r["rstd"]))
    if got.get("xf") is not None and got.get("xb") is not None:
        assert torch.equal(bits(got["xb"]), bits(got["xf"].to(torch.bfloat16))), w.tag


def judge_bwd(w, got, r, p):
    mult = r["mult"]
    if got.get("dh") is not None:
        w.add("dh", row_err(got["dh"], r["dh"], r["cond"]) / 1e-5)
    if got.get("dyb") is not None and got.get("dh") is not None:
        dyb, own = got["dyb"].double(), got["dh"].double() * mult
        assert bool((dyb[mult == 0] == 0).all()), w.tag
        if p == 0:
            assert torch.equal(bits(got["dyb"]), bits(got["dh"].to(torch.bfloat16))), w.tag
        w.add("dy_bf16", torch.where(mult == 0, torch.zeros_like(own), (dyb - own).abs() / (2.0 ** -8 * own.abs()).clamp(min=1e-300)))
    for k in ("dgamma", "dbeta", "dbias"):
        if got.get(k) is not None:
            w.add(k if k == "dbeta" else "%s(%s)" % (k, r["form"]), col_frac(got[k], r[k], r["lim_" + k]))


# ------------------------------------------------------------------------------------------------ stock torch float32 on the CPU
def torch_fp32(h, gamma, beta, eps, dy, mult):
    h32 = h.clone().requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    x = torch.nn.functional.layer_norm(h32, (H,), g32, b32, eps)
    x.backward(dy)
    mean = h.mean(1)
    rstd = torch.rsqrt(h.var(1, unbiased=False) + eps)
    m32 = mult.float()
    return dict(xf=x.detach(), st=torch.stack((mean, rstd), 1), dh=h32.grad, dgamma=g32.grad, dbeta=b32.grad, dbias=(h32.grad * m32).sum(0))


LN_CASES = ([(rows, "mixed", 1e-5, 0.1, 7 * H) for rows in ROWS] +
            [(rows, kind, eps, 0.1, 7 * H) for rows in (5, 17) for kind, eps in
             (("normal", 1e-12), ("small", 1e-5), ("small", 1e-12), ("offset", 1e-12), ("mixed", 1e-12))] +
            [(2049, "mixed", 1e-12, 0.1, 7 * H)])
# dropout: rate x offset -- none, even, odd (dropout_mult_n's element-by-element branch), and three that wrap the uint32 index inside
# the second row: at a float4 boundary, odd, and even INSIDE a float4 (element 0xFFFFFFFE first: the pair branch's second pair is
# pair 0 again -- it used to hash pair 0x80000000 there, unlike dropout_mult and the oracle)
OFFSETS = (0, 7 * H, 4097, WRAP - H - 256, WRAP - H - 255, WRAP - H - 254)
DROP_CASES = [(rows, "normal", 1e-12, p, off) for rows in (5, 2049) for p in (0.1, 0.5) for off in OFFSETS] + \
             [(rows, "normal", 1e-12, 0.0, 7 * H) for rows in (5, 2049)]


def case_id(c):
    return "r%d-%s-eps%g-p%g-off%d" % c


def case_inputs(c, device="cpu"):
    rows, kind, eps, p, off = c
    h, offset_rows = make_rows(rows, kind, 11)
    gamma, beta = make_affine(12)
    dy = torch.randn((rows, H), generator=torch.Generator().manual_seed(13))
    return tuple(t.to(device) for t in (h, gamma, beta, dy)) + (offset_rows,)


def test_torch_fp32_within_half_of_every_bound():
    """The inputs are fit to be judged by these bounds: stock torch float32 stays within half of each, every row and column.  Of the
    row counts from 2047 on, 2048 (one row per wave), 2049 (two), 4097 and 8193 (four) are run here: make_rows draws the same rows for
    every count (the first k rows of a larger case are the rows of the k-row case), so the 8193-row case judges every row any case
    uses; the column bounds of the counts left out lie between those of their neighbours."""
    worst = {}
    with one_thread():
        _torch_fp32_cases(worst)
    print("torch float32, worst fraction of each bound: " + "  ".join("%s %.3f" % kv for kv in worst.items()))


def _torch_fp32_cases(worst):
    for c in [c for c in LN_CASES if c[0] <= 17 or c[0] in (2048, 2049, 4097, 8193)] + [c for c in DROP_CASES if c[0] == 5] + \
            [(17, "normal", 1e-12, 0.1, 4097), (2049, "normal", 1e-12, 0.5, 0), (2049, "normal", 1e-12, 0.0, 7 * H)]:
        rows, kind, eps, p, off = c
        h, gamma, beta, dy, offset_rows = case_inputs(c)
        mult = drop_mult(rows, (SEED, SITE, off, p), None, "cpu")
        r = reference(h, gamma, beta, eps, dy, mult, offset_rows, literal_form(rows, kind))
        got = torch_fp32(h, gamma, beta, eps, dy, mult)
        w = Worst("torch float32 " + case_id(c), 0.5)
        judge_fwd(w, got, r)
        judge_bwd(w, got, r, p)
        w.done()
        for k, v in w.rows.items():
            worst[k] = max(worst.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------ the kernels
def hip_fwd(h, gamma, beta, eps, omit=(), seed=1):
    lib, rows = L.load(), h.shape[0]
    A = Arena(seed)
    out = dict(xf=A.nan((rows, H)), xb=A.nan((rows, H), torch.bfloat16), st=A.nan((rows, 2)))
    ptr = {k: (None if k in omit else v.ptr) for k, v in out.items()}
    L.check(lib.carel_layernorm_fwd(h.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, rows, H, ptr["xf"], ptr["xb"], ptr["st"],
                                    L.current_stream()), "carel_layernorm_fwd")
    torch.cuda.synchronize()
    assert A.intact()
    for k in omit:
        assert bool(torch.isnan(out[k].t.float()).all()), k                      # not requested, not written
    return {k: (None if k in omit else v.t.clone()) for k, v in out.items()}


def hip_bwd(dy, h, st, gamma, drop, row_map=None, packed=False, omit=(), seed=1):
    lib, rows = L.load(), h.shape[0]
    nblk = lib.carel_layernorm_bwd_blocks(rows)
    assert nblk == blocks(rows) == -(-rows // (4 * rpw(rows)))
    A = Arena(seed)
    out = dict(dh=A.nan((rows, H)), dyb=A.nan((rows, H), torch.bfloat16), dgamma=A.nan((H,)), dbeta=A.nan((H,)), dbias=A.nan((H,)),
               part=A.nan((nblk * 3 * H,)))
    ptr = {k: (None if k in omit else v.ptr) for k, v in out.items()}
    seed_, site, off, p = drop
    if packed or row_map is not None:
        L.check(lib.carel_layernorm_bwd_packed(dy.data_ptr(), h.data_ptr(), st.data_ptr(), gamma.data_ptr(), rows, H, seed_, site, off, p,
                                               None if row_map is None else row_map.data_ptr(), ptr["dh"], ptr["dyb"], ptr["dgamma"],
                                               ptr["dbeta"], ptr["dbias"], ptr["part"], L.current_stream()), "carel_layernorm_bwd_packed")
    else:
        L.check(lib.carel_layernorm_bwd(dy.data_ptr(), h.data_ptr(), st.data_ptr(), gamma.data_ptr(), rows, H, seed_, site, off, p,
                                        ptr["dh"], ptr["dyb"], ptr["dgamma"], ptr["dbeta"], ptr["dbias"], ptr["part"], L.current_stream()),
                "carel_layernorm_bwd")
    torch.cuda.synchronize()
    assert A.intact()
    for k in omit:
        assert bool(torch.isnan(out[k].t.float()).all()), k
    assert not bool(torch.isnan(out["part"].t).any())                             # every partial block written: none left for the reduction to read unset
    return {k: (None if k in omit else v.t.clone()) for k, v in out.items() if k != "part"}


def same(a, b, keys=None):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in (keys or a) if a[k] is not None and b[k] is not None)


def run_case(c, row_map=None):
    rows, kind, eps, p, off = c
    h, gamma, beta, dy, offset_rows = case_inputs(c, "cuda")
    drop = (SEED, SITE, off % WRAP, p)
    mult = drop_mult(rows, drop, row_map, "cuda")
    r = reference(h, gamma, beta, eps, dy, mult, offset_rows, literal_form(rows, kind))
    fwd = hip_fwd(h, gamma, beta, eps)
    assert same(fwd, hip_fwd(h, gamma, beta, eps, seed=2)), "forward not reproducible"
    bwd = hip_bwd(dy, h, fwd["st"], gamma, drop, row_map)
    assert same(bwd, hip_bwd(dy, h, fwd["st"], gamma, drop, row_map, seed=2)), "backward not reproducible"
    w = Worst(case_id(c) + ("-packed" if row_map is not None else ""))
    judge_fwd(w, fwd, r)
    judge_bwd(w, bwd, r, p)
    if kind == "mixed" and rows >= 2:                                             # the all-zero row: x == beta exactly, stats == (0, rsqrt(eps))
        z = rows // 2
        assert torch.equal(fwd["xf"][z], beta) and float(fwd["st"][z, 0]) == 0.0
        assert abs(float(fwd["st"][z, 1]) - eps ** -0.5) <= 1e-5 * eps ** -0.5
    w.done()
    return fwd, bwd, (h, gamma, beta, dy, drop)


@pytest.mark.gpu
@pytest.mark.parametrize("c", LN_CASES, ids=case_id)
def test_layernorm_rows_and_inputs(c):
    run_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", DROP_CASES, ids=case_id)
def test_layernorm_bwd_dropout(c):
    run_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [5, 17, 2049, 4097])
def test_layernorm_bwd_packed(rows):
    """drop_row_map: the mask is the oracle's at map[row] * 768 + col + offset; with the identity map, carel_layernorm_bwd's bits."""
    for off in (7 * H, 4097):
        c = (rows, "normal", 1e-12, 0.1, off)
        fwd, bwd, (h, gamma, beta, dy, drop) = run_case(c, make_map(rows, rows).cuda())
        plain = hip_bwd(dy, h, fwd["st"], gamma, drop)
        assert not same(plain, bwd, ("dyb",))                                     # (the map matters)
        ident = hip_bwd(dy, h, fwd["st"], gamma, drop, torch.arange(rows, dtype=torch.int32).cuda())
        assert same(plain, ident) and same(plain, hip_bwd(dy, h, fwd["st"], gamma, drop, None, packed=True))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [3, 17])
def test_layernorm_optional_outputs(rows):
    """Each optional output left out in turn: it is not written and the others keep their bits."""
    c = (rows, "normal", 1e-12, 0.1, 7 * H)
    fwd, bwd, (h, gamma, beta, dy, drop) = run_case(c)
    for k in ("xf", "xb", "st"):
        assert same(fwd, hip_fwd(h, gamma, beta, 1e-12, omit=(k,))), k
    for k in ("dh", "dyb", "dbias"):
        assert same(bwd, hip_bwd(dy, h, fwd["st"], gamma, drop, omit=(k,))), k


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("n", [8, 264, 768, 2304])
def test_colsum_bf16(rows, n):
    """ld = n and ld = n + 24 (a column slice of a wider matrix whose other columns hold NaN: reading one poisons the sum)."""
    lib = L.load()
    g = torch.Generator().manual_seed(rows * 10000 + n)
    w = Worst("colsum r%d n%d" % (rows, n))
    for ld in (n, n + 24):
        wide = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16)
        c0 = 0 if ld == n else 16
        wide[:, c0:c0 + n] = torch.randn((rows, n), generator=g).bfloat16()
        x = wide.cuda()
        xs = x[:, c0:c0 + n]
        chunks = -(-rows // 256)
        prior = torch.randn(n, generator=g)
        for acc in (0, 1):
            outs = []
            for run in range(2):
                A = Arena(run)
                out, part = A.put(prior.cuda()) if acc else A.nan((n,)), A.nan((chunks * n,))
                L.check(lib.carel_colsum_bf16(xs.data_ptr(), ld, rows, n, out.ptr, acc, part.ptr, L.current_stream()), "carel_colsum_bf16")
                torch.cuda.synchronize()
                assert A.intact()
                outs.append(out.t.clone())
            assert torch.equal(bits(outs[0]), bits(outs[1]))
            ref = xs.double().sum(0) + (prior.double().cuda() if acc else 0.0)
            lim = chain_colsum(rows, acc) * U * (xs.double().abs().sum(0) + (prior.double().abs().cuda() if acc else 0.0))
            w.add("ld%d-acc%d" % (ld - n, acc), col_frac(outs[0], ref, lim))
    w.done()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 768])
def test_partial_reduce_f32(n):
    """nparts over the loop's 32-stride body and its 8-stride remainder."""
    lib = L.load()
    w = Worst("partial_reduce n%d" % n)
    for nparts in (1, 7, 8, 9, 31, 32, 33, 57, 512):
        g = torch.Generator().manual_seed(n * 1000 + nparts)
        part, prior = torch.randn((nparts, n), generator=g).cuda(), torch.randn(n, generator=g)
        for acc in (0, 1):
            outs = []
            for run in range(2):
                A = Arena(run)
                out = A.put(prior.cuda()) if acc else A.nan((n,))
                L.check(lib.carel_partial_reduce_f32(part.data_ptr(), out.ptr, n, nparts, acc, L.current_stream()), "carel_partial_reduce_f32")
                torch.cuda.synchronize()
                assert A.intact()
                outs.append(out.t.clone())
            assert torch.equal(bits(outs[0]), bits(outs[1]))
            ref = part.double().sum(0) + (prior.double().cuda() if acc else 0.0)
            lim = (chain_reduce(nparts) + acc) * U * (part.double().abs().sum(0) + (prior.double().abs().cuda() if acc else 0.0))
            w.add("parts%d-acc%d" % (nparts, acc), col_frac(outs[0], ref, lim))
    w.done()
