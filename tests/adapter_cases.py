"""Case table of the sentence-adapter sweep (tests/test_gpu_adapter_sweep.py; judged without a device by
tests/test_adapter_cases_host.py): designed score rows with a known support, the layout of x that makes csrc/adapter.hip's kernels
observable one by one, the float64 references (tests/adapter_restate.py) and the error bounds.

OBSERVABLE KERNELS.  carel_adapter_forward / _backward take u as an input, so a sparse-mode case sets u[a] = e_a (the unit vector of
column a) and lays x [B, S, 768] out as
    column 0            the designed scores of the emotion adapter
    column 1            the designed scores of the cause adapter (another support size, another permutation)
    columns 2 .. 2+S-1  one-hot(s)
    columns 2+S .. 767  random f32 values
The scores the normaliser sees are then x[:, a] exactly (one non-zero product, every other term an exact zero), out[a, b, 2 + s] is
p[a, b, s] bit for bit, and with d_out[:, :, 0:2] = 0, dx[b*S + s, a] is dz[a, b, s] bit for bit.  Because p is observed exactly, the
weighted sum, the p * d_out term and the normaliser backward are each judged against float64 ON THE KERNEL'S OWN p: every bound below is
the bound of one kernel's chain, never a sum over the kernels before it.

DESIGNED ROWS (designed_row).  The top k values are 3.25 - j g, j = 0..k-1, the other S - k values 20 below the maximum, shuffled by a
seeded permutation.  sparsemax: g = 1 / (k (k - 1)), so sum_j (z_0 - z_j) = 1/2 < 1 over the top k, the support is k and the smallest
p is 1 / (2 k) >= 1/256.  entmax-1.5: the support is k as long as the gap h of x = z / 2 has h^2 k (k - 1) (2 k - 1) / 6 <= 1; g is
that limit in score units, so h is half of it.  "tied": g = 0 (a tie block of k).  "dyadic" (sparsemax, k a power of two):
g = 2^-ceil(log2(k (k - 1))), every partial sum and the division by k exact in float32, so float32 equals float64 bit for bit.

BOUNDS, with u = 2^-24, first order, per element; k is the support, xs the sorted shifted scores, A = sum_{j<=k} |xs_j|.
  p, sparsemax   tau = (sum_{j<=k} xs_j - 1) / k: a sum of k non-zero terms (at most k - 1 inexact adds in any order: the sequential
                 prefix loop, or the wave sum whose other lanes add exact zeros), one subtraction, one division; p = x - tau.
                   E_p = ((k - 1) u A + u |sum - 1|) / k + u |tau| + u p            (x = z - max z is exact: Sterbenz, and -20)
  p, entmax      mean = c_k / k          E_m  = ((k - 1) u A + u |c_k|) / k
                 ss = sum fmaf(d, d, .)  E_ss = k u ss + sum_j 2 |d_j| (E_m + u |d_j|),  d_j = xs_j - mean
                 v = (1 - ss) / k        E_v  = (E_ss + u |1 - ss|) / k + u v
                 sq = sqrt(v)            E_sq = E_v / (2 sq) + u sq
                 tau = mean - sq         E_t  = E_m + E_sq + u |tau|
                 p = (x - tau)^2         E_p  = 2 (x - tau) (E_t + u (x - tau)) + u p
  out (combine)  S/16 sequential fmaf, two shuffle levels, three adds across the waves: (S/16 + 5) u sum_s p |H|
  dp (rowdot)    12 products per lane and six butterfly levels: E_dp = 18 u sum_c |x_c d_c|   (no term passes more than 12 roundings)
  dz, sparsemax  mean over the support by a wave sum (7 roundings) and a division, one subtraction:
                   E = E_dp + mean_supp(E_dp) + 9 u mean_supp|dp| + u |dz|
  dz, entmax     q = sqrt(p) (u), d = dp q (2 u |d| + q E_dp), N = sum d and D = sum q by wave sums (7 u each), qq = N / D,
                 r = d - qq q:   E_N = sum E_d + 7 u sum |d|,  E_D = 8 u D,  E_qq = E_N / D + |N| E_D / D^2 + u |qq|,
                   E = E_d + E_qq q + 2 u |qq| q + u |r|
  dx, columns >= 2   fmaf(p_0, d_0, 0) then fmaf(p_1, d_1, .) (the dz u terms are exact zeros): the chain reaches
                 u (2 |p_0 d_0| + |p_1 d_1|) at worst, i.e. all of 2 u (|p_0 d_0| + |p_1 d_1|) when the second product is small, so no
                 float32 evaluation can be promised half of that: the bound is twice it, 4 u (|p_0 d_0| + |p_1 d_1|)   (DX_C = 2)
tests/test_adapter_cases_host.py holds the float32 restatement (torch on the CPU, the reference alone) to half of each: stock float32
torch for p, dp and dz, and for the two fmaf chains the kernels' own order of operations written out in torch (combine_chain32,
dx_chain32; an fmaf is the float64 product and sum rounded once to float32), since stock einsum sums S terms in one chain where the
kernel sums S/16.

RAW CASES are random (tests/test_gpu_adapter.py's _weights / _inputs, with its tied, constant and dominant samples where B allows)
and judged per sample: the larger of that module's bound (1e-5 out, 1e-4 dx) and four times the float32 restatement's own error on
that sample.  Weight gradients: 1e-4 per destination or four times the float32 restatement's error (the rule of F32_LIMITED in
tests/test_gpu_adapter_train.py), every sample kept, on inputs that meet that module's conditioned()."""
import math

import numpy as np
import torch

from tests import adapter_restate as R
from tests import test_gpu_adapter as A
from tests import test_gpu_adapter_train as TR

H = 768
U = 2.0 ** -24
S_ALL = (32, 64, 96, 128)
K_LIST = (1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)
HEADS = (1, 2, 3, 4, 6, 8, 12)
NV_ALL = (2, 4, 6, 8, 12, 16, 24)            # AD_NV_SWITCH
OFFSET, DROP = 3.25, 20.0
P_MARGIN, X_MARGIN = 1.0 / 256, 0.04         # the smallest sparsemax p / entmax x - tau a designed row may have
OUT_BOUND, DX_BOUND, WGRAD_BOUND = 1e-5, 1e-4, 1e-4
F64, F32 = torch.float64, torch.float32


def supports(S):
    """The support sizes of one designed batch of length S: K_LIST up to S, S - 1 and S."""
    return sorted(set(k for k in K_LIST if k <= S) | {S - 1, S})


def gap(k, mode, kind):
    if kind == "tied" or k == 1:
        return 0.0
    if mode == "entmax":
        return math.sqrt(6.0 / ((k - 1) * k * (2 * k - 1)))
    if kind == "dyadic":
        return 2.0 ** -math.ceil(math.log2(k * (k - 1)))
    return 1.0 / (k * (k - 1))


def designed_row(S, k, mode, kind, seed):
    """[S] float64 holding float32 values: a score row whose support under `mode` is exactly k."""
    z = torch.full((S,), OFFSET - DROP, dtype=F64)
    z[:k] = OFFSET - gap(k, mode, kind) * torch.arange(k, dtype=F64)
    perm = torch.from_numpy(np.random.RandomState(seed).permutation(S))
    return z.float().double()[perm]


# ------------------------------------------------------------------------------------------------ the table
def _designed(name, mode, S, kind, ks, Bp_extra=3, wgrad=False, seed=0):
    ks = list(ks)
    B = len(ks)
    pairs = [(ks[b], ks[(b + 1) % B]) for b in range(B)] if B > 1 else [(ks[0], ks[0] - 1)]
    return dict(name=name, kind="designed", mode=mode, S=S, G=1, B=B, Bp=B + Bp_extra, rows=kind, ks=pairs, wgrad=wgrad, seed=seed)


def _raw(name, G, S, B, kscale, Bp_extra, wgrad=False, seed=0):
    return dict(name=name, kind="raw", mode="raw", S=S, G=G, B=B, Bp=B + Bp_extra, kscale=float(kscale), wgrad=wgrad, seed=seed)


def designed_cases():
    out = []
    for mode in ("sparsemax", "entmax"):
        for S in S_ALL:
            for kind in ("spaced", "tied"):
                out.append(_designed("%s_S%d_%s" % (mode, S, kind), mode, S, kind, supports(S), seed=len(out)))
    for S in S_ALL:
        ks = [k for k in (1, 2, 4, 8, 16, 32, 64, 128) if k <= S]
        out.append(_designed("sparsemax_S%d_dyadic" % S, "sparsemax", S, "dyadic", ks, seed=len(out)))
    # a single sample: supports 65 (emotion) and 64 (cause), on the two sides of the lane / +64 boundary
    out.append(_designed("sparsemax_S128_B1", "sparsemax", 128, "spaced", [65], seed=len(out)))
    out.append(_designed("entmax_S96_B1", "entmax", 96, "spaced", [65], seed=len(out)))
    return out


def designed_wgrad_cases():
    """The designed cases whose weight gradients are run: u is built by carel_adapter_build_u from k_proj.weight = I, q_proj.weight = 0,
    q_proj.bias = float32(sqrt(768)) e_side, i.e. e_side up to one rounding."""
    out = []
    for mode in ("sparsemax", "entmax"):
        for S, kind in ((64, "spaced"), (128, "spaced"), (96, "tied")):
            out.append(_designed("wgrad_%s_S%d_%s" % (mode, S, kind), mode, S, kind, supports(S), wgrad=True, seed=100 + len(out)))
    out.append(_designed("wgrad_entmax_S128_B1", "entmax", 128, "spaced", [65], wgrad=True, seed=100 + len(out)))
    return out


# seeds of the raw weight-gradient cases that the default stream leaves without signal in a q / k gradient (conditioned(), on the
# float64 reference alone; see SALT in tests/test_gpu_adapter_train.py) -- asserted by tests/test_adapter_cases_host.py
RAW_SALT = {}


def raw_cases():
    out = []
    for S in (64, 128):
        for G in HEADS:
            for kscale in (1, 40):
                name = "raw_G%d_S%d_k%d" % (G, S, kscale)
                out.append(_raw(name, G, S, 5, kscale, 3 if kscale == 40 else 0, wgrad=(S == 64 or kscale == 1), seed=RAW_SALT.get(name, 0)))
    for S in (32, 96):                                       # every S at a head count that no other test runs
        for kscale in (1, 40):
            out.append(_raw("raw_G3_S%d_k%d" % (S, kscale), 3, S, 5, kscale, 0 if kscale == 40 else 3))
    for B in (1, 3, 4, 5, 8, 9):                             # the remainders of gemv's 4-sample and gemvT_part's 8-sample trips
        for extra in (0, 3):
            out.append(_raw("raw_G6_S32_B%d_pad%d" % (B, extra), 6, 32, B, 40 if extra else 1, extra))
    return out


def all_cases():
    return designed_cases() + designed_wgrad_cases() + raw_cases()


# ------------------------------------------------------------------------------------------------ inputs
def unit_u():
    u = torch.zeros(2, 1, H, dtype=F64)
    u[0, 0, 0] = u[1, 0, 1] = 1.0
    return u


def designed_inputs(c):
    """-> dict: Hs [B, S, 768], z [2, B, S] (the designed scores, = Hs[:, :, a]), u [2, 1, 768], d_out [2, B, 768] with columns 0:2
    zero; float64 tensors of float32 values."""
    B, S = c["B"], c["S"]
    g = torch.Generator().manual_seed(5000 + c["seed"])
    Hs = torch.zeros(B, S, H, dtype=F64)
    Hs[:, :, 2 + S:] = torch.randn(B, S, H - 2 - S, generator=g).double()
    Hs[:, :, 2:2 + S] = torch.eye(S, dtype=F64)
    for b, pair in enumerate(c["ks"]):
        for a, k in enumerate(pair):
            Hs[b, :, a] = designed_row(S, k, c["mode"], c["rows"], seed=1000 * c["seed"] + 2 * b + a)
    d_out = torch.randn(2, B, H, generator=g).double()
    d_out[:, :, 0:2] = 0.0
    return dict(Hs=Hs, z=Hs[:, :, 0:2].permute(2, 0, 1).contiguous(), u=unit_u(), d_out=d_out)


def designed_weights(side):
    """Weights under which carel_adapter_build_u gives u[side] = e_side up to one rounding (and the float64 reference the same scores up
    to float32(sqrt(768)) / sqrt(768))."""
    b = torch.zeros(H, dtype=F64)
    b[side] = float(torch.tensor(math.sqrt(H), dtype=F32))
    return {"q_proj.weight": torch.zeros(H, H, dtype=F64), "q_proj.bias": b, "k_proj.weight": torch.eye(H, dtype=F64),
            "k_proj.bias": torch.zeros(H, dtype=F64)}


def designed_wgrad_inputs(c):
    d = designed_inputs(c)
    g = torch.Generator().manual_seed(6000 + c["seed"])
    d["ws"] = [designed_weights(side) for side in range(2)]
    d["qs"] = [torch.randn(H, generator=g).double() for _ in range(2)]
    d["d_out"] = torch.randn(2, c["B"], H, generator=g).double()
    return d


def built_u32(side):
    """What carel_adapter_build_u computes from designed_weights(side), restated in float32: qv = 0 + b_q exactly, then
    u = (W_k^T qv) * (1 / sqrt(768))."""
    qv = designed_weights(side)["q_proj.bias"].float()
    return qv * (torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(float(H), dtype=F32)))


def raw_inputs(c):
    B, S, G = c["B"], c["S"], c["G"]
    g = torch.Generator().manual_seed(100000 * c["seed"] + 1000 * S + 10 * B + G + int(c["kscale"]))
    ws = [A._weights("raw", g, c["kscale"]) for _ in range(2)]
    qs = [torch.randn(H, generator=g).double() for _ in range(2)]
    Hs = A._inputs(B, S, seed=7 * S + B + G)
    d_out = torch.randn(2, B, H, generator=g).double()
    return dict(Hs=Hs, ws=ws, qs=qs, d_out=d_out)


# ------------------------------------------------------------------------------------------------ references
def normalise(z, mode, dtype=F64):
    z = z.to(dtype)
    return R.sparsemax(z) if mode == "sparsemax" else R.entmax15(z)


def normalise_backward(p, dp, mode):
    return R.sparsemax_backward(p, dp) if mode == "sparsemax" else R.entmax15_backward(p, dp)


def decisions(z, mode, dtype=F64):
    """The comparisons that fix the support of z [..., S], evaluated in `dtype` -> (support [...], margin [...]): margin is the smallest
    distance of any of them from its threshold (sparsemax: |1 + j zs_j - c_j| and the smallest p on the support; entmax:
    |xs_j - tau_j| and the smallest x - tau on the support)."""
    z = z.to(dtype)
    S = z.shape[-1]
    j = torch.arange(1, S + 1, dtype=dtype)
    x = z - z.max(-1, keepdim=True).values
    if mode == "entmax":
        x = x / 2
    xs = torch.sort(x, dim=-1, descending=True).values
    c = xs.cumsum(-1)
    if mode == "sparsemax":
        lhs = 1 + j * xs - c
        k = ((lhs > 0).to(dtype) * j).max(-1).values.long()
        p = R.sparsemax(z)
        on = torch.where(p > 0, p, torch.full_like(p, float("inf"))).min(-1).values
        return k, torch.minimum(lhs.abs().min(-1).values, on)
    mean = c / j
    tri = torch.tril(torch.ones(S, S, dtype=dtype))
    ss = (((xs.unsqueeze(-2) - mean.unsqueeze(-1)) ** 2) * tri).sum(-1)
    tau = mean - torch.sqrt(torch.clamp((1 - ss) / j, min=0))
    k = (tau <= xs).sum(-1)
    q = R.entmax15(z).sqrt()
    on = torch.where(q > 0, q, torch.full_like(q, float("inf"))).min(-1).values
    return k, torch.minimum((xs - tau).abs().min(-1).values, on)


def combine_ref(p, Hs):
    """out[a, b, :] = sum_s p[a, b, s] Hs[b, s, :] and its scale sum_s p |Hs|, in the dtype of the arguments."""
    return torch.einsum("abs,bsd->abd", p, Hs), torch.einsum("abs,bsd->abd", p.abs(), Hs.abs())


def dp_ref(Hs, d_out):
    """dp[a, b, s] = Hs[b, s, :] . d_out[a, b, :] and its scale sum_c |Hs d_out|."""
    return torch.einsum("bsd,abd->abs", Hs, d_out), torch.einsum("bsd,abd->abs", Hs.abs(), d_out.abs())


def raw_reference(c, d, dtype=F64):
    """Raw mode, in `dtype`: out [2, B, 768] and dx [B, S, 768] (autograd of sum(out * d_out)) of the reference's own computation."""
    Hr = d["Hs"].to(dtype).clone().requires_grad_()
    outs, total = [], 0.0
    for side in range(2):
        w = {k: v.to(dtype) for k, v in d["ws"][side].items()}
        o, _ = R.adapter_out(Hr, d["qs"][side].to(dtype), w, "raw", c["G"])
        outs.append(o.detach())
        total = total + (o * d["d_out"][side].to(dtype)).sum()
    total.backward()
    return torch.stack(outs).double(), Hr.grad.double()


def sample_err(got, ref, dims):
    """Relative norm per sample over `dims`; a sample whose reference is exactly zero must be matched exactly (-> 0 or inf)."""
    num, den = (got.double() - ref).pow(2).sum(dims).sqrt(), ref.pow(2).sum(dims).sqrt()
    return torch.where(den > 0, num / den.clamp(min=1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))


def raw_bounds(c, d, ref=None):
    """Per-sample bounds of a raw case: (out [2, B], dx [B]) = max(fixed, 4 x the float32 restatement's error), and that error."""
    ref = ref or raw_reference(c, d)
    o32, g32 = raw_reference(c, d, F32)
    e_out, e_dx = sample_err(o32, ref[0], (-1,)), sample_err(g32, ref[1], (-2, -1))
    return (torch.clamp(4 * e_out, min=OUT_BOUND), torch.clamp(4 * e_dx, min=DX_BOUND)), (e_out, e_dx)


# ------------------------------------------------------------------------------------------------ bounds
def p_bound(z, mode):
    """Elementwise bound on the kernel's p for score rows z [..., S] (float64 tensors of float32 values); see the module docstring."""
    x = z - z.max(-1, keepdim=True).values
    if mode == "entmax":
        x = x / 2
    p = normalise(z, mode)
    k = (p > 0).sum(-1, keepdim=True).double()
    xs = torch.sort(x, dim=-1, descending=True).values
    on = (torch.arange(z.shape[-1]) < k).double()                      # the support, in sorted order
    Aabs, c = (xs.abs() * on).sum(-1, keepdim=True), (xs * on).sum(-1, keepdim=True)
    if mode == "sparsemax":
        tau = (c - 1) / k
        return ((k - 1) * U * Aabs + U * (c - 1).abs()) / k + U * tau.abs() + U * p
    mean = c / k
    Em = ((k - 1) * U * Aabs + U * c.abs()) / k
    dj = (xs - mean) * on
    ss = (dj * dj).sum(-1, keepdim=True)
    Ess = k * U * ss + (2 * dj.abs() * (Em + U * dj.abs())).sum(-1, keepdim=True)
    v = (1 - ss) / k
    Ev = (Ess + U * (1 - ss).abs()) / k + U * v
    sq = v.sqrt()
    Esq = Ev / (2 * sq) + U * sq
    tau = mean - sq
    Et = Em + Esq + U * tau.abs()
    dd = torch.clamp(x - tau, min=0)
    return 2 * dd * (Et + U * dd) + U * p


def combine_bound(S, scale):
    return (S // 16 + 5) * U * scale


def dp_bound(scale):
    return 18 * U * scale


def dz_bound(p, dp, Edp, mode):
    """Elementwise bound on the kernel's dz given ITS OWN p [..., S] (as float64), the float64 dp and dp's bound; zero off the support."""
    on = (p > 0).double()
    k = on.sum(-1, keepdim=True)
    if mode == "sparsemax":
        dz = R.sparsemax_backward(p, dp)
        return on * (Edp + (Edp * on).sum(-1, keepdim=True) / k + 9 * U * (dp.abs() * on).sum(-1, keepdim=True) / k + U * dz.abs())
    q = p.sqrt()
    dd = dp * q
    Ed = q * Edp + 2 * U * dd.abs()
    N, D = dd.sum(-1, keepdim=True), q.sum(-1, keepdim=True)
    EN = Ed.sum(-1, keepdim=True) + 7 * U * dd.abs().sum(-1, keepdim=True)
    ED = 8 * U * D
    qq = N / D
    Eqq = EN / D + N.abs() * ED / (D * D) + U * qq.abs()
    r = dd - qq * q
    return on * (Ed + Eqq * q + 2 * U * qq.abs() * q + U * r.abs())


DX_C = 2


def dx_cols_ref(p, d_out):
    """dx[b, s, c] = sum_a p[a, b, s] d_out[a, b, c] (the columns where u is zero) and the two-fmaf bound."""
    return torch.einsum("abs,abd->bsd", p, d_out), DX_C * 2 * U * torch.einsum("abs,abd->bsd", p.abs(), d_out.abs())


def fma32(a, b, c):
    """fmaf on float32 tensors: the product is exact in float64, the sum rounded to float64 and then to float32."""
    return (a.double() * b.double() + c.double()).float()


def combine_chain32(p, Hs):
    """adapter_combine_kernel's own order in float32: row group rg = s % 16 runs its S/16 rows through fmaf, the four groups of a wave
    (rg = 4 w + i) meet by the xor-16 and xor-32 shuffles, the four waves are added in ascending order.  p [2, B, S], Hs [B, S, 768]."""
    p, Hs = p.float(), Hs.float()
    A, B, S = p.shape
    acc = torch.zeros(A, B, 16, Hs.shape[-1], dtype=F32)
    for s0 in range(0, S, 16):
        acc = fma32(p[:, :, s0:s0 + 16, None], Hs[None, :, s0:s0 + 16, :], acc)
    acc = acc.view(A, B, 4, 4, -1)                                   # [wave, i]
    w = (acc[:, :, :, 0] + acc[:, :, :, 1]) + (acc[:, :, :, 2] + acc[:, :, :, 3])      # xor 16 then xor 32
    return ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]


def dx_chain32(p, d_out):
    """adapter_dzdh_kernel's columns where u is zero, in float32: fmaf(p_1, d_1, fmaf(p_0, d_0, 0))."""
    p, d = p.float(), d_out.float()
    t = fma32(p[0][:, :, None], d[0][:, None, :], torch.zeros((), dtype=F32))
    return fma32(p[1][:, :, None], d[1][:, None, :], t)


def wgrad_bounds(mode, G, d):
    """{(side, dest): bound} of a weight-gradient case and the float64 reference: WGRAD_BOUND, or four times the float32 restatement's
    own error where that is larger."""
    ref = TR.reference_grads(mode, G, d["ws"], d["qs"], d["Hs"], d["d_out"])
    e32 = TR.f32_error(ref, TR.reference_grads(mode, G, d["ws"], d["qs"], d["Hs"], d["d_out"], dtype=F32))
    return {k: max(WGRAD_BOUND, 4 * e) for k, e in e32.items()}, ref, e32
