"""Torch restatement of the EMNLP scripts' sentence adapters (drl_classifier_ec_mmd_final_mul_emnlp.py :162-256, :334-354) for the
tests: the entmax-1.5 and sparsemax normalisers from their sort-based definitions (the `entmax` / `sparsemax` packages the reference
imports), differentiable, in any float dtype, and the adapters computed the reference's way (q_proj / k_proj projections of every
position, no reassociation) so that the kernels' reassociated form is checked against the literal one."""
import math

import torch

H = 768


def entmax15(z, dim=-1):
    """entmax-1.5 along `dim`: x = (z - max z) / 2, tau from the sorted prefix statistics, p = max(x - tau, 0)^2."""
    x = (z - z.max(dim=dim, keepdim=True).values) / 2
    xs = torch.sort(x, dim=dim, descending=True).values
    n = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = n
    k = torch.arange(1, n + 1, dtype=x.dtype, device=x.device).view(shape)
    mean = xs.cumsum(dim) / k
    # ss_k = sum_{j <= k} (xs_j - mean_k)^2, written out (well conditioned in any dtype)
    xs_t, mean_t = xs.movedim(dim, -1), mean.movedim(dim, -1)
    tri = torch.tril(torch.ones(n, n, dtype=x.dtype, device=x.device))            # [k, j]: j <= k
    ss = (((xs_t.unsqueeze(-2) - mean_t.unsqueeze(-1)) ** 2) * tri).sum(-1).movedim(-1, dim)
    tau = mean - torch.sqrt(torch.clamp((1 - ss) / k, min=0))
    support = (tau <= xs).sum(dim=dim, keepdim=True)
    tau_star = tau.gather(dim, support - 1)
    return torch.clamp(x - tau_star, min=0) ** 2


def entmax15_backward(p, dp, dim=-1):
    g = p.sqrt()
    q = (g * dp).sum(dim, keepdim=True) / g.sum(dim, keepdim=True)
    return g * dp - q * g


def sparsemax(z, dim=-1):
    """sparsemax along `dim`: k* = max{k : 1 + k zs_k > sum_{j<=k} zs_j}, tau = (sum_{j<=k*} zs_j - 1) / k*."""
    z = z - z.max(dim=dim, keepdim=True).values
    zs = torch.sort(z, dim=dim, descending=True).values
    n = z.shape[dim]
    shape = [1] * z.dim()
    shape[dim] = n
    k = torch.arange(1, n + 1, dtype=z.dtype, device=z.device).view(shape)
    gt = (1 + k * zs > zs.cumsum(dim)).to(z.dtype)
    kstar = (gt * k).max(dim=dim, keepdim=True).values
    tau = ((gt * zs).sum(dim=dim, keepdim=True) - 1) / kstar
    return torch.clamp(z - tau, min=0)


def sparsemax_backward(p, dp, dim=-1):
    nz = (p != 0).to(dp.dtype)
    mean = (dp * nz).sum(dim, keepdim=True) / nz.sum(dim, keepdim=True)
    return nz * (dp - mean)


class _Entmax15(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, dim):
        p = entmax15(z, dim)
        ctx.save_for_backward(p)
        ctx.dim = dim
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        return entmax15_backward(p, dp, ctx.dim), None


class _Sparsemax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, dim):
        p = sparsemax(z, dim)
        ctx.save_for_backward(p)
        ctx.dim = dim
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        return sparsemax_backward(p, dp, ctx.dim), None


def entmax15_fn(z, dim=-1):
    return _Entmax15.apply(z, dim)


def sparsemax_fn(z, dim=-1):
    return _Sparsemax.apply(z, dim)


def adapter_weights(sd, side, dtype=torch.float64):
    """The adapter tensors of one side ("emotion" / "cause") out of a state_dict, as `dtype` CPU tensors."""
    p = side + "_adapter."
    return {k[len(p):]: v.detach().to("cpu", dtype) for k, v in sd.items() if k.startswith(p)}


def adapter_out(Hs, q, w, mode, heads=4):
    """One adapter on the last hidden states Hs [B, S, 768] with the fixed query q [768]: the reference's computation (autograd-able).
    mode "sparsemax" / "entmax": q_proj(q) . k_proj(Hs) / sqrt(768), normalised over all S positions, weighted sum of the raw Hs.
    mode "raw": nn.MultiheadAttention(768, heads) forward with (q, Hs, Hs), dropout 0, no mask."""
    B, S, _ = Hs.shape
    if mode in ("sparsemax", "entmax"):
        qp = q @ w["q_proj.weight"].T + w["q_proj.bias"]
        kp = Hs @ w["k_proj.weight"].T + w["k_proj.bias"]
        scores = (kp @ qp) / math.sqrt(H)                            # [B, S]
        p = entmax15_fn(scores, -1) if mode == "entmax" else sparsemax_fn(scores, -1)
        return torch.einsum("bs,bsd->bd", p, Hs), p
    Wi, bi = w["in_proj_weight"], w["in_proj_bias"]
    dh = H // heads
    qp = (q @ Wi[:H].T + bi[:H]).view(heads, dh)
    kp = (Hs @ Wi[H:2 * H].T + bi[H:2 * H]).view(B, S, heads, dh)
    vp = (Hs @ Wi[2 * H:].T + bi[2 * H:]).view(B, S, heads, dh)
    scores = torch.einsum("hd,bshd->bhs", qp, kp) / math.sqrt(dh)
    p = torch.softmax(scores, -1)
    ctx = torch.einsum("bhs,bshd->bhd", p, vp).reshape(B, H)
    return ctx @ w["out_proj.weight"].T + w["out_proj.bias"], p


def reference_state_keys(mode, heads=4):
    """{key: shape} of one reference adapter: nn.MultiheadAttention's own parameters plus, for the sparse modes, the three nn.Linear
    (:164-166 / :213-215) -- built from torch's own module, as the reference does."""
    m = torch.nn.MultiheadAttention(H, heads, batch_first=True)
    if mode in ("sparsemax", "entmax"):
        m.q_proj, m.k_proj, m.v_proj = torch.nn.Linear(H, H), torch.nn.Linear(H, H), torch.nn.Linear(H, H)
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def adapter_params(mode, heads=4, seed=0, kscale=1.0):
    """Adapter weights for both sides, regenerated from a frozen numpy stream (fixtures store the seed, not the weights): the
    reference modules' initial distributions -- nn.MultiheadAttention: xavier-uniform in_proj_weight, zero in_proj_bias / out_proj.bias,
    out_proj.weight U(+-1/sqrt(768)); q_proj / k_proj / v_proj: nn.Linear's U(+-1/sqrt(768)) -- with the key projection scaled by
    `kscale` (kscale >> 1 gives supports of a few tokens).  -> {state_dict key: f32 tensor}."""
    import numpy as np
    rs = np.random.RandomState(seed)
    out = {}
    for side in ("emotion", "cause"):
        for k, shape in reference_state_keys(mode, heads).items():
            if k == "in_proj_weight":
                b = math.sqrt(6.0 / (shape[0] + shape[1]))
            elif k in ("in_proj_bias", "out_proj.bias"):
                b = 0.0
            else:
                b = 1.0 / math.sqrt(H)
            t = torch.from_numpy(rs.uniform(-b, b, size=shape).astype(np.float32)) if b else torch.zeros(shape)
            if (k == "k_proj.weight") or (k == "in_proj_weight" and mode == "raw"):
                if k == "in_proj_weight":
                    t[H:2 * H] *= kscale
                else:
                    t *= kscale
            out["%s_adapter.%s" % (side, k)] = t
    return out
