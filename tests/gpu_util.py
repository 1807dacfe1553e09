"""Helpers for the -m gpu tests: all calls go through the C ABI (carel_vae_amd._lib)."""
import ctypes as C
import math

import numpy as np
import torch

from carel_vae_amd import _lib as L


def dev():
    return torch.device("cuda:0")


def to_bf16_bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 tensor -> bf16 tensor (round to nearest even), on the same device."""
    return t.to(torch.bfloat16)


def gemm(A, B, form, epi, M, N, K, splits=1, out_bf16=None, out2_bf16=None, out_f32=None, bias=None,
         resid=None, aux=None, drop=(0, 0, 0, 0.0), lda=None, ldb=None, ldc=None, colsum_part=None, colsum_a=None, splitk_ws=None,
         ws_zeroed=False, resid_ln=None, drop_row_map=None):
    a = L.GemmArgs()
    a.A, a.B = A.data_ptr(), B.data_ptr()
    a.lda = lda if lda is not None else A.stride(0)
    a.ldb = ldb if ldb is not None else B.stride(0)
    a.ldc = ldc if ldc is not None else N
    a.M, a.N, a.K = M, N, K
    a.form, a.epilogue, a.splits = form, epi, splits
    for name, t in (("out_bf16", out_bf16), ("out2_bf16", out2_bf16), ("out_f32", out_f32), ("bias", bias),
                    ("resid_f32", resid), ("aux_bf16", aux)):
        setattr(a, name, None if t is None else t.data_ptr())
    a.drop_seed, a.drop_site, a.drop_idx_offset, a.drop_p = drop
    a.drop_row_map = None if drop_row_map is None else drop_row_map.data_ptr()          # int32 [M]
    a.colsum_part = None if colsum_part is None else colsum_part.data_ptr()
    a.colsum_a = None if colsum_a is None else colsum_a.data_ptr()
    a.splitk_ws = None if splitk_ws is None else splitk_ws.data_ptr()
    a.splitk_ws_bytes = 0 if splitk_ws is None else splitk_ws.numel() * splitk_ws.element_size()
    a.splitk_ws_zeroed = 1 if ws_zeroed else 0
    if resid_ln is not None:           # (stats [M, 2], gamma [N], beta [N]): resid holds the pre-LayerNorm rows
        a.resid_ln_stats, a.resid_ln_gamma, a.resid_ln_beta = (t.data_ptr() for t in resid_ln)
    L.check(L.load().carel_gemm_bf16(C.byref(a), L.current_stream()), "carel_gemm_bf16")


def keep_mask(seed, site, n, p, off=0, device="cuda"):
    """Dropout multipliers (0 or 1/(1-p), float64) of the n elements off .. off + n - 1 (uint32, wrapping) from oracle.dropout_keep."""
    from oracle import carel_oracle as O
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(off)).astype(np.uint32)
    return torch.from_numpy(O.dropout_keep(seed, site, idx, p).astype(np.float64) / (1 - p)).to(device)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bits as integers on the CPU, so that torch.equal compares NaNs and signed zeros as bits."""
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class one_thread:
    """`with one_thread():` -- torch's CPU ops on one thread (many small tensors: a thread pool only gets in its own way)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / max(ref.norm().item(), 1e-30))


# ------------------------------------------------------------------------------------------------ attention: fp64 reference, block metric
ATT_NH, ATT_HD = 12, 64
ATT_H = ATT_NH * ATT_HD


def attn_keep(B, S, drop, device="cuda"):
    """Dropout multipliers [B, 12, S, S] (0 or 1/(1-p), float64) of the attention probabilities from oracle.dropout_keep: element
    ((b*12 + h)*S + q)*S + k + offset as a uint32 (wrapping); None for p <= 0."""
    from oracle import carel_oracle as O
    seed, site, off, p = drop
    if p <= 0:
        return None
    idx = (np.arange(B * ATT_NH * S * S, dtype=np.uint64) + np.uint64(off)).astype(np.uint32)
    keep = torch.from_numpy(O.dropout_keep(seed, site, idx, p)).to(device)
    return keep.view(B, ATT_NH, S, S).double() / (1.0 - p)


def _mpnet_bias(tab, n):
    """[12, n, n]: tab[bucket(key - query), head] (transformers MPNetAttention position_bias) from the [32, 12] table."""
    from oracle import carel_oracle as O
    pos = torch.arange(n)
    return tab[O.mpnet_relative_position_bucket(pos[None, :] - pos[:, None]).to(tab.device)].permute(2, 0, 1)


def _eager_fp64(qkv_rows, b, n, add, keep, bias):
    x = qkv_rows.double().view(b, n, 3, ATT_NH, ATT_HD).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                 # [b, 12, n, 64]
    s = q @ k.transpose(-1, -2) / math.sqrt(ATT_HD)
    if bias is not None:
        s = s + bias
    if add is not None:
        s = s + add
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep
    return x, (pr @ v).transpose(1, 2).reshape(b * n, ATT_H), lse


def attn_ref_fp64(qkv, dctx, B, S, mask=None, cu=None, drop=(0, 0, 0, 0.0), table=None):
    """HF eager attention in float64 on the kernels' own bf16 inputs: softmax(QK^T/8 [+ MPNet bias] + (1 - mask) * finfo(float32).min)
    -> dropout (attn_keep) -> PV, and its autograd backward for the upstream gradient dctx.  Packed (cu_seqlens, int list or tensor
    [B+1]): one call per sample on its own rows, no mask term.  table: the MPNet [32, 12] bias table (None = no bias).
    Returns (ctx [rows, 768], lse [B, 12, S] (nan past a packed sample), dqkv [rows, 2304], d table [32, 12] or None), float64 on
    qkv's device; rows of qkv outside every sample stay 0."""
    dev, rows = qkv.device, qkv.shape[0]
    keep = attn_keep(B, S, drop, dev)
    tab = None if table is None else table.detach().to(dev).double().requires_grad_(True)
    ctx = torch.zeros((rows, ATT_H), dtype=torch.float64, device=dev)
    dqkv = torch.zeros((rows, 3 * ATT_H), dtype=torch.float64, device=dev)
    lse = torch.full((B, ATT_NH, S), float("nan"), dtype=torch.float64, device=dev)
    if cu is None:
        add = None if mask is None else ((1.0 - mask.double()) * torch.finfo(torch.float32).min)[:, None, None, :]
        x, c, l = _eager_fp64(qkv[:B * S], B, S, add, keep, None if tab is None else _mpnet_bias(tab, S))
        c.backward(dctx[:B * S].double())
        ctx[:B * S], lse[:], dqkv[:B * S] = c.detach(), l.detach(), x.grad.reshape(B * S, 3 * ATT_H)
    else:
        cu = [int(v) for v in cu]
        for b in range(B):
            r0, n = cu[b], cu[b + 1] - cu[b]
            if n == 0:
                continue
            x, c, l = _eager_fp64(qkv[r0:r0 + n], 1, n, None, None if keep is None else keep[b:b + 1, :, :n, :n],
                                  None if tab is None else _mpnet_bias(tab, n))
            c.backward(dctx[r0:r0 + n].double())
            ctx[r0:r0 + n], lse[b, :, :n], dqkv[r0:r0 + n] = c.detach(), l.detach()[0], x.grad.reshape(n, 3 * ATT_H)
    return ctx, lse, dqkv, (None if tab is None else tab.grad)


def block_rel_err(got, ref, segs, floor=0.05):
    """Worst relative error over the (sample, head, 32-row tile) blocks of a [rows, 12 * 64] tensor; segs = [(first row, rows)] of the
    samples, tiles counted from each sample's first row (the last one partial).  A block's error is ||got - ref|| / max(||ref||,
    floor * median of the tensor's nonzero block norms): a block that is (nearly) zero in exact arithmetic is measured against the
    typical block instead of itself.  Returns ((error, (sample, tile, head))) of the blocks at or above that floor and of those below
    it, separately: below it the attention backward's error is that of delta = rowsum(dO * O) taken from the bf16 context rows (a
    query whose softmax sits on one key has an exact dQ of 0), which sets a looser bound than the other blocks need."""
    got = got.to(ref.device).double().reshape(-1, ATT_NH, ATT_HD)
    ref = ref.double().reshape(-1, ATT_NH, ATT_HD)
    rows, ids, where = [], [], []
    for s, (r0, n) in enumerate(segs):
        r = torch.arange(n, device=ref.device)
        rows.append(r0 + r)
        ids.append(len(where) + r // 32)
        where += [(s, t) for t in range((n + 31) // 32)]
    rows, ids = torch.cat(rows), torch.cat(ids)
    d2 = torch.zeros((len(where), ATT_NH), dtype=torch.float64, device=ref.device)
    r2 = torch.zeros_like(d2)
    d2.index_add_(0, ids, ((got[rows] - ref[rows]) ** 2).sum(-1))
    r2.index_add_(0, ids, (ref[rows] ** 2).sum(-1))
    dn, rn = d2.sqrt(), r2.sqrt()
    nz = rn[rn > 0]
    med = float(nz.median()) if nz.numel() else 0.0
    lim = max(floor * med, 1e-30)
    err = dn / rn.clamp(min=lim)
    out = []
    for sel in (rn >= lim, rn < lim):
        e = torch.where(sel, err, torch.zeros_like(err))
        i = int(e.argmax())
        out.append((float(e.flatten()[i]), where[i // ATT_NH] + (i % ATT_NH,)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ guarded output buffers
GUARD = 160 << 10          # bytes of random guard before and after every output buffer (more than 32 rows of the attention dqkv)


class Guarded:
    """A tensor of `shape` between two GUARD-byte regions of random bytes, in one allocation."""

    def __init__(self, shape, dtype, fill, gen):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device="cuda")
        self.pattern = torch.randint(0, 256, (2, GUARD), generator=gen, dtype=torch.uint8).cuda()
        self.buf[:GUARD] = self.pattern[0]
        self.buf[GUARD + self.nbytes:] = self.pattern[1]
        self.t = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        self.ptr = self.buf.data_ptr() + GUARD
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return torch.equal(self.buf[:GUARD], self.pattern[0]) and torch.equal(self.buf[GUARD + self.nbytes:], self.pattern[1])


class Arena:
    """The Guarded buffers of one case: nan() hands out a NaN-filled one, put() one holding a copy of `src`; intact() checks them all."""

    def __init__(self, seed=0):
        self.gen, self.all = torch.Generator().manual_seed(seed), []

    def nan(self, shape, dtype=torch.float32):
        self.all.append(Guarded(tuple(shape), dtype, float("nan"), self.gen))
        return self.all[-1]

    def put(self, src):
        self.all.append(Guarded(tuple(src.shape), src.dtype, None, self.gen))
        self.all[-1].t.copy_(src)
        return self.all[-1]

    def intact(self):
        return all(b.intact() for b in self.all)
