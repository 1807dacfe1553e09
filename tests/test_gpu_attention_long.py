"""Long-sequence attention (128 < S <= 512, csrc/attention_long.hip) against fp64 eager attention on the same bf16 inputs: padding
masks, dropout with the shared counter-based masks, token packing, q_rows, the MPNet relative-position bias and its table gradient
(span 1024), exact zeros for padded keys and bitwise-reproducible gradients."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from oracle import carel_oracle as O
from tests.gpu_util import rel_err

pytestmark = pytest.mark.gpu
NH, HD, H = 12, 64, 768
SPAN = 1024


def keep_mask(B, S, drop):
    seed, site, off, p = drop
    idx = (np.arange(B * NH * S * S, dtype=np.uint64) + np.uint64(off)).astype(np.uint32)
    return torch.from_numpy(O.dropout_keep(seed, site, idx, p).astype(np.float64) / (1 - p)).view(B, NH, S, S).cuda()


def attn_args(qkv, B, S, ctx, lse, mask=None, drop=(0, 0, 0, 0.0), dctx=None, dqkv=None, cu=None, rel=None, drel=None, q_rows=0):
    a = L.AttnArgs()
    a.qkv, a.attention_mask, a.ctx, a.lse = qkv.data_ptr(), (None if mask is None else mask.data_ptr()), ctx.data_ptr(), lse.data_ptr()
    a.batch, a.seq_len, a.heads, a.head_dim = B, S, NH, HD
    a.drop_seed, a.drop_site, a.drop_idx_offset, a.drop_p = drop
    a.q_rows = q_rows
    a.cu_seqlens = None if cu is None else cu.data_ptr()
    a.rel_bias_dist = None if rel is None else rel.data_ptr()
    a.d_rel_bias_dist = None if drel is None else drel.data_ptr()
    if dctx is not None:
        a.dctx, a.dqkv = dctx.data_ptr(), dqkv.data_ptr()
        n = L.load().carel_attention_bwd_workspace_bytes(B, S, 0 if rel is None else 1)
        ws = torch.empty(max(n, 1), device="cuda", dtype=torch.uint8)
        a.workspace, a.workspace_bytes = ws.data_ptr(), n
        a._ws = ws                              # keep alive with the struct
    return a


def run(a, bwd):
    lib = L.load()
    L.check(lib.carel_attention_fwd(C.byref(a), L.current_stream()), "attn fwd")
    if bwd:
        L.check(lib.carel_attention_bwd(C.byref(a), L.current_stream()), "attn bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,S,masked,p", [(2, 160, False, 0.0), (3, 256, True, 0.0), (2, 256, True, 0.1), (2, 384, False, 0.1),
                                           (2, 512, True, 0.0), (1, 512, True, 0.1)])
def test_long_attention_fwd_bwd(B, S, masked, p):
    g = torch.Generator().manual_seed(B * 1000 + S + int(p * 10))
    qkv = (torch.randn((B * S, 3 * H), generator=g) * 1.5).cuda().bfloat16()
    mask = None
    if masked:
        mask = torch.ones((B, S), dtype=torch.int64)
        for b in range(B):
            mask[b, int(torch.randint(3, S + 1, (1,), generator=g)):] = 0
        mask[0, S - 40:] = 0                      # at least one sample with padded keys
        mask = mask.cuda()
    dctx = torch.randn((B * S, H), generator=g).cuda().bfloat16()
    drop = (77, O.site_attn_probs(4), 3 * NH * S * S, p)
    ctx = torch.full((B * S, H), float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full((B, NH, S), float("nan"), device="cuda")
    dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
    a = attn_args(qkv, B, S, ctx, lse, mask, drop, dctx, dqkv)
    run(a, True)
    x = qkv.double().view(B, S, 3, NH, HD).requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(HD)
    if mask is not None:
        s = s + (1.0 - mask.double())[:, None, None, :] * torch.finfo(torch.float32).min
    pr = torch.softmax(s, dim=-1)
    if p > 0:
        pr = pr * keep_mask(B, S, drop)
    rctx = (pr @ v).transpose(1, 2).reshape(B * S, H)
    assert rel_err(ctx, rctx.detach()) < 8e-3
    np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(s, -1).detach().cpu().numpy(), rtol=1e-4, atol=1e-4)
    rctx.backward(dctx.double())
    rg = x.grad.reshape(B * S, 3 * H)
    got = dqkv.double()
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        e = rel_err(got[:, sl], rg[:, sl])
        assert e < 1.5e-2, (name, e)
    if masked:       # padded keys get exactly zero dK / dV
        for b in range(B):
            pad = (mask[b] == 0).nonzero().flatten()
            if len(pad):
                assert float(got[b * S + pad, H:].abs().max()) == 0.0
    assert torch.isfinite(got).all()
    # bitwise reproducible: a second backward gives the same bits
    first = dqkv.clone()
    dqkv.fill_(float("nan"))
    L.check(L.load().carel_attention_bwd(C.byref(a), L.current_stream()), "attn bwd 2")
    torch.cuda.synchronize()
    assert torch.equal(first, dqkv)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_attention_packed(p):
    """cu_seqlens: lengths around every tile and block edge in one call; rows past the samples are never written."""
    S = 512
    lens = [1, 127, 128, 129, 255, 256, 257, 511, 512]
    B = len(lens)
    T = sum(lens)
    Tp = (T + 127) // 128 * 128
    g = torch.Generator().manual_seed(5)
    qkv = torch.zeros((B * S, 3 * H), dtype=torch.bfloat16, device="cuda")
    qkv[:Tp] = (torch.randn((Tp, 3 * H), generator=g) * 1.5).cuda().bfloat16()
    dctx = torch.zeros((B * S, H), dtype=torch.bfloat16, device="cuda")
    dctx[:Tp] = torch.randn((Tp, H), generator=g).cuda().bfloat16()
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    ctx = torch.full((B * S, H), 7.0, device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros((B, NH, S), device="cuda")
    dqkv = torch.full((B * S, 3 * H), 7.0, device="cuda", dtype=torch.bfloat16)
    seed, site = 5, O.site_attn_probs(2)
    a = attn_args(qkv, B, S, ctx, lse, None, (seed, site, 0, p), dctx, dqkv, cu=cu)
    run(a, True)
    keep = keep_mask(B, S, (seed, site, 0, p)) if p > 0 else None
    start = 0
    for b, n in enumerate(lens):
        x = qkv[start:start + n].double().view(n, 3, NH, HD).requires_grad_(True)
        q, k, v = (x[:, i].transpose(0, 1) for i in range(3))
        pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(HD), dim=-1)
        if keep is not None:
            pr = pr * keep[b, :, :n, :n]
        out = (pr @ v).transpose(0, 1).reshape(n, H)
        assert rel_err(ctx[start:start + n], out.detach()) < 8e-3, (b, n)
        out.backward(dctx[start:start + n].double())
        e = rel_err(dqkv[start:start + n], x.grad.reshape(n, 3 * H))
        assert e < 1.5e-2, (b, n, e)
        start += n
    assert float((ctx[T:] - 7.0).abs().max()) == 0.0 and float((dqkv[T:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("packed", [False, True])
def test_long_attention_relative_position_bias(packed):
    """MPNet bias by distance [12][1024] (entry 511 + key - query) from carel_relpos_expand_span; its gradient by distance folded into
    the 32 x 12 table by carel_relpos_reduce_span; against fp64 autograd through the same bucket map; bitwise reproducible."""
    lib = L.load()
    g = torch.Generator().manual_seed(11)
    S = 384
    lens = [384, 200, 129, 31]
    B = len(lens)
    table = (torch.randn((32, NH), generator=g) * 0.7).cuda()
    rp = O.mpnet_relative_position_bucket(torch.arange(-511, 513)).to(torch.int32).cuda().contiguous()
    dist, ddist = torch.empty((NH, SPAN), device="cuda"), torch.zeros((B * NH, SPAN), device="cuda")
    L.check(lib.carel_relpos_expand_span(table.data_ptr(), rp.data_ptr(), dist.data_ptr(), SPAN, L.current_stream()), "relpos expand")
    T = sum(lens)
    if packed:
        Tp = (T + 127) // 128 * 128
        qkv = torch.zeros((B * S, 3 * H), dtype=torch.bfloat16, device="cuda")
        qkv[:Tp] = (torch.randn((Tp, 3 * H), generator=g) * 1.5).cuda().bfloat16()
        dctx = torch.zeros((B * S, H), dtype=torch.bfloat16, device="cuda")
        dctx[:Tp] = torch.randn((Tp, H), generator=g).cuda().bfloat16()
        cu, mask = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda"), None
        row0 = [int(v) for v in np.cumsum([0] + lens[:-1])]
    else:
        qkv = (torch.randn((B * S, 3 * H), generator=g) * 1.5).cuda().bfloat16()
        dctx = torch.randn((B * S, H), generator=g).cuda().bfloat16()
        mask = torch.zeros((B, S), dtype=torch.int64)
        for b, n in enumerate(lens):
            mask[b, :n] = 1
            dctx[b * S + n:(b + 1) * S] = 0
        mask, cu = mask.cuda(), None
        row0 = [b * S for b in range(B)]
    p, seed, site = 0.1, 9, O.site_attn_probs(1)
    ctx = torch.zeros((B * S, H), device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros((B, NH, S), device="cuda")
    dqkv = torch.zeros((B * S, 3 * H), device="cuda", dtype=torch.bfloat16)
    a = attn_args(qkv, B, S, ctx, lse, mask, (seed, site, 0, p), dctx, dqkv, cu=cu, rel=dist, drel=ddist)
    run(a, True)
    dtable = torch.empty((32, NH), device="cuda")
    L.check(lib.carel_relpos_reduce_span(ddist.data_ptr(), B, rp.data_ptr(), dtable.data_ptr(), 0, SPAN, L.current_stream()), "relpos reduce")
    torch.cuda.synchronize()
    keep = keep_mask(B, S, (seed, site, 0, p))
    tab = table.double().requires_grad_(True)
    worst = 0.0
    for b, n in enumerate(lens):
        r0 = row0[b]
        x = qkv[r0:r0 + n].double().view(n, 3, NH, HD).requires_grad_(True)
        q, k, v = (x[:, i].transpose(0, 1) for i in range(3))
        bias = tab[O.mpnet_relative_position_bucket(torch.arange(n)[None, :] - torch.arange(n)[:, None]).cuda()].permute(2, 0, 1)
        s = q @ k.transpose(-1, -2) / math.sqrt(HD) + bias
        pr = torch.softmax(s, dim=-1) * keep[b, :, :n, :n]
        out = (pr @ v).transpose(0, 1).reshape(n, H)
        assert rel_err(ctx[r0:r0 + n], out.detach()) < 8e-3, b
        np.testing.assert_allclose(lse[b, :, :n].cpu().numpy(), torch.logsumexp(s, -1).detach().cpu().numpy(), rtol=1e-4, atol=1e-4)
        out.backward(dctx[r0:r0 + n].double())
        worst = max(worst, rel_err(dqkv[r0:r0 + n], x.grad.reshape(n, 3 * H)))
    assert worst < 1.5e-2, worst
    assert rel_err(dtable, tab.grad) < 1e-2, rel_err(dtable, tab.grad)
    # accumulates (every encoder layer adds to the same buffer), and is bitwise reproducible
    first = (ddist.clone(), dqkv.clone())
    L.check(lib.carel_attention_bwd(C.byref(a), L.current_stream()), "attn bwd rel 2")
    torch.cuda.synchronize()
    assert torch.equal(ddist, 2 * first[0]) or rel_err(ddist, 2 * first[0]) < 1e-6
    ddist.zero_(); dqkv.zero_()
    L.check(lib.carel_attention_bwd(C.byref(a), L.current_stream()), "attn bwd rel 3")
    dtable2 = torch.empty((32, NH), device="cuda")
    L.check(lib.carel_relpos_reduce_span(ddist.data_ptr(), B, rp.data_ptr(), dtable2.data_ptr(), 0, SPAN, L.current_stream()), "relpos reduce")
    torch.cuda.synchronize()
    assert torch.equal(ddist, first[0]) and torch.equal(dqkv, first[1]) and torch.equal(dtable2, dtable)


def relpos_host(table, bucket, dd, batch, span):
    """carel_relpos_expand_span / carel_relpos_reduce_span restated on the host in the documented order, every add rounded to float32:
    dist[h][i] = table[bucket[i]][h] with the last entry 0; the gradient of (head, distance) is the sum over the samples in order
    starting from 0, and a bucket's is the sum of its distances in ascending order."""
    dist = np.zeros((NH, span), dtype=np.float32)
    dtable = np.zeros((32, NH), dtype=np.float32)
    for h in range(NH):
        for i in range(span - 1):
            dist[h, i] = table[bucket[i], h]
        t = [np.float32(0) for _ in range(32)]
        for i in range(span - 1):
            s = np.float32(0)
            for b in range(batch):
                s = np.float32(s + dd[b * NH + h, i])
            t[bucket[i]] = np.float32(t[bucket[i]] + s)
        for k in range(32):
            dtable[k, h] = t[k]
    return torch.from_numpy(dist), torch.from_numpy(dtable)


def relpos_span(span, batch, seed):
    lib = L.load()
    g = torch.Generator().manual_seed(seed)
    table = torch.randn((32, NH), generator=g).cuda()
    half = span // 2
    rp = O.mpnet_relative_position_bucket(torch.arange(-(half - 1), half + 1)).to(torch.int32).cuda().contiguous()
    d1 = torch.empty((NH, span), device="cuda")
    L.check(lib.carel_relpos_expand_span(table.data_ptr(), rp.data_ptr(), d1.data_ptr(), span, L.current_stream()), "expand span")
    dd = torch.randn((batch * NH, span), generator=g).cuda()
    t1 = torch.empty((32, NH), device="cuda")
    L.check(lib.carel_relpos_reduce_span(dd.data_ptr(), batch, rp.data_ptr(), t1.data_ptr(), 0, span, L.current_stream()), "reduce span")
    torch.cuda.synchronize()
    d_host, t_host = relpos_host(table.cpu().numpy(), rp.cpu().numpy(), dd.cpu().numpy(), batch, span)
    assert torch.equal(d1.cpu(), d_host) and torch.equal(t1.cpu(), t_host)
    return table, rp, dd, d1, t1


def test_relpos_span_256_matches_the_original_entry_points():
    """carel_relpos_expand / carel_relpos_reduce are the span-256 calls of the _span functions: equal bits, and both the bits of the
    host restatement (relpos_host)."""
    lib = L.load()
    table, rp, dd, d1, t1 = relpos_span(256, 3, 4)
    d0, t0 = torch.empty((NH, 256), device="cuda"), torch.empty((32, NH), device="cuda")
    L.check(lib.carel_relpos_expand(table.data_ptr(), rp.data_ptr(), d0.data_ptr(), L.current_stream()), "expand")
    L.check(lib.carel_relpos_reduce(dd.data_ptr(), 3, rp.data_ptr(), t0.data_ptr(), 0, L.current_stream()), "reduce")
    torch.cuda.synchronize()
    assert torch.equal(d0, d1) and torch.equal(t0, t1)


def test_relpos_span_1024_matches_the_host_restatement():
    relpos_span(1024, 2, 5)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_attention_query_row_limit(p):
    """q_rows = 32 at S = 512: the first query tile's ctx / lse bits equal the unrestricted launch's, the other rows are not written;
    with dctx zero off those rows, dK / dV / dQ equal the unrestricted launch's and dQ past the limit is zero."""
    B, S = 2, 512
    g = torch.Generator().manual_seed(77)
    qkv = (torch.randn((B * S, 3 * H), generator=g) * 1.5).cuda().bfloat16()
    mask = torch.ones((B, S), dtype=torch.int64); mask[1, 300:] = 0
    mask = mask.cuda()
    dctx = torch.zeros((B * S, H), device="cuda", dtype=torch.bfloat16)
    dctx.view(B, S, H)[:, 0] = torch.randn((B, H), generator=g).cuda().bfloat16()
    drop = (5, 7, 64, p)
    outs = []
    for qr in (0, 32):
        ctx = torch.full((B * S, H), float("nan"), device="cuda", dtype=torch.bfloat16)
        lse = torch.full((B, NH, S), float("nan"), device="cuda")
        dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
        a = attn_args(qkv, B, S, ctx, lse, mask, drop, dctx, dqkv, q_rows=qr)
        run(a, True)
        outs.append((ctx, lse, dqkv))
    (c0, l0, d0), (c1, l1, d1) = outs
    first = torch.zeros((B, S), dtype=torch.bool, device="cuda"); first[:, :32] = True
    assert torch.equal(c1.view(B, S, H)[first], c0.view(B, S, H)[first])
    assert bool(torch.isnan(c1.view(B, S, H)[~first].float()).all())
    assert torch.equal(l1[:, :, :32], l0[:, :, :32]) and bool(torch.isnan(l1[:, :, 32:]).all())
    assert torch.equal(d1.float(), d0.float())
    assert bool((d1.view(B, S, 3 * H)[:, 32:, :H] == 0).all())


def test_long_attention_rejects_bad_shapes_and_missing_workspace():
    lib = L.load()
    for S in (144, 544):
        qkv = torch.zeros((S, 3 * H), device="cuda", dtype=torch.bfloat16)
        ctx = torch.zeros((S, H), device="cuda", dtype=torch.bfloat16)
        lse = torch.zeros((1, NH, S), device="cuda")
        a = attn_args(qkv, 1, S, ctx, lse)
        assert lib.carel_attention_fwd(C.byref(a), L.current_stream()) == -2
    S = 256
    qkv = torch.zeros((S, 3 * H), device="cuda", dtype=torch.bfloat16)
    ctx, dctx = torch.zeros((S, H), device="cuda", dtype=torch.bfloat16), torch.zeros((S, H), device="cuda", dtype=torch.bfloat16)
    lse = torch.zeros((1, NH, S), device="cuda")
    dqkv = torch.zeros((S, 3 * H), device="cuda", dtype=torch.bfloat16)
    a = attn_args(qkv, 1, S, ctx, lse, None, (0, 0, 0, 0.0), dctx, dqkv)
    a.workspace, a.workspace_bytes = None, 0
    assert lib.carel_attention_bwd(C.byref(a), L.current_stream()) == -1
    # the 32-bit dropout element index: 1366 samples at S = 512 would wrap (checked before any launch)
    a = attn_args(qkv, 1366, 512, ctx, lse, None, (1, 1, 0, 0.1))
    assert lib.carel_attention_fwd(C.byref(a), L.current_stream()) == -2
    torch.cuda.synchronize()
