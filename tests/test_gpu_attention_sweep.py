"""Both attention kernel families (csrc/attention.hip for S <= 128, csrc/attention_long.hip above) at every sequence length 32 .. 512
against HF eager attention in float64 on the same bf16 inputs (tests/gpu_util.py attn_ref_fp64), scored per (sample, head, 32-row
tile) block so that an error confined to one head or one partial tile cannot hide in the norm of a whole launch (block_rel_err):
prefix masks at the tile and block edges, holes, dropout up to the largest legal element offset, packing, q_rows and the MPNet bias.
Every output buffer (and the backward workspace, at exactly its declared size) sits between guard regions that must come back
unchanged.  Also the contract edges of the C ABI: odd dropout offsets, the 32-bit element index, a sample with no attended key."""
import ctypes as C

import numpy as np
import pytest
import torch

from carel_vae_amd import _lib as L
from oracle import carel_oracle as O
from tests.gpu_util import Guarded, attn_ref_fp64, block_rel_err

pytestmark = pytest.mark.gpu
NH, HD, H = 12, 64, 768
SEQS = list(range(32, 513, 32))
# 1.5x the worst block errors over this module's cases measured on an MI355X: (blocks at or above the floor of block_rel_err, blocks
# below it); dtable: per head of the table gradient
BOUND = {"ctx": (4.8e-3, 2.5e-3), "dq": (0.20, 0.50), "dk": (0.058, 2.6), "dv": (6.7e-3, 5.1e-3), "dtable": (0.026,)}
ERR_ARG, ERR_SHAPE = -1, -2


def check(name, errs, tag):
    """errs: block_rel_err's ((error, where) of the blocks above its floor, (error, where) of those below)."""
    for (e, where), bound in zip(errs, BOUND[name]):
        assert e <= bound, (name, e, bound, tag, where)


def bits_equal(x, y):
    return torch.equal(x.view(torch.int16) if x.element_size() == 2 else x.view(torch.int32),
                       y.view(torch.int16) if y.element_size() == 2 else y.view(torch.int32))


class Attn:
    """One forward (and with dctx one backward) through the C ABI, every output guarded.  fill: initial value of ctx / lse / dqkv."""

    def __init__(self, qkv, B, S, mask=None, cu=None, drop=(0, 0, 0, 0.0), dctx=None, table=None, q_rows=0, fill=float("nan"),
                 lse_fill=None):
        self.lib, self.B, self.S, self.fill = L.load(), B, S, fill
        g = torch.Generator().manual_seed(B * 1000 + S)
        rows = qkv.shape[0]
        self.bufs = [Guarded((rows, H), torch.bfloat16, fill, g), Guarded((B, NH, S), torch.float32, fill if lse_fill is None else lse_fill, g)]
        self.ctx, self.lse = self.bufs[0].t, self.bufs[1].t
        self.cu_t = None if cu is None else torch.tensor(cu, dtype=torch.int32, device="cuda")
        a = self.a = L.AttnArgs()
        a.qkv, a.attention_mask = qkv.data_ptr(), (None if mask is None else mask.data_ptr())
        a.ctx, a.lse = self.bufs[0].ptr, self.bufs[1].ptr
        a.batch, a.seq_len, a.heads, a.head_dim = B, S, NH, HD
        a.drop_seed, a.drop_site, a.drop_idx_offset, a.drop_p = drop
        a.cu_seqlens = None if cu is None else self.cu_t.data_ptr()
        a.q_rows = q_rows
        self.table, self.span = table, (256 if S <= 128 else 1024)
        if table is not None:
            self.bucket = O.mpnet_relative_position_bucket(torch.arange(1 - self.span // 2, self.span // 2 + 1)).to(torch.int32).cuda().contiguous()
            self.dist = torch.empty((NH, self.span), device="cuda")
            L.check(self.lib.carel_relpos_expand_span(table.data_ptr(), self.bucket.data_ptr(), self.dist.data_ptr(), self.span,
                                                      L.current_stream()), "relpos expand")
            a.rel_bias_dist = self.dist.data_ptr()
        self.rc_fwd = self.lib.carel_attention_fwd(C.byref(a), L.current_stream())
        self.dqkv = self.ddist = self.dtable = None
        if dctx is not None and self.rc_fwd == 0:
            self.bufs.append(Guarded((rows, 3 * H), torch.bfloat16, fill, g))
            self.dqkv = self.bufs[-1].t
            need = self.lib.carel_attention_bwd_workspace_bytes(B, S, 0 if table is None else 1)
            self.bufs.append(Guarded((need,), torch.uint8, 0xCD, g))
            a.dctx, a.dqkv = dctx.data_ptr(), self.bufs[2].ptr
            a.workspace, a.workspace_bytes = self.bufs[3].ptr, need
            if table is not None:
                self.bufs.append(Guarded((B * NH, self.span), torch.float32, 0.0, g))
                self.ddist = self.bufs[-1].t
                a.d_rel_bias_dist = self.bufs[-1].ptr
            self.backward()
        torch.cuda.synchronize()

    def backward(self):
        self.rc_bwd = self.lib.carel_attention_bwd(C.byref(self.a), L.current_stream())
        if self.rc_bwd == 0 and self.table is not None:
            self.dtable = torch.empty((32, NH), device="cuda")
            L.check(self.lib.carel_relpos_reduce_span(self.ddist.data_ptr(), self.B, self.bucket.data_ptr(), self.dtable.data_ptr(), 0,
                                                      self.span, L.current_stream()), "relpos reduce")
        torch.cuda.synchronize()

    def ok(self):
        assert self.rc_fwd == 0, L.load().carel_last_error().decode()
        assert self.dqkv is None or self.rc_bwd == 0, L.load().carel_last_error().decode()
        return self

    def guards_intact(self):
        return all(b.intact() for b in self.bufs)


def check_run(run, ref, segs, tag, mask=None, q_rows=0):
    """The checks of every case: block errors of ctx / dQ / dK / dV, lse element by element, every output finite, exact zeros for the
    dK / dV of masked keys, a second backward bitwise identical to the first (bias: also its gradient), and intact guards."""
    rctx, rlse, rdqkv, rdtab = ref
    qsegs = [(r0, min(n, q_rows)) for r0, n in segs] if q_rows else segs
    check("ctx", block_rel_err(run.ctx, rctx, qsegs), tag)
    for b, (r0, n) in enumerate(qsegs):
        got, want = run.lse[b, :, :n], rlse[b, :, :n]
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(run.ctx[r0:r0 + n].float()).all()), (tag, b)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=str((tag, b)))
    if run.dqkv is None:
        return
    for name, c0, sg in (("dq", 0, qsegs), ("dk", H, segs), ("dv", 2 * H, segs)):
        check(name, block_rel_err(run.dqkv[:, c0:c0 + H], rdqkv[:, c0:c0 + H], sg), tag)
    for r0, n in segs:
        assert bool(torch.isfinite(run.dqkv[r0:r0 + n].float()).all()), tag
    if mask is not None:
        for b in range(run.B):
            pad = (mask[b] == 0).nonzero().flatten()
            if len(pad):
                assert float(run.dqkv[b * run.S + pad, H:].float().abs().max()) == 0.0, (tag, b)
    if run.table is not None:
        de = (run.dtable.double() - rdtab).norm(dim=0) / rdtab.norm(dim=0)
        check("dtable", ((float(de.max()), int(de.argmax())),), tag)
    first = (run.dqkv.clone(), None if run.ddist is None else run.ddist.clone(), None if run.dtable is None else run.dtable.clone())
    run.dqkv.fill_(run.fill)
    if run.ddist is not None:
        run.ddist.zero_()
    run.backward()
    assert run.rc_bwd == 0
    assert bits_equal(first[0], run.dqkv), tag
    if run.ddist is not None:
        assert bits_equal(first[1], run.ddist) and bits_equal(first[2], run.dtable), tag
    assert run.guards_intact(), tag


def prefix_mask(S, lens):
    m = torch.zeros((len(lens), S), dtype=torch.int64)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


def prefix_lens(S):
    return sorted({n for n in (1, 31, 32, 33, 127, 128, 129, S - 1, S) if 1 <= n <= S})


def sweep_masks(S):
    """One prefix mask per length at the tile and block edges; then holes, a masked first key, and for S >= 256 / 384 a masked
    128-key block at the start / inside a live sample (the model takes such masks dense)."""
    rows = [prefix_mask(S, prefix_lens(S))]
    holes = torch.ones((1, S), dtype=torch.int64)
    holes[0, 3::7] = 0
    first = torch.ones((1, S), dtype=torch.int64)
    first[0, 0] = 0
    rows += [holes, first]
    if S >= 256:
        blk = torch.ones((1, S), dtype=torch.int64)
        blk[0, :128] = 0
        rows.append(blk)
    if S >= 384:
        blk = torch.ones((1, S), dtype=torch.int64)
        blk[0, 128:256] = 0
        rows.append(blk)
    return torch.cat(rows).cuda()


def inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn((rows, 3 * H), generator=g) * 1.5).cuda().bfloat16()
    dctx = torch.randn((rows, H), generator=g).cuda().bfloat16()
    return qkv, dctx


def dense_case(S, B, mask, drop, qkv, dctx, tag, table=None):
    run = Attn(qkv, B, S, mask, drop=drop, dctx=dctx, table=table).ok()
    ref = attn_ref_fp64(qkv, dctx, B, S, mask=mask, drop=drop, table=table)
    check_run(run, ref, [(b * S, S) for b in range(B)], tag, mask=mask)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", SEQS)
def test_dense_sweep_masks(S, p):
    """Every S: one sample per prefix length at the tile / block edges plus holes and masked key blocks; with dropout, the largest
    legal element offset 2^32 - B*12*S*S at S = 96 (short kernels) and S = 320 (long kernels)."""
    mask = sweep_masks(S)
    B = mask.shape[0]
    off = 2 ** 32 - B * NH * S * S if (p > 0 and S in (96, 320)) else 2 * NH * S * S
    qkv, dctx = inputs(B * S, S * 10 + int(p * 10))
    dense_case(S, B, mask, (31, O.site_attn_probs(2), off, p), qkv, dctx, ("masks", S, p, off))


@pytest.mark.parametrize("S", SEQS)
def test_dense_sweep_no_mask(S):
    B = 2
    qkv, dctx = inputs(B * S, S * 10 + 7)
    dense_case(S, B, None, (8, O.site_attn_probs(0), 4 * NH * S * S, 0.1), qkv, dctx, ("nomask", S))


@pytest.mark.parametrize("S", SEQS)
def test_dense_sweep_large_score_range(S):
    """Scores spanning more than 40 nats, every row's maximum among the last 32 keys (the last, partial key block whenever
    S % 128 != 0): the online softmax rescales its running sums by large factors.  Sample 1 has its last 8 keys masked."""
    B, c, nb = 2, 20.0, min(32, S // 2)
    g = torch.Generator().manual_seed(S + 5)
    x = torch.randn((B * S, 3 * H), generator=g) * 1.5
    u = torch.randn((NH, HD), generator=g)
    u = (u / u.norm(dim=1, keepdim=True)).reshape(H) * c
    x[:, :H] += u                                             # every query
    for b in range(B):
        x[b * S + S - nb:(b + 1) * S, H:2 * H] += u           # the last 32 keys of each sample (S = 32: 16)
    qkv = x.cuda().bfloat16()
    dctx = torch.randn((B * S, H), generator=g).cuda().bfloat16()
    mask = prefix_mask(S, [S, S - 8]).cuda()
    s = torch.einsum("qhd,khd->hqk", qkv[:S, :H].double().view(S, NH, HD), qkv[:S, H:2 * H].double().view(S, NH, HD)) / 8
    assert float((s.amax(-1) - s.amin(-1)).min()) > 40 and bool((s.argmax(-1) >= S - nb).all())
    dense_case(S, B, mask, (3, O.site_attn_probs(5), 0, 0.1), qkv, dctx, ("range", S))


@pytest.mark.parametrize("S", [32, 96, 160, 192, 224, 320, 480])
def test_packed_sweep(S):
    """cu_seqlens: sample lengths at the tile and block edges (one of length S) back to back; rows past the last sample and lse past each
    sample's length keep their sentinels."""
    lens = []
    for n in (33, 1, S, 127, 31, 129, 64, S - 31, 32, 128, 65, S - 1, 63):
        if 1 <= n <= S and n not in lens:
            lens.append(n)
    B = len(lens)
    cu = [0] + [int(v) for v in np.cumsum(lens)]
    T = cu[-1]
    qkv, dctx = inputs(B * S, S + 3)
    drop = (5, O.site_attn_probs(3), 6 * NH * S * S, 0.1)
    run = Attn(qkv, B, S, cu=cu, drop=drop, dctx=dctx, fill=7.0, lse_fill=-7.0).ok()
    assert float((run.ctx[T:].float() - 7.0).abs().max()) == 0.0 and float((run.dqkv[T:].float() - 7.0).abs().max()) == 0.0
    for b, n in enumerate(lens):
        assert bool((run.lse[b, :, n:] == -7.0).all()), (b, n)
    ref = attn_ref_fp64(qkv, dctx, B, S, cu=cu, drop=drop)
    check_run(run, ref, [(cu[b], n) for b, n in enumerate(lens)], ("packed", S))


@pytest.mark.parametrize("S,q_rows", [(S, q) for S in (96, 160, 192, 224, 480) for q in (32, 64, 96) if q < S])
def test_query_row_limit_sweep(S, q_rows):
    """q_rows: live rows bitwise equal to the unrestricted launch (dctx zero past q_rows, as the encoder hands it over), rows past it
    not written (ctx / lse) or zero (dQ); the live rows and every dK / dV against fp64."""
    lens = [S, S - 1, 33, 1]
    B = len(lens)
    mask = prefix_mask(S, lens).cuda()
    qkv, dctx = inputs(B * S, S * 3 + q_rows)
    dctx.view(B, S, H)[:, q_rows:] = 0
    drop = (12, O.site_attn_probs(1), 0, 0.1)
    full = Attn(qkv, B, S, mask, drop=drop, dctx=dctx).ok()
    run = Attn(qkv, B, S, mask, drop=drop, dctx=dctx, q_rows=q_rows).ok()
    live = torch.zeros((B, S), dtype=torch.bool, device="cuda")
    live[:, :q_rows] = True
    assert bits_equal(run.ctx.view(B, S, H)[live], full.ctx.view(B, S, H)[live])
    assert bool(torch.isnan(run.ctx.view(B, S, H)[~live].float()).all())
    assert bits_equal(run.lse[:, :, :q_rows].contiguous(), full.lse[:, :, :q_rows].contiguous()) and bool(torch.isnan(run.lse[:, :, q_rows:]).all())
    assert torch.equal(run.dqkv.float(), full.dqkv.float())       # (+0 against -0 is the only licence)
    assert bool((run.dqkv.view(B, S, 3 * H)[:, q_rows:, :H] == 0).all())
    ref = attn_ref_fp64(qkv, dctx, B, S, mask=mask, drop=drop)
    check_run(run, ref, [(b * S, S) for b in range(B)], ("q_rows", S, q_rows), mask=mask, q_rows=q_rows)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("S", [32, 96, 160, 192, 480])
def test_relative_position_bias_sweep(S, packed):
    """MPNet bias by distance (span 256 for S <= 128, 1024 above: the bias partials round the key blocks up) through
    carel_relpos_expand_span / carel_relpos_reduce_span: forward, backward and the [32, 12] table gradient against fp64 autograd."""
    lens = []
    for n in (S, S - 31, 33, 1):
        if 1 <= n <= S and n not in lens:
            lens.append(n)
    B = len(lens)
    g = torch.Generator().manual_seed(S + 11)
    table = (torch.randn((32, NH), generator=g) * 0.7).cuda()
    qkv, dctx = inputs(B * S, S * 7 + packed)
    drop = (9, O.site_attn_probs(1), 0, 0.1)
    if packed:
        cu = [0] + [int(v) for v in np.cumsum(lens)]
        run = Attn(qkv, B, S, cu=cu, drop=drop, dctx=dctx, table=table, fill=7.0).ok()
        ref = attn_ref_fp64(qkv, dctx, B, S, cu=cu, drop=drop, table=table)
        check_run(run, ref, [(cu[b], n) for b, n in enumerate(lens)], ("bias packed", S))
    else:
        mask = prefix_mask(S, lens).cuda()
        dense_case(S, B, mask, drop, qkv, dctx, ("bias dense", S), table=table)


# ------------------------------------------------------------------------------------------------ contract edges of the C ABI

def keep_probe(S, off, lib_check=True):
    """The dropout decisions the kernels apply, read back exactly: Q = K = 0 (uniform probabilities over the live keys), V = the one-hot
    of the key's position inside a 64-key live window, so ctx[q, head, d] != 0 iff (q, key d of the window) is kept; dO = the one-hot of
    the query for queries 0..63, so dV[key, head, d] != 0 iff (query d, key) is kept.  Sample 0 attends to keys 0..63, sample 1 to
    keys S-64..S-1.  Returns (forward decisions [2, 12, S, 64], backward decisions [2, 12, 64, 64] (query, key)) or the error code."""
    B, p = 2, 0.1
    win = [0, S - 64]
    mask = torch.zeros((B, S), dtype=torch.int64)
    qkv = torch.zeros((B * S, 3 * H))
    dctx = torch.zeros((B * S, H))
    for b in range(B):
        mask[b, win[b]:win[b] + 64] = 1
        for d in range(64):
            qkv[b * S + win[b] + d, 2 * H + d:3 * H:HD] = 1.0
            dctx[b * S + d, d::HD] = 1.0
    qkv, dctx, mask = qkv.cuda().bfloat16(), dctx.cuda().bfloat16(), mask.cuda()
    run = Attn(qkv, B, S, mask, drop=(21, O.site_attn_probs(7), off, p), dctx=dctx)
    if run.rc_fwd or run.rc_bwd:
        return run.rc_fwd or run.rc_bwd
    fwd = torch.stack([run.ctx[b * S:(b + 1) * S].view(S, NH, HD).permute(1, 0, 2) != 0 for b in range(B)])
    bwd = torch.stack([run.dqkv[b * S + win[b]:b * S + win[b] + 64, 2 * H:].view(64, NH, HD).permute(1, 2, 0) != 0 for b in range(B)])
    return fwd, bwd


def keep_expected(S, off):
    keep = O.dropout_keep(21, O.site_attn_probs(7), (np.arange(2 * NH * S * S, dtype=np.uint64) + np.uint64(off)).astype(np.uint32), 0.1)
    keep = torch.from_numpy(keep).view(2, NH, S, S)
    fwd = torch.stack([keep[0, :, :, :64], keep[1, :, :, S - 64:]])
    bwd = torch.stack([keep[0, :, :64, :64], keep[1, :, :64, S - 64:]])
    return fwd, bwd


@pytest.mark.parametrize("S", [128, 256, 480])
def test_dropout_decisions_equal_the_documented_masks(S):
    """At the largest legal (even) element offset, the decisions of the forward and of the backward are exactly O.dropout_keep's."""
    off = 2 ** 32 - 2 * NH * S * S
    fwd, bwd = keep_probe(S, off)
    efwd, ebwd = keep_expected(S, off)
    assert torch.equal(fwd.cpu(), efwd) and torch.equal(bwd.cpu(), ebwd)


@pytest.mark.parametrize("S", [128, 256])
def test_odd_dropout_offset_is_refused(S):
    """The kernels hash whole pairs of elements starting at an even index: with dropout on, an odd drop_idx_offset is refused (forward
    and backward) before any launch; with dropout off the offset is not used and any value is accepted."""
    B = 2
    qkv, dctx = inputs(B * S, S + 1)
    run = Attn(qkv, B, S, drop=(1, 1, 2 * NH * S * S + 1, 0.1), dctx=dctx)
    assert run.rc_fwd == ERR_ARG and "even" in L.load().carel_last_error().decode()
    assert bool(torch.isnan(run.ctx.float()).all()) and bool(torch.isnan(run.lse).all())
    ok = Attn(qkv, B, S, drop=(1, 1, 2 * NH * S * S, 0.1), dctx=dctx).ok()
    ok.a.drop_idx_offset = 2 * NH * S * S + 1
    ok.dqkv.fill_(float("nan"))
    ok.backward()
    assert ok.rc_bwd == ERR_ARG and bool(torch.isnan(ok.dqkv.float()).all())
    odd = Attn(qkv, B, S, drop=(1, 1, 7, 0.0), dctx=dctx).ok()
    even = Attn(qkv, B, S, drop=(1, 1, 0, 0.0), dctx=dctx).ok()
    assert bits_equal(odd.ctx, even.ctx) and bits_equal(odd.lse, even.lse) and bits_equal(odd.dqkv, even.dqkv)


def test_dropout_index_wrap_is_refused_on_the_short_path():
    """S = 128, B = 1: an offset past 2^32 - 12*128*128 would wrap the 32-bit element index; refused before any launch."""
    S, B = 128, 1
    qkv, dctx = inputs(B * S, 5)
    last = 2 ** 32 - NH * S * S
    for off, rc in ((last + 1, None), (last + 2, ERR_SHAPE)):
        run = Attn(qkv, B, S, drop=(1, 1, off, 0.1), dctx=dctx)
        assert run.rc_fwd != 0 and (rc is None or run.rc_fwd == rc), (off, run.rc_fwd)
        assert bool(torch.isnan(run.ctx.float()).all()) and bool(torch.isnan(run.lse).all())
    Attn(qkv, B, S, drop=(1, 1, last, 0.1), dctx=dctx).ok()
    Attn(qkv, B, S, drop=(1, 1, last + 2, 0.0), dctx=dctx).ok()          # dropout off: no element index


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [128, 256])
def test_sample_with_no_attended_key(S, p):
    """A sample whose mask is all zeros: the forward gives HF's uniform row (the mean of the dropped-out V rows), the backward the
    documented exact zeros for all of its dQ / dK / dV rows (HF autograd would give nonzero dK / dV); the other sample is unaffected."""
    B = 2
    mask = prefix_mask(S, [S - 5, 0]).cuda()
    qkv, dctx = inputs(B * S, S + 17)
    drop = (4, O.site_attn_probs(2), 0, p)
    run = Attn(qkv, B, S, mask, drop=drop, dctx=dctx).ok()
    rctx, rlse, rdqkv, _ = attn_ref_fp64(qkv, dctx, B, S, mask=mask, drop=drop)
    check("ctx", block_rel_err(run.ctx, rctx, [(0, S), (S, S)]), ("no key", S, p))
    if p == 0:
        assert float((rctx[S:] - rctx[S:].mean(0)).abs().max()) < 1e-12          # the uniform row: every query gets the mean of V
    assert bool(torch.isfinite(run.lse).all()) and bool(torch.isfinite(run.ctx.float()).all())
    np.testing.assert_allclose(run.lse[0].cpu().numpy(), rlse[0].cpu().numpy(), rtol=1e-4, atol=1e-4)
    assert bool(torch.isfinite(run.dqkv.float()).all()) and float(run.dqkv[S:].float().abs().max()) == 0.0
    for name, c0 in (("dq", 0), ("dk", H), ("dv", 2 * H)):
        check(name, block_rel_err(run.dqkv[:S, c0:c0 + H], rdqkv[:S, c0:c0 + H], [(0, S)]), ("no key", S, p))
    assert run.guards_intact()
