"""The batch-tiled loss step (carel_tail_losses_tiled: tail_heads_kernel over slabs of R = 64 rows, mmd_global_kernel on the batch's
own z, decoder_tiled_kernel over batch tiles of TB = 32 rows, 16 at ec_dim > 25) against oracle.carel_oracle.tail_forward in float64
on the same float32 inputs, in the form of tests/test_gpu_tail_sweep.py and with its tolerances: S = 2, every output starts as NaN,
the workspace / dx_last / z / decoder gradients sit between guard regions, two identical runs must give the same bits.

Batches over the limit of carel_tail_losses reach the tiled form by themselves (hip_tail goes through ops.tail_losses, which
dispatches on carel_tail_batch_limit); a case whose batch is at or below the limit of its width is driven through it by replacing
ops.tail_losses with ops.tail_losses_tiled.  Then the small batches (also against the single-workgroup path on the same inputs: z,
lat and pooled bit for bit, the rest printed), the data-parallel hooks over the limit, the refusals, and the dispatch at the limit.
Every case prints, per quantity, the worst fraction of its bound and the worst error over max|ref| (run with -s).  Worst over this
module on an MI355X: 0.10 of the bound on pooled, 0.04 on dx_last, 0.02 on lat / z / the gradients, below 0.005 on the terms."""
import ctypes as C

import pytest
import torch

from carel_vae_amd import _lib as L
from carel_vae_amd import ops
from tests.tail_restate import TAIL_KEYS, hip_tail, oracle_tail, setup
from tests.test_gpu_tail_sweep import (ERR_SHAPE, IT, S, SEED, TERMS, Report, _losses_args, _valid_run, bits, case, case_id, check_dx,
                                       check_local, outputs, pin_labels, run_checked)

pytestmark = pytest.mark.gpu
R, TB = 64, 32          # slab height of the heads kernel, batch tile of the decoder (csrc/tail.hip: TT_R; TB = 32 at 2 * ec_dim <= 50)


def _cases():
    c = [case(B) for B in (115, 150, 2 * R - 1, 2 * R, 2 * R + 1, 5 * TB - 1, 5 * TB, 5 * TB + 1, 257, 1024)]
    c += [case(143, D=8), case(128, D=16), case(102, D=32), case(257, D=32)]          # run-time-width decoder, zero-padded MMD; TB = 16
    c += [case(129, EC=2), case(129, EC=8)]
    c += [case(129, D=8, EC=1, head="bce"), case(129, D=24, EC=1, head="bce")]
    c += [case(129, dis="none")]
    c += [case(129, V=V) for V in (2, 127, 129, 8193)] + [case(128, V=23771)]
    c += [case(129, allneg=True), case(129, allneg=True, p=0.0)]
    c += [case(129, grad_out=2.5)]
    return c


CASES = _cases()
assert (5 * TB) % R and len({case_id(c) for c in CASES}) == len(CASES)
# Inputs are the sweep's, setup(B, 2, V, seed=B + V + D), except where that draw makes the yardstick itself unusable: at
# B129-D8-EC1-bce seed 394 gives a cause_classifier.bias gradient (one number: the sum of 129 terms of ~0.04) of 1.68e-4, a
# cancellation to 4e-5 of its summands, and the bound is relative to that number.  No float32 evaluation can meet it: the float32
# oracle itself sits at 4.44 of the bound against its float64 self on the CPU (the tiled kernels at 2.14 on an MI355X, every other
# quantity of the case below 0.05).  The case keeps its shape and its bound and takes the next draw, seed + 1000, at which the
# float32 oracle sits at 0.03 of the bound on every gradient -- a choice made on the reference's own error, not on the kernels'.
SEED_SHIFT = {"B129-D8-EC1-V257-mmd-bce": 1000}
assert set(SEED_SHIFT) <= {case_id(c) for c in CASES}


def limit_of(c):
    return L.load().carel_tail_batch_limit(c["D"], c["EC"])


def run_case(c, rep, monkeypatch, force):
    B, D, V = c["B"], c["D"], c["V"]
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + D + SEED_SHIFT.get(case_id(c), 0), all_negative=c["allneg"], ec_dim=D,
                                                     e_num_class=c["EC"], disentangle=c["dis"], emotion_head=c["head"])
    pin_labels(batch, c["allneg"])
    assert c["p"] in (0.0, opt.dropout)
    ref = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, c["p"] > 0, SEED, dtype=torch.float64)
    args = (P, x_last, batch, eps_e, eps_c, opt, B, S, V, IT, (c["p"], SEED, 0))
    if force:
        monkeypatch.setattr(ops, "tail_losses", ops.tail_losses_tiled)
    else:
        assert B > limit_of(c), "this case would not reach the tiled form"
    buf, G = run_checked(args, dict(grad_out=c["grad_out"]), rep)
    check_local(rep, buf, G, ref, B, D, c["grad_out"], 2e-4, 2e-5)
    return args, buf, G


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_tiled_tail(c, monkeypatch):
    rep = Report("tiled " + case_id(c))
    args, buf, G = run_case(c, rep, monkeypatch, force=c["B"] <= limit_of(c))          # (only B129-D8: the limit at ec_dim 8 is 142)
    if c["allneg"]:
        assert float(buf.terms[4]) == 0.0 and not bool(G["pair_classifier.weight"].any()) and not bool(G["pair_classifier.bias"].any())
        off = L.load().carel_tail_pair_dead_offset(c["B"], c["D"], c["V"])
        assert float(buf.work[off]) == 1.0
    rep.finish()


@pytest.mark.parametrize("B", [2, 7, 64, 114])
def test_small_batches_through_the_tiled_entry(B, monkeypatch):
    c = case(B)
    rep = Report("tiled-small " + case_id(c))
    args, buf, G = run_case(c, rep, monkeypatch, force=True)
    monkeypatch.undo()
    buf0, G0 = hip_tail(*args)                      # the single-workgroup path on the same inputs
    worst = []
    for (name, x), (_, y) in zip(outputs(buf, G), outputs(buf0, G0)):
        d, m = float((x - y).abs().max()), float(y.abs().max())
        worst.append("%s %.1e" % (name, d / m if m > 0 else d))
        if name in ("pooled", "lat", "z"):
            assert torch.equal(bits(x), bits(y)), (name, "differs from the single-workgroup path")
    print("tiled vs single-workgroup, B = %d, worst |difference| / max|single|: %s" % (B, "  ".join(worst)))
    rep.finish()


@pytest.mark.parametrize("Rk,Bl,D", [(2, 120, 24), (3, 115, 32)])
def test_tiled_tail_global_batch(Rk, Bl, D):
    """The data-parallel hooks with a local batch over the limit, in the layout of test_tail_sweep_global_batch: Rk shards,
    rank-averaged gradients and every rank's global statistic against the oracle on the unsharded batch."""
    assert Bl > L.load().carel_tail_batch_limit(D, 6)
    B, V = Rk * Bl, 257
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + D, ec_dim=D)
    pin_labels(batch, False)
    out, pooled, grads, dx = oracle_tail(P, x_last, batch, eps_e, eps_c, opt, B, S, IT, True, SEED, dtype=torch.float64)
    rep = Report("tiled-global-R%d-B%d-D%d" % (Rk, Bl, D))
    shards = [({k: v[r * Bl:(r + 1) * Bl] for k, v in batch.items()}, x_last[r * Bl * S:(r + 1) * Bl * S]) for r in range(Rk)]
    stride = Bl * 2 * D + 16
    packed = torch.full((Rk, stride), float("nan"), device="cuda")
    for r, (sb, xl) in enumerate(shards):          # pass 1: the latents of each shard -> "all-gather"
        buf, _ = hip_tail(P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl))
        packed[r, :Bl * 2 * D] = buf.z.reshape(-1)
        packed[r, Bl * 2 * D] = float(sb["labels"].sum())
    tot = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in P.items()}
    terms = torch.zeros(9, dtype=torch.float64)
    z_ref = torch.cat((out["z_e"], out["z_c"]), dim=1)
    for r, (sb, xl) in enumerate(shards):
        kw = dict(global_label_sum=packed.view(-1)[Bl * 2 * D:], global_n=B, global_row_offset=r * Bl, z_global=packed,
                  mmd_grad_scale=float(Rk), global_rank_stride=stride, global_label_ranks=Rk)
        buf, G = run_checked((P, xl, sb, eps_e, eps_c, opt, Bl, S, V, IT, (opt.dropout, SEED, r * Bl)), kw, rep)
        sl = slice(r * Bl, (r + 1) * Bl)
        rep.cmp("pooled%d" % r, buf.pooled, pooled[sl], 1e-5, 5e-6)
        rep.cmp("z%d" % r, buf.z, z_ref[sl], 1e-5, 2e-5)
        rep.cmp("mmd%d" % r, buf.terms[1].cpu(), out["mmd"], 3e-5, 2e-6, scale=abs(float(out["mmd"])))      # the global statistic on every rank
        check_dx(rep, buf.dx_last / Rk, dx[r * Bl * S:(r + 1) * Bl * S], Bl, 3e-4, 3e-5, "dx%d" % r)
        terms += buf.terms[:9].double().cpu() / Rk
        for k in tot:
            tot[k] += G[k].double().cpu() / Rk          # gradient averaging over ranks
    for i, k in TERMS[1:]:                              # equal shards: the mean of the ranks' means
        rep.cmp(k, terms[i], out[k], 1e-4, 1e-5, scale=abs(float(out[k])))
    for k in TAIL_KEYS:
        scale = float(grads[k].abs().max()) + 1e-12
        rep.cmp(k, tot[k], grads[k], 3e-4, 3e-5 * scale)
    rep.finish()


# ---- refusals: a batch past 1024, a batch of one without a global batch, HSIC (which keeps the single-workgroup limit)
@pytest.mark.parametrize("B,dis_mode,needle", [(1025, 0, "1024"), (1, 0, "batch must be >= 2"), (115, 1, "114")])
def test_tiled_refusals_come_before_anything_is_launched(B, dis_mode, needle):
    """CAREL_ERR_SHAPE naming carel_tail_losses_tiled; after a device synchronise terms, z, the classifier and decoder gradients and
    the workspace still hold the NaN sentinel bit for bit; a valid call before and after gives identical bits."""
    before = _valid_run()
    a, watched = _losses_args(B, 24)
    a.dis_mode = dis_mode
    snap = [(n, t.clone()) for n, t in watched]
    rc = L.load().carel_tail_losses_tiled(C.byref(a), L.current_stream())
    msg = L.load().carel_last_error().decode()
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE and "carel_tail_losses_tiled" in msg and needle in msg, (rc, msg)
    if dis_mode == 1:
        assert "HSIC" in msg
    for (n, t), (_, s) in zip(watched, snap):
        assert torch.equal(bits(t), bits(s)), (B, n, "written by a refused call")
    after = _valid_run()
    for (n, x), (_, y) in zip(before, after):
        assert torch.equal(bits(x), bits(y)), (n, "a valid call differs after the refused one")
    del a, watched


def test_dispatch_keeps_the_single_workgroup_call_at_the_limit(monkeypatch):
    """ops.tail_losses at B = 114 (the limit at ec_dim 24) still makes the carel_tail_losses call: the same bits as a direct call."""
    B, V = 114, 257
    assert L.load().carel_tail_batch_limit(24, 6) == B
    cfg, opt, P, x_last, batch, eps_e, eps_c = setup(B, S, V, seed=B + V + 24)
    pin_labels(batch, False)
    args = (P, x_last, batch, eps_e, eps_c, opt, B, S, V, IT, (opt.dropout, SEED, 0))
    buf, G = hip_tail(*args)
    calls = []

    def direct(a):
        calls.append(a.batch)
        L.check(L.load().carel_tail_losses(C.byref(a), L.current_stream()), "carel_tail_losses")
    monkeypatch.setattr(ops, "tail_losses", direct)
    buf1, G1 = hip_tail(*args)
    assert calls == [B]
    for (name, x), (_, y) in zip(outputs(buf, G), outputs(buf1, G1)):
        assert torch.equal(bits(x), bits(y)), (name, "the dispatch changed the bits at the limit")
