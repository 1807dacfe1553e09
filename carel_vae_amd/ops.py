"""Thin torch-tensor wrappers over the C ABI (include/carel_hip.h).  PyTorch is used for device memory
and streams only; every numeric operation happens inside libcarel_hip.so.  No fallbacks."""
import ctypes as C
import math

import torch

from . import _lib as L

H = 768
NH, HD = 12, 64


def _chk_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.CarelError("carel_vae_amd kernels need CUDA/HIP tensors; got a %s tensor. "
                               "There is no CPU fallback in the product path." % t.device)


def gemm(A, B, form, epi, M, N, K, *, splits=1, out_bf16=None, out2_bf16=None, out_f32=None, bias=None,
         resid=None, aux=None, drop=(0, 0, 0, 0.0), lda=None, ldb=None, ldc=None, colsum_part=None, colsum_a=None, splitk_ws=None):
    a = L.GemmArgs()
    a.A, a.B = A.data_ptr(), B.data_ptr()
    a.lda = lda if lda is not None else A.stride(0)
    a.ldb = ldb if ldb is not None else B.stride(0)
    a.ldc = ldc if ldc is not None else N
    a.M, a.N, a.K = M, N, K
    a.form, a.epilogue, a.splits = form, epi, splits
    a.out_bf16 = None if out_bf16 is None else out_bf16.data_ptr()
    a.out2_bf16 = None if out2_bf16 is None else out2_bf16.data_ptr()
    a.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.resid_f32 = None if resid is None else resid.data_ptr()
    a.aux_bf16 = None if aux is None else aux.data_ptr()
    a.drop_seed, a.drop_site, a.drop_idx_offset, a.drop_p = drop
    a.colsum_part = None if colsum_part is None else colsum_part.data_ptr()
    a.colsum_a = None if colsum_a is None else colsum_a.data_ptr()
    a.splitk_ws = None if splitk_ws is None else splitk_ws.data_ptr()
    a.splitk_ws_bytes = 0 if splitk_ws is None else splitk_ws.numel() * splitk_ws.element_size()
    L.check(L.load().carel_gemm_bf16(C.byref(a), L.current_stream()), "carel_gemm_bf16")


# ---- the single-workgroup statistic operators keep both samples in one workgroup's LDS (160 KB); above that the tiled entries take over
SINGLE_LDS_FLOATS = 160 * 1024 // 4
STAT_TILED_MAX_ROWS = 8192


def _largest(fits):
    n = 1
    while fits(n + 1):
        n += 1
    return n


def mmd_single_limit(d):
    """the largest n1 + n2 that carel_rbf_mmd_fwd/bwd accept at feature width d (mmd_prepare of csrc/mmd.hip): 1572 at d = 24"""
    return _largest(lambda n: 64 + ((n + 3) & ~3) + n * (d | 1) <= SINGLE_LDS_FLOATS)


def hsic_single_limit(d):
    """the largest m that carel_hsic_fwd/bwd accept at feature width d (hsic_launch of csrc/hsic.hip): 757 at d = 24"""
    return _largest(lambda m: 64 + 4 * ((m + 3) & ~3) + 2 * m * (d | 1) <= SINGLE_LDS_FLOATS)


def _mmd_goes_tiled(s1, s2):
    """above the single-workgroup limit and inside the tiled one; every other shape keeps the single-workgroup entry and its errors"""
    n, d = s1.shape[0] + s2.shape[0], s1.shape[1]
    return 1 <= d <= 64 and mmd_single_limit(d) < n <= STAT_TILED_MAX_ROWS and s1.shape[0] >= 2 and s2.shape[0] >= 2


def _hsic_goes_tiled(x):
    m, d = x.shape
    return 1 <= d <= 64 and hsic_single_limit(d) < m <= STAT_TILED_MAX_ROWS


def _work(nbytes, device):
    return torch.empty(max(int(nbytes), 8) // 8 + 1, device=device, dtype=torch.float64)


def _perm_outputs(P, nbytes, device):
    """the outputs and the workspace of a permutation test: (stats f64 [P+1], count i32 [1], workspace, its size in bytes)"""
    stats = torch.empty(P + 1, device=device, dtype=torch.float64)
    count = torch.empty(1, device=device, dtype=torch.int32)
    return stats, count, _work(nbytes, device), int(nbytes)


def _chk_sample(x, who):
    _chk_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise L.CarelError("%s: a float32 [m, d] sample with contiguous rows is required" % who)


def rbf_mmd(s1, s2, alphas, eps=1e-5, ret_matrix=False):
    """MMDStatistic.__call__ forward (ref :547-569).  Returns (mmd[1], kernels or None).  Samples that one workgroup's LDS holds go to
    carel_rbf_mmd_fwd, larger ones (n1 + n2 <= 8192) to `rbf_mmd_tiled`, the matrix then from `rbf_gram` (the same expression)."""
    _chk_cuda(s1, s2)
    a = _mmd_args(s1, s2, alphas, eps)
    if _mmd_goes_tiled(s1, s2):
        return rbf_mmd_tiled(s1, s2, alphas, eps), (rbf_gram(s1, s2, alphas, eps) if ret_matrix else None)
    out = torch.empty(1, device=s1.device, dtype=torch.float32)
    n = s1.shape[0] + s2.shape[0]
    kern = torch.empty((n, n), device=s1.device, dtype=torch.float32) if ret_matrix else None
    a.mmd_out = out.data_ptr()
    a.kernels_out = None if kern is None else kern.data_ptr()
    L.check(L.load().carel_rbf_mmd_fwd(C.byref(a), L.current_stream()), "carel_rbf_mmd_fwd")
    return out, kern


def rbf_mmd_backward(s1, s2, alphas, grad, eps=1e-5):
    if _mmd_goes_tiled(s1, s2):
        return rbf_mmd_tiled_backward(s1, s2, alphas, grad, eps)
    a = _mmd_args(s1, s2, alphas, eps)
    g1 = torch.empty((s1.shape[0], s1.shape[1]), device=s1.device, dtype=torch.float32)
    g2 = torch.empty((s2.shape[0], s2.shape[1]), device=s1.device, dtype=torch.float32)
    grad = grad.reshape(1).to(torch.float32).contiguous()
    a.grad_mmd, a.g1, a.g2 = grad.data_ptr(), g1.data_ptr(), g2.data_ptr()
    L.check(L.load().carel_rbf_mmd_bwd(C.byref(a), L.current_stream()), "carel_rbf_mmd_bwd")
    return g1, g2


def rbf_mmd_tiled(s1, s2, alphas, eps=1e-5):
    """carel_rbf_mmd_tiled_fwd: the statistic of `rbf_mmd` summed tile by tile on the whole chip, n1, n2 >= 2, n1 + n2 <= 8192.
    Returns mmd f32 [1] on the device."""
    _chk_cuda(s1, s2)
    a = _mmd_args(s1, s2, alphas, eps)
    lib = L.load()
    out = torch.empty(1, device=s1.device, dtype=torch.float32)
    work = _work(lib.carel_rbf_mmd_tiled_workspace_bytes(a.n1, a.n2, a.d), s1.device)
    a.mmd_out = out.data_ptr()
    L.check(lib.carel_rbf_mmd_tiled_fwd(C.byref(a), work.data_ptr(), L.current_stream()), "carel_rbf_mmd_tiled_fwd")
    return out


def rbf_mmd_tiled_backward(s1, s2, alphas, grad, eps=1e-5):
    """carel_rbf_mmd_tiled_bwd: (g1 [n1, d], g2 [n2, d]) = grad * d mmd / d s; grad None = 1."""
    _chk_cuda(s1, s2)
    a = _mmd_args(s1, s2, alphas, eps)
    lib = L.load()
    g1 = torch.empty((s1.shape[0], s1.shape[1]), device=s1.device, dtype=torch.float32)
    g2 = torch.empty((s2.shape[0], s2.shape[1]), device=s1.device, dtype=torch.float32)
    grad = None if grad is None else grad.reshape(1).to(torch.float32).contiguous()
    work = _work(lib.carel_rbf_mmd_tiled_workspace_bytes(a.n1, a.n2, a.d), s1.device)
    a.grad_mmd, a.g1, a.g2 = None if grad is None else grad.data_ptr(), g1.data_ptr(), g2.data_ptr()
    L.check(lib.carel_rbf_mmd_tiled_bwd(C.byref(a), work.data_ptr(), L.current_stream()), "carel_rbf_mmd_tiled_bwd")
    return g1, g2


def _pdist_args(s1, s2, eps):
    if s1.dtype != torch.float32 or s2.dtype != torch.float32:
        raise L.CarelError("pdist: float32 samples required")
    if s1.stride(1) != 1 or s2.stride(1) != 1 or s1.shape[1] != s2.shape[1]:
        raise L.CarelError("pdist: samples must share the feature width and be contiguous along it")
    a = L.PdistArgs()
    a.s1, a.s2, a.ld1, a.ld2 = s1.data_ptr(), s2.data_ptr(), s1.stride(0), s2.stride(0)
    a.n1, a.n2, a.d, a.eps = s1.shape[0], s2.shape[0], s1.shape[1], eps
    return a


def pdist(s1, s2, eps=1e-5):
    """ref :580-589 (norm = 2): [n1, n2] distances."""
    _chk_cuda(s1, s2)
    a = _pdist_args(s1, s2, eps)
    out = torch.empty((s1.shape[0], s2.shape[0]), device=s1.device, dtype=torch.float32)
    a.dist_out = out.data_ptr()
    L.check(L.load().carel_pdist_fwd(C.byref(a), L.current_stream()), "carel_pdist_fwd")
    return out


def pdist_backward(s1, s2, grad, eps=1e-5):
    a = _pdist_args(s1, s2, eps)
    grad = grad.to(torch.float32).contiguous()
    g1 = torch.empty((s1.shape[0], s1.shape[1]), device=s1.device, dtype=torch.float32)
    g2 = torch.empty((s2.shape[0], s2.shape[1]), device=s1.device, dtype=torch.float32)
    a.grad_dist, a.g1, a.g2 = grad.data_ptr(), g1.data_ptr(), g2.data_ptr()
    L.check(L.load().carel_pdist_bwd(C.byref(a), L.current_stream()), "carel_pdist_bwd")
    return g1, g2


def _mmd_args(s1, s2, alphas, eps):
    if s1.dtype != torch.float32 or s2.dtype != torch.float32:
        raise L.CarelError("rbf_mmd: float32 samples required")
    if s1.stride(1) != 1 or s2.stride(1) != 1 or s1.shape[1] != s2.shape[1]:
        raise L.CarelError("rbf_mmd: samples must share the feature width and be contiguous along it")
    if len(alphas) > 8:
        raise L.CarelError("rbf_mmd: at most 8 alphas (got %d)" % len(alphas))
    a = L.MmdArgs()
    a.s1, a.s2, a.ld1, a.ld2 = s1.data_ptr(), s2.data_ptr(), s1.stride(0), s2.stride(0)
    a.n1, a.n2, a.d, a.n_alphas, a.eps = s1.shape[0], s2.shape[0], s1.shape[1], len(alphas), eps
    for i, v in enumerate(alphas):
        a.alphas[i] = float(v)
    return a


MODEL_MMD_ALPHAS = (0.1,)          # the kernel width of the training loss's MMD term (tail_args: mmd_alpha)


def rbf_gram(s1, s2, alphas, eps=1e-5):
    """carel_rbf_gram: the [n1 + n2, n1 + n2] kernel matrix of two samples, tiled (n1 + n2 <= 8192), bitwise symmetric."""
    _chk_cuda(s1, s2)
    a = _mmd_args(s1, s2, alphas, eps)
    n = s1.shape[0] + s2.shape[0]
    kern = torch.empty((n, n), device=s1.device, dtype=torch.float32)
    a.kernels_out = kern.data_ptr()
    L.check(L.load().carel_rbf_gram(C.byref(a), L.current_stream()), "carel_rbf_gram")
    return kern


def mmd_perm_test(matrix, labels, n1, n2, a00, a01, a11):
    """carel_mmd_perm_test: matrix f32 [n, n] (rows contiguous), labels uint8 [P+1, n] whose row 0 is the observed labelling.
    Returns (stats f64 [P+1], count int32 [1]) on the device; nothing is read back."""
    _chk_cuda(matrix, labels)
    n = int(n1) + int(n2)
    if matrix.dtype != torch.float32 or matrix.dim() != 2 or tuple(matrix.shape) != (n, n) or matrix.stride(1) != 1:
        raise L.CarelError("mmd_perm_test: the matrix must be float32 [n1 + n2, n1 + n2] with contiguous rows")
    if labels.dtype != torch.uint8 or labels.dim() != 2 or labels.shape[1] != n or labels.shape[0] < 2 or not labels.is_contiguous():
        raise L.CarelError("mmd_perm_test: labels must be contiguous uint8 [n_permutations + 1, n1 + n2]")
    if labels.device != matrix.device:
        raise L.CarelError("mmd_perm_test: the matrix and the labels are on different devices")
    P = labels.shape[0] - 1
    lib = L.load()
    a = L.MmdPermArgs()
    a.matrix, a.ldm, a.labels = matrix.data_ptr(), matrix.stride(0), labels.data_ptr()
    a.n1, a.n2, a.n_permutations = int(n1), int(n2), P
    a.a00, a.a01, a.a11 = float(a00), float(a01), float(a11)
    stats, count, work, nbytes = _perm_outputs(P, lib.carel_mmd_perm_workspace_bytes(n, P), matrix.device)
    a.stats, a.count, a.workspace, a.workspace_bytes = stats.data_ptr(), count.data_ptr(), work.data_ptr(), nbytes
    L.check(lib.carel_mmd_perm_test(C.byref(a), L.current_stream()), "carel_mmd_perm_test")
    return stats, count


def sample_latents(lat, eps_e, eps_c, D):
    """carel_sample_latents: z f32 [N, 2 D] = [mu_e + eps_e e^lv_e | mu_c + eps_c e^lv_c] of lat f32 [N, 4 D] with one noise pair [D]."""
    _chk_cuda(lat, eps_e, eps_c)
    if lat.dtype != torch.float32 or lat.dim() != 2 or lat.shape[1] != 4 * D or not lat.is_contiguous() or lat.shape[0] < 1:
        raise L.CarelError("sample_latents: lat must be contiguous float32 [N, 4 * ec_dim]")
    if any(e.dtype != torch.float32 or e.numel() != D or not e.is_contiguous() for e in (eps_e, eps_c)):
        raise L.CarelError("sample_latents: eps_e and eps_c must be contiguous float32 [ec_dim]")
    z = torch.empty((lat.shape[0], 2 * D), device=lat.device, dtype=torch.float32)
    L.check(L.load().carel_sample_latents(lat.data_ptr(), eps_e.data_ptr(), eps_c.data_ptr(), lat.shape[0], D, z.data_ptr(), L.current_stream()),
            "carel_sample_latents")
    return z


def kl_anneal_weight(iteration, opt):
    """ref :515-523 (host double arithmetic) gated by :242/:248."""
    if iteration < opt.kl_ann_iterations:
        return (math.tanh((iteration - opt.kl_ann_iterations * 1.5) / (opt.kl_ann_iterations / 3)) + 1) * opt.ec_kl_lambda
    return 1.0


DISENTANGLE_MODES = ("mmd", "hsic", "none", "vi", "gan")


class TailBuffers:
    """Outputs + workspace of the tail calls for one (batch, ec_dim, bow_dim) shape."""

    def __init__(self, B, S, D, EC, V, device, rows=None):
        f = dict(device=device, dtype=torch.float32)
        self.B, self.S, self.D, self.EC, self.V = B, S, D, EC, V
        self.rows = rows if rows is not None else B * S        # rows of the encoder's last hidden state / its gradient
        self.pooled = torch.empty((B, H), **f)
        self.lat = torch.empty((B, 4 * D), **f)
        # z sits at the head of a buffer with 16 spare floats: a data-parallel caller all-gathers the whole thing (z + its
        # label sum in [n]) in ONE collective without packing anything (carel_vae_amd.dp.DataParallel.fill_global)
        self.zpack = torch.zeros(B * 2 * D + 16, **f)
        self.z = self.zpack[:B * 2 * D].view(B, 2 * D)
        self.terms = torch.zeros(16, **f)
        self.work = torch.empty(L.load().carel_tail_workspace_floats(B, D, V), **f)
        self.dx_last = torch.empty((self.rows, H), **f)


def tail_args(buf: TailBuffers, x_last, W, labels, eps_e, eps_c, opt, kl_weight, *, grads=None, drop=(0.0, 0, 0),
              global_label_sum=None, global_n=0, global_row_offset=0, z_global=None, mmd_grad_scale=1.0, global_rank_stride=0, global_label_ranks=0, cls_rows=None,
              n_rows=0, head_in=None, d_head_in=None):
    """W / grads: dicts keyed by the reference's state_dict names (tail part).  head_in / d_head_in: f32 [2, B, 768] adapter outputs and
    their gradient (AdapterBuffers.out / .d_out): the latent heads read them instead of the pooler."""
    a = L.TailArgs()
    a.batch, a.seq_len, a.hidden, a.ec_dim, a.e_classes, a.bow_dim = buf.B, buf.S, H, buf.D, buf.EC, buf.V
    a.x_last_f32 = x_last.data_ptr()
    a.pooler_w, a.pooler_b = W["encoder.pooler.dense.weight"].data_ptr(), W["encoder.pooler.dense.bias"].data_ptr()
    heads = ("emotion_mu", "emotion_log_var", "cause_mu", "cause_log_var")
    for i, n in enumerate(heads):
        a.head_w[i] = W[n + ".weight"].data_ptr()
        a.head_b[i] = W[n + ".bias"].data_ptr()
    a.emo_w, a.emo_b = W["emotion_classifier.weight"].data_ptr(), W["emotion_classifier.bias"].data_ptr()
    a.cau_w, a.cau_b = W["cause_classifier.weight"].data_ptr(), W["cause_classifier.bias"].data_ptr()
    a.pair_w, a.pair_b = W["pair_classifier.weight"].data_ptr(), W["pair_classifier.bias"].data_ptr()
    a.dec_w, a.dec_b = W["decoder.weight"].data_ptr(), W["decoder.bias"].data_ptr()
    if labels is not None:
        a.emo_labels, a.cau_labels = labels["emo"].data_ptr(), labels["cau"].data_ptr()
        a.pair_labels, a.bow = labels["pair"].data_ptr(), labels["bow"].data_ptr()
    a.eps_e = None if eps_e is None else eps_e.data_ptr()
    a.eps_c = None if eps_c is None else eps_c.data_ptr()
    if getattr(opt, "disentangle", "mmd") == "gan":      # drl_classifier_ec_gan.py:275-279: no statistic, one weight for both one-logit heads
        a.w_mmd, a.w_emo, a.w_cau, a.w_pair = 0.0, opt.ec_mul_loss_weight, opt.ec_mul_loss_weight, opt.pair_mul_loss_weight
    else:
        a.w_mmd, a.w_emo, a.w_cau, a.w_pair = (opt.mmd_loss_weight, opt.emo_mul_loss_weight, opt.cau_mul_loss_weight,
                                                opt.pair_mul_loss_weight)
    a.kl_weight, a.label_smoothing = kl_weight, opt.label_smoothing
    a.drop_p, a.drop_seed, a.drop_row_offset = drop
    a.mmd_alpha, a.mmd_eps = 0.1, 1e-5
    mode = getattr(opt, "disentangle", "mmd")
    if mode not in DISENTANGLE_MODES:
        raise L.CarelError("opt.disentangle must be 'mmd', 'hsic', 'vi', 'gan' or 'none'")
    # vi: the CLUB term is added outside the tail (vi_upper); gan: the adversaries run beside it (gan_disc)
    a.dis_mode = {"mmd": 0, "hsic": 1, "none": 2, "vi": 2, "gan": 2}[mode]
    if mode == "hsic":
        a.w_mmd = getattr(opt, "hsic_loss_weight", 1.0)      # the HSIC script adds the statistic unweighted
    a.emo_bce = int(getattr(opt, "emotion_head", "ce") == "bce")
    if mode == "gan" and not a.emo_bce:
        raise L.CarelError("opt.disentangle == 'gan' needs opt.emotion_head == 'bce' (one-logit heads, drl_classifier_ec_gan.py:496-526)")
    a.global_label_sum = None if global_label_sum is None else global_label_sum.data_ptr()
    a.global_n, a.global_row_offset = global_n, global_row_offset
    a.z_global = None if z_global is None else z_global.data_ptr()
    a.mmd_grad_scale = mmd_grad_scale
    a.global_rank_stride = global_rank_stride
    a.global_label_ranks = global_label_ranks
    a.pooled, a.lat, a.z, a.terms, a.work = (buf.pooled.data_ptr(), buf.lat.data_ptr(), buf.z.data_ptr(),
                                             buf.terms.data_ptr(), buf.work.data_ptr())
    a.dx_last_f32 = buf.dx_last.data_ptr()
    a.cls_rows = None if cls_rows is None else cls_rows.data_ptr()
    a.n_rows = n_rows if n_rows else buf.rows
    a.head_in_f32 = None if head_in is None else head_in.data_ptr()
    a.d_head_in_f32 = None if d_head_in is None else d_head_in.data_ptr()
    if grads is not None:
        a.d_emo_w, a.d_emo_b = grads["emotion_classifier.weight"].data_ptr(), grads["emotion_classifier.bias"].data_ptr()
        a.d_cau_w, a.d_cau_b = grads["cause_classifier.weight"].data_ptr(), grads["cause_classifier.bias"].data_ptr()
        a.d_pair_w, a.d_pair_b = grads["pair_classifier.weight"].data_ptr(), grads["pair_classifier.bias"].data_ptr()
        a.d_dec_w, a.d_dec_b = grads["decoder.weight"].data_ptr(), grads["decoder.bias"].data_ptr()
        for i, n in enumerate(heads):
            a.d_head_w[i] = grads[n + ".weight"].data_ptr() if (n + ".weight") in grads else None
            a.d_head_b[i] = grads[n + ".bias"].data_ptr() if (n + ".bias") in grads else None
        a.d_pooler_w = grads["encoder.pooler.dense.weight"].data_ptr()
        a.d_pooler_b = grads["encoder.pooler.dense.bias"].data_ptr()
    return a


def tail_latents(a):
    L.check(L.load().carel_tail_latents(C.byref(a), L.current_stream()), "carel_tail_latents")


def tail_batch_limit(ec_dim, e_classes):
    """The largest batch carel_tail_losses (the single-workgroup form) accepts; above it tail_losses takes the batch-tiled form."""
    return int(L.load().carel_tail_batch_limit(int(ec_dim), int(e_classes)))


def tail_losses_tiled(a):
    """carel_tail_losses_tiled: the batch-tiled loss step, 2 <= batch <= 1024 (MMD or no statistic)."""
    L.check(L.load().carel_tail_losses_tiled(C.byref(a), L.current_stream()), "carel_tail_losses_tiled")


def tail_losses(a):
    """The loss step: carel_tail_losses up to its batch limit (unchanged kernels, launches and bits), the batch-tiled form above it."""
    if a.batch <= tail_batch_limit(a.ec_dim, a.e_classes):
        L.check(L.load().carel_tail_losses(C.byref(a), L.current_stream()), "carel_tail_losses")
    else:
        tail_losses_tiled(a)


def tail_backward(a, grad_out=None, dz_extra=None):
    """grad_out: device f32 scalar tensor (upstream gradient of the loss) or None for 1.
    dz_extra: optional f32 [B, 2*ec_dim] additional gradient on the sampled embeddings (not scaled by grad_out)."""
    if dz_extra is not None:
        _chk_cuda(dz_extra)
        if dz_extra.dtype != torch.float32 or not dz_extra.is_contiguous() or dz_extra.numel() != a.batch * 2 * a.ec_dim:
            raise L.CarelError("dz_extra must be a contiguous f32 [batch, 2*ec_dim] tensor")
    L.check(L.load().carel_tail_backward_dz(C.byref(a), None if grad_out is None else grad_out.data_ptr(),
                                            None if dz_extra is None else dz_extra.data_ptr(), L.current_stream()),
            "carel_tail_backward_dz")


ADAPTER_MODES = {"raw": 0, "sparsemax": 1, "entmax": 2}


class AdapterBuffers:
    """Outputs + workspace of the sentence-adapter calls for one (batch, seq_len) shape: out / d_out f32 [2, B, 768] (emotion, cause)."""

    def __init__(self, B, S, heads, device):
        f = dict(device=device, dtype=torch.float32)
        self.B, self.S, self.heads = B, S, heads
        self.out = torch.empty((2, B, H), **f)
        self.d_out = torch.empty((2, B, H), **f)
        self.work = torch.empty(L.load().carel_adapter_workspace_floats(B, S, heads), **f)
        self.wgrad_work = None           # carel_adapter_backward_weights' own scratch (opt.train_adapter): allocated by adapter_wgrad_args


def adapter_args(mode, heads, queries, weights, u, buf, Bp, x=None, dx=None):
    """mode: "raw" / "sparsemax" / "entmax"; queries: two f32 [768] device tensors (emotion, cause); weights: two dicts with q_w, q_b,
    k_w and (raw) v_w, v_b, o_w, o_b (contiguous f32); u: f32 [2, heads, 768]; buf: AdapterBuffers; x / dx: f32 [Bp*S, 768] (tensor or
    anything with data_ptr())."""
    a = L.AdapterArgs()
    a.batch, a.batch_padded, a.seq_len, a.mode, a.heads = buf.B, Bp, buf.S, ADAPTER_MODES[mode], heads
    for i in range(2):
        a.query[i] = queries[i].data_ptr()
        for f in ("q_w", "q_b", "k_w", "v_w", "v_b", "o_w", "o_b"):
            t = weights[i].get(f)
            getattr(a, f)[i] = None if t is None else t.data_ptr()
    a.u, a.work, a.out_f32, a.d_out_f32 = u.data_ptr(), buf.work.data_ptr(), buf.out.data_ptr(), buf.d_out.data_ptr()
    a.x_f32 = None if x is None else x.data_ptr()
    a.dx_f32 = None if dx is None else dx.data_ptr()
    a._keep = (queries, weights)
    return a


def adapter_build_u(a):
    L.check(L.load().carel_adapter_build_u(C.byref(a), L.current_stream()), "carel_adapter_build_u")


def adapter_forward(a):
    L.check(L.load().carel_adapter_forward(C.byref(a), L.current_stream()), "carel_adapter_forward")


def adapter_backward(a):
    L.check(L.load().carel_adapter_backward(C.byref(a), L.current_stream()), "carel_adapter_backward")


def adapter_wgrad_args(buf, grads, accumulate=False):
    """grads: two dicts (emotion, cause) of contiguous f32 destinations keyed like adapter_args' weights with a d_ prefix: d_q_w, d_q_b,
    d_k_w, d_k_b [768, 768] / [768] and (raw) d_v_w, d_v_b, d_o_w, d_o_b; buf: the AdapterBuffers of the forward / backward calls (its
    own scratch for this call is allocated on first use); accumulate: add to the destinations instead of overwriting them."""
    g = L.AdapterWgradArgs()
    for i in range(2):
        for f in ("d_q_w", "d_q_b", "d_k_w", "d_k_b", "d_v_w", "d_v_b", "d_o_w", "d_o_b"):
            t = grads[i].get(f)
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != buf.out.device):
                raise L.CarelError("adapter gradient destination %s must be a contiguous f32 tensor on the adapter's device" % f)
            getattr(g, f)[i] = None if t is None else t.data_ptr()
    if buf.wgrad_work is None:
        buf.wgrad_work = torch.empty(L.load().carel_adapter_wgrad_workspace_floats(buf.B, buf.heads), device=buf.out.device, dtype=torch.float32)
    g.work, g.accumulate = buf.wgrad_work.data_ptr(), int(bool(accumulate))
    g._keep = (grads, buf.wgrad_work)
    return g


def adapter_backward_weights(a, g):
    """Adapter weight gradients; after adapter_forward(a) and adapter_backward(a), whose workspace regions it reads."""
    L.check(L.load().carel_adapter_backward_weights(C.byref(a), C.byref(g), L.current_stream()), "carel_adapter_backward_weights")


def en_bow_workspace(batch, con_dim, bow_dim, device):
    """Scratch of carel_en_tail_losses_bow: the site-120 copy of the content sample [B, con_dim], then the weight matrix [B, V]."""
    return torch.empty(L.load().carel_en_tail_bow_workspace_floats(batch, con_dim, bow_dim), device=device, dtype=torch.float32)


def en_bow_args(work):
    """carel_en_bow_args around a scratch tensor from en_bow_workspace (kept alive by the returned struct)."""
    _chk_cuda(work)
    if work.dtype != torch.float32 or not work.is_contiguous():
        raise L.CarelError("the weight scratch must be a contiguous f32 tensor")
    b = L.EnBowArgs()
    b.work = work.data_ptr()
    b._keep = work
    return b


def en_tail_losses_bow(a, b):
    """carel_en_tail_losses with the element-weighted content losses of drl_classifier_bow_loss.py; a: EnTailArgs, b: en_bow_args(...)."""
    L.check(L.load().carel_en_tail_losses_bow(C.byref(a), C.byref(b), L.current_stream()), "carel_en_tail_losses_bow")


def _vi_args(z, net):
    _chk_cuda(z, *net)
    if z.dtype != torch.float32 or not z.is_contiguous() or z.dim() != 2 or z.shape[1] % 2:
        raise L.CarelError("z must be a contiguous f32 [batch, 2*ec_dim] tensor")
    D = z.shape[1] // 2
    shapes = [(D, D), (D,), (D, D), (D,)] * 2
    if len(net) != 8 or any(tuple(w.shape) != sh or w.dtype != torch.float32 or not w.is_contiguous() for w, sh in zip(net, shapes)):
        raise L.CarelError("the approximation network is 8 contiguous f32 tensors: (w1 [D,D], b1 [D], w2 [D,D], b2 [D]) x (mu, log_var)")
    a = L.ViArgs()
    a.z, a.batch, a.ec_dim = z.data_ptr(), z.shape[0], D
    for i, w in enumerate(net):
        a.net[i] = w.data_ptr()
    return a


def vi_aprx(z, net):
    """-> (loss [1], [8 gradients of the approximation network]); drl_classifier_ec_vi.py:422-427."""
    a = _vi_args(z, net)
    loss = torch.empty(1, device=z.device, dtype=torch.float32)
    grads = [torch.empty_like(w) for w in net]
    a.loss_out = loss.data_ptr()
    for i, g in enumerate(grads):
        a.d_net[i] = g.data_ptr()
    L.check(L.load().carel_vi_aprx(C.byref(a), L.current_stream()), "carel_vi_aprx")
    return loss, grads


def vi_upper(z, net, perm):
    """-> (CLUB upper bound [1], d bound / d z [B, 2D]); drl_classifier_ec_vi.py:429-440; perm: int32 [B] device tensor."""
    a = _vi_args(z, net)
    _chk_cuda(perm)
    if perm.dtype != torch.int32 or perm.numel() != z.shape[0]:
        raise L.CarelError("perm must be an int32 [batch] tensor")
    loss = torch.empty(1, device=z.device, dtype=torch.float32)
    dz = torch.empty_like(z)
    a.perm, a.loss_out, a.dz = perm.data_ptr(), loss.data_ptr(), dz.data_ptr()
    L.check(L.load().carel_vi_upper(C.byref(a), L.current_stream()), "carel_vi_upper")
    return loss, dz


GAN_TERM_NAMES = ("ec_disc_loss", "ce_disc_loss", "ec_entropy", "ce_entropy")


def gan_disc(z, emo_labels, cau_labels, disc_w, disc_b, opt, terms, g_loss_w, g_loss_b, g_ent_w, g_ent_b, *, drop=(0.0, 0, 0), vae_loss_in=None):
    """carel_gan_disc: the two adversaries of drl_classifier_ec_gan.py on the sampled embeddings z f32 [B, 2*ec_dim].
    disc_w / disc_b and the four g_* : pairs (ec_disc, ce_disc) of f32 device tensors ([ec_dim] weights, [1] biases); terms: f32 [8]
    -> GAN_TERM_NAMES in [0..3] and, with vae_loss_in (f32 [1]), the vae loss plus the weighted entropies in [4]."""
    ts = [z, emo_labels, cau_labels, terms, *disc_w, *disc_b, *g_loss_w, *g_loss_b, *g_ent_w, *g_ent_b]
    _chk_cuda(*ts, vae_loss_in)
    if any(t.dtype != torch.float32 for t in ts) or z.dim() != 2 or z.shape[1] % 2 or not z.is_contiguous():
        raise L.CarelError("gan_disc: float32 tensors and a contiguous z [batch, 2*ec_dim] are required")
    B, D = z.shape[0], z.shape[1] // 2
    if emo_labels.numel() != B or cau_labels.numel() != B or not emo_labels.is_contiguous() or not cau_labels.is_contiguous():
        raise L.CarelError("gan_disc: the emotion / cause labels are contiguous f32 [batch] tensors")
    if terms.numel() < 8 or any(w.numel() != D for w in (*disc_w, *g_loss_w, *g_ent_w)) or any(b.numel() != 1 for b in (*disc_b, *g_loss_b, *g_ent_b)):
        raise L.CarelError("gan_disc: terms holds 8 floats, weights and their images ec_dim, biases and their images 1")
    a = L.GanArgs()
    a.z, a.batch, a.ec_dim = z.data_ptr(), B, D
    a.emo_labels, a.cau_labels = emo_labels.data_ptr(), cau_labels.data_ptr()
    for i in range(2):
        a.disc_w[i], a.disc_b[i] = disc_w[i].data_ptr(), disc_b[i].data_ptr()
        a.g_loss_w[i], a.g_loss_b[i] = g_loss_w[i].data_ptr(), g_loss_b[i].data_ptr()
        a.g_ent_w[i], a.g_ent_b[i] = g_ent_w[i].data_ptr(), g_ent_b[i].data_ptr()
    a.label_smoothing, a.epsilon = opt.label_smoothing, opt.epsilon
    a.drop_p, a.drop_seed, a.drop_row_offset = drop
    a.vae_loss_in = None if vae_loss_in is None else vae_loss_in.data_ptr()
    a.w_entropy = getattr(opt, "ecce_adv_loss_weight", 1.0)
    a.terms = terms.data_ptr()
    L.check(L.load().carel_gan_disc(C.byref(a), L.current_stream()), "carel_gan_disc")


def axpy_(dst, src, scale_dev, accumulate):
    """dst = (accumulate ? dst : 0) + *scale_dev * src (carel_axpy_f32; scale_dev: device f32 [1])."""
    L.check(L.load().carel_axpy_f32(dst.data_ptr(), src.data_ptr(), dst.numel(), scale_dev.data_ptr(), int(accumulate), L.current_stream()),
            "carel_axpy_f32")


def bow_expand(trip, nnz, out):
    """trip: device int32 [3 * nnz] (rows, cols, f32 value bits); out: device f32 [B, V] (overwritten)."""
    L.check(L.load().carel_bow_expand(trip.data_ptr() if nnz else None, int(nnz), out.data_ptr(), out.shape[0], out.shape[1], L.current_stream()),
            "carel_bow_expand")
    return out


def pair_probs(lat, eps_e, eps_c, pair_w, pair_b, D):
    B = lat.shape[0]
    prob = torch.empty(B, device=lat.device, dtype=torch.float32)
    L.check(L.load().carel_pair_probs(lat.data_ptr(), eps_e.data_ptr(), eps_c.data_ptr(), pair_w.data_ptr(),
                                      pair_b.data_ptr(), B, D, prob.data_ptr(), L.current_stream()), "carel_pair_probs")
    return prob


PAIR_DRAWS_MAX_GROUPS = 8


def pair_probs_draws(lat, eps_e, eps_c, pair_w, pair_b, D, labels=None, groups=None, n_groups=1, want_prob=True, counts_out=None):
    """carel_pair_probs_draws: K = eps_e.shape[0] noise draws over the same latents.  Returns (prob [K, N] f32 or None,
    counts [K, n_groups, 3] int32 = TP / FP / FN or None -- counted when `labels` is given).  labels: f32 [N]; groups: int32 [N]
    whose ids the CALLER has checked to be in [0, n_groups) (a row outside is counted nowhere)."""
    _chk_cuda(lat, eps_e, eps_c)
    N, K = lat.shape[0], eps_e.shape[0]
    if (eps_e.dtype != torch.float32 or eps_c.dtype != torch.float32 or tuple(eps_e.shape) != (K, D) or tuple(eps_c.shape) != (K, D)
            or not eps_e.is_contiguous() or not eps_c.is_contiguous()):
        raise L.CarelError("pair_probs_draws: eps_e and eps_c must be contiguous float32 [n_draws, ec_dim]")
    if lat.dtype != torch.float32 or lat.dim() != 2 or lat.shape[1] != 4 * D or not lat.is_contiguous():
        raise L.CarelError("pair_probs_draws: lat must be contiguous float32 [N, 4 * ec_dim]")
    prob = torch.empty((K, N), device=lat.device, dtype=torch.float32) if want_prob else None
    counts = None
    if labels is not None:
        _chk_cuda(labels)
        if labels.dtype != torch.float32 or labels.numel() != N or not labels.is_contiguous():
            raise L.CarelError("pair_probs_draws: labels must be contiguous float32 [N]")
        if groups is not None:
            _chk_cuda(groups)
            if groups.dtype != torch.int32 or groups.numel() != N or not groups.is_contiguous():
                raise L.CarelError("pair_probs_draws: groups must be contiguous int32 [N]")
        counts = counts_out if counts_out is not None else torch.empty((K, n_groups, 3), device=lat.device, dtype=torch.int32)
        if counts.dtype != torch.int32 or counts.numel() != K * n_groups * 3 or not counts.is_contiguous() or not counts.is_cuda:
            raise L.CarelError("pair_probs_draws: counts must be a contiguous int32 [n_draws, n_groups, 3] device tensor")
    L.check(L.load().carel_pair_probs_draws(lat.data_ptr(), eps_e.data_ptr(), eps_c.data_ptr(), pair_w.data_ptr(), pair_b.data_ptr(), N, D, K,
                                            None if prob is None else prob.data_ptr(), None if labels is None else labels.data_ptr(),
                                            None if groups is None else groups.data_ptr(), int(n_groups),
                                            None if counts is None else counts.data_ptr(), L.current_stream()), "carel_pair_probs_draws")
    return prob, counts


def _hsic_args(x, y, s_x, s_y):
    _chk_cuda(x, y)
    if x.shape != y.shape or x.dtype != torch.float32 or y.dtype != torch.float32 or x.stride(1) != 1 or y.stride(1) != 1:
        raise L.CarelError("hsic: two float32 [m, d] samples of equal shape, contiguous rows")
    a = L.HsicArgs()
    a.x, a.y, a.ldx, a.ldy, a.m, a.d, a.s_x, a.s_y = x.data_ptr(), y.data_ptr(), x.stride(0), y.stride(0), x.shape[0], x.shape[1], s_x, s_y
    return a


def hsic(x, y, s_x=1.0, s_y=1.0):
    """carel_hsic_fwd while one workgroup's LDS holds both samples (m <= 757 at d = 24), `hsic_tiled` above (m <= 8192)."""
    a = _hsic_args(x, y, s_x, s_y)
    if _hsic_goes_tiled(x):
        return hsic_tiled(x, y, s_x, s_y)
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    a.hsic_out = out.data_ptr()
    L.check(L.load().carel_hsic_fwd(C.byref(a), L.current_stream()), "carel_hsic_fwd")
    return out


def hsic_tiled(x, y, s_x=1.0, s_y=1.0):
    """carel_hsic_tiled_fwd: the statistic of `hsic` summed tile by tile on the whole chip, 2 <= m <= 8192.  Returns f32 [1]."""
    a = _hsic_args(x, y, s_x, s_y)
    lib = L.load()
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    work = _work(lib.carel_hsic_tiled_workspace_bytes(a.m, a.d), x.device)
    a.hsic_out = out.data_ptr()
    L.check(lib.carel_hsic_tiled_fwd(C.byref(a), work.data_ptr(), L.current_stream()), "carel_hsic_tiled_fwd")
    return out


def hsic_tiled_backward(x, y, grad, s_x=1.0, s_y=1.0):
    """carel_hsic_tiled_bwd: (gx, gy) [m, d] = grad * d hsic / d (x, y); grad None = 1."""
    a = _hsic_args(x, y, s_x, s_y)
    lib = L.load()
    gx, gy = torch.empty(x.shape, device=x.device, dtype=torch.float32), torch.empty(y.shape, device=x.device, dtype=torch.float32)
    grad = None if grad is None else grad.reshape(1).to(torch.float32).contiguous()
    work = _work(lib.carel_hsic_tiled_workspace_bytes(a.m, a.d), x.device)
    a.grad_hsic, a.gx, a.gy = None if grad is None else grad.data_ptr(), gx.data_ptr(), gy.data_ptr()
    L.check(lib.carel_hsic_tiled_bwd(C.byref(a), work.data_ptr(), L.current_stream()), "carel_hsic_tiled_bwd")
    return gx, gy


def hsic_gram(x, s=1.0):
    """carel_hsic_gram: K = exp(-D(x) / s) f32 [m, m] of the rows of x f32 [m, d], tiled (2 <= m <= 8192, d <= 64): the kernel matrix
    of `hsic`, element by element the same expression, bitwise symmetric, diagonal exactly 1."""
    _chk_sample(x, "hsic_gram")
    m = x.shape[0]
    out = torch.empty((m, m), device=x.device, dtype=torch.float32)
    a = L.HsicGramArgs()
    a.x, a.ldx, a.m, a.d, a.s, a.k_out, a.ldk = x.data_ptr(), x.stride(0), m, x.shape[1], float(s), out.data_ptr(), m
    L.check(L.load().carel_hsic_gram(C.byref(a), L.current_stream()), "carel_hsic_gram")
    return out


def hsic_perm_test(K, Lm, perms):
    """carel_hsic_perm_test: K, Lm f32 [m, m] (rows contiguous), perms int32 [P+1, m] whose row 0 is the observed pairing (the
    identity).  Returns (stats f64 [P+1], count int32 [1]) on the device; nothing is read back."""
    _chk_cuda(K, Lm, perms)
    m = K.shape[0] if K.dim() == 2 else -1
    if any(t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (m, m) or t.stride(1) != 1 for t in (K, Lm)):
        raise L.CarelError("hsic_perm_test: K and L must be float32 [m, m] with contiguous rows")
    if perms.dtype != torch.int32 or perms.dim() != 2 or perms.shape[1] != m or perms.shape[0] < 2 or not perms.is_contiguous():
        raise L.CarelError("hsic_perm_test: perms must be contiguous int32 [n_permutations + 1, m]")
    if Lm.device != K.device or perms.device != K.device:
        raise L.CarelError("hsic_perm_test: the matrices and the permutations are on different devices")
    P = perms.shape[0] - 1
    lib = L.load()
    a = L.HsicPermArgs()
    a.k, a.ldk, a.l, a.ldl, a.perms = K.data_ptr(), K.stride(0), Lm.data_ptr(), Lm.stride(0), perms.data_ptr()
    a.m, a.n_permutations = m, P
    stats, count, work, nbytes = _perm_outputs(P, lib.carel_hsic_perm_workspace_bytes(m, P), K.device)
    a.stats, a.count, a.workspace, a.workspace_bytes = stats.data_ptr(), count.data_ptr(), work.data_ptr(), nbytes
    L.check(lib.carel_hsic_perm_test(C.byref(a), L.current_stream()), "carel_hsic_perm_test")
    return stats, count


def pdist_select(x, ranks):
    """carel_pdist_select: the exact order statistics of { D_ij : i < j }, D the squared distances `hsic_gram` exponentiates (bit for
    bit), of the rows of x f32 [m, d] (2 <= m <= 8192, d <= 64), without the matrix.  ranks: up to 8 host integers in
    [0, m (m-1) / 2), 0-based.  Returns (values f32 [n], counts int64 [n, 2] = #{D < v}, #{D == v}) on the device; nothing is read
    back."""
    _chk_sample(x, "pdist_select")
    ranks = [int(r) for r in ranks]
    n = len(ranks)
    if not 1 <= n <= L.PDIST_SELECT_MAX_RANKS:
        raise L.CarelError("pdist_select: 1 to %d ranks are required (got %d)" % (L.PDIST_SELECT_MAX_RANKS, n))
    m = x.shape[0]
    lib = L.load()
    a = L.PdistSelectArgs()
    a.x, a.ldx, a.m, a.d, a.n_ranks = x.data_ptr(), x.stride(0), m, x.shape[1], n
    for q, r in enumerate(ranks):
        a.ranks[q] = r
    values = torch.empty(n, device=x.device, dtype=torch.float32)
    counts = torch.empty((n, 2), device=x.device, dtype=torch.int64)
    nbytes = int(lib.carel_pdist_select_workspace_bytes(m, n))
    work = _work(nbytes, x.device)
    a.values, a.counts, a.workspace, a.workspace_bytes = values.data_ptr(), counts.data_ptr(), work.data_ptr(), nbytes
    L.check(lib.carel_pdist_select(C.byref(a), L.current_stream()), "carel_pdist_select")
    return values, counts


def hsic_backward(x, y, grad, s_x=1.0, s_y=1.0):
    if x.dim() == 2 and _hsic_goes_tiled(x):
        return hsic_tiled_backward(x, y, grad, s_x, s_y)
    a = _hsic_args(x, y, s_x, s_y)
    gx, gy = torch.empty(x.shape, device=x.device, dtype=torch.float32), torch.empty(y.shape, device=x.device, dtype=torch.float32)
    grad = grad.reshape(1).to(torch.float32).contiguous()
    a.grad_hsic, a.gx, a.gy = grad.data_ptr(), gx.data_ptr(), gy.data_ptr()
    L.check(L.load().carel_hsic_bwd(C.byref(a), L.current_stream()), "carel_hsic_bwd")
    return gx, gy
