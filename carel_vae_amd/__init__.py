"""carel_vae_amd -- MI355X (gfx950) implementation of the CAREL-VAE training hot path.

The Python host code mirrors the module surface of the reference's drl_classifier_ec_mmd_final_mul.py
(`ECPEDataset`, `DrlClassifier`, `MMDStatistic`, `pdist`, `read_ECPE_data`, `train`, `save_ckp`, `load_ckp`,
`generate_self_train_data`); every numeric operation of the step is a HIP kernel in libcarel_hip.so behind the
C ABI of include/carel_hip.h.  There is no CPU / eager fallback.
`carel_vae_amd.drl_classifier_en` is the same for the reference's drl_classifier_en.py (config 4).
"""
from . import _lib  # noqa: F401
from .data import BatchLoader, PrefetchLoader, ECPEDataset, get_bow_en, get_bow_zh, newsplit_paths, read_ECPE_data  # noqa: F401
from .drl_classifier import (HSIC, DrlClassifier, FusedAdam, FusedRMSprop, MMDStatistic, encoder_config, hsic_independence_test,  # noqa: F401
                             hsic_permutation_test, make_gan_opt, make_newsplit_opt, make_opt, median_alphas, median_heuristic,
                             mmd_two_sample_test, pdist, pdist_quantile, permutation_test_mat, random_labellings, random_permutations)
from . import drl_classifier_en  # noqa: F401   the three-space adversarial model of drl_classifier_en.py (same class name: DrlClassifier)
from .training import generate_self_train_data, load_ckp, prf_from_counts, save_ckp, train  # noqa: F401

__all__ = ["ECPEDataset", "BatchLoader", "PrefetchLoader", "DrlClassifier", "MMDStatistic", "pdist", "HSIC", "permutation_test_mat", "mmd_two_sample_test", "random_labellings", "hsic_permutation_test", "hsic_independence_test", "random_permutations", "pdist_quantile", "median_heuristic", "median_alphas", "read_ECPE_data", "train",
           "generate_self_train_data", "save_ckp", "load_ckp", "get_bow_zh", "get_bow_en", "FusedAdam", "FusedRMSprop", "make_opt", "make_gan_opt",
           "encoder_config", "make_newsplit_opt", "newsplit_paths", "prf_from_counts"]
