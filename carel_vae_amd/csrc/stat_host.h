// Host side of the MMD entries (mmd.hip, mmd_perm.hip, stat_tiled.hip): the one place the kernels' MmdCfg is filled from a call.
#pragma once
#include "carel_hip_internal.h"
#include "mmd_device.h"

namespace carel {

// shape, widths and eps; zs: the staged row stride of the kernel launched.  Copies only: the entry has made every check before.
inline void fill_mmd_cfg(MmdCfg* c, const carel_mmd_args* a, int zs) {
  c->n1 = a->n1; c->n2 = a->n2; c->d = a->d; c->zs = zs; c->n_alphas = a->n_alphas;
  for (int i = 0; i < 8; ++i) c->alphas[i] = i < a->n_alphas ? a->alphas[i] : 0.f;
  c->eps = a->eps;
}

}  // namespace carel
