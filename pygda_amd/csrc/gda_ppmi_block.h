// The gathered PPMI block of a mini-batch (batch_ppmi of pygda/models/acdne.py and dmgnn.py), shared by the proximity
// kernels of gda_acdne.hip and gda_dmgnn.hip.
#pragma once
#include <stdint.h>

// Entry (i, j) of the h x h block of one domain's dense PPMI P (leading dimension ld, np nodes) at the batch's PPMI
// indices idx: the diagonal is zero, and an index outside [0, np) reads 0.
__device__ __forceinline__ float ppmi_block_entry(const float* __restrict__ P, int64_t ld, int np,
                                                  const int64_t* __restrict__ idx, int i, int j) {
    const int64_t gi = idx[i], gj = idx[j];
    const bool ok = j != i && gi >= 0 && gi < np && gj >= 0 && gj < np;
    return ok ? P[gi * ld + gj] : 0.f;
}
