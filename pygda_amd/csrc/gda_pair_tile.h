// The streamed all-pairs tile that gda_graphcta.hip and gda_kbl.hip share: a 64x64 block of A B^T on
// v_mfma_f32_32x32x2_f32 (four waves, a 32x32 quarter each), staged through LDS in chunks of DK features as in
// gda_mmd.hip's k_pairdist, and the (value descending, index ascending) order of their running lists.
#ifndef GDA_PAIR_TILE_H
#define GDA_PAIR_TILE_H

#include "gda_common.h"

namespace gda_pair_tile {

constexpr int TB = 256;                       // threads per workgroup (4 waves)
constexpr int TILE = 64;
constexpr int DK = 16;                        // features staged per step
constexpr int LDT = TILE + 1;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct TileLds {
    float As[DK][LDT];
    float Bs[DK][LDT];
};

// four consecutive features k..k+3 of a row (nullptr: a row past the end), zeros past d
__device__ __forceinline__ float4 load4(const float* __restrict__ row, int k, int d, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row == nullptr || k >= d) return v;
    if (vec) return *reinterpret_cast<const float4*>(row + k);
    v.x = row[k];
    if (k + 1 < d) v.y = row[k + 1];
    if (k + 2 < d) v.z = row[k + 2];
    if (k + 3 < d) v.w = row[k + 3];
    return v;
}

// The 64x64 tile A[i0.., :] B[j0.., :]^T.  Element r of the result is row (r % 4) + 8 (r / 4) + 4 (lane / 32) of the
// wave's quarter and column lane % 32 (the C/D layout of the 32x32 MFMA).  Rows past na / nb count as zeros.
__device__ __forceinline__ f32x16 tile_product(const float* __restrict__ A, int64_t na, int64_t i0,
                                               const float* __restrict__ B, int64_t nb, int64_t j0, int d, bool vec,
                                               TileLds& L) {
    const int tid = threadIdx.x, lr = tid >> 2, kq = (tid & 3) * 4;
    const int wave = tid >> 6, lane = tid & 63, la = lane & 31, ka = lane >> 5;
    const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
    const float* pa = i0 + lr < na ? A + (i0 + lr) * d : nullptr;
    const float* pb = j0 + lr < nb ? B + (j0 + lr) * d : nullptr;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < d; k0 += DK) {
        const float4 va = load4(pa, k0 + kq, d, vec), vb = load4(pb, k0 + kq, d, vec);
        __syncthreads();                                   // the previous chunk's MFMAs have read their operands
        L.As[kq + 0][lr] = va.x; L.As[kq + 1][lr] = va.y; L.As[kq + 2][lr] = va.z; L.As[kq + 3][lr] = va.w;
        L.Bs[kq + 0][lr] = vb.x; L.Bs[kq + 1][lr] = vb.y; L.Bs[kq + 2][lr] = vb.z; L.Bs[kq + 3][lr] = vb.w;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L.As[kk + ka][wi + la], L.Bs[kk + ka][wj + la], acc, 0, 0, 0);
    }
    return acc;
}

}  // namespace gda_pair_tile

#endif  // GDA_PAIR_TILE_H
