// What the wave tiles of the MX cross-term GEMM share (gemm256x.hip: the 8-wave and the one-wave-per-SIMD 256 x 256 tiles; gemm128x.hip: the
// 128 x 128 tile): the LDS-DMA request and the XCD tile order; the ONE epilogue behind every main loop is gemm_mx_epilogue.h.
// Included by those two files only.  The main loops, the ring geometry (TM, TN, STAGE), the kernels and their launch bounds stay with each file:
// they are different schedules.  Row formats, fragment maps and the arithmetic order: gemm256x.hip's header.
// (The fragment-offset block and the ld32 lambda are repeated in each main loop on purpose: as shared functions they change the kernels'
//  instruction order — profiles/mx_epilogue/kernel_resources.txt.)
#pragma once
#include "glc_common.h"
#include "glc_kernels.h"
#include "glc_layout.h"

namespace {

constexpr int LINE = 128;                  // bytes per row and group
constexpr int NSLOT = 4;                   // ring stages: stage 2 s = A rows of group s, 2 s + 1 = W rows; slot = stage & 3
constexpr int EPI_PATCH = 9216;            // bytes of wave-private fp32 epilogue staging
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// (the request through the compiler's builtin: it sets m0 itself — no hand-written m0 write to get the clobbers of wrong)
// AUX: the cache-policy bits of the request (gfx950: 1 = sc0, 2 = nt, 16 = sc1)
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void* g, unsigned char* l) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g, (void __attribute__((address_space(3)))*)l, 16, 0, AUX);
}

// XCD-aware tile order (gemm256s.hip): this workgroup's (M-tile, N-tile) of a launch over ntn N-tiles, row-major inside an XCD's share;
// n_group > 0: the order sweeps the M-tiles once per group of n_group N-tiles (GemmArgs::n_group)
__device__ __forceinline__ void x_tile_of_block(int n_group, int ntn, int& mt, int& nt) {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    mt = tile / ntn; nt = tile % ntn;
    if (n_group > 0) {
        const int mts = nwg / ntn, mpx = mts >> 3, nb = n_group;
        const int i = bid >> 3, per = mpx * nb;
        const int cg = i / per, r = i - cg * per;
        mt = xcd * mpx + r / nb;
        nt = cg * nb + r % nb;
    }
}

}  // namespace
