// The record of the affine resampler and the device functions that sample ONE output voxel from its source coordinate (layout and rule:
// include/veloxseg_hip.h), shared by vx_affine_k (augment_affine.hip) and vx_elastic_k (augment_elastic.hip): both take a voxel from s_a on with the SAME code,
// so a record without a displacement field gives the same bytes through either kernel.
#pragma once
#include "vx_common.h"
#include "../../include/veloxseg_hip.h"

struct VxAffineRecord {
    const void* src;
    void* dst;
    long stride[3];
    int n[3], lo[3], hi[3];
    int dtype, mode, pad;
    float cval;
    float A[9], c[3];
    int unused;
};
static_assert(sizeof(VxAffineRecord) == VX_AFFINE_RECORD_BYTES, "record layout drifted from the header");

#define VX_AFF_GLOBAL __attribute__((address_space(1)))

// every product, sum and difference of the rule is rounded on its own (hipcc contracts a * b + c under plain -O3 unless told otherwise)
__device__ __forceinline__ float vx_aff_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float vx_aff_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float vx_aff_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float vx_aff_lerp(float u, float v, float l) {
    return vx_aff_add(vx_aff_mul(vx_aff_sub(1.0f, l), u), vx_aff_mul(l, v));
}
__device__ __forceinline__ float vx_aff_coord(const float* __restrict__ A, float c, float p0, float p1, float p2) {
    return vx_aff_add(vx_aff_add(vx_aff_add(vx_aff_mul(A[0], p0), vx_aff_mul(A[1], p1)), vx_aff_mul(A[2], p2)), c);
}

// sources live in device memory: the loads go through global pointers (a pointer read from the table is generic to the compiler, which would emit flat loads).
// Strides fit 32 bits (the host checks): an element offset is three 32 x 32 -> 64-bit multiply-adds, formed ONCE per voxel; the other seven corners are that offset
// plus a stride or nothing.  (The first form multiplied index by 64-bit stride for every corner, each load under its own exec-mask branch: 64 quarter-rate integer
// multiplies per wave, and the pass ran at the speed of those, not of its loads: DESIGN.md section 28.)
__device__ __forceinline__ long vx_aff_offset(const VxAffineRecord* __restrict__ R, int d, int h, int w) {
    // the strides as 32-bit scalars (the kernel has checked that they fit): through readfirstlane, or the compiler sees the 64-bit value behind them and multiplies by that
    const int s0 = __builtin_amdgcn_readfirstlane((int)R->stride[0]), s1 = __builtin_amdgcn_readfirstlane((int)R->stride[1]), s2 = __builtin_amdgcn_readfirstlane((int)R->stride[2]);
    return (long)d * s0 + (long)h * s1 + (long)w * s2;
}

template <typename T>
__device__ __forceinline__ T vx_aff_nearest(const VxAffineRecord* __restrict__ R, float sd, float sh, float sw) {
    const int d = (int)nearbyintf(sd), h = (int)nearbyintf(sh), w = (int)nearbyintf(sw);
    const int lo0 = R->lo[0], lo1 = R->lo[1], lo2 = R->lo[2], hi0 = R->hi[0], hi1 = R->hi[1], hi2 = R->hi[2];
    const bool in = d >= lo0 && d <= hi0 && h >= lo1 && h <= hi1 && w >= lo2 && w <= hi2;                  // (border: always)
    // the load is unconditional, from an index clamped into the range (always a valid address); a sample outside the range takes cval instead
    const T t = ((const VX_AFF_GLOBAL T*)R->src)[vx_aff_offset(R, min(max(d, lo0), hi0), min(max(h, lo1), hi1), min(max(w, lo2), hi2))];
    return in ? t : (T)R->cval;
}

__device__ __forceinline__ float vx_aff_trilinear(const VxAffineRecord* __restrict__ R, float sd, float sh, float sw) {
    const int lo0 = R->lo[0], lo1 = R->lo[1], lo2 = R->lo[2], hi0 = R->hi[0], hi1 = R->hi[1], hi2 = R->hi[2];
    const float fd = floorf(sd), fh = floorf(sh), fw = floorf(sw);
    const int d0 = (int)fd, h0 = (int)fh, w0 = (int)fw;
    const float ld = vx_aff_sub(sd, fd), lh = vx_aff_sub(sh, fh), lw = vx_aff_sub(sw, fw);
    // border: the coordinate was clamped, so i0 is in range and the upper corner is min(i0 + 1, hi).  constant: i0 in [lo - 1, hi + 1]; a corner outside [lo, hi]
    // reads cval -- its LOAD goes to the index clamped into the range (always a valid address) and is thrown away.  Either way the two addresses of an axis are
    // clamp(i0) and clamp(i0 + 1): the same or one stride apart.
    const int a0 = min(max(d0, lo0), hi0), a1 = min(max(d0 + 1, lo0), hi0), b0 = min(max(h0, lo1), hi1), b1 = min(max(h0 + 1, lo1), hi1);
    const int c0 = min(max(w0, lo2), hi2), c1 = min(max(w0 + 1, lo2), hi2);
    const bool border = R->pad == 0;
    const bool okd0 = border || a0 == d0, okd1 = border || a1 == d0 + 1, okh0 = border || b0 == h0, okh1 = border || b1 == h0 + 1;
    const bool okw0 = border || c0 == w0, okw1 = border || c1 == w0 + 1;
    const long ed = a1 != a0 ? R->stride[0] : 0L, eh = b1 != b0 ? R->stride[1] : 0L, ew = c1 != c0 ? R->stride[2] : 0L;
    const VX_AFF_GLOBAL float* p = (const VX_AFF_GLOBAL float*)R->src + vx_aff_offset(R, a0, b0, c0);
    const float t000 = p[0], t001 = p[ew], t010 = p[eh], t011 = p[eh + ew], t100 = p[ed], t101 = p[ed + ew], t110 = p[ed + eh], t111 = p[ed + eh + ew];
    const float cval = R->cval;
    const float v000 = okd0 && okh0 && okw0 ? t000 : cval, v001 = okd0 && okh0 && okw1 ? t001 : cval, v010 = okd0 && okh1 && okw0 ? t010 : cval;
    const float v011 = okd0 && okh1 && okw1 ? t011 : cval, v100 = okd1 && okh0 && okw0 ? t100 : cval, v101 = okd1 && okh0 && okw1 ? t101 : cval;
    const float v110 = okd1 && okh1 && okw0 ? t110 : cval, v111 = okd1 && okh1 && okw1 ? t111 : cval;
    const float r00 = vx_aff_lerp(v000, v001, lw), r01 = vx_aff_lerp(v010, v011, lw), r10 = vx_aff_lerp(v100, v101, lw), r11 = vx_aff_lerp(v110, v111, lw);
    const float q0 = vx_aff_lerp(r00, r01, lh), q1 = vx_aff_lerp(r10, r11, lh);
    return vx_aff_lerp(q0, q1, ld);
}
