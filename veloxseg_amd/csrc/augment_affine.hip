// Spatial augmentation: 3-D affine resampling of any number of volumes in ONE launch.  One record = one output volume (layout and the whole
// rule: include/veloxseg_hip.h); a block works on ONE record, so the record is block-uniform (blockIdx only) and its fields come through scalar loads.
//
// Coordinate rule, stated once (tests/affine_ref.py follows it to the operation; nothing below is contracted):
//   p_a = (float)o_a - 0.5f * (float)(Out_a - 1);        s_a = ((A[a][0] * p_0 + A[a][1] * p_1) + A[a][2] * p_2) + c_a
//   border: s_a clamped to [lo_a, hi_a];  constant: s_a clamped to [lo_a - 1, hi_a + 1] (further out every corner reads cval and the weights are 1 and 0)
//   nearest: nearbyintf (half to even);  trilinear: from the floor corner, lerp(u, v, l) = (1 - l) * u + l * v along W, then H, then D; the upper corner is
//   min(i0 + 1, hi) under border and i0 + 1 under constant, where a corner outside [lo, hi] reads cval.
//
// The pass is a gather: each lane computes its own source address and loads its eight corners (one for nearest) with 4-byte loads; no operation of the rule is
// contracted.  Block shape (measured at B 4, two modalities + label, 128^3 from 160 x 160 x 144, one MI355X run, kernel alone, z-rotation / three rotations + scale):
//   built: 256 threads as 4 x 8 x 8 (lanes along W), two voxels per thread four planes apart = an 8 x 8 x 8 output brick     93 / 122 us
//   tried and removed: the same threads, one voxel each 119 / 132; four each 98 / 126; whole rows (1 x 2 x 128 threads) 114 / 138, four voxels each 87 / 127;
//   1 x 4 x 64 threads 114 / 138, four voxels each 87 / 127; 2 x 8 x 16 threads 114 / 137.
// The shapes differ by a few per cent; what moved the time is the number of voxels a thread has in flight.
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

// One thread, VPT output voxels BD apart along D: every value is formed before the first store, so the loads of all VPT voxels are in flight together.
template <typename T, bool TRI, int BD, int VPT>
__device__ __forceinline__ void vx_aff_run(const VxAffineRecord* __restrict__ R, int od0, int oh, int ow, int Do, int Ho, int Wo) {
    const float m = R->pad == 0 ? 0.0f : 1.0f;                   // constant: one voxel of slack on either side, where both corners already read cval
    const float p1 = vx_aff_sub((float)oh, vx_aff_mul(0.5f, (float)(Ho - 1))), p2 = vx_aff_sub((float)ow, vx_aff_mul(0.5f, (float)(Wo - 1)));
    T val[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int od = min(od0 + v * BD, Do - 1);                // (a voxel past the end recomputes the last one and is not stored)
        const float p0 = vx_aff_sub((float)od, vx_aff_mul(0.5f, (float)(Do - 1)));
        float sd = vx_aff_coord(R->A, R->c[0], p0, p1, p2), sh = vx_aff_coord(R->A + 3, R->c[1], p0, p1, p2), sw = vx_aff_coord(R->A + 6, R->c[2], p0, p1, p2);
        sd = fminf(fmaxf(sd, (float)R->lo[0] - m), (float)R->hi[0] + m);
        sh = fminf(fmaxf(sh, (float)R->lo[1] - m), (float)R->hi[1] + m);
        sw = fminf(fmaxf(sw, (float)R->lo[2] - m), (float)R->hi[2] + m);
        if (TRI) val[v] = (T)vx_aff_trilinear(R, sd, sh, sw);
        else val[v] = vx_aff_nearest<T>(R, sd, sh, sw);
    }
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int od = od0 + v * BD;
        if (od < Do) ((VX_AFF_GLOBAL T*)R->dst)[(unsigned)(od * Ho + oh) * (unsigned)Wo + (unsigned)ow] = val[v];      // (an output volume is below 2^31 voxels: the entry checks)
    }
}

// Block shape: 256 threads = BD x BH x BW, lanes along W, VPT voxels per thread along D: a block writes a (BD VPT) x BH x BW brick.  grid = n records x bricks of one volume.
template <int BD, int BH, int BW, int VPT>
__global__ void __launch_bounds__(256) vx_affine_k(const VxAffineRecord* __restrict__ recs, int Do, int Ho, int Wo, int th, int tw, int bpr) {
    static_assert(BD * BH * BW == 256, "a block is 256 threads");
    const VxAffineRecord* __restrict__ R = recs + (blockIdx.x / (unsigned)bpr);
    const unsigned tile = blockIdx.x % (unsigned)bpr;
    const unsigned trow = tile / (unsigned)tw;
    const int tz = (int)(trow / (unsigned)th), ty = (int)(trow - (unsigned)tz * (unsigned)th), tx = (int)(tile - trow * (unsigned)tw);
    const int od = tz * (BD * VPT) + (int)(threadIdx.x / (BH * BW)), oh = ty * BH + (int)((threadIdx.x / BW) % BH), ow = tx * BW + (int)(threadIdx.x % BW);
    const int ty_ = R->dtype, mode = R->mode, pad = R->pad;
    // a record the host should not have sent writes nothing (block-uniform: scalar compares)
    if (!(ty_ == 0 || ty_ == 1 || ty_ == 4 || ty_ == 8 || ty_ == -4) || (mode != 0 && mode != 1) || (pad != 0 && pad != 1)) return;
    if (mode == 0 && !(ty_ == 0 || ty_ == -4)) return;
    if (R->lo[0] > R->hi[0] || R->lo[1] > R->hi[1] || R->lo[2] > R->hi[2] || !R->src || !R->dst) return;
    if ((long)(int)R->stride[0] != R->stride[0] || (long)(int)R->stride[1] != R->stride[1] || (long)(int)R->stride[2] != R->stride[2]) return;
    if (od >= Do || oh >= Ho || ow >= Wo) return;
    if (mode == 0) vx_aff_run<float, true, BD, VPT>(R, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 1) vx_aff_run<unsigned char, false, BD, VPT>(R, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 4) vx_aff_run<int, false, BD, VPT>(R, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 8) vx_aff_run<long long, false, BD, VPT>(R, od, oh, ow, Do, Ho, Wo);
    else vx_aff_run<float, false, BD, VPT>(R, od, oh, ow, Do, Ho, Wo);
}

template <int BD, int BH, int BW, int VPT>
static int vx_affine_launch(const VxAffineRecord* recs, int n_records, int Do, int Ho, int Wo, hipStream_t st) {
    const long td = (Do + BD * VPT - 1) / (BD * VPT), th = (Ho + BH - 1) / BH, tw = (Wo + BW - 1) / BW;
    const long bpr = td * th * tw;
    if (bpr * (long)n_records > 0x7fffffffL) VX_FAIL(-3, "vx_affine_batch: %ld blocks per record x %d records exceed one grid", bpr, n_records);
    vx_affine_k<BD, BH, BW, VPT><<<dim3((unsigned)(bpr * n_records)), dim3(256), 0, st>>>(recs, Do, Ho, Wo, (int)th, (int)tw, (int)bpr);
    VX_LAUNCH_CHECK("vx_affine_batch");
    return 0;
}

extern "C" int vx_affine_batch(const void* records, int n_records, int Do, int Ho, int Wo, void* stream) {
    VX_REQUIRE(records, "vx_affine_batch: null pointer (records)");
    VX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0, "vx_affine_batch: misaligned table (8 bytes)");
    VX_REQUIRE(n_records > 0, "vx_affine_batch: no records (n_records %d)", n_records);
    VX_REQUIRE(Do > 0 && Ho > 0 && Wo > 0, "vx_affine_batch: non-positive output extent (Do %d, Ho %d, Wo %d)", Do, Ho, Wo);
    if ((long)Do * Ho * Wo > 0x7fffffffL) VX_FAIL(-3, "vx_affine_batch: an output volume of %d x %d x %d voxels is not supported (below 2^31)", Do, Ho, Wo);
    const VxAffineRecord* recs = static_cast<const VxAffineRecord*>(records);
    hipStream_t st = (hipStream_t)stream;
    return vx_affine_launch<4, 8, 8, 2>(recs, n_records, Do, Ho, Wo, st);
}
