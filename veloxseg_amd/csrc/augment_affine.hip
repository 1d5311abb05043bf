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
#include "augment_affine.h"

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
