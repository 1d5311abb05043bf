// The record of the batch-assembly table and its pointwise step program (DESIGN.md sections 25 and 29; layout: include/veloxseg_hip.h), shared by the final pass
// (augment_batch.hip) and the statistics pass (augment_stats.hip): both evaluate a program with the SAME device function, so a statistic is taken over exactly the
// bits the final pass will see at that step.
#pragma once
#include "vx_common.h"
#include "../../include/veloxseg_hip.h"

struct VxAugStep { uint32_t op; float a, b; uint32_t key; };
struct VxAugStat { float mn, mx, mean, sd; double s1, s2; };
struct VxAugRecord {
    const void* src;
    long stride[3];
    int dtype, b, c, flip;
    int n_steps, pad;
    const VxAugStat* stats;            // bytes 56..63: the device statistics table of ops 4..6, or 0 (none: every table without such a step)
    VxAugStep step[VX_AUG_MAX_STEPS];
};
static_assert(sizeof(VxAugRecord) == VX_AUG_RECORD_BYTES, "record layout drifted from the header");
static_assert(sizeof(VxAugStat) == VX_AUG_STAT_BYTES, "statistics slot drifted from the header");

// every product and sum of the program is rounded on its own (hipcc contracts a * b + c under plain -O3 unless told otherwise)
__device__ __forceinline__ float vx_aug_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float vx_aug_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float vx_aug_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float vx_aug_div(float a, float b) {          // IEEE division (hipcc's default: correctly rounded)
#pragma clang fp contract(off)
    return a / b;
}

// Box-Muller on the 24-bit uniforms of the dropout code: u1 in (0, 1] (the logarithm's argument), u2 in [0, 1); precise library functions
__device__ __forceinline__ void vx_aug_normal_pair(uint32_t ra, uint32_t rb, float& n0, float& n1) {
    const float u1 = (float)((ra >> 8) + 1u) * (1.0f / 16777216.0f);
    const float two_u2 = (float)(rb >> 8) * (1.0f / 8388608.0f);          // 2 * u2, exact
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(two_u2, &sn, &cs);
    n0 = vx_aug_mul(rad, cs);
    n1 = vx_aug_mul(rad, sn);
}
// the normals of elements e0 .. e0 + 3, e0 % 4 == 0: one Philox call
__device__ __forceinline__ void vx_aug_normal4(uint32_t key, long e0, float (&n)[4]) {
    uint32_t r[4];
    vx_philox4((uint64_t)key, VX_AUG_NOISE_STREAM, (uint64_t)e0 >> 2, r);
    vx_aug_normal_pair(r[0], r[1], n[0], n[1]);
    vx_aug_normal_pair(r[2], r[3], n[2], n[3]);
}
__device__ __forceinline__ float vx_aug_normal1(uint32_t key, long e) {
    uint32_t r[4];
    vx_philox4((uint64_t)key, VX_AUG_NOISE_STREAM, (uint64_t)e >> 2, r);
    const bool hi = (e & 2) != 0;
    float n0, n1;
    vx_aug_normal_pair(hi ? r[2] : r[0], hi ? r[3] : r[1], n0, n1);
    return (e & 1) ? n1 : n0;
}

// (d, h, w) of the flat patch index v: the index is `long`, but a patch below 2^31 voxels (uniform test) takes 32-bit divisions instead of the software sequence
// of a 64-bit one (measured at B 4, M 2, 128^3: 39.9 -> 39.3 us, so the divisions are not what bounds the pass)
__device__ __forceinline__ void vx_aug_coords(long v, long V, int H, int W, int& d, int& h, int& w) {
    if (V <= 0x7fffffffL) {
        const unsigned u = (unsigned)v, row = u / (unsigned)W;
        w = (int)(u - row * (unsigned)W);
        d = (int)(row / (unsigned)H);
        h = (int)(row - (unsigned)d * (unsigned)H);
    } else {
        const long row = v / W;
        w = (int)(v - row * W);
        d = (int)(row / H);
        h = (int)(row - (long)d * H);
    }
}

// steps 0 .. ns-1 of R's program on the N voxels t[0..N-1] that sit at (d, h, w .. w+N-1) of the frame the caller works in.  `fm` is the mask of the flips between that
// frame and the OUTPUT (0 in the final pass; the step's own mask in the statistics pass): a noise step finds its element under its mask ^ fm.
// EXT = true adds ops 4..6, which read the record's statistics table.  Ops 1..3 are the operations of vx_augment_image_k (augment_batch.hip), written with the same
// helpers: the same bits.
template <int N, bool EXT>
__device__ __forceinline__ void vx_aug_run_steps(const VxAugRecord* __restrict__ R, int ns, float (&t)[N], int d, int h, int w, int D, int H, int W, long V, int fm) {
    for (int s = 0; s < ns; ++s) {                                              // block-uniform program: scalar loads, uniform branches
        const uint32_t op = R->step[s].op;
        const float a = R->step[s].a;
        if ((op & 15u) == 1u) {
#pragma unroll
            for (int k = 0; k < N; ++k) t[k] = vx_aug_mul(t[k], a);
        } else if ((op & 15u) == 2u) {
#pragma unroll
            for (int k = 0; k < N; ++k) t[k] = vx_aug_add(t[k], a);
        } else if ((op & 15u) == 3u) {
            const float sdv = R->step[s].b;
            const uint32_t key = R->step[s].key;
            const int pm = ((int)(op >> 4) & 7) ^ fm;                            // flips that follow the noise step: the voxel it was added at
            const int nd = (pm & 1) ? D - 1 - d : d, nh = (pm & 2) ? H - 1 - h : h, nw = (pm & 4) ? W - N - w : w;
            const long e = (long)(op >> 8) * V + ((long)nd * H + nh) * W + nw;
            if (N == 4) {                                                        // V % 4 == 0 and nw % 4 == 0: e is a multiple of 4
                float n[4];
                vx_aug_normal4(key, e, n);
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] = vx_aug_add(t[k], vx_aug_add(a, vx_aug_mul(sdv, (pm & 4) ? n[3 - k] : n[k])));
            } else {
                t[0] = vx_aug_add(t[0], vx_aug_add(a, vx_aug_mul(sdv, vx_aug_normal1(key, e))));
            }
        } else if (EXT && R->stats != nullptr) {
            const VxAugStat* __restrict__ S = R->stats + R->step[s].key;         // written by an earlier launch of this stream; uniform: scalar loads
            if ((op & 15u) == 4u) {                                              // fixed-mean contrast: ((t - mean) * a) + mean, clamp to [min, max] when b != 0
                const float mean = S->mean, mn = S->mn, mx = S->mx;
                const bool clamp = R->step[s].b != 0.0f;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    float u = vx_aug_add(vx_aug_mul(vx_aug_sub(t[k], mean), a), mean);
                    t[k] = clamp ? fminf(fmaxf(u, mn), mx) : u;
                }
            } else if ((op & 15u) == 5u) {                                       // gamma: powf((t - min) / (r + 1e-7f), a) * r + min, r = max - min
                const float mn = S->mn, r = vx_aug_sub(S->mx, mn), den = vx_aug_add(r, 1e-7f);
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] = vx_aug_add(vx_aug_mul(powf(vx_aug_div(vx_aug_sub(t[k], mn), den), a), r), mn);
            } else if ((op & 15u) == 6u) {                                       // retain statistics: (t - mean2) / (std2 + 1e-8f) * std1 + mean1; slot 1 = op >> 8
                const VxAugStat* __restrict__ S1 = R->stats + (op >> 8);
                const float m2 = S->mean, den = vx_aug_add(S->sd, 1e-8f), s1 = S1->sd, m1 = S1->mean;
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] = vx_aug_add(vx_aug_mul(vx_aug_div(vx_aug_sub(t[k], m2), den), s1), m1);
            }
        }
    }
}
