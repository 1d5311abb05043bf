// Training batch assembly: MONAI RandFlipd / RandScaleIntensityd / RandShiftIntensityd / RandGaussianNoised folded into one table-driven
// pass that writes every modality of every sample straight into the (B, M, D, H, W) fp32 batch and the (B, 1, D, H, W) int64 label batch.  One record = one channel
// of one source (layout: include/veloxseg_hip.h); each source voxel is read once, each batch element written once.  Streaming kernels (HBM-bound): a block works on
// ONE record, so the record is block-uniform (blockIdx only) and its fields, the step program included, come through scalar loads; the lanes walk the patch in flat
// order, four voxels each when W % 4 == 0 (16-byte stores always; 16-byte loads when the source row is contiguous and aligned, four scalar loads otherwise), one
// voxel each when it is not.  No operation of the pointwise program is contracted with another: the fused result has the bits of the transforms applied one by one.
#include "augment_steps.h"

// four consecutive source elements p[0], p[s], p[2s], p[3s]: ONE 16-byte (4 x sizeof(T) for the narrower / wider types) access when they are adjacent and aligned.
// Sources live in device memory: the loads go through global pointers (a pointer read from the table is generic to the compiler, which would emit flat loads).
// A non-temporal wide load was tried and is slower (B 4, M 2, 128^3: 45.0 against 39.3 us): the sources were just written by the crop and sit in the cache.
#define VX_AUG_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ void vx_aug_load4(const T* __restrict__ p, long s, T (&t)[4]) {
    typedef T VT __attribute__((ext_vector_type(4)));
    if (s == 1 && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0) {
        const VT q = *(const VX_AUG_GLOBAL VT*)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = q[k];
    } else {
        const VX_AUG_GLOBAL T* g = (const VX_AUG_GLOBAL T*)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = g[k * s];
    }
}

// QUAD: W % 4 == 0, an item is four voxels of one row; otherwise an item is one voxel.  grid = n records x bpr blocks.
template <bool QUAD>
__global__ void __launch_bounds__(256) vx_augment_image_k(const VxAugRecord* __restrict__ recs, float* __restrict__ out, int B, int M, int D, int H, int W, long items, int bpr) {
    const VxAugRecord* __restrict__ R = recs + (blockIdx.x / (unsigned)bpr);
    const long it = (long)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
    const int b = R->b, c = R->c, flip = R->flip;
    if (R->dtype != 0 || b < 0 || b >= B || c < 0 || c >= M || it >= items) return;
    const long V = (long)D * H * W;
    const long v = QUAD ? it * 4 : it;
    int d, h, w;
    vx_aug_coords(v, V, H, W, d, h, w);
    constexpr int N = QUAD ? 4 : 1;
    const int sd = (flip & 1) ? D - 1 - d : d, sh = (flip & 2) ? H - 1 - h : h, sw = (flip & 4) ? W - N - w : w;
    const long s2 = R->stride[2];
    const float* __restrict__ p = static_cast<const float*>(R->src) + sd * R->stride[0] + sh * R->stride[1] + sw * s2;
    float t[N];
    if (QUAD) {
        float q[4];
        vx_aug_load4<float>(p, s2, q);
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = (flip & 4) ? q[3 - k] : q[k];        // a W-flip reads the mirrored four voxels and reverses them in registers
    } else {
        t[0] = ((const VX_AUG_GLOBAL float*)p)[0];
    }
    const int ns = min(max(R->n_steps, 0), VX_AUG_MAX_STEPS);
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
            const int pm = (int)(op >> 4) & 7;                                   // flips that follow the noise step: the voxel it was added at
            const int nd = (pm & 1) ? D - 1 - d : d, nh = (pm & 2) ? H - 1 - h : h, nw = (pm & 4) ? W - N - w : w;
            const long e = (long)(op >> 8) * V + ((long)nd * H + nh) * W + nw;
            if (QUAD) {                                                          // V % 4 == 0 and nw % 4 == 0: e is a multiple of 4
                float n[4];
                vx_aug_normal4(key, e, n);
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] = vx_aug_add(t[k], vx_aug_add(a, vx_aug_mul(sdv, (pm & 4) ? n[3 - k] : n[k])));
            } else {
                t[0] = vx_aug_add(t[0], vx_aug_add(a, vx_aug_mul(sdv, vx_aug_normal1(key, e))));
            }
        }
    }
    float* __restrict__ o = out + ((long)b * M + c) * V + v;
    if (QUAD) *reinterpret_cast<float4*>(o) = make_float4(t[0], t[N > 1 ? 1 : 0], t[N > 2 ? 2 : 0], t[N > 3 ? 3 : 0]);
    else o[0] = t[0];
}

// The same pass with the statistics ops 4..6, through the step function the statistics pass shares (augment_steps.h).  A kernel of its own:
// the kernel above keeps the code it had before these ops existed (folding them into it cost the noise program 3 % at B 4, M 2, 128^3: 51.3 -> 52.8 us).
template <bool QUAD>
__global__ void __launch_bounds__(256) vx_augment_image_ext_k(const VxAugRecord* __restrict__ recs, float* __restrict__ out, int B, int M, int D, int H, int W, long items, int bpr) {
    const VxAugRecord* __restrict__ R = recs + (blockIdx.x / (unsigned)bpr);
    const long it = (long)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
    const int b = R->b, c = R->c, flip = R->flip;
    if (R->dtype != 0 || b < 0 || b >= B || c < 0 || c >= M || it >= items) return;
    const long V = (long)D * H * W;
    const long v = QUAD ? it * 4 : it;
    int d, h, w;
    vx_aug_coords(v, V, H, W, d, h, w);
    constexpr int N = QUAD ? 4 : 1;
    const int sd = (flip & 1) ? D - 1 - d : d, sh = (flip & 2) ? H - 1 - h : h, sw = (flip & 4) ? W - N - w : w;
    const long s2 = R->stride[2];
    const float* __restrict__ p = static_cast<const float*>(R->src) + sd * R->stride[0] + sh * R->stride[1] + sw * s2;
    float t[N];
    if (QUAD) {
        float q[4];
        vx_aug_load4<float>(p, s2, q);
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = (flip & 4) ? q[3 - k] : q[k];        // a W-flip reads the mirrored four voxels and reverses them in registers
    } else {
        t[0] = ((const VX_AUG_GLOBAL float*)p)[0];
    }
    const int ns = min(max(R->n_steps, 0), VX_AUG_MAX_STEPS);
    vx_aug_run_steps<N, true>(R, ns, t, d, h, w, D, H, W, V, 0);
    float* __restrict__ o = out + ((long)b * M + c) * V + v;
    if (QUAD) *reinterpret_cast<float4*>(o) = make_float4(t[0], t[N > 1 ? 1 : 0], t[N > 2 ? 2 : 0], t[N > 3 ? 3 : 0]);
    else o[0] = t[0];
}

template <typename T, bool QUAD>
__device__ __forceinline__ void vx_aug_label_item(const VxAugRecord* __restrict__ R, long long* __restrict__ o, int sd, int sh, int sw, bool wflip) {
    const long s2 = R->stride[2];
    const T* __restrict__ p = static_cast<const T*>(R->src) + sd * R->stride[0] + sh * R->stride[1] + sw * s2;
    if (QUAD) {
        T q[4];
        vx_aug_load4<T>(p, s2, q);
        long long t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = (long long)(wflip ? q[3 - k] : q[k]);
        reinterpret_cast<longlong2*>(o)[0] = make_longlong2(t[0], t[1]);
        reinterpret_cast<longlong2*>(o)[1] = make_longlong2(t[2], t[3]);
    } else {
        o[0] = (long long)((const VX_AUG_GLOBAL T*)p)[0];
    }
}

template <bool QUAD>
__global__ void __launch_bounds__(256) vx_augment_label_k(const VxAugRecord* __restrict__ recs, long long* __restrict__ out, int B, int D, int H, int W, long items, int bpr) {
    const VxAugRecord* __restrict__ R = recs + (blockIdx.x / (unsigned)bpr);
    const long it = (long)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
    const int b = R->b, flip = R->flip, ty = R->dtype;
    if (R->c != VX_AUG_LABEL || b < 0 || b >= B || it >= items) return;
    const long V = (long)D * H * W;
    const long v = QUAD ? it * 4 : it;
    int d, h, w;
    vx_aug_coords(v, V, H, W, d, h, w);
    constexpr int N = QUAD ? 4 : 1;
    const int sd = (flip & 1) ? D - 1 - d : d, sh = (flip & 2) ? H - 1 - h : h, sw = (flip & 4) ? W - N - w : w;
    long long* __restrict__ o = out + (long)b * V + v;
    const bool wf = (flip & 4) != 0;
    if (ty == 1) vx_aug_label_item<unsigned char, QUAD>(R, o, sd, sh, sw, wf);
    else if (ty == 4) vx_aug_label_item<int, QUAD>(R, o, sd, sh, sw, wf);
    else if (ty == 8) vx_aug_label_item<long long, QUAD>(R, o, sd, sh, sw, wf);
    else if (ty == -4) vx_aug_label_item<float, QUAD>(R, o, sd, sh, sw, wf);
}

template <bool EXT>
static int vx_augment_batch_impl(const char* who, const void* records, int n_image, int n_label, float* x_out, void* y_out, int label_bytes, int B, int M, int D, int H, int W, void* stream) {
    VX_REQUIRE(records, "%s: null pointer (records)", who);
    VX_REQUIRE(n_image >= 0 && n_label >= 0 && (long)n_image + n_label > 0, "%s: no records (n_image %d, n_label %d)", who, n_image, n_label);
    VX_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "%s: non-positive extent (B %d, D %d, H %d, W %d)", who, B, D, H, W);
    VX_REQUIRE(M >= 1 && M <= 64, "%s: M %d outside 1..64", who, M);
    VX_REQUIRE(label_bytes == 8, "%s: label width %d bytes not supported (the label batch is int64: 8)", who, label_bytes);
    VX_REQUIRE(n_image == 0 || x_out, "%s: null pointer (x_out with %d image records)", who, n_image);
    VX_REQUIRE(n_label == 0 || y_out, "%s: null pointer (y_out with %d label records)", who, n_label);
    VX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(x_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(y_out) & 15) == 0,
               "%s: misaligned table (8 bytes) or output (16 bytes)", who);
    const long V = (long)D * H * W;
    const bool quad = (W & 3) == 0;
    const long items = quad ? V / 4 : V;
    const long bpr = (items + 255) / 256;
    VX_REQUIRE(bpr * (long)(n_image > n_label ? n_image : n_label) <= 0x7fffffffL, "%s: %ld blocks per record x %d records exceed one grid", who, bpr, n_image > n_label ? n_image : n_label);
    hipStream_t st = (hipStream_t)stream;
    const VxAugRecord* recs = static_cast<const VxAugRecord*>(records);
    if (n_image > 0) {
        const dim3 g((unsigned)(bpr * n_image)), blk(256);
        if (EXT) {
            if (quad) vx_augment_image_ext_k<true><<<g, blk, 0, st>>>(recs, x_out, B, M, D, H, W, items, (int)bpr);
            else vx_augment_image_ext_k<false><<<g, blk, 0, st>>>(recs, x_out, B, M, D, H, W, items, (int)bpr);
        } else {
            if (quad) vx_augment_image_k<true><<<g, blk, 0, st>>>(recs, x_out, B, M, D, H, W, items, (int)bpr);
            else vx_augment_image_k<false><<<g, blk, 0, st>>>(recs, x_out, B, M, D, H, W, items, (int)bpr);
        }
        VX_LAUNCH_CHECK("vx_augment_batch (images)");
    }
    if (n_label > 0) {
        const dim3 g((unsigned)(bpr * n_label)), blk(256);
        if (quad) vx_augment_label_k<true><<<g, blk, 0, st>>>(recs + n_image, static_cast<long long*>(y_out), B, D, H, W, items, (int)bpr);
        else vx_augment_label_k<false><<<g, blk, 0, st>>>(recs + n_image, static_cast<long long*>(y_out), B, D, H, W, items, (int)bpr);
        VX_LAUNCH_CHECK("vx_augment_batch (labels)");
    }
    return 0;
}

extern "C" int vx_augment_batch(const void* records, int n_image, int n_label, float* x_out, void* y_out, int label_bytes, int B, int M, int D, int H, int W, void* stream) {
    return vx_augment_batch_impl<false>("vx_augment_batch", records, n_image, n_label, x_out, y_out, label_bytes, B, M, D, H, W, stream);
}
// the same pass with ops 4..6: chosen by the host only for a table that holds one (the statistics they read were left in the table by vx_augment_stats)
extern "C" int vx_augment_batch_ext(const void* records, int n_image, int n_label, float* x_out, void* y_out, int label_bytes, int B, int M, int D, int H, int W, void* stream) {
    return vx_augment_batch_impl<true>("vx_augment_batch_ext", records, n_image, n_label, x_out, y_out, label_bytes, B, M, D, H, W, stream);
}
