// Separable Gaussian blur of any number of (D, H, W) channels in one call: MONAI RandGaussianSmoothd / GaussianFilter with zero padding.
// One record = one channel: its own source view (any strides), destination and three symmetric weight vectors, of which the table holds the halves w_0 .. w_tail
// (layout: include/veloxseg_hip.h).  Three plain passes, W then H then D, each rounded to fp32 before the next: source -> dst, dst -> tmp, tmp -> dst.
// The rule of a pass, y = w_0 x_0 + sum_{k = 1 .. tail} w_k (x_-k + x_+k) in ascending k with the pair added FIRST and zeros outside the patch, is written once
// (vx_blur_tap) and does not depend on the tiling: a thread forms one output voxel.  The pair sum is commutative, so the blur commutes with every mirror to the byte.
// A block works on ONE record: the weights and the tail come through scalar loads and the tap loop is uniform; lanes walk W fastest, so every tap of every pass is a
// coalesced row read (the taps of the W pass overlap in the same rows, those of the H and D passes are other rows), and a 128^3 channel stays in the cache.
#include "vx_common.h"
#include "../../include/veloxseg_hip.h"

struct VxBlurRecord {
    const float* src;
    float* dst;
    long stride[3];
    int tail[3];
    int pad;
    float w[3][VX_BLUR_MAX_TAIL + 1];
    int pad2[3];
};
static_assert(sizeof(VxBlurRecord) == VX_BLUR_RECORD_BYTES, "record layout drifted from the header");

#define VX_BLUR_GLOBAL __attribute__((address_space(1)))

// one output voxel of one pass: p points at x_0, `step` is the element stride along the axis, i the index along it, n its extent
__device__ __forceinline__ float vx_blur_tap(const float* __restrict__ p, long step, int i, int n, const float* __restrict__ w, int tail) {
    const VX_BLUR_GLOBAL float* g = (const VX_BLUR_GLOBAL float*)p;
    float acc = w[0] * g[0];
    for (int k = 1; k <= tail; ++k) {
        const float lo = (i - k >= 0) ? g[-(long)k * step] : 0.0f;
        const float hi = (i + k < n) ? g[(long)k * step] : 0.0f;
        const float pair = lo + hi;                                              // first; what follows may be an fma or not: one code, the same for every voxel
        acc = fmaf(w[k], pair, acc);
    }
    return acc;
}

// AXIS 2: W pass, reads the record's strided source; AXIS 1, 0: H and D passes over contiguous (D, H, W) channels `in` + r * V.  grid = n records x bpr blocks.
template <int AXIS>
__global__ void __launch_bounds__(256) vx_blur_pass_k(const VxBlurRecord* __restrict__ recs, const float* __restrict__ in, float* __restrict__ out, int D, int H, int W, long V, int bpr) {
    const int r = (int)(blockIdx.x / (unsigned)bpr);
    const VxBlurRecord* __restrict__ R = recs + r;
    const long v = (long)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
    const int tail = R->tail[AXIS];
    if (v >= V || R->src == nullptr || R->dst == nullptr || tail < 0 || tail > VX_BLUR_MAX_TAIL) return;
    const long row = v / W;
    const int w = (int)(v - row * W), d = (int)(row / H), h = (int)(row - (long)d * H);
    float y;
    if (AXIS == 2) {
        y = vx_blur_tap(R->src + d * R->stride[0] + h * R->stride[1] + w * R->stride[2], R->stride[2], w, W, R->w[2], tail);
        R->dst[v] = y;
    } else if (AXIS == 1) {
        y = vx_blur_tap((in ? in + (long)r * V : R->dst) + v, W, h, H, R->w[1], tail);
        out[(long)r * V + v] = y;
    } else {
        y = vx_blur_tap(in + (long)r * V + v, (long)H * W, d, D, R->w[0], tail);
        R->dst[v] = y;
    }
}

extern "C" int vx_blur_batch(const void* records, int n_records, float* tmp, int D, int H, int W, void* stream) {
    VX_REQUIRE(records && tmp, "vx_blur_batch: null pointer (records %p, tmp %p)", records, (void*)tmp);
    VX_REQUIRE(n_records > 0, "vx_blur_batch: no records (%d)", n_records);
    VX_REQUIRE(D > 0 && H > 0 && W > 0, "vx_blur_batch: non-positive extent (D %d, H %d, W %d)", D, H, W);
    VX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(tmp) & 3) == 0, "vx_blur_batch: misaligned table (8 bytes) or tmp (4 bytes)");
    const long V = (long)D * H * W;
    const long bpr = (V + 255) / 256;
    if (bpr * (long)n_records > 0x7fffffffL) VX_FAIL(-3, "vx_blur_batch: %ld blocks per record x %d records exceed one grid", bpr, n_records);
    hipStream_t st = (hipStream_t)stream;
    const VxBlurRecord* recs = static_cast<const VxBlurRecord*>(records);
    const dim3 g((unsigned)(bpr * n_records)), blk(256);
    vx_blur_pass_k<2><<<g, blk, 0, st>>>(recs, nullptr, nullptr, D, H, W, V, (int)bpr);
    VX_LAUNCH_CHECK("vx_blur_batch (W)");
    vx_blur_pass_k<1><<<g, blk, 0, st>>>(recs, nullptr, tmp, D, H, W, V, (int)bpr);
    VX_LAUNCH_CHECK("vx_blur_batch (H)");
    vx_blur_pass_k<0><<<g, blk, 0, st>>>(recs, tmp, nullptr, D, H, W, V, (int)bpr);
    VX_LAUNCH_CHECK("vx_blur_batch (D)");
    return 0;
}
