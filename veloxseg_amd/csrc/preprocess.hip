// Volume preprocessing on the GPU: masked fp64 moments, z-score / CT apply, radix-select histograms for exact dataset order statistics, separable resampling.
// Reference call sites: preprocess/normalization_MRI.py:7-12,52 and preprocess/normalization_CT_PET.py:6-11,67 (zscore), :23-31 (CTnorm), :65-81 (foreground intensity
// statistics with np.percentile), utils/inference_extern_mri.py:73-75,95 (MONAI Spacingd(bilinear, bilinear, nearest) + NormalizeIntensityd(channel_wise=True)).  MONAI is not
// available: the resampling restates Spacing for axis-aligned affines (tests/preprocess_ref.py) and is unpinned against MONAI itself.  All kernels are streaming
// passes with `long` indexing (HBM-bound); contracts in include/veloxseg_hip.h.
#include "vx_common.h"

#define VX_MOM_BLOCKS 1024

// sum of three doubles over a 256-thread block in a fixed order (butterfly inside the wave, then wave 0..3); valid in thread 0
__device__ __forceinline__ void vx_block_sum3(double& a, double& b, double& c, double* sm) {
    a = vx_wave_sum(a); b = vx_wave_sum(b); c = vx_wave_sum(c);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm[wid] = a; sm[4 + wid] = b; sm[8 + wid] = c; }
    __syncthreads();
    a = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    b = ((sm[4] + sm[5]) + sm[6]) + sm[7];
    c = ((sm[8] + sm[9]) + sm[10]) + sm[11];
}

// per-block partials (count, sum d, sum d^2), d = x - *center, over {x > *thr} & {mask > 0}; 16-byte loads when there is no mask and x is aligned
template <typename M, bool MASK>
__global__ void __launch_bounds__(256) vx_moments_partials_k(const float* __restrict__ x, long n, const float* __restrict__ thr, const M* __restrict__ mask,
                                                             const double* __restrict__ center, double* __restrict__ ws) {
    __shared__ double sm[12];
    const bool ht = thr != nullptr;
    const float t = ht ? thr[0] : 0.0f;
    const double c = center ? center[0] : 0.0;
    double cnt = 0.0, s = 0.0, q = 0.0;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    long done = 0;
    if (!MASK && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const long n4 = n >> 2;
        for (long i = tid; i < n4; i += nth) {
            const float4 v4 = vx_ld4(x, 4 * i);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (!ht || v[k] > t) { const double d = (double)v[k] - c; cnt += 1.0; s += d; q += d * d; }
        }
        done = n4 << 2;
    }
    for (long i = done + tid; i < n; i += nth) {
        const float v = x[i];
        bool sel = !ht || v > t;
        if (MASK) sel = sel && mask[i] > 0;
        if (sel) { const double d = (double)v - c; cnt += 1.0; s += d; q += d * d; }
    }
    vx_block_sum3(cnt, s, q, sm);
    if (threadIdx.x == 0) { ws[blockIdx.x] = cnt; ws[VX_MOM_BLOCKS + blockIdx.x] = s; ws[2 * VX_MOM_BLOCKS + blockIdx.x] = q; }
}

// one block: the VX_MOM_BLOCKS partials added in a fixed order (thread t takes t, t + 256, ...; then the block sum)
__global__ void __launch_bounds__(256) vx_moments_reduce_k(const double* __restrict__ ws, double* __restrict__ acc, int accumulate, double* __restrict__ stats, int phase) {
    __shared__ double sm[12];
    double cnt = 0.0, s = 0.0, q = 0.0;
    for (int j = threadIdx.x; j < VX_MOM_BLOCKS; j += 256) { cnt += ws[j]; s += ws[VX_MOM_BLOCKS + j]; q += ws[2 * VX_MOM_BLOCKS + j]; }
    vx_block_sum3(cnt, s, q, sm);
    if (threadIdx.x == 0) {
        if (acc) {
            if (accumulate) { cnt += acc[0]; s += acc[1]; q += acc[2]; }
            acc[0] = cnt; acc[1] = s; acc[2] = q;
        }
        if (stats && phase == 0) { stats[0] = cnt; stats[1] = cnt > 0.0 ? s / cnt : 0.0; }
        if (stats && phase == 1) stats[2] = cnt > 0.0 ? sqrt(q / cnt) : 0.0;
    }
}

__device__ __forceinline__ float vx_norm1(float v, bool ht, float t, int clip, float lo, float hi, float m, float s) {
    if (ht && !(v > t)) return v;
    const float c = clip ? (v < lo ? lo : (v > hi ? hi : v)) : v;          // NaN stays NaN, as in np.clip
    return (c - m) / s;
}

template <bool VEC>
__global__ void __launch_bounds__(256) vx_normalize_apply_k(const float* x, float* out, long n, const float* __restrict__ thr, const double* __restrict__ stats,
                                                            float mean, float stdv, int clip, float lo, float hi, int policy, float floor_) {
    const bool ht = thr != nullptr;
    const float t = ht ? thr[0] : 0.0f;
    const float m = stats ? (float)stats[1] : mean;
    const double sd = stats ? stats[2] : (double)stdv;
    const float s = (float)(policy == 0 ? fmax(sd, (double)floor_) : (sd == 0.0 ? 1.0 : sd));
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    long done = 0;
    if (VEC) {
        const long n4 = n >> 2;
        for (long i = tid; i < n4; i += nth) {
            float4 v = vx_ld4(x, 4 * i);
            v.x = vx_norm1(v.x, ht, t, clip, lo, hi, m, s); v.y = vx_norm1(v.y, ht, t, clip, lo, hi, m, s);
            v.z = vx_norm1(v.z, ht, t, clip, lo, hi, m, s); v.w = vx_norm1(v.w, ht, t, clip, lo, hi, m, s);
            vx_st4(out, 4 * i, v);
        }
        done = n4 << 2;
    }
    for (long i = done + tid; i < n; i += nth) out[i] = vx_norm1(x[i], ht, t, clip, lo, hi, m, s);
}

// order-preserving key of a float's bits
__device__ __forceinline__ unsigned int vx_float_key(unsigned int b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }

// four consecutive mask entries with one (two for 8-byte masks) vector load; the mask pointer is 16-byte aligned and i a multiple of 4
template <typename M, bool MASK>
__device__ __forceinline__ void vx_sel4(const M* __restrict__ mask, long i, bool (&sel)[4]) {
    if (!MASK) { sel[0] = sel[1] = sel[2] = sel[3] = true; return; }
    struct alignas(sizeof(M) * 4 > 16 ? 16 : sizeof(M) * 4) Pack { M v[4]; };
    const Pack p = *reinterpret_cast<const Pack*>(mask + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) sel[k] = p.v[k] > 0;
}

// one voxel of every lane of the block (called with a block-uniform trip count, so the ballots see whole waves): a wave whose hits all fall into one bin (tie-heavy
// CT) sends one LDS add for the whole wave
__device__ __forceinline__ void vx_hist_one(unsigned int b, bool sel, unsigned int prefix, int prefix_bits, int shift, unsigned int bin_mask, unsigned int* sh,
                                            unsigned int& kmin, unsigned int& kmax, unsigned int& nans) {
    bool hit = false;
    unsigned int bin = 0u;
    if (sel) {
        if ((b & 0x7fffffffu) > 0x7f800000u) {
            ++nans;
        } else {
            const unsigned int key = vx_float_key(b);
            kmin = min(kmin, key); kmax = max(kmax, key);
            hit = prefix_bits == 0 || (key >> (32 - prefix_bits)) == prefix;
            bin = (key >> shift) & bin_mask;
        }
    }
    const unsigned long long m = __ballot(hit);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        const unsigned int lb = (unsigned int)__shfl((int)bin, leader, 64);
        const unsigned long long same = __ballot(hit && bin == lb);
        if (same == m) { if ((int)(threadIdx.x & 63) == leader) atomicAdd(&sh[lb], (unsigned int)__popcll(m)); }
        else if (hit) atomicAdd(&sh[bin], 1u);
    }
}

// radix-select histogram: per-block LDS bins; only non-zero bins reach the global counters, one 64-bit integer atomic each.  VEC: x and the mask are 16-byte aligned, four
// voxels per lane and iteration from one 16-byte load
template <typename M, bool MASK, bool VEC>
__global__ void __launch_bounds__(256) vx_key_histogram_k(const unsigned int* __restrict__ xb, const M* __restrict__ mask, long n, unsigned int prefix, int prefix_bits,
                                                          int bin_bits, unsigned long long* __restrict__ hist, unsigned int* __restrict__ minmax,
                                                          unsigned long long* __restrict__ nan_count) {
    __shared__ unsigned int sh[2048];
    const int nb = 1 << bin_bits, shift = 32 - prefix_bits - bin_bits, lane = threadIdx.x & 63;
    const unsigned int bin_mask = (unsigned int)(nb - 1);
    for (int b = threadIdx.x; b < nb; b += 256) sh[b] = 0u;
    __syncthreads();
    unsigned int kmin = 0xffffffffu, kmax = 0u, nans = 0u;
    const long n4 = VEC ? (n >> 2) : 0;
    for (long base = (long)blockIdx.x * 256; base < n4; base += (long)gridDim.x * 256) {
        const long i = base + threadIdx.x;
        uint4 b4 = make_uint4(0u, 0u, 0u, 0u);
        bool sel[4] = {false, false, false, false};
        if (i < n4) { b4 = *reinterpret_cast<const uint4*>(xb + 4 * i); vx_sel4<M, MASK>(mask, 4 * i, sel); }
        vx_hist_one(b4.x, sel[0], prefix, prefix_bits, shift, bin_mask, sh, kmin, kmax, nans);
        vx_hist_one(b4.y, sel[1], prefix, prefix_bits, shift, bin_mask, sh, kmin, kmax, nans);
        vx_hist_one(b4.z, sel[2], prefix, prefix_bits, shift, bin_mask, sh, kmin, kmax, nans);
        vx_hist_one(b4.w, sel[3], prefix, prefix_bits, shift, bin_mask, sh, kmin, kmax, nans);
    }
    for (long base = (n4 << 2) + (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
        const long i = base + threadIdx.x;
        bool sel = false;
        unsigned int b = 0u;
        if (i < n) {
            sel = true;
            if (MASK) sel = mask[i] > 0;
            b = xb[i];
        }
        vx_hist_one(b, sel, prefix, prefix_bits, shift, bin_mask, sh, kmin, kmax, nans);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 256) { const unsigned int c = sh[b]; if (c) atomicAdd(hist + b, (unsigned long long)c); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, 64)); kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, 64));
        nans += (unsigned int)__shfl_xor((int)nans, o, 64);
    }
    if (lane == 0) {
        if (minmax && kmin <= kmax) { atomicMin(minmax, kmin); atomicMax(minmax + 1, kmax); }
        if (nan_count && nans) atomicAdd(nan_count, (unsigned long long)nans);
    }
}

__device__ __forceinline__ int vx_clampi(int v, int n) { return min(max(v, 0), n - 1); }

// one wave per output row (c, zo, yo): the row's z / y table entries are wave-uniform (scalar loads), the lanes walk x
__global__ void __launch_bounds__(256) vx_resample_axes_k(const float* __restrict__ x, float* __restrict__ out, long Vi, long rows, int D, int H, int W, int Do, int Ho, int Wo,
                                                          const int* __restrict__ i0, const int* __restrict__ i1, const float* __restrict__ w, int mode) {
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= rows) return;
    const int yo = (int)(row % Ho), zo = (int)((row / Ho) % Do);
    const long c = row / ((long)Ho * Do);
    const float* __restrict__ xc = x + c * Vi;
    float* __restrict__ orow = out + row * Wo;
    const int lane = threadIdx.x & 63;
    const int z0 = vx_clampi(i0[zo], D), y0 = vx_clampi(i0[Do + yo], H);
    const int* __restrict__ x0t = i0 + Do + Ho;
    if (mode == 1) {
        const float* __restrict__ r = xc + ((long)z0 * H + y0) * W;
        for (int xo = lane; xo < Wo; xo += 64) orow[xo] = r[vx_clampi(x0t[xo], W)];
        return;
    }
    const int z1 = vx_clampi(i1[zo], D), y1 = vx_clampi(i1[Do + yo], H);
    const float wz = w[zo], wy = w[Do + yo];
    const int* __restrict__ x1t = i1 + Do + Ho;
    const float* __restrict__ wxt = w + Do + Ho;
    const float* __restrict__ r00 = xc + ((long)z0 * H + y0) * W;
    const float* __restrict__ r01 = xc + ((long)z0 * H + y1) * W;
    const float* __restrict__ r10 = xc + ((long)z1 * H + y0) * W;
    const float* __restrict__ r11 = xc + ((long)z1 * H + y1) * W;
    for (int xo = lane; xo < Wo; xo += 64) {
        const int x0 = vx_clampi(x0t[xo], W), x1 = vx_clampi(x1t[xo], W);
        const float wx = wxt[xo];
        const float a00 = r00[x0], a01 = r01[x0], a10 = r10[x0], a11 = r11[x0];
        const float l00 = fmaf(wx, r00[x1] - a00, a00), l01 = fmaf(wx, r01[x1] - a01, a01);
        const float l10 = fmaf(wx, r10[x1] - a10, a10), l11 = fmaf(wx, r11[x1] - a11, a11);
        const float m0 = fmaf(wy, l01 - l00, l00), m1 = fmaf(wy, l11 - l10, l10);
        orow[xo] = fmaf(wz, m1 - m0, m0);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) vx_resample_axes_label_k(const T* __restrict__ x, T* __restrict__ out, long Vi, long rows, int D, int H, int W, int Do, int Ho, int Wo,
                                                                const int* __restrict__ i0) {
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= rows) return;
    const int yo = (int)(row % Ho), zo = (int)((row / Ho) % Do);
    const long c = row / ((long)Ho * Do);
    const int z0 = vx_clampi(i0[zo], D), y0 = vx_clampi(i0[Do + yo], H);
    const T* __restrict__ r = x + c * Vi + ((long)z0 * H + y0) * W;
    T* __restrict__ orow = out + row * Wo;
    const int* __restrict__ x0t = i0 + Do + Ho;
    for (int xo = (int)(threadIdx.x & 63); xo < Wo; xo += 64) orow[xo] = r[vx_clampi(x0t[xo], W)];
}

// One output row of vx_native_argmax_k.  ZS / YS: the row's two z / y source indices are the same (a clamped edge, a volume one voxel thick): the second plane / row
// would load the bytes the first one has loaded, so its lerps are taken over instead of formed again -- the same values, the same seven fmaf, half or a quarter of the gathers.
template <bool ZS, bool YS>
__device__ __forceinline__ void vx_native_argmax_row(const float* __restrict__ x, unsigned char* __restrict__ orow, int C, long Vi, int W, int Wo, int lane, long o00, long o01,
                                                     long o10, long o11, float wy, float wz, const int* __restrict__ x0t, const int* __restrict__ x1t, const float* __restrict__ wxt) {
    for (int xo = lane; xo < Wo; xo += 64) {
        const int x0 = vx_clampi(x0t[xo], W), x1 = vx_clampi(x1t[xo], W);
        const float wx = wxt[xo];
        float best = -INFINITY;
        int arg = 0;
        const float* __restrict__ xc = x;
        for (int c = 0; c < C; ++c, xc += Vi) {
            const float a00 = xc[o00 + x0];
            const float l00 = fmaf(wx, xc[o00 + x1] - a00, a00);
            float l01 = l00, l10 = l00, l11 = l00;
            if (!YS) { const float a01 = xc[o01 + x0]; l01 = fmaf(wx, xc[o01 + x1] - a01, a01); }
            if (!ZS) {
                const float a10 = xc[o10 + x0];
                l10 = fmaf(wx, xc[o10 + x1] - a10, a10);
                l11 = l10;
                if (!YS) { const float a11 = xc[o11 + x0]; l11 = fmaf(wx, xc[o11 + x1] - a11, a11); }
            } else {
                l11 = l01;
            }
            const float m0 = fmaf(wy, l01 - l00, l00);
            const float m1 = ZS ? m0 : fmaf(wy, l11 - l10, l10);
            const float q = fmaf(wz, m1 - m0, m0);
            if (q > best || (q != q && !(best != best))) { best = q; arg = c; }          // NaN ranks highest, first occurrence wins
        }
        orow[xo] = (unsigned char)arg;
    }
}

// labels[zo, yo, xo] = arg-max over c of the trilinear value vx_resample_axes_k forms for (c, zo, yo, xo): the same clamped indices and the same seven fmaf in the same
// order, so the label is that of vx_argmax_channels on the resampled volume, which is never written.  One wave per output row (zo, yo) as above, the lanes walk x (their
// gathers of a source row are contiguous); the classes are walked in registers with a running best (first NaN, else first maximum: the rule of vx_sw_finalize_k); one
// byte per lane is stored.  (A form with four consecutive voxels per lane and one 32-bit store was measured 2.3 - 2.4 times slower: DESIGN.md section 27.)
__global__ void __launch_bounds__(256) vx_native_argmax_k(const float* __restrict__ x, unsigned char* __restrict__ labels, int C, long Vi, long rows, int D, int H, int W,
                                                          int Do, int Ho, int Wo, const int* __restrict__ i0, const int* __restrict__ i1, const float* __restrict__ w) {
    const long row = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= rows) return;
    const int yo = (int)(row % Ho), zo = (int)(row / Ho);
    const int lane = threadIdx.x & 63;
    const int z0 = vx_clampi(i0[zo], D), y0 = vx_clampi(i0[Do + yo], H);
    const int z1 = vx_clampi(i1[zo], D), y1 = vx_clampi(i1[Do + yo], H);
    const float wz = w[zo], wy = w[Do + yo];
    const int* __restrict__ x0t = i0 + Do + Ho;
    const int* __restrict__ x1t = i1 + Do + Ho;
    const float* __restrict__ wxt = w + Do + Ho;
    const long o00 = ((long)z0 * H + y0) * W, o01 = ((long)z0 * H + y1) * W, o10 = ((long)z1 * H + y0) * W, o11 = ((long)z1 * H + y1) * W;
    unsigned char* __restrict__ orow = labels + row * Wo;
    if (z1 == z0) {          // wave-uniform: z0, z1, y0, y1 come from scalar loads
        if (y1 == y0) vx_native_argmax_row<true, true>(x, orow, C, Vi, W, Wo, lane, o00, o01, o10, o11, wy, wz, x0t, x1t, wxt);
        else vx_native_argmax_row<true, false>(x, orow, C, Vi, W, Wo, lane, o00, o01, o10, o11, wy, wz, x0t, x1t, wxt);
    } else {
        if (y1 == y0) vx_native_argmax_row<false, true>(x, orow, C, Vi, W, Wo, lane, o00, o01, o10, o11, wy, wz, x0t, x1t, wxt);
        else vx_native_argmax_row<false, false>(x, orow, C, Vi, W, Wo, lane, o00, o01, o10, o11, wy, wz, x0t, x1t, wxt);
    }
}

static inline int vx_stream_grid(long n, int cap) { const long g = (n + 255) / 256; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }

extern "C" int vx_moments_blocks(void) { return VX_MOM_BLOCKS; }
extern "C" int vx_moments_ws_doubles(void) { return 3 * VX_MOM_BLOCKS; }

extern "C" int vx_moments_partials(const float* x, long n, const float* thr, const void* mask, int mask_bytes, const double* center, double* ws, void* stream) {
    VX_REQUIRE(x && ws && n > 0, "vx_moments_partials: bad args (null pointer or n <= 0)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(VX_MOM_BLOCKS), b(256);          // always every block: each one writes its partials, so the workspace needs no zero-fill
    if (!mask) vx_moments_partials_k<unsigned char, false><<<g, b, 0, st>>>(x, n, thr, nullptr, center, ws);
    else if (mask_bytes == 1) vx_moments_partials_k<unsigned char, true><<<g, b, 0, st>>>(x, n, thr, (const unsigned char*)mask, center, ws);
    else if (mask_bytes == 4) vx_moments_partials_k<int, true><<<g, b, 0, st>>>(x, n, thr, (const int*)mask, center, ws);
    else if (mask_bytes == 8) vx_moments_partials_k<long long, true><<<g, b, 0, st>>>(x, n, thr, (const long long*)mask, center, ws);
    else if (mask_bytes == -4) vx_moments_partials_k<float, true><<<g, b, 0, st>>>(x, n, thr, (const float*)mask, center, ws);
    else VX_FAIL(-3, "vx_moments_partials: mask width %d bytes not supported", mask_bytes);
    VX_LAUNCH_CHECK("vx_moments_partials");
    return 0;
}

extern "C" int vx_moments_reduce(const double* ws, double* acc, int accumulate, double* stats, int phase, void* stream) {
    VX_REQUIRE(ws && (acc || stats) && phase >= -1 && phase <= 1 && (stats || phase == -1), "vx_moments_reduce: bad args");
    vx_moments_reduce_k<<<dim3(1), dim3(256), 0, (hipStream_t)stream>>>(ws, acc, accumulate, stats, phase);
    VX_LAUNCH_CHECK("vx_moments_reduce");
    return 0;
}

extern "C" int vx_moments_stats(const float* x, long n, const float* thr, double* ws, double* stats, void* stream) {
    VX_REQUIRE(x && ws && stats && n > 0, "vx_moments_stats: bad args (null pointer or n <= 0)");
    int rc = vx_moments_partials(x, n, thr, nullptr, 0, nullptr, ws, stream);
    if (rc == 0) rc = vx_moments_reduce(ws, nullptr, 0, stats, 0, stream);
    if (rc == 0) rc = vx_moments_partials(x, n, thr, nullptr, 0, stats + 1, ws, stream);
    if (rc == 0) rc = vx_moments_reduce(ws, nullptr, 0, stats, 1, stream);
    return rc;
}

extern "C" int vx_normalize_apply(const float* x, float* out, long n, const float* thr, const double* stats, float mean, float std, int clip, float lo, float hi,
                                  int policy, float floor, void* stream) {
    VX_REQUIRE(x && out && n > 0, "vx_normalize_apply: bad args (null pointer or n <= 0)");
    VX_REQUIRE(policy == 0 || policy == 1, "vx_normalize_apply: policy %d is neither 0 (max(std, floor)) nor 1 (std == 0 -> 1)", policy);
    VX_REQUIRE(!clip || lo <= hi, "vx_normalize_apply: clip bounds out of order");
    VX_REQUIRE(out == x || out + n <= x || x + n <= out, "vx_normalize_apply: out overlaps x without being x");
    hipStream_t st = (hipStream_t)stream;
    const dim3 b(256);
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0)
        vx_normalize_apply_k<true><<<dim3(vx_stream_grid((n + 3) / 4, 8192)), b, 0, st>>>(x, out, n, thr, stats, mean, std, clip, lo, hi, policy, floor);
    else
        vx_normalize_apply_k<false><<<dim3(vx_stream_grid(n, 8192)), b, 0, st>>>(x, out, n, thr, stats, mean, std, clip, lo, hi, policy, floor);
    VX_LAUNCH_CHECK("vx_normalize_apply");
    return 0;
}

extern "C" int vx_key_histogram(const float* x, const void* mask, int mask_bytes, long n, long prefix, int prefix_bits, int bin_bits, unsigned long long* hist,
                                unsigned int* minmax_key, unsigned long long* nan_count, void* stream) {
    VX_REQUIRE(x && hist && n > 0, "vx_key_histogram: bad args (null pointer or n <= 0)");
    VX_REQUIRE(bin_bits >= 1 && bin_bits <= 11 && prefix_bits >= 0 && prefix_bits + bin_bits <= 32, "vx_key_histogram: bad bit split (%d prefix + %d bin bits)", prefix_bits, bin_bits);
    VX_REQUIRE(prefix >= 0 && (prefix_bits == 0 ? prefix == 0 : prefix < (1L << prefix_bits)), "vx_key_histogram: prefix does not fit its %d bits", prefix_bits);
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(vx_stream_grid((n + 3) / 4, 1024)), b(256);
    const unsigned int* xb = reinterpret_cast<const unsigned int*>(x);
    const unsigned int p = (unsigned int)prefix;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0;
#define VX_HIST(M, MASK)                                                                                                                                  \
    do {                                                                                                                                                  \
        if (vec) vx_key_histogram_k<M, MASK, true><<<g, b, 0, st>>>(xb, (const M*)mask, n, p, prefix_bits, bin_bits, hist, minmax_key, nan_count);       \
        else vx_key_histogram_k<M, MASK, false><<<g, b, 0, st>>>(xb, (const M*)mask, n, p, prefix_bits, bin_bits, hist, minmax_key, nan_count);          \
    } while (0)
    if (!mask) VX_HIST(unsigned char, false);
    else if (mask_bytes == 1) VX_HIST(unsigned char, true);
    else if (mask_bytes == 4) VX_HIST(int, true);
    else if (mask_bytes == 8) VX_HIST(long long, true);
    else if (mask_bytes == -4) VX_HIST(float, true);
    else VX_FAIL(-3, "vx_key_histogram: mask width %d bytes not supported", mask_bytes);
#undef VX_HIST
    VX_LAUNCH_CHECK("vx_key_histogram");
    return 0;
}

static int vx_resample_check(const char* name, const void* x, const void* out, const int* i0, int C, int D, int H, int W, int Do, int Ho, int Wo, long* total) {      // *total = output rows
    VX_REQUIRE(x && out && i0 && x != out, "%s: bad args (null pointer, or out aliases x)", name);
    VX_REQUIRE(C > 0 && D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0, "%s: bad sizes", name);
    *total = (long)C * Do * Ho;          // output rows: one wave each
    VX_REQUIRE((*total + 3) / 4 <= 0x7fffffffL, "%s: output of %ld rows is too large for one launch", name, *total);
    return 0;
}

extern "C" int vx_resample_axes(const float* x, float* out, int C, int D, int H, int W, int Do, int Ho, int Wo, const int* i0, const int* i1, const float* w, int mode, void* stream) {
    long total = 0;
    if (int rc = vx_resample_check("vx_resample_axes", x, out, i0, C, D, H, W, Do, Ho, Wo, &total)) return rc;
    VX_REQUIRE(mode == 0 || mode == 1, "vx_resample_axes: mode %d is neither 0 (trilinear) nor 1 (nearest)", mode);
    VX_REQUIRE(mode == 1 || (i1 && w), "vx_resample_axes: bad args (the trilinear mode needs i1 and w)");
    vx_resample_axes_k<<<dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(x, out, (long)D * H * W, total, D, H, W, Do, Ho, Wo, i0, i1, w, mode);
    VX_LAUNCH_CHECK("vx_resample_axes");
    return 0;
}

extern "C" int vx_resample_axes_label(const void* x, void* out, int lab_bytes, int C, int D, int H, int W, int Do, int Ho, int Wo, const int* i0, void* stream) {
    long total = 0;
    if (int rc = vx_resample_check("vx_resample_axes_label", x, out, i0, C, D, H, W, Do, Ho, Wo, &total)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g((unsigned)((total + 3) / 4)), b(256);
    const long Vi = (long)D * H * W;
    if (lab_bytes == 1) vx_resample_axes_label_k<unsigned char><<<g, b, 0, st>>>((const unsigned char*)x, (unsigned char*)out, Vi, total, D, H, W, Do, Ho, Wo, i0);
    else if (lab_bytes == 4 || lab_bytes == -4) vx_resample_axes_label_k<unsigned int><<<g, b, 0, st>>>((const unsigned int*)x, (unsigned int*)out, Vi, total, D, H, W, Do, Ho, Wo, i0);
    else if (lab_bytes == 8) vx_resample_axes_label_k<unsigned long long><<<g, b, 0, st>>>((const unsigned long long*)x, (unsigned long long*)out, Vi, total, D, H, W, Do, Ho, Wo, i0);
    else VX_FAIL(-3, "vx_resample_axes_label: label width %d bytes not supported", lab_bytes);
    VX_LAUNCH_CHECK("vx_resample_axes_label");
    return 0;
}

extern "C" int vx_native_argmax(const float* logits, unsigned char* labels, int C, int D, int H, int W, int Do, int Ho, int Wo, const int* i0, const int* i1, const float* w,
                                void* stream) {
    VX_REQUIRE(logits && labels && i0 && i1 && w, "vx_native_argmax: bad args (null pointer)");
    VX_REQUIRE(C >= 1 && C <= 256, "vx_native_argmax: %d classes (1 .. 256 fit a uint8 label)", C);
    VX_REQUIRE(D > 0 && H > 0 && W > 0 && Do > 0 && Ho > 0 && Wo > 0, "vx_native_argmax: bad sizes");
    const long rows = (long)Do * Ho;          // output rows: one wave each
    VX_REQUIRE((rows + 3) / 4 <= 0x7fffffffL, "vx_native_argmax: output of %ld rows is too large for one launch", rows);
    const dim3 g((unsigned)((rows + 3) / 4)), b(256);
    const long Vi = (long)D * H * W;
    vx_native_argmax_k<<<g, b, 0, (hipStream_t)stream>>>(logits, labels, C, Vi, rows, D, H, W, Do, Ho, Wo, i0, i1, w);
    VX_LAUNCH_CHECK("vx_native_argmax");
    return 0;
}
