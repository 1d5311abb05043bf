// Ensemble inference for gfx950: fold-averaged soft-max probabilities, their arg-max and the entropy of the mean (utils/ensemble.py).
// Two HBM-bound streaming passes over (B, K, V) fp32 volumes: one thread per voxel column (or per four neighbouring columns with 16-byte accesses), the lanes of a wave
// on consecutive voxels of every class row.  No atomics, no LDS, nothing shared between threads: the same bits every run.
#include "vx_common.h"
#include "../../include/veloxseg_hip.h"

#define VX_ENS_REG_K 8          // a column of at most this many classes stays in registers between the three steps (maximum, sum, quotient)

// (the ensemble weights are not powers of two: every weight * p and every sum goes through vx_mul_rn / vx_add_rn of vx_common.h and stays two roundings)

// V = 1: one voxel of a class row; V = 4: four neighbouring ones behind one 16-byte access (the last two indices are written through V so that the V = 1
// instantiation names no element it lacks)
template <int V> __device__ __forceinline__ void vx_ens_ld(const float* p, long i, float (&a)[V]) {
    if (V == 4) { const float4 t = vx_ld4(p, i); a[0] = t.x; a[1] = t.y; a[V - 2] = t.z; a[V - 1] = t.w; }
    else a[0] = p[i];
}
template <int V> __device__ __forceinline__ void vx_ens_st(float* p, long i, const float (&a)[V]) {
    if (V == 4) vx_st4(p, i, make_float4(a[0], a[1], a[V - 2], a[V - 1]));
    else p[i] = a[0];
}

// the running maximum that a NaN takes over for good: a column with a NaN has the maximum NaN and comes out all-NaN, as from torch.softmax
__device__ __forceinline__ float vx_max_nan(float m, float x) { return (x > m || x != x) ? x : m; }

// o[at ..] = (first ? 0 : o[at ..]) + weight * (e / s): the quotient, the product and the sum are three roundings
template <int V> __device__ __forceinline__ void vx_ens_add(float* o, long at, const float (&e)[V], const float (&s)[V], float weight, int first) {
    float q[V];
    if (first) {
#pragma unroll
        for (int j = 0; j < V; ++j) q[j] = 0.f;
    } else vx_ens_ld<V>(o, at, q);
#pragma unroll
    for (int j = 0; j < V; ++j) q[j] = vx_add_rn(q[j], vx_mul_rn(weight, e[j] / s[j]));
    vx_ens_st<V>(o, at, q);
}

// psum[b, c, v] = (first ? 0 : psum[b, c, v]) + weight * softmax_c(logits[b, :, v]).  Per column: m = max_c x_c; e_c = expf(x_c - m); s = the e_c added in class order
// from 0; p_c = e_c / s.  x - m is NaN for +inf - +inf and for -inf - -inf, so a column with a +inf and a column of -inf only come out all-NaN through s; expf(-inf) is
// exactly 0.
// REG: the column (K <= VX_ENS_REG_K classes) is read once and kept in registers; otherwise it is read three times (maximum, sum, quotient) and e_c is formed again by the
// same instructions on the same operands, so both forms give the same bits.  V = 4: four voxels per thread (Vn % 4 == 0, bases 16-byte aligned); V = 1 otherwise.
template <int V, bool REG>
__global__ void __launch_bounds__(256) vx_softmax_accumulate_k(const float* __restrict__ logits, float* __restrict__ psum, int B, int K, long Vn, float weight, int first) {
    const long n = Vn / V;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ x = logits + (long)b * K * Vn;
        float* __restrict__ o = psum + (long)b * K * Vn;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
            const long v = i * V;
            float m[V], s[V];
#pragma unroll
            for (int j = 0; j < V; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
            if (REG) {
                float e[VX_ENS_REG_K][V];
#pragma unroll
                for (int c = 0; c < VX_ENS_REG_K; ++c)
                    if (c < K) {
                        vx_ens_ld<V>(x, (long)c * Vn + v, e[c]);
#pragma unroll
                        for (int j = 0; j < V; ++j) m[j] = vx_max_nan(m[j], e[c][j]);
                    }
#pragma unroll
                for (int c = 0; c < VX_ENS_REG_K; ++c)
                    if (c < K) {
#pragma unroll
                        for (int j = 0; j < V; ++j) { e[c][j] = expf(e[c][j] - m[j]); s[j] = vx_add_rn(s[j], e[c][j]); }
                    }
#pragma unroll
                for (int c = 0; c < VX_ENS_REG_K; ++c)
                    if (c < K) vx_ens_add<V>(o, (long)c * Vn + v, e[c], s, weight, first);
            } else {
                float e[V];
                for (int c = 0; c < K; ++c) {
                    vx_ens_ld<V>(x, (long)c * Vn + v, e);
#pragma unroll
                    for (int j = 0; j < V; ++j) m[j] = vx_max_nan(m[j], e[j]);
                }
                for (int c = 0; c < K; ++c) {
                    vx_ens_ld<V>(x, (long)c * Vn + v, e);
#pragma unroll
                    for (int j = 0; j < V; ++j) s[j] = vx_add_rn(s[j], expf(e[j] - m[j]));
                }
                for (int c = 0; c < K; ++c) {
                    vx_ens_ld<V>(x, (long)c * Vn + v, e);
#pragma unroll
                    for (int j = 0; j < V; ++j) e[j] = expf(e[j] - m[j]);
                    vx_ens_add<V>(o, (long)c * Vn + v, e, s, weight, first);
                }
            }
        }
    }
}

// one term of the entropy: -(p ln p), exactly +0 for p == 0
__device__ __forceinline__ float vx_ens_term(float p) { return p == 0.f ? 0.f : -vx_mul_rn(p, logf(p)); }

// labels[b, v] = arg-max_c psum[b, c, v] by the rule of vx_argmax_k (csrc/infer.hip): first NaN, else first maximum;  entropy[b, v] = sum_c -(p ln p), the terms added in
// class order from +0, each product and each sum rounded; a term with p == 0 is +0, so a one-hot column gives +0 (the -0 of 1 * ln 1 added to +0) and a NaN gives NaN.
// One pass, every class row read once; either output may be null.  V as above (labels: four bytes behind one 32-bit store).
template <int V>
__global__ void __launch_bounds__(256) vx_prob_finalize_k(const float* __restrict__ psum, unsigned char* __restrict__ labels, float* __restrict__ entropy, int B, int K, long Vn) {
    const long n = Vn / V;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ x = psum + (long)b * K * Vn;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
            const long v = i * V;
            float best[V], h[V], p[V];
            int arg[V];
            vx_ens_ld<V>(x, v, best);
#pragma unroll
            for (int j = 0; j < V; ++j) { arg[j] = 0; h[j] = entropy ? vx_add_rn(0.f, vx_ens_term(best[j])) : 0.f; }
            for (int c = 1; c < K; ++c) {
                vx_ens_ld<V>(x, (long)c * Vn + v, p);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (p[j] > best[j] || (p[j] != p[j] && !(best[j] != best[j]))) { best[j] = p[j]; arg[j] = c; }
                    if (entropy) h[j] = vx_add_rn(h[j], vx_ens_term(p[j]));
                }
            }
            if (labels) {
                if (V == 4) *reinterpret_cast<uint32_t*>(labels + (long)b * Vn + v) = (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[V - 2] << 16 | (uint32_t)arg[V - 1] << 24;
                else labels[(long)b * Vn + v] = (unsigned char)arg[0];
            }
            if (entropy) vx_ens_st<V>(entropy + (long)b * Vn, v, h);
        }
    }
}

static inline bool vx_ens_al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// grid of a streaming pass over n work items per batch item (guide: about 8 blocks per CU, the rest by the grid-stride loops); y walks the batch
static inline dim3 vx_ens_grid(long n, int B) {
    const long gy = B > 64 ? 64 : B, cap = 2048 / gy;
    const long g = (n + 255) / 256;
    return dim3((unsigned)(g > cap ? cap : (g < 1 ? 1 : g)), (unsigned)gy);
}

extern "C" int vx_softmax_accumulate(const float* logits, float* psum, int B, int K, long V, float weight, int first, void* stream) {
    VX_REQUIRE(logits && psum, "vx_softmax_accumulate: null pointer");
    VX_REQUIRE(logits != psum, "vx_softmax_accumulate: logits and psum must not alias");
    VX_REQUIRE(K >= 1 && K <= 256, "vx_softmax_accumulate: %d classes outside 1..256", K);
    VX_REQUIRE(B > 0 && V > 0, "vx_softmax_accumulate: non-positive extent");
    const bool v4 = V % 4 == 0 && vx_ens_al(logits, 16) && vx_ens_al(psum, 16);
    const bool reg = K <= VX_ENS_REG_K;
    const dim3 grid = vx_ens_grid(v4 ? V / 4 : V, B);
    hipStream_t s = (hipStream_t)stream;
    if (v4 && reg) vx_softmax_accumulate_k<4, true><<<grid, dim3(256), 0, s>>>(logits, psum, B, K, V, weight, first);
    else if (v4) vx_softmax_accumulate_k<4, false><<<grid, dim3(256), 0, s>>>(logits, psum, B, K, V, weight, first);
    else if (reg) vx_softmax_accumulate_k<1, true><<<grid, dim3(256), 0, s>>>(logits, psum, B, K, V, weight, first);
    else vx_softmax_accumulate_k<1, false><<<grid, dim3(256), 0, s>>>(logits, psum, B, K, V, weight, first);
    VX_LAUNCH_CHECK("vx_softmax_accumulate");
    return 0;
}

extern "C" int vx_prob_finalize(const float* psum, unsigned char* labels, float* entropy, int B, int K, long V, void* stream) {
    VX_REQUIRE(psum && (labels || entropy), "vx_prob_finalize: null pointer");
    VX_REQUIRE(K >= 1 && K <= 256, "vx_prob_finalize: %d classes outside 1..256", K);
    VX_REQUIRE(B > 0 && V > 0, "vx_prob_finalize: non-positive extent");
    const bool v4 = V % 4 == 0 && vx_ens_al(psum, 16) && vx_ens_al(entropy, 16) && vx_ens_al(labels, 4);      // (a null output counts as aligned)
    const dim3 grid = vx_ens_grid(v4 ? V / 4 : V, B);
    if (v4) vx_prob_finalize_k<4><<<grid, dim3(256), 0, (hipStream_t)stream>>>(psum, labels, entropy, B, K, V);
    else vx_prob_finalize_k<1><<<grid, dim3(256), 0, (hipStream_t)stream>>>(psum, labels, entropy, B, K, V);
    VX_LAUNCH_CHECK("vx_prob_finalize");
    return 0;
}
