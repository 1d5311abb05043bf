// Paired-Window Attention on the matrix cores (gfx950, v_mfma_f32_16x16x4_f32): reference PWA.py:308-327 (attention_operation) with the relative
// position bias of attention_utils.py:120-125.  Used by vx_pwa_attn_fwd / vx_pwa_attn_bwd (pwa.hip) whenever a window's tokens tile into 16-token
// blocks (l % 64 == 0: every 128^3 configuration); other geometries keep the fp32-VALU kernels of pwa.hip.
//
// MFMA operand geometry (A lane = (row l%16, k l/16), B lane = (k l/16, col l%16), D reg i = (row 4*(l/16)+i, col l%16)); m = l%16, q' = l/16:
//   forward / dQ pass  -- "S^T" orientation, a wave owns 16 QUERIES (columns) and walks the key tiles of its window:
//        S^T[key, q] = K[key, :] . Qs[q, :]        A = K (LDS, staged once per block in operand order), B = scaled Q (registers); K = c_qk exactly:
//                                                  c_qk / 4 MFMAs per 16 x 16 tile, no padding
//        soft-max / bias / Philox mask on the 4 accumulator registers of a lane = 4 CONSECUTIVE keys of one query (one Philox call, the
//        element -> word mapping of the VALU kernels, so the masks are identical); online maximum per query (2 cross-lane steps per tile)
//        O^T[c, q] += V^T[c, key] . P^T[key, q]    the accumulator registers of S^T ARE the B operand (reduction over the tile's 16 keys = its rows):
//                                                  4 MFMAs per tile and 16 output channels, A = V^T from LDS (rows >= c_v are zero padding)
//        dP^T = V . dO^T,  dQ^T[c, q] += K^T[c, key] . dS^T[key, q]  likewise (backward pass 1, which also sums d(bias) and delta = rowsum(dO * O))
//   dK / dV pass       -- "S" orientation, a wave owns 16 KEYS (columns) and walks the query tiles:
//        S[q, key] = Qs . K^T, dP = dO . V^T,  dV^T[c, key] += dO^T[c, q] . (P*M)[q, key],  dK^T[c, key] += Qs^T[c, q] . dS[q, key]
// A block = 8 waves = 128 queries (or keys) of ONE window: K and V (resp. Q, dO, LSE, delta) of the whole window are staged in LDS once per block
// and shared by the 8 waves, instead of being re-fetched by every 64-row unit as in the VALU kernels.
#include "vx_common.h"
#include <stdlib.h>
#include "../../include/veloxseg_hip.h"

typedef float vx_f32x4 __attribute__((ext_vector_type(4)));
#define VX_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define VX_DTABLE_REPLICAS 16          // must match pwa.hip

struct VxAttnM {
    int BH, heads, Nt, ML, l, M;
    int n[3];
    float scale;
    int lin_cst, Tsz;
    int xcd;       // (round 6) bit 0 / 1: forward / backward blocks of one window are placed on one XCD (vx_xcd_rows); always 3
};

// Staging loops: 8 independent loads per thread are issued before the first LDS store (a rolled load -> store loop pays one L2 round trip per
// element: that was half of the forward kernel's time).
// lin[t] of every token of a window + the bias table of head a (bias[k] = table[k * heads + a])
__device__ __forceinline__ void vx_am_tables(const VxAttnM& A, const float* __restrict__ table, int a, int* lin, float* bias, int nthr) {
    for (int t = threadIdx.x; t < A.l; t += nthr) {
        const int t2 = t % A.n[2], t1 = (t / A.n[2]) % A.n[1], t0 = t / (A.n[2] * A.n[1]);
        lin[t] = (t0 * (2 * A.n[1] - 1) + t1) * (2 * A.n[2] - 1) + t2;
    }
    for (int k0 = threadIdx.x; k0 < A.Tsz; k0 += nthr * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * nthr; v[u] = table[(long)(k < A.Tsz ? k : 0) * A.heads + a]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * nthr; if (k < A.Tsz) bias[k] = v[u]; }
    }
}
// rows of a (ML, C) matrix in MFMA operand order: dst[((tile * C/4 + ks) * 64) + lane] = src[(16 tile + lane%16) * C + 4 ks + lane/16] * mul.
// Thread -> (row, float4 column group): one 16-byte global load, four scattered LDS stores (ML * C / 4 float4s, 8 per thread in flight).
template <int C>
__device__ __forceinline__ void vx_am_stage_op(float* __restrict__ dst, const float* __restrict__ src, int ML, float mul, int nthr) {
    const int n4 = ML * (C / 4);
    for (int e0 = threadIdx.x; e0 < n4; e0 += nthr * 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * nthr; v[u] = reinterpret_cast<const float4*>(src)[e < n4 ? e : 0]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * nthr;
            if (e < n4) {
                const int row = e / (C / 4), ks = e - row * (C / 4);
                float* d = dst + ((row >> 4) * (C / 4) + ks) * 64 + (row & 15);      // lane = 16 * (c % 4) + row % 16
                d[0] = v[u].x * mul; d[16] = v[u].y * mul; d[32] = v[u].z * mul; d[48] = v[u].w * mul;
            }
        }
    }
}
// element (row 16 tile + r, column c) of a matrix staged by vx_am_stage_op
template <int C> __device__ __forceinline__ int vx_am_op_index(int tile, int r, int c) { return ((tile * (C / 4) + (c >> 2)) * 64) + (c & 3) * 16 + r; }

// ---------------------------------------------------------------------------------------------------------------------------- forward
template <int CQ, int CV>
__global__ void __launch_bounds__(512) vx_pwa_attn_mfma_fwd_k(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ Vt,
                                                              const float* __restrict__ table, float* __restrict__ O, float* __restrict__ LSE,
                                                              VxAttnM A, VxDrop drop, unsigned short* __restrict__ mbits) {
    constexpr int KSQ = CQ / 4, CVB = (CV + 15) / 16, SV = CV + 1;      // (16 SV = 16 mod 64 banks: the four lane groups of a P.V operand read fall on different banks)
    extern __shared__ __attribute__((aligned(16))) float vx_am_lds[];
    int* __restrict__ lin = reinterpret_cast<int*>(vx_am_lds);
    float* __restrict__ bias = vx_am_lds + ((A.l + 3) & ~3);
    float* __restrict__ Kop = bias + ((A.Tsz + 3) & ~3);
    float* __restrict__ Vs = Kop + A.ML * CQ;
    int bx_, by_;
    vx_xcd_rows(bx_, by_, A.xcd & 1);         // (round 6) the blocks of a window on ONE XCD: they all stage the window's K and V
    const long win = by_;
    const int a = (int)((win / A.Nt) % A.heads);
    const float* __restrict__ kp = K + win * A.ML * CQ;
    const float* __restrict__ vp = Vt + win * A.ML * CV;
    vx_am_tables(A, table, a, lin, bias, 512);
    // K in MFMA operand order for the KEY OWNERSHIP of this kernel: in an iteration of 4 key tiles (64 keys) lane group qg owns the 16 CONSECUTIVE keys 16 qg .. 16 qg + 15
    // (row m = 4 g + i of tile u is key 16 g + 4 u + i), so that a lane's 16 dropout decisions of an iteration are 16 consecutive elements of its query's row = two
    // Philox calls (vx_attn_drop16) instead of four, and its keep bits are one whole word of the mask tensor (no cross-lane assembly)
    {
        const int n4 = A.ML * KSQ;
        for (int e0 = threadIdx.x; e0 < n4; e0 += 512 * 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + u * 512; v[u] = reinterpret_cast<const float4*>(kp)[e < n4 ? e : 0]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * 512;
                if (e < n4) {
                    const int key = e / KSQ, ks = e - key * KSQ;
                    const int it = key >> 6, w = key & 63, tu = (w >> 2) & 3, mrow = 4 * (w >> 4) + (w & 3);
                    float* d = Kop + ((4 * it + tu) * KSQ + ks) * 64 + mrow;
                    d[0] = v[u].x; d[16] = v[u].y; d[32] = v[u].z; d[48] = v[u].w;
                }
            }
        }
    }
    for (int e0 = threadIdx.x; e0 < A.ML * (CV / 4); e0 += 512 * 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * 512; v[u] = reinterpret_cast<const float4*>(vp)[e < A.ML * (CV / 4) ? e : 0]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * 512;
            if (e < A.ML * (CV / 4)) { const int key = e / (CV / 4), c4 = e - key * (CV / 4); float* d = Vs + key * SV + 4 * c4; d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w; }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, qg = lane >> 4;
    const int q0 = (bx_ * 8 + wave) * 16;
    if (q0 >= A.ML) return;
    const VxDropCtx dc = vx_attn_ctx(drop);
    const long row = win * A.ML + q0 + m;
    float qb[KSQ];
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) qb[ks] = Q[row * CQ + 4 * ks + qg] * A.scale;
    const int lin_q = lin[(q0 + m) % A.l] + A.lin_cst;
    float mrun = -INFINITY, lsum = 0.0f;
    vx_f32x4 oacc[CVB];
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) oacc[cb] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
    // KU key tiles per iteration: their S tiles, bias gathers, exponentials and Philox draws are independent, so the LDS / MFMA / transcendental
    // latencies of one tile hide behind the others', and the per-query maximum needs ONE cross-lane reduction per KU tiles
    constexpr int KU = 4;
    const int ntile = A.ML / 16;                     // l % 16 == 0 and ML >= 64: a multiple of KU
    vx_f32x4 oacc2[CVB];
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) oacc2[cb] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kt0 = 0; kt0 < ntile; kt0 += KU) {
        vx_f32x4 s[KU];
        int4 lk[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            s[u] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
            lk[u] = *reinterpret_cast<const int4*>(&lin[(16 * (kt0 + qg)) % A.l + 4 * u]);         // keys 16 (kt0 + qg) + 4 u .. + 3
        }
#pragma unroll
        for (int ks = 0; ks < KSQ; ++ks)
#pragma unroll
            for (int u = 0; u < KU; ++u) s[u] = VX_MFMA(Kop[((kt0 + u) * KSQ + ks) * 64 + lane], qb[ks], s[u]);
        float mt = -INFINITY;
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            s[u][0] += bias[lin_q - lk[u].x]; s[u][1] += bias[lin_q - lk[u].y]; s[u][2] += bias[lin_q - lk[u].z]; s[u][3] += bias[lin_q - lk[u].w];
            mt = fmaxf(mt, fmaxf(fmaxf(s[u][0], s[u][1]), fmaxf(s[u][2], s[u][3])));
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(mrun, mt);
        const float alpha = __expf(mrun - mn);
        mrun = mn;
        float psum = 0.0f;
        float m16[16];
        vx_attn_drop16(dc, (uint64_t)row * (uint64_t)A.ML + (uint64_t)(16 * (kt0 + qg)), m16);      // this lane's 16 keys of the iteration: element 4 u + i
        if (mbits != nullptr && dc.on) {               // their keep bits = the word (key tile kt0 + qg, this query) of the mask tensor (read back by the one-pass backward)
            unsigned w = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) w |= (m16[e] != 0.0f ? 1u : 0u) << e;
            mbits[(win * (A.ML >> 4) + (kt0 + qg)) * A.ML + q0 + m] = (unsigned short)w;
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { const float p = __expf(s[u][i] - mn); psum += p; s[u][i] = p * m16[4 * u + i]; }
        }
        lsum = lsum * alpha + psum;
#pragma unroll
        for (int cb = 0; cb < CVB; ++cb) { oacc[cb] *= alpha; oacc2[cb] *= alpha; }
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int cb = 0; cb < CVB; ++cb) {
                    const int ch = 16 * cb + m;
                    const float va = ch < CV ? Vs[(16 * (kt0 + qg) + 4 * u + i) * SV + ch] : 0.0f;
                    if (u & 1) oacc2[cb] = VX_MFMA(va, s[u][i], oacc2[cb]);      // two accumulators: half the dependent-MFMA chain
                    else oacc[cb] = VX_MFMA(va, s[u][i], oacc[cb]);
                }
    }
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) oacc[cb] += oacc2[cb];
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) {
        const int ch = 16 * cb + 4 * qg;                 // this lane's 4 channels of query m
        if (ch < CV) *reinterpret_cast<float4*>(O + row * CV + ch) = make_float4(oacc[cb][0] * inv, oacc[cb][1] * inv, oacc[cb][2] * inv, oacc[cb][3] * inv);
    }
    if (qg == 0) LSE[row] = mrun + __logf(lsum);
}

// ---------------------------------------------------------------------------------------------------------------------------- backward 1: dQ, delta, d(bias)
template <int CQ, int CV>
__global__ void __launch_bounds__(512) vx_pwa_attn_mfma_bwd_q_k(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ Vt,
                                                                const float* __restrict__ table, const float* __restrict__ O, const float* __restrict__ LSE,
                                                                const float* __restrict__ dO, float* __restrict__ dQ, float* __restrict__ Delta,
                                                                float* __restrict__ dtable_rep, VxAttnM A, VxDrop drop) {
    constexpr int KSQ = CQ / 4, KSV = CV / 4;
    extern __shared__ __attribute__((aligned(16))) float vx_am_lds[];
    int* __restrict__ lin = reinterpret_cast<int*>(vx_am_lds);
    float* __restrict__ bias = vx_am_lds + ((A.l + 3) & ~3);
    const int tpad = (A.Tsz + 3) & ~3;
    float* __restrict__ gtab = bias + tpad;                   // 4 replicas of the bias-gradient table, one per lane group
    float* __restrict__ Kop = gtab + 4 * tpad;
    float* __restrict__ Vop = Kop + A.ML * CQ;
    const long win = blockIdx.y;
    const int a = (int)((win / A.Nt) % A.heads);
    vx_am_tables(A, table, a, lin, bias, 512);
    for (int k = threadIdx.x; k < 4 * tpad; k += 512) gtab[k] = 0.0f;
    vx_am_stage_op<CQ>(Kop, K + win * A.ML * CQ, A.ML, 1.0f, 512);
    vx_am_stage_op<CV>(Vop, Vt + win * A.ML * CV, A.ML, 1.0f, 512);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, qg = lane >> 4;
    const int q0 = (blockIdx.x * 8 + wave) * 16;
    if (q0 < A.ML) {
        const VxDropCtx dc = vx_attn_ctx(drop);
        const long row = win * A.ML + q0 + m;
        float qb[KSQ], dob[KSV];
#pragma unroll
        for (int ks = 0; ks < KSQ; ++ks) qb[ks] = Q[row * CQ + 4 * ks + qg] * A.scale;
        float delta = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks) { dob[ks] = dO[row * CV + 4 * ks + qg]; delta = fmaf(dob[ks], O[row * CV + 4 * ks + qg], delta); }
        delta += __shfl_xor(delta, 16, 64);
        delta += __shfl_xor(delta, 32, 64);
        const float lse = LSE[row];
        const int lin_q = lin[(q0 + m) % A.l] + A.lin_cst;
        vx_f32x4 dq = {0.f, 0.f, 0.f, 0.f}, dq2 = {0.f, 0.f, 0.f, 0.f};
        constexpr int KU = 4;
        const int ntile = A.ML / 16;
        float* __restrict__ gmine = gtab + qg * tpad;          // this lane group's replica: the 16 lanes of an instruction hold 16 DIFFERENT queries of one key => distinct bins
        for (int kt0 = 0; kt0 < ntile; kt0 += KU) {
            vx_f32x4 s[KU], dp[KU];
            int4 lk[KU];
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                s[u] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
                dp[u] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
                lk[u] = *reinterpret_cast<const int4*>(&lin[(16 * (kt0 + u)) % A.l + 4 * qg]);
            }
#pragma unroll
            for (int ks = 0; ks < KSQ; ++ks)
#pragma unroll
                for (int u = 0; u < KU; ++u) s[u] = VX_MFMA(Kop[((kt0 + u) * KSQ + ks) * 64 + lane], qb[ks], s[u]);
#pragma unroll
            for (int ks = 0; ks < KSV; ++ks)
#pragma unroll
                for (int u = 0; u < KU; ++u) dp[u] = VX_MFMA(Vop[((kt0 + u) * KSV + ks) * 64 + lane], dob[ks], dp[u]);
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const int bi[4] = {lin_q - lk[u].x, lin_q - lk[u].y, lin_q - lk[u].z, lin_q - lk[u].w};
                float m4[4];
                vx_attn_masks_vox4(dc, (uint64_t)row, A.ML, 16 * (kt0 + u) + 4 * qg, m4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = __expf(s[u][i] + bias[bi[i]] - lse);
                    const float ds = p * (dp[u][i] * m4[i] - delta);
                    atomicAdd(&gmine[bi[i]], ds);
                    s[u][i] = ds;
                }
            }
#pragma unroll
            for (int u = 0; u < KU; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ka = m < CQ ? Kop[vx_am_op_index<CQ>(kt0 + u, 4 * qg + i, m < CQ ? m : 0)] : 0.0f;     // K[16kt + 4q' + i][c = m]
                    if (u & 1) dq2 = VX_MFMA(ka, s[u][i], dq2);
                    else dq = VX_MFMA(ka, s[u][i], dq);
                }
        }
        dq += dq2;
        if (4 * qg < CQ) *reinterpret_cast<float4*>(dQ + row * CQ + 4 * qg) = make_float4(dq[0] * A.scale, dq[1] * A.scale, dq[2] * A.scale, dq[3] * A.scale);
        if (qg == 0) Delta[row] = delta;
    }
    __syncthreads();
    // one of VX_DTABLE_REPLICAS copies per block: thousands of blocks adding into the same few hundred addresses serialise (folded by the dK/dV kernel)
    float* __restrict__ dst = dtable_rep + (long)((blockIdx.x + gridDim.x * blockIdx.y) % VX_DTABLE_REPLICAS) * A.Tsz * A.heads;
    for (int k = threadIdx.x; k < A.Tsz; k += 512) {
        const float g = (gtab[k] + gtab[tpad + k]) + (gtab[2 * tpad + k] + gtab[3 * tpad + k]);
        if (g != 0.0f) atomicAdd(dst + (long)k * A.heads + a, g);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- backward 2: dK, dV
template <int CQ, int CV>
__global__ void __launch_bounds__(512) vx_pwa_attn_mfma_bwd_kv_k(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ Vt,
                                                                 const float* __restrict__ table, const float* __restrict__ LSE, const float* __restrict__ Delta,
                                                                 const float* __restrict__ dO, float* __restrict__ dK, float* __restrict__ dV,
                                                                 const float* __restrict__ dtable_rep, float* __restrict__ dtable, VxAttnM A, VxDrop drop) {
    constexpr int KSQ = CQ / 4, KSV = CV / 4, CVB = (CV + 15) / 16;
    {   // fold the dQ kernel's replicated bias-gradient tables into dtable (it ran before this kernel on the same stream): one owner thread per entry
        const long nb = (long)gridDim.x * gridDim.y, bid = blockIdx.x + (long)gridDim.x * blockIdx.y;
        for (long k = bid * 512 + threadIdx.x; k < (long)A.Tsz * A.heads; k += nb * 512) {
            float g = 0.0f;
#pragma unroll
            for (int r = 0; r < VX_DTABLE_REPLICAS; ++r) g += dtable_rep[(long)r * A.Tsz * A.heads + k];
            dtable[k] += g;
        }
    }
    extern __shared__ __attribute__((aligned(16))) float vx_am_lds[];
    int* __restrict__ lin = reinterpret_cast<int*>(vx_am_lds);
    float* __restrict__ bias = vx_am_lds + ((A.l + 3) & ~3);
    float* __restrict__ Qop = bias + ((A.Tsz + 3) & ~3);
    float* __restrict__ dOop = Qop + A.ML * CQ;
    float* __restrict__ lse_s = dOop + A.ML * CV;
    float* __restrict__ del_s = lse_s + A.ML;
    const long win = blockIdx.y;
    const int a = (int)((win / A.Nt) % A.heads);
    vx_am_tables(A, table, a, lin, bias, 512);
    vx_am_stage_op<CQ>(Qop, Q + win * A.ML * CQ, A.ML, A.scale, 512);
    vx_am_stage_op<CV>(dOop, dO + win * A.ML * CV, A.ML, 1.0f, 512);
    for (int e = threadIdx.x; e < A.ML; e += 512) { lse_s[e] = LSE[win * A.ML + e]; del_s[e] = Delta[win * A.ML + e]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, qg = lane >> 4;
    const int k0 = (blockIdx.x * 8 + wave) * 16;
    if (k0 >= A.ML) return;
    const VxDropCtx dc = vx_attn_ctx(drop);
    const long krow = win * A.ML + k0 + m;
    float kb[KSQ], vb[KSV];
#pragma unroll
    for (int ks = 0; ks < KSQ; ++ks) kb[ks] = K[krow * CQ + 4 * ks + qg];
#pragma unroll
    for (int ks = 0; ks < KSV; ++ks) vb[ks] = Vt[krow * CV + 4 * ks + qg];
    const int lin_k = lin[(k0 + m) % A.l] - A.lin_cst;
    vx_f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv[CVB];
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) dv[cb] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int KU = 4;
    const int ntile = A.ML / 16;
    vx_f32x4 dk2 = {0.f, 0.f, 0.f, 0.f}, dv2[CVB];
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) dv2[cb] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
    for (int qt0 = 0; qt0 < ntile; qt0 += KU) {
        vx_f32x4 s[KU], dp[KU];
#pragma unroll
        for (int u = 0; u < KU; ++u) { s[u] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; dp[u] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int ks = 0; ks < KSQ; ++ks)
#pragma unroll
            for (int u = 0; u < KU; ++u) s[u] = VX_MFMA(Qop[((qt0 + u) * KSQ + ks) * 64 + lane], kb[ks], s[u]);
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks)
#pragma unroll
            for (int u = 0; u < KU; ++u) dp[u] = VX_MFMA(dOop[((qt0 + u) * KSV + ks) * 64 + lane], vb[ks], dp[u]);
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int qt = qt0 + u;
            const int4 lq = *reinterpret_cast<const int4*>(&lin[(16 * qt) % A.l + 4 * qg]);
            const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[16 * qt + 4 * qg]);
            const float4 d4 = *reinterpret_cast<const float4*>(&del_s[16 * qt + 4 * qg]);
            const int bi[4] = {lq.x - lin_k, lq.y - lin_k, lq.z - lin_k, lq.w - lin_k};
            const float lse[4] = {l4.x, l4.y, l4.z, l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
            float m4[4];
            vx_attn_masks_rows4(dc, (uint64_t)(win * A.ML + 16 * qt + 4 * qg), 1, A.ML, k0 + m, m4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = __expf(s[u][i] + bias[bi[i]] - lse[i]);
                s[u][i] = p * (dp[u][i] * m4[i] - del[i]);      // dS
                dp[u][i] = p * m4[i];                            // P * M
            }
        }
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int cb = 0; cb < CVB; ++cb) {
                    const int ch = 16 * cb + m;
                    const float da = ch < CV ? dOop[vx_am_op_index<CV>(qt0 + u, 4 * qg + i, ch < CV ? ch : 0)] : 0.0f;          // dO[16qt + 4q' + i][ch]
                    if (u & 1) dv2[cb] = VX_MFMA(da, dp[u][i], dv2[cb]);
                    else dv[cb] = VX_MFMA(da, dp[u][i], dv[cb]);
                }
                const float qa = m < CQ ? Qop[vx_am_op_index<CQ>(qt0 + u, 4 * qg + i, m < CQ ? m : 0)] : 0.0f;                 // scale * Q[16qt + 4q' + i][c = m]
                if (u & 1) dk2 = VX_MFMA(qa, s[u][i], dk2);
                else dk = VX_MFMA(qa, s[u][i], dk);
            }
    }
    dk += dk2;
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) dv[cb] += dv2[cb];
    if (4 * qg < CQ) *reinterpret_cast<float4*>(dK + krow * CQ + 4 * qg) = make_float4(dk[0], dk[1], dk[2], dk[3]);
#pragma unroll
    for (int cb = 0; cb < CVB; ++cb) {
        const int ch = 16 * cb + 4 * qg;
        if (ch < CV) *reinterpret_cast<float4*>(dV + krow * CV + ch) = make_float4(dv[cb][0], dv[cb][1], dv[cb][2], dv[cb][3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- backward, ONE pass
// dQ, dK, dV and d(bias) from ONE evaluation of S, P, dP, dS per (query, key) pair (the two-kernel backward above evaluates the soft-max side -- exp,
// Philox mask, bias gather -- once per kernel).  Key-owner layout: a wave owns the 16-key tile kt of EVERY modality (MF = M folded tiles: tokens t and
// t + l share their relative-position bins); a block = 4 waves = 4 key tiles x NTq <= 4 query tiles (x M x M modality pairs), so a 1024-token window is
// 8 x 8 short blocks (72 long windows in few long blocks left the last round of blocks alone on the chip: 578 -> 149 us from the decomposition alone).
// "S" orientation: rows = queries 4 qg + i, columns = keys m.
//   S = Qs K^T, dP = dO V^T                     A = the query tile (global loads, prefetched one step ahead), B = this wave's K / V (registers)
//   dV^T += dO^T (P*M),  dK^T += Qs^T dS         the accumulators ARE the B operands (reduction over the tile's queries = its rows)
//   dQ^T += K^T dS^T                             needs the tile transposed: one trip through a wave-private 16 x 20 LDS patch (4 ds_write_b32 + 1 ds_read_b128 per lane)
//   dQ: each wave sums into ITS OWN LDS image of the block's query rows (plain read-add-write, no barrier in the loop); the four images are added after the
//   loop and leave as float atomics (several key chunks per window) or stores.  dK / dV leave as float atomics when a window's queries are split over blocks.
//   d(bias): the MF x MF tiles of a step hit the same bins, their dS are added in registers first; then, WIN = true, into a wave-private window of 256
//   consecutive bins (the bins of 16 keys x <= 64 queries span < 256 values for every shipped geometry; host-checked) with plain read-add-write, one 16-lane
//   group at a time (the 16 lanes of a group hold 16 different keys of one query: distinct bins) -- an LDS float atomic per lane cost ~700 clocks per wave
//   instruction here (94 of 347 us at the 8^3-window level).  WIN = false (span too wide): LDS float atomics into a full table.
// The keep bits of the forward's dropout mask (vx_pwa_attn_fwd_mb) replace the Philox draw when given.
// Any l: tiles are laid out per modality in a padded token index (16 * ceil(l / 16)); rows / columns beyond l contribute zeros.
#define VX_B1_WIN 256
template <int CQ, int CV, int MF, bool AL, bool WIN>
__global__ void __launch_bounds__(256) vx_pwa_attn_bwd1_k(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ Vt,
                                                          const float* __restrict__ table, const float* __restrict__ O, const float* __restrict__ LSE,
                                                          const float* __restrict__ dO, float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV,
                                                          float* __restrict__ dtable_rep, VxAttnM A, VxDrop drop, int waves_used, int atomic_dq, int QS, int NTq,
                                                          const unsigned short* __restrict__ mbits) {
    constexpr int KSQ = CQ / 4, KSV = CV / 4, CVB = (CV + 15) / 16, TS = 20;
    extern __shared__ __attribute__((aligned(16))) float vx_am_lds[];
    const int NT = (A.l + 15) >> 4, lp = NT * 16;
    const int nq = NTq * 16;                                                     // padded query tokens of this block (per modality)
    const int nbias = WIN ? 2 * VX_B1_WIN : ((A.Tsz + 3) & ~3);
    int* __restrict__ lin = reinterpret_cast<int*>(vx_am_lds);                  // [lp]
    float* __restrict__ bias = vx_am_lds + lp;                                   // WIN: the block's window of the bias column (512 bins); else the whole column
    float* __restrict__ gwin = bias + nbias;                                     // WIN: [4 waves][256] bias-gradient windows; else [tpad] shared table
    float* __restrict__ lse_s = gwin + (WIN ? 4 * VX_B1_WIN : nbias);            // [MF * nq]
    float* __restrict__ del_s = lse_s + MF * nq;                                 // [MF * nq]
    float* __restrict__ dqw = del_s + MF * nq;                                   // [4 waves][MF * nq][CQ]
    float* __restrict__ trb = dqw + 4 * MF * nq * CQ;                            // [4 waves][MF][16 * TS]
    int bx_, by_;
    vx_xcd_rows(bx_, by_, A.xcd & 2);                                            // (round 6) the blocks of a window on ONE XCD
    const long win = by_;
    const int a = (int)((win / A.Nt) % A.heads);
    const long wrow = win * A.ML;
    const int qsi = bx_ % QS, q_lo = qsi * NTq;                                  // this block's query tiles: [q_lo, q_lo + NTq)
    const int kc = bx_ / QS;                                                     // its key chunk: tiles kc * waves_used ..
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, qg = lane >> 4;
    // ---- token -> linear coordinate, this block's lse / delta = rowsum(dO * O), zeroed accumulators
    for (int t = threadIdx.x; t < lp; t += 256) {
        const int tc = t < A.l ? t : A.l - 1;
        const int t2 = tc % A.n[2], t1 = (tc / A.n[2]) % A.n[1], t0 = tc / (A.n[2] * A.n[1]);
        lin[t] = (t0 * (2 * A.n[1] - 1) + t1) * (2 * A.n[2] - 1) + t2;
    }
    for (int e = threadIdx.x; e < MF * nq; e += 256) {
        const int f = e / nq, t = 16 * q_lo + (e - f * nq);
        float lse = 0.0f, del = 0.0f;
        if (t < A.l) {
            const long r = wrow + (long)f * A.l + t;
            lse = LSE[r];
#pragma unroll
            for (int c4 = 0; c4 < CV / 4; ++c4) {
                const float4 g4 = *reinterpret_cast<const float4*>(dO + r * CV + 4 * c4), o4 = *reinterpret_cast<const float4*>(O + r * CV + 4 * c4);
                del = fmaf(g4.x, o4.x, fmaf(g4.y, o4.y, fmaf(g4.z, o4.z, fmaf(g4.w, o4.w, del))));
            }
        }
        lse_s[e] = lse; del_s[e] = del;
    }
    for (int e = threadIdx.x; e < 4 * MF * nq * CQ; e += 256) dqw[e] = 0.0f;
    for (int e = threadIdx.x; e < (WIN ? 4 * VX_B1_WIN : nbias); e += 256) gwin[e] = 0.0f;
    __syncthreads();
    // ---- bin ranges: raw bin = lin_q - lin_k; the block's queries x its 64 keys, and this wave's 16 keys
    const int kt = kc * waves_used + wave;
    const bool wlive = wave < waves_used && kt < NT;
    const int ktc = wlive ? kt : 0;
    const int kcol = 16 * ktc + m;                                               // padded token of this lane's key column
    const bool kval = wlive && kcol < A.l;
    const int kcl = kcol < A.l ? kcol : A.l - 1;
    int bbase = 0, wbase = 0;
    if (WIN) {
        const int tq = min(16 * q_lo + min(lane, nq - 1), A.l - 1), tk = min(16 * kc * waves_used + lane, A.l - 1);      // (clamped tokens repeat a valid one: harmless for min / max)
        int qmin = lin[tq], kmax = lin[tk], kmaxw = lin[min(16 * ktc + m, A.l - 1)];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { qmin = min(qmin, __shfl_xor(qmin, o, 64)); kmax = max(kmax, __shfl_xor(kmax, o, 64)); kmaxw = max(kmaxw, __shfl_xor(kmaxw, o, 64)); }
        bbase = qmin - kmax;                                                     // smallest raw bin of the block
        wbase = qmin - kmaxw;                                                    // ... of this wave
        for (int x = threadIdx.x; x < 2 * VX_B1_WIN; x += 256) {
            const int k = bbase + x + A.lin_cst;
            bias[x] = table[(long)(k < 0 ? 0 : (k >= A.Tsz ? A.Tsz - 1 : k)) * A.heads + a];
        }
    } else {
        for (int k0 = threadIdx.x; k0 < A.Tsz; k0 += 256 * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int k = k0 + u * 256; v[u] = table[(long)(k < A.Tsz ? k : 0) * A.heads + a]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int k = k0 + u * 256; if (k < A.Tsz) bias[k] = v[u]; }
        }
    }
    __syncthreads();
    const VxDropCtx dc = vx_attn_ctx(drop);
    float* __restrict__ tr = trb + wave * (MF * 16 * TS);
    float* __restrict__ dqm = dqw + wave * (MF * nq * CQ);
    float* __restrict__ gw = gwin + (WIN ? wave * VX_B1_WIN : 0);
    // ---- this wave's keys
    float kb[MF][KSQ], vb[MF][KSV], kA[MF][4];
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const long kr = wrow + (long)f * A.l + kcl;
#pragma unroll
        for (int ks = 0; ks < KSQ; ++ks) { const float t_ = K[kr * CQ + 4 * ks + qg]; kb[f][ks] = kval ? t_ : 0.0f; }
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks) { const float t_ = Vt[kr * CV + 4 * ks + qg]; vb[f][ks] = kval ? t_ : 0.0f; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                            // A operand of dQ^T: K[key 4 qg + i][c = m]
            const int kk = 16 * ktc + 4 * qg + i;
            const float t_ = K[(wrow + (long)f * A.l + (kk < A.l ? kk : A.l - 1)) * CQ + (m < CQ ? m : 0)];
            kA[f][i] = (wlive && kk < A.l && m < CQ) ? t_ : 0.0f;
        }
    }
    const int lin_k = lin[kcol];
    vx_f32x4 dk[MF], dv[MF][CVB];
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        dk[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cb = 0; cb < CVB; ++cb) dv[f][cb] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // ---- operands of one query tile (every modality).  mk[g][f]: the forward's keep bits of the 4 query rows x 16 keys of tile (g, f)
    struct QOps { float qa[MF][KSQ], da[MF][KSV], qT[MF][4], dT[MF][CVB][4]; unsigned mk[MF][MF][4]; };
    const bool use_bits = mbits != nullptr && dc.on;
    const int NW16 = (A.ML + 15) >> 4;
    const unsigned short* __restrict__ mbw = use_bits ? mbits + win * NW16 * A.ML : nullptr;
    // (32-bit element offsets from the window's uniform base pointers: the loads take an SGPR base + VGPR offset, no 64-bit vector arithmetic)
    const float* __restrict__ Qw = Q + wrow * CQ;
    const float* __restrict__ dOw = dO + wrow * CV;
    auto load_q = [&](QOps& o, int qt) {
        const int qm = 16 * qt + m, qmc = qm < A.l ? qm : A.l - 1;
#pragma unroll
        for (int g = 0; g < MF; ++g) {
            const int r = g * A.l + qmc;
#pragma unroll
            for (int ks = 0; ks < KSQ; ++ks) o.qa[g][ks] = Qw[r * CQ + 4 * ks + qg] * A.scale;
#pragma unroll
            for (int ks = 0; ks < KSV; ++ks) o.da[g][ks] = dOw[r * CV + 4 * ks + qg];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qq = 16 * qt + 4 * qg + i;
                const int r2 = g * A.l + (qq < A.l ? qq : A.l - 1);
                o.qT[g][i] = Qw[r2 * CQ + (m < CQ ? m : 0)] * A.scale;
#pragma unroll
                for (int cb = 0; cb < CVB; ++cb) o.dT[g][cb][i] = dOw[r2 * CV + (16 * cb + m < CV ? 16 * cb + m : 0)];
            }
        }
        if (use_bits) {
#pragma unroll
            for (int g = 0; g < MF; ++g)
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const int k0 = f * A.l + 16 * ktc;                       // first key of the tile (window index); its 16 keys start at bit k0 & 15 of word k0 >> 4
                    const int w0 = k0 >> 4, w1 = min(w0 + 1, NW16 - 1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int qq = 16 * qt + 4 * qg + i;
                        const int rr = g * A.l + (qq < A.l ? qq : A.l - 1);
                        const unsigned lo = mbw[w0 * A.ML + rr], hi = mbw[w1 * A.ML + rr];
                        o.mk[g][f][i] = (lo | (hi << 16)) >> (k0 & 15);
                    }
                }
        }
    };
    QOps opa, opb;
    auto step = [&](QOps& cur, QOps& nxt, int j) {
        {
            const int qt = q_lo + j;
            if (j + 1 < NTq) load_q(nxt, qt + 1);
            const int4 lq = *reinterpret_cast<const int4*>(&lin[16 * qt + 4 * qg]);
            const int raw[4] = {lq.x - lin_k, lq.y - lin_k, lq.z - lin_k, lq.w - lin_k};
            bool qv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = kval && (16 * qt + 4 * qg + i < A.l);
            float bs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bs[i] = bias[qv[i] ? (WIN ? raw[i] - bbase : raw[i] + A.lin_cst) : 0];
            float dssum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < MF; ++g) {
                const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[g * nq + 16 * j + 4 * qg]);
                const float4 d4 = *reinterpret_cast<const float4*>(&del_s[g * nq + 16 * j + 4 * qg]);
                const float lse[4] = {l4.x, l4.y, l4.z, l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
                // the MF key tiles of this query tile are worked on TOGETHER, phase by phase: their MFMA chains, exponentials and LDS round trips are independent
                vx_f32x4 sv[MF], dp[MF];
#pragma unroll
                for (int f = 0; f < MF; ++f) { sv[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; dp[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
                for (int ks = 0; ks < KSQ; ++ks)
#pragma unroll
                    for (int f = 0; f < MF; ++f) sv[f] = VX_MFMA(cur.qa[g][ks], kb[f][ks], sv[f]);
#pragma unroll
                for (int ks = 0; ks < KSV; ++ks)
#pragma unroll
                    for (int f = 0; f < MF; ++f) dp[f] = VX_MFMA(cur.da[g][ks], vb[f][ks], dp[f]);
                float ds[MF][4], pm[MF][4];
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    float m4[4];
                    const uint64_t row0 = (uint64_t)(wrow + (long)g * A.l + 16 * qt + 4 * qg);
                    const long keyc = (long)f * A.l + kcol;
                    if (use_bits) {                          // one bit per pair, written by the forward: no Philox in the backward
#pragma unroll
                        for (int i = 0; i < 4; ++i) m4[i] = ((cur.mk[g][f][i] >> m) & 1u) ? dc.inv_keep : 0.0f;
                    } else if constexpr (AL) vx_attn_masks_rows4(dc, row0, 1, A.ML, keyc, m4);      // l % 4 == 0: one Philox call per lane and tile (DPP quad transpose)
                    else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) m4[i] = vx_attn_drop1(dc, (row0 + i) * (uint64_t)A.ML + (uint64_t)keyc);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float p = qv[i] ? __expf(sv[f][i] + bs[i] - lse[i]) : 0.0f;
                        pm[f][i] = p * m4[i];
                        ds[f][i] = p * (dp[f][i] * m4[i] - del[i]);
                        dssum[i] += ds[f][i];
                    }
                }
                // transpose dS through the wave's LDS patches (one per key tile): written [query 4 qg + i][key m], read [query m][keys 4 qg ..]
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int i = 0; i < 4; ++i) tr[f * (16 * TS) + (4 * qg + i) * TS + m] = ds[f][i];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int f = 0; f < MF; ++f) {
#pragma unroll
                        for (int cb = 0; cb < CVB; ++cb) dv[f][cb] = VX_MFMA(cur.dT[g][cb][i], pm[f][i], dv[f][cb]);
                        dk[f] = VX_MFMA(cur.qT[g][i], ds[f][i], dk[f]);
                    }
                // (a wave's LDS instructions execute in order: the reads below see every lane's writes; the barriers only pin the compiler's schedule --
                // a memory fence here would also wait for the prefetched global loads of the next query tile)
                __builtin_amdgcn_wave_barrier();
                float4 t4[MF];
#pragma unroll
                for (int f = 0; f < MF; ++f) t4[f] = *reinterpret_cast<const float4*>(&tr[f * (16 * TS) + m * TS + 4 * qg]);
                __builtin_amdgcn_wave_barrier();
                vx_f32x4 dqT[MF];
#pragma unroll
                for (int f = 0; f < MF; ++f) dqT[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int f = 0; f < MF; ++f) dqT[f] = VX_MFMA(kA[f][0], t4[f].x, dqT[f]);
#pragma unroll
                for (int f = 0; f < MF; ++f) dqT[f] = VX_MFMA(kA[f][1], t4[f].y, dqT[f]);
#pragma unroll
                for (int f = 0; f < MF; ++f) dqT[f] = VX_MFMA(kA[f][2], t4[f].z, dqT[f]);
#pragma unroll
                for (int f = 0; f < MF; ++f) dqT[f] = VX_MFMA(kA[f][3], t4[f].w, dqT[f]);
                if constexpr (MF == 2) dqT[0] += dqT[1];
                // dqT: lane (q = m, c = 4 qg + i) -> this wave's dQ image
                if (4 * qg < CQ) {
                    float4* dst = reinterpret_cast<float4*>(&dqm[(g * nq + 16 * j + m) * CQ + 4 * qg]);
                    float4 o4 = *dst;
                    o4.x += dqT[0][0]; o4.y += dqT[0][1]; o4.z += dqT[0][2]; o4.w += dqT[0][3];
                    *dst = o4;
                }
            }
            if constexpr (WIN) {
                // one 16-lane group at a time: its lanes are 16 different keys of one query -> 16 different bins -> plain read-add-write
#pragma unroll
                for (int ph = 0; ph < 4; ++ph) {
                    if (qg == ph) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (qv[i]) gw[raw[i] - wbase] += dssum[i];
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (qv[i]) atomicAdd(&gw[raw[i] + A.lin_cst], dssum[i]);
            }
        }
    };
    if (wlive) {
        load_q(opa, q_lo);
        for (int j = 0; j < NTq; j += 2) {          // two steps per trip: the operand sets swap roles instead of being copied
            step(opa, opb, j);
            if (j + 1 < NTq) step(opb, opa, j + 1);
        }
    }
    // ---- results
    if (kval) {
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const long kr = wrow + (long)f * A.l + kcol;
            if (QS == 1) {
                if (4 * qg < CQ) *reinterpret_cast<float4*>(dK + kr * CQ + 4 * qg) = make_float4(dk[f][0], dk[f][1], dk[f][2], dk[f][3]);
#pragma unroll
                for (int cb = 0; cb < CVB; ++cb) {
                    const int ch = 16 * cb + 4 * qg;
                    if (ch < CV) *reinterpret_cast<float4*>(dV + kr * CV + ch) = make_float4(dv[f][cb][0], dv[f][cb][1], dv[f][cb][2], dv[f][cb][3]);
                }
            } else {
                if (4 * qg < CQ) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) atomicAdd(dK + kr * CQ + 4 * qg + i, dk[f][i]);
                }
#pragma unroll
                for (int cb = 0; cb < CVB; ++cb) {
                    const int ch = 16 * cb + 4 * qg;
                    if (ch < CV) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) atomicAdd(dV + kr * CV + ch + i, dv[f][cb][i]);
                    }
                }
            }
        }
    }
    __syncthreads();
    const int img = MF * nq * CQ;
    for (int e = threadIdx.x; e < img; e += 256) {
        const int c = e % CQ, rr = e / CQ, f = rr / nq, t = 16 * q_lo + (rr - f * nq);
        if (t < A.l) {
            float* dst = dQ + (wrow + (long)f * A.l + t) * CQ + c;
            const float v = ((dqw[e] + dqw[img + e]) + (dqw[2 * img + e] + dqw[3 * img + e])) * A.scale;
            if (atomic_dq) atomicAdd(dst, v); else *dst = v;
        }
    }
    float* __restrict__ dst = dtable_rep + (long)((blockIdx.x + gridDim.x * blockIdx.y) % VX_DTABLE_REPLICAS) * A.Tsz * A.heads;
    if (WIN) {
        // raw bin x + bbase of the block window: the waves' windows start at wbase_w = qmin - kmax_w >= bbase
        __shared__ int wb_s[4];
        if (lane == 0) wb_s[wave] = wbase - bbase;
        __syncthreads();
        for (int x = threadIdx.x; x < 2 * VX_B1_WIN; x += 256) {
            float g = 0.0f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { const int y = x - wb_s[w]; if (y >= 0 && y < VX_B1_WIN) g += gwin[w * VX_B1_WIN + y]; }
            const int k = bbase + x + A.lin_cst;
            if (g != 0.0f && k >= 0 && k < A.Tsz) atomicAdd(dst + (long)k * A.heads + a, g);
        }
    } else {
        for (int k = threadIdx.x; k < A.Tsz; k += 256) {
            const float g = gwin[k];
            if (g != 0.0f) atomicAdd(dst + (long)k * A.heads + a, g);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- backward, ONE pass, 16x16x32 f16 pipe
// The one-pass decomposition above (key-owner waves, 4 key tiles x 4 query tiles per block, both modalities folded) with every GEMM on the 16-clock
// v_mfma_f32_16x16x32_f16 instead of the 32-clock fp32 16x16x4 form (16 fp32 MFMAs = 512 clocks per 16 x 16 score tile -> 5 f16 MFMAs = 80), and the operand
// traffic of the fp32 form (one register move per MFMA operand) gone.  fp32 accuracy is kept by splitting every operand into TWO fp16 pieces (22 mantissa
// bits) of the value scaled by a power of two chosen per block from the block's own maxima (exact rescale of the fp32 results):
//   S, dP      the reduction dimension is the head width (4 / 8), an MFMA reduces over 32 slots: the four piece products hi*hi, hi*lo, lo*hi, lo*lo sit side by side
//              in the slots (lane group G of the A operand reads the piece (G >> 1), of the B operand the piece (G & 1)) -> ONE MFMA per tile, all four products
//   dV, dK     reduction over 32 queries (the two modalities' tiles of a step: slot 4 g + i <-> accumulator register i of tile g, so the accumulators ARE the
//              B operand after the split); the A operand stacks the hi piece (rows 0 .. C-1) and the lo piece (rows C .. 2C-1) of dO^T / Q^T, the two row blocks
//              are added once after the loop: 2 MFMAs (B hi, B lo) per key tile
//   dQ         reduction over the wave's 32 keys; dS reaches the B operand transposed through a 16 x 20 LDS patch as ONE dword (hi | lo << 16) per element
//              (4 ds_write_b32 + 1 ds_read_b128 per tile, two v_perm_b32 per register pair split the halves again); K^T hi / lo are loop-invariant registers
// A block = 4 waves = 4 key tiles (x 2 modalities) and walks QCB chunks of 4 query tiles: per chunk the query-side operands (64 tokens x 2 modalities: Q, dO
// as pieces, row-major for S / dP and channel-major for dK / dV) are converted ONCE into LDS (the next chunk's rows are already in flight); the scales of Q / dO
// are per chunk, so dK / dV leave the MFMA accumulators after every chunk into fp32 totals in true units.  128^3 level 2 (32 query tiles): 2 blocks per key
// chunk -> two float atomics per dK / dV element instead of eight with one chunk per block (the atomics were 55 of 208 us), and the key side is set up once; soft-max side: p = exp2(fma(S, c, bias2[bin] - lse2)) with log2(e) folded into the staged bias window and lse; the dropout keep bits come from
// the forward (vx_pwa_attn_fwd_mb; 8 bytes = the 4 query rows of a lane per tile).  Geometry: l % 16 == 0, M = 2, head widths (4, 4) and (8, 8) -- the
// 128^3 levels 1 and 2; everything else keeps the kernels above.  d(bias), dQ images, atomics across blocks: as in vx_pwa_attn_bwd1_k.
typedef _Float16 vx_ah8 __attribute__((ext_vector_type(8)));
typedef _Float16 vx_ah2 __attribute__((ext_vector_type(2)));
typedef float vx_af2 __attribute__((ext_vector_type(2)));
typedef uint32_t vx_au4 __attribute__((ext_vector_type(4)));
#define VX_MFMA_H(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(vx_ah8, (a)), __builtin_bit_cast(vx_ah8, (b)), (c), 0, 0, 0)
// (a, b) -> the packed hi pieces and the packed lo pieces (hi = fp16(x), lo = fp16(x - hi); x - hi is exact in fp32)
__device__ __forceinline__ void vx_a_split2(float a, float b, uint32_t& hi, uint32_t& lo) {
    const vx_af2 v = {a, b};
    const vx_ah2 h = __builtin_convertvector(v, vx_ah2);
    const vx_ah2 l = __builtin_convertvector(v - __builtin_convertvector(h, vx_af2), vx_ah2);
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
}
// exponent e with max * 2^e in [2^(target-1), 2^target) (0 for max = 0 / inf / nan)
__device__ __forceinline__ int vx_a_exp(float mx, int target) {
    const uint32_t b = __builtin_bit_cast(uint32_t, mx);
    const int be = (int)((b >> 23) & 0xff);
    if (be == 0 || be == 255) return 0;
    int e = target - (be - 126);
    return e > 60 ? 60 : (e < -60 ? -60 : e);
}
#define VX_BH_RS 40        // halfs per row of the row-major piece image (32 used + 8 zeros: 80-byte rows, conflict-free ds_read_b128 over 16 rows)
#define VX_BH_TS 136       // halfs per row of the channel-major piece image (128 queries + 8: 272-byte rows)
// RAG (round 6; VERDICT r5 "missing" item 2: the window lengths the reference SHIPS -- 27 / 216 tokens at 96^3 patches, 32 at Hecktor's -- are not multiples of 64): the
// window is walked in chunks of 64 tokens per modality as before, LP = 64 ceil(l / 64); tokens >= l are PADDING -- their rows are staged as zeros, their linear
// coordinate repeats the last token's (every bias index stays in range and the bin windows are those vx_b1_span measures), their pairs are forced to P = dS = 0 by a
// select, nothing is stored for them; the forward's keep bits are read from words that straddle 16-key boundaries (key index f l + 16 kt is not a multiple of 16).
// `win_r`: the bias-gradient window of a lane group (a multiple of 64 >= the span the host measured; VX_B1_WIN in the aligned instances).
// MF (round 6): modalities of a window -- 2, or 1 (BraTS: one 4-channel modality group): the second modality's rows are staged as zeros and its loops are not run
template <int CQ, int CV, bool DROP, bool RAG = false, int MF = 2>
__global__ void __launch_bounds__(256, 2) vx_pwa_attn_bwd1h_k(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ Vt,
                                                           const float* __restrict__ table, const float* __restrict__ O, const float* __restrict__ LSE,
                                                           const float* __restrict__ dO, float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV,
                                                           float* __restrict__ dtable_rep, VxAttnM A, float inv_keep, int atomic_dq, int QS, int QCB,
                                                           const unsigned short* __restrict__ mbits, int LP_r, int win_r) {
    static_assert(CQ == CV && (CQ == 4 || CQ == 8), "head widths (4, 4) and (8, 8)");
    static_assert(MF == 1 || MF == 2, "one or two modalities");
    constexpr int C = CQ, TS = 20, NTq = 4, nq = 64, NR = 2 * nq;              // NR: query rows of a chunk (2 modalities x 64 tokens)
    constexpr float LOG2E = 1.4426950408889634f;
    const int LP = RAG ? LP_r : A.l, WIN = RAG ? win_r : VX_B1_WIN;
    extern __shared__ __attribute__((aligned(16))) float vx_am_lds[];
    int* __restrict__ lin = reinterpret_cast<int*>(vx_am_lds);                  // [LP]
    float* __restrict__ bias = vx_am_lds + LP;                                   // [Tsz] the head's bias column x log2(e)
    float* __restrict__ gwin = bias + ((A.Tsz + 3) & ~3);                        // [4 waves][4 lane groups][WIN] bias-gradient windows
    float* __restrict__ lse_s = gwin + 16 * WIN;                                  // [NR]  lse * log2(e)
    float* __restrict__ del_s = lse_s + NR;                                      // [NR]  delta in the units of dS
    float* __restrict__ dqw = del_s + NR;                                        // [4 waves][NR][C]
    uint32_t* __restrict__ trb = reinterpret_cast<uint32_t*>(dqw + 4 * NR * C);  // [4 waves][2][16 * TS]
    _Float16* __restrict__ rq = reinterpret_cast<_Float16*>(trb + 4 * 2 * 16 * TS);      // [NR][VX_BH_RS]: Q hi | Q lo | dO hi | dO lo | 0
    _Float16* __restrict__ tq = rq + NR * VX_BH_RS;                              // [2 (Q, dO)][16][VX_BH_TS]: rows 0..C-1 hi, C..2C-1 lo, rest 0
    float* __restrict__ red = reinterpret_cast<float*>(tq + 2 * 16 * VX_BH_TS);  // [16] block maxima, [16..19] the waves' window offsets
    int bx_, by_;
    vx_xcd_rows(bx_, by_, A.xcd & 2);         // (round 6) the blocks of a window on ONE XCD: they read the same Q / dO / K / V rows and keep bits
    const long win = by_;
    const int a = (int)((win / A.Nt) % A.heads);
    const long wrow = win * A.ML;
    const int qsi = bx_ % QS;
    const int kc = bx_ / QS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, qg = lane >> 4;
    // ---- this wave's keys
    const int kt = kc * 4 + wave;                             // key tile (of both modalities)
    const int kcol = 16 * kt + m;
    const bool kval = !RAG || kcol < A.l;                     // (RAG: this lane's key exists)
    const int kcc = RAG ? min(kcol, A.l - 1) : kcol;
    float kmax = 0.0f, vmax = 0.0f;
    vx_au4 kop[2], vop[2], kth, ktl;
    float kv[2][C], vv[2][C], t8[8];
    if constexpr (MF == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) t8[e] = 0.0f;
    }
    // every global load of the block's start is issued before the first wait: the key rows here, the first chunk's query rows below, then the LDS tables are built
    // (one exposed memory latency per block instead of three: 83 -> see DESIGN.md section 9.5)
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const long kr = wrow + (long)f * A.l + kcc;
#pragma unroll
        for (int c4 = 0; c4 < C / 4; ++c4) {
            float4 k4 = *reinterpret_cast<const float4*>(K + kr * C + 4 * c4), v4 = *reinterpret_cast<const float4*>(Vt + kr * C + 4 * c4);
            if (RAG && !kval) { k4 = make_float4(0.f, 0.f, 0.f, 0.f); v4 = make_float4(0.f, 0.f, 0.f, 0.f); }
            kv[f][4 * c4] = k4.x; kv[f][4 * c4 + 1] = k4.y; kv[f][4 * c4 + 2] = k4.z; kv[f][4 * c4 + 3] = k4.w;
            vv[f][4 * c4] = v4.x; vv[f][4 * c4 + 1] = v4.y; vv[f][4 * c4 + 2] = v4.z; vv[f][4 * c4 + 3] = v4.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {       // A of dQ^T: lane (row = channel m, slots 4 f + j <-> key 4 qg + j of tile f)
            const int kk = 16 * kt + 4 * qg + j;
            const float t_ = K[(wrow + (long)f * A.l + (RAG ? min(kk, A.l - 1) : kk)) * C + (m < C ? m : 0)];
            t8[4 * f + j] = (m < C && (!RAG || kk < A.l)) ? t_ : 0.0f;
        }
    }
    // ---- the chunk's query rows: threads 0..127 one Q row each, threads 128..255 one dO / O row each (loaded one chunk ahead)
    const int rr = threadIdx.x & 127;
    const int rf = rr / nq, rloc = rr - rf * nq;
    float xv[C], lse_r = 0.0f, del_r = 0.0f, omax = 0.0f;
    auto load_rows = [&](int qc) {
        const int tq_ = 64 * qc + rloc;
        const bool rv = (!RAG || tq_ < A.l) && rf < MF;      // (RAG: rows beyond the window's last token are staged as zeros; MF = 1: the second modality's rows too)
        const long grow = wrow + (long)(rf < MF ? rf : 0) * A.l + (RAG ? min(tq_, A.l - 1) : tq_);
        del_r = 0.0f; omax = 0.0f;
        if (threadIdx.x < 128) {
#pragma unroll
            for (int c4 = 0; c4 < C / 4; ++c4) {
                const float4 q4 = *reinterpret_cast<const float4*>(Q + grow * C + 4 * c4);
                xv[4 * c4] = q4.x; xv[4 * c4 + 1] = q4.y; xv[4 * c4 + 2] = q4.z; xv[4 * c4 + 3] = q4.w;
            }
        } else {
            lse_r = LSE[grow];
#pragma unroll
            for (int c4 = 0; c4 < C / 4; ++c4) {
                const float4 g4 = *reinterpret_cast<const float4*>(dO + grow * C + 4 * c4), o4 = *reinterpret_cast<const float4*>(O + grow * C + 4 * c4);
                xv[4 * c4] = g4.x; xv[4 * c4 + 1] = g4.y; xv[4 * c4 + 2] = g4.z; xv[4 * c4 + 3] = g4.w;
                del_r = fmaf(g4.x, o4.x, fmaf(g4.y, o4.y, fmaf(g4.z, o4.z, fmaf(g4.w, o4.w, del_r))));
                omax = fmaxf(omax, fmaxf(fmaxf(fabsf(o4.x), fabsf(o4.y)), fmaxf(fabsf(o4.z), fabsf(o4.w))));
            }
        }
        if ((RAG || MF == 1) && !rv) {
#pragma unroll
            for (int c = 0; c < C; ++c) xv[c] = 0.0f;
            lse_r = 0.0f; del_r = 0.0f; omax = 0.0f;
        }
    };
    load_rows(qsi * QCB);
    // ---- LDS tables (while the loads above travel)
    for (int tp = threadIdx.x; tp < LP; tp += 256) {
        const int t = RAG ? min(tp, A.l - 1) : tp;
        const int t2 = t % A.n[2], t1 = (t / A.n[2]) % A.n[1], t0 = t / (A.n[2] * A.n[1]);
        lin[tp] = (t0 * (2 * A.n[1] - 1) + t1) * (2 * A.n[2] - 1) + t2;
    }
    for (int e = threadIdx.x; e < 4 * NR * C; e += 256) dqw[e] = 0.0f;
    for (int e = threadIdx.x; e < 16 * WIN; e += 256) gwin[e] = 0.0f;
    for (int k0 = threadIdx.x; k0 < A.Tsz; k0 += 256 * 8) {           // (8 independent loads per thread in flight)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * 256; v[u] = table[(long)(k < A.Tsz ? k : 0) * A.heads + a]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * 256; if (k < A.Tsz) bias[k] = v[u] * LOG2E; }
    }
    {   // zero padding of the piece images (uint32 granules)
        uint32_t* z = reinterpret_cast<uint32_t*>(rq);
        for (int e = threadIdx.x; e < (NR * VX_BH_RS + 2 * 16 * VX_BH_TS) / 2; e += 256) z[e] = 0u;
    }
    {
#pragma unroll
        for (int f = 0; f < MF; ++f) {
#pragma unroll
            for (int c = 0; c < C; ++c) { kmax = fmaxf(kmax, fabsf(kv[f][c])); vmax = fmaxf(vmax, fabsf(vv[f][c])); }
        }
        kmax = vx_wave_max(kmax); vmax = vx_wave_max(vmax);
        if (lane == 0) { red[8 + wave] = kmax; red[12 + wave] = vmax; }
        __syncthreads();
        kmax = fmaxf(fmaxf(red[8], red[9]), fmaxf(red[10], red[11]));
        vmax = fmaxf(fmaxf(red[12], red[13]), fmaxf(red[14], red[15]));
        const float sk = ldexpf(1.0f, vx_a_exp(kmax, 10)), sv = ldexpf(1.0f, vx_a_exp(vmax, 5));
        // B of S / dP: lane (key m of tile f, group G) = the piece (G & 1) of K / V  [C = 4: groups 0, 1 hold hi | lo, groups 2, 3 nothing]
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            uint32_t kh[C / 2], kl[C / 2], vh[C / 2], vl[C / 2];
#pragma unroll
            for (int c = 0; c < C; c += 2) {
                vx_a_split2(kv[f][c] * sk, kv[f][c + 1] * sk, kh[c / 2], kl[c / 2]);
                vx_a_split2(vv[f][c] * sv, vv[f][c + 1] * sv, vh[c / 2], vl[c / 2]);
            }
            if constexpr (C == 8) {
                const bool lo_ = (qg & 1) != 0;
                kop[f] = (vx_au4){lo_ ? kl[0] : kh[0], lo_ ? kl[1] : kh[1], lo_ ? kl[2] : kh[2], lo_ ? kl[3] : kh[3]};
                vop[f] = (vx_au4){lo_ ? vl[0] : vh[0], lo_ ? vl[1] : vh[1], lo_ ? vl[2] : vh[2], lo_ ? vl[3] : vh[3]};
            } else {
                const bool on = qg < 2;
                kop[f] = on ? (vx_au4){kh[0], kh[1], kl[0], kl[1]} : (vx_au4){0u, 0u, 0u, 0u};
                vop[f] = on ? (vx_au4){vh[0], vh[1], vl[0], vl[1]} : (vx_au4){0u, 0u, 0u, 0u};
            }
        }
        uint32_t h[4], l[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) vx_a_split2(t8[2 * p] * sk, t8[2 * p + 1] * sk, h[p], l[p]);
        kth = (vx_au4){h[0], h[1], h[2], h[3]};
        ktl = (vx_au4){l[0], l[1], l[2], l[3]};
    }
    const int ek = vx_a_exp(kmax, 10), ev = vx_a_exp(vmax, 5);
    const float sv = ldexpf(1.0f, ev);
    uint32_t* __restrict__ tr = trb + wave * (2 * 16 * TS);
    float* __restrict__ dqm = dqw + wave * (NR * C);
    float* __restrict__ gw = gwin + (wave * 4 + qg) * WIN;                      // this lane group's window: its 16 lanes are 16 keys of ONE query -> 16 different bins
    const int lin_k = lin[kcol];
    int kmaxb, kmaxw;                                        // largest linear coordinate of the block's / this wave's keys
    {
        kmaxb = lin[min(16 * kc * 4 + lane, A.l - 1)]; kmaxw = lin_k;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { kmaxb = max(kmaxb, __shfl_xor(kmaxb, o, 64)); kmaxw = max(kmaxw, __shfl_xor(kmaxw, o, 64)); }
    }
    // offsets (halfs) of this lane group's pieces inside a row of rq: Q for S, dO for dP  (C = 4, groups 2 / 3: the row's zero padding)
    const int poffS = C == 8 ? ((qg >> 1) ? 8 : 0) : (qg == 0 ? 0 : (qg == 1 ? 8 : 32));
    const int poffP = (C == 4 && qg >= 2) ? 32 : 16 + poffS;
    float totk[2][4], totv[2][4];                             // dK / dV of this wave's keys in true units (rows still stacked hi | lo)
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) { totk[f][i] = 0.0f; totv[f][i] = 0.0f; }
    const int NW16 = (A.ML + 15) >> 4;
    const unsigned short* __restrict__ mbw = DROP ? mbits + win * NW16 * A.ML : nullptr;
    const float keepf = inv_keep;
    float* __restrict__ dtab_dst = dtable_rep + (long)((blockIdx.x + gridDim.x * blockIdx.y) % VX_DTABLE_REPLICAS) * A.Tsz * A.heads;
#pragma unroll 1
    for (int qc = qsi * QCB; qc < (qsi + 1) * QCB; ++qc) {
        const int q_lo = 4 * qc;
        const int mrow0 = 16 * q_lo + 4 * qg;                 // (+ g * l + 16 j): first of this lane's 4 query rows
        uint2 mk[2][2];
        auto load_bits = [&](int j) {
            if constexpr (DROP && !RAG) {
#pragma unroll
                for (int g = 0; g < MF; ++g)
#pragma unroll
                    for (int f = 0; f < MF; ++f)
                        mk[g][f] = *reinterpret_cast<const uint2*>(mbw + (long)(f * (A.l >> 4) + kt) * A.ML + g * A.l + mrow0 + 16 * j);
            }
            if constexpr (DROP && RAG) {          // the tile's 16 keys start at bit (f l + 16 kt) & 15 of word (f l + 16 kt) >> 4; the 4 query rows are 4 halfwords apart by one
#pragma unroll
                for (int g = 0; g < MF; ++g)
#pragma unroll
                    for (int f = 0; f < MF; ++f) {
                        const int k0 = f * A.l + min(16 * kt, A.l - 1);
                        const int w0 = k0 >> 4, w1 = min(w0 + 1, NW16 - 1), sh = k0 & 15;
                        unsigned b4[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = g * A.l + min(mrow0 + 16 * j + i, A.l - 1);
                            const unsigned lo = mbw[(long)w0 * A.ML + row], hi = mbw[(long)w1 * A.ML + row];
                            b4[i] = ((lo | (hi << 16)) >> sh) & 0xffffu;
                        }
                        mk[g][f] = make_uint2(b4[0] | (b4[1] << 16), b4[2] | (b4[3] << 16));
                    }
            }
        };
        load_bits(0);                                        // (the keep bits of the chunk's first step travel during the staging below)
        // ---- scales of the chunk: Q to < 2^10; dO to < 2^5 and such that |delta| < C 2^10 in the units of dS = 2^(ed + ev) (|dP| < C 2^10 by the scales of dO and V)
        float amax = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) amax = fmaxf(amax, fabsf(xv[c]));
        amax = vx_wave_max(amax);
        const float om = vx_wave_max(omax);
        if (lane == 0) { red[wave] = amax; red[4 + wave] = om; }
        __syncthreads();                                     // (also: the previous chunk's flush is complete)
        const float qmx = fmaxf(red[0], red[1]), domx = fmaxf(red[2], red[3]), omx = fmaxf(red[6], red[7]);
        const int eq = vx_a_exp(qmx, 10), ed = min(vx_a_exp(domx, 5), vx_a_exp(domx * omx * sv, 10));
        const float sq = ldexpf(1.0f, eq), sd = ldexpf(1.0f, ed);
        const float cS = A.scale * LOG2E * ldexpf(1.0f, -(eq + ek));
        {   // piece images of the row
            uint32_t hi[C / 2], lo[C / 2];
            const float sc = threadIdx.x < 128 ? sq : sd;
#pragma unroll
            for (int c = 0; c < C; c += 2) vx_a_split2(xv[c] * sc, xv[c + 1] * sc, hi[c / 2], lo[c / 2]);
            uint32_t* rrow = reinterpret_cast<uint32_t*>(rq + rr * VX_BH_RS) + (threadIdx.x < 128 ? 0 : 8);
            if constexpr (C == 8) {
                *reinterpret_cast<vx_au4*>(rrow) = (vx_au4){hi[0], hi[1], hi[2], hi[3]};
                *reinterpret_cast<vx_au4*>(rrow + 4) = (vx_au4){lo[0], lo[1], lo[2], lo[3]};
            } else {            // slots of a lane group: [piece | piece] against the key side's [hi | lo]
                *reinterpret_cast<vx_au4*>(rrow) = (vx_au4){hi[0], hi[1], hi[0], hi[1]};
                *reinterpret_cast<vx_au4*>(rrow + 4) = (vx_au4){lo[0], lo[1], lo[0], lo[1]};
            }
            unsigned short* tcol = reinterpret_cast<unsigned short*>(tq + (threadIdx.x < 128 ? 0 : 16 * VX_BH_TS) + rr);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint32_t h = hi[c / 2], l = lo[c / 2];
                tcol[c * VX_BH_TS] = (unsigned short)((c & 1) ? (h >> 16) : (h & 0xffffu));
                tcol[(C + c) * VX_BH_TS] = (unsigned short)((c & 1) ? (l >> 16) : (l & 0xffffu));
            }
            if (threadIdx.x >= 128) { lse_s[rr] = lse_r * LOG2E; del_s[rr] = del_r * sd * sv; }
        }
        // bin windows of the chunk (as vx_pwa_attn_bwd1_k): raw bin = lin_q - lin_k
        int qmin = lin[64 * qc + lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) qmin = min(qmin, __shfl_xor(qmin, o, 64));
        const int bbase = qmin - kmaxb, wbase = qmin - kmaxw;
        if (lane == 0) reinterpret_cast<int*>(red)[16 + wave] = wbase - bbase;
        if (qc + 1 < (qsi + 1) * QCB) load_rows(qc + 1);     // the next chunk's rows travel while this one is worked on
        __syncthreads();
        vx_f32x4 dk[2], dv[2];
#pragma unroll
        for (int f = 0; f < MF; ++f) { dk[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; dv[f] = (vx_f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll 1
        for (int j = 0; j < NTq; ++j) {
            const int qt = q_lo + j;
            const int4 lq = *reinterpret_cast<const int4*>(&lin[16 * qt + 4 * qg]);
            const int raw[4] = {lq.x - lin_k, lq.y - lin_k, lq.z - lin_k, lq.w - lin_k};
            float bs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bs[i] = bias[raw[i] + A.lin_cst];
            uint2 mkc[2][2];
#pragma unroll
            for (int g = 0; g < MF; ++g)
#pragma unroll
                for (int f = 0; f < MF; ++f) mkc[g][f] = mk[g][f];
            if (j + 1 < NTq) load_bits(j + 1);
            float dssum[4] = {0.f, 0.f, 0.f, 0.f};
            bool pv[4];                                      // (RAG) the pair (query row 4 qg + i of this step, this lane's key) exists
#pragma unroll
            for (int i = 0; i < 4; ++i) pv[i] = !RAG || (kval && 16 * qt + 4 * qg + i < A.l);
            uint32_t pmh[2][4], pml[2][4], dsh[2][4], dsl[2][4];          // [f][2 g + pair]: B operands of dV / dK (slots 4 g + i)
            if constexpr (MF == 1) {
#pragma unroll
                for (int e = 2; e < 4; ++e) { pmh[0][e] = 0u; pml[0][e] = 0u; dsh[0][e] = 0u; dsl[0][e] = 0u; }
            }
#pragma unroll
            for (int g = 0; g < MF; ++g) {
                const _Float16* rrow = rq + (g * nq + 16 * j + m) * VX_BH_RS;
                const vx_au4 aS = *reinterpret_cast<const vx_au4*>(rrow + poffS), aP = *reinterpret_cast<const vx_au4*>(rrow + poffP);
                const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[g * nq + 16 * j + 4 * qg]);
                const float4 d4 = *reinterpret_cast<const float4*>(&del_s[g * nq + 16 * j + 4 * qg]);
                const float bl[4] = {bs[0] - l4.x, bs[1] - l4.y, bs[2] - l4.z, bs[3] - l4.w}, del[4] = {d4.x, d4.y, d4.z, d4.w};
                vx_f32x4 sv_[2], dp[2];
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    sv_[f] = VX_MFMA_H(aS, kop[f], ((vx_f32x4){0.f, 0.f, 0.f, 0.f}));
                    dp[f] = VX_MFMA_H(aP, vop[f], ((vx_f32x4){0.f, 0.f, 0.f, 0.f}));
                }
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    float pm[4], ds[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float p = __builtin_amdgcn_exp2f(fmaf(sv_[f][i], cS, bl[i]));
                        if (RAG) p = pv[i] ? p : 0.0f;
                        float mkf = 1.0f;
                        if constexpr (DROP) {
                            const uint32_t w = (i < 2) ? mkc[g][f].x : mkc[g][f].y;
                            mkf = ((w >> (m + 16 * (i & 1))) & 1u) ? keepf : 0.0f;
                        }
                        pm[i] = p * mkf;
                        ds[i] = p * fmaf(dp[f][i], mkf, -del[i]);
                        dssum[i] += ds[i];
                    }
                    vx_a_split2(pm[0], pm[1], pmh[f][2 * g], pml[f][2 * g]);
                    vx_a_split2(pm[2], pm[3], pmh[f][2 * g + 1], pml[f][2 * g + 1]);
                    vx_a_split2(ds[0], ds[1], dsh[f][2 * g], dsl[f][2 * g]);
                    vx_a_split2(ds[2], ds[3], dsh[f][2 * g + 1], dsl[f][2 * g + 1]);
                }
                // dQ^T of query tile g: dS transposed through the wave's two patches (one per key tile), one dword = (hi | lo << 16) per element
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t h = dsh[f][2 * g + (i >> 1)], l = dsl[f][2 * g + (i >> 1)];
                        tr[f * (16 * TS) + (4 * qg + i) * TS + m] = (i & 1) ? __builtin_amdgcn_perm(l, h, 0x07060302u) : __builtin_amdgcn_perm(l, h, 0x05040100u);
                    }
                __builtin_amdgcn_wave_barrier();
                const vx_au4 r0 = *reinterpret_cast<const vx_au4*>(&tr[m * TS + 4 * qg]);
                const vx_au4 r1 = MF == 2 ? *reinterpret_cast<const vx_au4*>(&tr[16 * TS + m * TS + 4 * qg]) : (vx_au4){0u, 0u, 0u, 0u};
                __builtin_amdgcn_wave_barrier();
                const vx_au4 bh = {__builtin_amdgcn_perm(r0[1], r0[0], 0x05040100u), __builtin_amdgcn_perm(r0[3], r0[2], 0x05040100u),
                                   __builtin_amdgcn_perm(r1[1], r1[0], 0x05040100u), __builtin_amdgcn_perm(r1[3], r1[2], 0x05040100u)};
                const vx_au4 bl_ = {__builtin_amdgcn_perm(r0[1], r0[0], 0x07060302u), __builtin_amdgcn_perm(r0[3], r0[2], 0x07060302u),
                                    __builtin_amdgcn_perm(r1[1], r1[0], 0x07060302u), __builtin_amdgcn_perm(r1[3], r1[2], 0x07060302u)};
                vx_f32x4 dqT = VX_MFMA_H(kth, bh, ((vx_f32x4){0.f, 0.f, 0.f, 0.f}));
                dqT = VX_MFMA_H(ktl, bh, dqT);
                dqT = VX_MFMA_H(kth, bl_, dqT);
                if (4 * qg < C) {          // lane (q = m, channels 4 qg ..): this wave's dQ image  (LDS float atomics instead: 165 -> 220 us)
                    float4* dst = reinterpret_cast<float4*>(&dqm[(g * nq + 16 * j + m) * C + 4 * qg]);
                    float4 o4 = *dst;
                    o4.x += dqT[0]; o4.y += dqT[1]; o4.z += dqT[2]; o4.w += dqT[3];
                    *dst = o4;
                }
            }
            // dV^T += [dO hi; dO lo]^T (P*M),  dK^T += [Q hi; Q lo]^T dS: A = channel-major pieces of the step's 32 query rows (slots 4 g + i <-> row 4 qg + i of tile g)
            {
                const _Float16* tcol = tq + m * VX_BH_TS + 16 * j + 4 * qg;
                const uint2 q0 = *reinterpret_cast<const uint2*>(tcol), q1 = *reinterpret_cast<const uint2*>(tcol + nq);
                const uint2 o0 = *reinterpret_cast<const uint2*>(tcol + 16 * VX_BH_TS), o1 = *reinterpret_cast<const uint2*>(tcol + 16 * VX_BH_TS + nq);
                const vx_au4 aQ = {q0.x, q0.y, q1.x, q1.y}, aO = {o0.x, o0.y, o1.x, o1.y};
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    dv[f] = VX_MFMA_H(aO, ((vx_au4){pmh[f][0], pmh[f][1], pmh[f][2], pmh[f][3]}), dv[f]);
                    dv[f] = VX_MFMA_H(aO, ((vx_au4){pml[f][0], pml[f][1], pml[f][2], pml[f][3]}), dv[f]);
                    dk[f] = VX_MFMA_H(aQ, ((vx_au4){dsh[f][0], dsh[f][1], dsh[f][2], dsh[f][3]}), dk[f]);
                    dk[f] = VX_MFMA_H(aQ, ((vx_au4){dsl[f][0], dsl[f][1], dsl[f][2], dsl[f][3]}), dk[f]);
                }
            }
            // d(bias): plain read-add-write in the lane group's own window (one LDS round trip per step; a window shared by the wave needed four, group by group)
            // (the bins of a lane's 4 queries overlap those of its neighbours' -> one query at a time)
#pragma unroll
            for (int i = 0; i < 4; ++i) { if (kval) gw[raw[i] - wbase] += dssum[i]; __builtin_amdgcn_wave_barrier(); }      // (RAG: padding keys share the last token's coordinate -- their lanes would race with its lane for the bin)
        }
        // ---- the chunk's results: dK / dV into the totals (true units); the four dQ images and the bias-gradient windows leave (and are zeroed for the next chunk)
        const float fK = A.scale * ldexpf(1.0f, -(eq + ed + ev)), fV = ldexpf(1.0f, -ed), fQ = A.scale * ldexpf(1.0f, -(ek + ed + ev)), fB = ldexpf(1.0f, -(ed + ev));
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int i = 0; i < 4; ++i) { totk[f][i] = fmaf(dk[f][i], fK, totk[f][i]); totv[f][i] = fmaf(dv[f][i], fV, totv[f][i]); }
        __syncthreads();
        constexpr int img = NR * C;
        for (int e = threadIdx.x; e < img; e += 256) {
            const int c = e % C, r2 = e / C, f = r2 / nq, t = 16 * q_lo + (r2 - f * nq);
            float* dst = dQ + (wrow + (long)f * A.l + t) * C + c;
            const float v = ((dqw[e] + dqw[img + e]) + (dqw[2 * img + e] + dqw[3 * img + e])) * fQ;
            dqw[e] = 0.0f; dqw[img + e] = 0.0f; dqw[2 * img + e] = 0.0f; dqw[3 * img + e] = 0.0f;
            if ((RAG && t >= A.l) || f >= MF) continue;      // (a padding row)
            if (atomic_dq) atomicAdd(dst, v); else *dst = v;
        }
        {
            const int* wb_s = reinterpret_cast<const int*>(red) + 16;
            constexpr int NU = RAG ? 4 : 2;                  // 2 WIN bins of the block, 256 per pass (RAG: WIN <= 512)
            float gsum[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int x = threadIdx.x + 256 * u;
                float g = 0.0f;
                if (x < 2 * WIN) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int y = x - wb_s[w];
                        if (y >= 0 && y < WIN) g += (gwin[(4 * w) * WIN + y] + gwin[(4 * w + 1) * WIN + y]) + (gwin[(4 * w + 2) * WIN + y] + gwin[(4 * w + 3) * WIN + y]);
                    }
                }
                gsum[u] = g;
            }
            __syncthreads();                                 // every thread has read the windows: they can be zeroed
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int x = threadIdx.x + 256 * u;
                const int k = bbase + x + A.lin_cst;
                if (gsum[u] != 0.0f && k >= 0 && k < A.Tsz) atomicAdd(dtab_dst + (long)k * A.heads + a, gsum[u] * fB);
            }
            for (int e = threadIdx.x; e < 16 * WIN; e += 256) gwin[e] = 0.0f;
        }
    }
    // ---- dK / dV: rows 0..C-1 (hi piece of the A operand) + rows C..2C-1 (lo piece) = lanes l and l ^ (4 C)
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const long kr = wrow + (long)f * A.l + kcc;
        float k4[4], v4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k4[i] = totk[f][i] + __shfl_xor(totk[f][i], 4 * C, 64);
            v4[i] = totv[f][i] + __shfl_xor(totv[f][i], 4 * C, 64);
        }
        if (4 * qg < C && kval) {
            if (QS == 1) {
                *reinterpret_cast<float4*>(dK + kr * C + 4 * qg) = make_float4(k4[0], k4[1], k4[2], k4[3]);
                *reinterpret_cast<float4*>(dV + kr * C + 4 * qg) = make_float4(v4[0], v4[1], v4[2], v4[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) { atomicAdd(dK + kr * C + 4 * qg + i, k4[i]); atomicAdd(dV + kr * C + 4 * qg + i, v4[i]); }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- host
static bool vx_am_fill(VxAttnM& A, const VxPwaPlan* P, int B, int M, int cq) {
    A.BH = B * P->heads; A.heads = P->heads; A.Nt = P->Ntot; A.l = P->l; A.M = M; A.ML = M * P->l;
    A.n[0] = P->n[0]; A.n[1] = P->n[1]; A.n[2] = P->n[2];
    A.scale = 1.0f / sqrtf((float)cq);
    A.lin_cst = ((P->n[0] - 1) * (2 * P->n[1] - 1) + (P->n[1] - 1)) * (2 * P->n[2] - 1) + (P->n[2] - 1);
    A.Tsz = (2 * A.n[0] - 1) * (2 * A.n[1] - 1) * (2 * A.n[2] - 1);
    A.xcd = 3;
    return true;
}
static size_t vx_am_tab_floats(const VxAttnM& A) { return (size_t)((A.l + 3) & ~3) + (size_t)((A.Tsz + 3) & ~3); }
static size_t vx_am_lds_fwd(const VxAttnM& A, int cq, int cv) { return (vx_am_tab_floats(A) + (size_t)A.ML * cq + (size_t)A.ML * (cv + 2)) * 4; }
static size_t vx_am_lds_q(const VxAttnM& A, int cq, int cv) { return (vx_am_tab_floats(A) + (size_t)4 * ((A.Tsz + 3) & ~3) + (size_t)A.ML * (cq + cv)) * 4; }
static size_t vx_am_lds_kv(const VxAttnM& A, int cq, int cv) { return (vx_am_tab_floats(A) + (size_t)A.ML * (cq + cv + 2)) * 4; }

// Which passes take the MFMA kernels: bit 0 forward; bit 1 backward = the ONE-pass kernel vx_pwa_attn_bwd1_k where it is the faster one (below); bit 3
// (A/B, tests) the one-pass kernel for EVERY geometry it covers; bit 2 (A/B only) the older two-kernel MFMA backward where its geometry allows.  Default 3.
// Measured on one MI355X, B = 4, M = 2, p_drop 0.1 (tools/attn_bwd_probe.py, profiles/r03_attn_bwd_probe.txt), microseconds per backward:
//   128^3 (l = 64 / 512 / 64 / 64):   one-pass 133 / 332 / 33 / 44    VALU 122 / 304 / 32 / 43    two-kernel MFMA 313 / 778 / 43 / 51
//    96^3 (l = 27 / 216 / 27 / 27):   one-pass  74 / 111 / 21 / 26    VALU  82 / 119 / 36 / 46
// The one-pass kernel evaluates the soft-max side once per pair and runs all five GEMMs on MFMA, but its issue stream (~320 instructions per 16 x 16 tile:
// accumulator moves, the d(bias) windows, the dS transpose) is no shorter than the two VALU passes when the tokens fill the VALU kernels' 64-row units
// (l a multiple of 16); with the 27- / 216-token windows of the shipped 96^3 configurations the VALU units are ragged and it wins by 7 - 45 %.
// So: bit 1 selects it for l % 16 != 0, bit 3 everywhere.
static int vx_am_enabled = 3;
extern "C" int vx_pwa_attn_set_mfma(int mask) { vx_am_enabled = mask & 15; return 0; }

// bit mask of the passes this geometry can run on the MFMA kernels (0 = none), after the vx_pwa_attn_set_mfma selection
extern "C" int vx_pwa_attn_mfma_ok(const VxPwaPlan* P, int B, int M, int cq, int cv) {
    const int want = (vx_am_enabled & 1) | ((vx_am_enabled & 4) ? 2 : 0);      // bit 1 of the ANSWER = the two-kernel MFMA backward (A/B knob bit 2)
    if (!want || P == nullptr || B <= 0 || M <= 0) return 0;
    if (P->l % 64 != 0 || cq % 4 != 0 || cq > 16 || cv % 4 != 0 || cv > 32) return 0;
    if (!((cq == 4 && cv == 4) || (cq == 8 && cv == 8) || (cq == 8 && cv == 16) || (cq == 16 && cv == 32) || (cq == 16 && cv == 16) || (cq == 4 && cv == 8))) return 0;
    VxAttnM A;
    vx_am_fill(A, P, B, M, cq);
    const size_t cap = 150 * 1024;
    return (vx_am_lds_fwd(A, cq, cv) <= cap && vx_am_lds_q(A, cq, cv) <= cap && vx_am_lds_kv(A, cq, cv) <= cap) ? want : 0;
}

template <int A_, int B_> struct vx_am_pair { static constexpr int a = A_, b = B_; };
template <class F> static bool vx_am_dispatch(int cq, int cv, F&& f) {
#define VX_CASE(X, Y) if (cq == X && cv == Y) { f(vx_am_pair<X, Y>{}); return true; }
    VX_CASE(4, 4) VX_CASE(8, 8) VX_CASE(8, 16) VX_CASE(16, 32) VX_CASE(16, 16) VX_CASE(4, 8)
#undef VX_CASE
    return false;
}
template <class K> static void vx_am_attr(K kernel) { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }

// same contracts as vx_pwa_attn_fwd / vx_pwa_attn_bwd (include/veloxseg_hip.h); the caller checked vx_pwa_attn_mfma_ok and zeroed the replicas
int vx_pwa_attn_mfma_fwd(const float* Q, const float* K, const float* V, const float* table, float* O, float* LSE, unsigned short* mbits, const VxPwaPlan* plan, int B, int M,
                         int cq, int cv, VxDrop d, void* stream) {
    VxAttnM A;
    vx_am_fill(A, plan, B, M, cq);
    const dim3 grid(vx_cdiv(A.ML / 16, 8), (unsigned)((long)A.BH * A.Nt));
    const size_t shm = vx_am_lds_fwd(A, cq, cv);
    vx_am_dispatch(cq, cv, [&](auto pr) {
        constexpr int CQ = decltype(pr)::a, CV = decltype(pr)::b;
        static bool once = false;
        if (!once) { vx_am_attr(vx_pwa_attn_mfma_fwd_k<CQ, CV>); once = true; }
        vx_pwa_attn_mfma_fwd_k<CQ, CV><<<grid, dim3(512), shm, (hipStream_t)stream>>>(Q, K, V, table, O, LSE, A, d, mbits);
    });
    return 0;
}
int vx_pwa_attn_mfma_bwd(const float* Q, const float* K, const float* V, const float* table, const float* O, const float* LSE, const float* dO, float* dQ,
                         float* dK, float* dV, float* dtable, float* delta, float* rep, const VxPwaPlan* plan, int B, int M, int cq, int cv, VxDrop d,
                         void* stream) {
    VxAttnM A;
    vx_am_fill(A, plan, B, M, cq);
    const dim3 grid(vx_cdiv(A.ML / 16, 8), (unsigned)((long)A.BH * A.Nt));
    const size_t shm_q = vx_am_lds_q(A, cq, cv), shm_kv = vx_am_lds_kv(A, cq, cv);
    vx_am_dispatch(cq, cv, [&](auto pr) {
        constexpr int CQ = decltype(pr)::a, CV = decltype(pr)::b;
        static bool once = false;
        if (!once) { vx_am_attr(vx_pwa_attn_mfma_bwd_q_k<CQ, CV>); vx_am_attr(vx_pwa_attn_mfma_bwd_kv_k<CQ, CV>); once = true; }
        vx_pwa_attn_mfma_bwd_q_k<CQ, CV><<<grid, dim3(512), shm_q, (hipStream_t)stream>>>(Q, K, V, table, O, LSE, dO, dQ, delta, rep, A, d);
        vx_pwa_attn_mfma_bwd_kv_k<CQ, CV><<<grid, dim3(512), shm_kv, (hipStream_t)stream>>>(Q, K, V, table, LSE, delta, dO, dK, dV, rep, dtable, A, d);
    });
    return 0;
}

// ---- one-pass backward: geometry test + launch (contract of vx_pwa_attn_bwd without the fold; `rep` zeroed by the caller) -------------------------
struct VxB1Geo { int NT, waves_used, nbx, QS, NTq, win; size_t shm; };
// largest spread of the linear coordinate over `ntok` consecutive tokens starting at a multiple of `step` (tokens beyond l repeat the last one)
static int vx_b1_span(const VxAttnM& A, int ntok, int step) {
    int worst = 0;
    for (int t0 = 0; t0 < A.l; t0 += step) {
        int lo = 1 << 30, hi = -(1 << 30);
        for (int t = t0; t < t0 + ntok; ++t) {
            const int tc = t < A.l ? t : A.l - 1;
            const int t2 = tc % A.n[2], t1 = (tc / A.n[2]) % A.n[1], tz = tc / (A.n[2] * A.n[1]);
            const int v = (tz * (2 * A.n[1] - 1) + t1) * (2 * A.n[2] - 1) + t2;
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
        worst = (hi - lo) > worst ? (hi - lo) : worst;
    }
    return worst;
}
static VxB1Geo vx_b1_geo(const VxAttnM& A, int cq, int mf, bool few_windows = false) {
    VxB1Geo g;
    g.NT = (A.l + 15) / 16;
    g.waves_used = g.NT < 4 ? g.NT : 4;
    g.nbx = (g.NT + g.waves_used - 1) / g.waves_used;
    g.NTq = g.NT < 4 ? g.NT : 4;                          // query tiles per block: short blocks balance the chip (72 windows of 1024 tokens: 8 x 8 blocks each)
    if (few_windows) g.NTq = 1;                           // a handful of windows (the coarse levels): one query tile per block, 4 x the blocks, dK / dV through float atomics
    while (g.NT % g.NTq) --g.NTq;
    g.QS = g.NT / g.NTq;
    // bias-gradient windows: bins of (NTq * 16 queries) x (16 keys) inside 256 values, x (64 keys) inside 512
    const int sq = vx_b1_span(A, g.NTq * 16, g.NTq * 16), sk16 = vx_b1_span(A, 16, 16), sk64 = vx_b1_span(A, 16 * g.waves_used, 16 * g.waves_used);
    g.win = (sq + sk16 + 1 <= VX_B1_WIN && sq + sk64 + 1 <= 2 * VX_B1_WIN) ? 1 : 0;
    const size_t lp = (size_t)g.NT * 16, nq = (size_t)g.NTq * 16, tpad = (size_t)((A.Tsz + 3) & ~3);
    g.shm = (lp + (g.win ? 2 * VX_B1_WIN + 4 * VX_B1_WIN : 2 * tpad) + 2 * mf * nq + 4 * mf * nq * cq + (size_t)4 * mf * 16 * 20) * sizeof(float);
    return g;
}
struct VxZeroMany { float4* p[4]; long n4[4]; };
__global__ void __launch_bounds__(256) vx_zero_many_k(VxZeroMany z) {
    float4* __restrict__ p = z.p[blockIdx.y];
    const long n = z.n4[blockIdx.y];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long i = ((long)blockIdx.x * 4 + u) * 256 + threadIdx.x;
        if (i < n) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// Where the one-pass kernel is the faster backward although the window length is a multiple of 16 (round 6, tools/attn_bwd_probe.py with VX_PROBE_M / VX_PROBE_B; the
// selection of rounds 3 - 5 was measured at M = 2, B = 4 only).  The VALU kernels work in units of 64 query rows of one window and are efficient when a window has
// many such units; microseconds per backward, one-pass / VALU:
//   BraTS (M = 1), 128^3, B = 2:   l = 64: 35 / 87 (level 1), 22 / 49 (level 3), 27 / 60 (level 4);   l = 512 (level 2): 82 / 75
//   Hecktor (M = 2, l = 32 / 256), B = 4:   l = 32: 75 / 81, 21 / 38, 27 / 48;   l = 256 (level 2): 124 / 103
//   M = 2, l = 64 (128^3 levels 3 / 4):   34 / 33, 44 / 44 -- unchanged (VALU)
// => one-pass for a single modality below 512 tokens.  (Hecktor's 32-token windows -- 64 rows per window at M = 2 -- are faster alone too, but the STEP is not: 1445 vs
// 1455 patches/s with them on the one-pass kernel, whose blocks hold more LDS beside the other lanes' kernels; BraTS 128^3: 730 -> 748 fp32, 780 -> 821 in the bf16 mode.)
static bool vx_b1_short(const VxAttnM& A) { return A.M == 1 && A.l < 512; }
static int g_b1_short = 1;
static int vx_b1_short_on() { return g_b1_short; }      // A/B: 0 = the selection of rounds 3 - 5
extern "C" int vx_pwa_attn_set_short(int on) { g_b1_short = on ? 1 : 0; return 0; }
// fewer than 64 blocks with four query tiles per block: split the queries.  M = 2 (A/B experiment): 44 -> 32 us alone at the 4^3 level, no change of the
// step (894 vs 895) -> off.  The short-window geometries above: 22 -> 20 us (level 3) and 27 -> 20 us (level 4) at M = 1 -> on.
static bool vx_b1_few(const VxAttnM& A) {
    const int NT = (A.l + 15) / 16;
    const bool use = vx_b1_short_on() && vx_b1_short(A) && A.l % 16 == 0;
    return use && NT >= 2 && (long)A.BH * A.Nt * ((NT + 3) / 4) * ((NT + 3) / 4) < 64;
}
extern "C" int vx_pwa_attn_bwd1_ok(const VxPwaPlan* P, int B, int M, int cq, int cv) {
    if (!(vx_am_enabled & 10) || (vx_am_enabled & 4) || P == nullptr || B <= 0 || M < 1 || M > 2) return 0;
    if (!((cq == 4 && cv == 4) || (cq == 8 && cv == 8) || (cq == 8 && cv == 16) || (cq == 16 && cv == 32) || (cq == 16 && cv == 16) || (cq == 4 && cv == 8))) return 0;
    VxAttnM A;
    vx_am_fill(A, P, B, M, cq);
    // (measured: see vx_am_enabled and vx_b1_short)
    const bool prefer = (vx_am_enabled & 8) || P->l % 16 != 0 || vx_b1_few(A) || (vx_b1_short_on() && vx_b1_short(A));
    if (!prefer) return 0;
    return vx_b1_geo(A, cq, M, vx_b1_few(A)).shm <= 80 * 1024 ? 1 : 0;
}
int vx_pwa_attn_bwd1(const float* Q, const float* K, const float* V, const float* table, const float* O, const float* LSE, const float* dO, float* dQ,
                     float* dK, float* dV, float* rep, const unsigned short* mbits, const VxPwaPlan* plan, int B, int M, int cq, int cv, VxDrop d, void* stream) {
    VxAttnM A;
    vx_am_fill(A, plan, B, M, cq);
    const long nwin = (long)A.BH * A.Nt;
    const VxB1Geo g = vx_b1_geo(A, cq, M, vx_b1_few(A));
    const dim3 grid((unsigned)(g.nbx * g.QS), (unsigned)nwin);
    const int atomic_dq = g.nbx > 1 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const long rows = nwin * A.ML;
    if (atomic_dq || g.QS > 1) {          // one zeroing launch for the atomically summed outputs
        VxZeroMany z = {};
        int nz = 0;
        if (atomic_dq) { z.p[nz] = reinterpret_cast<float4*>(dQ); z.n4[nz] = rows * cq / 4; ++nz; }
        if (g.QS > 1) { z.p[nz] = reinterpret_cast<float4*>(dK); z.n4[nz] = rows * cq / 4; ++nz; z.p[nz] = reinterpret_cast<float4*>(dV); z.n4[nz] = rows * cv / 4; ++nz; }
        long mx = 0;
        for (int i = 0; i < nz; ++i) mx = z.n4[i] > mx ? z.n4[i] : mx;
        vx_zero_many_k<<<dim3((unsigned)vx_cdiv(mx, 256 * 4), (unsigned)nz), dim3(256), 0, st>>>(z);
    }
    vx_am_dispatch(cq, cv, [&](auto pr) {
        constexpr int CQ = decltype(pr)::a, CV = decltype(pr)::b;
        const bool al = (A.l & 3) == 0;
#define VX_B1(MF_, AL_, WIN_)                                                                                                         \
        {                                                                                                                             \
            static bool once = false;                                                                                                 \
            if (!once) {          /* (the kernel also has 16 bytes of static LDS: 160 KB of dynamic LDS would be refused) */                      \
                if (hipFuncSetAttribute((const void*)vx_pwa_attn_bwd1_k<CQ, CV, MF_, AL_, WIN_>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) (void)hipGetLastError(); \
                once = true;                                                                                                          \
            }                                                                                                                         \
            vx_pwa_attn_bwd1_k<CQ, CV, MF_, AL_, WIN_><<<grid, dim3(256), g.shm, st>>>(Q, K, V, table, O, LSE, dO, dQ, dK, dV, rep, A, d, g.waves_used, atomic_dq, \
                                                                                      g.QS, g.NTq, mbits);                         \
        }
#define VX_B1W(MF_, AL_) { if (g.win) VX_B1(MF_, AL_, true) else VX_B1(MF_, AL_, false) }
        if (M == 1) { if (al) VX_B1W(1, true) else VX_B1W(1, false) }
        else { if (al) VX_B1W(2, true) else VX_B1W(2, false) }
#undef VX_B1W
#undef VX_B1
    });
    return 0;
}

// ---- one-pass backward on the f16 matrix pipe (vx_pwa_attn_bwd1h_k): 128^3 levels 1 / 2 (windows of 64 / 512 tokens, two modalities, head widths (4, 4) / (8, 8)).
// Knob (A/B, tests): vx_pwa_attn_set_f16_bwd(0) returns those geometries to the fp32 kernels.  With dropout on the kernel needs the forward's keep bits.
static int vx_am_f16_bwd = 1;
extern "C" int vx_pwa_attn_set_f16_bwd(int on) { vx_am_f16_bwd = on ? 1 : 0; return 0; }
static size_t vx_b1h_shm(int LP, int Tsz, int win, int c) {
    return ((size_t)LP + (size_t)((Tsz + 3) & ~3) + 16 * (size_t)win + 2 * 128 + (size_t)4 * 128 * c + 4 * 2 * 16 * 20 + 32) * sizeof(float) + ((size_t)128 * VX_BH_RS + 2 * 16 * VX_BH_TS) * 2;
}
static size_t vx_b1h_shm(const VxAttnM& A, int c) { return vx_b1h_shm(A.l, A.Tsz, VX_B1_WIN, c); }
// Ragged windows (l % 64 != 0: the shipped 96^3 / Hecktor geometries) on the same kernel, RAG instance: padded length and the lane groups' bin window (0: does not fit)
struct VxB1hRag { int LP, win; };
static int g_b1h_rag = 1;
extern "C" int vx_pwa_attn_set_f16_bwd_ragged(int on) { g_b1h_rag = on < 0 ? 0 : on; return 0; }      // A/B (tests, probes): ragged windows on the f16-pipe backward -- 0 off, 1 (default) where a window fills >= 3/4 of its 64-token chunks, 2 every ragged length
static VxB1hRag vx_b1h_rag(const VxAttnM& A, int c) {
    VxB1hRag r = {0, 0};
    if (!g_b1h_rag || A.l < 8) return r;
    const int LP = (A.l + 63) / 64 * 64;
    // (measured alone, B = 4, M = 2, tools/attn_bwd_probe.py, f16 ragged / fp32 one-pass: l = 216 80 / 108 us; l = 27 92 / 74, l = 32 89 / 72 -- a 64-token chunk that is
    //  half padding, two of the four key-tile waves idle, 24 halfword loads of keep bits per step: the short windows stay on the fp32 kernels.  1: every ragged length, tests)
    if (g_b1h_rag == 1 && A.l * 4 < LP * 3) return r;
    const int sq = vx_b1_span(A, 64, 64), sk16 = vx_b1_span(A, 16, 16), sk64 = vx_b1_span(A, 64, 64);
    int win = (sq + sk16 + 1 + 63) / 64 * 64;
    if (win < VX_B1_WIN) win = VX_B1_WIN;
    while (sq + sk64 + 1 > 2 * win) win += 64;
    if (win > 512 || vx_b1h_shm(LP, A.Tsz, win, c) > 80 * 1024) return r;
    r.LP = LP; r.win = win;
    return r;
}
static int g_b1h_m1 = 0;
extern "C" int vx_pwa_attn_set_f16_bwd_m1(int on) { g_b1h_m1 = on < 0 ? 0 : on; return 0; }
extern "C" int vx_pwa_attn_bwd1h_ok(const VxPwaPlan* P, int B, int M, int cq, int cv) {
    if (!vx_am_f16_bwd || !(vx_am_enabled & 2) || (vx_am_enabled & 4) || P == nullptr || B <= 0 || M < 1 || M > 2) return 0;
    if (!((cq == 4 && cv == 4) || (cq == 8 && cv == 8))) return 0;
    if (M == 1) {        // (round 6) one modality (BraTS): the MF = 1 instance, off by default (the fp32 kernels); vx_pwa_attn_set_f16_bwd_m1(1 | 2) selects it (A/B)
        if (!g_b1h_m1 || (g_b1h_m1 == 2 && P->l < 512)) return 0;
    }
    VxAttnM A;
    vx_am_fill(A, P, B, M, cq);
    if (P->l % 64 != 0) return vx_b1h_rag(A, cq).LP > 0 ? 1 : 0;
    const VxB1Geo g = vx_b1_geo(A, cq, M);
    return (g.win && g.waves_used == 4 && g.NTq == 4 && vx_b1h_shm(A, cq) <= 80 * 1024) ? 1 : 0;
}
int vx_pwa_attn_bwd1h(const float* Q, const float* K, const float* V, const float* table, const float* O, const float* LSE, const float* dO, float* dQ,
                      float* dK, float* dV, float* rep, const unsigned short* mbits, const VxPwaPlan* plan, int B, int M, int cq, int cv, VxDrop d, void* stream) {
    VxAttnM A;
    vx_am_fill(A, plan, B, M, cq);
    const VxB1Geo g = vx_b1_geo(A, cq, M);
    const long nwin = (long)A.BH * A.Nt;
    const bool rag = A.l % 64 != 0;
    const VxB1hRag rg = rag ? vx_b1h_rag(A, cq) : VxB1hRag{A.l, VX_B1_WIN};
    if (rag && rg.LP == 0) return -4;
    const int nchunk = rag ? rg.LP / 64 : g.NT / 4;       // key chunks = query chunks per window (4 tiles each)
    // query splits: as few as fill the chip (every split costs one more float atomic per dK / dV element): >= 4 blocks per CU
    int QS = 1;
    while (QS < nchunk && nwin * nchunk * QS < 4 * 256) QS *= 2;
    const dim3 grid((unsigned)(nchunk * QS), (unsigned)nwin);
    const int atomic_dq = nchunk > 1 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const long rows = nwin * A.ML;
    const bool drop = d.seed_ptr != nullptr && d.p > 0.0f;
    if (drop && mbits == nullptr) return -3;
    // dQ (several key chunks per window) and dK / dV (several query splits) are summed with float atomics: zeroed in ONE launch (three memsets were 12 us of
    // launch latency in front of a 120 us kernel)
    if (atomic_dq || QS > 1) {
        VxZeroMany z = {};
        int nz = 0;
        if (atomic_dq) { z.p[nz] = reinterpret_cast<float4*>(dQ); z.n4[nz] = rows * cq / 4; ++nz; }
        if (QS > 1) { z.p[nz] = reinterpret_cast<float4*>(dK); z.n4[nz] = rows * cq / 4; ++nz; z.p[nz] = reinterpret_cast<float4*>(dV); z.n4[nz] = rows * cv / 4; ++nz; }
        long mx = 0;
        for (int i = 0; i < nz; ++i) mx = z.n4[i] > mx ? z.n4[i] : mx;
        vx_zero_many_k<<<dim3((unsigned)vx_cdiv(mx, 256 * 4), (unsigned)nz), dim3(256), 0, st>>>(z);
    }
    const float inv_keep = drop ? vx_attn_keep_scale(d.p) : 1.0f;          // (the forward's 16-bit threshold: vx_common.h vx_attn_ctx)
    const size_t shm = vx_b1h_shm(rg.LP, A.Tsz, rg.win, cq);
#define VX_B1H(C_, D_, R_, M_)                                                                                                                    \
    {                                                                                                                                             \
        static bool once = false;                                                                                                                 \
        if (!once) {                                                                                                                              \
            if (hipFuncSetAttribute((const void*)vx_pwa_attn_bwd1h_k<C_, C_, D_, R_, M_>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) (void)hipGetLastError(); \
            once = true;                                                                                                                          \
        }                                                                                                                                         \
        vx_pwa_attn_bwd1h_k<C_, C_, D_, R_, M_><<<grid, dim3(256), shm, st>>>(Q, K, V, table, O, LSE, dO, dQ, dK, dV, rep, A, inv_keep, atomic_dq, QS, nchunk / QS, mbits, rg.LP, rg.win); \
    }
#define VX_B1H_D(C_, R_, M_) { if (drop) VX_B1H(C_, true, R_, M_) else VX_B1H(C_, false, R_, M_) }
#define VX_B1H_C(R_, M_) { if (cq == 8) VX_B1H_D(8, R_, M_) else VX_B1H_D(4, R_, M_) }
    if (M == 1) { if (rag) VX_B1H_C(true, 1) else VX_B1H_C(false, 1) }
    else { if (rag) VX_B1H_C(true, 2) else VX_B1H_C(false, 2) }
#undef VX_B1H_C
#undef VX_B1H_D
#undef VX_B1H
    return 0;
}
