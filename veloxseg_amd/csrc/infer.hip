// Sliding-window inference and label metrics for gfx950.
// Reference call sites: utils/inference_runtime.py:4-19 (monai sliding_window_inference, constant blending), utils/inference_brats.py:209-217
// (argmax + Dice), utils/metric/metrics.py:44-91 (metrics_tensor), utils/metric/metrics_brats.py:22-35 (Dice / cal_dice).
// All kernels are HBM-bound streaming passes: float4 rows where the window geometry allows, one pass over the volume each.
#include "vx_common.h"
#include "../../include/veloxseg_hip.h"

struct VxWin {
    int C, D, H, W;        // volume (one batch item): (C, D, H, W)
    int rd, rh, rw;        // window extent
    int z0, y0, x0;        // window origin inside the volume
};

// win[c, z, y, x] = vol[c, z0+z, y0+y, x0+x]
__global__ void __launch_bounds__(256) vx_sw_extract_k(const float* __restrict__ vol, float* __restrict__ win, VxWin P) {
    const long n = (long)P.C * P.rd * P.rh * P.rw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int x = (int)(i % P.rw);
        long t = i / P.rw;
        const int y = (int)(t % P.rh); t /= P.rh;
        const int z = (int)(t % P.rd);
        const int c = (int)(t / P.rd);
        win[i] = vol[(((long)c * P.D + P.z0 + z) * P.H + P.y0 + y) * P.W + P.x0 + x];
    }
}

// acc[c, z0+z, y0+y, x0+x] += weight * win[c, z, y, x]   (windows are added one launch after the other: the fp32 summation order is the
// window order, as in the reference loop)
__global__ void __launch_bounds__(256) vx_sw_accumulate_k(const float* __restrict__ win, float* __restrict__ acc, VxWin P, float weight) {
    const long n = (long)P.C * P.rd * P.rh * P.rw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int x = (int)(i % P.rw);
        long t = i / P.rw;
        const int y = (int)(t % P.rh); t /= P.rh;
        const int z = (int)(t % P.rd);
        const int c = (int)(t / P.rd);
        float* __restrict__ a = acc + (((long)c * P.D + P.z0 + z) * P.H + P.y0 + y) * P.W + P.x0 + x;
        *a += weight * win[i];
    }
}

// out[c, v] = acc[c, v] / (cz[z] * cy[y] * cx[x])  (may alias acc);  labels[v] = first arg-max over c of the normalised value
__global__ void __launch_bounds__(256) vx_sw_finalize_k(const float* acc, float* out, unsigned char* __restrict__ labels,
                                                        const float* __restrict__ cz, const float* __restrict__ cy, const float* __restrict__ cx,
                                                        int C, int D, int H, int W) {
    const long V = (long)D * H * W;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const int x = (int)(v % W);
        const int y = (int)((v / W) % H);
        const int z = (int)(v / ((long)W * H));
        const float cnt = (cz[z] * cy[y]) * cx[x];
        float best = -INFINITY;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            const float q = acc[(long)c * V + v] / cnt;
            if (out) out[(long)c * V + v] = q;
            if (q > best || (q != q && !(best != best))) { best = q; arg = c; }    // NaN ranks highest, first occurrence wins (aten)
        }
        if (labels) labels[v] = (unsigned char)arg;
    }
}

// ---- mirror test-time augmentation: the window movers (utils/inference_runtime.py, mirror_axes) -----------------------------------------------
// A mirror is a mask: bit a set = spatial axis a (0 = D, 1 = H, 2 = W) runs backwards inside the window, m_a(i) = r_a - 1 - i.  All three kernels are
// streaming passes indexed by their OUTPUT element, so stores are contiguous; a mirrored axis only changes where the rows (D, H) or the 16-byte groups of a row (W)
// are read from: the lanes of a wave still read one contiguous stretch of every row, backwards for W, and a W-mirrored group of four is the 16-byte load at the
// mirrored position with its lanes reversed.  V = 4: four voxels along x per thread (rw, W and every x0 multiples of 4, bases 16-byte aligned); V = 1 otherwise.
struct VxWinTab { int b[VX_SW_MAX_WINDOWS], z0[VX_SW_MAX_WINDOWS], y0[VX_SW_MAX_WINDOWS], x0[VX_SW_MAX_WINDOWS]; };       // batch item and origin of every window of a launch, by value

__device__ __forceinline__ float4 vx_rev4(float4 v, bool on) { return on ? make_float4(v.w, v.z, v.y, v.x) : v; }

// win[w, c, z, y, x] = vol[b_w, c, z0_w + m_z(z), y0_w + m_y(y), x0_w + m_x(x)];  blockIdx.y = w (the table is read with scalar loads)
template <int V>
__global__ void __launch_bounds__(256) vx_sw_extract_mirror_k(const float* __restrict__ vol, float* __restrict__ win, VxWin P, VxWinTab T, int mask) {
    const int w = blockIdx.y;
    const int rwv = P.rw / V;
    const long n = (long)P.C * P.rd * P.rh * rwv;
    const float* __restrict__ src = vol + ((((long)T.b[w] * P.C) * P.D + T.z0[w]) * P.H + T.y0[w]) * P.W + T.x0[w];
    float* __restrict__ dst = win + (long)w * n * V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int xg = (int)(i % rwv);
        long t = i / rwv;
        const int y = (int)(t % P.rh); t /= P.rh;
        const int z = (int)(t % P.rd);
        const int c = (int)(t / P.rd);
        const int zs = (mask & 1) ? P.rd - 1 - z : z, ys = (mask & 2) ? P.rh - 1 - y : y, xs = (mask & 4) ? P.rw - V - xg * V : xg * V;
        const long s = (((long)c * P.D + zs) * P.H + ys) * P.W + xs;
        if (V == 4) vx_st4(dst, i * 4, vx_rev4(vx_ld4(src, s), mask & 4));
        else dst[i] = src[s];
    }
}

// wsum[r, z, y, x] (= | +=) pred[r, m_z(z), m_y(y), m_x(x)] over r < rows (= windows * classes)
template <int V>
__global__ void __launch_bounds__(256) vx_sw_mirror_sum_k(const float* __restrict__ pred, float* __restrict__ wsum, long rows, int rd, int rh, int rw, int mask, int first) {
    const int rwv = rw / V;
    const long n = rows * rd * rh * rwv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int xg = (int)(i % rwv);
        long t = i / rwv;
        const int y = (int)(t % rh); t /= rh;
        const int z = (int)(t % rd);
        const long r = t / rd;
        const int zs = (mask & 1) ? rd - 1 - z : z, ys = (mask & 2) ? rh - 1 - y : y, xs = (mask & 4) ? rw - V - xg * V : xg * V;
        const long s = ((r * rd + zs) * rh + ys) * rw + xs;
        if (V == 4) {
            float4 v = vx_rev4(vx_ld4(pred, s), mask & 4);
            if (!first) { const float4 o = vx_ld4(wsum, i * 4); v = make_float4(__fadd_rn(o.x, v.x), __fadd_rn(o.y, v.y), __fadd_rn(o.z, v.z), __fadd_rn(o.w, v.w)); }
            vx_st4(wsum, i * 4, v);
        } else {
            wsum[i] = first ? pred[s] : __fadd_rn(wsum[i], pred[s]);
        }
    }
}

// acc[c, z0+z, y0+y, x0+x] += weight * (wsum[c, z, y, x] + pred[c, m_z(z), m_y(y), m_x(x)]): the last mirror's add of one window fused into its blending (one launch per
// window, in window order, like vx_sw_accumulate_k).  Three roundings per element, in this order: the sum, the product, the accumulation (no contraction).
template <int V>
__global__ void __launch_bounds__(256) vx_sw_mirror_accumulate_k(const float* __restrict__ pred, const float* __restrict__ wsum, float* __restrict__ acc, VxWin P, int mask, float weight) {
    const int rwv = P.rw / V;
    const long n = (long)P.C * P.rd * P.rh * rwv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int xg = (int)(i % rwv);
        long t = i / rwv;
        const int y = (int)(t % P.rh); t /= P.rh;
        const int z = (int)(t % P.rd);
        const int c = (int)(t / P.rd);
        const int zs = (mask & 1) ? P.rd - 1 - z : z, ys = (mask & 2) ? P.rh - 1 - y : y, xs = (mask & 4) ? P.rw - V - xg * V : xg * V;
        const long s = (((long)c * P.rd + zs) * P.rh + ys) * P.rw + xs;
        const long a = (((long)c * P.D + P.z0 + z) * P.H + P.y0 + y) * P.W + P.x0 + xg * V;
        if (V == 4) {
            const float4 v = vx_rev4(vx_ld4(pred, s), mask & 4), o = vx_ld4(wsum, i * 4), q = vx_ld4(acc, a);
            vx_st4(acc, a, make_float4(__fadd_rn(q.x, __fmul_rn(weight, __fadd_rn(o.x, v.x))), __fadd_rn(q.y, __fmul_rn(weight, __fadd_rn(o.y, v.y))),
                                       __fadd_rn(q.z, __fmul_rn(weight, __fadd_rn(o.z, v.z))), __fadd_rn(q.w, __fmul_rn(weight, __fadd_rn(o.w, v.w)))));
        } else {
            acc[a] = __fadd_rn(acc[a], __fmul_rn(weight, __fadd_rn(wsum[i], pred[s])));
        }
    }
}

// ---- Gaussian importance blending (utils/inference_runtime.py, blend="gaussian") -------------------------------------------
// The weight of a window voxel is w[z, y, x] = max((g[z] * g[rd + y]) * g[rd + rh + x], floor): three host-made axis tables behind one pointer and a clamp that makes
// w non-separable.  It is formed in registers from the tables (a few hundred floats, cache-resident), never stored as a volume; both products are rounded.
// The weights are not powers of two, so acc + w * p contracted into an fma is NOT the bits of the product followed by the sum.  This toolchain's __fmul_rn / __fadd_rn are
// the plain operators and are contracted like them (the section-21 kernels above only ever scale by a power of two, where the fma gives the same bits); vx_mul_rn /
// vx_add_rn (vx_common.h) are emitted under `fp contract(off)` and stay a v_mul_f32 and a v_add_f32.
__device__ __forceinline__ float vx_blend_w(float gzy, float gx, float floor) { return fmaxf(vx_mul_rn(gzy, gx), floor); }

// acc[c, z0+z, y0+y, x0+x] += w[z, y, x] * p,  p = pred[c, m_z(z), m_y(y), m_x(x)] (MIRROR false: wsum is not read) or weight * (wsum[c, z, y, x] + that) (MIRROR true):
// vx_sw_mirror_accumulate_k with the window weight in front.  Every operation rounds on its own, in this order: the sum, weight *, w *, the accumulation.
// blockIdx.y walks the C * rd planes of the window, so channel, z and g[z] are uniform (scalar registers) and a thread splits its index inside the (rh, rw / V) plane
// with one 32-bit division; the lanes of a wave cover consecutive x of a row, as in the kernels above.
template <int V, bool MIRROR>
__global__ void __launch_bounds__(256) vx_sw_blend_accumulate_k(const float* __restrict__ pred, const float* __restrict__ wsum, float* __restrict__ acc,
                                                                const float* __restrict__ g, float floor, VxWin P, int mask, float weight) {
    const int rwv = P.rw / V;
    const int plane = P.rh * rwv, planes = P.C * P.rd;
    const long pstride = (long)P.rh * P.rw;
    const float* __restrict__ gy = g + P.rd;
    const float* __restrict__ gx = gy + P.rh;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        const int c = p / P.rd, z = p - c * P.rd;
        const int zs = (mask & 1) ? P.rd - 1 - z : z;
        const float gz = g[z];
        const float* __restrict__ src = pred + ((long)c * P.rd + zs) * pstride;
        const float* __restrict__ sum = MIRROR ? wsum + (long)p * pstride : nullptr;
        float* __restrict__ dst = acc + (((long)c * P.D + P.z0 + z) * P.H + P.y0) * P.W + P.x0;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
            const int y = i / rwv, xg = i - y * rwv;
            const int ys = (mask & 2) ? P.rh - 1 - y : y, xs = (mask & 4) ? P.rw - V - xg * V : xg * V;
            const long s = (long)ys * P.rw + xs;
            const long a = (long)y * P.W + xg * V;
            const float gzy = vx_mul_rn(gz, gy[y]);
            if (V == 4) {
                float4 v = vx_rev4(vx_ld4(src, s), mask & 4);
                if (MIRROR) {
                    const float4 o = vx_ld4(sum, (long)i * 4);
                    v = make_float4(vx_mul_rn(weight, vx_add_rn(o.x, v.x)), vx_mul_rn(weight, vx_add_rn(o.y, v.y)), vx_mul_rn(weight, vx_add_rn(o.z, v.z)), vx_mul_rn(weight, vx_add_rn(o.w, v.w)));
                }
                const float4 q = vx_ld4(dst, a);
                const float* __restrict__ gq = gx + xg * 4;
                vx_st4(dst, a, make_float4(vx_add_rn(q.x, vx_mul_rn(vx_blend_w(gzy, gq[0], floor), v.x)), vx_add_rn(q.y, vx_mul_rn(vx_blend_w(gzy, gq[1], floor), v.y)),
                                           vx_add_rn(q.z, vx_mul_rn(vx_blend_w(gzy, gq[2], floor), v.z)), vx_add_rn(q.w, vx_mul_rn(vx_blend_w(gzy, gq[3], floor), v.w))));
            } else {
                float v = src[s];
                if (MIRROR) v = vx_mul_rn(weight, vx_add_rn(sum[i], v));
                dst[a] = vx_add_rn(dst[a], vx_mul_rn(vx_blend_w(gzy, gx[xg], floor), v));
            }
        }
    }
}

// What the normaliser of a volume geometry needs, made on the host per axis: for every coordinate the number of windows that cover it (tab: n_z[D] n_y[H] n_x[W]) and
// the axis-table values of those windows in ascending window start (gc: GZ[D][cz] GY[H][cy] GX[W][cx], GZ[z][j] = g_0[z - (j-th covering start)]; cz / cy / cx = the
// largest count of the axis, the row stride).
struct VxBlendGeom { int C, D, H, W, cz, cy, cx; };

// out[c, v] = acc[c, v] / cnt[v] (may alias acc), labels[v] = first arg-max as in vx_sw_finalize_k; cnt[v] = the sum of w over the windows that cover v, added one after the
// other from 0 in ascending window index (iz * ny + iy) * nx + ix -- z outermost, x innermost -- which is the order the windows were accumulated in.  One thread per
// voxel, no atomics, nothing shared between threads: the same bits every run.  blockIdx.y walks z (uniform: its count and table row sit in scalar registers), a thread
// splits its index inside the (H, W) plane with one 32-bit division.  A count outside 0 .. stride is clamped: a wrong table gives wrong numbers, never a read outside it.
__global__ void __launch_bounds__(256) vx_sw_blend_finalize_k(const float* acc, float* out, unsigned char* __restrict__ labels, const float* __restrict__ gc, float floor,
                                                              const int* __restrict__ tab, VxBlendGeom P) {
    const int plane = P.H * P.W;
    const long V = (long)P.D * plane;
    const int* __restrict__ tz = tab;
    const int* __restrict__ ty = tz + P.D;
    const int* __restrict__ tx = ty + P.H;
    const float* __restrict__ GZ = gc;
    const float* __restrict__ GY = GZ + (long)P.D * P.cz;
    const float* __restrict__ GX = GY + (long)P.H * P.cy;
    for (int z = blockIdx.y; z < P.D; z += gridDim.y) {
        const int nz = min(max(tz[z], 0), P.cz);
        const float* __restrict__ gz = GZ + (long)z * P.cz;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
            const int y = i / P.W, x = i - y * P.W;
            const int ny = min(max(ty[y], 0), P.cy), nx = min(max(tx[x], 0), P.cx);
            const float* __restrict__ gy = GY + (long)y * P.cy;
            const float* __restrict__ gx = GX + (long)x * P.cx;
            float cnt = 0.f;
            for (int jz = 0; jz < nz; ++jz)
                for (int jy = 0; jy < ny; ++jy) {
                    const float gzy = vx_mul_rn(gz[jz], gy[jy]);
                    for (int jx = 0; jx < nx; ++jx) cnt = vx_add_rn(cnt, vx_blend_w(gzy, gx[jx], floor));
                }
            const long v = (long)z * plane + i;
            float best = -INFINITY;
            int arg = 0;
            for (int c = 0; c < P.C; ++c) {
                const float q = acc[(long)c * V + v] / cnt;
                if (out) out[(long)c * V + v] = q;
                if (q > best || (q != q && !(best != best))) { best = q; arg = c; }    // NaN ranks highest, first occurrence wins (aten)
            }
            if (labels) labels[v] = (unsigned char)arg;
        }
    }
}

// labels[b, v] = argmax_c logits[b, c, v]  (uint8; first maximum)
__global__ void __launch_bounds__(256) vx_argmax_k(const float* __restrict__ logits, unsigned char* __restrict__ labels, int C, long V) {
    const long b = blockIdx.y;
    const float* __restrict__ p = logits + b * C * V;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        float best = p[v];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float q = p[(long)c * V + v];
            if (q > best || (q != q && !(best != best))) { best = q; arg = c; }
        }
        labels[b * V + v] = (unsigned char)arg;
    }
}

// conf[b, g, p] = #voxels of sample b with ground truth g and prediction p (labels < 0 count as class 0, labels >= NC as class NC-1); LDS histogram per block
template <typename TP, typename TG>
__global__ void __launch_bounds__(256) vx_confusion_k(const TP* __restrict__ pred, const TG* __restrict__ gt, unsigned long long* __restrict__ conf, long V, int NC) {
    __shared__ unsigned int h[64];
    const int b = blockIdx.y;
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const TP* __restrict__ p = pred + (long)b * V;
    const TG* __restrict__ g = gt + (long)b * V;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const TP pv = p[v];                       // clamped in the SOURCE width, narrowed after: an int64 label of 2^32 + 1 is class NC-1, not class 1
        const TG gv = g[v];
        const int pi = pv < (TP)0 ? 0 : (pv >= (TP)NC ? NC - 1 : (int)pv);
        const int gi = gv < (TG)0 ? 0 : (gv >= (TG)NC ? NC - 1 : (int)gv);
        atomicAdd(&h[gi * NC + pi], 1u);
    }
    __syncthreads();
    if (threadIdx.x < NC * NC && h[threadIdx.x]) atomicAdd(conf + (long)b * NC * NC + threadIdx.x, (unsigned long long)h[threadIdx.x]);
}

static int vx_win_check(const VxWin& P, const char* who) {
    if (P.C <= 0 || P.D <= 0 || P.H <= 0 || P.W <= 0 || P.rd <= 0 || P.rh <= 0 || P.rw <= 0) VX_FAIL(-1, "%s: non-positive extent", who);
    if (P.z0 < 0 || P.y0 < 0 || P.x0 < 0 || P.z0 + P.rd > P.D || P.y0 + P.rh > P.H || P.x0 + P.rw > P.W)
        VX_FAIL(-1, "%s: window (%d,%d,%d)+(%d,%d,%d) leaves the volume (%d,%d,%d)", who, P.z0, P.y0, P.x0, P.rd, P.rh, P.rw, P.D, P.H, P.W);
    return 0;
}
static inline int vx_grid_for(long n) { long g = (n + 255) / 256; return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g)); }

extern "C" int vx_sw_extract(const float* vol, float* win, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0, void* stream) {
    VxWin P{C, D, H, W, rd, rh, rw, z0, y0, x0};
    if (int e = vx_win_check(P, "vx_sw_extract")) return e;
    VX_REQUIRE(vol && win, "vx_sw_extract: null pointer");
    vx_sw_extract_k<<<dim3(vx_grid_for((long)C * rd * rh * rw)), dim3(256), 0, (hipStream_t)stream>>>(vol, win, P);
    VX_LAUNCH_CHECK("vx_sw_extract");
    return 0;
}

extern "C" int vx_sw_accumulate(const float* win, float* acc, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0, float weight, void* stream) {
    VxWin P{C, D, H, W, rd, rh, rw, z0, y0, x0};
    if (int e = vx_win_check(P, "vx_sw_accumulate")) return e;
    VX_REQUIRE(win && acc, "vx_sw_accumulate: null pointer");
    vx_sw_accumulate_k<<<dim3(vx_grid_for((long)C * rd * rh * rw)), dim3(256), 0, (hipStream_t)stream>>>(win, acc, P, weight);
    VX_LAUNCH_CHECK("vx_sw_accumulate");
    return 0;
}

extern "C" int vx_sw_finalize(const float* acc, float* out, unsigned char* labels, const float* cz, const float* cy, const float* cx,
                              int C, int D, int H, int W, void* stream) {
    VX_REQUIRE(acc && cz && cy && cx && (out || labels), "vx_sw_finalize: null pointer");
    VX_REQUIRE(C > 0 && C <= 256 && D > 0 && H > 0 && W > 0, "vx_sw_finalize: bad shape");
    vx_sw_finalize_k<<<dim3(vx_grid_for((long)D * H * W)), dim3(256), 0, (hipStream_t)stream>>>(acc, out, labels, cz, cy, cx, C, D, H, W);
    VX_LAUNCH_CHECK("vx_sw_finalize");
    return 0;
}

static inline bool vx_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// grid of a streaming pass over n work items (guide: ~8 blocks per CU, the rest by the grid-stride loop)
static inline int vx_stream_grid(long n, int rows = 1) { long g = (n + 255) / 256, cap = 2048 / rows; if (cap < 1) cap = 1; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }

extern "C" int vx_sw_extract_mirror(const float* vol, float* win, const int* table, int nwin, int mask, int B, int C, int D, int H, int W, int rd, int rh, int rw, void* stream) {
    VX_REQUIRE(mask >= 0 && mask <= 7, "vx_sw_extract_mirror: mirror mask %d outside 0..7", mask);
    VX_REQUIRE(nwin >= 1 && nwin <= VX_SW_MAX_WINDOWS, "vx_sw_extract_mirror: %d windows, the table holds 1..%d", nwin, VX_SW_MAX_WINDOWS);
    VX_REQUIRE(vol && win && table, "vx_sw_extract_mirror: null pointer");
    VX_REQUIRE(B > 0, "vx_sw_extract_mirror: non-positive batch");
    VxWinTab T{};
    bool v4 = rw % 4 == 0 && W % 4 == 0 && vx_al16(vol) && vx_al16(win);
    for (int k = 0; k < nwin; ++k) {
        T.b[k] = table[4 * k]; T.z0[k] = table[4 * k + 1]; T.y0[k] = table[4 * k + 2]; T.x0[k] = table[4 * k + 3];
        VX_REQUIRE(T.b[k] >= 0 && T.b[k] < B, "vx_sw_extract_mirror: window %d names batch item %d of %d", k, T.b[k], B);
        VxWin Pk{C, D, H, W, rd, rh, rw, T.z0[k], T.y0[k], T.x0[k]};
        if (int e = vx_win_check(Pk, "vx_sw_extract_mirror")) return e;
        v4 = v4 && T.x0[k] % 4 == 0;
    }
    VxWin P{C, D, H, W, rd, rh, rw, 0, 0, 0};
    const long n = (long)C * rd * rh * rw;
    if (v4) vx_sw_extract_mirror_k<4><<<dim3(vx_stream_grid(n / 4, nwin), nwin), dim3(256), 0, (hipStream_t)stream>>>(vol, win, P, T, mask);
    else vx_sw_extract_mirror_k<1><<<dim3(vx_stream_grid(n, nwin), nwin), dim3(256), 0, (hipStream_t)stream>>>(vol, win, P, T, mask);
    VX_LAUNCH_CHECK("vx_sw_extract_mirror");
    return 0;
}

extern "C" int vx_sw_mirror_sum(const float* pred, float* wsum, long rows, int rd, int rh, int rw, int mask, int first, void* stream) {
    VX_REQUIRE(mask >= 0 && mask <= 7, "vx_sw_mirror_sum: mirror mask %d outside 0..7", mask);
    VX_REQUIRE(rows > 0 && rd > 0 && rh > 0 && rw > 0, "vx_sw_mirror_sum: non-positive extent");
    VX_REQUIRE(pred && wsum && pred != wsum, "vx_sw_mirror_sum: null or aliased pointer");
    const long n = rows * rd * rh * rw;
    if (rw % 4 == 0 && vx_al16(pred) && vx_al16(wsum)) vx_sw_mirror_sum_k<4><<<dim3(vx_stream_grid(n / 4)), dim3(256), 0, (hipStream_t)stream>>>(pred, wsum, rows, rd, rh, rw, mask, first);
    else vx_sw_mirror_sum_k<1><<<dim3(vx_stream_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(pred, wsum, rows, rd, rh, rw, mask, first);
    VX_LAUNCH_CHECK("vx_sw_mirror_sum");
    return 0;
}

extern "C" int vx_sw_mirror_accumulate(const float* pred, const float* wsum, float* acc, int C, int D, int H, int W, int rd, int rh, int rw, int z0, int y0, int x0,
                                       int mask, float weight, void* stream) {
    VX_REQUIRE(mask >= 0 && mask <= 7, "vx_sw_mirror_accumulate: mirror mask %d outside 0..7", mask);
    VxWin P{C, D, H, W, rd, rh, rw, z0, y0, x0};
    if (int e = vx_win_check(P, "vx_sw_mirror_accumulate")) return e;
    VX_REQUIRE(pred && wsum && acc, "vx_sw_mirror_accumulate: null pointer");
    const long n = (long)C * rd * rh * rw;
    if (rw % 4 == 0 && W % 4 == 0 && x0 % 4 == 0 && vx_al16(pred) && vx_al16(wsum) && vx_al16(acc))
        vx_sw_mirror_accumulate_k<4><<<dim3(vx_stream_grid(n / 4)), dim3(256), 0, (hipStream_t)stream>>>(pred, wsum, acc, P, mask, weight);
    else vx_sw_mirror_accumulate_k<1><<<dim3(vx_stream_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(pred, wsum, acc, P, mask, weight);
    VX_LAUNCH_CHECK("vx_sw_mirror_accumulate");
    return 0;
}

// grid of the plane-walking kernels above: x over the 256-thread chunks of a plane (at most 16), y over the planes, about 2048 blocks in all, the rest by the stride
// loops; both extents are levelled so that every block takes the same number of turns (9 chunks: 9 blocks of one turn, not 8 of two)
static inline long vx_level(long n, long cap) { const long turns = (n + cap - 1) / cap; return (n + turns - 1) / turns; }
static inline dim3 vx_plane_grid(long plane, long planes) {
    const long chunks = plane > 256 ? (plane + 255) / 256 : 1;
    const long gx = vx_level(chunks, 16);
    const long gy = vx_level(planes < 1 ? 1 : planes, 2048 / gx);
    return dim3((unsigned)gx, (unsigned)gy);
}

extern "C" int vx_sw_blend_accumulate(const float* pred, const float* wsum, float* acc, const float* g, float floor, int C, int D, int H, int W, int rd, int rh, int rw,
                                      int z0, int y0, int x0, int mask, float weight, void* stream) {
    VX_REQUIRE(mask >= 0 && mask <= 7, "vx_sw_blend_accumulate: mirror mask %d outside 0..7", mask);
    VxWin P{C, D, H, W, rd, rh, rw, z0, y0, x0};
    if (int e = vx_win_check(P, "vx_sw_blend_accumulate")) return e;
    VX_REQUIRE(pred && acc && g, "vx_sw_blend_accumulate: null pointer");
    VX_REQUIRE(floor > 0.f, "vx_sw_blend_accumulate: the floor of the weights must be positive");
    VX_REQUIRE((long)rh * rw <= (1L << 30) && (long)C * rd <= (1L << 30), "vx_sw_blend_accumulate: a window of %d x %d planes of %d x %d is beyond the 32-bit plane index", C, rd, rh, rw);
    const bool v4 = rw % 4 == 0 && W % 4 == 0 && x0 % 4 == 0 && vx_al16(pred) && vx_al16(wsum) && vx_al16(acc);      // (a null wsum counts as aligned)
    const dim3 grid = vx_plane_grid((long)rh * (rw / (v4 ? 4 : 1)), (long)C * rd);
    hipStream_t s = (hipStream_t)stream;
    if (v4 && wsum) vx_sw_blend_accumulate_k<4, true><<<grid, dim3(256), 0, s>>>(pred, wsum, acc, g, floor, P, mask, weight);
    else if (v4) vx_sw_blend_accumulate_k<4, false><<<grid, dim3(256), 0, s>>>(pred, wsum, acc, g, floor, P, mask, weight);
    else if (wsum) vx_sw_blend_accumulate_k<1, true><<<grid, dim3(256), 0, s>>>(pred, wsum, acc, g, floor, P, mask, weight);
    else vx_sw_blend_accumulate_k<1, false><<<grid, dim3(256), 0, s>>>(pred, wsum, acc, g, floor, P, mask, weight);
    VX_LAUNCH_CHECK("vx_sw_blend_accumulate");
    return 0;
}

extern "C" int vx_sw_blend_finalize(const float* acc, float* out, unsigned char* labels, const float* gc, float floor, const int* tab, int cz, int cy, int cx,
                                    int C, int D, int H, int W, void* stream) {
    VX_REQUIRE(acc && gc && tab && (out || labels), "vx_sw_blend_finalize: null pointer");
    VX_REQUIRE(C > 0 && C <= 256 && D > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 30), "vx_sw_blend_finalize: bad shape");
    VX_REQUIRE(cz > 0 && cy > 0 && cx > 0 && cz <= D && cy <= H && cx <= W, "vx_sw_blend_finalize: covering-window counts (%d,%d,%d) outside 1..(%d,%d,%d)", cz, cy, cx, D, H, W);
    VX_REQUIRE(floor > 0.f, "vx_sw_blend_finalize: the floor of the weights must be positive");
    VxBlendGeom P{C, D, H, W, cz, cy, cx};
    vx_sw_blend_finalize_k<<<vx_plane_grid((long)H * W, D), dim3(256), 0, (hipStream_t)stream>>>(acc, out, labels, gc, floor, tab, P);
    VX_LAUNCH_CHECK("vx_sw_blend_finalize");
    return 0;
}

extern "C" int vx_argmax_channels(const float* logits, unsigned char* labels, int B, int C, long V, void* stream) {
    VX_REQUIRE(logits && labels && B > 0 && C > 0 && C <= 256 && V > 0, "vx_argmax_channels: bad arguments");
    vx_argmax_k<<<dim3(vx_grid_for(V), B), dim3(256), 0, (hipStream_t)stream>>>(logits, labels, C, V);
    VX_LAUNCH_CHECK("vx_argmax_channels");
    return 0;
}

// pred_bytes / gt_bytes: element size of the label tensors (1 = uint8, 4 = int32, 8 = int64)
extern "C" int vx_confusion(const void* pred, int pred_bytes, const void* gt, int gt_bytes, unsigned long long* conf, int B, long V, int NC, void* stream) {
    VX_REQUIRE(pred && gt && conf && B > 0 && V > 0, "vx_confusion: bad arguments");
    VX_REQUIRE(NC >= 2 && NC <= 8, "vx_confusion: 2..8 classes supported, got %d", NC);
    int g = vx_grid_for(V);
    if (g > 1024) g = 1024;
    const dim3 grid(g, B), blk(256);
    hipStream_t s = (hipStream_t)stream;
#define VX_CONF(TP, TG) vx_confusion_k<TP, TG><<<grid, blk, 0, s>>>((const TP*)pred, (const TG*)gt, conf, V, NC)
    if (pred_bytes == 1 && gt_bytes == 1) VX_CONF(unsigned char, unsigned char);
    else if (pred_bytes == 1 && gt_bytes == 8) VX_CONF(unsigned char, long long);
    else if (pred_bytes == 1 && gt_bytes == 4) VX_CONF(unsigned char, int);
    else if (pred_bytes == 8 && gt_bytes == 8) VX_CONF(long long, long long);
    else if (pred_bytes == 8 && gt_bytes == 1) VX_CONF(long long, unsigned char);
    else if (pred_bytes == 4 && gt_bytes == 4) VX_CONF(int, int);
    else VX_FAIL(-3, "vx_confusion: unsupported label widths %d / %d bytes", pred_bytes, gt_bytes);
#undef VX_CONF
    VX_LAUNCH_CHECK("vx_confusion");
    return 0;
}
