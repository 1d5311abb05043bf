// Exact Euclidean distance transform of a bit-packed site mask, and the gather that turns a distance map into surface distances.  The
// reference reaches these through medpy.metric.binary.hd95 (utils/metric/metrics.py: get_hausdorff, utils/metric/metrics_brats.py: HD95 / cal_hd95), i.e. through
// scipy.ndimage.distance_transform_edt on the host.  Contracts in include/veloxseg_hip.h.
//
// Definition (all fp64, every product and sum rounded on its own: this file is compiled with contraction off, no fma anywhere):
//     t_a(d) = fl(fl(d * s_a) * fl(d * s_a))                                 d = integer offset along axis a
//     sq[v]  = min over the sites s of fl(fl(t_z(dz) + t_y(dy)) + t_x(dx))
// t_a is monotone in |d| and a rounded add is monotone in each operand, so the minimum commutes with every step and three passes along the axes give the bits of
// the brute-force minimum: z (integer distance to the nearest site of the column, then t_z), y (min over y' of fl(P1(y') + t_y(y - y'))), x (the same on P2).
//
// How a y / x pass finds its minimum: an outward scan.  The voxel starts from its own value and looks at the offsets k = 1, 2, ... on both sides; every candidate at
// offset k is >= t(k) (its other operand is >= 0), and t grows with k, so the scan stops at the first k with t(k) >= best.  Nothing is decided by a divided
// intersection point: every comparison is between values of the definition.  The work per voxel is its distance along the line, in voxels; a line that holds no
// finite value is skipped (its voxels stay +inf).  The worst case, one site in a corner, is measured by tools/edt_probe.py.
//
// The map lives in the output buffer from the first pass on (the y and x passes work in place, a tile at a time through LDS), so there is no workspace.
#include "vx_common.h"
#include <math.h>

#pragma clang fp contract(off)

typedef unsigned long long vx_u64;

#define VX_EDT_MAX_EXTENT 2048       // the longest line of a pass.  A y tile is (H x strip of x) doubles in LDS, an x tile whole rows; neither holds more than VX_EDT_LDS_BYTES of values
#define VX_EDT_LDS_BYTES 65536       // the values of a tile; with the flags in front of them a workgroup takes at most 65 KB: two of the largest fit the 160 KB of a CU
#define VX_EDT_FLAGS 256             // ints in front of the values of a tile: "this column / row holds a finite value" (1 KB = 128 doubles)
#define VX_EDT_GRID_CAP 4096         // every kernel here is a grid-stride loop above this block count
#define VX_EDT_X_ELEMS 4096          // doubles of an x tile (32 KB) when a row is shorter than that: whole rows, at most VX_EDT_X_ROWS of them
#define VX_EDT_X_ROWS VX_EDT_FLAGS
#define VX_EDT_INF __builtin_inf()

__device__ __forceinline__ double vx_edt_term(int d, double s) {
    const double a = (double)d * s;
    return a * a;
}

// z pass.  One thread per column (y, x), columns flat so that a wave reads and writes 64 consecutive doubles of a plane whatever W is.  Down the column once for the
// nearest site at or after z, up once for the nearest at or before it.
__global__ void __launch_bounds__(256) vx_edt_z_k(const vx_u64* __restrict__ bits, vx_u64 inv, double* __restrict__ out, int D, int H, int W, int Wq, double sz) {
    const long HW = (long)H * W, zs = (long)H * Wq;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < HW; c += (long)gridDim.x * 256) {
        const unsigned y = (unsigned)c / (unsigned)W, x = (unsigned)c % (unsigned)W;
        const vx_u64* col = bits + (long)y * Wq + (x >> 6);
        const int sh = (int)(x & 63u);
        int next = -1;
#pragma unroll 4
        for (int z = D - 1; z >= 0; --z) {
            if (((col[z * zs] ^ inv) >> sh) & 1ull) next = z;
            out[z * HW + c] = next < 0 ? VX_EDT_INF : vx_edt_term(next - z, sz);
        }
        int prev = -1;
#pragma unroll 4
        for (int z = 0; z < D; ++z) {
            if (((col[z * zs] ^ inv) >> sh) & 1ull) prev = z;
            if (prev >= 0) {
                const double t = vx_edt_term(z - prev, sz);
                if (t < out[z * HW + c]) out[z * HW + c] = t;
            }
        }
    }
}

// the outward scan of element p of a line of n values that sit `stride` doubles apart in LDS (f points at element p)
__device__ __forceinline__ double vx_edt_scan(const double* f, int p, int n, int stride, double s) {
    double best = f[0];
    const int far = p > n - 1 - p ? p : n - 1 - p;
    for (int k = 1; k <= far; ++k) {
        const double tk = vx_edt_term(k, s);
        if (!(tk < best)) break;
        if (k <= p) {
            const double c = f[-k * stride] + tk;
            best = c < best ? c : best;
        }
        if (p + k < n) {
            const double c = f[k * stride] + tk;
            best = c < best ? c : best;
        }
    }
    return best;
}

// y pass, in place.  A tile is every y of one z and a strip of XS = 2^xs_log2 consecutive x, staged as f[y * XS + x]: global accesses run along x, and the 32 lanes of
// a half-wave read 32 consecutive doubles at every step of the scan (conflict-free for 8-byte reads).  any[x] = the column holds a finite value.
__global__ void __launch_bounds__(256) vx_edt_y_k(double* io, int H, int W, int xs_log2, int strips, long ntiles, double sy) {
    extern __shared__ double vx_edt_lds[];
    int* any = (int*)vx_edt_lds;
    double* f = vx_edt_lds + VX_EDT_FLAGS / 2;
    const int XS = 1 << xs_log2, n = H << xs_log2;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int z = (int)(tile / strips), x0 = (int)(tile % strips) << xs_log2;
        const int xw = W - x0 < XS ? W - x0 : XS;
        double* base = io + (long)z * H * W + x0;
        __syncthreads();          // the scans of the trip before are done with f and any
        if (threadIdx.x < 32) any[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const int y = i >> xs_log2, x = i & (XS - 1);
            double v = VX_EDT_INF;
            if (x < xw) {
                v = base[(long)y * W + x];
                if (v < VX_EDT_INF) any[x] = 1;          // (every writer stores the same value)
            }
            f[i] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const int y = i >> xs_log2, x = i & (XS - 1);
            if (x < xw && any[x]) base[(long)y * W + x] = vx_edt_scan(f + i, y, H, XS, sy);
        }
    }
}

// x pass, in place.  A tile is nr consecutive rows = nr * W consecutive doubles of the volume; any[r] = the row holds a finite value.
__global__ void __launch_bounds__(256) vx_edt_x_k(double* io, long rows, int W, int nr, long ntiles, double sx) {
    extern __shared__ double vx_edt_lds[];
    int* any = (int*)vx_edt_lds;
    double* f = vx_edt_lds + VX_EDT_FLAGS / 2;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long r0 = tile * nr;
        const int rn = rows - r0 < nr ? (int)(rows - r0) : nr, n = rn * W;
        double* base = io + r0 * W;
        __syncthreads();
        for (int r = threadIdx.x; r < rn; r += 256) any[r] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const double v = base[i];
            if (v < VX_EDT_INF) any[(unsigned)i / (unsigned)W] = 1;
            f[i] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const unsigned r = (unsigned)i / (unsigned)W;
            if (any[r]) base[i] = vx_edt_scan(f + i, (int)((unsigned)i - r * (unsigned)W), W, 1, sx);
        }
    }
}

__global__ void __launch_bounds__(256) vx_edt_sqrt_k(double* x, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] = __dsqrt_rn(x[i]);
}

// set bits of every row (the tail bits of its last word left out)
__global__ void __launch_bounds__(256) vx_edt_count_k(const vx_u64* __restrict__ bits, int* __restrict__ counts, long rows, int Wq, vx_u64 tail) {
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const vx_u64* w = bits + r * Wq;
        int c = 0;
        for (int q = 0; q < Wq - 1; ++q) c += __popcll(w[q]);
        counts[r] = c + __popcll(w[Wq - 1] & tail);
    }
}

// one thread per word: its first output slot is the row's offset plus the set bits of the words of the row in front of it (at most 31 words: W <= 2048)
__global__ void __launch_bounds__(256) vx_edt_gather_k(const double* __restrict__ values, const vx_u64* __restrict__ bits, const long long* __restrict__ offsets,
                                                       double* __restrict__ out, long nw, int W, int Wq, vx_u64 tail) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nw; i += (long)gridDim.x * 256) {
        const unsigned row = (unsigned)i / (unsigned)Wq;
        const int q = (int)((unsigned)i - row * (unsigned)Wq);
        vx_u64 w = bits[i];
        if (q == Wq - 1) w &= tail;
        if (!w) continue;
        long long o = offsets[row];
        for (int p = 0; p < q; ++p) o += __popcll(bits[i - q + p]);
        const double* src = values + (long)row * W + q * 64;
        while (w) {
            out[o++] = src[__builtin_ctzll(w)];
            w &= w - 1;
        }
    }
}

static inline int vx_edt_grid(long n) { return (int)(n > VX_EDT_GRID_CAP ? VX_EDT_GRID_CAP : (n < 1 ? 1 : n)); }
static inline int vx_edt_wq(int W) { return (W + 63) / 64; }
static inline vx_u64 vx_edt_tail(int W) { return (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull; }
static inline bool vx_edt_extents_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D <= VX_EDT_MAX_EXTENT && H <= VX_EDT_MAX_EXTENT && W <= VX_EDT_MAX_EXTENT && (long)D * H * W <= 0x7fffffffL;
}
static inline bool vx_edt_spacing_ok(double s) { return isfinite(s) && s > 0.0; }
#define VX_EDT_EXTENTS(name) \
    VX_REQUIRE(vx_edt_extents_ok(D, H, W), name ": bad sizes %d x %d x %d (each 1 .. %d, D * H * W <= 2^31 - 1)", D, H, W, VX_EDT_MAX_EXTENT)

// the launches; every argument was checked by the caller
static size_t vx_edt_lds_bytes(long values) { return (size_t)VX_EDT_FLAGS * 4 + (size_t)values * 8; }
static void vx_edt_launch_z(const vx_u64* bits, int invert, double* io, int D, int H, int W, double sz, hipStream_t st) {
    vx_edt_z_k<<<dim3(vx_edt_grid(((long)H * W + 255) / 256)), dim3(256), 0, st>>>(bits, invert ? ~0ull : 0ull, io, D, H, W, vx_edt_wq(W), sz);
}
// the widest strip of 32, 16 or 8 columns whose tile stays within 32 KB (H <= 512); a longer line takes 8 columns up to 64 KB (H <= 1024), then 4 (H <= 2048)
static int vx_edt_y_strip_log2(int H) {
    int lg = 5;
    while (lg > 3 && ((long)H << lg) * 8 > VX_EDT_LDS_BYTES / 2) --lg;
    while (lg > 2 && ((long)H << lg) * 8 > VX_EDT_LDS_BYTES) --lg;
    return lg;
}
// Flags and values of the largest y tiles (a line longer than 1008) take 65 KB, one more than a kernel may ask for by default.  The limit is a property of the kernel on
// the CURRENT device, so it is raised at every call that needs it, before anything is launched; false = it could not be raised (the error is cleared).
static bool vx_edt_y_ready(int H) {
    const size_t lds = vx_edt_lds_bytes((long)H << vx_edt_y_strip_log2(H));
    if (lds <= 65536 || hipFuncSetAttribute((const void*)vx_edt_y_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
static void vx_edt_launch_y(double* io, int D, int H, int W, double sy, hipStream_t st) {
    const int lg = vx_edt_y_strip_log2(H), strips = (W + (1 << lg) - 1) >> lg;
    const long ntiles = (long)D * strips;
    vx_edt_y_k<<<dim3(vx_edt_grid(ntiles)), dim3(256), vx_edt_lds_bytes((long)H << lg), st>>>(io, H, W, lg, strips, ntiles, sy);
}
static void vx_edt_launch_x(double* io, int D, int H, int W, double sx, hipStream_t st) {
    const long rows = (long)D * H;
    int nr = VX_EDT_X_ELEMS / W;
    nr = nr < 1 ? 1 : (nr > VX_EDT_X_ROWS ? VX_EDT_X_ROWS : nr);
    const long ntiles = (rows + nr - 1) / nr;
    vx_edt_x_k<<<dim3(vx_edt_grid(ntiles)), dim3(256), vx_edt_lds_bytes((long)nr * W), st>>>(io, rows, W, nr, ntiles, sx);
}

extern "C" int vx_edt_max_extent(void) { return VX_EDT_MAX_EXTENT; }
extern "C" int vx_edt_grid_cap(void) { return VX_EDT_GRID_CAP; }

extern "C" int vx_edt_pass(int axis, const unsigned long long* bits, int invert, double* io, int D, int H, int W, double spacing, void* stream) {
    VX_REQUIRE(axis >= 0 && axis <= 2, "vx_edt_pass: axis %d is none of 0 (z), 1 (y), 2 (x)", axis);
    VX_REQUIRE(io && (bits || axis != 0), "vx_edt_pass: null pointer");
    VX_REQUIRE(invert == 0 || invert == 1, "vx_edt_pass: invert %d is neither 0 nor 1", invert);
    VX_EDT_EXTENTS("vx_edt_pass");
    VX_REQUIRE(vx_edt_spacing_ok(spacing), "vx_edt_pass: spacing %g is not a finite number > 0", spacing);
    VX_REQUIRE(axis != 1 || vx_edt_y_ready(H), "vx_edt_pass: the LDS limit of the y pass could not be raised");
    if (axis == 0) vx_edt_launch_z(bits, invert, io, D, H, W, spacing, (hipStream_t)stream);
    else if (axis == 1) vx_edt_launch_y(io, D, H, W, spacing, (hipStream_t)stream);
    else vx_edt_launch_x(io, D, H, W, spacing, (hipStream_t)stream);
    VX_LAUNCH_CHECK("vx_edt_pass");
    return 0;
}

extern "C" int vx_edt_sq(const unsigned long long* bits, int invert, double* out_sq, int D, int H, int W, double sz, double sy, double sx, void* stream) {
    VX_REQUIRE(bits && out_sq, "vx_edt_sq: null pointer");
    VX_REQUIRE(invert == 0 || invert == 1, "vx_edt_sq: invert %d is neither 0 nor 1", invert);
    VX_EDT_EXTENTS("vx_edt_sq");
    VX_REQUIRE(vx_edt_spacing_ok(sz) && vx_edt_spacing_ok(sy) && vx_edt_spacing_ok(sx), "vx_edt_sq: spacing (%g, %g, %g): three finite numbers > 0 wanted", sz, sy, sx);
    VX_REQUIRE(vx_edt_y_ready(H), "vx_edt_sq: the LDS limit of the y pass could not be raised");
    hipStream_t st = (hipStream_t)stream;
    vx_edt_launch_z(bits, invert, out_sq, D, H, W, sz, st);
    vx_edt_launch_y(out_sq, D, H, W, sy, st);
    vx_edt_launch_x(out_sq, D, H, W, sx, st);
    VX_LAUNCH_CHECK("vx_edt_sq");
    return 0;
}

extern "C" int vx_edt_sqrt(double* x, long n, void* stream) {
    VX_REQUIRE(x, "vx_edt_sqrt: null pointer");
    VX_REQUIRE(n > 0 && n <= 0x7fffffffL, "vx_edt_sqrt: bad size %ld (1 .. 2^31 - 1 values)", n);
    vx_edt_sqrt_k<<<dim3(vx_edt_grid((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(x, n);
    VX_LAUNCH_CHECK("vx_edt_sqrt");
    return 0;
}

extern "C" int vx_bits_count(const unsigned long long* bits, int D, int H, int W, int* counts, void* stream) {
    VX_REQUIRE(bits && counts, "vx_bits_count: null pointer");
    VX_EDT_EXTENTS("vx_bits_count");
    const long rows = (long)D * H;
    vx_edt_count_k<<<dim3(vx_edt_grid((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(bits, counts, rows, vx_edt_wq(W), vx_edt_tail(W));
    VX_LAUNCH_CHECK("vx_bits_count");
    return 0;
}

extern "C" int vx_edt_gather(const double* values, const unsigned long long* bits, const long long* offsets, double* out, int D, int H, int W, void* stream) {
    VX_REQUIRE(values && bits && offsets && out, "vx_edt_gather: null pointer");
    VX_EDT_EXTENTS("vx_edt_gather");
    const int Wq = vx_edt_wq(W);
    const long nw = (long)D * H * Wq;
    vx_edt_gather_k<<<dim3(vx_edt_grid((nw + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(values, bits, offsets, out, nw, W, Wq, vx_edt_tail(W));
    VX_LAUNCH_CHECK("vx_edt_gather");
    return 0;
}
