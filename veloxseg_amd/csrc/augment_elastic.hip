// Elastic deformation: a displacement field drawn and smoothed on the device, and the affine resampler with that displacement, for any number
// of volumes in ONE launch.  Layouts and the rules: include/veloxseg_hip.h.  Nothing here is an atomic, no workgroup waits for another, equal inputs give equal bits.
//   vx_elastic_noise   one thread = one Philox counter = four consecutive elements of a field; one launch for all planes
//   vx_elastic_smooth  three launches (W, H, D); a block stages its lines and their halo in LDS and every tap is an LDS read.  W pass: VX_ELASTIC_ROWS rows of up to
//                      VX_ELASTIC_TILE_W outputs (11 KB of LDS); H and D passes: VX_ELASTIC_STRIP consecutive x by up to VX_ELASTIC_TILE_LINE outputs along the axis, so
//                      global accesses run along W (as vx_edt_y_k's do) -- (min(n, TILE_LINE) + 2 MAX_TAIL) x STRIP floats of dynamic LDS, 28 KB at n = 128, 44 KB at most.
//                      A block works on ONE plane, so the weights are block-uniform; a thread forms four outputs per tap, so a weight is read once for eight data reads.
//   vx_elastic_batch   vx_affine_k's block (4 x 8 x 8 threads, two voxels per thread, block-uniform record through scalar loads) with the displacement in front of the
//                      matrix; from the source coordinate on it is the device code of augment_affine.h.  The three field reads of a voxel are coalesced along W; those
//                      of both voxels of a thread are issued before the first coordinate is formed, so they and all corner gathers of the thread are in flight together.
#include "augment_affine.h"

struct VxElasticRecord {
    VxAffineRecord a;
    const float* field;
    float m;
    int unused;
};
static_assert(sizeof(VxElasticRecord) == VX_ELASTIC_RECORD_BYTES, "record layout drifted from the header");
struct VxElasticWeights {
    int tail;
    float w[VX_ELASTIC_MAX_TAIL + 1];
};
static_assert(sizeof(VxElasticWeights) == VX_ELASTIC_WEIGHT_BYTES, "weight record drifted from the header");

// ---- noise ------------------------------------------------------------------------------------------------------------------------------------------------------
// grid = fields x bpf blocks; thread q of a field draws counter q = elements 4q .. 4q + 3 of the field's 3 V (fewer in a last, partial field)
__global__ void __launch_bounds__(256) vx_elastic_noise_k(const unsigned long long* __restrict__ keys, float* __restrict__ out, int n_planes, long V, int bpf, int vec) {
    const int f = (int)(blockIdx.x / (unsigned)bpf);
    const long q = (long)(blockIdx.x % (unsigned)bpf) * 256 + threadIdx.x;
    const long n_el = (long)min(3, n_planes - 3 * f) * V;
    const long e0 = q * 4;
    if (e0 >= n_el) return;
    uint32_t r[4];
    vx_philox4((uint64_t)keys[f], VX_ELASTIC_STREAM, (uint64_t)q, r);
    float u[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) u[t] = (float)((int)(r[t] >> 8) - 8388608) * (1.0f / 8388608.0f);          // exact: an integer below 2^23 times a power of two
    float* p = out + (long)f * 3 * V + e0;
    if (vec && e0 + 4 <= n_el) {                                                                           // vec: every field starts on 16 bytes
        *reinterpret_cast<float4*>(p) = make_float4(u[0], u[1], u[2], u[3]);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (e0 + t < n_el) p[t] = u[t];
    }
}

extern "C" int vx_elastic_noise(const void* keys, int n_planes, long V, float* out, void* stream) {
    VX_REQUIRE(keys && out, "vx_elastic_noise: null pointer (keys %p, out %p)", keys, (void*)out);
    VX_REQUIRE((reinterpret_cast<uintptr_t>(keys) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "vx_elastic_noise: misaligned keys (8 bytes) or out (4 bytes)");
    VX_REQUIRE(n_planes > 0, "vx_elastic_noise: no planes (n_planes %d)", n_planes);
    VX_REQUIRE(V > 0, "vx_elastic_noise: non-positive plane size (V %ld)", V);
    if (V > 0x7fffffffL) VX_FAIL(-3, "vx_elastic_noise: a plane of %ld elements is not supported (below 2^31)", V);
    const long n_fields = (n_planes + 2) / 3, bpf = ((3 * V + 3) / 4 + 255) / 256;
    if (bpf * n_fields > 0x7fffffffL) VX_FAIL(-3, "vx_elastic_noise: %ld blocks per field x %ld fields exceed one grid", bpf, n_fields);
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (3 * V) % 4 == 0;
    vx_elastic_noise_k<<<dim3((unsigned)(bpf * n_fields)), dim3(256), 0, (hipStream_t)stream>>>(static_cast<const unsigned long long*>(keys), out, n_planes, V, (int)bpf, vec);
    VX_LAUNCH_CHECK("vx_elastic_noise");
    return 0;
}

// ---- smoothing --------------------------------------------------------------------------------------------------------------------------------------------------
// The rule of a pass, written once: p points at x_0 of a line staged in LDS with `tail` zeros or neighbours on either side, `step` apart.  y = w_0 x_0 + sum_k w_k
// (x_-k + x_+k), k ascending, the pair added FIRST, then one fma per tap (vx_blur_tap's operations); four lines at once share the weight read.
__device__ __forceinline__ void vx_el_taps4(const float* __restrict__ sw, int tail, const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ p2,
                                            const float* __restrict__ p3, int step, float (&y)[4]) {
    const float w0 = sw[0];
    y[0] = w0 * p0[0];
    y[1] = w0 * p1[0];
    y[2] = w0 * p2[0];
    y[3] = w0 * p3[0];
    for (int k = 1; k <= tail; ++k) {
        const float wk = sw[k];
        const int o = k * step;
        const float a0 = p0[-o] + p0[o], a1 = p1[-o] + p1[o], a2 = p2[-o] + p2[o], a3 = p3[-o] + p3[o];
        y[0] = fmaf(wk, a0, y[0]);
        y[1] = fmaf(wk, a1, y[1]);
        y[2] = fmaf(wk, a2, y[2]);
        y[3] = fmaf(wk, a3, y[3]);
    }
}

// W pass.  grid = planes x bpp, bpp = row groups x chunks; a block takes VX_ELASTIC_ROWS consecutive rows of ONE plane and one chunk of up to VX_ELASTIC_TILE_W outputs.
// Thread t: row t / 32, outputs x, x + 32, x + 64, x + 96 (+ 128 ...) of the chunk with x = t % 32: lanes read consecutive LDS words.
__global__ void __launch_bounds__(256) vx_elastic_smooth_w_k(const VxElasticWeights* __restrict__ wt, const float* __restrict__ in, float* __restrict__ out, int rows, int W,
                                                             long V, int chunks, int bpp) {
    __shared__ float sx[VX_ELASTIC_ROWS][VX_ELASTIC_TILE_W + 2 * VX_ELASTIC_MAX_TAIL];
    __shared__ float sw[VX_ELASTIC_MAX_TAIL + 1];
    const int p = (int)(blockIdx.x / (unsigned)bpp), b = (int)(blockIdx.x % (unsigned)bpp);
    const VxElasticWeights* __restrict__ Wt = wt + p / 3;
    const int tail = Wt->tail;
    if (tail < 0 || tail > VX_ELASTIC_MAX_TAIL) return;                                    // block-uniform: before the barrier
    const int rb = b / chunks, cb = b - rb * chunks;
    const int r0 = rb * VX_ELASTIC_ROWS, w0 = cb * VX_ELASTIC_TILE_W;
    const int nr = min(VX_ELASTIC_ROWS, rows - r0), cw = min(VX_ELASTIC_TILE_W, W - w0), span = cw + 2 * tail;
    const float* __restrict__ src = in + (long)p * V + (long)r0 * W;
    for (int i = (int)threadIdx.x; i < nr * span; i += 256) {
        const int r = i / span, j = i - r * span, w = w0 - tail + j;
        sx[r][j] = (w >= 0 && w < W) ? src[(long)r * W + w] : 0.0f;
    }
    if ((int)threadIdx.x <= tail) sw[threadIdx.x] = Wt->w[threadIdx.x];
    __syncthreads();
    const int r = (int)(threadIdx.x >> 5), x = (int)(threadIdx.x & 31);
    if (r >= nr) return;
    float* __restrict__ dst = out + (long)p * V + (long)(r0 + r) * W + w0;
    for (int xb = x; xb < cw; xb += 128) {
        const float* q = &sx[r][tail];
        float y[4];
        vx_el_taps4(sw, tail, q + min(xb, cw - 1), q + min(xb + 32, cw - 1), q + min(xb + 64, cw - 1), q + min(xb + 96, cw - 1), 1, y);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (xb + 32 * t < cw) dst[xb + 32 * t] = y[t];
    }
}

// H and D passes.  The axis has n elements `step` apart; `other` counts the lines' remaining coordinate (d for the H pass, h for the D pass), `ostride` apart.
// grid = planes x bpp, bpp = n_other x tiles x strips (strips fastest: neighbouring blocks touch neighbouring memory).  A block stages (tl + 2 tail) rows of
// VX_ELASTIC_STRIP consecutive x (zeros outside the plane and past W); thread t forms the outputs of column t % 32 at rows t / 32 + 8 j.
__global__ void __launch_bounds__(256) vx_elastic_smooth_line_k(const VxElasticWeights* __restrict__ wt, const float* __restrict__ in, float* __restrict__ out, int n, long step,
                                                                long ostride, int W, long V, int strips, int tiles, int bpp) {
    extern __shared__ float sl[];
    __shared__ float sw[VX_ELASTIC_MAX_TAIL + 1];
    const int p = (int)(blockIdx.x / (unsigned)bpp), b = (int)(blockIdx.x % (unsigned)bpp);
    const VxElasticWeights* __restrict__ Wt = wt + p / 3;
    const int tail = Wt->tail;
    if (tail < 0 || tail > VX_ELASTIC_MAX_TAIL) return;                                    // block-uniform: before the barrier
    const int s = b % strips, bt = b / strips, t = bt % tiles, o = bt / tiles;
    const int x0 = s * VX_ELASTIC_STRIP, xw = min(VX_ELASTIC_STRIP, W - x0), i0 = t * VX_ELASTIC_TILE_LINE, tl = min(VX_ELASTIC_TILE_LINE, n - i0), span = tl + 2 * tail;
    const long base = (long)p * V + (long)o * ostride + x0;
    const float* __restrict__ src = in + base;
    for (int i = (int)threadIdx.x; i < span * VX_ELASTIC_STRIP; i += 256) {
        const int row = i / VX_ELASTIC_STRIP, x = i % VX_ELASTIC_STRIP, a = i0 - tail + row;
        sl[i] = (x < xw && a >= 0 && a < n) ? src[(long)a * step + x] : 0.0f;
    }
    if ((int)threadIdx.x <= tail) sw[threadIdx.x] = Wt->w[threadIdx.x];
    __syncthreads();
    const int x = (int)(threadIdx.x & 31), ry = (int)(threadIdx.x >> 5);
    if (x >= xw) return;
    float* __restrict__ dst = out + base + (long)i0 * step + x;
    for (int rb = ry; rb < tl; rb += 32) {
        const float* q = sl + tail * VX_ELASTIC_STRIP + x;
        float y[4];
        vx_el_taps4(sw, tail, q + min(rb, tl - 1) * VX_ELASTIC_STRIP, q + min(rb + 8, tl - 1) * VX_ELASTIC_STRIP, q + min(rb + 16, tl - 1) * VX_ELASTIC_STRIP,
                    q + min(rb + 24, tl - 1) * VX_ELASTIC_STRIP, VX_ELASTIC_STRIP, y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rb + 8 * j < tl) dst[(long)(rb + 8 * j) * step] = y[j];
    }
}

// every check of the two entries below, then the launch of ONE pass
static int vx_elastic_pass(const char* who, const void* weights, int n_planes, const float* in, float* out, int axis, int D, int H, int W, void* stream) {
    VX_REQUIRE(weights && in && out, "%s: null pointer (weights %p, planes %p, result %p)", who, weights, (const void*)in, (void*)out);
    VX_REQUIRE((reinterpret_cast<uintptr_t>(weights) & 7) == 0 && (reinterpret_cast<uintptr_t>(in) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
               "%s: misaligned table (8 bytes) or planes / result (4 bytes)", who);
    VX_REQUIRE(n_planes > 0, "%s: no planes (n_planes %d)", who, n_planes);
    VX_REQUIRE(D > 0 && H > 0 && W > 0, "%s: non-positive extent (D %d, H %d, W %d)", who, D, H, W);
    VX_REQUIRE(axis >= 0 && axis <= 2, "%s: axis %d (0 = D, 1 = H, 2 = W)", who, axis);
    const long V = (long)D * H * W;
    if (V > 0x7fffffffL) VX_FAIL(-3, "%s: a plane of %d x %d x %d voxels is not supported (below 2^31)", who, D, H, W);
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)n_planes * (uintptr_t)V * 4;
        VX_REQUIRE(a + bytes <= b || b + bytes <= a, "%s: planes and result overlap: a pass goes from one to the other", who);
    }
    const long rows = (long)D * H, chunks = (W + VX_ELASTIC_TILE_W - 1) / VX_ELASTIC_TILE_W, strips = (W + VX_ELASTIC_STRIP - 1) / VX_ELASTIC_STRIP;
    const int n = axis == 1 ? H : D;
    const long tiles = (n + VX_ELASTIC_TILE_LINE - 1) / VX_ELASTIC_TILE_LINE;
    const long bpp = axis == 2 ? ((rows + VX_ELASTIC_ROWS - 1) / VX_ELASTIC_ROWS) * chunks : (long)(axis == 1 ? D : H) * tiles * strips;
    if (bpp * n_planes > 0x7fffffffL) VX_FAIL(-3, "%s: %ld blocks per plane x %d planes exceed one grid", who, bpp, n_planes);
    hipStream_t st = (hipStream_t)stream;
    const VxElasticWeights* wt = static_cast<const VxElasticWeights*>(weights);
    const dim3 grid((unsigned)(bpp * n_planes)), blk(256);
    if (axis == 2) {
        vx_elastic_smooth_w_k<<<grid, blk, 0, st>>>(wt, in, out, (int)rows, W, V, (int)chunks, (int)bpp);
    } else {
        const size_t lds = (size_t)((n < VX_ELASTIC_TILE_LINE ? n : VX_ELASTIC_TILE_LINE) + 2 * VX_ELASTIC_MAX_TAIL) * VX_ELASTIC_STRIP * sizeof(float);
        if (axis == 1) vx_elastic_smooth_line_k<<<grid, blk, lds, st>>>(wt, in, out, H, (long)W, (long)H * W, W, V, (int)strips, (int)tiles, (int)bpp);
        else vx_elastic_smooth_line_k<<<grid, blk, lds, st>>>(wt, in, out, D, (long)H * W, (long)W, W, V, (int)strips, (int)tiles, (int)bpp);
    }
    VX_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int vx_elastic_smooth_pass(const void* weights, int n_planes, const float* planes, float* result, int axis, int D, int H, int W, void* stream) {
    return vx_elastic_pass("vx_elastic_smooth_pass", weights, n_planes, planes, result, axis, D, H, W, stream);
}

extern "C" int vx_elastic_smooth(const void* weights, int n_planes, float* planes, float* result, int D, int H, int W, void* stream) {
    // every check before the first launch: the W pass's are those of all three (the H and D grids are checked with it)
    for (int axis = 0; axis < 2; ++axis) {
        const long n = axis == 1 ? H : D, tiles = (n + VX_ELASTIC_TILE_LINE - 1) / VX_ELASTIC_TILE_LINE, strips = (W + VX_ELASTIC_STRIP - 1) / VX_ELASTIC_STRIP;
        if (D > 0 && H > 0 && W > 0 && n_planes > 0 && (long)(axis == 1 ? D : H) * tiles * strips * n_planes > 0x7fffffffL)
            VX_FAIL(-3, "vx_elastic_smooth: the blocks of the %s pass x %d planes exceed one grid", axis == 1 ? "H" : "D", n_planes);
    }
    int rc = vx_elastic_pass("vx_elastic_smooth", weights, n_planes, planes, result, 2, D, H, W, stream);
    if (rc == 0) rc = vx_elastic_pass("vx_elastic_smooth", weights, n_planes, result, planes, 1, D, H, W, stream);
    if (rc == 0) rc = vx_elastic_pass("vx_elastic_smooth", weights, n_planes, planes, result, 0, D, H, W, stream);
    return rc;
}

// ---- the resampler with a displacement --------------------------------------------------------------------------------------------------------------------------
// vx_aff_run with p' = p + m u in front of the matrix.  The field pointer is block-uniform: a record without a field takes p itself, the operations of vx_aff_run.
template <typename T, bool TRI, int BD, int VPT>
__device__ __forceinline__ void vx_el_run(const VxElasticRecord* __restrict__ E, int od0, int oh, int ow, int Do, int Ho, int Wo) {
    const VxAffineRecord* __restrict__ R = &E->a;
    const float m = R->pad == 0 ? 0.0f : 1.0f;                   // constant: one voxel of slack on either side, where both corners already read cval
    const float q1 = vx_aff_sub((float)oh, vx_aff_mul(0.5f, (float)(Ho - 1))), q2 = vx_aff_sub((float)ow, vx_aff_mul(0.5f, (float)(Wo - 1)));
    const VX_AFF_GLOBAL float* F = (const VX_AFF_GLOBAL float*)E->field;
    const float mag = E->m;
    const long V = (long)Do * Ho * Wo;
    float u[VPT][3];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {                              // the field reads of every voxel of the thread first: all in flight before a coordinate is formed
        const int od = min(od0 + v * BD, Do - 1);
        const unsigned at = (unsigned)(od * Ho + oh) * (unsigned)Wo + (unsigned)ow;
        u[v][0] = F ? F[at] : 0.0f;
        u[v][1] = F ? F[V + at] : 0.0f;
        u[v][2] = F ? F[2 * V + at] : 0.0f;
    }
    T val[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int od = min(od0 + v * BD, Do - 1);                // (a voxel past the end recomputes the last one and is not stored)
        float p0 = vx_aff_sub((float)od, vx_aff_mul(0.5f, (float)(Do - 1))), p1 = q1, p2 = q2;
        if (F) {
            p0 = vx_aff_add(p0, vx_aff_mul(mag, u[v][0]));
            p1 = vx_aff_add(p1, vx_aff_mul(mag, u[v][1]));
            p2 = vx_aff_add(p2, vx_aff_mul(mag, u[v][2]));
        }
        float sd = vx_aff_coord(R->A, R->c[0], p0, p1, p2), sh = vx_aff_coord(R->A + 3, R->c[1], p0, p1, p2), sw = vx_aff_coord(R->A + 6, R->c[2], p0, p1, p2);
        sd = fminf(fmaxf(sd, (float)R->lo[0] - m), (float)R->hi[0] + m);          // (a NaN coordinate comes out as lo - m: inside the range all the same)
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

// vx_affine_k's block: 256 threads = BD x BH x BW, lanes along W, VPT voxels per thread along D.  grid = n records x bricks of one volume.
template <int BD, int BH, int BW, int VPT>
__global__ void __launch_bounds__(256) vx_elastic_k(const VxElasticRecord* __restrict__ recs, int Do, int Ho, int Wo, int th, int tw, int bpr) {
    static_assert(BD * BH * BW == 256, "a block is 256 threads");
    const VxElasticRecord* __restrict__ E = recs + (blockIdx.x / (unsigned)bpr);
    const VxAffineRecord* __restrict__ R = &E->a;
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
    if (mode == 0) vx_el_run<float, true, BD, VPT>(E, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 1) vx_el_run<unsigned char, false, BD, VPT>(E, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 4) vx_el_run<int, false, BD, VPT>(E, od, oh, ow, Do, Ho, Wo);
    else if (ty_ == 8) vx_el_run<long long, false, BD, VPT>(E, od, oh, ow, Do, Ho, Wo);
    else vx_el_run<float, false, BD, VPT>(E, od, oh, ow, Do, Ho, Wo);
}

extern "C" int vx_elastic_batch(const void* records, int n_records, int Do, int Ho, int Wo, void* stream) {
    VX_REQUIRE(records, "vx_elastic_batch: null pointer (records)");
    VX_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0, "vx_elastic_batch: misaligned table (8 bytes)");
    VX_REQUIRE(n_records > 0, "vx_elastic_batch: no records (n_records %d)", n_records);
    VX_REQUIRE(Do > 0 && Ho > 0 && Wo > 0, "vx_elastic_batch: non-positive output extent (Do %d, Ho %d, Wo %d)", Do, Ho, Wo);
    if ((long)Do * Ho * Wo > 0x7fffffffL) VX_FAIL(-3, "vx_elastic_batch: an output volume of %d x %d x %d voxels is not supported (below 2^31)", Do, Ho, Wo);
    constexpr int BD = 4, BH = 8, BW = 8, VPT = 2;
    const long td = (Do + BD * VPT - 1) / (BD * VPT), th = (Ho + BH - 1) / BH, tw = (Wo + BW - 1) / BW;
    const long bpr = td * th * tw;
    if (bpr * (long)n_records > 0x7fffffffL) VX_FAIL(-3, "vx_elastic_batch: %ld blocks per record x %d records exceed one grid", bpr, n_records);
    vx_elastic_k<BD, BH, BW, VPT><<<dim3((unsigned)(bpr * n_records)), dim3(256), 0, (hipStream_t)stream>>>(static_cast<const VxElasticRecord*>(records), Do, Ho, Wo, (int)th,
                                                                                                            (int)tw, (int)bpr);
    VX_LAUNCH_CHECK("vx_elastic_batch");
    return 0;
}
