// Binary mask morphology on bit-packed volumes and hole filling of label maps.  No counterpart in the reference; the semantics are those of
// scipy.ndimage (binary_dilation / binary_erosion / binary_fill_holes with generate_binary_structure(3, 1 | 2 | 3)).  Contracts in include/veloxseg_hip.h.
//
// Packed layout: unsigned long long bits[D * H * Wq], Wq = (W + 63) / 64; bit i of word q of row (z, y) is voxel x = 64 q + i.  The tail bits of a row's last word
// are zero in every output and ignored in every input (they are forced to the border value on read).
//
// One thread owns one word = 64 voxels along x.  Only ONE operator is written, the dilation: an erosion is the complement of the dilation of the complement with the
// border value flipped, so a word is read as `w ^ inv` (inv = all ones for an erosion), everything outside the volume reads `bfill` (all ones or zero) and the result
// is stored as `r ^ inv`.  The x neighbours of a word are the word shifted by one with the carry bits of the words left and right of it.
#include "vx_common.h"

typedef unsigned long long vx_u64;

#define VX_MO_GRID_CAP 4096          // every kernel here is a grid-stride loop above this block count
#define VX_MO_FUSED 1                // iterations per launch of the step kernel.  A fused form (a 4 x 8 x 8-word tile with a halo of 2 rows and one word staged in LDS, two
                                     // iterations there, one store) gave the same bits and was 1.2 - 1.3 x SLOWER than two chained launches on both probe volumes
                                     // (DESIGN.md section 31.4): it is not kept
#define VX_MO_PACK_U 8               // words per wave and trip of the pack kernel: eight loads in flight ahead of the ballots

// dilation along x of word c, l / r the words left and right of it
__device__ __forceinline__ vx_u64 vx_mo_row(vx_u64 l, vx_u64 c, vx_u64 r) { return c | (c << 1) | (l >> 63) | (c >> 1) | (r << 63); }

// one dilation step of the word at the origin of get(dz, dy, dq); connectivity 6 reads 7 words, 18 and 26 the 9 rows around it
template <typename F>
__device__ __forceinline__ vx_u64 vx_mo_dilate(F get, int conn) {
    vx_u64 out = vx_mo_row(get(0, 0, -1), get(0, 0, 0), get(0, 0, 1));
    if (conn == 6) return out | get(-1, 0, 0) | get(1, 0, 0) | get(0, -1, 0) | get(0, 1, 0);
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            if (dz == 0 && dy == 0) continue;
            if (dz != 0 && dy != 0 && conn == 18) out |= get(dz, dy, 0);          // two non-zero coordinates already: no x neighbours
            else out |= vx_mo_row(get(dz, dy, -1), get(dz, dy, 0), get(dz, dy, 1));
        }
    return out;
}

// a word of the volume as the dilation sees it: complemented for an erosion, the border value outside the volume and in the tail bits
__device__ __forceinline__ vx_u64 vx_mo_fetch(const vx_u64* __restrict__ in, int z, int y, int q, int D, int H, int Wq, vx_u64 tail, vx_u64 inv, vx_u64 bfill) {
    if (z < 0 || z >= D || y < 0 || y >= H || q < 0 || q >= Wq) return bfill;
    vx_u64 w = in[((long)z * H + y) * Wq + q] ^ inv;
    if (q == Wq - 1) w = (w & tail) | (bfill & ~tail);
    return w;
}

// Flat indices (voxels, words) are below 2^31 (the entry points check the extents), so they are split into coordinates with 32-bit divisions; addresses are formed
// in `long`.
// one iteration, global memory to global memory.  boundary = 1: out = in & ~step(in) (the caller asks for an erosion with border value 0)
__global__ void __launch_bounds__(256) vx_mo_step_k(const vx_u64* __restrict__ in, vx_u64* __restrict__ out, int D, int H, int Wq, vx_u64 tail, vx_u64 inv, vx_u64 bfill,
                                                    int conn, int boundary) {
    const long nw = (long)D * H * Wq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nw; i += (long)gridDim.x * 256) {
        const unsigned u = (unsigned)i, rowi = u / (unsigned)Wq;
        const int q = (int)(u % (unsigned)Wq), y = (int)(rowi % (unsigned)H), z = (int)(rowi / (unsigned)H);
        vx_u64 r = vx_mo_dilate([&](int dz, int dy, int dq) { return vx_mo_fetch(in, z + dz, y + dy, q + dq, D, H, Wq, tail, inv, bfill); }, conn) ^ inv;
        if (boundary) r = in[i] & ~r;
        if (q == Wq - 1) r &= tail;
        out[i] = r;
    }
}

// ---- the ball: a structuring element given as a compact list of rows (dz, dy, hw), each the interval |dx| <= hw ------------------------------
#define VX_MO_BALL_ROWS 4096         // records one call takes: the list lives in LDS, 16 KB

// OR over k = 0 .. n of the 128-bit value (hi : lo) >> k, its low word; 1 <= n <= 63.  By doubling: after the loop acc holds the shifts 0 .. s - 1, s the largest power
// of two <= n + 1, and one more shift by n + 1 - s (< s) covers the rest.  Every shift count is in 1 .. 63.  A shift of the pair by at most 63 in total moves nothing
// above bit 126 into the low word, so the zeros that enter hi from above never reach it.
__device__ __forceinline__ vx_u64 vx_mo_spread_down(vx_u64 hi, vx_u64 lo, int n) {
    const int m = n + 1;
    int s = 1;
    for (; 2 * s <= m; s *= 2) {
        lo |= (lo >> s) | (hi << (64 - s));
        hi |= hi >> s;
    }
    const int t = m - s;
    if (t > 0) lo |= (lo >> t) | (hi << (64 - t));
    return lo;
}

// the mirror image: OR over k = 0 .. n of (hi : lo) << k, its HIGH word (hi = the word itself, lo = the word left of it)
__device__ __forceinline__ vx_u64 vx_mo_spread_up(vx_u64 hi, vx_u64 lo, int n) {
    const int m = n + 1;
    int s = 1;
    for (; 2 * s <= m; s *= 2) {
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
    }
    const int t = m - s;
    if (t > 0) hi |= (hi << t) | (lo >> (64 - t));
    return hi;
}

// One thread per output word, the record list staged once per block in LDS.  Every lane is on the same record, so hw and the trip counts of the spread are uniform.
// Nothing in a record is trusted: hw is masked to 0 .. 63, dz and dy are whatever their 8 bits say, and every fetch is bounds-checked (vx_mo_fetch).  Written as a
// dilation; an erosion is the complement form of vx_mo_step_k.  A word stops reading rows once every bit the caller asked for (the gate, or the whole word) is set:
// the gated form between two surfaces reads almost nothing.
__global__ void __launch_bounds__(256) vx_mo_ball_k(const vx_u64* __restrict__ in, const vx_u64* gate, vx_u64* __restrict__ out, int D, int H, int Wq, vx_u64 tail,
                                                    vx_u64 inv, vx_u64 bfill, const int* __restrict__ rows, int n_rows) {
    __shared__ int rec[VX_MO_BALL_ROWS];
    for (int k = threadIdx.x; k < n_rows; k += 256) rec[k] = rows[k];
    __syncthreads();
    const long nw = (long)D * H * Wq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nw; i += (long)gridDim.x * 256) {
        const unsigned u = (unsigned)i, rowi = u / (unsigned)Wq;
        const int q = (int)(u % (unsigned)Wq), y = (int)(rowi % (unsigned)H), z = (int)(rowi / (unsigned)H);
        vx_u64 want = q == Wq - 1 ? tail : ~0ull;
        if (gate) want &= gate[i];
        if (want == 0ull) { out[i] = 0ull; continue; }
        vx_u64 acc = 0ull;          // (of the complement for an erosion: a bit set here is a bit cleared in the result)
        for (int k = 0; k < n_rows; ++k) {
            const int r = rec[k], hw = (r >> 16) & 63;
            const int zz = z + (int)(signed char)(r & 0xff), yy = y + (int)(signed char)((r >> 8) & 0xff);
            const vx_u64 c = vx_mo_fetch(in, zz, yy, q, D, H, Wq, tail, inv, bfill);
            if (hw == 0) acc |= c;
            else {
                const vx_u64 l = vx_mo_fetch(in, zz, yy, q - 1, D, H, Wq, tail, inv, bfill), rr = vx_mo_fetch(in, zz, yy, q + 1, D, H, Wq, tail, inv, bfill);
                if ((l | c | rr) != 0ull) acc |= vx_mo_spread_down(rr, c, hw) | vx_mo_spread_up(c, l, hw);
            }
            if ((acc & want) == want) break;
        }
        out[i] = (acc ^ inv) & want;
    }
}

// one wave per word: its ballot over 64 consecutive voxels of a row IS the word.  A wave takes VX_MO_PACK_U consecutive words per trip.
template <typename T>
__global__ void __launch_bounds__(256) vx_mo_pack_k(const T* __restrict__ lab, T value, int match, vx_u64* __restrict__ bits, long rows, int W, int Wq) {
    const long nw = rows * Wq;
    const int lane = threadIdx.x & 63;
    for (long base = (long)blockIdx.x * (4 * VX_MO_PACK_U); base < nw; base += (long)gridDim.x * (4 * VX_MO_PACK_U)) {          // block-uniform trip count: the ballots see whole waves
        const long w0 = base + (threadIdx.x >> 6) * VX_MO_PACK_U;
        bool b[VX_MO_PACK_U];
#pragma unroll
        for (int k = 0; k < VX_MO_PACK_U; ++k) {
            b[k] = false;
            if (w0 + k < nw) {
                const unsigned wi = (unsigned)(w0 + k), row = wi / (unsigned)Wq;
                const int x = (int)(wi % (unsigned)Wq) * 64 + lane;
                if (x < W) {
                    const T v = lab[(long)row * W + x];
                    b[k] = match ? v == value : v != (T)0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VX_MO_PACK_U; ++k) {
            const vx_u64 m = __ballot(b[k]);
            if (lane == 0 && w0 + k < nw) bits[w0 + k] = m;
        }
    }
}

#define VX_MO_MASK 0
#define VX_MO_KEEP 1
#define VX_MO_RESTRICT 2
#define VX_MO_PAINT 3
template <typename T>
__global__ void __launch_bounds__(256) vx_mo_unpack_k(const vx_u64* __restrict__ bits, const T* in, T* out, T value, int mode, long V, int W, int Wq) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const unsigned row = (unsigned)v / (unsigned)W;
        const int x = (int)((unsigned)v % (unsigned)W);
        const bool bit = (bits[(long)row * Wq + (x >> 6)] >> (x & 63)) & 1ull;
        T r;
        if (mode == VX_MO_MASK) r = bit ? (T)1 : (T)0;
        else {
            const T a = in[v];
            if (mode == VX_MO_KEEP) r = bit ? a : (T)0;
            else if (mode == VX_MO_RESTRICT) r = (a == value && !bit) ? (T)0 : a;
            else r = (bit && a == (T)0) ? value : a;
        }
        out[v] = r;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) vx_mo_background_k(const T* __restrict__ lab, unsigned char* __restrict__ bg, long V) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) bg[v] = lab[v] == (T)0 ? 1 : 0;
}

// What a background voxel sees: a face of the volume (open) and the smallest / largest non-zero neighbour value.  Lanes are cut into runs of equal component id
// (0 = nothing to send); a run is folded onto its first lane by shuffles (a lane 2^k further on with the same id belongs to the run, or to another run of the same
// component: min, max and or do not mind) and that lane sends the atomics.  T is signed for 4 / 8 bytes: the values are taken as signed 64-bit numbers.
template <typename T>
__global__ void __launch_bounds__(256) vx_mo_hole_scan_k(const T* __restrict__ lab, const int* __restrict__ cc, int N, int D, int H, int W, int maxnz, long long* lo,
                                                         long long* hi, int* open) {
    const long V = (long)D * H * W;
    const int lane = threadIdx.x & 63;
    for (long base = (long)blockIdx.x * 256; base < V; base += (long)gridDim.x * 256) {          // block-uniform trip count: shuffles and ballots see whole waves
        const long v = base + threadIdx.x;
        int id = 0, op = 0;
        long long mn = INT64_MAX, mx = INT64_MIN;
        if (v < V && lab[v] == (T)0) {
            id = cc[v];
            if (id < 1 || id > N) id = 0;
        }
        if (id) {
            const unsigned rowi = (unsigned)v / (unsigned)W;
            const int x = (int)((unsigned)v % (unsigned)W), y = (int)(rowi % (unsigned)H), z = (int)(rowi / (unsigned)H);
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int nz = (dz != 0) + (dy != 0) + (dx != 0);
                        if (nz == 0 || nz > maxnz) continue;
                        const int zz = z + dz, yy = y + dy, xx = x + dx;
                        if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) { op = 1; continue; }
                        const T a = lab[((long)zz * H + yy) * W + xx];
                        if (a != (T)0) { const long long s = (long long)a; mn = s < mn ? s : mn; mx = s > mx ? s : mx; }
                    }
            if (!op && mn > mx) id = 0;          // an inner voxel of the component: nothing to send
        }
        const int prev = __shfl_up(id, 1, 64);
        const bool head = id != 0 && (lane == 0 || prev != id);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int oid = __shfl_down(id, o, 64), oop = __shfl_down(op, o, 64);
            const long long omn = __shfl_down(mn, o, 64), omx = __shfl_down(mx, o, 64);
            if (lane + o < 64 && oid == id) { op |= oop; mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; }
        }
        // lo only falls, hi only rises, open only goes to 1: whatever a read returns, a value it already covers need not be sent (a Bernoulli mask's background is
        // one component that every wave meets: without the reads, millions of atomics on three addresses)
        if (head) {
            if (op && !__hip_atomic_load(open + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) open[id] = 1;          // (every writer stores the same value)
            if (mn <= mx) {
                if (mn < __hip_atomic_load(lo + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo + id, mn);
                if (mx > __hip_atomic_load(hi + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hi + id, mx);
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) vx_mo_hole_fill_k(const T* lab, T* out, const int* __restrict__ cc, int N, const long long* __restrict__ lo,
                                                         const long long* __restrict__ hi, const int* __restrict__ open, const long long* __restrict__ applied,
                                                         int n_applied, long V) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        T r = lab[v];
        if (r == (T)0) {
            const int id = cc[v];
            if (id >= 1 && id <= N && !open[id] && lo[id] == hi[id]) {
                const long long c = lo[id];
                bool ok = n_applied == 0;
                for (int k = 0; k < n_applied; ++k) ok = ok || applied[k] == c;
                if (ok) r = (T)c;
            }
        }
        out[v] = r;
    }
}

static inline int vx_mo_grid(long n) { return (int)(n > VX_MO_GRID_CAP ? VX_MO_GRID_CAP : (n < 1 ? 1 : n)); }
static inline int vx_mo_wq(int W) { return (W + 63) / 64; }
static inline vx_u64 vx_mo_tail(int W) { return (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull; }
static inline bool vx_mo_extents_ok(int D, int H, int W) { return D > 0 && H > 0 && W > 0 && (long)D * H <= 0x7fffffffL && (long)D * H * W <= 0x7fffffffL; }
static inline bool vx_mo_conn_ok(int c) { return c == 6 || c == 18 || c == 26; }
static inline bool vx_mo_bytes_ok(int b) { return b == 1 || b == 4 || b == 8; }

extern "C" int vx_morph_grid_cap(void) { return VX_MO_GRID_CAP; }
extern "C" int vx_morph_max_fused(void) { return VX_MO_FUSED; }

extern "C" int vx_morph_words(int D, int H, int W) {
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_words: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    return (int)((long)D * H * vx_mo_wq(W));          // <= D * H * W
}

extern "C" int vx_morph_pack(const void* lab, int lab_bytes, long value, int match, unsigned long long* bits, int D, int H, int W, void* stream) {
    VX_REQUIRE(lab && bits, "vx_morph_pack: null pointer");
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_pack: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(vx_mo_bytes_ok(lab_bytes), "vx_morph_pack: label width %d bytes not supported", lab_bytes);
    VX_REQUIRE(match == 0 || match == 1, "vx_morph_pack: match %d is neither 0 nor 1", match);
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)D * H;
    const int Wq = vx_mo_wq(W);
    const dim3 g(vx_mo_grid((rows * Wq + 4 * VX_MO_PACK_U - 1) / (4 * VX_MO_PACK_U))), b(256);
    if (lab_bytes == 1) vx_mo_pack_k<unsigned char><<<g, b, 0, st>>>((const unsigned char*)lab, (unsigned char)value, match, bits, rows, W, Wq);
    else if (lab_bytes == 4) vx_mo_pack_k<unsigned int><<<g, b, 0, st>>>((const unsigned int*)lab, (unsigned int)value, match, bits, rows, W, Wq);
    else vx_mo_pack_k<vx_u64><<<g, b, 0, st>>>((const vx_u64*)lab, (vx_u64)value, match, bits, rows, W, Wq);
    VX_LAUNCH_CHECK("vx_morph_pack");
    return 0;
}

extern "C" int vx_morph_step(const unsigned long long* in, unsigned long long* out, unsigned long long* tmp, int D, int H, int W, int op, int connectivity, int iterations,
                             int border_value, void* stream) {
    VX_REQUIRE(in && out, "vx_morph_step: null pointer");
    VX_REQUIRE(in != out && in != tmp && out != tmp, "vx_morph_step: in, out and tmp must be three different buffers");
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_step: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(op == 0 || op == 1, "vx_morph_step: op %d is neither 0 (dilate) nor 1 (erode)", op);
    VX_REQUIRE(vx_mo_conn_ok(connectivity), "vx_morph_step: connectivity %d is none of 6, 18, 26", connectivity);
    VX_REQUIRE(iterations >= 1, "vx_morph_step: iterations %d, at least 1 wanted", iterations);
    VX_REQUIRE(border_value == 0 || border_value == 1, "vx_morph_step: border_value %d is neither 0 nor 1", border_value);
    VX_REQUIRE(tmp || iterations <= VX_MO_FUSED, "vx_morph_step: %d iterations (more than %d) need the tmp buffer", iterations, VX_MO_FUSED);
    // a voxel is at most D + H + W - 3 steps from any other and one more from the border: the result is stationary by then
    const long reach = (long)D + H + W;
    int n = iterations > reach ? (int)reach : iterations;
    hipStream_t st = (hipStream_t)stream;
    const int Wq = vx_mo_wq(W);
    const vx_u64 tail = vx_mo_tail(W), inv = op ? ~0ull : 0ull, bfill = (border_value ^ op) ? ~0ull : 0ull;
    const dim3 b(256), gw(vx_mo_grid(((long)D * H * Wq + 255) / 256));
    const vx_u64* src = in;
    for (; n > 0; --n) {
        vx_u64* dst = ((n - 1) & 1) ? tmp : out;          // the last launch writes out
        vx_mo_step_k<<<gw, b, 0, st>>>(src, dst, D, H, Wq, tail, inv, bfill, connectivity, 0);
        src = dst;
    }
    VX_LAUNCH_CHECK("vx_morph_step");
    return 0;
}

extern "C" int vx_morph_boundary(const unsigned long long* in, unsigned long long* out, int D, int H, int W, int connectivity, void* stream) {
    VX_REQUIRE(in && out, "vx_morph_boundary: null pointer");
    VX_REQUIRE(in != out, "vx_morph_boundary: out must not be in");
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_boundary: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(vx_mo_conn_ok(connectivity), "vx_morph_boundary: connectivity %d is none of 6, 18, 26", connectivity);
    const int Wq = vx_mo_wq(W);
    vx_mo_step_k<<<dim3(vx_mo_grid(((long)D * H * Wq + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(in, out, D, H, Wq, vx_mo_tail(W), ~0ull, ~0ull, connectivity, 1);
    VX_LAUNCH_CHECK("vx_morph_boundary");
    return 0;
}

extern "C" int vx_morph_ball_max_rows(void) { return VX_MO_BALL_ROWS; }

extern "C" int vx_morph_ball(const unsigned long long* in, const unsigned long long* gate, unsigned long long* out, int D, int H, int W, const int* rows, int n_rows, int op,
                             int border_value, void* stream) {
    VX_REQUIRE(in && out && rows, "vx_morph_ball: null pointer");
    VX_REQUIRE(out != in && out != gate, "vx_morph_ball: out must be neither in nor gate");
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_ball: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(n_rows >= 1 && n_rows <= VX_MO_BALL_ROWS, "vx_morph_ball: %d rows, 1 .. %d wanted", n_rows, VX_MO_BALL_ROWS);
    VX_REQUIRE(op == 0 || op == 1, "vx_morph_ball: op %d is neither 0 (dilate) nor 1 (erode)", op);
    VX_REQUIRE(border_value == 0 || border_value == 1, "vx_morph_ball: border_value %d is neither 0 nor 1", border_value);
    const int Wq = vx_mo_wq(W);
    vx_mo_ball_k<<<dim3(vx_mo_grid(((long)D * H * Wq + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(in, gate, out, D, H, Wq, vx_mo_tail(W), op ? ~0ull : 0ull,
                                                                                                       (border_value ^ op) ? ~0ull : 0ull, rows, n_rows);
    VX_LAUNCH_CHECK("vx_morph_ball");
    return 0;
}

extern "C" int vx_morph_unpack(const unsigned long long* bits, const void* in, void* out, int lab_bytes, long value, int mode, int D, int H, int W, void* stream) {
    VX_REQUIRE(bits && out, "vx_morph_unpack: null pointer");
    VX_REQUIRE(mode >= VX_MO_MASK && mode <= VX_MO_PAINT, "vx_morph_unpack: mode %d is none of 0 (mask), 1 (keep), 2 (restrict), 3 (paint)", mode);
    VX_REQUIRE(in || mode == VX_MO_MASK, "vx_morph_unpack: null pointer (mode %d reads in)", mode);
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_morph_unpack: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(vx_mo_bytes_ok(lab_bytes), "vx_morph_unpack: label width %d bytes not supported", lab_bytes);
    hipStream_t st = (hipStream_t)stream;
    const long V = (long)D * H * W;
    const int Wq = vx_mo_wq(W);
    const dim3 g(vx_mo_grid((V + 255) / 256)), b(256);
    if (lab_bytes == 1) vx_mo_unpack_k<unsigned char><<<g, b, 0, st>>>(bits, (const unsigned char*)in, (unsigned char*)out, (unsigned char)value, mode, V, W, Wq);
    else if (lab_bytes == 4) vx_mo_unpack_k<unsigned int><<<g, b, 0, st>>>(bits, (const unsigned int*)in, (unsigned int*)out, (unsigned int)value, mode, V, W, Wq);
    else vx_mo_unpack_k<vx_u64><<<g, b, 0, st>>>(bits, (const vx_u64*)in, (vx_u64*)out, (vx_u64)value, mode, V, W, Wq);
    VX_LAUNCH_CHECK("vx_morph_unpack");
    return 0;
}

extern "C" int vx_morph_background(const void* lab, int lab_bytes, unsigned char* bg, long V, void* stream) {
    VX_REQUIRE(lab && bg, "vx_morph_background: null pointer");
    VX_REQUIRE(V > 0 && V <= 0x7fffffffL, "vx_morph_background: bad size %ld (1 .. 2^31 - 1 voxels)", V);
    VX_REQUIRE(vx_mo_bytes_ok(lab_bytes), "vx_morph_background: label width %d bytes not supported", lab_bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(vx_mo_grid((V + 255) / 256)), b(256);
    if (lab_bytes == 1) vx_mo_background_k<unsigned char><<<g, b, 0, st>>>((const unsigned char*)lab, bg, V);
    else if (lab_bytes == 4) vx_mo_background_k<unsigned int><<<g, b, 0, st>>>((const unsigned int*)lab, bg, V);
    else vx_mo_background_k<vx_u64><<<g, b, 0, st>>>((const vx_u64*)lab, bg, V);
    VX_LAUNCH_CHECK("vx_morph_background");
    return 0;
}

extern "C" int vx_hole_scan(const void* lab, int lab_bytes, const int* cc, int N, int D, int H, int W, int connectivity, long long* lo, long long* hi, int* open,
                            void* stream) {
    VX_REQUIRE(lab && cc && lo && hi && open, "vx_hole_scan: null pointer");
    VX_REQUIRE(N >= 0, "vx_hole_scan: bad component count %d", N);
    VX_REQUIRE(vx_mo_extents_ok(D, H, W), "vx_hole_scan: bad sizes %d x %d x %d (each > 0, D * H * W <= 2^31 - 1)", D, H, W);
    VX_REQUIRE(vx_mo_conn_ok(connectivity), "vx_hole_scan: connectivity %d is none of 6, 18, 26", connectivity);
    VX_REQUIRE(vx_mo_bytes_ok(lab_bytes), "vx_hole_scan: label width %d bytes not supported", lab_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int maxnz = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
    const dim3 g(vx_mo_grid(((long)D * H * W + 255) / 256)), b(256);
    if (lab_bytes == 1) vx_mo_hole_scan_k<unsigned char><<<g, b, 0, st>>>((const unsigned char*)lab, cc, N, D, H, W, maxnz, lo, hi, open);
    else if (lab_bytes == 4) vx_mo_hole_scan_k<int><<<g, b, 0, st>>>((const int*)lab, cc, N, D, H, W, maxnz, lo, hi, open);
    else vx_mo_hole_scan_k<long long><<<g, b, 0, st>>>((const long long*)lab, cc, N, D, H, W, maxnz, lo, hi, open);
    VX_LAUNCH_CHECK("vx_hole_scan");
    return 0;
}

extern "C" int vx_hole_fill(const void* lab, void* out, int lab_bytes, const int* cc, int N, const long long* lo, const long long* hi, const int* open,
                            const long long* applied, int n_applied, long V, void* stream) {
    VX_REQUIRE(lab && out && cc && lo && hi && open, "vx_hole_fill: null pointer");
    VX_REQUIRE(N >= 0 && n_applied >= 0 && (applied || n_applied == 0), "vx_hole_fill: bad args (N < 0, n_applied < 0 or applied null with n_applied > 0)");
    VX_REQUIRE(V > 0 && V <= 0x7fffffffL, "vx_hole_fill: bad size %ld (1 .. 2^31 - 1 voxels)", V);
    VX_REQUIRE(vx_mo_bytes_ok(lab_bytes), "vx_hole_fill: label width %d bytes not supported", lab_bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(vx_mo_grid((V + 255) / 256)), b(256);
    if (lab_bytes == 1) vx_mo_hole_fill_k<unsigned char><<<g, b, 0, st>>>((const unsigned char*)lab, (unsigned char*)out, cc, N, lo, hi, open, applied, n_applied, V);
    else if (lab_bytes == 4) vx_mo_hole_fill_k<int><<<g, b, 0, st>>>((const int*)lab, (int*)out, cc, N, lo, hi, open, applied, n_applied, V);
    else vx_mo_hole_fill_k<long long><<<g, b, 0, st>>>((const long long*)lab, (long long*)out, cc, N, lo, hi, open, applied, n_applied, V);
    VX_LAUNCH_CHECK("vx_hole_fill");
    return 0;
}
