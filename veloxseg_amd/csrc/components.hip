// Connected-component labelling of a label volume on the GPU: union-find with the output array `cc` as the parent array, the per-component
// tallies (sizes, overlap hits) and the keep / drop filter.  No counterpart in the reference (its metrics are per voxel, utils/metric/metrics.py); the lesion-level
// false-positive / false-negative volumes of the autoPET challenge are defined on these components.  Contracts in include/veloxseg_hip.h.
//
// vx_cc_label runs five phases over seven launches (the scan takes three); phases meet at kernel boundaries only, no workgroup ever waits for another one:
//   1. tiles    every 8 x 8 x 32 tile is labelled in LDS: each voxel is united with its backward neighbours inside the tile, then the tile is flattened and
//               cc[v] = flat index of the tile-local root (the smallest flat index of the voxel's piece of the tile), -1 on background;
//   2. seams    voxels on a tile face are united with the backward neighbours that sit in another tile, in the global array;
//   3. roots    cc[v] = root(v); a wave's ballot of {cc[v] == v} is the 64-bit root mask of its 64 voxels, the popcount its entry of the prefix array;
//   4. scan     exclusive prefix sum over the popcounts (chunk sums, one block over the chunk sums, chunk scan); the total is N;
//   5. apply    cc[v] = 1 + #roots below root(v) = prefix[word] + popcount(mask[word] below the bit) + 1: components are numbered by their smallest flat index.
//
// Invariant of the parent array: cc[v] <= v for every foreground voxel, a stored parent is only ever replaced by a smaller index of the SAME set, and sets only
// merge.  Whatever value a read returns -- an old one from a non-coherent cache included -- was a parent of v at some time, so it is still an ancestor in v's set.
#include "vx_common.h"

#define VX_CC_TZ 8
#define VX_CC_TY 8
#define VX_CC_TX 32
#define VX_CC_TILE (VX_CC_TZ * VX_CC_TY * VX_CC_TX)          // 2048 voxels, 8 per thread
#define VX_CC_GRID_CAP 4096                                 // the kernels over tiles and over 256-voxel slabs are grid-stride loops above this block count
#define VX_CC_CHUNK 4096                                    // prefix entries per scan chunk (256 threads x 16)

// the 13 backward neighbours (lexicographically negative offsets, z slowest), ordered so that the first 3 have one non-zero coordinate and the first 9 at most two
__constant__ signed char vx_cc_off[13][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0},
                                             {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1}, {-1, -1, 0}, {-1, 1, 0},
                                             {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

__device__ __forceinline__ int vx_cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: every step moves to a strictly smaller index (the loop goes on only while the value read is below x and not negative), whatever the read returns;
// by the invariant above the result is an ancestor of x in x's set (the root, unless a concurrent union has just hung the root below another one).
__device__ __forceinline__ int vx_cc_find(const int* cc, int x) {
    for (;;) {
        const int p = vx_cc_ld(cc + x);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

// Unite the sets of a and b.  Terminates: a pass either ends the loop (a == b: one set already; or the atomicMin found the larger index still a root and hung it
// below the smaller one) or goes on with the larger index replaced by the value the atomic returned, which is strictly smaller (a parent is never above its child);
// find never raises an index, so a + b falls strictly with every retry and is bounded below by 0.  No pass waits for another thread's progress.
// Sets are preserved: when atomicMin(&cc[hi], lo) returns old != hi, cc[hi] now holds min(old, lo); if that dropped the edge hi -> old, the next pass unites old with
// lo, which restores it.
__device__ __forceinline__ void vx_cc_union(int* cc, int a, int b) {
    for (;;) {
        a = vx_cc_find(cc, a);
        b = vx_cc_find(cc, b);
        if (a == b) return;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int old = atomicMin(cc + hi, lo);
        if (old == hi) return;
        a = lo; b = old;
    }
}

// the same two loops on the LDS parent array of one tile (workgroup scope: coherent; the termination argument is the same)
__device__ __forceinline__ int vx_cc_lfind(const int* sp, int x) {
    for (;;) {
        const int p = __hip_atomic_load(sp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p >= x || p < 0) return x;
        x = p;
    }
}
__device__ __forceinline__ void vx_cc_lunion(int* sp, int a, int b) {
    for (;;) {
        a = vx_cc_lfind(sp, a);
        b = vx_cc_lfind(sp, b);
        if (a == b) return;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int old = atomicMin(sp + hi, lo);
        if (old == hi) return;
        a = lo; b = old;
    }
}

// phase 1: one tile per block iteration; thread t owns column (y, x) = (t >> 5, t & 31) of the tile, its 8 voxels along z
template <typename T>
__global__ void __launch_bounds__(256) vx_cc_tiles_k(const T* __restrict__ lab, int* __restrict__ cc, int D, int H, int W, int nnb, int tz_n, int ty_n, int tx_n) {
    __shared__ T sv[VX_CC_TILE];
    __shared__ int sp[VX_CC_TILE];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const long ntiles = (long)tz_n * ty_n * tx_n;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int x0 = (int)(tile % tx_n) * VX_CC_TX, y0 = (int)((tile / tx_n) % ty_n) * VX_CC_TY, z0 = (int)(tile / ((long)tx_n * ty_n)) * VX_CC_TZ;
        const bool col = y0 + y < H && x0 + x < W;
#pragma unroll
        for (int z = 0; z < VX_CC_TZ; ++z) {
            const int li = z * 256 + (int)threadIdx.x;
            T v = (T)0;
            if (col && z0 + z < D) v = lab[((long)(z0 + z) * H + (y0 + y)) * W + (x0 + x)];
            sv[li] = v;
            sp[li] = v != (T)0 ? li : -1;
        }
        __syncthreads();
#pragma unroll
        for (int z = 0; z < VX_CC_TZ; ++z) {
            const int li = z * 256 + (int)threadIdx.x;
            const T v = sv[li];
            if (v == (T)0) continue;
            for (int k = 0; k < nnb; ++k) {
                const int nz = z + vx_cc_off[k][0], ny = y + vx_cc_off[k][1], nx = x + vx_cc_off[k][2];
                if (nz < 0 || ny < 0 || ny >= VX_CC_TY || nx < 0 || nx >= VX_CC_TX) continue;
                const int ni = (nz * VX_CC_TY + ny) * VX_CC_TX + nx;
                if (sv[ni] == v) vx_cc_lunion(sp, li, ni);
            }
        }
        __syncthreads();
#pragma unroll
        for (int z = 0; z < VX_CC_TZ; ++z) {
            if (!(col && z0 + z < D)) continue;
            const int li = z * 256 + (int)threadIdx.x;
            int out = -1;
            if (sv[li] != (T)0) {
                const int r = vx_cc_lfind(sp, li);          // the unions are over: the tile-local root
                const int rz = r >> 8, ry = (r >> 5) & 7, rx = r & 31;
                out = (int)(((long)(z0 + rz) * H + (y0 + ry)) * W + (x0 + rx));          // the tile order is the volume order: a root stays below its voxels
            }
            cc[((long)(z0 + z) * H + (y0 + y)) * W + (x0 + x)] = out;
        }
        __syncthreads();
    }
}

// phase 2: unions in the global array, with the backward neighbours that sit in another tile (those inside the tile are united already).  A one-level variant
// (cc[v] = v, then every union here) gave the same maps and was 1.03 - 3 x slower on both probe volumes: it is not kept.
template <typename T>
__global__ void __launch_bounds__(256) vx_cc_merge_k(const T* __restrict__ lab, int* cc, int D, int H, int W, int nnb) {
    const long V = (long)D * H * W;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const T val = lab[v];
        if (val == (T)0) continue;
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
        const int tx = x % VX_CC_TX, ty = y % VX_CC_TY;
        if (z % VX_CC_TZ != 0 && ty != 0 && ty != VX_CC_TY - 1 && tx != 0 && tx != VX_CC_TX - 1) continue;          // no backward neighbour leaves the tile
        for (int k = 0; k < nnb; ++k) {
            const int dz = vx_cc_off[k][0], dy = vx_cc_off[k][1], dx = vx_cc_off[k][2];
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            if (nz / VX_CC_TZ == z / VX_CC_TZ && ny / VX_CC_TY == y / VX_CC_TY && nx / VX_CC_TX == x / VX_CC_TX) continue;
            const long n = ((long)nz * H + ny) * W + nx;
            if (lab[n] == val) vx_cc_union(cc, (int)v, (int)n);
        }
    }
}

// phase 3: flatten + root masks.  A wave covers 64 consecutive voxels from a multiple of 64, so its ballot is word v >> 6 of the mask.  Other threads overwrite
// the entries this find reads with their roots meanwhile: those are ancestors too.
__global__ void __launch_bounds__(256) vx_cc_roots_k(int* cc, long V, unsigned long long* __restrict__ mask, int* __restrict__ pre) {
    for (long base = (long)blockIdx.x * 256; base < V; base += (long)gridDim.x * 256) {          // block-uniform trip count: the ballots see whole waves
        const long v = base + threadIdx.x;
        bool root = false;
        if (v < V && vx_cc_ld(cc + v) >= 0) {
            const int r = vx_cc_find(cc, (int)v);
            root = r == (int)v;
            if (!root) cc[v] = r;
        }
        const unsigned long long m = __ballot(root);
        if ((threadIdx.x & 63) == 0 && v < V) { mask[v >> 6] = m; pre[v >> 6] = __popcll(m); }
    }
}

// inclusive scan of one value per thread over a 256-thread block; returns the block total in `total`
__device__ __forceinline__ int vx_cc_block_scan(int v, int* sm, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    __syncthreads();
    if (lane == 63) sm[wid] = v;
    __syncthreads();
    int add = 0;
    for (int w = 0; w < wid; ++w) add += sm[w];
    total = sm[0] + sm[1] + sm[2] + sm[3];
    return v + add;
}

// phase 4a: bsum[c] = sum of chunk c of pre; one block per chunk (at most 2^31 / 64 / VX_CC_CHUNK = 8192 of them)
__global__ void __launch_bounds__(256) vx_cc_chunk_sum_k(const int* __restrict__ pre, long nw, int* __restrict__ bsum) {
    __shared__ int sm[4];
    int s = 0;
    const long lo = (long)blockIdx.x * VX_CC_CHUNK + (long)threadIdx.x * 16;
    for (int k = 0; k < 16; ++k) if (lo + k < nw) s += pre[lo + k];
    int total;
    vx_cc_block_scan(s, sm, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// phase 4b: one block: bsum -> its exclusive prefix, num[0] = total
__global__ void __launch_bounds__(256) vx_cc_chunk_scan_k(int* __restrict__ bsum, int nchunks, int* __restrict__ num) {
    __shared__ int sm[4];
    int carry = 0;
    for (int base = 0; base < nchunks; base += 256) {
        const int i = base + (int)threadIdx.x;
        const int v = i < nchunks ? bsum[i] : 0;
        int total;
        const int inc = vx_cc_block_scan(v, sm, total);
        if (i < nchunks) bsum[i] = carry + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) num[0] = carry;
}

// phase 4c: pre -> its exclusive prefix (chunk-local scan + the chunk's offset); one block per chunk
__global__ void __launch_bounds__(256) vx_cc_chunk_apply_k(int* __restrict__ pre, long nw, const int* __restrict__ bsum) {
    __shared__ int sm[4];
    const long lo = (long)blockIdx.x * VX_CC_CHUNK + (long)threadIdx.x * 16;
    int e[16], s = 0;
    for (int k = 0; k < 16; ++k) { e[k] = lo + k < nw ? pre[lo + k] : 0; s += e[k]; }
    int total;
    int run = bsum[blockIdx.x] + vx_cc_block_scan(s, sm, total) - s;
    for (int k = 0; k < 16; ++k) { if (lo + k < nw) pre[lo + k] = run; run += e[k]; }
}

// phase 5: the id of a voxel is 1 + the number of roots below its root (reads cc[v] only: the masks and the prefix say the rest)
__global__ void __launch_bounds__(256) vx_cc_apply_k(int* __restrict__ cc, long V, const unsigned long long* __restrict__ mask, const int* __restrict__ pre) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const int p = cc[v];
        int id = 0;
        if (p >= 0) id = pre[p >> 6] + __popcll(mask[p >> 6] & ((1ull << (p & 63)) - 1ull)) + 1;
        cc[v] = id;
    }
}

// sizes[id] += 1, hits[id] += (other != 0), with few atomics on one address (a mask often holds ONE component with most of its voxels; per-voxel or per-run atomics
// on that id measured 143 ms on 56 M voxels, section 18):
//   - background (id 0) is counted from ballots into a register of lane 0 and leaves the wave once;
//   - the id of the wave's first foreground lane (mostly the id of all of them) is counted from one ballot, one add for the wave;
//   - the other lanes are cut into runs of equal id; the head of a run counts its lanes and hits from the ballots and sends one add;
//   - an add goes to a 256-slot table in LDS (slot id & 255, claimed by the first id that hashes there) and, when another id owns the slot, to the global array
//     with one 64-bit integer atomic; the table leaves the block once, at its end.
// Ids outside [0, N] are not counted.  Integer adds only: the sums do not depend on the order.
#define VX_CC_SLOTS 256
__device__ __forceinline__ void vx_cc_tally_add(int* sid, unsigned int* ssz, unsigned int* sht, int id, unsigned int n, unsigned int nh, unsigned long long* sizes,
                                                unsigned long long* hits) {
    const int slot = id & (VX_CC_SLOTS - 1);
    const int cur = atomicCAS(sid + slot, -1, id);
    if (cur == -1 || cur == id) {
        atomicAdd(ssz + slot, n);
        if (nh) atomicAdd(sht + slot, nh);
    } else {
        atomicAdd(sizes + id, (unsigned long long)n);
        if (nh) atomicAdd(hits + id, (unsigned long long)nh);
    }
}

template <typename T, bool OTHER>
__global__ void __launch_bounds__(256) vx_cc_tally_k(const int* __restrict__ cc, const T* __restrict__ other, long V, int N, unsigned long long* __restrict__ sizes,
                                                     unsigned long long* __restrict__ hits) {
    __shared__ int sid[VX_CC_SLOTS];
    __shared__ unsigned int ssz[VX_CC_SLOTS], sht[VX_CC_SLOTS];          // a block sees at most 2^31 / 256 / VX_CC_GRID_CAP + 1 slabs of 256 voxels: far below 2^32
    const int lane = threadIdx.x & 63;
    sid[threadIdx.x] = -1; ssz[threadIdx.x] = 0u; sht[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int bg = 0u, bgh = 0u;                                      // (the same in every lane; lane 0 sends them)
    for (long base = (long)blockIdx.x * 256; base < V; base += (long)gridDim.x * 256) {          // block-uniform trip count: the ballots see whole waves
        const long v = base + threadIdx.x;
        int id = -1;
        bool hit = false;
        if (v < V) {
            id = cc[v];
            if (id < 0 || id > N) id = -1;
            if (OTHER) hit = other[v] != (T)0;
        }
        const unsigned long long tm = OTHER ? __ballot(hit) : 0ull, bgm = __ballot(id == 0), fgm = __ballot(id > 0);
        bg += (unsigned int)__popcll(bgm);
        bgh += (unsigned int)__popcll(tm & bgm);
        if (fgm == 0ull) continue;                                       // (wave-uniform)
        const int lead = __ffsll((long long)fgm) - 1;
        const int lid = __shfl(id, lead, 64);
        const unsigned long long lm = __ballot(id == lid);
        if (lane == lead) vx_cc_tally_add(sid, ssz, sht, lid, (unsigned int)__popcll(lm), (unsigned int)__popcll(tm & lm), sizes, hits);
        const int prev = __shfl_up(id, 1, 64);
        const unsigned long long cuts = __ballot(lane == 0 || prev != id);          // the first lane of every run of equal ids
        if (id > 0 && id != lid && ((cuts >> lane) & 1ull)) {
            const unsigned long long above = lane == 63 ? 0ull : (cuts >> (lane + 1)) << (lane + 1);
            const int end = above ? __ffsll((long long)above) - 1 : 64;
            const unsigned long long run = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
            vx_cc_tally_add(sid, ssz, sht, id, (unsigned int)(end - lane), (unsigned int)__popcll(tm & run), sizes, hits);
        }
    }
    if (lane == 0) {
        if (bg) atomicAdd(sizes, (unsigned long long)bg);
        if (OTHER && bgh) atomicAdd(hits, (unsigned long long)bgh);
    }
    __syncthreads();
    const int id = sid[threadIdx.x];
    if (id >= 0) {
        if (ssz[threadIdx.x]) atomicAdd(sizes + id, (unsigned long long)ssz[threadIdx.x]);
        if (OTHER && sht[threadIdx.x]) atomicAdd(hits + id, (unsigned long long)sht[threadIdx.x]);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) vx_cc_select_k(const int* __restrict__ cc, const unsigned char* __restrict__ keep, int N, const T* in, T* out, long V) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
        const int id = cc[v];
        out[v] = (id >= 0 && id <= N && keep[id]) ? in[v] : (T)0;
    }
}

static inline int vx_cc_grid(long n) { return (int)(n > VX_CC_GRID_CAP ? VX_CC_GRID_CAP : (n < 1 ? 1 : n)); }
static inline long vx_cc_words(long V) { return (V + 63) / 64; }
static inline long vx_cc_chunks(long V) { return (vx_cc_words(V) + VX_CC_CHUNK - 1) / VX_CC_CHUNK; }
// workspace layout: u64 mask[words] | int pre[words] | int bsum[chunks]
static inline long vx_cc_ws(long V) { return vx_cc_words(V) * 12 + vx_cc_chunks(V) * 4; }

extern "C" int vx_cc_grid_cap(void) { return VX_CC_GRID_CAP; }

extern "C" int vx_cc_ws_bytes(int D, int H, int W) {
    VX_REQUIRE(D > 0 && H > 0 && W > 0, "vx_cc_ws_bytes: bad sizes");
    const long V = (long)D * H * W;
    VX_REQUIRE((long)D * H <= 0x7fffffffL && V <= 0x7fffffffL, "vx_cc_ws_bytes: %d x %d x %d voxels do not fit a 32-bit parent index", D, H, W);
    return (int)vx_cc_ws(V);
}

extern "C" int vx_cc_label(const void* labels, int lab_bytes, int* cc, int D, int H, int W, int connectivity, void* ws, int* num, void* stream) {
    VX_REQUIRE(labels && cc && ws && num, "vx_cc_label: null pointer");
    VX_REQUIRE(D > 0 && H > 0 && W > 0, "vx_cc_label: bad sizes");
    VX_REQUIRE((long)D * H <= 0x7fffffffL && (long)D * H * W <= 0x7fffffffL, "vx_cc_label: %d x %d x %d voxels do not fit a 32-bit parent index", D, H, W);
    VX_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "vx_cc_label: connectivity %d is none of 6, 18, 26", connectivity);
    VX_REQUIRE(lab_bytes == 1 || lab_bytes == 4 || lab_bytes == 8, "vx_cc_label: label width %d bytes not supported", lab_bytes);
    VX_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "vx_cc_label: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long V = (long)D * H * W, nw = vx_cc_words(V);
    const int nchunks = (int)vx_cc_chunks(V), nnb = connectivity == 6 ? 3 : (connectivity == 18 ? 9 : 13);
    unsigned long long* mask = (unsigned long long*)ws;
    int* pre = (int*)(mask + nw);
    int* bsum = pre + nw;
    const dim3 b(256), gv(vx_cc_grid((V + 255) / 256));
    const int tz = vx_cdiv(D, VX_CC_TZ), ty = vx_cdiv(H, VX_CC_TY), tx = vx_cdiv(W, VX_CC_TX);
    const dim3 gt(vx_cc_grid((long)tz * ty * tx));
#define VX_CC_PHASE12(T)                                                                              \
    do {                                                                                              \
        vx_cc_tiles_k<T><<<gt, b, 0, st>>>((const T*)labels, cc, D, H, W, nnb, tz, ty, tx);           \
        vx_cc_merge_k<T><<<gv, b, 0, st>>>((const T*)labels, cc, D, H, W, nnb);                       \
    } while (0)
    if (lab_bytes == 1) VX_CC_PHASE12(unsigned char);
    else if (lab_bytes == 4) VX_CC_PHASE12(unsigned int);
    else VX_CC_PHASE12(unsigned long long);
#undef VX_CC_PHASE12
    vx_cc_roots_k<<<gv, b, 0, st>>>(cc, V, mask, pre);
    vx_cc_chunk_sum_k<<<dim3(nchunks), b, 0, st>>>(pre, nw, bsum);
    vx_cc_chunk_scan_k<<<dim3(1), b, 0, st>>>(bsum, nchunks, num);
    vx_cc_chunk_apply_k<<<dim3(nchunks), b, 0, st>>>(pre, nw, bsum);
    vx_cc_apply_k<<<gv, b, 0, st>>>(cc, V, mask, pre);
    VX_LAUNCH_CHECK("vx_cc_label");
    return 0;
}

extern "C" int vx_cc_tally(const int* cc, const void* other, int other_bytes, long V, int N, unsigned long long* sizes, unsigned long long* hits, void* stream) {
    VX_REQUIRE(cc && sizes && V > 0 && N >= 0, "vx_cc_tally: bad args (null pointer, V <= 0 or N < 0)");
    VX_REQUIRE(V <= 0x7fffffffL, "vx_cc_tally: %ld voxels are more than a component map holds", V);
    VX_REQUIRE((other != nullptr) == (hits != nullptr), "vx_cc_tally: other and hits come together");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(vx_cc_grid((V + 255) / 256)), b(256);
    if (!other) vx_cc_tally_k<unsigned char, false><<<g, b, 0, st>>>(cc, nullptr, V, N, sizes, nullptr);
    else if (other_bytes == 1) vx_cc_tally_k<unsigned char, true><<<g, b, 0, st>>>(cc, (const unsigned char*)other, V, N, sizes, hits);
    else if (other_bytes == 4) vx_cc_tally_k<unsigned int, true><<<g, b, 0, st>>>(cc, (const unsigned int*)other, V, N, sizes, hits);
    else if (other_bytes == 8) vx_cc_tally_k<unsigned long long, true><<<g, b, 0, st>>>(cc, (const unsigned long long*)other, V, N, sizes, hits);
    else VX_FAIL(-3, "vx_cc_tally: label width %d bytes not supported", other_bytes);
    VX_LAUNCH_CHECK("vx_cc_tally");
    return 0;
}

extern "C" int vx_cc_select(const int* cc, const unsigned char* keep, int N, const void* in, void* out, int lab_bytes, long V, void* stream) {
    VX_REQUIRE(cc && keep && in && out && V > 0 && N >= 0, "vx_cc_select: bad args (null pointer, V <= 0 or N < 0)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(vx_cc_grid((V + 255) / 256)), b(256);
    if (lab_bytes == 1) vx_cc_select_k<unsigned char><<<g, b, 0, st>>>(cc, keep, N, (const unsigned char*)in, (unsigned char*)out, V);
    else if (lab_bytes == 4) vx_cc_select_k<unsigned int><<<g, b, 0, st>>>(cc, keep, N, (const unsigned int*)in, (unsigned int*)out, V);
    else if (lab_bytes == 8) vx_cc_select_k<unsigned long long><<<g, b, 0, st>>>(cc, keep, N, (const unsigned long long*)in, (unsigned long long*)out, V);
    else VX_FAIL(-3, "vx_cc_select: label width %d bytes not supported", lab_bytes);
    VX_LAUNCH_CHECK("vx_cc_select");
    return 0;
}
