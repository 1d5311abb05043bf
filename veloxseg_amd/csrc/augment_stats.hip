// Per-channel statistics for the batch-assembly programs: min, max, S1 = sum x, S2 = sum x^2 of what a record's program gives up to a step,
// left in the record's DEVICE statistics table, where ops 4..6 of the step program (augment_steps.h) read them.  Nothing visits the host and no workgroup waits for
// another: pass 1 reduces fixed chunks of VX_AUG_STAT_CHUNK voxels to partials, pass 2 (a second launch) folds a job's partials in index order.  Voxel -> lane ->
// chunk and the fold order depend on V alone, and every sum is carried in fp64 in a fixed order: a channel's statistics have the same bits in every run, on every
// rank, alone or among other records.  min / max go through fminf / fmaxf (a NaN voxel is skipped there); the sums take every voxel (a NaN or inf voxel makes
// mean and std NaN).
#include "augment_steps.h"

#define VX_AUG_GLOBAL __attribute__((address_space(1)))
struct VxAugStatJob { int rec, upto, slot, frame; };
struct VxAugPartial { double s1, s2; float mn, mx; };
static_assert(sizeof(VxAugStatJob) == VX_AUG_STAT_JOB_BYTES, "job layout drifted from the header");
static_assert(sizeof(VxAugPartial) == VX_AUG_STAT_PARTIAL_BYTES, "partial layout drifted from the header");

// fold the 256 lanes' (s1, s2, mn, mx) in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ void vx_aug_stat_fold(double& s1, double& s2, float& mn, float& mx, double (*sm)[256], float (*sf)[256]) {
    const int t = threadIdx.x;
    sm[0][t] = s1; sm[1][t] = s2; sf[0][t] = mn; sf[1][t] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            sm[0][t] += sm[0][t + o];
            sm[1][t] += sm[1][t + o];
            sf[0][t] = fminf(sf[0][t], sf[0][t + o]);
            sf[1][t] = fmaxf(sf[1][t], sf[1][t + o]);
        }
        __syncthreads();
    }
    s1 = sm[0][0]; s2 = sm[1][0]; mn = sf[0][0]; mx = sf[1][0];
}

// grid = n_jobs x nchunk blocks; block (job, chunk) reduces voxels chunk * CHUNK .. + CHUNK - 1 of the job's frame: lane t takes chunk * CHUNK + i * 256 + t, i ascending
__global__ void __launch_bounds__(256) vx_augment_stats_partial_k(const VxAugRecord* __restrict__ recs, int n_records, const VxAugStatJob* __restrict__ jobs,
                                                                  VxAugPartial* __restrict__ partials, int D, int H, int W, int nchunk) {
    __shared__ double sm[2][256];
    __shared__ float sf[2][256];
    const int j = (int)(blockIdx.x / (unsigned)nchunk), chunk = (int)(blockIdx.x % (unsigned)nchunk);
    const VxAugStatJob job = jobs[j];
    if (job.rec < 0 || job.rec >= n_records) return;                             // uniform over the block
    const VxAugRecord* __restrict__ R = recs + job.rec;
    if (R->dtype != 0 || R->stats == nullptr || job.slot < 0) return;
    const int ns = min(max(min(job.upto, R->n_steps), 0), VX_AUG_MAX_STEPS);
    const int fm = job.frame & 7, sf_mask = (R->flip ^ fm) & 7;                  // flips between the source and the frame the statistic is taken in
    const long V = (long)D * H * W;
    double s1 = 0.0, s2 = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < VX_AUG_STAT_CHUNK / 256; ++i) {
        const long v = (long)chunk * VX_AUG_STAT_CHUNK + i * 256 + threadIdx.x;
        if (v < V) {
            int d, h, w;
            vx_aug_coords(v, V, H, W, d, h, w);
            const int sd = (sf_mask & 1) ? D - 1 - d : d, sh = (sf_mask & 2) ? H - 1 - h : h, sw = (sf_mask & 4) ? W - 1 - w : w;
            float t[1];
            t[0] = ((const VX_AUG_GLOBAL float*)(static_cast<const float*>(R->src) + sd * R->stride[0] + sh * R->stride[1] + sw * R->stride[2]))[0];
            vx_aug_run_steps<1, true>(R, ns, t, d, h, w, D, H, W, V, fm);
            const double x = (double)t[0];
            s1 += x;
            s2 += x * x;
            mn = fminf(mn, t[0]);
            mx = fmaxf(mx, t[0]);
        }
    }
    vx_aug_stat_fold(s1, s2, mn, mx, sm, sf);
    if (threadIdx.x == 0) {
        VxAugPartial p;
        p.s1 = s1; p.s2 = s2; p.mn = mn; p.mx = mx;
        partials[(long)j * nchunk + chunk] = p;
    }
}

// grid = n_jobs blocks: lane t folds partials t, t + 256, ... in ascending order, then the tree; thread 0 writes the slot
__global__ void __launch_bounds__(256) vx_augment_stats_final_k(const VxAugRecord* __restrict__ recs, int n_records, const VxAugStatJob* __restrict__ jobs,
                                                                const VxAugPartial* __restrict__ partials, long V, int nchunk) {
    __shared__ double sm[2][256];
    __shared__ float sf[2][256];
    const int j = (int)blockIdx.x;
    const VxAugStatJob job = jobs[j];
    if (job.rec < 0 || job.rec >= n_records) return;
    const VxAugRecord* __restrict__ R = recs + job.rec;
    if (R->dtype != 0 || R->stats == nullptr || job.slot < 0) return;
    double s1 = 0.0, s2 = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int p = threadIdx.x; p < nchunk; p += 256) {
        const VxAugPartial q = partials[(long)j * nchunk + p];
        s1 += q.s1; s2 += q.s2; mn = fminf(mn, q.mn); mx = fmaxf(mx, q.mx);
    }
    vx_aug_stat_fold(s1, s2, mn, mx, sm, sf);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double n = (double)V;
        const double var = (s2 - s1 * s1 / n) / (n - 1.0);                       // torch's unbiased std; V = 1 gives NaN, as torch does
        VxAugStat o;
        o.mn = mn; o.mx = mx; o.mean = (float)(s1 / n); o.sd = (float)sqrt(var < 0.0 ? 0.0 : var);
        o.s1 = s1; o.s2 = s2;
        const_cast<VxAugStat*>(R->stats)[job.slot] = o;
    }
}

extern "C" int vx_augment_stats(const void* records, int n_records, const void* jobs, int n_jobs, void* partials, long partial_bytes, int D, int H, int W, void* stream) {
    VX_REQUIRE(records && jobs && partials, "vx_augment_stats: null pointer (records %p, jobs %p, partials %p)", records, jobs, partials);
    VX_REQUIRE(n_records > 0 && n_jobs > 0, "vx_augment_stats: no records or no jobs (n_records %d, n_jobs %d)", n_records, n_jobs);
    VX_REQUIRE(D > 0 && H > 0 && W > 0, "vx_augment_stats: non-positive extent (D %d, H %d, W %d)", D, H, W);
    VX_REQUIRE(((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(jobs) | reinterpret_cast<uintptr_t>(partials)) & 7) == 0,
               "vx_augment_stats: misaligned table, job list or partials (8 bytes)");
    const long V = (long)D * H * W;
    const long nchunk = (V + VX_AUG_STAT_CHUNK - 1) / VX_AUG_STAT_CHUNK;
    VX_REQUIRE(nchunk * (long)n_jobs <= 0x7fffffffL, "vx_augment_stats: %ld chunks x %d jobs exceed one grid", nchunk, n_jobs);
    VX_REQUIRE(partial_bytes >= nchunk * (long)n_jobs * VX_AUG_STAT_PARTIAL_BYTES, "vx_augment_stats: partials hold %ld bytes, %ld needed", partial_bytes,
               nchunk * (long)n_jobs * VX_AUG_STAT_PARTIAL_BYTES);
    hipStream_t st = (hipStream_t)stream;
    const VxAugRecord* recs = static_cast<const VxAugRecord*>(records);
    const VxAugStatJob* jb = static_cast<const VxAugStatJob*>(jobs);
    vx_augment_stats_partial_k<<<dim3((unsigned)(nchunk * n_jobs)), dim3(256), 0, st>>>(recs, n_records, jb, static_cast<VxAugPartial*>(partials), D, H, W, (int)nchunk);
    VX_LAUNCH_CHECK("vx_augment_stats (partials)");
    vx_augment_stats_final_k<<<dim3((unsigned)n_jobs), dim3(256), 0, st>>>(recs, n_records, jb, static_cast<const VxAugPartial*>(partials), V, (int)nchunk);
    VX_LAUNCH_CHECK("vx_augment_stats (fold)");
    return 0;
}
