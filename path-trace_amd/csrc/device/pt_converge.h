/*
 * pt_converge.h -- the device side of pt_render_converge (include/pt/pt.h):
 * per-entry moments of the 32-sample block sums a render pass staged, the
 * round-end stopping decision, and the ordered compaction of the entries that
 * continue into the next round's lists.  Scene-independent: one module for
 * every scene (converge.cpp converge_module), compiled with the scene modules'
 * options -- no FMA contraction, correctly rounded f32 '/'.
 *
 * An entry is one position k of the call's initial pixel list (lists may
 * repeat a pixel, so all state is indexed by k, never by pixel).  A round
 * renders the active entries as slots 0 .. n-1; `home` maps a slot to its k
 * (null: slot == k, the first round) and `pix` to its pixel (null: slot).
 * Both lists ascend in k, and the compaction keeps that order.
 *
 *   pt_converge_reduce   one thread per slot, after every render pass
 *   pt_converge_scan     one workgroup, once per round
 *   pt_converge_scatter  one thread per slot, once per round with survivors
 *
 * No kernel waits on another workgroup and no atomic decides a position: the
 * reduce leaves one count per workgroup, the scan (a launch of its own) turns
 * them into offsets, the scatter ranks its lanes again and writes.
 */
typedef unsigned int ptc_u32;
typedef unsigned long long ptc_u64;

#define PTC_BLOCK 256 /* threads per workgroup of every kernel here (4 waves) */

struct PtConverge /* must match converge.cpp PtConvergeHost */
{
    const float *stage;    /* the render pass's staged values (mode 1: per sample, mode 2: per block) */
    const int *pix;        /* slot -> pixel index, or null                                            */
    const int *home;       /* slot -> entry k, or null                                                */
    long long n;           /* active slots                                                            */
    int nsamp;             /* samples per slot in this pass                                           */
    int mode;              /* pt_reduce's: 1 per-sample stage, 2 block stage                          */
    int first;             /* the call's first pass: the entry's state starts from zero               */
    int last;              /* the round's last pass: decide                                           */
    int cap;               /* the sample cap (p->spp)                                                 */
    float rel_tol, abs_tol;
    float *acc;            /* [3k] running f32 sums, pt_reduce's accumulation                         */
    double *mom;           /* [2k] s1, s2 of the block luminance sums                                 */
    int *blocks;           /* [k]  m, blocks so far                                                   */
    float *rgb;            /* [3k] out                                                                */
    int *spp;              /* [k]  out                                                                */
    float *err;            /* [k]  out                                                                */
    int *keep;             /* [slot] 1 = the entry continues                                          */
    ptc_u32 *wg_keep;      /* [workgroup] entries that continue                                       */
    ptc_u32 *wg_capped;    /* [workgroup] entries that stopped only because they reached the cap      */
    ptc_u32 *wg_off;       /* [workgroup] exclusive scan of wg_keep                                   */
    ptc_u64 *word;         /* [0] survivors, [1] capped: what the host reads once per round           */
    int nwg;               /* workgroups of the reduce / scatter grid                                 */
    int *pix_next;         /* the next round's lists                                                  */
    int *home_next;
};

/* pt_device.h pt_tree32, restated: the 32-leaf pairwise tree of one block,
 * missing leaves -0.0f */
__device__ __forceinline__ float pt_tree32(const float *v, int n, int stride)
{
    float b[32];
#pragma unroll
    for (int k = 0; k < 32; k++)
        b[k] = k < n ? v[k * stride] : -0.0f;
#pragma unroll
    for (int w = 1; w < 32; w *= 2)
#pragma unroll
        for (int k = 0; k < 32; k += 2 * w)
            b[k] = b[k] + b[k + w];
    return b[0];
}

/* set bits of the wave-uniform mask m in the lanes below this one (v_mbcnt) */
__device__ __forceinline__ int ptc_mbcnt(ptc_u64 m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((ptc_u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((ptc_u32)m, 0u));
}

/* One block of an entry: pt_reduce's f32 accumulation, and the moments of the
 * block's luminance sum in f64 */
struct PtcEntry
{
    float ax, ay, az;
    double s1, s2;
    int m;
};
__device__ __forceinline__ void ptc_block(PtcEntry &e, float br, float bg, float bb)
{
    e.ax = e.ax + br;
    e.ay = e.ay + bg;
    e.az = e.az + bb;
    const float y = (br + bg) + bb;
    const double yd = (double)y;
    e.s1 = e.s1 + yd;
    e.s2 = e.s2 + yd * yd;
    e.m = e.m + 1;
}

extern "C" __global__ __launch_bounds__(PTC_BLOCK) void pt_converge_reduce(PtConverge a)
{
    __shared__ ptc_u32 wave_keep[PTC_BLOCK / 64], wave_capped[PTC_BLOCK / 64];
    const long long slot = (long long)blockIdx.x * PTC_BLOCK + threadIdx.x;
    bool keep = false, capped = false;
    if (slot < a.n) {
        const long long k = a.home ? (long long)a.home[slot] : slot;
        PtcEntry e;
        e.ax = e.ay = e.az = 0.0f;
        e.s1 = e.s2 = 0.0;
        e.m = 0;
        if (!a.first) {
            e.ax = a.acc[3 * k + 0], e.ay = a.acc[3 * k + 1], e.az = a.acc[3 * k + 2];
            e.s1 = a.mom[2 * k + 0], e.s2 = a.mom[2 * k + 1];
            e.m = a.blocks[k];
        }
        if (a.mode == 2) {
            const int nb = a.nsamp >> 5;
            const float *p = a.stage + 3 * slot * (long long)nb;
            for (int b = 0; b < nb; b++) ptc_block(e, p[3 * b + 0], p[3 * b + 1], p[3 * b + 2]);
        } else {
            const float *p = a.stage + 3 * slot * (long long)a.nsamp;
            for (int s = 0; s < a.nsamp; s += 32) {
                const int n = a.nsamp - s < 32 ? a.nsamp - s : 32;
                const float br = pt_tree32(p + 3 * s + 0, n, 3);
                const float bg = pt_tree32(p + 3 * s + 1, n, 3);
                const float bb = pt_tree32(p + 3 * s + 2, n, 3);
                ptc_block(e, br, bg, bb);
            }
        }
        if (a.last) {
            /* the round-end decision: the standard error of the mean of the m
             * block sums against the tolerance, all in f64 */
            const int n = 32 * e.m;
            const double md = (double)e.m;
            bool stop;
            float err;
            if (!__builtin_isfinite(e.s1) || !__builtin_isfinite(e.s2)) {
                stop = true; /* more samples cannot repair it */
                err = __builtin_nanf("");
            } else {
                const double d = e.s2 - (e.s1 * e.s1) / md;
                const double v = d > 0.0 ? d : 0.0;
                const double e2 = v / (md * (md - 1.0));
                const double ta = 32.0 * (double)a.abs_tol;
                const double tr = (double)a.rel_tol * __builtin_fabs(e.s1 / md);
                const double t = ta > tr ? ta : tr;
                const bool met = e2 <= t * t;
                stop = met || n >= a.cap;
                capped = !met && n >= a.cap;
                err = (float)(__builtin_sqrt(e2) / 32.0);
            }
            if (stop) {
                const float fn = (float)n;
                a.rgb[3 * k + 0] = e.ax / fn;
                a.rgb[3 * k + 1] = e.ay / fn;
                a.rgb[3 * k + 2] = e.az / fn;
                a.spp[k] = n;
                a.err[k] = err;
            }
            keep = !stop;
            a.keep[slot] = keep ? 1 : 0;
        }
        if (keep || !a.last) {
            a.acc[3 * k + 0] = e.ax, a.acc[3 * k + 1] = e.ay, a.acc[3 * k + 2] = e.az;
            a.mom[2 * k + 0] = e.s1, a.mom[2 * k + 1] = e.s2;
            a.blocks[k] = e.m;
        }
    }
    if (!a.last)
        return; /* uniform over the grid */
    const ptc_u64 bk = __ballot(keep), bc = __ballot(capped);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wave_keep[wave] = (ptc_u32)__popcll(bk);
        wave_capped[wave] = (ptc_u32)__popcll(bc);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ptc_u32 nk = 0, nc = 0;
        for (int w = 0; w < PTC_BLOCK / 64; w++) nk += wave_keep[w], nc += wave_capped[w];
        a.wg_keep[blockIdx.x] = nk;
        a.wg_capped[blockIdx.x] = nc;
    }
}

/* Exclusive scan of the per-workgroup counts, by one workgroup: tiles of
 * PTC_BLOCK counts, each a Hillis-Steele scan in LDS, the running total
 * carried from tile to tile. */
extern "C" __global__ __launch_bounds__(PTC_BLOCK) void pt_converge_scan(PtConverge a)
{
    __shared__ ptc_u32 buf[2][PTC_BLOCK];
    __shared__ ptc_u32 cap_sum[PTC_BLOCK];
    const int t = threadIdx.x;
    ptc_u64 carry = 0;
    ptc_u32 capped = 0;
    for (int base = 0; base < a.nwg; base += PTC_BLOCK) {
        const int i = base + t;
        const ptc_u32 v = i < a.nwg ? a.wg_keep[i] : 0u;
        if (i < a.nwg)
            capped += a.wg_capped[i];
        int cur = 0;
        buf[0][t] = v;
        __syncthreads();
        for (int d = 1; d < PTC_BLOCK; d *= 2) {
            const ptc_u32 x = buf[cur][t] + (t >= d ? buf[cur][t - d] : 0u);
            buf[cur ^ 1][t] = x;
            cur ^= 1;
            __syncthreads();
        }
        const ptc_u32 incl = buf[cur][t];
        const ptc_u32 total = buf[cur][PTC_BLOCK - 1];
        if (i < a.nwg)
            a.wg_off[i] = (ptc_u32)carry + (incl - v);
        carry += total;
        __syncthreads(); /* buf is written again by the next tile */
    }
    cap_sum[t] = capped;
    __syncthreads();
    for (int d = PTC_BLOCK / 2; d > 0; d /= 2) {
        if (t < d)
            cap_sum[t] += cap_sum[t + d];
        __syncthreads();
    }
    if (t == 0) {
        a.word[0] = carry;
        a.word[1] = (ptc_u64)cap_sum[0];
    }
}

/* The entries that continue, in slot order, into the next round's lists: a
 * lane's position is its workgroup's offset + the keeps of the waves before
 * its own + the keeps of the lanes below it. */
extern "C" __global__ __launch_bounds__(PTC_BLOCK) void pt_converge_scatter(PtConverge a)
{
    __shared__ ptc_u32 wave_keep[PTC_BLOCK / 64];
    const long long slot = (long long)blockIdx.x * PTC_BLOCK + threadIdx.x;
    const bool keep = slot < a.n && a.keep[slot] != 0;
    const ptc_u64 bk = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        wave_keep[wave] = (ptc_u32)__popcll(bk);
    __syncthreads();
    if (!keep)
        return;
    ptc_u32 at = a.wg_off[blockIdx.x];
    for (int w = 0; w < wave; w++) at += wave_keep[w];
    at += (ptc_u32)ptc_mbcnt(bk);
    a.pix_next[at] = a.pix ? a.pix[slot] : (int)slot;
    a.home_next[at] = a.home ? a.home[slot] : (int)slot;
}
