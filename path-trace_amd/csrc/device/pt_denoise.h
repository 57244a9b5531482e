/*
 * pt_denoise.h -- the device side of pt_denoise (include/pt/pt.h): an
 * edge-avoiding a-trous wavelet filter with variance guidance (Dammertz et al.
 * 2010; the spatial part of Schied et al. 2017) over a frame, its per-pixel error
 * estimate (pt_render_converge's err) and its guide buffers (pt_render_guides).
 * Scene-independent: one module for every scene (denoise.cpp), compiled with the
 * scene modules' options -- no FMA contraction, correctly rounded f32 '/' and
 * sqrt, denormals kept -- and free of transcendental functions, so that
 * tests/denoise_model.py restates it in numpy float32 bit for bit: every
 * expression below is one rounded operation per operator, in the order written.
 *
 *   ptd_prepare   packs each pixel into two 16-byte records: (signal rgb,
 *                 variance) and (unit normal, depth); the material plane is
 *                 read where it lies
 *   ptd_atrous    one pass: 5 x 5 taps `step` pixels apart, from one (signal,
 *                 variance) buffer into the other
 *   ptd_finalise  the image (and the variance) back out of the records
 *
 * A wave takes 64 consecutive x of one row, so every tap of every step is one
 * contiguous 16-byte-per-lane load per record (q = p + a constant); a workgroup
 * takes four rows, a tile of 64 x 4 pixels.  A lane past the row's end, or a
 * wave past the last row, works on the last pixel of its row or column with its
 * stores predicated off.  No LDS, no atomics, and no kernel waits on another
 * workgroup.
 *
 * PTD_LDS_TILE is the one probe define (tools/denoise_probe.py; denoise.cpp
 * sets it from PT_DENOISE_LDS_TILE, and nothing else does): the passes of step 1
 * and 2 stage their tile and its halo in LDS.  It computes the same bits; it
 * took 7 % less time on those two passes and 20 % more on the others (DESIGN.md
 * s7e), so it is not the form that ships.
 */
#define PTD_BLOCK 256 /* threads per workgroup of every kernel here (4 waves) */

struct __attribute__((aligned(16))) PtdRec
{
    float x, y, z, w;
};

struct PtDenoise /* must match denoise.cpp PtDenoiseHost */
{
    int W, H;
    int step;  /* ptd_atrous: the tap spacing of this pass                         */
    int demod; /* divide the albedo and the emission out, and put them back        */
    int npow;  /* the normal weight is squared this many times                     */
    int pad_;
    float sigma_l, sigma_z;
    const float *rgb;      /* [3p] the beauty image                                */
    const float *err;      /* [p]  its standard error, or null                     */
    const float *normal;   /* [3p]                                                 */
    const float *t;        /* [p]                                                  */
    const float *albedo;   /* [3p] read only with demod                            */
    const float *emission; /* [3p] read only with demod                            */
    const int *material;   /* [p]  -1 = a miss                                     */
    const PtdRec *sv_in;   /* (signal rgb, variance): what a pass reads and ptd_finalise ends on */
    PtdRec *sv_out;        /* ... and what ptd_prepare and a pass write            */
    PtdRec *geo;           /* (unit normal, depth)                                 */
    float *out;            /* [3p] may be rgb itself                               */
    float *var_out;        /* [p]  or null                                         */
};

struct PtdPix
{
    int x, y;
    int x0, y0; /* the tile's first pixel */
    bool live;
};

/* this lane's pixel: workgroup b is tile b % segs of tile row b / segs, wave k its row k */
__device__ __forceinline__ PtdPix ptd_pixel(int W, int H)
{
    const unsigned segs = ((unsigned)W + 63u) >> 6;
    PtdPix p;
    p.x0 = (int)(blockIdx.x % segs) * 64;
    p.y0 = (int)(blockIdx.x / segs) * 4; /* < H: the host launches segs * ceil(H / 4) workgroups */
    const int x = p.x0 + (int)(threadIdx.x & 63), y = p.y0 + (int)(threadIdx.x >> 6);
    p.live = x < W && y < H;
    p.x = x < W ? x : W - 1;
    p.y = y < H ? y : H - 1;
    return p;
}

__device__ __forceinline__ int ptd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

/* E(x) = (1 - x)^2 below 1, else 0; a NaN gives 0 */
__device__ __forceinline__ float ptd_edge(float x)
{
    const float u = 1.0f - x;
    return x < 1.0f ? u * u : 0.0f;
}

/* the albedo the signal is divided by, per channel, and its mean */
__device__ __forceinline__ void ptd_albedo(const PtDenoise &a, long long p, float &ar, float &ag, float &ab,
                                           float &abar)
{
    ar = ag = ab = abar = 1.0f;
    if (a.demod) {
        const float r = a.albedo[3 * p], g = a.albedo[3 * p + 1], b = a.albedo[3 * p + 2];
        ar = r > 0.01f ? r : 0.01f;
        ag = g > 0.01f ? g : 0.01f;
        ab = b > 0.01f ? b : 0.01f;
        abar = ((ar + ag) + ab) / 3.0f;
    }
}

/* the signal of pixel p: (rgb - emission) / albedo, or rgb itself without demod */
__device__ __forceinline__ void ptd_signal(const PtDenoise &a, long long p, float &sr, float &sg, float &sb)
{
    sr = a.rgb[3 * p], sg = a.rgb[3 * p + 1], sb = a.rgb[3 * p + 2];
    if (a.demod) {
        float ar, ag, ab, abar;
        ptd_albedo(a, p, ar, ag, ab, abar);
        sr = (sr - a.emission[3 * p]) / ar;
        sg = (sg - a.emission[3 * p + 1]) / ag;
        sb = (sb - a.emission[3 * p + 2]) / ab;
    }
}

extern "C" __global__ __launch_bounds__(PTD_BLOCK) void ptd_prepare(PtDenoise a)
{
    const PtdPix px = ptd_pixel(a.W, a.H);
    const long long p = (long long)px.y * a.W + px.x;
    float ar, ag, ab, abar;
    ptd_albedo(a, p, ar, ag, ab, abar);
    PtdRec s;
    ptd_signal(a, p, s.x, s.y, s.z);
    if (a.err) { /* a launch argument: uniform */
        const float e = a.err[p];
        s.w = __builtin_isfinite(e) ? (e * e) / (abar * abar) : 0.0f;
    } else {
        /* the sample variance of the signal's luminance over the 5 x 5 pixels
         * around p that are in the image, share p's material and are finite */
        const int mp = a.material[p];
        float yv[25];
        bool ok[25];
        float n = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 25; k++) {
            const int qy = px.y + (k / 5 - 2), qx = px.x + (k % 5 - 2);
            const bool in = qy >= 0 && qy < a.H && qx >= 0 && qx < a.W;
            const long long q = (long long)ptd_clamp(qy, a.H - 1) * a.W + ptd_clamp(qx, a.W - 1);
            float r, g, b;
            ptd_signal(a, q, r, g, b);
            yv[k] = (r + g) + b;
            ok[k] = in && a.material[q] == mp && __builtin_isfinite(yv[k]);
            if (ok[k]) {
                n = n + 1.0f;
                s1 = s1 + yv[k];
            }
        }
        const float mean = s1 / n;
        float s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 25; k++) {
            const float d = yv[k] - mean;
            if (ok[k])
                s2 = s2 + d * d;
        }
        s.w = n >= 2.0f ? s2 / (n - 1.0f) : 0.0f;
    }
    const float nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
    const float n2 = (nx * nx + ny * ny) + nz * nz;
    PtdRec g;
    g.x = g.y = g.z = 0.0f;
    if (n2 > 0.0f) {
        const float l = __builtin_sqrtf(n2);
        g.x = nx / l, g.y = ny / l, g.z = nz / l;
    }
    g.w = a.t[p];
    if (!px.live)
        return;
    a.sv_out[p] = s;
    a.geo[p] = g;
}

extern "C" __global__ __launch_bounds__(PTD_BLOCK) void ptd_atrous(PtDenoise a)
{
    const PtdPix px = ptd_pixel(a.W, a.H);
    const long long p = (long long)px.y * a.W + px.x;
#ifdef PTD_LDS_TILE
    /* the tile and a halo of 2 * step pixels, coordinates clamped: what the
     * taps below would load from memory, pixel for pixel */
    __shared__ PtdRec l_sv[72 * 12], l_geo[72 * 12];
    __shared__ int l_mat[72 * 12];
    const bool tile = a.step <= 2; /* uniform */
    const int halo = 2 * a.step, tw = 64 + 2 * halo, th = 4 + 2 * halo;
    if (tile) {
        for (int i = threadIdx.x; i < tw * th; i += PTD_BLOCK) {
            const long long q = (long long)ptd_clamp(px.y0 - halo + i / tw, a.H - 1) * a.W +
                                ptd_clamp(px.x0 - halo + i % tw, a.W - 1);
            l_sv[i] = a.sv_in[q], l_geo[i] = a.geo[q], l_mat[i] = a.material[q];
        }
        __syncthreads();
    }
#define PTD_FETCH(qy, qx, S, G, M)                                                                     \
    do {                                                                                               \
        if (tile) {                                                                                    \
            const int li_ = ((qy) - (px.y0 - halo)) * tw + ((qx) - (px.x0 - halo));                    \
            S = l_sv[li_], G = l_geo[li_], M = l_mat[li_];                                             \
        } else {                                                                                       \
            const long long q_ = (long long)ptd_clamp(qy, a.H - 1) * a.W + ptd_clamp(qx, a.W - 1);     \
            S = a.sv_in[q_], G = a.geo[q_], M = a.material[q_];                                        \
        }                                                                                              \
    } while (0)
#else
#define PTD_FETCH(qy, qx, S, G, M)                                                                     \
    do {                                                                                               \
        const long long q_ = (long long)ptd_clamp(qy, a.H - 1) * a.W + ptd_clamp(qx, a.W - 1);         \
        S = a.sv_in[q_], G = a.geo[q_], M = a.material[q_];                                            \
    } while (0)
#endif
    PtdRec sp, gp;
    int mp;
    PTD_FETCH(px.y, px.x, sp, gp, mp);
    const float yp = (sp.x + sp.y) + sp.z;

    /* the 3 x 3 Gaussian of the variance around p, coordinates clamped; a
     * neighbour of another material counts as p itself, so that nothing
     * crosses a material edge */
    float vt = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int dy = k / 3 - 1, dx = k % 3 - 1;
        const float g = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
        PtdRec sq, gq;
        int mq;
        PTD_FETCH(px.y + dy, px.x + dx, sq, gq, mq);
        (void)gq;
        vt = vt + g * (mq == mp ? sq.w : sp.w);
    }
    const float den = a.sigma_l * __builtin_sqrtf(vt > 0.0f ? vt : 0.0f) + 1e-4f;
    /* sigma_l = +inf switches the luminance weight off exactly: every finite
     * difference weighs 1 (inf * 0 above is a NaN, so the quotient is not used) */
    const bool lum_off = a.sigma_l == __builtin_inff();

    float cr = 0.0f, cg = 0.0f, cb = 0.0f, sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int k = 0; k < 25; k++) {
        const int dy = k / 5 - 2, dx = k % 5 - 2;
        const float kk[3] = {0.375f, 0.25f, 0.0625f};
        const float h = kk[dy < 0 ? -dy : dy] * kk[dx < 0 ? -dx : dx];
        float w;
        PtdRec sq;
        if (k == 12) {
            w = h; /* the centre: 9/64 */
            sq = sp;
        } else {
            const int qy = px.y + a.step * dy, qx = px.x + a.step * dx;
            const bool in = qy >= 0 && qy < a.H && qx >= 0 && qx < a.W;
            PtdRec gq;
            int mq;
            PTD_FETCH(qy, qx, sq, gq, mq);
            float wn = 1.0f, wz = 1.0f;
            if (mp != -1) {
                const float dot = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                wn = dot > 0.0f ? dot : 0.0f;
                for (int i = 0; i < a.npow; i++) wn = wn * wn;
                const float d = __builtin_fabsf(gp.w - gq.w);
                const float tm = gp.w > gq.w ? gp.w : gq.w;
                wz = d > 0.0f ? ptd_edge(d / (a.sigma_z * tm)) : 1.0f;
            }
            const float dl = __builtin_fabsf(yp - ((sq.x + sq.y) + sq.z));
            const float wl = lum_off ? (dl < __builtin_inff() ? 1.0f : 0.0f) : ptd_edge(dl / den);
            w = ((h * wn) * wz) * wl;
            if (!(in && mq == mp))
                w = 0.0f;
        }
        /* a tap without weight is left out, not multiplied by zero */
        if (w > 0.0f) {
            cr = cr + w * sq.x;
            cg = cg + w * sq.y;
            cb = cb + w * sq.z;
            sv = sv + (w * w) * sq.w;
            sw = sw + w;
        }
    }
    if (!px.live)
        return;
    PtdRec o;
    o.x = cr / sw, o.y = cg / sw, o.z = cb / sw;
    o.w = sv / (sw * sw);
    a.sv_out[p] = o;
#undef PTD_FETCH
}

extern "C" __global__ __launch_bounds__(PTD_BLOCK) void ptd_finalise(PtDenoise a)
{
    const PtdPix px = ptd_pixel(a.W, a.H);
    const long long p = (long long)px.y * a.W + px.x;
    const PtdRec s = a.sv_in[p];
    float r = s.x, g = s.y, b = s.z, v = s.w;
    if (a.demod) {
        float ar, ag, ab, abar;
        ptd_albedo(a, p, ar, ag, ab, abar);
        r = a.emission[3 * p] + r * ar;
        g = a.emission[3 * p + 1] + g * ag;
        b = a.emission[3 * p + 2] + b * ab;
        v = v * (abar * abar);
    }
    if (!px.live)
        return;
    a.out[3 * p] = r, a.out[3 * p + 1] = g, a.out[3 * p + 2] = b;
    if (a.var_out)
        a.var_out[p] = v;
}
