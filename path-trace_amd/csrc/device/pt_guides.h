/*
 * pt_guides.h -- what traceRay sees at the first surface, served two ways:
 * first-hit queries for caller rays (pt_query_hits) and per-pixel guide buffers
 * beside the beauty image (pt_render_guides).
 *
 * Appended by codegen.cpp to a module kind of its own, after device/pt_device.h
 * and the scene's full `ptgen::Scene` (root type and material dispatchers); no
 * other module kind carries it, so their text and code-object keys do not know
 * it exists.  Both kernels run one entry per lane with no LDS and no atomics,
 * under the scene modules' compiler options (no FMA contraction, correctly
 * rounded '/' and sqrt, denormals kept), and state traceRay's first steps
 * (include/path-trace.h:66-129) with the device library's own functions:
 *
 *   query     PT_HIT_MERGE: first_hit<Root>, the lazy merge -- traceRay's scan
 *             (path-trace.h:66-100);
 *             PT_HIT_FAST: Root::span into PrimSpans, then span_first_hit<Root>,
 *             and first_hit_ps<Root> on the lanes where the check's verdict is
 *             false -- what the spine and lane queries of the render kernel run.
 *             Both give the same bits; `decided` is the check's verdict.
 *   normal    Root::normal(ref_prim, t, o, d, e), negated if the ref carries
 *             FLIP, negated again on an exit: what traceRay shades with.
 *   pos       o + t * d.
 *   shading   the material's five lookups at pos (path-trace.h:101-129),
 *             unclamped: emis, refl, trans (colours), scat, trc (floats).
 *
 * No lane leaves before a cross-lane operation (prep_l, span_first_hit and the
 * exact-division fallbacks ballot through wave_any): a lane past the end takes
 * the last entry's work and its stores are predicated off.
 */
#ifndef PT_GUIDES_H
#define PT_GUIDES_H

/* the query paths of pt_hits (include/pt/pt.h has the same values) */
#define PT_HIT_FAST 0
#define PT_HIT_MERGE 1

namespace ptd
{

/* the first hit of one ray: valid fields only where hit */
struct GuideHit
{
    bool hit, ex;
    int decided; /* the fast check's verdict (0 on the merge path) */
    float t;
    u32 ref;
};

template <class R>
__device__ __forceinline__ GuideHit guide_query(const typename R::Ctx &ctx, V3 d, const Env &e, int path)
{
    GuideHit h;
    h.hit = false, h.ex = false, h.decided = 0, h.t = 0.0f, h.ref = 0u;
    if (path == PT_HIT_MERGE) { /* a launch argument: wave-uniform */
        h.hit = first_hit<R>(ctx, d, e, h.t, h.ref, h.ex);
    } else {
        PrimSpans<R::HI> ps;
        R::span(ps, ctx, mkray(d), e);
        const int fok = span_first_hit<R>(ps, h.hit, h.t, h.ref, h.ex);
        h.decided = fok ? 1 : 0;
        if (wave_any(!fok)) {
            if (!fok)
                h.hit = first_hit_ps<R>(ps, h.t, h.ref, h.ex);
        }
    }
    return h;
}

/* the normal traceRay shades with (path-trace.h:84-96) */
template <class R>
__device__ __forceinline__ V3 guide_normal(const GuideHit &h, V3 o, V3 d, const Env &e)
{
    V3 nn = R::normal(ref_prim(h.ref), h.t, o, d, e);
    if (h.ref & FLIP)
        nn = -nn;
    return h.ex ? -nn : nn;
}

/* pt_query_hits: one ray per lane (6 floats: origin, unnormalised direction),
 * planar outputs; on a miss every int field is 0, the material -1 and every
 * float +0.  shade (11 floats per ray: emis rgb, refl rgb, trans rgb, scat,
 * trc) may be null. */
template <class S>
__device__ __forceinline__ void hits(const Env &e, const float *__restrict__ rays, long long n, int path,
                                     int *__restrict__ hit_o, int *__restrict__ exit_o, int *__restrict__ dec_o,
                                     int *__restrict__ mat_o, float *__restrict__ t_o, float *__restrict__ nrm_o,
                                     float *__restrict__ pos_o, float *__restrict__ ior_o,
                                     float *__restrict__ shade_o)
{
    typedef typename S::Root R;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const long long k = live ? i : n - 1; /* n >= 1 (the host launches nothing for n == 0) */
    const float *r = rays + 6 * k;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    typename R::Ctx ctx;
    R::prep_l(ctx, o, e);
    const GuideHit h = guide_query<R>(ctx, d, e, path);
    const V3 z = mk(0.0f, 0.0f, 0.0f);
    V3 nrm = z, pos = z, em = z, rc = z, tr = z;
    float t = 0.0f, ior = 0.0f, sc = 0.0f, trc = 0.0f;
    int mat = -1;
    if (h.hit) {
        t = h.t;
        mat = ref_mat(h.ref);
        pos = o + h.t * d;
        nrm = guide_normal<R>(h, o, d, e);
        ior = S::ior(mat, e);
        if (shade_o) {
            em = S::emis(mat, pos, e);
            rc = S::refl(mat, pos, e);
            tr = S::trans(mat, pos, e);
            sc = S::scat(mat, pos, e);
            trc = S::trc(mat, pos, e);
        }
    }
    if (!live)
        return;
    hit_o[k] = h.hit ? 1 : 0;
    exit_o[k] = h.hit && h.ex ? 1 : 0;
    dec_o[k] = h.decided;
    mat_o[k] = mat;
    t_o[k] = t;
    nrm_o[3 * k] = nrm.x, nrm_o[3 * k + 1] = nrm.y, nrm_o[3 * k + 2] = nrm.z;
    pos_o[3 * k] = pos.x, pos_o[3 * k + 1] = pos.y, pos_o[3 * k + 2] = pos.z;
    ior_o[k] = ior;
    if (shade_o) {
        float *q = shade_o + 11 * k;
        q[0] = em.x, q[1] = em.y, q[2] = em.z;
        q[3] = rc.x, q[4] = rc.y, q[5] = rc.z;
        q[6] = tr.x, q[7] = tr.y, q[8] = tr.z;
        q[9] = sc, q[10] = trc;
    }
}

/* pt_render_guides' launch: the camera of pt_render (PtLaunch's fields of the
 * same names) and the output planes, each optional (null = skip) */
struct PtGuideLaunch
{
    u64 seed;
    int W, H;
    float sw, sh, dist;
    int gw;  /* pixel index = py * gw + px */
    int s0;  /* first engine sample index */
    int spp; /* samples per entry */
    float *emission, *albedo, *normal, *t, *coverage;
    int *material; /* compact index of the first sample's hit, or -1 */
};

/* One pixel entry per lane, the sample loop inside the lane.  Sample s of pixel
 * pix draws its camera ray from the engine keyed (seed, pix, s) exactly as
 * pt_render does (rng_seed, then camera_dir's two draws); every quantity is
 * summed in f32 from +0 in sample order, acc = acc + x_s, a miss adding +0, and
 * divided by (float)spp at the end -- for the emission plane this is
 * tracePixel's own accumulation at rayDepth 0 (path-trace.h:192-199), where
 * traceRay returns the emission of the first hit (:97-108). */
template <class S>
__device__ __forceinline__ void guides(const Env &e, const int *__restrict__ pixels, long long n,
                                       const PtGuideLaunch &gl)
{
    typedef typename S::Root R;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const long long k = live ? i : n - 1;
    const int pix = pixels ? pixels[k] : (int)k;
    PtLaunch lp = {};
    lp.W = gl.W, lp.H = gl.H, lp.sw = gl.sw, lp.sh = gl.sh, lp.dist = gl.dist, lp.gw = gl.gw;
    const V3 z = mk(0.0f, 0.0f, 0.0f);
    const V3 o = z;
    typename R::Ctx ctx;
    R::prep_l(ctx, o, e);
    V3 aem = z, aal = z, anr = z;
    float at = 0.0f, acov = 0.0f;
    int mat0 = -1;
    for (int s = 0; s < gl.spp; s++) { /* wave-uniform trip count */
        Rng rng;
        rng_seed(rng, gl.seed, (u64)pix, (u64)(gl.s0 + s));
        const V3 d = camera_dir(lp, pix, rng);
        const GuideHit h = guide_query<R>(ctx, d, e, PT_HIT_FAST);
        V3 em = z, al = z, nr = z;
        float t = 0.0f, c = 0.0f;
        if (h.hit) {
            const int mat = ref_mat(h.ref);
            const V3 pos = o + h.t * d;
            t = h.t, c = 1.0f;
            if (s == 0)
                mat0 = mat;
            if (gl.normal)
                nr = guide_normal<R>(h, o, d, e);
            if (gl.emission)
                em = S::emis(mat, pos, e);
            if (gl.albedo)
                al = S::refl(mat, pos, e);
        }
        aem = aem + em, aal = aal + al, anr = anr + nr;
        at = at + t, acov = acov + c;
    }
    if (!live)
        return;
    const float spp = (float)gl.spp;
    if (gl.emission)
        gl.emission[3 * k] = aem.x / spp, gl.emission[3 * k + 1] = aem.y / spp, gl.emission[3 * k + 2] = aem.z / spp;
    if (gl.albedo)
        gl.albedo[3 * k] = aal.x / spp, gl.albedo[3 * k + 1] = aal.y / spp, gl.albedo[3 * k + 2] = aal.z / spp;
    if (gl.normal)
        gl.normal[3 * k] = anr.x / spp, gl.normal[3 * k + 1] = anr.y / spp, gl.normal[3 * k + 2] = anr.z / spp;
    if (gl.t)
        gl.t[k] = at / spp;
    if (gl.coverage)
        gl.coverage[k] = acov / spp;
    if (gl.material)
        gl.material[k] = mat0;
}

} // namespace ptd

#define PT_DEFINE_GUIDES(SCENE)                                                                             \
    extern "C" __global__ __launch_bounds__(256) void pt_hits(                                             \
        const float *__restrict__ P, const ptd::PtImage *__restrict__ imgs, const float *__restrict__ rays, \
        long long n, int path, int *__restrict__ hit_o, int *__restrict__ exit_o, int *__restrict__ dec_o, \
        int *__restrict__ mat_o, float *__restrict__ t_o, float *__restrict__ nrm_o,                        \
        float *__restrict__ pos_o, float *__restrict__ ior_o, float *__restrict__ shade_o)                 \
    {                                                                                                       \
        const ptd::Env e = {P, imgs};                                                                       \
        ptd::hits<SCENE>(e, rays, n, path, hit_o, exit_o, dec_o, mat_o, t_o, nrm_o, pos_o, ior_o, shade_o); \
    }                                                                                                       \
    extern "C" __global__ __launch_bounds__(256) void pt_guides(                                           \
        const float *__restrict__ P, const ptd::PtImage *__restrict__ imgs, const int *__restrict__ pixels, \
        long long n, ptd::PtGuideLaunch gl)                                                                 \
    {                                                                                                       \
        const ptd::Env e = {P, imgs};                                                                       \
        ptd::guides<SCENE>(e, pixels, n, gl);                                                               \
    }

#endif
