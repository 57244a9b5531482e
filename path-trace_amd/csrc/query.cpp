/* query.cpp -- the boundary's query calls (include/pt/pt.h): pt_query_spans and
 * pt_tex_eval over a query module (codegen.cpp generate_query), pt_query_hits
 * and pt_render_guides over the guides module (device/pt_guides.h).  Each call
 * restores the caller's current device. */
#include <algorithm>
#include <climits>
#include <cstring>

#include "device_state.h"

namespace pt
{
namespace
{

/* A query or guides module loaded on one device with its own copy of the
 * parameters and images; everything is released with it.  A scene keeps
 * the modules it has served (SceneImpl::qcache): a scene only grows, so a
 * module whose source key, parameters and image slots match is the same
 * module, and the facade's per-ray / per-point virtuals (SpanIterator::init,
 * Texture::getColor) reuse it instead of loading a code object per call. */
struct QueryModule
{
    int device;
    Module mod;
    SceneUpload up;
    QueryModule(const SceneImpl &s, const Generated &g, int dev) : device(dev)
    {
        const std::vector<char> &code = code_object(g);
        HIPCHECK(hipSetDevice(device));
        mod.load(code);
        up.sync(s, g);
    }
};

} // namespace

/* the scene's loaded query modules, by (source key, device) */
struct QueryCache
{
    std::map<std::pair<std::string, int>, std::unique_ptr<QueryModule, OnDevice>> mods;
};

namespace
{

QueryModule &query_module(SceneImpl &s, const Generated &g, int device)
{
    if (!s.qcache)
        s.qcache = std::shared_ptr<QueryCache>(new QueryCache);
    auto &q = s.qcache->mods[{g.key, device}];
    if (q && (q->up.params != g.params || q->up.image_ids != g.image_ids))
        q.reset();
    if (!q)
        q.reset(new QueryModule(s, g, device));
    HIPCHECK(hipSetDevice(device));
    return *q;
}

/* One launch of a guides-module kernel between two HIP events, waited for: the
 * kernel's device time goes to pt_call_profile's PT_PROF_KERNEL (microseconds) */
void guides_launch(hipFunction_t fn, long long n, void **args)
{
    Events ev;
    ev.create(2);
    ev.record(0, nullptr);
    HIPCHECK(hipModuleLaunchKernel(fn, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, nullptr, args, nullptr));
    ev.record(1, nullptr);
    HIPCHECK(hipDeviceSynchronize());
    g_prof[PT_PROF_KERNEL] = (double)ev.ms(0, 1) * 1e3;
}

struct PtGuideLaunchHost /* must match pt_guides.h PtGuideLaunch */
{
    uint64_t seed;
    int W, H;
    float sw, sh, dist;
    int gw, s0, spp;
    float *emission, *albedo, *normal, *t, *coverage;
    int *material;
};

} // namespace
} // namespace pt

using namespace pt;

extern "C" {

int pt_query_spans(pt_scene *s, pt_id obj, const float *rays, int64_t n, int max_spans, pt_span *out,
                   int32_t *counts, int device)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (obj < 0)
            obj = sc.root;
        check_obj(sc, obj);
        if (n < 0 || max_spans < 0 || (n > 0 && (!rays || !counts || (max_spans > 0 && !out))))
            throw Error(PT_ERR_ARG, "bad query arguments");
        if (n == 0)
            return PT_OK;
        static_assert(sizeof(pt_span) == 40, "pt_span is ten 4-byte words");
        Generated g = generate_query(sc, obj, -1);
        DeviceGuard dg;
        QueryModule &q = query_module(sc, g, device);
        Scratch sm;
        float *dr = (float *)sm.upload(rays, (size_t)n * 24);
        float *dout = (float *)sm.alloc((size_t)n * std::max(1, max_spans) * 40);
        int *dc = (int *)sm.alloc((size_t)n * 4);
        const float *Pp = q.up.P.p;
        const PtImageDev *ip = q.up.imgs.p;
        long long nn = n;
        int ms = max_spans;
        void *args[] = {&Pp, &ip, &dr, &nn, &ms, &dout, &dc};
        HIPCHECK(hipModuleLaunchKernel(q.mod.fn("pt_query_spans"), (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0,
                                       nullptr, args, nullptr));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(counts, dc, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (max_spans > 0) {
            HIPCHECK(hipMemcpy(out, dout, (size_t)n * max_spans * 40, hipMemcpyDeviceToHost));
            /* compact material indices -> the scene's material ids */
            for (int64_t i = 0; i < n; i++)
                for (int c = 0; c < std::min<int>(counts[i], max_spans); c++) {
                    pt_span &sp = out[i * max_spans + c];
                    sp.mat_start = g.mat_ids.at((size_t)sp.mat_start);
                    sp.mat_end = g.mat_ids.at((size_t)sp.mat_end);
                }
        }
        return PT_OK;
    });
}

int pt_tex_eval(pt_scene *s, pt_id tex, const float *points, int64_t n, float *rgb, float *value, int device)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        check_tex(sc, tex);
        if (n < 0 || (n > 0 && (!points || !rgb || !value)))
            throw Error(PT_ERR_ARG, "bad texture query arguments");
        if (n == 0)
            return PT_OK;
        Generated g = generate_query(sc, -1, tex);
        DeviceGuard dg;
        QueryModule &q = query_module(sc, g, device);
        Scratch sm;
        float *dp = (float *)sm.upload(points, (size_t)n * 12), *dc = (float *)sm.alloc((size_t)n * 12);
        float *dv = (float *)sm.alloc((size_t)n * 4);
        const float *Pp = q.up.P.p;
        const PtImageDev *ip = q.up.imgs.p;
        long long nn = n;
        void *args[] = {&Pp, &ip, &dp, &nn, &dc, &dv};
        HIPCHECK(hipModuleLaunchKernel(q.mod.fn("pt_tex_eval"), (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0,
                                       nullptr, args, nullptr));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(rgb, dc, (size_t)n * 12, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(value, dv, (size_t)n * 4, hipMemcpyDeviceToHost));
        return PT_OK;
    });
}

/* Compile (or fetch from the cache) the query module of pt_query_spans /
 * pt_tex_eval without a device. */
int pt_query_compile(pt_scene *s, pt_id obj, pt_id tex)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (obj >= 0)
            check_obj(sc, obj);
        if (tex >= 0)
            check_tex(sc, tex);
        /* obj -1: the root (unless only a texture is asked for); obj -2: no object */
        if (obj == -1 && tex < 0)
            obj = sc.root, check_obj(sc, obj);
        (void)code_object(generate_query(sc, obj < 0 ? -1 : obj, tex));
        return PT_OK;
    });
}

/* pt_query_hits: the guides module's pt_hits kernel (device/pt_guides.h), one
 * ray per lane into planar device arrays, assembled into pt_hit records here */
int pt_query_hits(pt_scene *s, const float *rays, int64_t n, int path, pt_hit *out, float *shade_out,
                  int32_t *decided, int device)
{
    const double t0 = now_us();
    for (double &v : g_prof) v = 0.0;
    return guard([&] {
        SceneImpl &sc = S(s);
        if (n < 0 || n >= (1ll << 31))
            throw Error(PT_ERR_ARG, "pt_query_hits: n must be in [0, 2^31)");
        if (path != PT_HIT_FAST && path != PT_HIT_MERGE)
            throw Error(PT_ERR_ARG, "pt_query_hits: path must be PT_HIT_FAST or PT_HIT_MERGE");
        if (device < 0)
            throw Error(PT_ERR_ARG, "pt_query_hits: device is negative");
        if (n > 0 && !rays)
            throw Error(PT_ERR_ARG, "pt_query_hits: rays is null");
        if (n > 0 && !out)
            throw Error(PT_ERR_ARG, "pt_query_hits: out is null");
        check_rays(rays, n, 6, "pt_query_hits: rays[");
        static_assert(sizeof(pt_hit) == 44, "pt_hit is eleven 4-byte words");
        std::shared_ptr<const Generated> gp = generated(sc, 0, false, false, true);
        const Generated &g = *gp;
        if (n == 0)
            return PT_OK;
        DeviceGuard dg;
        QueryModule &q = query_module(sc, g, device);
        Scratch sm;
        const size_t N = (size_t)n;
        float *dr = (float *)sm.upload(rays, N * 24);
        int *dhit = (int *)sm.alloc(N * 4), *dex = (int *)sm.alloc(N * 4), *ddec = (int *)sm.alloc(N * 4);
        int *dmat = (int *)sm.alloc(N * 4);
        float *dt = (float *)sm.alloc(N * 4), *dn = (float *)sm.alloc(N * 12), *dp = (float *)sm.alloc(N * 12);
        float *dior = (float *)sm.alloc(N * 4);
        float *dsh = shade_out ? (float *)sm.alloc(N * 44) : nullptr;
        const float *Pp = q.up.P.p;
        const PtImageDev *ip = q.up.imgs.p;
        long long nn = n;
        void *args[] = {&Pp, &ip, &dr, &nn, &path, &dhit, &dex, &ddec, &dmat, &dt, &dn, &dp, &dior, &dsh};
        guides_launch(q.mod.fn("pt_hits"), n, args);
        std::vector<int32_t> hhit(N), hex(N), hmat(N);
        std::vector<float> ht(N), hn(3 * N), hp(3 * N), hior(N);
        HIPCHECK(hipMemcpy(hhit.data(), dhit, N * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hex.data(), dex, N * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hmat.data(), dmat, N * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(ht.data(), dt, N * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hn.data(), dn, N * 12, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hp.data(), dp, N * 12, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hior.data(), dior, N * 4, hipMemcpyDeviceToHost));
        if (decided)
            HIPCHECK(hipMemcpy(decided, ddec, N * 4, hipMemcpyDeviceToHost));
        if (shade_out)
            HIPCHECK(hipMemcpy(shade_out, dsh, N * 44, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; i++) {
            pt_hit &h = out[i];
            h.hit = hhit[i], h.exit = hex[i];
            /* compact material index -> the scene's material id */
            h.material = hmat[i] < 0 ? -1 : g.mat_ids.at((size_t)hmat[i]);
            h.t = ht[i], h.ior = hior[i];
            for (int c = 0; c < 3; c++) h.normal[c] = hn[3 * i + c], h.pos[c] = hp[3 * i + c];
        }
        g_prof[PT_PROF_TOTAL] = now_us() - t0;
        return PT_OK;
    });
}

/* pt_render_guides: the guides module's pt_guides kernel, one pixel entry per
 * lane with its sample loop inside the lane */
int pt_render_guides(pt_scene *s, const pt_render_params *p, const pt_guide_buffers *out)
{
    const double t0 = now_us();
    for (double &v : g_prof) v = 0.0;
    return guard([&] {
        SceneImpl &sc = S(s);
        if (!p)
            throw Error(PT_ERR_ARG, "pt_render_guides: p is null");
        if (!out)
            throw Error(PT_ERR_ARG, "pt_render_guides: out is null");
        if (!out->emission && !out->albedo && !out->normal && !out->t && !out->coverage && !out->material)
            throw Error(PT_ERR_ARG, "pt_render_guides: out has every plane null");
        if (p->device < 0)
            throw Error(PT_ERR_ARG, "pt_render_guides: p->device is negative");
        if (p->pixels && p->npixels < 0)
            throw Error(PT_ERR_ARG, "pt_render_guides: p->npixels is negative");
        if (p->pixels && p->width > 0 && p->height > 0) {
            const int64_t limit = p->grid_width ? (int64_t)INT32_MAX : (int64_t)p->width * p->height;
            for (int64_t k = 0; k < p->npixels; k++)
                if (p->pixels[k] < 0 || p->pixels[k] >= limit)
                    throw Error(PT_ERR_ARG, "pt_render_guides: p->pixels[" + std::to_string(k) + "] is out of range");
        }
        pt_render_params v = *p; /* depth, order, sum_only and max_buffer_bytes are ignored */
        v.depth = 0, v.order = PT_ORDER_REFERENCE, v.sum_only = 0, v.max_buffer_bytes = 0;
        try {
            validate(&v);
        } catch (const Error &e) {
            throw Error(e.code, std::string("pt_render_guides: p: ") + e.what());
        }
        std::shared_ptr<const Generated> gp = generated(sc, 0, false, false, true);
        const Generated &g = *gp;
        const long long n = p->pixels ? (long long)p->npixels : (long long)p->width * p->height;
        if (n == 0)
            return PT_OK;
        DeviceGuard dg;
        QueryModule &q = query_module(sc, g, p->device);
        Scratch sm;
        const size_t N = (size_t)n;
        PtGuideLaunchHost gl;
        memset(&gl, 0, sizeof gl);
        gl.seed = p->seed;
        gl.W = p->width, gl.H = p->height;
        gl.sw = p->screen_w, gl.sh = p->screen_h, gl.dist = p->screen_dist;
        gl.gw = p->grid_width > 0 ? p->grid_width : p->width;
        gl.s0 = p->sample_begin, gl.spp = p->spp;
        gl.emission = out->emission ? (float *)sm.alloc(N * 12) : nullptr;
        gl.albedo = out->albedo ? (float *)sm.alloc(N * 12) : nullptr;
        gl.normal = out->normal ? (float *)sm.alloc(N * 12) : nullptr;
        gl.t = out->t ? (float *)sm.alloc(N * 4) : nullptr;
        gl.coverage = out->coverage ? (float *)sm.alloc(N * 4) : nullptr;
        gl.material = out->material ? (int *)sm.alloc(N * 4) : nullptr;
        int *dpix = p->pixels ? (int *)sm.upload(p->pixels, N * 4) : nullptr;
        const float *Pp = q.up.P.p;
        const PtImageDev *ip = q.up.imgs.p;
        long long nn = n;
        void *args[] = {&Pp, &ip, &dpix, &nn, &gl};
        guides_launch(q.mod.fn("pt_guides"), n, args);
        if (out->emission)
            HIPCHECK(hipMemcpy(out->emission, gl.emission, N * 12, hipMemcpyDeviceToHost));
        if (out->albedo)
            HIPCHECK(hipMemcpy(out->albedo, gl.albedo, N * 12, hipMemcpyDeviceToHost));
        if (out->normal)
            HIPCHECK(hipMemcpy(out->normal, gl.normal, N * 12, hipMemcpyDeviceToHost));
        if (out->t)
            HIPCHECK(hipMemcpy(out->t, gl.t, N * 4, hipMemcpyDeviceToHost));
        if (out->coverage)
            HIPCHECK(hipMemcpy(out->coverage, gl.coverage, N * 4, hipMemcpyDeviceToHost));
        if (out->material) {
            HIPCHECK(hipMemcpy(out->material, gl.material, N * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < N; k++)
                if (out->material[k] >= 0)
                    out->material[k] = g.mat_ids.at((size_t)out->material[k]);
        }
        g_prof[PT_PROF_TOTAL] = now_us() - t0;
        return PT_OK;
    });
}

int pt_guides_compile(pt_scene *s)
{
    return guard([&] {
        (void)code_object(generate_guides(S(s)));
        return PT_OK;
    });
}

const char *pt_scene_guides_key(pt_scene *s)
{
    thread_local std::string k;
    return key_text(k, [&] { return code_object_key(generate_guides(S(s))); });
}

} // extern "C"
