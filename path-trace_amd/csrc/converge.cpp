/* converge.cpp -- pt_render_converge (include/pt/pt.h): rounds of the render
 * module's passes (runtime.cpp launch_pass) over the entries still active,
 * each followed by the scene-independent module of device/pt_converge.h, which
 * folds the staged samples into per-entry moments, decides who is done and
 * compacts the survivors into the next round's list. */
#include <algorithm>
#include <cstring>

#include "device_state.h"

namespace pt
{
namespace
{

struct PtConvergeHost /* must match pt_converge.h PtConverge */
{
    const float *stage;
    const int *pix;
    const int *home;
    long long n;
    int nsamp, mode, first, last, cap;
    float rel_tol, abs_tol;
    float *acc;
    double *mom;
    int *blocks;
    float *rgb;
    int *spp;
    float *err;
    int *keep;
    unsigned *wg_keep, *wg_capped, *wg_off;
    uint64_t *word;
    int nwg;
    int *pix_next, *home_next;
};

/* pt_render_converge's scene-independent module (device/pt_converge.h), with
 * the scene modules' compiler options */
Generated converge_generated()
{
    Generated g;
    g.source = device_converge_source();
    g.key = "converge";
    return g;
}

/* pt_render_converge's argument check, before any device is touched */
void converge_validate(const pt_render_params *p, const pt_converge_params *cp, const float *rgb_out)
{
    if (!p)
        throw Error(PT_ERR_ARG, "pt_render_converge: p is null");
    if (!cp)
        throw Error(PT_ERR_ARG, "pt_render_converge: cp is null");
    if (!rgb_out)
        throw Error(PT_ERR_ARG, "pt_render_converge: rgb_out is null");
    validate(p);
    if (p->pixels && p->npixels < 0)
        throw Error(PT_ERR_ARG, "pt_render_converge: p->npixels is negative");
    if (p->order != PT_ORDER_FAST)
        throw Error(PT_ERR_ARG, "pt_render_converge: p->order must be PT_ORDER_FAST");
    if (p->sample_begin != 0)
        throw Error(PT_ERR_ARG, "pt_render_converge: p->sample_begin must be 0");
    if (p->sum_only != 0)
        throw Error(PT_ERR_ARG, "pt_render_converge: p->sum_only must be 0");
    if (p->spp % 32 != 0)
        throw Error(PT_ERR_ARG, "pt_render_converge: p->spp (the cap) must be a multiple of 32");
    if (cp->min_spp < 64 || cp->min_spp % 32 != 0 || cp->min_spp > p->spp)
        throw Error(PT_ERR_ARG, "pt_render_converge: cp->min_spp must be a multiple of 32, >= 64 and <= p->spp");
    if (!(cp->rel_tol >= 0.0f))
        throw Error(PT_ERR_ARG, "pt_render_converge: cp->rel_tol must be >= 0 and not NaN");
    if (!(cp->abs_tol >= 0.0f))
        throw Error(PT_ERR_ARG, "pt_render_converge: cp->abs_tol must be >= 0 and not NaN");
}

void render_converge(SceneImpl &s, const pt_render_params *p, pt_converge_params *cp, float *rgb_out,
                     int32_t *spp_out, float *err_out, pt_render_stats *st)
{
    converge_validate(p, cp, rgb_out);
    cp->rounds = 0, cp->samples = 0, cp->capped = 0;
    if (st)
        memset(st, 0, sizeof(*st));
    const long long n0 = p->pixels ? (long long)p->npixels : (long long)p->width * p->height;
    if (n0 == 0)
        return;
    const std::vector<char> &code = code_object(converge_generated());
    /* the first round sizes the render module's buffers */
    pt_render_params q = *p;
    q.spp = cp->min_spp;
    std::shared_ptr<const Generated> gp;
    DeviceState &ds = prepare(s, &q, gp);
    const Generated &g = *gp;
    ConvergeDev &cv = ds.conv;
    if (!cv.mod) {
        cv.mod.load(code);
        cv.reduce = cv.mod.fn("pt_converge_reduce");
        cv.scan = cv.mod.fn("pt_converge_scan");
        cv.scatter = cv.mod.fn("pt_converge_scatter");
    }
    constexpr int kBlock = 256; /* pt_converge.h PTC_BLOCK */
    const size_t n = (size_t)n0, nwg0 = (n + kBlock - 1) / kBlock;
    cv.acc.ensure(3 * n), cv.rgb.ensure(3 * n), cv.err.ensure(n), cv.mom.ensure(2 * n);
    cv.blocks.ensure(n), cv.spp.ensure(n), cv.keep.ensure(n);
    for (auto &l : cv.list) l.ensure(n);
    cv.wg.ensure(3 * nwg0), cv.word.ensure(2);

    hipStream_t stream = nullptr;
    /* a call with stats reports itself alone; one without joins timed renders
     * that wait for their collect */
    const Timing tm = begin_timing(ds, st ? Timing::Sync : Timing::None, st, true, stream);
    const bool timed = tm != Timing::None;
    const int *pix = nullptr, *home = nullptr;
    if (p->pixels) {
        HIPCHECK(hipMemcpyAsync(ds.pixels.p, p->pixels, n * 4, hipMemcpyHostToDevice, stream));
        pix = ds.pixels.p;
    }
    PendingRender pr;
    pr.n_spheres = g.n_spheres, pr.n_planes = g.n_planes;
    const PassLaunch L{s, ds, stream, timed, pr, nullptr, 0};
    auto launch = [&](hipFunction_t fn, unsigned blocks, PtConvergeHost &a) {
        void *args[] = {&a};
        int e0 = 0;
        if (timed)
            e0 = pr.ev.add(stream);
        HIPCHECK(hipModuleLaunchKernel(fn, blocks, 1, 1, kBlock, 1, 1, 0, stream, args, nullptr));
        if (timed)
            pr.rspans.push_back({e0, pr.ev.add(stream)});
    };
    PtConvergeHost a;
    memset(&a, 0, sizeof a);
    a.cap = p->spp;
    a.rel_tol = cp->rel_tol, a.abs_tol = cp->abs_tol;
    a.acc = cv.acc.p, a.mom = cv.mom.p, a.blocks = cv.blocks.p;
    a.rgb = cv.rgb.p, a.spp = cv.spp.p, a.err = cv.err.p;
    a.keep = cv.keep.p;
    a.wg_keep = cv.wg.p, a.wg_capped = cv.wg.p + nwg0, a.wg_off = cv.wg.p + 2 * nwg0;
    a.word = cv.word.p;

    long long active = n0;
    int flip = 0;
    for (int done = 0, next = cp->min_spp; active > 0; done = next, next = (int)std::min<long long>(2ll * done, p->spp)) {
        /* round: samples [done, next) of the active entries */
        q.spp = next - done;
        q.sample_begin = done;
        const unsigned nwg = (unsigned)((active + kBlock - 1) / kBlock);
        const long long per_pass = pass_samples(&q, active);
        a.pix = pix, a.home = home, a.n = active, a.nwg = (int)nwg;
        for (int s0 = 0; s0 < q.spp; s0 += (int)per_pass) {
            const int nsamp = (int)std::min<long long>(per_pass, q.spp - s0);
            a.mode = launch_pass(L, &q, pix, active, s0, nsamp);
            a.stage = ds.stage.p;
            a.nsamp = nsamp;
            a.first = done == 0 && s0 == 0;
            a.last = s0 + nsamp == q.spp;
            launch(cv.reduce, nwg, a);
            pr.samples += (uint64_t)(active * nsamp);
        }
        launch(cv.scan, 1, a);
        uint64_t word[2];
        HIPCHECK(hipMemcpyAsync(word, cv.word.p, sizeof word, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        cp->rounds++;
        cp->capped += (int64_t)word[1];
        const long long left = (long long)word[0];
        if (left < 0 || left > active)
            throw Error(PT_ERR_DEVICE, "pt_render_converge: survivor count out of range");
        if (left > 0) {
            a.pix_next = cv.list[2 * flip].p, a.home_next = cv.list[2 * flip + 1].p;
            launch(cv.scatter, nwg, a);
            pix = a.pix_next, home = a.home_next;
            flip ^= 1;
        }
        active = left;
    }
    cp->samples = (int64_t)pr.samples;
    HIPCHECK(hipMemcpy(rgb_out, cv.rgb.p, 3 * n * 4, hipMemcpyDeviceToHost));
    if (spp_out)
        HIPCHECK(hipMemcpy(spp_out, cv.spp.p, n * 4, hipMemcpyDeviceToHost));
    if (err_out)
        HIPCHECK(hipMemcpy(err_out, cv.err.p, n * 4, hipMemcpyDeviceToHost));
    finish_timing(ds, tm, pr, st);
}

} // namespace
} // namespace pt

using namespace pt;

extern "C" {

int pt_render_converge(pt_scene *s, const pt_render_params *p, pt_converge_params *cp, float *rgb_out,
                       int32_t *spp_out, float *err_out, pt_render_stats *stats)
{
    return guard([&] {
        render_converge(S(s), p, cp, rgb_out, spp_out, err_out, stats);
        return PT_OK;
    });
}

int pt_converge_compile(void)
{
    return guard([&] {
        (void)code_object(converge_generated());
        return PT_OK;
    });
}

} // extern "C"
