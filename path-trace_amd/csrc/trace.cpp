/* trace.cpp -- pt_trace_rays and pt_trace_chains (include/pt/pt.h): the render
 * module's kernels over caller rays and over chains of entries on a caller's
 * engine state, and the compiles of those module kinds. */
#include <algorithm>
#include <cstring>

#include "device_state.h"

using namespace pt;

/* traceRay<T>(ray, spanIterator, depth, engine, strength), include/path-trace.h:
 * 58-165, for n caller rays in one launch of the ray-list module: the render
 * kernel with slot k = ray k (origin, direction, strength) instead of a camera
 * ray, spp samples per ray keyed (seed, k, sample), summed in the call's order
 * and divided by spp -- tracePixel's float-coordinate overload (:172-185) when
 * every sample traces the same ray. */
static pt_render_params trace_params(const pt_trace_params *tp, int64_t n)
{
    if (!tp)
        throw Error(PT_ERR_ARG, "null params");
    if (n < 0 || n >= (1ll << 31))
        throw Error(PT_ERR_ARG, "ray count must be in [0, 2^31)");
    if (tp->ray_begin < 0 || tp->ray_begin + n > (1ll << 43))
        throw Error(PT_ERR_ARG, "ray keys must lie in [0, 2^43) (engine key layout)");
    pt_render_params p;
    memset(&p, 0, sizeof p);
    p.width = (int)std::max<int64_t>(1, n), p.height = 1;
    p.spp = tp->spp, p.depth = tp->depth;
    p.screen_w = p.screen_h = p.screen_dist = 1.0f; /* unused: no camera */
    p.seed = tp->seed, p.order = tp->order, p.device = tp->device;
    p.max_buffer_bytes = tp->max_buffer_bytes;
    p.sample_begin = tp->sample_begin;
    return p;
}

extern "C" {

int pt_trace_rays(pt_scene *s, const pt_trace_params *tp, const float *rays, int64_t n, float *rgb_out,
                  pt_render_stats *stats)
{
    return guard([&] {
        pt_render_params p = trace_params(tp, n);
        validate(&p);
        if (n == 0) {
            if (stats)
                memset(stats, 0, sizeof(*stats));
            return PT_OK;
        }
        if (!rays || !rgb_out)
            throw Error(PT_ERR_ARG, "null rays or output");
        check_rays(rays, n, 7, "ray ");
        SceneImpl &sc = S(s);
        HIPCHECK(hipSetDevice(p.device));
        DevBuf<float> fb, rb;
        fb.ensure((size_t)n * 3);
        rb.ensure((size_t)n * 7);
        HIPCHECK(hipMemcpy(rb.p, rays, (size_t)n * 7 * 4, hipMemcpyHostToDevice));
        pt_render_stats local;
        render_device(sc, &p, fb.p, nullptr, stats ? stats : &local, Timing::Sync, true, rb.p, tp->ray_begin);
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(rgb_out, fb.p, (size_t)n * 3 * 4, hipMemcpyDeviceToHost));
        return PT_OK;
    });
}

int pt_trace_compile(pt_scene *s, int depth)
{
    return guard([&] {
        Generated g = generate(S(s), depth, true);
        code_object(g);
        return PT_OK;
    });
}

int pt_chain_compile(pt_scene *s, int depth, int rays)
{
    return guard([&] {
        Generated g = generate(S(s), depth, rays != 0, true);
        code_object(g);
        return PT_OK;
    });
}

/* One launch of the chained module per step (chain.cpp chain_schedule), all on
 * the null stream, then one copy back and one synchronise.  The dependence of a
 * chain's sample on the one before is the stream's order: launch t reads the
 * engine states launch t - 1 wrote.  The device buffer, in 8-byte words:
 *   [states nc][state_after n][rgb 3n floats][begin nc + 1][order nc ints]
 *   [entries n ints | rays 7n floats][acc 3nc floats][work: one counter per step]
 * -- the first three come back in one copy, states and the tables go up in one. */
int pt_trace_chains(pt_scene *s, const pt_chain_params *p, const int32_t *pixels, const float *rays,
                    const int64_t *begin, int64_t nchains, uint64_t *states, float *rgb_out, uint64_t *state_after,
                    pt_render_stats *stats)
{
    return guard([&] {
        chain_validate(p, pixels, rays, begin, nchains, states, rgb_out);
        if (stats)
            memset(stats, 0, sizeof(*stats));
        std::vector<int32_t> order;
        std::vector<int64_t> items;
        chain_schedule(begin, nchains, p->spp, order, items);
        const size_t steps = items.size();
        if (steps == 0) /* every chain is empty: nothing runs, the states stay */
            return PT_OK;
        const size_t nc = (size_t)nchains, n = (size_t)begin[nchains];
        auto words = [](size_t bytes) { return (bytes + 7) / 8; };
        const size_t o_after = nc, o_rgb = o_after + n, o_begin = o_rgb + words(12 * n), o_order = o_begin + nc + 1,
                     o_entry = o_order + words(4 * nc), o_acc = o_entry + words(rays ? 28 * n : 4 * n),
                     o_work = o_acc + words(12 * nc), total = o_work + steps;
        SceneImpl &sc = S(s);
        HIPCHECK(hipSetDevice(p->device));
        std::shared_ptr<const Generated> gp = generated(sc, p->depth, rays != nullptr, true);
        DeviceState &ds = device_state(sc, p->device, *gp, rays != nullptr, true);
        ds.chain.ensure(total);
        ds.hchain.ensure(o_acc);
        uint64_t *const d = ds.chain.p, *const h = ds.hchain.p;
        memcpy(h, states, 8 * nc);
        memcpy(h + o_begin, begin, 8 * (nc + 1));
        memcpy(h + o_order, order.data(), 4 * nc);
        if (rays)
            memcpy(h + o_entry, rays, 28 * n);
        else
            memcpy(h + o_entry, pixels, 4 * n);
        hipStream_t stream = nullptr;
        HIPCHECK(hipMemcpyAsync(d, h, 8 * nc, hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(d + o_begin, h + o_begin, 8 * (o_acc - o_begin), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemsetAsync(d + o_work, 0, 8 * steps, stream));
        HIPCHECK(hipMemsetAsync(ds.stats.p, 0, kCounterWords * 8, stream));
        PtLaunchHost lp;
        memset(&lp, 0, sizeof lp);
        lp.W = rays ? 1 : p->width, lp.H = rays ? 1 : p->height;
        lp.sw = p->screen_w, lp.sh = p->screen_h, lp.dist = p->screen_dist;
        lp.depth = p->depth;
        lp.nsamp = 1; /* an item is one sample; its chain decides which (pt_device.h PT_CHAIN) */
        lp.gw = lp.W;
        lp.rays = rays ? (const float *)(d + o_entry) : nullptr;
        lp.grab = 1;
        lp.states = d, lp.state_after = d + o_after, lp.rgb = (float *)(d + o_rgb);
        lp.begin = (const long long *)(d + o_begin), lp.order = (const int *)(d + o_order);
        lp.acc = (float *)(d + o_acc);
        lp.spp = p->spp;
        const float *Pp = ds.up.P.p;
        const PtImageDev *ip = ds.up.imgs.p;
        const uint64_t *jp = ds.jump.p;
        float *op = lp.rgb; /* the stage of the other kinds: a chained kernel writes lp.rgb itself */
        const int *pp = rays ? nullptr : (const int *)(d + o_entry);
        uint64_t *sp = ds.stats.p;
        void *args[] = {&Pp, &ip, &jp, &op, &pp, &sp, &lp};
        Events ev;
        if (stats) {
            ev.create(2);
            ev.record(0, stream);
        }
        uint64_t samples = 0;
        for (size_t t = 0; t < steps; t++) {
            const Grid gr = chunk_grid(ds, items[t], 64);
            lp.n_items = items[t];
            lp.chunk = gr.chunk;
            lp.step = (int)t;
            lp.work = d + o_work + t;
            HIPCHECK(hipModuleLaunchKernel(ds.strict, (unsigned)gr.blocks, 1, 1, 64 * ds.wpw, 1, 1, 0, stream, args,
                                           nullptr));
            samples += (uint64_t)items[t];
        }
        if (stats)
            ev.record(1, stream);
        HIPCHECK(hipMemcpyAsync(h, d, 8 * o_begin, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        /* rgb of an entry is written with its last sample: every entry of every chain has one */
        memcpy(states, h, 8 * nc);
        if (state_after)
            memcpy(state_after, h + o_after, 8 * n);
        memcpy(rgb_out, h + o_rgb, 12 * n);
        if (stats) {
            uint64_t c[kCounterWords];
            HIPCHECK(hipMemcpy(c, ds.stats.p, sizeof c, hipMemcpyDeviceToHost));
            /* first launch's start to last launch's end, the gaps between them included */
            stats->kernel_ms = ev.ms(0, 1);
            stats->launches = steps;
            stats->samples = samples;
            decode_counters(c, stats);
        }
        return PT_OK;
    });
}

} // extern "C"
