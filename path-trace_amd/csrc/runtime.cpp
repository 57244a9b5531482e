/*
 * runtime.cpp -- libpt.so's render pipeline (include/pt/pt.h: pt_prepare,
 * pt_render*, pt_render_collect).
 *
 * Takes the host copy of the scene graph (scene.cpp), flattened into a device
 * module (codegen.cpp) and compiled to a gfx950 code object (jit.cpp), and
 * drives the megakernel:
 *
 *   items = (pixel slot, sample) pairs; a persistent grid of waves pulls
 *   chunks of up to 32 items from a counter (pt_render_fast / _strict),
 *   slot-major for large launches, sample-major for launches of <= 64 samples
 *   per slot.  Reference order stages each sample's radiance and pt_reduce
 *   sums a pixel's samples in sample order, exactly tracePixel's loop; the
 *   fast order stages one pairwise partial per 32-sample block (whole
 *   blocks per chunk) or per-sample values, and pt_reduce adds the blocks in
 *   order.  Large frames run in sample passes bounded by max_buffer_bytes,
 *   the running per-pixel sums carried between passes.
 *
 * This replaces RenderBlock::calcPixelColor's per-pixel tracePixel calls
 * (reference src/test.cpp:441-465); the block farm / thread pool around it
 * (src/test.cpp:147-518) becomes the hardware dispatcher plus, across GPUs,
 * one process per device (bench.py / pathtrace.dist).
 *
 * The other entry-point families build on what device_state.h declares of
 * this file: converge.cpp, trace.cpp, query.cpp, adaptive.cpp, selftest.cpp.
 */
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>

#include "../../include/pt/pt_engine.h"
#include "device_state.h"

namespace pt
{

/* Host-clock phases of this thread's last pt_render (pt_call_profile). */
thread_local double g_prof[PT_PROF_N];
double now_us()
{
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
               .count() /
           1e3;
}

void DeviceStateDelete::operator()(DeviceState *ds) const { OnDevice()(ds); }

void SceneUpload::sync(const SceneImpl &s, const Generated &g)
{
    if (params != g.params) {
        P.ensure(g.params.size());
        HIPCHECK(hipMemcpy(P.p, g.params.data(), g.params.size() * 4, hipMemcpyHostToDevice));
        params = g.params;
    }
    if (image_ids != g.image_ids) {
        img_data.clear();
        img_data.resize(g.image_ids.size());
        std::vector<PtImageDev> desc(g.image_ids.size() + 1);
        for (size_t k = 0; k < g.image_ids.size(); k++) {
            const ImageRec &im = s.images.at(g.image_ids[k]);
            img_data[k].ensure(im.rgba.size());
            HIPCHECK(hipMemcpy(img_data[k].p, im.rgba.data(), im.rgba.size() * 4, hipMemcpyHostToDevice));
            desc[k].data = img_data[k].p;
            desc[k].w = (uint32_t)im.w;
            desc[k].h = (uint32_t)im.h;
        }
        imgs.ensure(desc.size());
        HIPCHECK(hipMemcpy(imgs.p, desc.data(), desc.size() * sizeof(PtImageDev), hipMemcpyHostToDevice));
        image_ids = g.image_ids;
    }
}

void decode_counters(const uint64_t *c, pt_render_stats *st)
{
    st->queries = c[0] + c[1];
    st->leaf_queries = c[1];
    st->attempts = c[2];
    st->rounds = c[3];
    st->shaded = c[4];
    st->slow_queries = c[6];
    st->dark_queries = c[7];
    st->mid_queries = c[24];
}

Grid chunk_grid(const DeviceState &ds, long long n_items, int chunk)
{
    const long long waves = (long long)ds.resident_blocks * ds.wpw;
    while (chunk > 1 && n_items / chunk < 4 * waves) chunk /= 2;
    const long long chunks = (n_items + chunk - 1) / chunk;
    return {chunk, chunks, std::min<long long>(ds.resident_blocks, (chunks + ds.wpw - 1) / ds.wpw)};
}

namespace
{

/* jump table (A_{3m}, G_{3m}), m = 0..1024 (PT_KATT <= 16), of state_{n+3m} = A*state_n + G*inc
 * (PT_JUMP_ENTRIES of the device code: up to 16 x 64 attempts per round) */
std::vector<uint64_t> jump_table()
{
    constexpr uint32_t kEntries = 1025;
    std::vector<uint64_t> t(2 * kEntries);
    for (uint32_t m = 0; m < kEntries; m++) pt_lcg_jump_coeffs(3 * m, &t[2 * m], &t[2 * m + 1]);
    return t;
}

constexpr int kRaysState = 1 << 16, kChainState = 1 << 17;

} // namespace

DeviceState &device_state(SceneImpl &s, int device, const Generated &g, bool rays, bool chain)
{
    HIPCHECK(hipSetDevice(device));
    auto &ds = s.devices[device | (rays ? kRaysState : 0) | (chain ? kChainState : 0)];
    if (!ds) {
        ds.reset(new DeviceState);
        ds->device = device;
        std::vector<uint64_t> jt = jump_table();
        ds->jump.ensure(jt.size());
        HIPCHECK(hipMemcpy(ds->jump.p, jt.data(), jt.size() * 8, hipMemcpyHostToDevice));
        ds->stats.ensure(kCounterWords);
    }
    if (ds->key != g.key) {
        ds->mod.load(code_object(g));
        ds->strict = ds->mod.fn("pt_render_strict");
        ds->reduce = ds->mod.fn("pt_reduce");
        /* a chained module has the reference-order kernel alone (same launch bounds) */
        ds->fast = chain ? ds->strict : ds->mod.fn("pt_render_fast");
        int mt = 0;
        HIPCHECK(hipFuncGetAttribute(&mt, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, ds->fast));
        if (mt < 64 || mt % 64)
            throw Error(PT_ERR_DEVICE, "unexpected megakernel block size " + std::to_string(mt));
        ds->wpw = mt / 64;
        int per_cu = 0, cus = 0;
        HIPCHECK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ds->fast, mt, 0));
        HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        ds->resident_blocks = std::max(1, per_cu) * std::max(1, cus);
        /* lane-walk modules define pt_render_light (pt_device.h PT_DEFINE_LIGHT) */
        ds->light = nullptr;
        ds->light_blocks = 0;
        if (hipModuleGetFunction(&ds->light, ds->mod.m, "pt_render_light") != hipSuccess) {
            (void)hipGetLastError();
            ds->light = nullptr;
        } else {
            int lt = 0;
            HIPCHECK(hipFuncGetAttribute(&lt, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, ds->light));
            if (lt != mt)
                throw Error(PT_ERR_DEVICE, "light kernel block size differs from the megakernel's");
            HIPCHECK(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ds->light, mt, 0));
            ds->light_blocks = std::max(1, per_cu) * std::max(1, cus);
        }
        ds->key = g.key;
    }
    ds->up.sync(s, g);
    return *ds;
}

void validate(const pt_render_params *p)
{
    if (!p)
        throw Error(PT_ERR_ARG, "null params");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0)
        throw Error(PT_ERR_ARG, "width, height and spp must be positive");
    if ((int64_t)p->width * p->height >= (1ll << 31))
        throw Error(PT_ERR_ARG, "frame too large");
    if (p->spp >= (1 << 20))
        throw Error(PT_ERR_ARG, "spp must be < 2^20 (engine key layout)");
    if (p->sample_begin < 0 || (int64_t)p->sample_begin + p->spp > (1 << 20))
        throw Error(PT_ERR_ARG, "samples must lie in [0, 2^20) (engine key layout)");
    if (p->depth < 0 || p->depth > 64)
        throw Error(PT_ERR_ARG, "depth must be in [0, 64]");
    if (p->order != PT_ORDER_FAST && p->order != PT_ORDER_REFERENCE)
        throw Error(PT_ERR_ARG, "bad order");
    if (p->grid_width != 0 && p->grid_width < p->width)
        throw Error(PT_ERR_ARG, "grid_width must be 0 or >= width");
    if (p->pixels) {
        const int64_t limit = p->grid_width ? (int64_t)INT32_MAX : (int64_t)p->width * p->height;
        for (int64_t k = 0; k < p->npixels; k++)
            if (p->pixels[k] < 0 || p->pixels[k] >= limit)
                throw Error(PT_ERR_ARG, "pixel index out of range");
    }
}

namespace
{

/* frame-buffer floats a render with p addresses */
size_t frame_floats(const pt_render_params *p)
{
    size_t n = (size_t)p->width * p->height;
    if (p->pixels)
        for (int64_t k = 0; k < p->npixels; k++) n = std::max(n, (size_t)p->pixels[k] + 1);
    return 3 * n;
}

/* The fast order sums a pixel's samples in blocks of 32 (pt_device.h
 * pt_reduce); a slot-major launch of whole blocks stages one partial per
 * block instead of one value per sample (32x less: C4 3.2 GB, C5 25 GB in one
 * pass). */
bool block_staging(const pt_render_params *p)
{
    static const bool off = [] {
        const char *env = getenv("PT_BLOCK_SUMS"); /* experiment hook: 0 = per-sample staging only */
        if (!env || !*env)
            return false;
        fprintf(stderr, "pt: experiment hook PT_BLOCK_SUMS=%s active\n", env);
        return atoi(env) == 0;
    }();
    return !off && p->order == PT_ORDER_FAST && p->spp > 64 && p->spp % 32 == 0;
}

} // namespace

long long pass_samples(const pt_render_params *p, long long npix)
{
    int64_t budget = p->max_buffer_bytes > 0 ? p->max_buffer_bytes : (8ll << 30);
    long long per_pass = budget / (12ll * npix) * (block_staging(p) ? 32 : 1);
    per_pass = per_pass / 64 * 64;
    if (per_pass < 64)
        per_pass = 64;
    if (per_pass > p->spp)
        per_pass = p->spp;
    return per_pass;
}

namespace
{

/* Multiplier of the sample-major slot permutation (pt_device.h item_slot): a
 * prime near nslots / phi that does not divide nslots, so consecutive slots
 * of a chunk land ~0.38 of the list apart; 0 (identity) below 128 slots or
 * with PT_SAMPLE_PERM=0 (experiment hook). */
long long slot_permutation(long long nslots)
{
    static const bool on = [] {
        const char *env = getenv("PT_SAMPLE_PERM");
        if (env && *env == '0') {
            fprintf(stderr, "pt: experiment hook PT_SAMPLE_PERM=0 active\n");
            return false;
        }
        return true;
    }();
    if (!on || nslots < 128)
        return 0;
    auto prime = [](long long v) {
        if (v < 2)
            return false;
        for (long long d = 2; d * d <= v; d++)
            if (v % d == 0)
                return false;
        return true;
    };
    for (long long m = (long long)((double)nslots * 0.6180339887) | 1; m > 2; m -= 2)
        if (prime(m) && nslots % m != 0)
            return m;
    return 0;
}

/* split launches of lane-walk modules (pt_render_light + pt_render_fast);
 * PT_SPLIT=0 is an experiment hook: every chunk through the full kernel */
bool split_launches()
{
    static const bool on = [] {
        const char *env = getenv("PT_SPLIT");
        if (!env || !*env)
            return true;
        fprintf(stderr, "pt: experiment hook PT_SPLIT=%s active\n", env);
        return atoi(env) != 0;
    }();
    return on;
}

/* Chunks a wave takes per work-queue atomic while its chunks are cheap and
 * plenty are left (pt_device.h render_chunk): 8 in lane-walk scenes, whose
 * chunks are uniformly cheap and whose launches the single counter's atomic
 * rate bounds (C5 5 296 -> 8 112 Msamples/s), 1 elsewhere (C3: -0.45 % with
 * runs).  PT_GRAB=n is an experiment hook. */
int grab_chunks(const SceneImpl &s)
{
    static const int env_g = [] {
        const char *env = getenv("PT_GRAB");
        if (!env || !*env)
            return 0;
        fprintf(stderr, "pt: experiment hook PT_GRAB=%s active\n", env);
        return std::max(1, std::min(64, atoi(env)));
    }();
    if (env_g)
        return env_g;
    return (s.lane_walk > 0 || s.lane_scatter) ? 8 : 1;
}

/* Stage floats for the largest launch of a render: block partials for
 * slot-major whole-block launches, else one value per sample -- launches of
 * <= 64 samples per slot (sample-major) and small launches whose chunks fall
 * below 32 items (at most 4 * 32 items per resident wave). */
size_t stage_floats(const pt_render_params *p, long long npix, long long per_pass)
{
    if (!block_staging(p))
        return (size_t)(npix * per_pass * 3);
    size_t n = (size_t)(npix * (per_pass / 32) * 3);
    n = std::max(n, (size_t)(npix * std::min<long long>(64, p->spp) * 3));
    n = std::max(n, (size_t)(4ll * 64 * 16384 * 3)); /* a small launch: < 4 chunks of 64 per wave, <= 16384 waves */
    return std::min(n, (size_t)(npix * per_pass * 3));
}

/* generate() is a pure function of the scene records, the depth, the module
 * kind and the experiment hooks it reads; its text (the ~200 KB device library
 * plus the scene's types) and the FNV key over it cost about 0.1 ms, which a
 * caller tracing pixel by pixel (src/test.cpp:450) would pay per call.  A
 * scene keeps what it generated under a fingerprint of those inputs. */
struct Fnv
{
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n)
    {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t k = 0; k < n; k++) h = (h ^ b[k]) * 0x100000001b3ull;
    }
    template <class T>
    void add(const T &v)
    {
        bytes(&v, sizeof v);
    }
    void str(const char *v)
    {
        const size_t n = v ? strlen(v) : (size_t)-1;
        add(n);
        if (v)
            bytes(v, n);
    }
};

} // namespace

std::shared_ptr<const Generated> generated(SceneImpl &s, int depth, bool rays, bool chain, bool guides)
{
    auto make = [&] { return guides ? generate_guides(s) : generate(s, depth, rays, chain); };
    if (const char *hdr = getenv("PT_DEVICE_HEADER")) /* experiment hook: the file may change under us */
        if (*hdr)
            return std::make_shared<const Generated>(make());
    Fnv f;
    for (const ObjRec &o : s.objects) {
        f.add(o.kind), f.add(o.mat), f.add(o.a), f.add(o.b);
        f.bytes(o.f, sizeof o.f);
        f.str(o.span_body.c_str()), f.str(o.normal_body.c_str());
        f.add(o.max_spans);
        f.add(o.params.size());
        if (!o.params.empty())
            f.bytes(o.params.data(), o.params.size() * sizeof(float));
    }
    f.add(s.objects.size());
    for (const MatRec &m : s.materials) {
        f.add(m.reflect), f.add(m.scatter), f.add(m.emissive), f.add(m.transmit), f.add(m.trc), f.add(m.ior);
    }
    f.add(s.materials.size());
    for (const TexRec &t : s.textures) {
        f.add(t.kind), f.add(t.child);
        f.bytes(t.f, sizeof t.f), f.bytes(t.img, sizeof t.img);
        f.str(t.color_body.c_str()), f.str(t.value_body.c_str());
        f.add(t.params.size());
        if (!t.params.empty())
            f.bytes(t.params.data(), t.params.size() * sizeof(float));
    }
    f.add(s.textures.size());
    for (const ImageRec &im : s.images) /* images are immutable once created */
        f.add(im.w), f.add(im.h);
    f.add(s.images.size());
    f.add(s.root), f.add(s.default_tex[0]), f.add(s.default_tex[1]);
    f.add(s.wg_per_cu), f.add(s.fast_spine), f.add(s.lane_walk), f.add(s.lane_scatter);
    f.add(s.lane_resume);
    f.add(depth), f.add(rays), f.add(chain), f.add(guides);
    f.str(getenv("PT_DEVICE_DEFINES")), f.str(getenv("PT_JIT_OPTIONS"));
    auto it = s.gen_cache.find(f.h);
    if (it != s.gen_cache.end())
        return it->second;
    if (s.gen_cache.size() >= 16)
        s.gen_cache.clear();
    auto g = std::make_shared<const Generated>(make());
    s.gen_cache[f.h] = g;
    return g;
}

DeviceState &prepare(SceneImpl &s, const pt_render_params *p, std::shared_ptr<const Generated> &gp, bool rays)
{
    validate(p);
    gp = generated(s, p->depth, rays);
    const Generated &g = *gp;
    s.last_key = g.key;
    DeviceState &ds = device_state(s, p->device, g, rays);
    const long long npix = p->pixels ? (long long)p->npixels : (long long)p->width * p->height;
    if (npix > 0) {
        long long per_pass = pass_samples(p, npix);
        ds.stage.ensure(stage_floats(p, npix, per_pass));
        if (p->spp > per_pass)
            ds.accum.ensure((size_t)npix * 3);
        if (p->pixels)
            ds.pixels.ensure((size_t)npix);
    }
    return ds;
}

void collect_timings(DeviceState &ds, pt_render_stats *st)
{
    memset(st, 0, sizeof(*st));
    if (ds.pending.empty())
        return;
    /* renders may have been queued on different streams: wait for each one's
     * last event before reading any elapsed time */
    for (auto &pr : ds.pending)
        HIPCHECK(hipEventSynchronize(pr.ev.e.back()));
    for (auto &pr : ds.pending) {
        for (auto &sp : pr.spans) {
            st->kernel_ms += pr.ev.ms(sp.first, sp.second);
            st->launches++;
        }
        for (auto &sp : pr.rspans) st->reduce_ms += pr.ev.ms(sp.first, sp.second);
        st->samples += pr.samples;
    }
    uint64_t c[kCounterWords];
    HIPCHECK(hipMemcpy(c, ds.stats.p, sizeof c, hipMemcpyDeviceToHost));
    decode_counters(c, st);
    if (c[29])
        st->wave_ms = (double)c[28] * (double)st->launches / (double)c[29] / 1e5; /* 100 MHz clock */
    if (getenv("PT_PHASE_DUMP")) /* profiling builds (PT_PHASE_TIMING): per-phase wave cycles */
    {
        fprintf(stderr, "pt_phases");
        for (int k = 8; k < 15; k++)
            fprintf(stderr, " %llu", (unsigned long long)c[k]);
        for (int k = 16; k < 24; k++)
            fprintf(stderr, " %llu", (unsigned long long)c[k]);
        fprintf(stderr, " %llu", (unsigned long long)c[25]); /* whole chunk loop */
        fprintf(stderr, " %llu %llu", (unsigned long long)c[30], (unsigned long long)c[31]); /* spine queries */
        fprintf(stderr, " %llu %llu", (unsigned long long)c[32], (unsigned long long)c[33]); /* lane front end, writes */
        fprintf(stderr, " %llu", (unsigned long long)c[34]); /* spine queries that ran the lazy merge */
        fprintf(stderr, " %llu %llu", (unsigned long long)c[37], (unsigned long long)c[38]); /* lane-resume walk steps, service overhead */
        fprintf(stderr, "\n");
    }
    st->sphere_tests = st->queries * (uint64_t)ds.pending.back().n_spheres;
    st->plane_tests = st->queries * (uint64_t)ds.pending.back().n_planes;
    ds.pending.clear();
}

constexpr size_t kMaxPending = 1024; /* deferred renders a device keeps before a collect is required */

Timing begin_timing(DeviceState &ds, Timing tm, pt_render_stats *st, bool launches, hipStream_t stream)
{
    /* an untimed call queued while timed renders wait for their collect joins
     * them: its launches are timed too, so the counters the collect reads and
     * the kernel times it sums cover the same renders.  The pending cap binds
     * only renders the caller asked to time: a plain render never fails
     * because of another call's uncollected timings */
    const bool joined = tm == Timing::None && !ds.pending.empty();
    if (joined)
        tm = Timing::Deferred;
    if (tm == Timing::Deferred && !joined && ds.pending.size() >= kMaxPending)
        throw Error(PT_ERR_ARG, "too many timed renders pending: call pt_render_collect");
    if (tm == Timing::Sync) { /* a synchronous call reports itself alone */
        memset(st, 0, sizeof(*st));
        ds.pending.clear();
    }
    /* the counters restart with the first recorded render */
    if (launches && (tm == Timing::None || ds.pending.empty()))
        HIPCHECK(hipMemsetAsync(ds.stats.p, 0, kCounterWords * 8, stream));
    return tm;
}

void finish_timing(DeviceState &ds, Timing tm, PendingRender &pr, pt_render_stats *st)
{
    if (tm == Timing::None)
        return;
    ds.pending.push_back(std::move(pr));
    if (tm == Timing::Sync)
        collect_timings(ds, st);
}

int launch_pass(const PassLaunch &L, const pt_render_params *p, const int *dpix, long long npix, int s0, int nsamp)
{
    SceneImpl &s = L.s;
    DeviceState &ds = L.ds;
    hipStream_t stream = L.stream;
    PendingRender &pr = L.pr;
    hipFunction_t fn = p->order == PT_ORDER_REFERENCE ? ds.strict : ds.fast;
    long long n_items = npix * nsamp;
    /* 64 items per dequeue: every lane of the chunk's camera phase busy
     * (same-box A/B: C5 2430 -> 4490 Msamples/s, C3 +0.5 %; round 1: C3
     * 16 -> 32 +2.7 %); a launch too small to give every resident wave a
     * few chunks takes fewer (chunk_grid), so one wave does not trace many
     * samples of one expensive pixel while others idle */
    static const int chunk_max = [] {
        const char *env = getenv("PT_CHUNK_MAX"); /* experiment hook (1..64) */
        if (!env || !*env)
            return 64;
        fprintf(stderr, "pt: experiment hook PT_CHUNK_MAX=%s active\n", env);
        return std::max(1, std::min(64, atoi(env)));
    }();
    /* slot-major launches of few samples per pixel (a multi-GPU rank's
     * share: C3 at 8 ranks = 128 per pixel) take 32-sample chunks: a
     * chunk is then half as many samples of one expensive pixel, which
     * shortens the launch's tail (same-box A/B at 128 spp: 147.2 -> 153.3
     * Msamples/s; at 256 spp 64 stays ahead, 156.0 vs 153.2) */
    const Grid gr = chunk_grid(ds, n_items, nsamp > 64 && nsamp <= 128 ? std::min(chunk_max, 32) : chunk_max);
    const int chunk = gr.chunk, wpw = ds.wpw;
    const long long chunks = gr.chunks;
    PtLaunchHost lp;
    memset(&lp, 0, sizeof lp);
    lp.seed = p->seed;
    lp.n_items = n_items;
    lp.W = p->width, lp.H = p->height;
    lp.sw = p->screen_w, lp.sh = p->screen_h, lp.dist = p->screen_dist;
    lp.depth = p->depth;
    lp.nsamp = nsamp;
    lp.s0 = p->sample_begin + s0;
    lp.gw = p->grid_width > 0 ? p->grid_width : p->width;
    lp.chunk = chunk;
    /* sample-major item order for launches of up to 64 samples per slot
     * (pt_device.h item_slot) */
    lp.sample_major = nsamp <= 64 ? 1 : 0;
    if (lp.sample_major)
        lp.perm = slot_permutation(npix);
    /* one staged partial per 32-sample block when a chunk is a block */
    lp.block_sums =
        (block_staging(p) && !lp.sample_major && (chunk == 32 || chunk == 64) && nsamp % chunk == 0) ? 1 : 0;
    lp.rays = L.rays;
    lp.ray0 = L.ray0;
    lp.grab = grab_chunks(s);
    /* split launch (lane-walk modules, fast order): the light kernel
     * over every chunk, then the full kernel over the ones it left */
    const bool split = ds.light && fn == ds.fast && s.split && split_launches() && chunks < (1ll << 32);
    const int reduce_mode = p->order == PT_ORDER_REFERENCE ? 0 : lp.block_sums ? 2 : 1;
    ds.stage.ensure((size_t)(lp.block_sums ? npix * (nsamp / 32) * 3 : npix * nsamp * 3));
    const float *Pp = ds.up.P.p;
    const PtImageDev *ip = ds.up.imgs.p;
    const uint64_t *jp = ds.jump.p;
    float *op = ds.stage.p;
    const int *pp = dpix;
    uint64_t *sp = ds.stats.p; /* counters + the persistent chunk counter */
    HIPCHECK(hipMemsetAsync(ds.stats.p + kChunkCounter, 0, 8, stream));
    void *args[] = {&Pp, &ip, &jp, &op, &pp, &sp, &lp};
    int e0 = 0;
    if (L.timed)
        e0 = pr.ev.add(stream);
    if (split) {
        ds.bail.ensure((size_t)chunks);
        HIPCHECK(hipMemsetAsync(ds.stats.p + kBailWords, 0, 16, stream));
        lp.bail = ds.bail.p;
        const long long lblocks = std::min<long long>(ds.light_blocks, (chunks + wpw - 1) / wpw);
        HIPCHECK(hipModuleLaunchKernel(ds.light, (unsigned)lblocks, 1, 1, 64 * wpw, 1, 1, 0, stream, args, nullptr));
        lp.bail = nullptr;
        lp.list = ds.bail.p;
    }
    HIPCHECK(hipModuleLaunchKernel(fn, (unsigned)gr.blocks, 1, 1, 64 * wpw, 1, 1, 0, stream, args, nullptr));
    if (L.timed)
        pr.spans.push_back({e0, pr.ev.add(stream)});
    return reduce_mode;
}

void render_device(SceneImpl &s, const pt_render_params *p, float *fb, hipStream_t stream, pt_render_stats *st,
                   Timing tm, bool compact, const float *rays, int64_t ray0)
{
    std::shared_ptr<const Generated> gp;
    DeviceState &ds = prepare(s, p, gp, rays != nullptr);
    const Generated &g = *gp;
    const long long npix = p->pixels ? (long long)p->npixels : (long long)p->width * p->height;
    tm = begin_timing(ds, tm, st, npix != 0, stream);
    if (npix == 0)
        return;
    const int *dpix = nullptr;
    if (p->pixels) {
        HIPCHECK(hipMemcpyAsync(ds.pixels.p, p->pixels, (size_t)npix * 4, hipMemcpyHostToDevice, stream));
        dpix = ds.pixels.p;
    }
    const long long per_pass = pass_samples(p, npix);
    const bool timed = tm != Timing::None;
    PendingRender pr;
    pr.n_spheres = g.n_spheres, pr.n_planes = g.n_planes;
    const PassLaunch L{s, ds, stream, timed, pr, rays, ray0};
    for (int s0 = 0; s0 < p->spp; s0 += (int)per_pass) {
        int nsamp = (int)std::min<long long>(per_pass, p->spp - s0);
        long long n_items = npix * nsamp;
        int reduce_mode = launch_pass(L, p, dpix, npix, s0, nsamp);
        {
            const float *in = ds.stage.p;
            float *acc = ds.accum.p;
            const int *pp = compact ? nullptr : dpix; /* output index: slot (compact) or pixel */
            long long ns = npix;
            int first = s0 == 0, last = s0 + nsamp == p->spp;
            float spp = p->sum_only ? 1.0f : (float)p->spp; /* x / 1 == x: the raw sum */
            void *args[] = {&in, &acc, &fb, &pp, &ns, &nsamp, &first, &last, &spp, &reduce_mode};
            unsigned blocks = (unsigned)((npix + 255) / 256);
            int e0 = 0;
            if (timed)
                e0 = pr.ev.add(stream);
            HIPCHECK(hipModuleLaunchKernel(ds.reduce, blocks, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
            if (timed)
                pr.rspans.push_back({e0, pr.ev.add(stream)});
        }
        pr.samples += (uint64_t)n_items;
    }
    finish_timing(ds, tm, pr, st);
}

} // namespace pt

using namespace pt;

extern "C" {

int pt_prepare(pt_scene *s, const pt_render_params *p)
{
    return guard([&] {
        std::shared_ptr<const Generated> g;
        prepare(S(s), p, g);
        return PT_OK;
    });
}

int pt_render_device(pt_scene *s, const pt_render_params *p, float *fb, void *stream, pt_render_stats *stats)
{
    return guard([&] {
        if (!fb)
            throw Error(PT_ERR_ARG, "null frame buffer");
        render_device(S(s), p, fb, (hipStream_t)stream, stats, stats ? Timing::Sync : Timing::None);
        return PT_OK;
    });
}

int pt_render_device_timed(pt_scene *s, const pt_render_params *p, float *fb, void *stream)
{
    return guard([&] {
        if (!fb)
            throw Error(PT_ERR_ARG, "null frame buffer");
        render_device(S(s), p, fb, (hipStream_t)stream, nullptr, Timing::Deferred);
        return PT_OK;
    });
}

int pt_render_collect(pt_scene *s, int device, pt_render_stats *stats)
{
    return guard([&] {
        if (!stats)
            throw Error(PT_ERR_ARG, "null stats");
        SceneImpl &sc = S(s);
        auto it = sc.devices.find(device);
        if (it == sc.devices.end() || !it->second) {
            memset(stats, 0, sizeof(*stats));
            return PT_OK;
        }
        HIPCHECK(hipSetDevice(device));
        collect_timings(*it->second, stats);
        return PT_OK;
    });
}

constexpr size_t kPinFloats = (size_t)1 << 20; /* results up to 4 MB go through pinned staging */

int pt_render(pt_scene *s, const pt_render_params *p, float *rgb_out, pt_render_stats *stats)
{
    const double t0 = now_us();
    for (double &v : g_prof) v = 0.0;
    return guard([&] {
        if (!rgb_out)
            throw Error(PT_ERR_ARG, "null output");
        validate(p);
        SceneImpl &sc = S(s);
        HIPCHECK(hipSetDevice(p->device));
        /* a pixel list renders into a compact buffer, pixel k at 3k; pt_reduce
         * writes every slot of it, so the buffer needs no clearing */
        const size_t n = p->pixels ? (size_t)std::max<int64_t>(1, p->npixels) * 3 : frame_floats(p);
        std::shared_ptr<const Generated> gp;
        DeviceState &ds = prepare(sc, p, gp, false);
        ds.out.ensure(n);
        const size_t nout = p->pixels ? (size_t)p->npixels * 3 : n;
        /* small calls (a pixel, a block) stage the pixel list and the result in
         * pinned memory: asynchronous DMA both ways and one synchronisation */
        const bool pin = nout <= kPinFloats;
        pt_render_params q = *p;
        if (pin && p->pixels && p->npixels > 0) {
            ds.hpix.ensure((size_t)p->npixels);
            memcpy(ds.hpix.p, p->pixels, (size_t)p->npixels * 4);
            q.pixels = ds.hpix.p;
        }
        if (pin)
            ds.hout.ensure(std::max<size_t>(nout, 1));
        const double t1 = now_us();
        /* without stats the launches carry no events and no counter read-back */
        pt_render_stats local;
        const bool want = stats != nullptr || getenv("PT_CALL_KERNEL_TIME");
        render_device(sc, &q, ds.out.p, nullptr, stats ? stats : &local, want ? Timing::Sync : Timing::None, true);
        if (pin && nout)
            HIPCHECK(hipMemcpyAsync(ds.hout.p, ds.out.p, nout * 4, hipMemcpyDeviceToHost, nullptr));
        const double t2 = now_us();
        HIPCHECK(hipStreamSynchronize(nullptr));
        const double t3 = now_us();
        if (nout) {
            if (pin)
                memcpy(rgb_out, ds.hout.p, nout * 4);
            else
                HIPCHECK(hipMemcpy(rgb_out, ds.out.p, nout * 4, hipMemcpyDeviceToHost));
        }
        const double t4 = now_us();
        g_prof[PT_PROF_SETUP] = t1 - t0;
        g_prof[PT_PROF_ENQUEUE] = t2 - t1;
        g_prof[PT_PROF_WAIT] = t3 - t2;
        g_prof[PT_PROF_D2H] = t4 - t3;
        g_prof[PT_PROF_TOTAL] = t4 - t0;
        if (want) {
            const pt_render_stats &st = stats ? *stats : local;
            g_prof[PT_PROF_KERNEL] = st.kernel_ms * 1e3;
            g_prof[PT_PROF_REDUCE] = st.reduce_ms * 1e3;
        }
        return PT_OK;
    });
}

int pt_rank_pixels(int width, int height, int rank, int world, int tile, int32_t *pixels, int64_t capacity,
                   int64_t *count)
{
    return guard([&] {
        if (width <= 0 || height <= 0 || (int64_t)width * height >= (1ll << 31))
            throw Error(PT_ERR_ARG, "bad frame size");
        if (world < 1 || rank < 0 || rank >= world || tile < 1)
            throw Error(PT_ERR_ARG, "need 0 <= rank < world and tile >= 1");
        if (!count || (pixels && capacity < 0))
            throw Error(PT_ERR_ARG, "null count or negative capacity");
        int64_t n = 0;
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const int64_t owner = world == 1 ? 0 : ((int64_t)(x / tile) + 3ll * (y / tile)) % world;
                if (owner != rank)
                    continue;
                if (pixels && n < capacity)
                    pixels[n] = y * width + x;
                n++;
            }
        *count = n;
        if (pixels && n > capacity)
            throw Error(PT_ERR_ARG, "capacity below the rank's pixel count");
        return PT_OK;
    });
}

int pt_call_profile(double *out, int n)
{
    if (!out || n < 0)
        return PT_ERR_ARG;
    for (int k = 0; k < n && k < PT_PROF_N; k++) out[k] = g_prof[k];
    return PT_OK;
}

} // extern "C"
