/* denoise.cpp -- the host side of pt_denoise (include/pt/pt.h): the argument
 * check, the scene-independent module of device/pt_denoise.h, its records on
 * each device, and the launches: ptd_prepare, one ptd_atrous per iteration
 * between two (signal, variance) buffers, ptd_finalise. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "hip_util.h"

namespace pt
{

namespace
{

struct PtDenoiseHost /* must match pt_denoise.h PtDenoise */
{
    int W, H, step, demod, npow, pad_;
    float sigma_l, sigma_z;
    const float *rgb, *err, *normal, *t, *albedo, *emission;
    const int *material;
    const void *sv_in;
    void *sv_out, *geo;
    float *out, *var_out;
};

/* the module and the grow-only records of one device: two (signal, variance)
 * buffers written in turn and the (normal, depth) buffer, 16 bytes a pixel each */
struct DenoiseDev
{
    int arm = 0; /* the probe arm the module was built for */
    Module mod;
    hipFunction_t prepare = nullptr, atrous = nullptr, finalise = nullptr;
    DevBuf<char> rec;
    size_t pixels = 0;
};
std::mutex g_mu;
/* lives as long as the library: a process's devices are few.  Never destroyed,
 * so nothing is freed while the process exits; enqueue() replaces a device's
 * module and records with that device current */
std::map<int, DenoiseDev> &g_dev = *new std::map<int, DenoiseDev>;

/* probe hook: PT_DENOISE_LDS_TILE=1 builds pt_denoise.h's measured alternative,
 * an LDS tile for the step 1 and 2 passes (tools/denoise_probe.py); it computes
 * the same bits */
int probe_arm()
{
    const char *e = getenv("PT_DENOISE_LDS_TILE");
    return e && e[0] == '1' && !e[1] ? 1 : 0;
}

Generated denoise_generated()
{
    Generated g;
    const int arm = probe_arm();
    if (arm) {
        static const bool announce = (fprintf(stderr, "pt: experiment hook PT_DENOISE_LDS_TILE active\n"), true);
        (void)announce;
        g.source = "#define PTD_LDS_TILE 1\n";
    }
    g.source += device_denoise_source();
    g.key = arm ? "denoise-lds-tile" : "denoise";
    return g;
}

void validate(const pt_denoise_params *p, const pt_denoise_buffers *b)
{
    const std::string f = "pt_denoise: ";
    if (!p)
        throw Error(PT_ERR_ARG, f + "p is null");
    if (!b)
        throw Error(PT_ERR_ARG, f + "b is null");
    if (p->width < 1)
        throw Error(PT_ERR_ARG, f + "p->width must be >= 1");
    if (p->height < 1)
        throw Error(PT_ERR_ARG, f + "p->height must be >= 1");
    if ((int64_t)p->width * p->height >= (1ll << 31))
        throw Error(PT_ERR_ARG, f + "p->width * p->height must be below 2^31");
    if (p->iterations < 0 || p->iterations > 8)
        throw Error(PT_ERR_ARG, f + "p->iterations must be in 0..8");
    if (!(p->sigma_l > 0.0f))
        throw Error(PT_ERR_ARG, f + "p->sigma_l must be > 0 and not NaN");
    if (!(p->sigma_z > 0.0f))
        throw Error(PT_ERR_ARG, f + "p->sigma_z must be > 0 and not NaN");
    if (p->normal_power_log2 < 0 || p->normal_power_log2 > 8)
        throw Error(PT_ERR_ARG, f + "p->normal_power_log2 must be in 0..8");
    if (p->demodulate != 0 && p->demodulate != 1)
        throw Error(PT_ERR_ARG, f + "p->demodulate must be 0 or 1");
    if (p->device < 0)
        throw Error(PT_ERR_ARG, f + "p->device is negative");
    if (!b->rgb)
        throw Error(PT_ERR_ARG, f + "b->rgb is null");
    if (!b->normal)
        throw Error(PT_ERR_ARG, f + "b->normal is null");
    if (!b->t)
        throw Error(PT_ERR_ARG, f + "b->t is null");
    if (!b->material)
        throw Error(PT_ERR_ARG, f + "b->material is null");
    if (p->demodulate && !b->albedo)
        throw Error(PT_ERR_ARG, f + "b->albedo is null with p->demodulate set");
    if (p->demodulate && !b->emission)
        throw Error(PT_ERR_ARG, f + "b->emission is null with p->demodulate set");
    if (!b->out)
        throw Error(PT_ERR_ARG, f + "b->out is null");
}

/* The launches of one call, on `stream`; the planes of b are device memory.
 * Allocates only when the frame is larger than any this device has seen.
 * ev (null, or iterations + 3 events) is recorded before each launch and after
 * the last. */
void enqueue(const pt_denoise_params *p, const pt_denoise_buffers *b, hipStream_t stream, hipEvent_t *ev)
{
    const std::vector<char> &code = code_object(denoise_generated());
    HIPCHECK(hipSetDevice(p->device));
    std::lock_guard<std::mutex> lk(g_mu);
    DenoiseDev &d = g_dev[p->device];
    if (d.mod && d.arm != probe_arm()) {
        HIPCHECK(hipDeviceSynchronize());
        d.mod.unload();
    }
    if (!d.mod) {
        d.arm = probe_arm();
        d.mod.load(code);
        d.prepare = d.mod.fn("ptd_prepare");
        d.atrous = d.mod.fn("ptd_atrous");
        d.finalise = d.mod.fn("ptd_finalise");
    }
    const size_t n = (size_t)p->width * (size_t)p->height;
    if (n > d.pixels) {
        if (d.rec.p) /* a call still queued may be reading the old records */
            HIPCHECK(hipDeviceSynchronize());
        d.pixels = 0;
        d.rec.release();
        d.rec.ensure(3 * n * 16);
        d.pixels = n;
    }
    char *buf[2] = {d.rec.p, d.rec.p + 16 * d.pixels};
    PtDenoiseHost a;
    memset(&a, 0, sizeof a);
    a.W = p->width, a.H = p->height;
    a.demod = p->demodulate, a.npow = p->normal_power_log2;
    a.sigma_l = p->sigma_l, a.sigma_z = p->sigma_z;
    a.rgb = b->rgb, a.err = b->err, a.normal = b->normal, a.t = b->t;
    a.albedo = p->demodulate ? b->albedo : nullptr, a.emission = p->demodulate ? b->emission : nullptr;
    a.material = b->material;
    a.geo = d.rec.p + 32 * d.pixels;
    a.out = b->out, a.var_out = b->var_out;
    /* one workgroup per tile of 64 x 4 pixels, a wave per row of it */
    const unsigned segs = ((unsigned)p->width + 63u) / 64u;
    const unsigned blocks = segs * (((unsigned)p->height + 3u) / 4u);
    void *args[] = {&a};
    int launches = 0;
    auto launch = [&](hipFunction_t fn) {
        if (ev)
            HIPCHECK(hipEventRecord(ev[launches], stream));
        launches++;
        HIPCHECK(hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, stream, args, nullptr));
    };
    int cur = 0;
    a.sv_out = buf[cur];
    launch(d.prepare);
    for (int i = 0; i < p->iterations; i++) {
        a.step = 1 << i;
        a.sv_in = buf[cur], a.sv_out = buf[cur ^ 1];
        launch(d.atrous);
        cur ^= 1;
    }
    a.sv_in = buf[cur], a.sv_out = nullptr;
    launch(d.finalise);
    if (ev)
        HIPCHECK(hipEventRecord(ev[launches], stream));
}

} // namespace
} // namespace pt

using namespace pt;

extern "C" {

int pt_denoise(const pt_denoise_params *p, const pt_denoise_buffers *b)
{
    const double t0 = now_us();
    for (double &v : g_prof) v = 0.0;
    return guard([&] {
        validate(p, b);
        DeviceGuard dg;
        HIPCHECK(hipSetDevice(p->device));
        const size_t n = (size_t)p->width * (size_t)p->height;
        Scratch sm;
        pt_denoise_buffers d;
        memset(&d, 0, sizeof d);
        d.rgb = (const float *)sm.upload(b->rgb, n * 12);
        d.err = b->err ? (const float *)sm.upload(b->err, n * 4) : nullptr;
        d.normal = (const float *)sm.upload(b->normal, n * 12);
        d.t = (const float *)sm.upload(b->t, n * 4);
        d.material = (const int32_t *)sm.upload(b->material, n * 4);
        if (p->demodulate) {
            d.albedo = (const float *)sm.upload(b->albedo, n * 12);
            d.emission = (const float *)sm.upload(b->emission, n * 12);
        }
        d.out = (float *)sm.upload(nullptr, n * 12);
        d.var_out = b->var_out ? (float *)sm.upload(nullptr, n * 4) : nullptr;
        Events ev;
        ev.create(p->iterations + 3);
        enqueue(p, &d, nullptr, ev.e.data());
        HIPCHECK(hipDeviceSynchronize());
        const float ms = ev.ms(0, p->iterations + 2);
        HIPCHECK(hipMemcpy(b->out, d.out, n * 12, hipMemcpyDeviceToHost));
        if (b->var_out)
            HIPCHECK(hipMemcpy(b->var_out, d.var_out, n * 4, hipMemcpyDeviceToHost));
        g_prof[PT_PROF_KERNEL] = (double)ms * 1e3;
        g_prof[PT_PROF_TOTAL] = now_us() - t0;
        return PT_OK;
    });
}

int pt_denoise_device(const pt_denoise_params *p, const pt_denoise_buffers *b, void *stream)
{
    return guard([&] {
        validate(p, b);
        DeviceGuard dg;
        enqueue(p, b, (hipStream_t)stream, nullptr);
        return PT_OK;
    });
}

int pt_denoise_device_timed(const pt_denoise_params *p, const pt_denoise_buffers *b, void *stream, float *ms)
{
    return guard([&] {
        validate(p, b);
        if (!ms)
            throw Error(PT_ERR_ARG, "pt_denoise: ms is null");
        DeviceGuard dg;
        HIPCHECK(hipSetDevice(p->device));
        Events ev;
        ev.create(p->iterations + 3);
        enqueue(p, b, (hipStream_t)stream, ev.e.data());
        HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
        for (int k = 0; k < p->iterations + 2; k++) ms[k] = ev.ms(k, k + 1);
        return PT_OK;
    });
}

int pt_denoise_compile(void)
{
    return guard([&] {
        (void)code_object(denoise_generated());
        return PT_OK;
    });
}

const char *pt_denoise_key(void)
{
    thread_local std::string k;
    return key_text(k, [&] { return code_object_key(denoise_generated()); });
}

} // extern "C"
