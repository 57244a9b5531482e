/* device_state.h -- what the entry-point families share of the render path
 * (runtime.cpp): a scene's state on one device, the upload of its parameters
 * and images, the launch record, and how a call is timed. */
#ifndef PT_DEVICE_STATE_H
#define PT_DEVICE_STATE_H

#include "hip_util.h"

namespace pt
{

struct PtImageDev
{
    const void *data;
    uint32_t w, h;
};

struct PtLaunchHost /* must match ptd::PtLaunch */
{
    uint64_t seed;
    long long n_items;
    long long chunk0;
    int W, H;
    float sw, sh, dist;
    int depth;
    int nsamp;
    int s0;
    int gw, chunk;
    int sample_major;
    int block_sums;
    long long perm;
    const float *rays;
    long long ray0;
    int grab;
    const unsigned *list;
    unsigned *bail;
    /* chained modules (PT_CHAIN) read on: other kernels take the fields above */
    uint64_t *states;
    const int *order;
    const long long *begin;
    int step, spp;
    float *acc;
    float *rgb;
    uint64_t *state_after;
    uint64_t *work;
};

/* The 64-bit words of a render module's counter block.  Must match
 * pt_device.h: render_chunk's flush (stats[0..7], stats[24], the wave clock
 * stats[26..29]) and the render kernels' work queues, `stats + (lp.list ? 36 :
 * 15)` and the bail list's length `stats[35]`. */
constexpr int kCounterWords = 40;
constexpr int kChunkCounter = 15; /* the persistent grid's chunk counter, zeroed before every launch */
constexpr int kBailWords = 35;    /* two words: the light kernel's list length, then that list's queue */
/* the counters both render and chained calls report */
void decode_counters(const uint64_t *c, pt_render_stats *st);

/* A module's copy of the scene parameter block and images on one device */
struct SceneUpload
{
    std::vector<float> params;
    std::vector<int> image_ids;
    DevBuf<float> P;
    DevBuf<PtImageDev> imgs; /* one entry per image slot and a spare one */
    std::vector<DevBuf<float>> img_data;
    /* uploads what differs from g: the block when the parameters do, every
     * image and the table when the image slots do (device current) */
    void sync(const SceneImpl &s, const Generated &g);
};

/* The HIP events and sample count of one render whose timings are not read yet */
struct PendingRender
{
    Events ev;
    std::vector<std::pair<int, int>> spans, rspans; /* (start, end) event of each render / reduce launch */
    uint64_t samples = 0;
    int n_spheres = 0, n_planes = 0;
};

/* pt_render_converge's module (pt_converge.h) and per-entry state on one device */
struct ConvergeDev
{
    Module mod;
    hipFunction_t reduce = nullptr, scan = nullptr, scatter = nullptr;
    DevBuf<float> acc, rgb, err;
    DevBuf<double> mom;
    DevBuf<int> blocks, spp, keep, list[4]; /* list: two (pixel, home) pairs, written in turn */
    DevBuf<unsigned> wg;                    /* per-workgroup keeps, capped counts and offsets */
    DevBuf<uint64_t> word;
};

/* A scene's state on one device; SceneImpl::devices destroys it on that device
 * (DeviceStateDelete), so every member here simply owns what it holds. */
struct DeviceState
{
    int device = 0;
    std::string key;
    Module mod;
    hipFunction_t fast = nullptr, strict = nullptr, reduce = nullptr;
    hipFunction_t light = nullptr; /* lane-walk modules: the split launch's light kernel */
    int wpw = 1; /* waves (chunks of 64 items) per workgroup, from the kernel's launch bounds */
    int resident_blocks = 0; /* persistent grid size: resident workgroups per CU x CUs */
    int light_blocks = 0;    /* the same for the light kernel */
    DevBuf<unsigned> bail;   /* the chunks the light kernel leaves to the full one */
    SceneUpload up;
    DevBuf<uint64_t> jump;
    DevBuf<float> stage, accum;
    DevBuf<float> out; /* pt_render's output (grow-only: no allocation per call) */
    PinBuf<int> hpix;  /* pt_render's pixel list and result, staged in pinned memory */
    PinBuf<float> hout;
    DevBuf<int> pixels;
    DevBuf<uint64_t> stats;
    DevBuf<uint64_t> chain;  /* pt_trace_chains' tables, sums, results and step counters (grow-only) */
    PinBuf<uint64_t> hchain; /* ... and their pinned staging */
    ConvergeDev conv;
    std::vector<PendingRender> pending; /* deferred timings (pt_render_device_timed) */
};

/* generate() (or, guides, generate_guides()) through the scene's cache */
std::shared_ptr<const Generated> generated(SceneImpl &s, int depth, bool rays, bool chain = false,
                                           bool guides = false);
/* A scene's state on one device: the render module, (rays) the ray-list
 * module of pt_trace_rays or (chain) a chained module of pt_trace_chains, each
 * with its own buffers so that alternating calls reload nothing.  Leaves
 * `device` current. */
DeviceState &device_state(SceneImpl &s, int device, const Generated &g, bool rays = false, bool chain = false);
/* Module, parameters and every device buffer a render with p needs. */
DeviceState &prepare(SceneImpl &s, const pt_render_params *p, std::shared_ptr<const Generated> &gp,
                     bool rays = false);
long long pass_samples(const pt_render_params *p, long long npix);

/* Items per dequeue and the persistent grid of one launch: the chunk size is
 * halved from `chunk` until every resident wave gets a few chunks */
struct Grid
{
    int chunk;
    long long chunks, blocks;
};
Grid chunk_grid(const DeviceState &ds, long long n_items, int chunk);

/* How a render reports its timings: not at all, synchronously (the call waits
 * for the kernels and fills pt_render_stats), or deferred (HIP events and the
 * device counters accumulate in the device state until pt_render_collect, so
 * the render stays asynchronous on the caller's stream: bench.py's reduce
 * follows it without a host round trip). */
enum class Timing
{
    None,
    Sync,
    Deferred
};
/* Before a call's first launch: returns how the call is timed after all (an
 * untimed call joins timed ones that wait for their collect), lets a
 * synchronous call report itself alone (st zeroed, pending forgotten) and,
 * when the call launches, restarts the counters with the first recorded
 * render.  After its last launch: keeps pr's events, and fills st for a
 * synchronous call. */
Timing begin_timing(DeviceState &ds, Timing tm, pt_render_stats *st, bool launches, hipStream_t stream);
void finish_timing(DeviceState &ds, Timing tm, PendingRender &pr, pt_render_stats *st);
/* Reads the recorded launches and the device counters of ds into st (after the
 * last recorded event completes) and forgets them. */
void collect_timings(DeviceState &ds, pt_render_stats *st);

/* What the passes of one call share (render_device, pt_render_converge) */
struct PassLaunch
{
    SceneImpl &s;
    DeviceState &ds;
    hipStream_t stream;
    bool timed;
    PendingRender &pr;
    const float *rays;
    int64_t ray0;
};
/* One render pass: samples p->sample_begin + s0 .. + nsamp - 1 of the npix
 * slots of the device-resident list dpix (null: slot = pixel) into ds.stage.
 * Returns pt_reduce's mode for the layout the launch staged. */
int launch_pass(const PassLaunch &L, const pt_render_params *p, const int *dpix, long long npix, int s0, int nsamp);
/* compact: with a pixel list, pixel k's result goes to fb[3k..3k+2] (else to
 * its frame position, fb[3 * pixels[k]]).  rays (device memory, 7 floats per
 * slot): the ray-list module of pt_trace_rays renders slot k = ray k instead
 * of a camera pixel */
void render_device(SceneImpl &s, const pt_render_params *p, float *fb, hipStream_t stream, pt_render_stats *st,
                   Timing tm, bool compact = false, const float *rays = nullptr, int64_t ray0 = 0);

} // namespace pt

#endif
