/*
 * pt.h -- C-ABI drop-in boundary of the MI355X path tracer (libpt.so).
 *
 * The reference has no C ABI: its boundary is the C++ scene API of namespace
 * PathTrace plus the templates tracePixel<T>/traceRay<T>.
 * Every entry point below replaces one reference interface, cited per line.
 * Plain pointers and sizes only; no exceptions cross the ABI: functions return
 * a status (PT_OK = 0, negative on error) or an id (>= 0, negative on error),
 * and pt_last_error() describes the last failure on the calling thread.
 *
 * Ownership mirrors the reference: a scene owns every texture, material,
 * object and image created in it; ids stay valid until pt_scene_destroy.
 * Objects may be referenced by several parents (the reference would
 * duplicate() them), materials are shared by reference as in the reference
 * (`const Material *`, include/sphere.h:12).
 *
 * Threading: a pt_scene may be rendered from one thread at a time; distinct
 * scenes are independent.  Rendering is synchronous unless pt_render_device
 * is given a stream.
 */
#ifndef PT_PT_H
#define PT_PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_ERR_ARG (-1)      /* bad id / argument (reference: assert or UB)          */
#define PT_ERR_MATH (-2)     /* singular matrix: std::domain_error, transform.h:353   */
#define PT_ERR_IO (-3)       /* ImageLoadError / ImageStoreError, image.h:30-46       */
#define PT_ERR_DEVICE (-4)   /* HIP runtime failure or no device                      */
#define PT_ERR_COMPILE (-5)  /* device code generation / hiprtc failure               */

typedef struct pt_scene pt_scene;
typedef int32_t pt_id;

/* ------------------------------------------------------------ lifetime -- */
pt_scene *pt_scene_create(void);
void pt_scene_destroy(pt_scene *s);
const char *pt_last_error(void);
const char *pt_version(void);

/* ------------------------------------------------------------- images --- */
/* Image(string fileName) for ".hdr"/".pic" (reference src/image.cpp:83-324). */
pt_id pt_image_load_hdr(pt_scene *s, const char *path);
/* Image(string fileName) for ".png": PngDecoder (reference src/png_decoder.cpp:
 * 40-128) + byte / 255.0f (src/image.cpp:60-79); RGB gets alpha 0 (the
 * png_set_filler(0) of :94-97), palette tRNS becomes alpha.  Grayscale PNGs
 * are PT_ERR_IO (the reference's decoder leaves their rows half written). */
pt_id pt_image_load_png(pt_scene *s, const char *path);
/* Image(string fileName) with the format taken from the extension
 * (src/image.cpp:49-59): "png", "hdr", "pic" (case-insensitive). */
pt_id pt_image_load(pt_scene *s, const char *path);
/* MutableImage -> Image (include/image.h:110-211): rgba is h rows of w RGBA
 * floats, row 0 = top; copied. */
pt_id pt_image_from_rgba32f(pt_scene *s, const float *rgba, int w, int h);
/* Decode a Radiance HDR file into caller memory (w*h*4 floats); pass
 * rgba=NULL to query the size. */
int pt_hdr_read(const char *path, float *rgba, int *w, int *h);
/* The same for a PNG file (pt_image_load_png's decoding). */
int pt_png_read(const char *path, float *rgba, int *w, int *h);

/* ----------------------------------------------------------- textures --- */
pt_id pt_tex_color(pt_scene *s, float r, float g, float b);              /* ColorTexture       texture.h:29-58  */
pt_id pt_tex_image(pt_scene *s, pt_id image);                            /* ImageTexture       image_texture.h:9-33 */
pt_id pt_tex_image_alpha(pt_scene *s, pt_id image);                      /* ImageAlphaTexture  image_texture.h:35-70 */
pt_id pt_tex_skybox(pt_scene *s, pt_id top, pt_id bottom, pt_id left,    /* ImageSkyboxTexture image_texture.h:72-115 */
                    pt_id right, pt_id front, pt_id back);
pt_id pt_tex_skybox_alpha(pt_scene *s, pt_id top, pt_id bottom, pt_id left, /* ImageSkyboxAlphaTexture :117-181 */
                          pt_id right, pt_id front, pt_id back);
pt_id pt_tex_multiply(pt_scene *s, float r, float g, float b, pt_id t);  /* MultiplyTexture    filter_texture.h:36-56 */
pt_id pt_tex_log(pt_scene *s, pt_id t);                                  /* LogTexture         filter_texture.h:58-82 */
pt_id pt_tex_mirrorball(pt_scene *s, pt_id t);                           /* MirrorBallSkymapTexture transform_texture.h:33-59 */
pt_id pt_tex_spherical(pt_scene *s, pt_id t);                            /* SphericalCoordinatesSkymapTexture :61-85 */
pt_id pt_tex_transformed(pt_scene *s, const float m[12], pt_id t);      /* TransformedTexture texture.h:60-90 */
pt_id pt_tex_coord(pt_scene *s);                                         /* test instrument: colour = coordinate */
/* A user-defined Texture subclass (include/texture.h:10-27: the virtual
 * getColor, and getFloat unless it keeps the default mean of getColor) as
 * device source.  color_body is the body of
 *     V3 getColor(V3 p)           -- p.x, p.y, p.z: the lookup point
 * and value_body (NULL = the reference's default) the body of
 *     float getFloat(V3 p)
 * in the device library's vocabulary (V3, mk(x, y, z), the f32 math builtins
 * floorf, fabsf, sqrtf, fminf, ...); both read their nparams parameters as
 * `const float *prm`.  The bodies are compiled into every module of the scene
 * that reaches the texture, with the scene's options: no FMA contraction and
 * correctly rounded '/' and sqrt, so a body computes what the same text
 * compiled on the host with -ffp-contract=off computes.  A body that does not
 * compile makes the render fail with PT_ERR_COMPILE and the compiler's log in
 * pt_last_error(). */
pt_id pt_tex_device(pt_scene *s, const char *color_body, const char *value_body, const float *params, int nparams);

/* ---------------------------------------------------------- materials --- */
/* Material(reflect, scatter_coefficient, emissive, transmit, ior,
 * transmit_reflect_coefficient), include/material.h:18.  Pass -1 for a
 * texture to get the reference default (1, 1, 0, 0, -, 0). */
pt_id pt_material(pt_scene *s, pt_id reflect, pt_id scatter, pt_id emissive, pt_id transmit, float ior,
                  pt_id transmit_reflect);

/* ------------------------------------------------------------ objects --- */
pt_id pt_sphere(pt_scene *s, float cx, float cy, float cz, float r, pt_id mat);   /* Sphere  sphere.h:12 */
pt_id pt_plane(pt_scene *s, float nx, float ny, float nz, float d, pt_id mat);    /* Plane(n, d)   plane.h:12 */
pt_id pt_plane_through(pt_scene *s, float nx, float ny, float nz,                 /* Plane(n, pos) plane.h:13 */
                       float px, float py, float pz, pt_id mat);
#define PT_CSG_UNION 0        /* Union        union.h:12        */
#define PT_CSG_INTERSECTION 1 /* Intersection intersection.h:12 */
#define PT_CSG_DIFFERENCE 2   /* Difference   difference.h:12   */
pt_id pt_csg(pt_scene *s, int op, pt_id a, pt_id b);
pt_id pt_transformed(pt_scene *s, const float m[12], pt_id child);             /* TransformedObject object.h:78 */
/* A user-defined Object subclass (include/object.h:10-24: the virtual
 * makeSpanIterator) whose iterator yields at most one span per ray -- a convex
 * shape -- as device source, compiled into the scene's modules
 * (path-trace_amd/csrc/device/pt_user_object.h).  span_body is the body of
 *     bool span(V3 o, V3 d, float &t0, float &t1)
 * returning whether the ray o + t d (d not normalised) meets the object, and
 * then its entry and exit parameters t0 <= t1 (the Span's start and end,
 * include/span.h); normal_body is the body of
 *     V3 normal(V3 p)
 * returning the outward surface normal at p, which is the span's start normal
 * at the entry point and its end normal at the exit.  Both read the nparams
 * parameters as `const float *prm` and use the device library's vocabulary
 * (V3, mk, dot, normalize, the f32 math builtins), compiled without FMA
 * contraction and with correctly rounded '/' and sqrt, so they compute what
 * the same text compiled on the host with -ffp-contract=off computes.  The
 * object takes part in every CSG node and transform like a built-in
 * primitive; the kernel's fast paths treat it conservatively (never dark). */
pt_id pt_object_device(pt_scene *s, const char *span_body, const char *normal_body, const float *params,
                       int nparams, pt_id mat);
/* The same for a subclass whose iterator yields several spans per ray
 * (include/object.h:14-20: makeSpanIterator returns any SpanIterator;
 * include/span.h:129-171: init(ray), then next() until isAtEnd()) -- a hollow
 * shell, a torus, a dumbbell, user-side CSG -- as a bounded span list
 * (path-trace_amd/csrc/device/pt_user_object_n.h).  spans_body is the body of
 *     int spans(V3 o, V3 d, float *t0, float *t1)
 * returning the number n of spans, 0 <= n <= max_spans, the ray o + t d (d not
 * normalised) has with the object, and filling t0[k] <= t1[k] for k < n in ray
 * order and strictly separated: t1[k] < t0[k + 1]; normal_body is the body of
 *     V3 normal(V3 p, int k)
 * returning the outward surface normal at the boundary point p of span k (its
 * start normal at the entry point, its end normal at the exit; traceRay flips
 * the end normal itself).  Parameters (`const float *prm`), vocabulary and
 * arithmetic are pt_object_device's: no FMA contraction, correctly rounded '/'
 * and sqrt.  max_spans is 1..PT_OBJECT_MAX_SPANS (1 is legal: one span, with
 * these signatures); each span takes one primitive slot of the tree, i.e.
 * three words of registers per lane in the kernel's fast checks, so declare
 * what the shape needs (a shell 2, a torus 4) -- 8 is a design bound, not a
 * measured one.  A body that breaks its contract (a count above max_spans,
 * unordered or touching spans) gives wrong pixels, never an access out of
 * range.  All spans carry the one material.  PT_ERR_ARG, with the entry
 * point's name in pt_last_error(): an empty body, a bad parameter block,
 * max_spans out of range, a bad material. */
#define PT_OBJECT_MAX_SPANS 8
pt_id pt_object_device_spans(pt_scene *s, const char *spans_body, const char *normal_body, const float *params,
                             int nparams, int max_spans, pt_id mat);
int pt_set_root(pt_scene *s, pt_id obj);
/* Load a whole scene from the plain-text scene format (oracle/scene_text.h
 * documents it; pathtrace.scene.to_text writes it).  Replaces the current
 * contents of s. */
int pt_scene_from_text(pt_scene *s, const char *text);

/* ---------------------------------------------------- matrix helpers --- */
/* Float arithmetic of include/transform.h:207-421, m in constructor order
 * x00 x10 x20 x30 x01 x11 x21 x31 x02 x12 x22 x32. */
void pt_matrix_rotate(const float axis[3], double angle, float out[12]);
int pt_matrix_inverse(const float m[12], float out[12]);                /* PT_ERR_MATH if singular */
void pt_matrix_concat(const float a[12], const float b[12], float out[12]);

/* ------------------------------------------------------------- render --- */
#define PT_ORDER_FAST 0      /* fast path: a burst's non-zero leaf-child terms dealt round-robin to 64
                                lane sums, added as their pairwise tree; samples in
                                32-sample pairwise blocks (oracle.cpp ORDER_FAST)     */
#define PT_ORDER_REFERENCE 1 /* bit-for-bit the reference's sequential child order          */
#define PT_ORDER_GROUP64 PT_ORDER_FAST /* deprecated name of PT_ORDER_FAST (rounds 1-2)      */

typedef struct pt_render_params {
    int width, height;             /* screenXResolution, screenYResolution                      */
    int spp;                       /* sampleCount                                               */
    int depth;                     /* rayDepth                                                  */
    float screen_w, screen_h;      /* screenWidth, screenHeight                                 */
    float screen_dist;             /* screenDistance                                            */
    uint64_t seed;                 /* run seed of the per-(pixel, sample) engine (pt_engine.h)  */
    int order;                     /* PT_ORDER_*                                                */
    int device;                    /* HIP device ordinal                                        */
    const int32_t *pixels;         /* optional host list of pixel indices (y*width+x) to render;
                                      NULL = all pixels                                         */
    int64_t npixels;               /* length of pixels                                          */
    int64_t max_buffer_bytes;      /* per-sample staging budget (0 = 8 GiB)                     */
    int grid_width;                /* pixel index = y * grid_width + x (0 = width); > width
                                      addresses pixels past the right / bottom edge, as the
                                      adaptive caller's block edges do                          */
    int sample_begin;              /* engine sample index of this call's first sample: the call
                                      renders samples sample_begin .. sample_begin + spp - 1 of
                                      each pixel (a rank's share when samples are split)        */
    int sum_only;                  /* nonzero: write each pixel's sum of those samples, in
                                      sample order, without the division by spp               */
} pt_render_params;

typedef struct pt_render_stats {
    double kernel_ms;              /* summed render-kernel time (HIP events)                    */
    double reduce_ms;              /* summed reduce-kernel time                                 */
    uint64_t launches;             /* render-kernel launches                                    */
    uint64_t samples;              /* traceRay calls from tracePixel                            */
    uint64_t queries;              /* root span queries (spine + leaf children)                 */
    uint64_t leaf_queries;         /* of which wave-cooperative leaf children                   */
    uint64_t attempts;             /* rejection attempts consumed (a round evaluates 512)       */
    uint64_t rounds;               /* attempt rounds                                            */
    uint64_t sphere_tests, sphere_hits, plane_tests;
    uint64_t slow_queries;         /* leaf children that needed the full CSG merge (slow pass)  */
    uint64_t dark_queries;         /* leaf children no emissive primitive can light: weight * 0 */
    uint64_t mid_queries;          /* leaf children the clear pass could not finish (fast check) */
    double wave_ms;                /* mean render-wave lifetime (device clock); kernel_ms minus
                                      this is the launch's tail, where waves have run out of work */
    uint64_t shaded;               /* traceRay activations that shade their hit (depth and strength left) */
} pt_render_stats;

/* Synchronous: renders the frame into rgb_out (host memory), which receives,
 * for each pixel of params->pixels (or of the whole frame, row-major), the
 * mean radiance (r, g, b) exactly as tracePixel returns it (path-trace.h:187-201).
 * Replaces the per-pixel tracePixel calls of RenderBlock::calcPixelColor
 * (reference src/test.cpp:441-465).  stats = NULL skips the launches' timing
 * events and the counter read-back (the per-pixel caller's fast path). */
int pt_render(pt_scene *s, const pt_render_params *p, float *rgb_out, pt_render_stats *stats);

/* The multi-GPU partition (replaces the reference's TCP block farm,
 * src/test.cpp:520-778): the pixel indices (y * width + x, raster order) rank
 * `rank` of `world` renders in the lattice deal of tile x tile tiles -- tile
 * (tx, ty) belongs to rank (tx + 3 ty) mod world -- the default of bench.py
 * and pathtrace.dist.rank_pixels.  Every pixel has exactly one owner, so the
 * ranks' frames (pt_render_device with the list into a zeroed full frame)
 * sum to the one-GPU frame bit for bit.  pixels = NULL: *count receives the
 * number only; else at most capacity indices are written. */
int pt_rank_pixels(int width, int height, int rank, int world, int tile, int32_t *pixels, int64_t capacity,
                   int64_t *count);

/* Host-clock phases (microseconds) of the calling thread's last pt_render --
 * the breakdown of a per-pixel tracePixel call.  out[k]
 * for k < n: */
#define PT_PROF_TOTAL 0   /* the whole call                                                   */
#define PT_PROF_SETUP 1   /* validation, the scene's generated module (cached), device buffers */
#define PT_PROF_ENQUEUE 2 /* pixel upload, counter reset, render + reduce launches, the
                             result's copy-back (with stats: also the wait for the
                             launches' timing events)                                       */
#define PT_PROF_WAIT 3    /* stream synchronise: the kernels' remaining run time and the
                             copy-back (results up to 4 MB: a DMA into pinned staging)       */
#define PT_PROF_D2H 4     /* the result into the caller's memory (pinned staging: a memcpy;
                             larger results: a synchronous device-to-host copy)              */
#define PT_PROF_KERNEL 5  /* render launch(es) by HIP events (0 unless stats were asked for,
                             or PT_CALL_KERNEL_TIME is set)                                   */
#define PT_PROF_REDUCE 6  /* pt_reduce by HIP events (the same condition)                     */
#define PT_PROF_N 7
/* pt_query_hits and pt_render_guides record PT_PROF_TOTAL and PT_PROF_KERNEL
 * (their one launch, by HIP events) the same way, and so does pt_denoise (its
 * launches, prepare to finalise); the other phases read 0. */
int pt_call_profile(double *out, int n);

/* Device variant: writes W*H*3 floats into device memory fb (full frame,
 * row-major; with params->pixels, 3 floats at 3*index for every listed index,
 * so fb must cover the largest one; other pixels are left untouched) on the
 * given hipStream_t (NULL = default stream) and returns once the work is
 * enqueued... or completed when stats != NULL (stats need the timings). */
int pt_render_device(pt_scene *s, const pt_render_params *p, float *fb, void *stream, pt_render_stats *stats);

/* pt_render_device that stays asynchronous and still keeps its timings: HIP
 * events around each launch and the device counters accumulate on the scene's
 * device until pt_render_collect, so a caller can queue the render, a
 * collective on the same stream and more renders without a host round trip
 * (bench.py's multi-GPU step: render, then the RCCL reduce of the frame).
 * At most 1024 timed renders may wait for a collect (PT_ERR_ARG after that).
 * An untimed pt_render_device queued while timed renders wait joins them: its
 * launches are timed and its counters go into the next collect's totals, and
 * it never counts against the cap. */
int pt_render_device_timed(pt_scene *s, const pt_render_params *p, float *fb, void *stream);

/* Waits for the timed renders queued on `device` since the last collect and
 * returns their summed statistics (kernel_ms, launches, samples, counters);
 * all zero when none are pending. */
int pt_render_collect(pt_scene *s, int device, pt_render_stats *stats);

/* The reference demo's image-formation policy, RenderBlock::renderSquare
 * (src/test.cpp:423-507): per block of block_size x block_size pixels, trace
 * the corners, then recursively either interpolate a square (size <=
 * max_interp and all six corner pairs within min_delta: colorCloseEnough,
 * :437-440, interpolateSquare :423-436) or trace its five subdivision points
 * and recurse into the quadrants.  Pixels are traced with p->spp samples each,
 * one GPU batch per subdivision level over all blocks; engine keys use the
 * grid y * gw + x with gw = ceil(width / block) * block + 1 (block corners
 * reach past the right edge).  rgb_out receives
 * the W*H*3 image.  block_size / max_interp <= 0 select the demo's values
 * (getBlockSize(width / 8), height / 120, :40-50); min_delta <= 0 selects 0.003. */
typedef struct pt_adaptive_params {
    int block_size;
    int max_interp;
    float min_delta;
    int64_t traced_pixels;         /* out: pixels traced whose colour the image used            */
    int levels;                    /* out: GPU batches                                          */
    int exact_batches;             /* in: nonzero = one batch per level, only needed points     */
    int64_t lookahead_pixels;      /* out: traced one level ahead and never used                */
} pt_adaptive_params;
int pt_render_adaptive(pt_scene *s, const pt_render_params *p, pt_adaptive_params *ap, float *rgb_out,
                       pt_render_stats *stats);

/* Converged rendering, no reference counterpart: every entry (a pixel of
 * p->pixels, or of the whole frame) is sampled until the standard error of its
 * mean is within a tolerance, instead of p->spp times.  Rounds: round 0 traces
 * samples [0, min_spp) of every entry, round r + 1 samples [n_r, min(2 n_r,
 * p->spp)) of the entries that have not stopped; the call ends when none is
 * left.  At the end of a round an entry with n = 32 m samples has m block sums
 * B_j (the fast order's 32-sample blocks); with y_j = (B_j.r + B_j.g) + B_j.b
 * in f32 and s1 = sum y_j, s2 = sum y_j^2 in f64 (block order),
 *     e2 = max(s2 - s1 s1 / m, 0) / (m (m - 1)),
 *     t  = max(32 abs_tol, rel_tol |s1 / m|),
 * it stops iff e2 <= t t or n == p->spp; an entry whose s1 or s2 is not finite
 * stops at once with err = NaN.  A stopped entry holds rgb = its sums / n --
 * bit for bit what pt_render gives that pixel with spp = n --, spp = n and
 * err = sqrt(e2) / 32: the standard error of the mean per-sample r + g + b,
 * estimated from the spread of the block means (batch means).
 * p->spp is the cap (a multiple of 32), p->order PT_ORDER_FAST, p->sample_begin
 * and p->sum_only 0; pixels and grid_width as in pt_render.  Outputs are per
 * entry, compact (3 floats, 1 int, 1 float at entry k); spp_out and err_out
 * may be NULL.  stats sum over the rounds (reduce_ms: the moments, decision
 * and compaction kernels).  Every argument is checked before a device is
 * touched: PT_ERR_ARG names the argument in pt_last_error(). */
typedef struct pt_converge_params {
    int min_spp;                   /* first round; a multiple of 32, >= 64, <= p->spp           */
    float rel_tol, abs_tol;        /* >= 0, not NaN                                             */
    int rounds;                    /* out                                                       */
    int64_t samples;               /* out: samples traced                                       */
    int64_t capped;                /* out: entries that stopped only because n reached p->spp   */
} pt_converge_params;
int pt_render_converge(pt_scene *s, const pt_render_params *p, pt_converge_params *cp, float *rgb_out,
                       int32_t *spp_out, float *err_out, pt_render_stats *stats);
/* JIT-compile (or fetch from the code-object cache) pt_render_converge's
 * scene-independent module without touching a GPU. */
int pt_converge_compile(void);

/* traceRay<T>(const Ray &ray, SpanIterator &, int depth, T &engine, float
 * strength) of include/path-trace.h:58-165 for a batch of caller rays, in one
 * device launch.  rays = n records of 7 floats: origin xyz, direction xyz
 * (non-zero: Ray's assert, include/ray.h:17; not normalised), strength.
 * Origin and direction components must be finite (PT_ERR_ARG otherwise): the
 * kernel's axis-aligned plane forms keep only the product that is non-zero for
 * finite operands, where the reference's full dot product of an infinite
 * component would be NaN.
 * rgb_out receives, per ray, the mean of spp traceRay samples -- sample s of ray
 * k drawing from the engine keyed (seed, ray_begin + k, sample_begin + s), include/pt/
 * pt_engine.h -- summed in `order` and divided by spp: with spp = 1 the
 * traceRay value itself (as (0 + c) / 1: a -0 channel reads +0), with the
 * camera ray of a point and spp = sampleCount tracePixel's float-coordinate
 * overload (path-trace.h:172-185). */
typedef struct pt_trace_params {
    int spp;                       /* samples per ray (>= 1)                                    */
    int depth;                     /* rayDepth                                                  */
    uint64_t seed;                 /* run seed of the per-(ray, sample) engine                  */
    int order;                     /* PT_ORDER_*                                                */
    int device;                    /* HIP device ordinal                                        */
    int sample_begin;              /* engine sample index of the first sample                   */
    int64_t max_buffer_bytes;      /* per-sample staging budget (0 = 8 GiB)                     */
    int64_t ray_begin;             /* engine key index of rays[0] (ray k: ray_begin + k), so
                                      successive calls can draw fresh streams                  */
} pt_trace_params;
int pt_trace_rays(pt_scene *s, const pt_trace_params *p, const float *rays, int64_t n, float *rgb_out,
                  pt_render_stats *stats);
/* JIT-compile (or fetch from the cache) pt_trace_rays' module for this scene
 * and depth without touching a GPU. */
int pt_trace_compile(pt_scene *s, int depth);

/* Chained rendering: the reference's one deterministic mode, a program that
 * owns a single DefaultRandomEngine and calls tracePixel / traceRay with it
 * entry after entry, every sample starting where the one before left the
 * engine.  A chain is such a sequence: entries begin[c] .. begin[c + 1] - 1 of
 * `pixels` (indices py * width + px; each entry is tracePixel<T>'s int
 * overload, include/path-trace.h:187-201) or of `rays` (7 floats as for
 * pt_trace_rays; each entry is the sample loop of :178-183 over traceRay<T>
 * with the ray's strength), with ONE engine threaded through every sample of
 * every entry, starting from states[c] (DefaultRandomEngine's 64-bit state v,
 * the recurrence of include/pt/pt_engine.h; seed(x) leaves (uint32_t)x ^
 * 0x12476242).  Exactly one of pixels / rays is given.
 * Chains are independent of each other and run side by side; a chain's samples
 * run one after another, so the call issues max(entries of a chain) x spp
 * launches of the chained module, each tracing at most one sample of every
 * chain in the reference's order.  Results are the reference's bit for bit:
 * rgb_out[3e..] = entry e's colour, state_after[e] = the engine's state after
 * entry e (may be NULL), states[c] = after chain c's last entry (an empty
 * chain's stays as given).  A chain cut in two calls, the second starting from
 * the first's returned state, gives the same results as one call.
 * Arguments are checked before any device is touched: PT_ERR_ARG names the
 * argument in pt_last_error(). */
typedef struct pt_chain_params {
    int width, height;             /* screenXResolution, screenYResolution (pixels only)        */
    int spp;                       /* sampleCount (>= 1)                                        */
    int depth;                     /* rayDepth                                                  */
    float screen_w, screen_h, screen_dist; /* pixels only                                       */
    int device;                    /* HIP device ordinal                                        */
} pt_chain_params;
int pt_trace_chains(pt_scene *s, const pt_chain_params *p, const int32_t *pixels, const float *rays,
                    const int64_t *begin, int64_t nchains, uint64_t *states, float *rgb_out,
                    uint64_t *state_after, pt_render_stats *stats);
/* JIT-compile (or fetch from the cache) pt_trace_chains' module for this scene
 * and depth -- the pixel kind, or with rays != 0 the ray kind -- without
 * touching a GPU. */
int pt_chain_compile(pt_scene *s, int depth, int rays);

/* Everything a render with p needs -- code object loaded, scene parameters
 * and images uploaded, staging buffers allocated -- without rendering, so a
 * timed or latency-sensitive render does no compilation or allocation. */
int pt_prepare(pt_scene *s, const pt_render_params *p);

/* JIT-compile (or fetch from the code-object cache) the megakernel for this
 * scene and depth without touching a GPU.  Used by build() to pre-populate the
 * in-tree cache. */
int pt_scene_compile(pt_scene *s, int depth);
/* MI355X tuning knob, no reference counterpart: build this scene's megakernel
 * for 1..5 resident workgroups (of 4 waves) per CU instead of the most its
 * LDS allows (0 = auto).  Fewer workgroups raise the VGPR cap (5: 96, 4: 128,
 * 3: 168, 2: 256): scenes whose CSG tree spills at the default cap and whose
 * samples are mostly spine walks run faster (C5: 2.3x at 2), burst-bound
 * scenes slower (C2 at 2: -8 %).  Takes effect at the next compile/render. */
int pt_scene_set_occupancy(pt_scene *s, int workgroups_per_cu);
/* MI355X tuning knob, no reference counterpart: the wave-walked (spine) and
 * lane-walked (camera, lane-finished child) queries of this scene first take
 * every primitive's span and the fast checks, and run the lazy merge only
 * where those cannot decide (same bits either way).  Pays where rays rarely
 * start inside overlapping CSG spans (C5: 288 -> 568 Msamples/s), costs
 * where they often do (C3 spine: -0.9 %).  Takes effect at the next
 * compile/render. */
int pt_scene_set_fast_spine(pt_scene *s, int on);
/* MI355X tuning knob, no reference counterpart: each lane of a chunk walks its
 * own sample's ray tree when no node of it has a scatter loop (mirrors, glass,
 * emitters), with `frames` (1..8) register frames for pending nodes; samples
 * that need a scatter loop or a deeper stack go to the wave as before (same
 * bits either way).  Pays where such trees are common (C5's glass ball), costs
 * registers elsewhere.  0 = off.  Takes effect at the next compile/render. */
int pt_scene_set_lane_walk(pt_scene *s, int frames);
/* MI355X tuning knob, no reference counterpart: each lane of a chunk walks its
 * own sample's whole ray tree, scatter loops included, drawing its engine's
 * numbers one rejection attempt after another; loops of more than 64 children
 * that mostly end in leaves (a plain diffuse bounce) and fast-order runs of
 * more than 64 non-zero terms go to the wave as before (same bits either way).
 * Pays where scatter loops are small or recurse often (C2's
 * matBrightDiffuseWhite: ~10^4 children, a quarter of them recursing into a
 * dozen leaves each); supersedes pt_scene_set_lane_walk.  Takes effect at the
 * next compile/render. */
int pt_scene_set_lane_scatter(pt_scene *s, int on);
/* MI355X tuning knob, no reference counterpart: each lane of a chunk keeps its
 * sample and walks the whole ray tree; at a scatter loop it suspends, the wave
 * runs that one burst for it and hands back the sum and the advanced engine
 * state, and the lane resumes.  The wave never walks a sample's spine (same
 * bits either way).  Applies where no burst can end in a recursing child
 * (pt_scene_reach_facts: bursts_all_leaf) and neither pt_scene_set_lane_walk
 * nor pt_scene_set_lane_scatter is chosen; asked for elsewhere, the module is
 * built without it.  1 = on, 0 = off, -1 = auto (the default).  Takes effect
 * at the next compile/render. */
int pt_scene_set_lane_resume(pt_scene *s, int on);
/* MI355X tuning knob, no reference counterpart: lane-walk scenes render in
 * split launches (default on) -- a light kernel (no lazy merges, no wave walk,
 * higher occupancy) over every chunk, then the full kernel over the chunks
 * with a lane it could not finish.  A chunk's sums come from one kernel, so
 * the bits are the same either way.  0 = every chunk through the full kernel.
 * Takes effect at the next render. */
int pt_scene_set_split(pt_scene *s, int on);
/* Key of the code object for this scene/depth: a hash of the generated source,
 * the compiler options and the hiprtc version -- the file name of its entry in
 * the code-object cache (hex string, thread-local storage). */
const char *pt_scene_kernel_key(pt_scene *s, int depth);
/* The same for any of the scene's module kinds: rays != 0 the ray-list module
 * of pt_trace_rays, chain != 0 the chained module of pt_trace_chains (with
 * rays, its ray kind); both 0 is pt_scene_kernel_key. */
const char *pt_scene_module_key(pt_scene *s, int depth, int rays, int chain);
/* What code generation proved about the scatter bursts this scene's materials
 * can reach; the render kernel is compiled with only those variants.
 * *kr_reach: bit 0 = a burst with scatter coefficient exactly 1 is possible,
 * bit 1 = one with another coefficient (3 = both or unknown, 0 = no material
 * scatters).  *bursts_all_leaf: 1 when every child of every burst is provably
 * a leaf (strength below eps), else 0.  Either pointer may be null. */
int pt_scene_reach_facts(pt_scene *s, int *kr_reach, int *bursts_all_leaf);

/* ------------------------------------------------------------ queries --- */
/* The reference's query virtuals, evaluated on the device.
 *
 * pt_query_spans: obj->makeSpanIterator() (include/object.h:14), then for each
 * ray (6 floats: origin xyz, direction xyz) init(ray) and next() until
 * isAtEnd() (include/span.h:129-171).  counts[i] receives ray i's number of
 * spans; the first min(counts[i], max_spans) spans go to out[i * max_spans ..]
 * in the reference's Span form (span.h:12-120; materials as pt_ids).  obj < 0
 * queries the scene root.  The lists are bit-identical to the reference's,
 * including the Difference quirk (src/difference.cpp:124-130). */
typedef struct pt_span {
    float t_start, n_start[3];     /* start, startNormal   */
    int32_t mat_start;             /* startMaterial        */
    float t_end, n_end[3];         /* end, endNormal       */
    int32_t mat_end;               /* endMaterial          */
} pt_span;
int pt_query_spans(pt_scene *s, pt_id obj, const float *rays, int64_t n, int max_spans, pt_span *out,
                   int32_t *counts, int device);
/* Texture::getColor (rgb: 3 floats per point) and Texture::getFloat (value: 1
 * float per point) of texture tex at n points (3 floats each),
 * include/texture.h:13-18 with every subclass's override. */
int pt_tex_eval(pt_scene *s, pt_id tex, const float *points, int64_t n, float *rgb, float *value, int device);
/* Compile (or fetch from the code-object cache) the query module of obj
 * (-1: the root, when tex < 0; -2: none) and/or tex (-1: none), without a
 * device. */
int pt_query_compile(pt_scene *s, pt_id obj, pt_id tex);

/* What traceRay sees at the first surface (include/path-trace.h:66-129), for n
 * caller rays (6 floats each: origin xyz, direction xyz, not normalised) against
 * the scene root, one ray per lane of the scene's guides module
 * (path-trace_amd/csrc/device/pt_guides.h).  path chooses the query:
 * PT_HIT_MERGE the lazy merge of the CSG tree, traceRay's scan itself;
 * PT_HIT_FAST every primitive's span and the fast checks first and the lazy
 * merge only on the rays the checks cannot decide, as the render kernel's spine
 * and lane queries run.  Both give the same bits in every field.
 * out[i]: hit = 0 / 1 (a span list that runs out and a span at or beyond 1e20
 * are both 0); exit = 1 when the hit is a span's end; t the ray parameter;
 * normal the shading normal (the span's, negated on an exit; not normalised
 * again); pos = origin + t * direction; material its pt_id; ior the material's
 * own.  On a miss hit = exit = 0, material = -1 and every float is +0.
 * shade_out (NULL, or 11 floats per ray) receives the material's five texture
 * lookups at pos, unclamped: emissive rgb, reflect rgb, transmit rgb, scatter
 * coefficient, transmit-reflect coefficient (:101-129); +0 on a miss.
 * decided (NULL, or one int per ray) receives the fast check's verdict for the
 * ray, hit or miss: 1 where span_first_hit's answer stood, 0 where the ray took
 * the lazy merge; always 0 on PT_HIT_MERGE.
 * Rays must have finite components and a non-zero direction, as for
 * pt_trace_rays.  Every argument is checked before a device is touched:
 * PT_ERR_ARG names the argument in pt_last_error(). */
#define PT_HIT_FAST 0
#define PT_HIT_MERGE 1
typedef struct pt_hit {
    int32_t hit, exit, material;
    float t, normal[3], pos[3], ior;
} pt_hit;
int pt_query_hits(pt_scene *s, const float *rays, int64_t n, int path, pt_hit *out, float *shade_out,
                  int32_t *decided, int device);

/* Guide buffers beside the beauty image: per pixel entry, means over the
 * camera samples of what the first hit shows.  Sample s = p->sample_begin ..
 * p->sample_begin + p->spp - 1 of pixel index y * grid_width + x draws its camera
 * ray from the engine keyed (p->seed, index, s) exactly as pt_render does, and is
 * queried with PT_HIT_FAST.  Summation rule: each quantity is accumulated in
 * f32 from +0 in sample order, acc = acc + x_s, a miss adding +0, and divided by
 * (float)spp at the end.  So `emission` is pt_render's frame at depth 0 in
 * PT_ORDER_REFERENCE, bit for bit.  Planes (host memory; NULL = skip):
 * emission, albedo (the reflect colour) and normal (the shading normal, not
 * normalised again) 3 floats per entry; t (misses as 0) and coverage (hits /
 * spp) 1 float; material 1 int, the pt_id at the first sample's hit or -1.
 * Entries are p->pixels (compact: entry k at k) or the whole frame, row-major.
 * Honoured: width, height, spp, screen_w / _h / _dist, seed, device, pixels,
 * npixels, grid_width, sample_begin; depth, order, sum_only and max_buffer_bytes
 * are ignored.  Every argument is checked before a device is touched:
 * PT_ERR_ARG names the argument in pt_last_error(). */
typedef struct pt_guide_buffers {
    float *emission, *albedo, *normal, *t, *coverage;
    int32_t *material;
} pt_guide_buffers;
int pt_render_guides(pt_scene *s, const pt_render_params *p, const pt_guide_buffers *out);
/* JIT-compile (or fetch from the code-object cache) the scene's guides module
 * -- pt_query_hits' and pt_render_guides' kernels -- without touching a GPU. */
int pt_guides_compile(pt_scene *s);
/* Its code-object key (as pt_scene_module_key: hex string, thread-local). */
const char *pt_scene_guides_key(pt_scene *s);

/* Guide-driven denoiser, no reference counterpart: an edge-avoiding a-trous
 * wavelet filter with variance guidance (Dammertz et al. 2010; the spatial part
 * of Schied et al. 2017) over a width x height frame, row-major, one entry per
 * pixel, on the device (path-trace_amd/csrc/device/pt_denoise.h; one module for
 * every scene).  Planes as pt_guide_buffers names them: rgb the beauty image
 * (3 floats), err (NULL, or 1 float) the standard error of the mean r + g + b
 * as pt_render_converge's err_out, normal (3), t (1, used as given), material
 * (1 int, -1 a miss), albedo and emission (3 each; read only with demodulate).
 * Every expression is f32, one rounding per operator in the order written; a
 * comparison with a NaN is false.
 *  Prepare, per pixel: a = demodulate ? (albedo > 0.01 ? albedo : 0.01) per
 *   channel : 1, e = demodulate ? emission : 0; the signal s = (rgb - e) / a
 *   (without demodulate s is rgb itself); abar = ((a.r + a.g) + a.b) / 3; the
 *   variance v = err err / (abar abar) where err is finite, else +0.  With err
 *   NULL, v is the sample variance of Y(s) = (s.r + s.g) + s.b over the pixels of
 *   the 5 x 5 neighbourhood that are in the image, share the centre's material
 *   and have a finite Y: n of them, S1 their sum in row-major order, m = S1 / n,
 *   S2 the sum of (Y - m)^2 in the same order, v = S2 / (n - 1), or 0 for n < 2.
 *   nhat = normal / sqrt((nx nx + ny ny) + nz nz) if that sum is > 0, else 0.
 *  Pass i = 0 .. iterations - 1, step = 2^i, from one (s, v) buffer into another:
 *   vt = the 3 x 3 Gaussian (1/4, 1/2, 1/4)^2 of v around p, coordinates clamped
 *   to the image and a neighbour of another material taken as p itself,
 *   accumulated from +0 in row-major order; den = sigma_l sqrt(vt >
 *   0 ? vt : 0) + 1e-4; E(x) = x < 1 ? (1 - x)^2 : 0.  Taps (dy, dx) in -2 .. 2,
 *   row-major, q = p + step (dx, dy), k = (3/8, 1/4, 1/16).  The centre tap has w
 *   = 9/64.  Another tap is skipped if q is outside the image or material[q] !=
 *   material[p]; else h = k[|dy|] k[|dx|]; wn = max(0, (nx nx' + ny ny') + nz
 *   nz') squared normal_power_log2 times; d = |t_p - t_q|, wz = d > 0 ? E(d /
 *   (sigma_z max(t_p, t_q))) : 1; where material[p] is -1, wn = wz = 1; dl =
 *   |Y(s_p) - Y(s_q)|, wl = E(dl / den), and with sigma_l = +inf wl = dl < inf ?
 *   1 : 0; w = ((h wn) wz) wl.  A tap whose w is not > 0 is left out (not
 *   multiplied by zero: a non-finite neighbour cannot spread).  In tap order, from
 *   +0: Sc += w s_q, Sv += (w w) v_q, Sw += w; then s' = Sc / Sw, v' = Sv / (Sw
 *   Sw).  Sw >= 9/64.
 *  Finalise: out = e + s a, var_out = v (abar abar); without demodulate out = s
 *   and var_out = v.
 * tests/denoise_model.py restates this in numpy, bit for bit. */
typedef struct pt_denoise_params {
    int width, height;
    int iterations;                /* 0..8 (0: prepare and finalise only); 5 is the usual choice */
    float sigma_l;                 /* > 0; +inf switches the luminance weight off; usual 2       */
    float sigma_z;                 /* > 0; usual 0.1                                             */
    int normal_power_log2;         /* 0..8; usual 5 (the 32nd power)                             */
    int demodulate;                /* 0 or 1                                                     */
    int device;
} pt_denoise_params;
typedef struct pt_denoise_buffers {
    const float *rgb, *err, *normal, *t;
    const int32_t *material;
    const float *albedo, *emission; /* may be NULL without demodulate                            */
    float *out;                     /* 3 floats per pixel                                        */
    float *var_out;                 /* NULL, or 1 float per pixel                                */
} pt_denoise_buffers;
/* The planes are host memory: upload, pt_denoise_device, download.  Records
 * PT_PROF_TOTAL and PT_PROF_KERNEL (prepare to finalise, by HIP events) for
 * pt_call_profile.  Every argument is checked before a device is touched:
 * PT_ERR_ARG names the argument in pt_last_error(). */
int pt_denoise(const pt_denoise_params *p, const pt_denoise_buffers *b);
/* The planes are device memory of p->device; the kernels are only enqueued on
 * the hipStream_t (NULL = default stream).  out may be rgb itself.  The filter's
 * records (48 bytes a pixel) are kept per device and grow with the largest frame
 * seen (the only allocation); calls on one device share them, so two calls must
 * not run at the same time on different streams. */
int pt_denoise_device(const pt_denoise_params *p, const pt_denoise_buffers *b, void *stream);
/* pt_denoise_device that waits for its launches and returns the device time of
 * each, by HIP events: ms[0] prepare, ms[1 .. iterations] the passes,
 * ms[iterations + 1] finalise (iterations + 2 floats). */
int pt_denoise_device_timed(const pt_denoise_params *p, const pt_denoise_buffers *b, void *stream, float *ms);
/* JIT-compile (or fetch from the code-object cache) the denoiser's module
 * without touching a GPU. */
int pt_denoise_compile(void);
/* Its code-object key (hex string, thread-local). */
const char *pt_denoise_key(void);

/* Device self-test: the megakernel's exact fast paths for f32 sqrt / '/' /
 * normalize against the compiler's correctly rounded ones on n hashed inputs.
 * mismatches[0..2] receive the sqrt, div and normalize mismatch counts. */
int pt_selftest_math(int device, uint64_t n, uint64_t seed, uint64_t *mismatches);

/* Device self-test of the restated glibc float libm the texture maps use
 * (SphericalCoordinatesSkymapTexture's atan2f / asinf, transform_texture.h:
 * 73-85; LogTexture's logf, filter_texture.h:62-67): for n operand pairs
 * ops[2i] = y, ops[2i+1] = x, out[3i..3i+2] = atan2f(y, x), asinf(y), logf(x)
 * as the device computes them, for comparison with the host's libm. */
int pt_selftest_libm(int device, const float *ops, int64_t n, float *out);

/* ------------------------------------------------------------- output --- */
/* MutableImage::writeHDR (reference src/image.cpp:398-481), rgb = w*h*3 floats. */
int pt_write_hdr(const char *path, const float *rgb, int w, int h);
/* 24-bpp BGR bottom-up BMP as SDL_SaveBMP writes it, bytes
 * clamp(floor(256*c/count), 0, 255) (reference src/test.cpp:1037-1059). */
int pt_write_bmp(const char *path, const float *rgb, int w, int h, int count);

#ifdef __cplusplus
}
#endif

#endif
