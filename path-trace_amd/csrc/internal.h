/* internal.h -- host-side data model of libpt.so (not part of the C ABI). */
#ifndef PT_INTERNAL_H
#define PT_INTERNAL_H

#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pt/pt.h"

namespace pt
{

/* An error carrying a C-ABI status code; caught at every extern "C" boundary. */
struct Error : std::runtime_error
{
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

void set_error(const std::string &msg); /* pt_last_error's text (scene.cpp) */
/* pt_call_profile's record of the calling thread's last call, and its clock (runtime.cpp) */
extern thread_local double g_prof[PT_PROF_N];
double now_us();

/* Every extern "C" entry runs its body through this. */
template <class F>
int guard(F f)
{
    try {
        return f();
    } catch (Error &e) {
        set_error(e.what());
        return e.code;
    } catch (std::exception &e) {
        set_error(e.what());
        return PT_ERR_ARG;
    }
}

/* A key entry: k = f(), or "" and pt_last_error's text if f throws */
template <class F>
const char *key_text(std::string &k, F f)
{
    try {
        k = f();
    } catch (std::exception &e) {
        set_error(e.what());
        k.clear();
    }
    return k.c_str();
}

/* Host copies of the reference scene graph, one record per constructor call. */
struct ImageRec
{
    int w = 0, h = 0;
    std::vector<float> rgba; /* row 0 = top */
};

enum class TexKind { Color, Image, ImageAlpha, Skybox, SkyboxAlpha, Multiply, Log, MirrorBall, Spherical, Xform, Coord, User };

struct TexRec
{
    TexKind kind;
    float f[12] = {0};
    int child = -1;   /* inner texture */
    int img[6] = {-1, -1, -1, -1, -1, -1};
    /* User (pt_tex_device): the caller's device bodies and parameters */
    std::string color_body, value_body;
    std::vector<float> params;
};

struct MatRec
{
    int reflect, scatter, emissive, transmit, trc;
    float ior;
};

enum class ObjKind { Sphere, Plane, Union, Intersection, Difference, Xform, User };

struct ObjRec
{
    ObjKind kind;
    float f[12] = {0}; /* sphere: c, r; plane: n, d; xform: m */
    int mat = -1;
    int a = -1, b = -1; /* children */
    /* User (pt_object_device): the caller's device bodies and parameters */
    std::string span_body, normal_body;
    std::vector<float> params;
    /* User through pt_object_device_spans: the primitive slots its span list
     * takes, 1..PT_OBJECT_MAX_SPANS (0 = pt_object_device's one-span form) */
    int max_spans = 0;
};

struct DeviceState; /* device_state.h */
struct DeviceStateDelete /* on the state's own device (runtime.cpp) */
{
    void operator()(DeviceState *ds) const;
};
struct Generated;

struct SceneImpl
{
    std::vector<ImageRec> images;
    std::vector<TexRec> textures;
    std::vector<MatRec> materials;
    std::vector<ObjRec> objects;
    int root = -1;
    int default_tex[2] = {-1, -1}; /* lazily created ColorTexture(0), ColorTexture(1) */
    int wg_per_cu = 0;             /* resident workgroups per CU the kernel is built for (0 = auto) */
    int fast_spine = 0;            /* spine queries try all spans + the fast checks first */
    int lane_walk = 0;             /* register frames of the per-lane scatter-free tree walk (0 = off) */
    int lane_scatter = 0;          /* per-lane walk of whole trees, scatter loops included */
    int lane_resume = -1;          /* lanes walk whole trees, the wave serves their bursts (-1 = auto) */
    int split = 1;                /* lane-walk scenes: light kernel first (launch-time only) */
    std::map<int, std::unique_ptr<DeviceState, DeviceStateDelete>> devices;
    std::shared_ptr<struct QueryCache> qcache; /* loaded query modules (query.cpp) */
    std::string last_key;
    /* generated render modules by a fingerprint of everything generate() reads
     * (runtime.cpp generated(): per-call callers skip the ~200 KB source text) */
    std::map<uint64_t, std::shared_ptr<const Generated>> gen_cache;
    void clear()
    {
        images.clear(), textures.clear(), materials.clear(), objects.clear();
        gen_cache.clear();
        qcache.reset(); /* its modules hold copies of the old images */
        root = -1;
        default_tex[0] = default_tex[1] = -1;
    }
};

/* Generated device module for one (scene, depth). */
struct Generated
{
    std::string source;         /* full hiprtc translation unit                      */
    std::string key;            /* content hash of the source (code_object_key adds options + compiler) */
    std::vector<float> params;  /* scene parameter block P                           */
    std::vector<int> image_ids; /* slot -> scene image index                          */
    std::vector<int> mat_ids;   /* compact material index -> scene material index     */
    int maxd = 0;
    int n_prims = 0, n_spheres = 0, n_planes = 0, n_mats = 0;
    std::vector<std::string> options; /* per-scene compiler options (part of the code-object key) */
    int kr_reach = 3;                 /* burst variants reachable: bit 0 sc == 1, bit 1 sc != 1 (codegen reach_facts) */
    bool bursts_all_leaf = false;     /* every burst's children are provably leaves */
};

/* rays: the module of pt_trace_rays (PT_RAYS), whose items are caller rays;
 * chain: the module of pt_trace_chains (PT_CHAIN), whose items draw from a
 * chain's own engine state, one sample of each chain per launch */
Generated generate(const SceneImpl &s, int depth, bool rays = false, bool chain = false);
/* The guides module of pt_query_hits / pt_render_guides: the scene's full
 * `ptgen::Scene` as generate() writes it -- root type and material dispatchers
 * -- under none of the render kernels' per-scene knobs, followed by
 * device/pt_guides.h and its two kernels instead of the render kernels. */
Generated generate_guides(const SceneImpl &s);

/* pt_trace_chains' step sequence.  Chain c has len[c] * spp steps; step t runs
 * the chains with more than t steps.  order = the chain ids by descending
 * length (ties by id), so those chains are the prefix order[0 .. items[t]);
 * items has one count per step, max(len) * spp of them. */
void chain_schedule(const int64_t *begin, int64_t nchains, int spp, std::vector<int32_t> &order,
                    std::vector<int64_t> &items);
/* pt_trace_chains' argument check, before any device is touched: throws
 * Error(PT_ERR_ARG) naming the argument */
void chain_validate(const pt_chain_params *p, const int32_t *pixels, const float *rays, const int64_t *begin,
                    int64_t nchains, const uint64_t *states, const float *rgb_out);
/* The argument check of every render: throws Error(PT_ERR_ARG) (runtime.cpp) */
void validate(const pt_render_params *p);
/* The ray check of pt_trace_rays, pt_trace_chains and pt_query_hits (chain.cpp):
 * n rays of `stride` floats, origin and direction first.  Throws
 * Error(PT_ERR_ARG) "<prefix><k> has ..." for the first ray with a zero
 * direction or a non-finite origin or direction; a prefix ending in '[' gets
 * its ']' after k. */
void check_rays(const float *rays, int64_t n, int stride, const std::string &prefix);
/* Query module for the boundary's query virtuals: pt_query_spans over object
 * `obj` (if >= 0) and pt_tex_eval of texture `tex` (if >= 0). */
Generated generate_query(const SceneImpl &s, int obj, int tex);
/* Returns the gfx950 code object for g (from the cache or compiled now). */
const std::vector<char> &code_object(const Generated &g);
/* The code object's cache key: source + compiler options + hiprtc version
 * (the _jit_cache file name; what a profile is bound to). */
std::string code_object_key(const Generated &g);

/* Matrix helpers (reference include/transform.h arithmetic). */
void mat_inverse(const float *m, float *out); /* throws Error(PT_ERR_MATH) */
void mat_concat(const float *a, const float *b, float *out);
void mat_rotate(const float *axis, double angle, float *out);

/* Image I/O (reference src/image.cpp). */
ImageRec read_hdr(const std::string &path);
ImageRec read_png(const std::string &path);
ImageRec read_image(const std::string &path);
void write_hdr(const std::string &path, const float *rgb, int w, int h);
void write_bmp(const std::string &path, const float *rgb, int w, int h, int count);

/* embedded pt_device.h; without its PT_CHAIN regions unless chain, so that the
 * text -- and with it the code-object key -- of every other module kind is
 * what it would be had the chained kind never been written */
std::string device_library_source(bool chain = false);
std::string device_user_object_source(); /* embedded pt_user_object.h (scenes with user objects) */
std::string device_user_object_n_source(); /* embedded pt_user_object_n.h (scenes with multi-span user objects) */
std::string device_converge_source(); /* embedded pt_converge.h (pt_render_converge's scene-independent module) */
std::string device_guides_source(); /* embedded pt_guides.h (the guides module: pt_query_hits, pt_render_guides) */
std::string device_denoise_source(); /* embedded pt_denoise.h (pt_denoise's scene-independent module) */

} // namespace pt

struct pt_scene
{
    pt::SceneImpl impl;
};

namespace pt
{

inline SceneImpl &S(pt_scene *s)
{
    if (!s)
        throw Error(PT_ERR_ARG, "null scene");
    return s->impl;
}
inline void check_id(int id, size_t count, const char *what)
{
    if (id < 0 || id >= (int)count)
        throw Error(PT_ERR_ARG, std::string("bad ") + what + " id " + std::to_string(id));
}
inline void check_img(const SceneImpl &s, int id) { check_id(id, s.images.size(), "image"); }
inline void check_tex(const SceneImpl &s, int id) { check_id(id, s.textures.size(), "texture"); }
inline void check_mat(const SceneImpl &s, int id) { check_id(id, s.materials.size(), "material"); }
inline void check_obj(const SceneImpl &s, int id) { check_id(id, s.objects.size(), "object"); }

} // namespace pt

#endif
