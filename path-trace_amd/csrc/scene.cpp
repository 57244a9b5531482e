/*
 * scene.cpp -- the host copy of the scene graph behind include/pt/pt.h: the
 * reference-shaped constructors, the plain-text scene format, the per-scene
 * knobs, module keys and compiles that need no device, the matrix helpers and
 * the image file wrappers.  No HIP in this file.
 */
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

#include "internal.h"

namespace pt
{

thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

/* ------------------------------------------------------------ matrices -- */
/* transform.h:342-383 */
void mat_inverse(const float *m, float *out)
{
    const float x00 = m[0], x10 = m[1], x20 = m[2], x30 = m[3], x01 = m[4], x11 = m[5], x21 = m[6], x31 = m[7],
                x02 = m[8], x12 = m[9], x22 = m[10], x32 = m[11];
    float det = x00 * (x11 * x22 - x12 * x21) + x10 * (x02 * x21 - x01 * x22) + x20 * (x01 * x12 - x02 * x11);
    if (det == 0.0f)
        throw Error(PT_ERR_MATH, "can't invert singular matrix");
    float f = 1.0f / det;
    out[0] = (x11 * x22 - x12 * x21) * f;
    out[1] = (x12 * x20 - x10 * x22) * f;
    out[2] = (x10 * x21 - x11 * x20) * f;
    out[3] = (-x10 * x21 * x32 + x11 * x20 * x32 + x10 * x22 * x31 - x12 * x20 * x31 - x11 * x22 * x30 +
              x12 * x21 * x30) *
             f;
    out[4] = (x02 * x21 - x01 * x22) * f;
    out[5] = (x00 * x22 - x02 * x20) * f;
    out[6] = (x01 * x20 - x00 * x21) * f;
    out[7] = (x00 * x21 * x32 - x01 * x20 * x32 - x00 * x22 * x31 + x02 * x20 * x31 + x01 * x22 * x30 -
              x02 * x21 * x30) *
             f;
    out[8] = (x01 * x12 - x02 * x11) * f;
    out[9] = (x02 * x10 - x00 * x12) * f;
    out[10] = (x00 * x11 - x01 * x10) * f;
    out[11] = (-x00 * x11 * x32 + x01 * x10 * x32 + x00 * x12 * x31 - x02 * x10 * x31 - x01 * x12 * x30 +
               x02 * x11 * x30) *
              f;
}

/* Matrix::concat, transform.h:391-406: this->concat(rt) = "apply this, then rt" */
void mat_concat(const float *a, const float *b, float *out)
{
    const float t00 = a[0], t10 = a[1], t20 = a[2], t30 = a[3], t01 = a[4], t11 = a[5], t21 = a[6], t31 = a[7],
                t02 = a[8], t12 = a[9], t22 = a[10], t32 = a[11];
    const float r00 = b[0], r10 = b[1], r20 = b[2], r30 = b[3], r01 = b[4], r11 = b[5], r21 = b[6], r31 = b[7],
                r02 = b[8], r12 = b[9], r22 = b[10], r32 = b[11];
    out[0] = t00 * r00 + t01 * r10 + t02 * r20;
    out[1] = t10 * r00 + t11 * r10 + t12 * r20;
    out[2] = t20 * r00 + t21 * r10 + t22 * r20;
    out[3] = t30 * r00 + t31 * r10 + t32 * r20 + r30;
    out[4] = t00 * r01 + t01 * r11 + t02 * r21;
    out[5] = t10 * r01 + t11 * r11 + t12 * r21;
    out[6] = t20 * r01 + t21 * r11 + t22 * r21;
    out[7] = t30 * r01 + t31 * r11 + t32 * r21 + r31;
    out[8] = t00 * r02 + t01 * r12 + t02 * r22;
    out[9] = t10 * r02 + t11 * r12 + t12 * r22;
    out[10] = t20 * r02 + t21 * r12 + t22 * r22;
    out[11] = t30 * r02 + t31 * r12 + t32 * r22 + r32;
}

/* Matrix::rotate, transform.h:207-225 (cos/sin of a double angle, float math) */
void mat_rotate(const float *axis, double angle, float *out)
{
    float ax = axis[0], ay = axis[1], az = axis[2];
    float m = std::sqrt((ax * ax + ay * ay) + az * az);
    if (m == 0)
        m = 1;
    ax /= m, ay /= m, az /= m;
    float c = (float)std::cos(angle), s = (float)std::sin(angle), v = 1 - c;
    float xx = ax * ax, xy = ax * ay, xz = ax * az, yy = ay * ay, yz = ay * az, zz = az * az;
    float r[12] = {xx + (1 - xx) * c, xy * v - az * s, xz * v + ay * s, 0, xy * v + az * s, yy + (1 - yy) * c,
                   yz * v - ax * s,   0,               xz * v - ay * s, yz * v + ax * s, zz + (1 - zz) * c, 0};
    memcpy(out, r, sizeof r);
}

/* -------------------------------------------------------------- helpers -- */
namespace
{

int add_tex(SceneImpl &s, const TexRec &t)
{
    s.textures.push_back(t);
    return (int)s.textures.size() - 1;
}

int default_tex(SceneImpl &s, int which) /* ColorTexture(0) / ColorTexture(1) */
{
    TexRec t;
    t.kind = TexKind::Color;
    t.f[0] = t.f[1] = t.f[2] = (float)which;
    return add_tex(s, t);
}

std::string trim(const std::string &s)
{
    size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r");
    return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

float tof(const std::string &t)
{
    char *end = nullptr;
    float v = strtof(t.c_str(), &end);
    if (end == t.c_str() || *end)
        throw Error(PT_ERR_ARG, "bad float '" + t + "'");
    return v;
}

int toi(const std::string &t)
{
    char *end = nullptr;
    long v = strtol(t.c_str(), &end, 10);
    if (end == t.c_str() || *end)
        throw Error(PT_ERR_ARG, "bad int '" + t + "'");
    return (int)v;
}

/* Loads the plain-text scene format into s (ids are renumbered). */
void load_text(SceneImpl &s, const std::string &text)
{
    s.clear();
    std::map<int, int> img, tex, mat, obj;
    std::istringstream in(text);
    std::string line;
    int root = -1;
    auto need = [](const std::vector<std::string> &t, size_t n) {
        if (t.size() != n)
            throw Error(PT_ERR_ARG, "scene text: wrong operand count near '" + (t.empty() ? "" : t[0]) + "'");
    };
    auto look = [](std::map<int, int> &m, int id, const char *what) {
        auto it = m.find(id);
        if (it == m.end())
            throw Error(PT_ERR_ARG, std::string("scene text: unknown ") + what + " " + std::to_string(id));
        return it->second;
    };
    while (std::getline(in, line)) {
        line = trim(line);
        if (line.empty() || line[0] == '#')
            continue;
        std::istringstream ls(line);
        std::vector<std::string> t;
        std::string w;
        while (ls >> w) t.push_back(w);
        const std::string &k = t[0];
        if (k == "root") {
            need(t, 2);
            root = look(obj, toi(t[1]), "object");
            continue;
        }
        if (t.size() < 3)
            throw Error(PT_ERR_ARG, "scene text: short line");
        int id = toi(t[1]);
        const std::string &ty = t[2];
        if (k == "image") {
            if (ty == "hdr") {
                need(t, 4);
                s.images.push_back(read_hdr(t[3]));
            } else if (ty == "png") {
                need(t, 4);
                s.images.push_back(read_png(t[3]));
            } else if (ty == "raw") {
                need(t, 6);
                ImageRec r;
                r.w = toi(t[3]), r.h = toi(t[4]);
                std::ifstream f(t[5], std::ios::binary);
                if (!f)
                    throw Error(PT_ERR_IO, "can't open " + t[5]);
                r.rgba.resize((size_t)4 * r.w * r.h);
                f.read((char *)r.rgba.data(), (std::streamsize)(r.rgba.size() * 4));
                if (!f)
                    throw Error(PT_ERR_IO, "short raw image " + t[5]);
                s.images.push_back(std::move(r));
            } else
                throw Error(PT_ERR_ARG, "scene text: image kind " + ty);
            img[id] = (int)s.images.size() - 1;
        } else if (k == "tex") {
            TexRec r;
            if (ty == "color") {
                need(t, 6);
                r.kind = TexKind::Color;
                for (int j = 0; j < 3; j++) r.f[j] = tof(t[3 + j]);
            } else if (ty == "coord") {
                need(t, 3);
                r.kind = TexKind::Coord;
            } else if (ty == "image" || ty == "image_alpha") {
                need(t, 4);
                r.kind = ty == "image" ? TexKind::Image : TexKind::ImageAlpha;
                r.img[0] = look(img, toi(t[3]), "image");
            } else if (ty == "skybox" || ty == "skybox_alpha") {
                need(t, 9);
                r.kind = ty == "skybox" ? TexKind::Skybox : TexKind::SkyboxAlpha;
                for (int j = 0; j < 6; j++) r.img[j] = look(img, toi(t[3 + j]), "image");
            } else if (ty == "multiply") {
                need(t, 7);
                r.kind = TexKind::Multiply;
                for (int j = 0; j < 3; j++) r.f[j] = tof(t[3 + j]);
                r.child = look(tex, toi(t[6]), "texture");
            } else if (ty == "log" || ty == "mirrorball" || ty == "spherical") {
                need(t, 4);
                r.kind = ty == "log" ? TexKind::Log : ty == "mirrorball" ? TexKind::MirrorBall : TexKind::Spherical;
                r.child = look(tex, toi(t[3]), "texture");
            } else if (ty == "xform") {
                need(t, 16);
                r.kind = TexKind::Xform;
                for (int j = 0; j < 12; j++) r.f[j] = tof(t[3 + j]);
                r.child = look(tex, toi(t[15]), "texture");
            } else
                throw Error(PT_ERR_ARG, "scene text: texture kind " + ty);
            tex[id] = add_tex(s, r);
        } else if (k == "mat") {
            need(t, 8);
            MatRec m;
            m.reflect = look(tex, toi(t[2]), "texture");
            m.scatter = look(tex, toi(t[3]), "texture");
            m.emissive = look(tex, toi(t[4]), "texture");
            m.transmit = look(tex, toi(t[5]), "texture");
            m.ior = tof(t[6]);
            m.trc = look(tex, toi(t[7]), "texture");
            s.materials.push_back(m);
            mat[id] = (int)s.materials.size() - 1;
        } else if (k == "obj") {
            ObjRec o;
            if (ty == "sphere" || ty == "plane") {
                need(t, 8);
                o.kind = ty == "sphere" ? ObjKind::Sphere : ObjKind::Plane;
                for (int j = 0; j < 4; j++) o.f[j] = tof(t[3 + j]);
                o.mat = look(mat, toi(t[7]), "material");
            } else if (ty == "union" || ty == "intersection" || ty == "difference") {
                need(t, 5);
                o.kind = ty == "union" ? ObjKind::Union : ty == "intersection" ? ObjKind::Intersection
                                                                                : ObjKind::Difference;
                o.a = look(obj, toi(t[3]), "object");
                o.b = look(obj, toi(t[4]), "object");
            } else if (ty == "xform") {
                need(t, 16);
                o.kind = ObjKind::Xform;
                for (int j = 0; j < 12; j++) o.f[j] = tof(t[3 + j]);
                o.a = look(obj, toi(t[15]), "object");
            } else
                throw Error(PT_ERR_ARG, "scene text: object kind " + ty);
            s.objects.push_back(o);
            obj[id] = (int)s.objects.size() - 1;
        } else
            throw Error(PT_ERR_ARG, "scene text: unknown line kind " + k);
    }
    if (root < 0)
        throw Error(PT_ERR_ARG, "scene text: no root");
    s.root = root;
}

int push_image(pt_scene *s, ImageRec (*read)(const std::string &), const char *path)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        sc.images.push_back(read(path ? path : ""));
        return (int)sc.images.size() - 1;
    });
}

int read_into(ImageRec (*read)(const std::string &), const char *path, float *rgba, int *w, int *h)
{
    return guard([&] {
        ImageRec r = read(path ? path : "");
        if (w)
            *w = r.w;
        if (h)
            *h = r.h;
        if (rgba)
            memcpy(rgba, r.rgba.data(), r.rgba.size() * 4);
        return PT_OK;
    });
}

int push_object(SceneImpl &sc, const ObjRec &o)
{
    sc.objects.push_back(o);
    return (int)sc.objects.size() - 1;
}

template <class F>
int set_knob(pt_scene *s, F f) /* a setter: f(scene), then PT_OK */
{
    return guard([&] {
        f(S(s));
        return PT_OK;
    });
}

} // namespace
} // namespace pt

using namespace pt;

extern "C" {

const char *pt_last_error(void) { return g_error.c_str(); }
const char *pt_version(void) { return "pt-mi355x 0.1 (gfx950)"; }

pt_scene *pt_scene_create(void) { return new pt_scene; }
void pt_scene_destroy(pt_scene *s) { delete s; }

pt_id pt_image_load_hdr(pt_scene *s, const char *path) { return push_image(s, read_hdr, path); }
pt_id pt_image_load_png(pt_scene *s, const char *path) { return push_image(s, read_png, path); }
pt_id pt_image_load(pt_scene *s, const char *path) { return push_image(s, read_image, path); }

pt_id pt_image_from_rgba32f(pt_scene *s, const float *rgba, int w, int h)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (!rgba || w <= 0 || h <= 0)
            throw Error(PT_ERR_ARG, "bad image");
        ImageRec r;
        r.w = w, r.h = h;
        r.rgba.assign(rgba, rgba + (size_t)4 * w * h);
        sc.images.push_back(std::move(r));
        return (int)sc.images.size() - 1;
    });
}

int pt_png_read(const char *path, float *rgba, int *w, int *h) { return read_into(read_png, path, rgba, w, h); }
int pt_hdr_read(const char *path, float *rgba, int *w, int *h) { return read_into(read_hdr, path, rgba, w, h); }

pt_id pt_tex_color(pt_scene *s, float r, float g, float b)
{
    return guard([&] {
        TexRec t;
        t.kind = TexKind::Color;
        t.f[0] = r, t.f[1] = g, t.f[2] = b;
        return add_tex(S(s), t);
    });
}

static pt_id tex_image(pt_scene *s, TexKind k, pt_id image)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        check_img(sc, image);
        TexRec t;
        t.kind = k;
        t.img[0] = image;
        return add_tex(sc, t);
    });
}
pt_id pt_tex_image(pt_scene *s, pt_id image) { return tex_image(s, TexKind::Image, image); }
pt_id pt_tex_image_alpha(pt_scene *s, pt_id image) { return tex_image(s, TexKind::ImageAlpha, image); }

static pt_id tex_skybox(pt_scene *s, TexKind k, const pt_id *f)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        TexRec t;
        t.kind = k;
        for (int j = 0; j < 6; j++) {
            check_img(sc, f[j]);
            t.img[j] = f[j];
        }
        return add_tex(sc, t);
    });
}
pt_id pt_tex_skybox(pt_scene *s, pt_id top, pt_id bottom, pt_id left, pt_id right, pt_id front, pt_id back)
{
    pt_id f[6] = {top, bottom, left, right, front, back};
    return tex_skybox(s, TexKind::Skybox, f);
}
pt_id pt_tex_skybox_alpha(pt_scene *s, pt_id top, pt_id bottom, pt_id left, pt_id right, pt_id front, pt_id back)
{
    pt_id f[6] = {top, bottom, left, right, front, back};
    return tex_skybox(s, TexKind::SkyboxAlpha, f);
}

static pt_id tex_wrap(pt_scene *s, TexKind k, pt_id inner, const float *f, int nf)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        check_tex(sc, inner);
        TexRec t;
        t.kind = k;
        t.child = inner;
        for (int j = 0; j < nf; j++) t.f[j] = f[j];
        return add_tex(sc, t);
    });
}
pt_id pt_tex_multiply(pt_scene *s, float r, float g, float b, pt_id t)
{
    float f[3] = {r, g, b};
    return tex_wrap(s, TexKind::Multiply, t, f, 3);
}
pt_id pt_tex_log(pt_scene *s, pt_id t) { return tex_wrap(s, TexKind::Log, t, nullptr, 0); }
pt_id pt_tex_mirrorball(pt_scene *s, pt_id t) { return tex_wrap(s, TexKind::MirrorBall, t, nullptr, 0); }
pt_id pt_tex_spherical(pt_scene *s, pt_id t) { return tex_wrap(s, TexKind::Spherical, t, nullptr, 0); }
pt_id pt_tex_transformed(pt_scene *s, const float m[12], pt_id t)
{
    if (!m) {
        set_error("null matrix");
        return PT_ERR_ARG;
    }
    return tex_wrap(s, TexKind::Xform, t, m, 12);
}
pt_id pt_tex_coord(pt_scene *s)
{
    return guard([&] {
        TexRec t;
        t.kind = TexKind::Coord;
        return add_tex(S(s), t);
    });
}

/* A user-defined Texture subclass (include/texture.h:10-27: getColor, and
 * getFloat's default unless overridden) as device source, compiled into every
 * module of the scene that reaches it (codegen.cpp UTex_<id>). */
pt_id pt_tex_device(pt_scene *s, const char *color_body, const char *value_body, const float *params, int nparams)
{
    return guard([&] {
        if (!color_body || !*color_body)
            throw Error(PT_ERR_ARG, "pt_tex_device: empty getColor body");
        if (nparams < 0 || nparams > (1 << 16) || (nparams > 0 && !params))
            throw Error(PT_ERR_ARG, "pt_tex_device: bad parameter block");
        TexRec t;
        t.kind = TexKind::User;
        t.color_body = color_body;
        t.value_body = value_body ? value_body : "";
        t.params.assign(params, params + nparams);
        return add_tex(S(s), t);
    });
}

pt_id pt_material(pt_scene *s, pt_id reflect, pt_id scatter, pt_id emissive, pt_id transmit, float ior,
                  pt_id transmit_reflect)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        /* include/material.h:18 defaults: reflect 1, scatter 1, emissive 0, transmit 0, trc 0 */
        if (reflect < 0)
            reflect = default_tex(sc, 1);
        if (scatter < 0)
            scatter = default_tex(sc, 1);
        if (emissive < 0)
            emissive = default_tex(sc, 0);
        if (transmit < 0)
            transmit = default_tex(sc, 0);
        if (transmit_reflect < 0)
            transmit_reflect = default_tex(sc, 0);
        for (int t : {reflect, scatter, emissive, transmit, transmit_reflect}) check_tex(sc, t);
        MatRec m{reflect, scatter, emissive, transmit, transmit_reflect, ior};
        sc.materials.push_back(m);
        return (int)sc.materials.size() - 1;
    });
}

static pt_id leaf(pt_scene *s, ObjKind kind, float a, float b, float c, float d, pt_id mat)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        check_mat(sc, mat);
        ObjRec o;
        o.kind = kind;
        o.f[0] = a, o.f[1] = b, o.f[2] = c, o.f[3] = d;
        o.mat = mat;
        return push_object(sc, o);
    });
}
pt_id pt_sphere(pt_scene *s, float cx, float cy, float cz, float r, pt_id mat)
{
    return leaf(s, ObjKind::Sphere, cx, cy, cz, r, mat);
}
pt_id pt_plane(pt_scene *s, float nx, float ny, float nz, float d, pt_id mat)
{
    return leaf(s, ObjKind::Plane, nx, ny, nz, d, mat);
}

pt_id pt_plane_through(pt_scene *s, float nx, float ny, float nz, float px, float py, float pz, pt_id mat)
{
    /* Plane(normal, pos): d = -dot(normal, pos), src/plane.cpp:11-14 */
    float d = -((nx * px + ny * py) + nz * pz);
    return pt_plane(s, nx, ny, nz, d, mat);
}

pt_id pt_csg(pt_scene *s, int op, pt_id a, pt_id b)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        check_obj(sc, a);
        check_obj(sc, b);
        ObjRec o;
        if (op == PT_CSG_UNION)
            o.kind = ObjKind::Union;
        else if (op == PT_CSG_INTERSECTION)
            o.kind = ObjKind::Intersection;
        else if (op == PT_CSG_DIFFERENCE)
            o.kind = ObjKind::Difference;
        else
            throw Error(PT_ERR_ARG, "bad csg op");
        o.a = a, o.b = b;
        return push_object(sc, o);
    });
}

pt_id pt_transformed(pt_scene *s, const float m[12], pt_id child)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (!m)
            throw Error(PT_ERR_ARG, "null matrix");
        check_obj(sc, child);
        float inv[12];
        mat_inverse(m, inv); /* the reference inverts in the iterator ctor and throws there */
        ObjRec o;
        o.kind = ObjKind::Xform;
        memcpy(o.f, m, 48);
        o.a = child;
        return push_object(sc, o);
    });
}

/* A user-defined Object subclass (include/object.h:10-24: the virtual
 * makeSpanIterator) with one span per ray, as device source compiled into the
 * scene's modules (device/pt_user_object.h). */
pt_id pt_object_device(pt_scene *s, const char *span_body, const char *normal_body, const float *params,
                       int nparams, pt_id mat)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (!span_body || !*span_body || !normal_body || !*normal_body)
            throw Error(PT_ERR_ARG, "pt_object_device: empty span or normal body");
        if (nparams < 0 || nparams > (1 << 16) || (nparams > 0 && !params))
            throw Error(PT_ERR_ARG, "pt_object_device: bad parameter block");
        check_mat(sc, mat);
        ObjRec o;
        o.kind = ObjKind::User;
        o.mat = mat;
        o.span_body = span_body;
        o.normal_body = normal_body;
        o.params.assign(params, params + nparams);
        return push_object(sc, o);
    });
}

/* The same with a span list: up to max_spans ordered, strictly separated spans
 * per ray (include/object.h:14-20, include/span.h:129-171), one primitive slot
 * each (device/pt_user_object_n.h). */
pt_id pt_object_device_spans(pt_scene *s, const char *spans_body, const char *normal_body, const float *params,
                             int nparams, int max_spans, pt_id mat)
{
    return guard([&] {
        SceneImpl &sc = S(s);
        if (!spans_body || !*spans_body || !normal_body || !*normal_body)
            throw Error(PT_ERR_ARG, "pt_object_device_spans: empty spans or normal body");
        if (nparams < 0 || nparams > (1 << 16) || (nparams > 0 && !params))
            throw Error(PT_ERR_ARG, "pt_object_device_spans: bad parameter block");
        if (max_spans < 1 || max_spans > PT_OBJECT_MAX_SPANS)
            throw Error(PT_ERR_ARG, "pt_object_device_spans: max_spans outside 1.." +
                                        std::to_string(PT_OBJECT_MAX_SPANS));
        if (mat < 0 || mat >= (pt_id)sc.materials.size())
            throw Error(PT_ERR_ARG, "pt_object_device_spans: bad material id");
        ObjRec o;
        o.kind = ObjKind::User;
        o.mat = mat;
        o.span_body = spans_body;
        o.normal_body = normal_body;
        o.params.assign(params, params + nparams);
        o.max_spans = max_spans;
        return push_object(sc, o);
    });
}

int pt_set_root(pt_scene *s, pt_id obj)
{
    return set_knob(s, [&](SceneImpl &sc) {
        check_obj(sc, obj);
        sc.root = obj;
    });
}

int pt_scene_from_text(pt_scene *s, const char *text)
{
    return set_knob(s, [&](SceneImpl &sc) { load_text(sc, text ? text : ""); });
}

void pt_matrix_rotate(const float axis[3], double angle, float out[12]) { mat_rotate(axis, angle, out); }
int pt_matrix_inverse(const float m[12], float out[12])
{
    return guard([&] {
        mat_inverse(m, out);
        return PT_OK;
    });
}
void pt_matrix_concat(const float a[12], const float b[12], float out[12]) { mat_concat(a, b, out); }

int pt_scene_compile(pt_scene *s, int depth)
{
    return guard([&] {
        Generated g = generate(S(s), depth);
        code_object(g);
        S(s).last_key = g.key;
        return PT_OK;
    });
}

int pt_scene_set_occupancy(pt_scene *s, int workgroups_per_cu)
{
    return set_knob(s, [&](SceneImpl &sc) {
        if (workgroups_per_cu < 0 || workgroups_per_cu > 5)
            throw Error(PT_ERR_ARG, "workgroups_per_cu must be 0 (auto) or 1..5");
        sc.wg_per_cu = workgroups_per_cu;
    });
}

int pt_scene_set_fast_spine(pt_scene *s, int on)
{
    return set_knob(s, [&](SceneImpl &sc) { sc.fast_spine = on ? 1 : 0; });
}

int pt_scene_set_lane_walk(pt_scene *s, int frames)
{
    return set_knob(s, [&](SceneImpl &sc) {
        if (frames < 0 || frames > 8)
            throw Error(PT_ERR_ARG, "lane walk frames must be in [0, 8]");
        sc.lane_walk = frames;
    });
}

int pt_scene_set_split(pt_scene *s, int on)
{
    return set_knob(s, [&](SceneImpl &sc) { sc.split = on ? 1 : 0; });
}

int pt_scene_set_lane_scatter(pt_scene *s, int on)
{
    return set_knob(s, [&](SceneImpl &sc) { sc.lane_scatter = on ? 1 : 0; });
}

int pt_scene_set_lane_resume(pt_scene *s, int on)
{
    return set_knob(s, [&](SceneImpl &sc) { sc.lane_resume = on < 0 ? -1 : on ? 1 : 0; });
}

const char *pt_scene_module_key(pt_scene *s, int depth, int rays, int chain)
{
    thread_local std::string k;
    return key_text(k, [&] { return code_object_key(generate(S(s), depth, rays != 0, chain != 0)); });
}

const char *pt_scene_kernel_key(pt_scene *s, int depth) { return pt_scene_module_key(s, depth, 0, 0); }

int pt_scene_reach_facts(pt_scene *s, int *kr_reach, int *bursts_all_leaf)
{
    return guard([&] {
        const Generated g = generate(S(s), 1); /* the facts depend on the materials only */
        if (kr_reach)
            *kr_reach = g.kr_reach;
        if (bursts_all_leaf)
            *bursts_all_leaf = g.bursts_all_leaf ? 1 : 0;
        return PT_OK;
    });
}

int pt_write_hdr(const char *path, const float *rgb, int w, int h)
{
    return guard([&] {
        if (!path || !rgb || w <= 0 || h <= 0)
            throw Error(PT_ERR_ARG, "bad arguments");
        write_hdr(path, rgb, w, h);
        return PT_OK;
    });
}

int pt_write_bmp(const char *path, const float *rgb, int w, int h, int count)
{
    return guard([&] {
        if (!path || !rgb || w <= 0 || h <= 0 || count <= 0)
            throw Error(PT_ERR_ARG, "bad arguments");
        write_bmp(path, rgb, w, h, count);
        return PT_OK;
    });
}

} // extern "C"
