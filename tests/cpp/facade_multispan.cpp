// The multi-span user objects of tests/multispan.py built with the C++ facade
// include/pt/PathTrace.hpp: Object subclasses that override deviceSpans /
// deviceMaxSpans / deviceNormal (pt_object_device_spans) -- a hollow shell, a
// dumbbell and a shell around a ball -- put together into multi_zoo as the
// Python mirror builds it, then
//   facade_multispan key DEPTH                 -> prints the scene's code-object key (no GPU)
//   facade_multispan render W H SPP DEPTH OUT  -> renders on device 0, writes W*H*3 f32 to OUT
// The body text is tests/multispan.py's, character for character: the two
// scenes generate the same device module, which the key comparison checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pt/PathTrace.hpp"

using namespace PathTrace;

/* Difference(Sphere(c, R), Sphere(c, r)) as one object: up to two spans,
 * [outer.t0, inner.t0] and [inner.t1, outer.t1] (src/difference.cpp:84-135),
 * each sphere by src/sphere.cpp:31-49.  prm: c, R*R, r*r, R, r. */
class Shell : public Object
{
public:
    Shell(Vector3D c, float R, float r, const Material *m) : c_(c), R_(R), r_(r), m_(m) {}
    Object *duplicate() const override { return new Shell(c_, R_, r_, m_); }
    const char *deviceSpans() const override
    {
        return R"PT(
    const V3 oc = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float a = dot(d, d);
    const float b = dot(oc, d);
    const float cc = dot(oc, oc);
    const float disco = b * b - a * (cc - prm[3]);
    if (disco <= 1e-3f)
        return 0;
    const float so = sqrtf(disco);
    const float o0 = (-b - so) / a, o1 = (-b + so) / a;
    const float disci = b * b - a * (cc - prm[4]);
    if (disci <= 1e-3f) {
        t0[0] = o0, t1[0] = o1;
        return 1;
    }
    const float si = sqrtf(disci);
    t0[0] = o0, t1[0] = (-b - si) / a;
    t0[1] = (-b + si) / a, t1[1] = o1;
    return 2;
)PT";
    }
    int deviceMaxSpans() const override { return 2; }
    /* V3 normal(V3 p, int k): q / |q| on the outer surface, its negation on the inner one */
    const char *deviceNormal() const override
    {
        return R"PT(
    const V3 q = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    float m = sqrtf(dot(q, q));
    const float eo = m > prm[5] ? m - prm[5] : prm[5] - m;
    const float ei = m > prm[6] ? m - prm[6] : prm[6] - m;
    if (m == 0.0f)
        m = 1.0f;
    const V3 n = mk(q.x / m, q.y / m, q.z / m);
    return ei < eo ? mk(-n.x, -n.y, -n.z) : n;
)PT";
    }
    std::vector<float> deviceParams() const override { return {c_.x, c_.y, c_.z, R_ * R_, r_ * r_, R_, r_}; }
    const Material *deviceMaterial() const override { return m_; }

private:
    Vector3D c_;
    float R_, r_;
    const Material *m_;
};

/* Union(Sphere(a, ra), Sphere(b, rb)) of two disjoint balls as one object: the
 * two spans in ray order by the union's own test a.t1 < b.t0 (src/union.cpp).
 * prm: a, ra*ra, b, rb*rb, ra, rb. */
class Dumbbell : public Object
{
public:
    Dumbbell(Vector3D a, float ra, Vector3D b, float rb, const Material *m) : a_(a), b_(b), ra_(ra), rb_(rb), m_(m) {}
    Object *duplicate() const override { return new Dumbbell(a_, ra_, b_, rb_, m_); }
    const char *deviceSpans() const override
    {
        return R"PT(
    const float a = dot(d, d);
    const V3 pa = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float ba = dot(pa, d);
    const float da = ba * ba - a * (dot(pa, pa) - prm[3]);
    const V3 pb = mk(o.x - prm[4], o.y - prm[5], o.z - prm[6]);
    const float bb = dot(pb, d);
    const float db = bb * bb - a * (dot(pb, pb) - prm[7]);
    const bool la = !(da <= 1e-3f), lb = !(db <= 1e-3f);
    float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
    if (la) {
        const float s = sqrtf(da);
        a0 = (-ba - s) / a, a1 = (-ba + s) / a;
    }
    if (lb) {
        const float s = sqrtf(db);
        b0 = (-bb - s) / a, b1 = (-bb + s) / a;
    }
    if (la && lb) {
        const bool af = a1 < b0;
        t0[0] = af ? a0 : b0, t1[0] = af ? a1 : b1;
        t0[1] = af ? b0 : a0, t1[1] = af ? b1 : a1;
        return 2;
    }
    if (la) {
        t0[0] = a0, t1[0] = a1;
        return 1;
    }
    if (lb) {
        t0[0] = b0, t1[0] = b1;
        return 1;
    }
    return 0;
)PT";
    }
    int deviceMaxSpans() const override { return 2; }
    const char *deviceNormal() const override
    {
        return R"PT(
    const V3 qa = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    const V3 qb = mk(p.x - prm[4], p.y - prm[5], p.z - prm[6]);
    const float ma = sqrtf(dot(qa, qa)), mb = sqrtf(dot(qb, qb));
    const float ea = ma > prm[8] ? ma - prm[8] : prm[8] - ma;
    const float eb = mb > prm[9] ? mb - prm[9] : prm[9] - mb;
    const V3 q = eb < ea ? qb : qa;
    float m = eb < ea ? mb : ma;
    if (m == 0.0f)
        m = 1.0f;
    return mk(q.x / m, q.y / m, q.z / m);
)PT";
    }
    std::vector<float> deviceParams() const override
    {
        return {a_.x, a_.y, a_.z, ra_ * ra_, b_.x, b_.y, b_.z, rb_ * rb_, ra_, rb_};
    }
    const Material *deviceMaterial() const override { return m_; }

private:
    Vector3D a_, b_;
    float ra_, rb_;
    const Material *m_;
};

/* Difference(Sphere(c, R1), Difference(Sphere(c, R2), Sphere(c, R3))), a shell
 * around a ball, as one object of up to three spans.
 * prm: c, R1*R1, R2*R2, R3*R3, R1, R2, R3. */
class Onion : public Object
{
public:
    Onion(Vector3D c, float r1, float r2, float r3, const Material *m) : c_(c), r1_(r1), r2_(r2), r3_(r3), m_(m) {}
    Object *duplicate() const override { return new Onion(c_, r1_, r2_, r3_, m_); }
    const char *deviceSpans() const override
    {
        return R"PT(
    const V3 oc = mk(o.x - prm[0], o.y - prm[1], o.z - prm[2]);
    const float a = dot(d, d);
    const float b = dot(oc, d);
    const float cc = dot(oc, oc);
    const float d1 = b * b - a * (cc - prm[3]);
    if (d1 <= 1e-3f)
        return 0;
    const float s1 = sqrtf(d1);
    const float o0 = (-b - s1) / a, o1 = (-b + s1) / a;
    const float d2 = b * b - a * (cc - prm[4]);
    if (d2 <= 1e-3f) {
        t0[0] = o0, t1[0] = o1;
        return 1;
    }
    const float s2 = sqrtf(d2);
    const float m0 = (-b - s2) / a, m1 = (-b + s2) / a;
    const float d3 = b * b - a * (cc - prm[5]);
    if (d3 <= 1e-3f) {
        t0[0] = o0, t1[0] = m0;
        t0[1] = m1, t1[1] = o1;
        return 2;
    }
    const float s3 = sqrtf(d3);
    t0[0] = o0, t1[0] = m0;
    t0[1] = (-b - s3) / a, t1[1] = (-b + s3) / a;
    t0[2] = m1, t1[2] = o1;
    return 3;
)PT";
    }
    int deviceMaxSpans() const override { return 3; }
    const char *deviceNormal() const override
    {
        return R"PT(
    const V3 q = mk(p.x - prm[0], p.y - prm[1], p.z - prm[2]);
    float m = sqrtf(dot(q, q));
    const float e1 = m > prm[6] ? m - prm[6] : prm[6] - m;
    const float e2 = m > prm[7] ? m - prm[7] : prm[7] - m;
    const float e3 = m > prm[8] ? m - prm[8] : prm[8] - m;
    if (m == 0.0f)
        m = 1.0f;
    const V3 n = mk(q.x / m, q.y / m, q.z / m);
    return e2 < e1 && e2 < e3 ? mk(-n.x, -n.y, -n.z) : n;
)PT";
    }
    std::vector<float> deviceParams() const override
    {
        return {c_.x, c_.y, c_.z, r1_ * r1_, r2_ * r2_, r3_ * r3_, r1_, r2_, r3_};
    }
    const Material *deviceMaterial() const override { return m_; }

private:
    Vector3D c_;
    float r1_, r2_, r3_;
    const Material *m_;
};

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    Material diffuse(new ColorTexture(0.8f), new ColorTexture(1));
    Material mirror(new ColorTexture(0.99f), new ColorTexture(0));
    Material glass(new ColorTexture(0.7f), new ColorTexture(0), new ColorTexture(0), new ColorTexture(0.9f), 1.3f,
                   new ColorTexture(1));
    Material emitW(new ColorTexture(0), new ColorTexture(0), new ColorTexture(2));
    /* tests/multispan.py multi_zoo(user=True) */
    Object *shells = new Union(new Shell(Vector3D(0.9f, 0.1f, -3.2f), 0.5f, 0.3f, &glass),
                               new Shell(Vector3D(-1.0f, 0.05f, -3.4f), 0.5f, 0.3f, &diffuse));
    const Matrix rot = Matrix::rotateY(0.5).concat(Matrix::rotateX(0.2)).concat(Matrix::translate(-0.2f, 0.9f, -4.5f));
    Object *carved = new Difference(
        new TransformedObject(rot, new Dumbbell(Vector3D(-0.35f, 0, 0), 0.25f, Vector3D(0.35f, 0, 0), 0.25f, &diffuse)),
        new Sphere(Vector3D(-0.2f, 1.15f, -4.4f), 0.4f, &mirror));
    Object *dented = new Difference(
        new Sphere(Vector3D(0.0f, -0.1f, -5.5f), 0.7f, &diffuse),
        new Dumbbell(Vector3D(-0.3f, -0.1f, -5.0f), 0.25f, Vector3D(0.3f, -0.1f, -5.0f), 0.25f, &mirror));
    Object *capped = new Intersection(
        new Dumbbell(Vector3D(-1.9f, 0.6f, -4.5f), 0.25f, Vector3D(-1.3f, 0.6f, -4.5f), 0.25f, &diffuse),
        new Plane(Vector3D(0, 1, 0), -0.6f, &diffuse));
    Object *layers = new Onion(Vector3D(1.6f, 0.3f, -4.8f), 0.5f, 0.38f, 0.2f, &glass);
    std::unique_ptr<Object> world(new Union(new Union(shells, new Union(carved, dented)),
                                            new Union(new Union(capped, layers),
                                                      new Plane(Vector3D(0, 1, 0), 0.5f, &emitW))));
    try {
        Renderer renderer(world.get());
        if (!strcmp(argv[1], "key") && argc == 3) {
            printf("%s\n", pt_scene_kernel_key(renderer.handle(), atoi(argv[2])));
            return 0;
        }
        if (!strcmp(argv[1], "render") && argc == 7) {
            Renderer::Settings st;
            st.width = atoi(argv[2]), st.height = atoi(argv[3]);
            st.sampleCount = atoi(argv[4]), st.rayDepth = atoi(argv[5]);
            std::vector<Color> img = renderer.render(st);
            FILE *f = fopen(argv[6], "wb");
            if (!f)
                return 5;
            fwrite(img.data(), sizeof(Color), img.size(), f);
            fclose(f);
            return 0;
        }
    } catch (std::exception &e) {
        fprintf(stderr, "facade_multispan: %s\n", e.what());
        return 1;
    }
    return 2;
}
