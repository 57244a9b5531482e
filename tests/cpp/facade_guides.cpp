// Guide buffers and first-hit queries through the C++ facade (include/pt/PathTrace.hpp) on scene
// P1, built as tests/cpp/facade_p1.cpp builds it:
//   facade_guides W H SPP
// Renderer::renderGuides must return the bits of pt_render_guides on the renderer's scene, and
// firstHits (both paths) the bits of pt_query_hits for camera-like rays through the frame's pixel
// centres.  Prints "guides ok <entries> hits ok <rays> <hits>"; exit 10.. on a difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "pt/PathTrace.hpp"

using namespace PathTrace;

static bool same(const void *a, const void *b, size_t n) { return memcmp(a, b, n) == 0; }

int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), spp = atoi(argv[3]);
    Material diffuse(new ColorTexture(0.8f), new ColorTexture(1));
    Material mirror(new ColorTexture(0.99f), new ColorTexture(0));
    Material glass(new ColorTexture(0.7f), new ColorTexture(0), new ColorTexture(0), new ColorTexture(0.9f), 1.3f,
                   new ColorTexture(1));
    Material sky(new ColorTexture(0), new ColorTexture(0), new ColorTexture(0.5f, 0.7f, 1.0f));
    Object *left = new Difference(new Union(new Sphere(Vector3D(-1, 0, -4), .6f, &diffuse),
                                            new Sphere(Vector3D(-.5f, 0, -4), .6f, &diffuse)),
                                  new Sphere(Vector3D(-.7f, .3f, -3.6f), .4f, &diffuse));
    Object *right = new Difference(new Union(new Sphere(Vector3D(1, 0, -4), .6f, &glass),
                                             new Sphere(Vector3D(1.4f, .2f, -4.2f), .5f, &mirror)),
                                   new Sphere(Vector3D(1, 0, -3.4f), .3f, &glass));
    std::unique_ptr<Object> world(new Union(left, new Union(right, new Plane(Vector3D(0, 0, 1), 200, &sky))));
    try {
        Renderer renderer(world.get());
        Renderer::Settings st;
        st.width = W, st.height = H, st.sampleCount = spp;
        const Renderer::Guides g = renderer.renderGuides(st);
        const size_t n = (size_t)W * H;
        std::vector<float> em(3 * n), al(3 * n), nr(3 * n), t(n), cov(n);
        std::vector<int32_t> mat(n);
        pt_guide_buffers b = {em.data(), al.data(), nr.data(), t.data(), cov.data(), mat.data()};
        pt_render_params p = Renderer::params(st, nullptr, 0);
        if (pt_render_guides(renderer.handle(), &p, &b) != PT_OK)
            return 3;
        if (g.emission.size() != n || g.albedo.size() != n || g.normal.size() != n || g.t.size() != n ||
            g.coverage.size() != n || g.material.size() != n)
            return 10;
        if (!same(g.emission.data(), em.data(), 12 * n) || !same(g.albedo.data(), al.data(), 12 * n) ||
            !same(g.normal.data(), nr.data(), 12 * n))
            return 11;
        if (!same(g.t.data(), t.data(), 4 * n) || !same(g.coverage.data(), cov.data(), 4 * n) ||
            !same(g.material.data(), mat.data(), 4 * n))
            return 12;
        // a pixel list: compact, the frame's entries
        const int32_t list[3] = {W + 1, 0, W + 1};
        const Renderer::Guides gl = renderer.renderGuides(st, list, 3);
        for (int k = 0; k < 3; k++)
            if (!same(&gl.emission[k], &g.emission[list[k]], 12) || !same(&gl.normal[k], &g.normal[list[k]], 12) ||
                gl.material[k] != g.material[list[k]] || !same(&gl.t[k], &g.t[list[k]], 4))
                return 13;

        // firstHits: rays from the origin through the pixel centres, and back out of the scene from behind
        std::vector<Ray> rays;
        std::vector<float> flat;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const Vector3D d(2.0f * (x + 0.5f) / W - 1.0f, 1.0f - 2.0f * (y + 0.5f) / H, -1.5f);
                rays.push_back(Ray(Vector3D(0, 0, 0), d));
                rays.push_back(Ray(Vector3D(-1, 0, -4), d)); // from inside a sphere: exits
            }
        for (const Ray &r : rays) {
            const float f[6] = {r.origin.x, r.origin.y, r.origin.z, r.dir.x, r.dir.y, r.dir.z};
            flat.insert(flat.end(), f, f + 6);
        }
        size_t hits = 0, exits = 0;
        for (int path : {PT_HIT_FAST, PT_HIT_MERGE}) {
            const std::vector<FirstHit> fh = firstHits(*world, rays, path);
            std::vector<pt_hit> want(rays.size());
            if (pt_query_hits(renderer.handle(), flat.data(), (int64_t)rays.size(), path, want.data(), nullptr,
                              nullptr, 0) != PT_OK)
                return 4;
            if (fh.size() != rays.size())
                return 14;
            std::map<int32_t, const Material *> ids; // one Material per material id
            for (size_t k = 0; k < fh.size(); k++) {
                const FirstHit &a = fh[k];
                const pt_hit &w = want[k];
                if (a.hit != (w.hit != 0) || a.exit != (w.exit != 0) || !same(&a.t, &w.t, 4) ||
                    !same(&a.normal, w.normal, 12) || !same(&a.pos, w.pos, 12) || !same(&a.ior, &w.ior, 4))
                    return 15;
                if (!a.hit) {
                    if (a.material || w.material != -1)
                        return 16;
                    continue;
                }
                if (a.material != &diffuse && a.material != &mirror && a.material != &glass && a.material != &sky)
                    return 17;
                if (!ids.count(w.material))
                    ids[w.material] = a.material;
                if (ids[w.material] != a.material || a.ior != a.material->ior)
                    return 18;
                hits++, exits += a.exit;
            }
        }
        if (!exits)
            return 19;
        printf("guides ok %zu hits ok %zu %zu %zu\n", n, rays.size(), hits, exits);
    } catch (std::exception &ex) {
        fprintf(stderr, "facade_guides: %s\n", ex.what());
        return 1;
    }
    return 0;
}
