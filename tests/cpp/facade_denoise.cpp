// The denoiser through the C++ facade (include/pt/PathTrace.hpp) on scene P1, built as
// tests/cpp/facade_p1.cpp builds it:
//   facade_denoise W H CAP
// Renderer::denoise must return the bits of pt_denoise on the same planes -- with the error estimate and
// without it, with the variance and without demodulation --, and Renderer::renderDenoised the bits of
// renderConverged, renderGuides and denoise called one after the other.
// Prints "denoise ok <pixels> <changed>"; exit 10.. on a difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pt/PathTrace.hpp"

using namespace PathTrace;

static bool same(const void *a, const void *b, size_t n) { return memcmp(a, b, n) == 0; }

int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), cap = atoi(argv[3]);
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
        st.width = W, st.height = H, st.sampleCount = cap, st.rayDepth = 8;
        const size_t n = (size_t)W * H;
        std::vector<float> err;
        const std::vector<Color> rgb = renderer.renderConverged(st, 0.05f, 0, 64, nullptr, &err);
        Renderer::Settings gs = st;
        gs.sampleCount = 16;
        const Renderer::Guides g = renderer.renderGuides(gs);

        // the C call on the same planes
        pt_denoise_params p = {};
        p.width = W, p.height = H, p.iterations = 5, p.sigma_l = 2, p.sigma_z = 0.1f, p.normal_power_log2 = 5;
        p.demodulate = 1, p.device = 0;
        std::vector<float> want(3 * n), wvar(n);
        pt_denoise_buffers b = {};
        b.rgb = reinterpret_cast<const float *>(rgb.data()), b.err = err.data();
        b.normal = reinterpret_cast<const float *>(g.normal.data()), b.t = g.t.data(), b.material = g.material.data();
        b.albedo = reinterpret_cast<const float *>(g.albedo.data());
        b.emission = reinterpret_cast<const float *>(g.emission.data());
        b.out = want.data(), b.var_out = wvar.data();
        if (pt_denoise(&p, &b) != PT_OK)
            return 3;
        std::vector<float> var;
        const std::vector<Color> out = Renderer::denoise(W, H, rgb, g, &err, Renderer::DenoiseSettings(), &var);
        if (out.size() != n || var.size() != n)
            return 10;
        if (!same(out.data(), want.data(), 12 * n) || !same(var.data(), wvar.data(), 4 * n))
            return 11;
        size_t changed = 0;
        for (size_t k = 0; k < n; k++) changed += !same(&out[k], &rgb[k], 12);
        if (!changed)
            return 12;

        // no error estimate, no demodulation, other parameters
        Renderer::DenoiseSettings ds;
        ds.iterations = 2, ds.sigmaL = 4, ds.sigmaZ = 0.5f, ds.normalPowerLog2 = 3, ds.demodulate = false;
        p.iterations = 2, p.sigma_l = 4, p.sigma_z = 0.5f, p.normal_power_log2 = 3, p.demodulate = 0;
        b.err = nullptr, b.albedo = b.emission = nullptr, b.var_out = nullptr;
        if (pt_denoise(&p, &b) != PT_OK)
            return 4;
        const std::vector<Color> out2 = Renderer::denoise(W, H, rgb, g, nullptr, ds);
        if (out2.size() != n || !same(out2.data(), want.data(), 12 * n))
            return 13;
        if (same(out2.data(), out.data(), 12 * n))
            return 14;

        // the chain
        std::vector<Color> raw;
        std::vector<float> err2;
        const std::vector<Color> chained = renderer.renderDenoised(st, 0.05f, 16, Renderer::DenoiseSettings(), &raw,
                                                                   nullptr, &err2);
        if (raw.size() != n || !same(raw.data(), rgb.data(), 12 * n) || !same(err2.data(), err.data(), 4 * n))
            return 15;
        if (chained.size() != n || !same(chained.data(), out.data(), 12 * n))
            return 16;

        // a plane of the wrong size is refused before the C call
        std::vector<Color> shorter(rgb.begin(), rgb.end() - 1);
        try {
            Renderer::denoise(W, H, shorter, g);
            return 17;
        } catch (DeviceError &) {
        }
        printf("denoise ok %zu %zu\n", n, changed);
    } catch (std::exception &ex) {
        fprintf(stderr, "facade_denoise: %s\n", ex.what());
        return 1;
    }
    return 0;
}
