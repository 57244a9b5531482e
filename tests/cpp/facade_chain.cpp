// The reference's one-engine mode through the C++ facade (include/pt/PathTrace.hpp):
// a program that owns ONE DefaultRandomEngine and calls tracePixel with it pixel
// after pixel, on scene P1 built as tests/cpp/facade_p1.cpp builds it.
//   facade_chain W H SPP DEPTH SW SH DIST SEED PIXELS
// PIXELS: int32 pixel indices (py * W + px).  Prints, as integers,
//   P r g b state   per pixel: tracePixel(..., engine)'s colour bits and engine.state() after it
//   C r g b         per pixel: the same chain through one tracePixelsChained call (a fresh engine)
//   E state         that engine's state after the call
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pt/PathTrace.hpp"

using namespace PathTrace;

static unsigned bits(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 10)
        return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), spp = atoi(argv[3]), depth = atoi(argv[4]);
    const float sw = strtof(argv[5], nullptr), sh = strtof(argv[6], nullptr), dist = strtof(argv[7], nullptr);
    const unsigned seed = (unsigned)strtoul(argv[8], nullptr, 10);
    std::vector<int> px, py;
    {
        FILE *f = fopen(argv[9], "rb");
        if (!f)
            return 3;
        int32_t p;
        while (fread(&p, 4, 1, f) == 1) px.push_back(p % W), py.push_back(p / W);
        fclose(f);
    }
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
        std::unique_ptr<SpanIterator> it(world->makeSpanIterator());
        DefaultRandomEngine e;
        e.seed(seed);
        for (size_t k = 0; k < px.size(); k++) {
            const Color c = tracePixel(*it, px[k], py[k], W, H, spp, depth, sw, sh, dist, e);
            printf("P %u %u %u %" PRIu64 "\n", bits(c.x), bits(c.y), bits(c.z), (uint64_t)e.state());
        }
        DefaultRandomEngine g;
        g.seed(seed);
        std::vector<Color> out(px.size());
        tracePixelsChained(*it, px.data(), py.data(), px.size(), W, H, spp, depth, sw, sh, dist, g, out.data());
        for (const Color &c : out) printf("C %u %u %u\n", bits(c.x), bits(c.y), bits(c.z));
        printf("E %" PRIu64 "\n", (uint64_t)g.state());
    } catch (std::exception &ex) {
        fprintf(stderr, "facade_chain: %s\n", ex.what());
        return 1;
    }
    return 0;
}
