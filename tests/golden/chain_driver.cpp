/*
 * chain_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/golden/make_chain_golden.py).
 *
 * Drives the UNMODIFIED reference's tracePixel<T> / traceRay<T> templates
 * (reference include/path-trace.h:58-165, :187-201) the way a program that owns
 * one DefaultRandomEngine does: one engine threaded through every sample of
 * every pixel of a chain.  T is a counting wrapper that steps
 * DefaultRandomEngine's recurrence (include/pt/pt_engine.h) from a given 64-bit
 * state, so that each entry's colour, the engine state after it and the number
 * of draws so far can be frozen into tests/golden/chain_*.npz.
 *
 * It contains no reference code.  Scenes are built by oracle/ref_driver.cpp's
 * build_world, included here as a translation unit with its main renamed, and
 * the program links the reference objects `make -C oracle ref` leaves in
 * oracle/_ref/.  The binary goes to oracle/_ref/ only.
 *
 *   chain_driver pixels scene.txt W H spp depth sw sh dist pixels.bin begin.bin states.bin out.bin
 *   chain_driver rays   scene.txt spp depth rays.bin begin.bin states.bin out.bin
 *
 * pixels.bin: int32 pixel indices (py * W + px); rays.bin: 7 float32 per ray;
 * begin.bin: nchains + 1 int64 offsets; states.bin: nchains uint64.
 * out.bin: float32 colour[3n], uint64 state_after[n], uint64 draws[n] (since
 * the chain's start), uint64 final_state[nchains].
 *
 * The reference asserts count <= 1000 in its rejection loop (path-trace.h:148):
 * a fixture sample that reaches the cap aborts this program.
 */
#define main ptref_main
#include "../../oracle/ref_driver.cpp"
#undef main

namespace
{

struct CountingEngine
{
    PtSampleEngine e; /* state = DefaultRandomEngine's v, inc = its increment */
    unsigned long long draws;
    explicit CountingEngine(uint64_t v) : draws(0)
    {
        e.state = v;
        e.inc = PT_LCG_INC;
    }
    static unsigned min() { return 0; }
    static unsigned max() { return 0xFFFFFFFFu; }
    unsigned operator()()
    {
        draws++;
        return e();
    }
};

template <class T>
std::vector<T> read_array(const char *path)
{
    std::vector<char> raw = read_file(path);
    return std::vector<T>((const T *)raw.data(), (const T *)raw.data() + raw.size() / sizeof(T));
}

struct Out
{
    std::vector<float> colour;
    std::vector<uint64_t> state, draws, final_state;
    void entry(const Color &c, const CountingEngine &g)
    {
        colour.push_back(c.x), colour.push_back(c.y), colour.push_back(c.z);
        state.push_back(g.e.state);
        draws.push_back(g.draws);
    }
    void write(const char *path) const
    {
        std::vector<char> b;
        auto put = [&](const void *p, size_t n) { b.insert(b.end(), (const char *)p, (const char *)p + n); };
        put(colour.data(), colour.size() * 4);
        put(state.data(), state.size() * 8);
        put(draws.data(), draws.size() * 8);
        put(final_state.data(), final_state.size() * 8);
        write_file(path, b.data(), b.size());
    }
};

World load_world(const char *path)
{
    std::vector<char> txt = read_file(path);
    scenetext::Desc d = scenetext::parse(std::string(txt.data(), txt.size()));
    World w;
    build_world(d, w);
    return w;
}

int mode_pixels(char **a)
{
    World w = load_world(a[2]);
    const int W = atoi(a[3]), H = atoi(a[4]), spp = atoi(a[5]), depth = atoi(a[6]);
    const float sw = scenetext::parse_float(a[7]), sh = scenetext::parse_float(a[8]), dist = scenetext::parse_float(a[9]);
    const std::vector<int32_t> pix = read_array<int32_t>(a[10]);
    const std::vector<int64_t> begin = read_array<int64_t>(a[11]);
    const std::vector<uint64_t> states = read_array<uint64_t>(a[12]);
    std::unique_ptr<SpanIterator> it(w.root->makeSpanIterator());
    Out o;
    for (size_t c = 0; c < states.size(); c++) {
        CountingEngine g(states[c]);
        for (int64_t k = begin[c]; k < begin[c + 1]; k++)
            o.entry(tracePixel(*it, pix[k] % W, pix[k] / W, W, H, spp, depth, sw, sh, dist, g), g);
        o.final_state.push_back(g.e.state);
    }
    o.write(a[13]);
    return 0;
}

int mode_ray_chains(char **a)
{
    World w = load_world(a[2]);
    const int spp = atoi(a[3]), depth = atoi(a[4]);
    const std::vector<float> r = read_array<float>(a[5]);
    const std::vector<int64_t> begin = read_array<int64_t>(a[6]);
    const std::vector<uint64_t> states = read_array<uint64_t>(a[7]);
    std::unique_ptr<SpanIterator> it(w.root->makeSpanIterator());
    Out o;
    for (size_t c = 0; c < states.size(); c++) {
        CountingEngine g(states[c]);
        for (int64_t k = begin[c]; k < begin[c + 1]; k++) {
            const float *q = &r[7 * k];
            const Ray ray(Vector3D(q[0], q[1], q[2]), Vector3D(q[3], q[4], q[5]));
            /* the sample loop of tracePixel's float-coordinate overload (path-trace.h:178-183) */
            Color acc(0, 0, 0);
            for (int s = 0; s < spp; s++) acc += traceRay(ray, *it, depth, g, q[6]);
            acc /= spp;
            o.entry(acc, g);
        }
        o.final_state.push_back(g.e.state);
    }
    o.write(a[8]);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    try {
        if (argc == 14 && std::string(argv[1]) == "pixels")
            return mode_pixels(argv);
        if (argc == 9 && std::string(argv[1]) == "rays")
            return mode_ray_chains(argv);
        fprintf(stderr, "chain_driver: bad arguments\n");
        return 2;
    } catch (std::exception &e) {
        fprintf(stderr, "chain_driver error: %s\n", e.what());
        return 1;
    }
}
