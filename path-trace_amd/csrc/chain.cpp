/*
 * chain.cpp -- the part of pt_trace_chains (include/pt/pt.h) that needs no
 * device: the argument check and the step schedule.  A chain is a list of
 * entries (pixels or rays) traced one after another on ONE
 * DefaultRandomEngine, every sample starting where the one before left the
 * engine (reference include/path-trace.h:187-201 called pixel after pixel with
 * the caller's engine).  That dependence lives here, on the host: the runtime
 * launches the chained module once per step, and step t traces sample
 * t % spp of entry t / spp of every chain that has one.  Also the ray check
 * every entry taking caller rays shares (check_rays).  No HIP in this file:
 * tests/cpp/chain_schedule_main.cpp builds it alone under the sanitizers.
 */
#include <algorithm>
#include <cmath>
#include <numeric>

#include "internal.h"

namespace pt
{

void chain_schedule(const int64_t *begin, int64_t nchains, int spp, std::vector<int32_t> &order,
                    std::vector<int64_t> &items)
{
    auto len = [&](int32_t c) { return begin[c + 1] - begin[c]; };
    order.resize((size_t)nchains);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len(a) > len(b); });
    const int64_t longest = nchains > 0 ? len(order[0]) : 0;
    items.assign((size_t)(longest * spp), 0);
    int64_t k = nchains; /* chains with more than e entries: order[0 .. k) */
    for (int64_t e = 0; e < longest; e++) {
        while (k > 0 && len(order[(size_t)k - 1]) <= e) k--;
        std::fill_n(items.begin() + e * spp, spp, k);
    }
}

void chain_validate(const pt_chain_params *p, const int32_t *pixels, const float *rays, const int64_t *begin,
                    int64_t nchains, const uint64_t *states, const float *rgb_out)
{
    if (!p)
        throw Error(PT_ERR_ARG, "null params");
    if ((pixels != nullptr) == (rays != nullptr))
        throw Error(PT_ERR_ARG, "exactly one of pixels and rays must be given");
    if (p->spp < 1 || p->spp >= (1 << 20))
        throw Error(PT_ERR_ARG, "spp must be in [1, 2^20)");
    if (p->depth < 0 || p->depth > 64)
        throw Error(PT_ERR_ARG, "depth must be in [0, 64]");
    if (nchains < 0 || nchains >= (1ll << 31))
        throw Error(PT_ERR_ARG, "nchains must be in [0, 2^31)");
    if (!begin)
        throw Error(PT_ERR_ARG, "null begin");
    if (begin[0] != 0)
        throw Error(PT_ERR_ARG, "begin[0] must be 0");
    for (int64_t c = 0; c < nchains; c++)
        if (begin[c + 1] < begin[c])
            throw Error(PT_ERR_ARG, "begin decreases at chain " + std::to_string(c));
    const int64_t n = begin[nchains];
    if (n >= (1ll << 31))
        throw Error(PT_ERR_ARG, "begin: entry count must be below 2^31");
    int64_t longest = 0;
    for (int64_t c = 0; c < nchains; c++) longest = std::max(longest, begin[c + 1] - begin[c]);
    if (longest * p->spp >= (1ll << 31))
        throw Error(PT_ERR_ARG, "begin: a chain's entries x spp must be below 2^31 steps");
    if (nchains > 0 && !states)
        throw Error(PT_ERR_ARG, "null states");
    if (n > 0 && !rgb_out)
        throw Error(PT_ERR_ARG, "null rgb_out");
    if (pixels) {
        if (p->width <= 0 || p->height <= 0 || (int64_t)p->width * p->height >= (1ll << 31))
            throw Error(PT_ERR_ARG, "width and height must be positive, width x height below 2^31");
        const int64_t limit = (int64_t)p->width * p->height;
        for (int64_t k = 0; k < n; k++)
            if (pixels[k] < 0 || pixels[k] >= limit)
                throw Error(PT_ERR_ARG, "pixels[" + std::to_string(k) + "] lies outside width x height");
    } else {
        check_rays(rays, n, 7, "rays[");
    }
}

void check_rays(const float *rays, int64_t n, int stride, const std::string &prefix)
{
    const char *close = !prefix.empty() && prefix.back() == '[' ? "]" : "";
    for (int64_t k = 0; k < n; k++) {
        const float *r = rays + stride * k;
        /* Ray(o, d) asserts d != 0 (include/ray.h:17) */
        if (r[3] == 0.0f && r[4] == 0.0f && r[5] == 0.0f)
            throw Error(PT_ERR_ARG, prefix + std::to_string(k) + close + " has a zero direction");
        /* The kernel's axis-aligned plane forms take d.n as the one product
         * that survives for finite operands (the other terms are +-0); an
         * infinite or NaN component would make the reference's full dot
         * product NaN where the device has a number, so such rays are
         * refused rather than traced differently. */
        for (int c = 0; c < 6; c++)
            if (!std::isfinite(r[c]))
                throw Error(PT_ERR_ARG, prefix + std::to_string(k) + close + " has a non-finite origin or direction");
    }
}

} // namespace pt
