// pt_trace_chains' host side under the sanitizers: a stand-alone program over
// path-trace_amd/csrc/chain.cpp (no HIP, no libpt.so).
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/cpp/chain_schedule_main.cpp path-trace_amd/csrc/chain.cpp -o chain_schedule && ./chain_schedule
// chain_schedule on the fixtures' chain lengths and on degenerate ones (no
// chains, all empty, one chain, equal lengths), checked against the definition:
// step t runs exactly the chains with more than t steps, as a prefix of `order`.
// chain_validate on one good and several bad argument sets.  check_rays, the
// ray check pt_trace_rays, pt_trace_chains and pt_query_hits share, on each
// caller's stride and message prefix.
#include <cstdio>
#include <string>
#include <vector>

#include "../../path-trace_amd/csrc/internal.h"

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            failures++;                                         \
        }                                                       \
    } while (0)

static void schedule_case(const std::vector<int64_t> &len, int spp)
{
    std::vector<int64_t> begin(1, 0);
    for (int64_t l : len) begin.push_back(begin.back() + l);
    std::vector<int32_t> order;
    std::vector<int64_t> items;
    pt::chain_schedule(begin.data(), (int64_t)len.size(), spp, order, items);
    int64_t longest = 0, total = 0, sum = 0;
    for (int64_t l : len) longest = l > longest ? l : longest, total += l * spp;
    CHECK(order.size() == len.size());
    CHECK((int64_t)items.size() == longest * spp);
    std::vector<int> seen(len.size(), 0);
    for (int32_t c : order) {
        CHECK(c >= 0 && (size_t)c < len.size());
        if (c >= 0 && (size_t)c < len.size())
            seen[(size_t)c]++;
    }
    for (int s : seen) CHECK(s == 1);
    for (size_t t = 0; t < items.size(); t++) {
        int64_t want = 0;
        for (int64_t l : len) want += l * spp > (int64_t)t;
        CHECK(items[t] == want);
        CHECK(items[t] >= 1 && items[t] <= (int64_t)len.size());
        for (int64_t k = 0; k < (int64_t)order.size(); k++)
            CHECK((len[(size_t)order[(size_t)k]] * spp > (int64_t)t) == (k < items[t]));
        sum += items[t];
    }
    CHECK(sum == total);
}

template <class F>
static bool refused(F f)
{
    try {
        f();
    } catch (pt::Error &e) {
        return e.code == PT_ERR_ARG;
    }
    return false;
}

/* what check_rays says of ray 1 of three rays of `stride` floats, the others valid ("" = accepted) */
static std::string ray_message(int stride, const std::string &prefix, int component, float value, bool zero_dir)
{
    const float inf = __builtin_inff();
    /* the seventh float of a ray is its strength, which the check must not read as a direction:
     * make it what would be refused there */
    std::vector<float> r((size_t)stride * 3, stride == 7 ? inf : 0.0f);
    for (int k = 0; k < 3; k++) {
        float *q = &r[(size_t)stride * k];
        q[0] = 1, q[1] = 2, q[2] = 3, q[3] = 0, q[4] = -0.0f, q[5] = -1;
    }
    if (zero_dir)
        r[(size_t)stride + 5] = 0.0f;
    if (component >= 0)
        r[(size_t)stride + component] = value;
    try {
        pt::check_rays(r.data(), 3, stride, prefix);
    } catch (pt::Error &e) {
        CHECK(e.code == PT_ERR_ARG);
        return e.what();
    }
    return "";
}

static void ray_check_cases()
{
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    const struct
    {
        int stride;
        const char *prefix, *name;
    } callers[] = {{7, "ray ", "ray 1"}, {7, "rays[", "rays[1]"}, {6, "pt_query_hits: rays[", "pt_query_hits: rays[1]"}};
    for (const auto &c : callers) {
        const std::string name = c.name;
        CHECK(ray_message(c.stride, c.prefix, -1, 0, false) == "");
        CHECK(ray_message(c.stride, c.prefix, -1, 0, true) == name + " has a zero direction");
        CHECK(ray_message(c.stride, c.prefix, 1, nan, false) == name + " has a non-finite origin or direction");
        CHECK(ray_message(c.stride, c.prefix, 4, inf, false) == name + " has a non-finite origin or direction");
        CHECK(ray_message(c.stride, c.prefix, 3, -inf, false) == name + " has a non-finite origin or direction");
        pt::check_rays(nullptr, 0, c.stride, c.prefix); /* n = 0 reads nothing */
    }
}

int main()
{
    for (int spp : {1, 2, 3, 5}) {
        schedule_case({36}, spp);                     /* mixed, rays1 */
        schedule_case({0, 1, 2, 7, 17, 1}, spp);      /* uneven1, uneven5 */
        schedule_case(std::vector<int64_t>(300, 2), spp); /* many */
        schedule_case({8, 8, 8, 8}, spp);             /* csg */
        schedule_case(std::vector<int64_t>(8, 6), spp);   /* rays8 */
        schedule_case({}, spp);
        schedule_case({0, 0, 0}, spp);
        schedule_case({1}, spp);
        schedule_case({0}, spp);
        schedule_case({3, 0, 3, 0, 3}, spp);
        schedule_case({1, 2, 3, 4, 5, 4, 3, 2, 1}, spp);
    }
    pt_chain_params p = {};
    p.width = 8, p.height = 4, p.spp = 2, p.depth = 8;
    const int32_t pix[3] = {0, 31, 5};
    const float rays[14] = {0, 0, 0, 0, 0, -1, 1, 0, 0, 0, 1, 0, -1, 1};
    const int64_t begin[3] = {0, 1, 3}, bad0[3] = {1, 1, 3}, down[3] = {0, 2, 1};
    uint64_t st[2] = {1, 2};
    float out[9];
    CHECK(!refused([&] { pt::chain_validate(&p, pix, nullptr, begin, 2, st, out); }));
    CHECK(!refused([&] { pt::chain_validate(&p, nullptr, rays, begin, 1, st, out); }));
    CHECK(refused([&] { pt::chain_validate(&p, pix, rays, begin, 2, st, out); }));
    CHECK(refused([&] { pt::chain_validate(&p, nullptr, nullptr, begin, 2, st, out); }));
    CHECK(refused([&] { pt::chain_validate(&p, pix, nullptr, bad0, 2, st, out); }));
    CHECK(refused([&] { pt::chain_validate(&p, pix, nullptr, down, 2, st, out); }));
    const int32_t outside[3] = {0, 32, 5};
    CHECK(refused([&] { pt::chain_validate(&p, outside, nullptr, begin, 2, st, out); }));
    pt_chain_params q = p;
    q.spp = 0;
    CHECK(refused([&] { pt::chain_validate(&q, pix, nullptr, begin, 2, st, out); }));
    q = p, q.depth = -1;
    CHECK(refused([&] { pt::chain_validate(&q, pix, nullptr, begin, 2, st, out); }));
    ray_check_cases();
    printf(failures ? "chain_schedule: %d checks FAILED\n" : "chain_schedule ok\n", failures);
    return failures ? 1 : 0;
}
