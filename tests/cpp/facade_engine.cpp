// PathTrace::DefaultRandomEngine of the facade (include/pt/PathTrace.hpp) against
// the reference engine's public behaviour (include/path-trace.h:21-54); no GPU.
//   facade_engine  -> prints the first 5 outputs for seeds 0, 1, 12345 (one per
//                     line, the layout of tests/golden/kat.npy's first 15 words);
//                     exit code != 0 names the failed member check
#include <cstdio>

#include "pt/PathTrace.hpp"

using namespace PathTrace;

int main()
{
    if (DefaultRandomEngine::min() != 0u || DefaultRandomEngine::max() != 0xFFFFFFFFu)
        return 3;
    DefaultRandomEngine d, z;
    z.seed(0);
    if (d.state() != z.state() || d.state() != 0x12476242ull) /* the default constructor is seed(0) */
        return 4;
    const unsigned seeds[3] = {0, 1, 12345};
    for (unsigned s : seeds) {
        DefaultRandomEngine e;
        e.seed(s);
        if (e.state() != (uint64_t)(s ^ 0x12476242u))
            return 5;
        for (int k = 0; k < 5; k++) printf("%u\n", e());
    }
    const unsigned long long counts[] = {0, 1, 2, 7, 1000, 65537};
    for (unsigned long long n : counts) { /* discard(n) is n calls */
        DefaultRandomEngine a, b;
        a.seed(77), b.seed(77);
        a.discard(n);
        for (unsigned long long k = 0; k < n; k++) b();
        if (a.state() != b.state() || a() != b())
            return 6;
    }
    DefaultRandomEngine a, b; /* state() round trip, full 64 bits */
    a.seed(5);
    a.discard(12345);
    b.state(a.state());
    if (b.state() != a.state() || a() != b())
        return 7;
    b.state(0xFEDCBA9876543210ull);
    if (b.state() != 0xFEDCBA9876543210ull)
        return 8;
    return 0;
}
