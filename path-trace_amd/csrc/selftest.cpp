/* selftest.cpp -- the device library's self-tests (include/pt/pt.h
 * pt_selftest_*): pt_device.h compiled with PT_SELFTEST, loaded for one call. */
#include <algorithm>

#include "hip_util.h"

using namespace pt;

/* compiled before any device is touched: a build without a GPU fills the
 * code-object cache through pt_selftest_math and takes its device error */
static const std::vector<char> &selftest_code()
{
    Generated g;
    g.source = "#define PT_SELFTEST 1\n" + device_library_source();
    g.key = "selftest";
    return code_object(g);
}

extern "C" {

/* Runs the device self-test of the exact sqrt/div fast paths on n inputs;
 * mismatches[0..2] = sqrt, div, normalize mismatch counts (all 0 expected). */
int pt_selftest_math(int device, uint64_t n, uint64_t seed, uint64_t *mismatches)
{
    return guard([&] {
        if (!mismatches)
            throw Error(PT_ERR_ARG, "null mismatches");
        const std::vector<char> &code = selftest_code();
        HIPCHECK(hipSetDevice(device));
        Module mod;
        mod.load(code);
        hipFunction_t fn = mod.fn("pt_selftest_math");
        DevBuf<uint64_t> bad;
        bad.ensure(4);
        HIPCHECK(hipMemset(bad.p, 0, 32));
        void *args[] = {&n, &seed, &bad.p};
        HIPCHECK(hipModuleLaunchKernel(fn, 4096, 1, 1, 256, 1, 1, 0, nullptr, args, nullptr));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(mismatches, bad.p, 24, hipMemcpyDeviceToHost));
        return PT_OK;
    });
}

/* The device's restated glibc float libm on n operand pairs (pt_device.h
 * pt_selftest_libm): out = n x (atan2f(y, x), asinf(y), logf(x)). */
int pt_selftest_libm(int device, const float *ops, int64_t n, float *out)
{
    return guard([&] {
        if (!ops || !out || n < 0)
            throw Error(PT_ERR_ARG, "bad arguments");
        const std::vector<char> &code = selftest_code();
        HIPCHECK(hipSetDevice(device));
        Module mod;
        mod.load(code);
        hipFunction_t fn = mod.fn("pt_selftest_libm");
        DevBuf<float> d_ops, d_out;
        d_ops.ensure((size_t)std::max<int64_t>(1, 2 * n));
        d_out.ensure((size_t)std::max<int64_t>(1, 3 * n));
        if (n) {
            HIPCHECK(hipMemcpy(d_ops.p, ops, (size_t)n * 8, hipMemcpyHostToDevice));
            uint64_t nn = (uint64_t)n;
            void *args[] = {&d_ops.p, &nn, &d_out.p};
            HIPCHECK(hipModuleLaunchKernel(fn, 1024, 1, 1, 256, 1, 1, 0, nullptr, args, nullptr));
            HIPCHECK(hipDeviceSynchronize());
            HIPCHECK(hipMemcpy(out, d_out.p, (size_t)n * 12, hipMemcpyDeviceToHost));
        }
        return PT_OK;
    });
}

} // extern "C"
