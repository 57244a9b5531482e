/* devsrc.cpp -- the device library text (device/pt_device.h), embedded at
 * build time so every generated scene module carries the exact header the
 * library was built with (the JIT cache key hashes it). */
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "internal.h"

namespace pt
{
std::string device_library_source()
{
    /* experiment hook: A/B a different device library text in the same run,
     * e.g. PT_DEVICE_HEADER=tools/ab/old.h (profiling only); every module
     * kind takes it, so tools/same_code.py compares all of them */
    const char *hdr = getenv("PT_DEVICE_HEADER");
    if (hdr && *hdr) {
        std::ifstream f(hdr);
        if (!f)
            throw Error(PT_ERR_ARG, std::string("PT_DEVICE_HEADER not readable: ") + hdr);
        std::ostringstream text;
        text << f.rdbuf();
        return text.str();
    }
    static const char src[] =
#include "pt_device_src.inc"
        ;
    return src;
}
std::string device_user_object_source()
{
    static const char src[] =
#include "pt_user_object_src.inc"
        ;
    return src;
}
std::string device_user_object_n_source()
{
    static const char src[] =
#include "pt_user_object_n_src.inc"
        ;
    return src;
}
} // namespace pt
