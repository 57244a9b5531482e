/* devsrc.cpp -- the device library text (device/pt_device.h), embedded at
 * build time so every generated scene module carries the exact header the
 * library was built with (the JIT cache key hashes it) -- chained modules the
 * whole text, every other kind the text without its PT_CHAIN regions. */
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "internal.h"

namespace pt
{
namespace
{
/* text without the lines from each `#ifdef PT_CHAIN` line to the `#endif` line
 * that carries the PT_CHAIN comment (pt_device.h keeps everything of the
 * chained kind between such pairs, never nested, and nothing of it elsewhere) */
std::string without_chain(const std::string &text)
{
    static const std::string open = "#ifdef PT_CHAIN", close = "#endif /* PT_CHAIN */";
    std::string out;
    out.reserve(text.size());
    bool skip = false;
    for (size_t b = 0; b < text.size();) {
        const size_t nl = text.find('\n', b);
        const size_t len = (nl == std::string::npos ? text.size() : nl) - b; /* the line without its newline */
        const size_t e = nl == std::string::npos ? text.size() : nl + 1;
        if (text.compare(b, len, open) == 0)
            skip = true;
        if (!skip)
            out.append(text, b, e - b);
        else if (text.compare(b, len, close) == 0)
            skip = false;
        b = e;
    }
    return out;
}
} // namespace

std::string device_library_source(bool chain)
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
        return chain ? text.str() : without_chain(text.str());
    }
    static const char src[] =
#include "pt_device_src.inc"
        ;
    static const std::string plain = without_chain(src);
    return chain ? std::string(src) : plain;
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
std::string device_converge_source()
{
    static const char src[] =
#include "pt_converge_src.inc"
        ;
    return src;
}
std::string device_guides_source()
{
    static const char src[] =
#include "pt_guides_src.inc"
        ;
    return src;
}
std::string device_denoise_source()
{
    static const char src[] =
#include "pt_denoise_src.inc"
        ;
    return src;
}
} // namespace pt
