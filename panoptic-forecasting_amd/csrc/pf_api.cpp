// Error reporting + version of libpfhip.so, and the host view of label_scan.h's span computation (tests).
#include <cstring>

#include "label_scan.h"
#include "pf_common.h"

namespace pf {

char *error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace pf

extern "C" int pf_version(void) { return 1000; }
extern "C" const char *pf_last_error(void) { return pf::error_buffer(); }

extern "C" int pf_debug_label_scan_span(unsigned long long addr_a, unsigned long long addr_b, int esz_a, int esz_b, int align_a, int align_b,
                                        unsigned long long n, int P, unsigned long long *out5) {
    if (!out5 || esz_a < 1 || esz_b < 1 || align_a < 1 || align_b < 1 || P < 1)
        return pf::fail(PF_EINVAL, "pf_debug_label_scan_span: null output or a size, alignment or unit below 1");
    const pf::ScanSpan s = pf::scan_span((uintptr_t)addr_a, (uintptr_t)addr_b, (size_t)esz_a, (size_t)esz_b, (size_t)align_a, (size_t)align_b,
                                         (size_t)n, (size_t)P);
    out5[0] = s.head;
    out5[1] = s.units;
    out5[2] = s.tail0;
    out5[3] = s.al_a;
    out5[4] = s.al_b;
    return PF_OK;
}
