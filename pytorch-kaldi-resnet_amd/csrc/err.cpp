// Error string storage + version for libspkhip.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "spk_common.h"

static thread_local char g_err[512] = "";

void spk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* spk_last_error(void) { return g_err; }
extern "C" int spk_version(void) { return 300; }

// environment SPK_FL_VARIANTS (default 1), read once per process: 0 = every launch takes the generic instance of its kernel
// (A/B runs and identity tests on one build)
bool spk_fl_variants_enabled() {
    static const bool on = [] {
        const char* e = getenv("SPK_FL_VARIANTS");
        return !(e && e[0] == '0' && e[1] == 0);
    }();
    return on;
}
// bit 0: built with SPK_EXPERIMENTAL - the measured, not-faster kernel forms are present (producer / consumer convolution and
// weight gradient, in-wave pipelined weight gradient, in-wave pipelined fused-BatchNorm-backward data gradient)
extern "C" int spk_build_flags(void) {
#ifdef SPK_EXPERIMENTAL
    return 1;
#else
    return 0;
#endif
}
