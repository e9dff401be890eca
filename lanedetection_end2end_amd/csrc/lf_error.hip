// The library's per-thread error message (lf_fail fills it, every entry point returns -1 then) and its ABI version.
#include "lf_common.h"

#include <stdarg.h>

thread_local char lf_err_buf[512] = "";
int lf_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(lf_err_buf, sizeof(lf_err_buf), fmt, ap);
    va_end(ap);
    return -1;
}
extern "C" const char* lf_last_error(void) { return lf_err_buf; }
extern "C" int lf_abi_version(void) { return LF_ABI_VERSION; }
