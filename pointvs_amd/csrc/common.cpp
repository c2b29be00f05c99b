#include <stdarg.h>
#include <stdio.h>
#include "../../include/pvs_egnn.h"

static thread_local char g_err[512] = "";

void pvs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* pvs_last_error(void) { return g_err; }
extern "C" int pvs_version(void) { return 113; }
