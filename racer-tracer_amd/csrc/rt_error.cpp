// rt_error.cpp — the thread-local error text of the library (rt_error.h).  Host code, no device runtime needed.
#include "rt_error.h"
#include <stdio.h>

namespace {
thread_local char g_last_error[1024]; // a fixed buffer: setting it cannot throw (rtapi::guarded's handlers use it)
} // namespace

int rtapi::fail(int code, const char *msg) noexcept {
    snprintf(g_last_error, sizeof g_last_error, "%s", msg);
    return code;
}
int rtapi::fail_in(int code, const char *what, const char *msg) noexcept {
    snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, msg);
    return code;
}

extern "C" const char *rt_last_error_message(void) { return g_last_error; }
