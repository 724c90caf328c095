// rt_error.h — the error text behind rt_last_error_message (include/rt_abi.h) and the guard every C entry point of the
// library runs its body through.  Host code that needs no HIP (rt_error.cpp); private to the library.
#pragma once
#include <exception>
#include <new>
#include <string>
#include "../../include/rt_abi.h"

namespace rtapi {

// set the thread-local text behind rt_last_error_message (truncated, never throws) and return `code`
int fail(int code, const char *msg) noexcept;
inline int fail(int code, const std::string &msg) { return fail(code, msg.c_str()); }
// ... as "<what>: <msg>"
int fail_in(int code, const char *what, const char *msg) noexcept;

// Every exported function of the library runs its body through this: nothing unwinds into a C, Rust or ctypes caller.
// std::bad_alloc is RT_ERR_OUT_OF_MEMORY, any other exception RT_ERR_INVALID_ARGUMENT; the message names the entry point.
template <class F> int guarded(const char *what, F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail_in(RT_ERR_OUT_OF_MEMORY, what, "host allocation failed");
    } catch (const std::exception &e) {
        return fail_in(RT_ERR_INVALID_ARGUMENT, what, e.what());
    } catch (...) {
        return fail_in(RT_ERR_INVALID_ARGUMENT, what, "unknown exception");
    }
}

} // namespace rtapi
