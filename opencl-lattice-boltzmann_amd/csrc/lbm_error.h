// The error channel of liblbm_hip.so for its translation units besides lbm_hip.cpp (which owns the thread's message,
// lbm_last_error()): records a printf-style message for the calling thread and returns `code`.
#pragma once

__attribute__((visibility("hidden"), format(printf, 2, 3))) int lbm_fail(int code, const char *fmt, ...);
