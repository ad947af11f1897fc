// The one formatter behind the library's error texts.  Every subsystem keeps a thread-local text and a printf-style `fail` of its
// own - azmi_last_error, azmi_net_last_error, azmi_cache_last_error and azmi_samples_last_error are separate symbols over
// separate texts - and the body of each `fail` is this: the message is cut to 511 characters.  (symmetries.hip and leafnet_f32.hip
// write a fixed "what: HIP error" into 256 bytes and keep their own.)
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

// inside `int fail(int code, const char* fmt, ...)`: formats the arguments behind `fmt` into the std::string `text`
#define AZMI_FORMAT_ERROR(text, fmt)         \
  do {                                       \
    char buf_[512];                          \
    va_list ap_;                             \
    va_start(ap_, fmt);                      \
    vsnprintf(buf_, sizeof(buf_), fmt, ap_); \
    va_end(ap_);                             \
    (text) = buf_;                           \
  } while (0)
