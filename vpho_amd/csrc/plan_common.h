// What the host-only plan headers (conv_plan.h, score_plan.h) share: the refusal text buffer and the environment reader.
// The C and C++ standard library only.
#ifndef VPHO_PLAN_COMMON_H
#define VPHO_PLAN_COMMON_H
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

namespace {

constexpr int PLAN_ERR = 512;                 // bytes of an error text: vpho_last_error()'s own buffer, so nothing is cut that was not cut before
#if defined(__GNUC__) || defined(__clang__)
__attribute__((format(printf, 2, 3)))
#endif
inline int plan_fail(char* err, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, PLAN_ERR, fmt, ap);
    va_end(ap);
    return 1;
}
#define PLAN_REQUIRE(err, cond, ...) do { if (!(cond)) return plan_fail(err, __VA_ARGS__); } while (0)
inline int env_int(const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; }

}  // namespace
#endif
