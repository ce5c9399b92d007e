// Error convention of librga3_hip.so: 0 = ok, negative code otherwise; the message is thread-local (rga3_last_error).
// No HIP headers: shared by the device sources (through common.h) and by the host-only C++ files that also build under the CPU sanitizers.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include "../../include/rga3_hip.h"

namespace rga3 {

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define RGA3_CHECK_ARG(cond, ...)                                   \
    do {                                                            \
        if (!(cond)) return ::rga3::fail(RGA3_EINVAL, __VA_ARGS__); \
    } while (0)

// A view must hold its rows: a row stride (leading dimension, token / head / frame stride; elements) shorter than the width read or written through it makes rows
// overlap -- silently, for an output.  Refused before any launch.  A single row never uses its stride, so `rows` <= 1 passes whatever the stride says.
#define RGA3_CHECK_LD(who, name, ld, width, rows) \
    RGA3_CHECK_ARG((rows) <= 1 || (int64_t)(ld) >= (int64_t)(width), "%s: %s %ld is shorter than the %ld elements of a row", who, name, (long)(ld), (long)(width))

// The same for a [tokens, heads, D] operand addressed through (token, head) strides: a head stride must hold D, a token stride must hold D, and the tensor is either
// token-major (the token stride spans its heads) or head-major (the head stride spans its tokens; checked when the caller knows `tokens`, 0 = unknown).
inline int check_head_strides(const char* who, const char* name, int64_t st, int64_t sh, int64_t tokens, int64_t heads, int64_t D) {
    if (heads > 1 && sh < D) return fail(RGA3_EINVAL, "%s: %s head stride %ld is shorter than D = %ld", who, name, (long)sh, (long)D);
    if (tokens != 1 && st < D) return fail(RGA3_EINVAL, "%s: %s token stride %ld is shorter than D = %ld", who, name, (long)st, (long)D);
    if (heads > 1 && tokens != 1 && st < (heads - 1) * sh + D) {
        if (sh < st) return fail(RGA3_EINVAL, "%s: %s token stride %ld is shorter than the %ld heads of %ld it spans", who, name, (long)st, (long)heads, (long)sh);
        if (tokens > 0 && sh < (tokens - 1) * st + D)
            return fail(RGA3_EINVAL, "%s: %s head stride %ld is shorter than the %ld tokens of %ld it spans", who, name, (long)sh, (long)tokens, (long)st);
    }
    return 0;
}
#define RGA3_CHECK_HEADS(who, name, st, sh, tokens, heads, D)                                                  \
    do {                                                                                                       \
        if (int rc_ = ::rga3::check_head_strides(who, name, st, sh, tokens, heads, D)) return rc_;             \
    } while (0)

}  // namespace rga3
