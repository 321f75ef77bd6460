// Error reporting of the echoscene HIP library without a HIP header: what the host-only units (es_conv_route) share with the rest
// through es_common.h.
#pragma once

void es_set_error(const char* fmt, ...);        // the text es_last_error() returns (es_runtime.hip; per thread)

#define ES_REQUIRE(cond, ...)                                                                \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            es_set_error(__VA_ARGS__);                                                       \
            return 2;                                                                        \
        }                                                                                    \
    } while (0)
