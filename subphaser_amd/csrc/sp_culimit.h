// sp_culimit.h -- the SP_CU_LIMIT switch of sp_ctx_create as plain C++: no HIP types, so the host compiler alone builds
// it (tests/culimit_host_check.cpp).
//
// Every capped launch sizes its grid from ctx->n_cu and walks the work in a grid-stride loop; no output depends on the
// count.  SP_CU_LIMIT=n makes a context reckon with n compute units, so that the suite reaches the second and later
// passes of those loops on inputs of a megabase or two (tests/test_gpu_cu_limit.py).
#pragma once
#include <errno.h>
#include <stdlib.h>

// the compute units a context reckons with: `text` (the value of SP_CU_LIMIT, or NULL) when it is a decimal integer
// 1 <= n < n_cu with nothing before or after it, else the device's own n_cu
inline int sp_cu_limit(const char *text, int n_cu) {
    if (!text || text[0] < '0' || text[0] > '9') return n_cu;      // unset, empty, a sign, white space, garbage
    char *end = nullptr;
    errno = 0;
    const long long n = strtoll(text, &end, 10);
    if (errno || *end != '\0') return n_cu;
    return n >= 1 && n < (long long)n_cu ? (int)n : n_cu;
}
