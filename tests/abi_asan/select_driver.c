/* Host sanitizer run of flame_agg_select / flame_agg_select_max_clients: built against a copy of
 * libflame_amd.so whose HOST code is compiled with -fsanitize=address,undefined
 * (tests/abi_asan/Makefile).  Every call carries at least one invalid argument and must be
 * refused on the host with an error code and a message, before any HIP call, without a sanitizer
 * report.  No GPU is needed. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flame_amd.h"

static int failures = 0;
#define EXPECT(cond, what)                                                                   \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "FAIL %s:%d %s (last error: %s)\n", __FILE__, __LINE__, what,     \
                    flame_last_error());                                                     \
            ++failures;                                                                      \
        }                                                                                    \
    } while (0)
#define EXPECT_ERR(call, code, substr)                                                       \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        EXPECT(rc_ == (code), #call);                                                        \
        EXPECT(strstr(flame_last_error(), "flame_agg_select") != NULL || strstr(flame_last_error(), "n_chunks") != NULL, \
               #call " names the entry point");                                              \
        if ((substr)[0]) EXPECT(strstr(flame_last_error(), (substr)) != NULL, #call " msg");  \
    } while (0)

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    const flame_segment *fake = (const flame_segment *)(uintptr_t)4096;   /* never dereferenced: checks run first */
    const void *const *cl = (const void *const *)(uintptr_t)8192;
    const int cap = flame_agg_select_max_clients();
    EXPECT(cap >= 4096, "max_clients");
    EXPECT(flame_agg_trimmed_max_k() == 16, "the chain kernel's capacity is unchanged");

    /* one defect per call */
    EXPECT_ERR(flame_agg_select(0, 0, NULL, 1, 1, cl, 64, 31, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 0, 1, cl, 64, 31, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_select(0, 0, fake, -2, 1, cl, 64, 31, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 0, cl, 64, 31, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, -1, cl, 64, 31, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 0x80000000ll, cl, 64, 31, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, NULL, 64, 31, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 64, -1, NULL), FLAME_EINVAL, "trim_k");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 64, INT32_MIN, NULL), FLAME_EINVAL, "trim_k");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 64, 32, NULL), FLAME_EINVAL, "2 * trim_k");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 34, 17, NULL), FLAME_EINVAL, "2 * trim_k");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 4096, INT32_MAX, NULL), FLAME_EINVAL, "2 * trim_k");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, 0, 0, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, INT32_MIN, 0, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, cap + 1, 17, NULL), FLAME_ENOTSUP, "flame_agg_select_max_clients");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, INT32_MAX, 0, NULL), FLAME_ENOTSUP, "flame_agg_select_max_clients");
    EXPECT_ERR(flame_agg_select(0, 0, fake, 1, 1, cl, INT32_MAX, INT32_MAX, NULL), FLAME_ENOTSUP, "flame_agg_select_max_clients");
    EXPECT_ERR(flame_agg_select(FLAME_I64, 0, fake, 1, 1, cl, 64, 31, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_agg_select(FLAME_I32, 0, fake, 1, 1, cl, 64, 31, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_agg_select(6, 0, fake, 1, 1, cl, 64, 31, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_agg_select(-1, 0, fake, 1, 1, cl, 64, 31, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_agg_select(0, 8u, fake, 1, 1, cl, 64, 31, NULL), FLAME_EINVAL, "unknown flags");
    EXPECT_ERR(flame_agg_select(0, 0x80000000u, fake, 1, 1, cl, 64, 31, NULL), FLAME_EINVAL, "unknown flags");
    EXPECT_ERR(flame_agg_select(0, FLAME_AGG_SEG_RATES, fake, 1, 1, cl, 64, 31, NULL), FLAME_ENOTSUP, "SEG_RATES");

    /* 4,000 randomized calls, every one with a defect picked at random on top of random (possibly
     * also invalid) other arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 4);
        unsigned flags = (unsigned)(next() % 2) | ((next() & 1) ? FLAME_AGG_XCD_MAP : 0u);
        int32_t n_segs = (int32_t)(next() % 5) + 1;
        int32_t k = (int32_t)(next() % 3000);
        int32_t n_clients = 2 * k + 1 + (int32_t)(next() % 2000);
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        const flame_segment *segs = fake;
        const void *const *c = cl;
        switch (next() % 9) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = 2 * k - (int32_t)(next() % 1000); break;
        case 4: c = NULL; break;
        case 5: dtype = 4 + (int)(next() % 1000); break;
        case 6: flags |= (next() & 1) ? FLAME_AGG_SEG_RATES : (8u << (next() % 20)); break;
        case 7: k = -1 - (int32_t)(next() % 100000); break;
        default: n_clients = cap + 1 + (int32_t)(next() % 100000); k = (int32_t)(next() % 40000); break;
        }
        int rc = flame_agg_select(dtype, flags, segs, n_segs, n_chunks, c, n_clients, k, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_agg_select refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_agg_select message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("select abi asan OK\n");
    return 0;
}
