/* Host sanitizer run of flame_noise_fill: built against a copy of libflame_amd.so whose HOST code is
 * compiled with -fsanitize=address,undefined (tests/abi_asan/Makefile).  Every call carries at
 * least one invalid argument and must be refused on the host with an error code and a message, before
 * any HIP call, without a sanitizer report.  No GPU is needed. */
#include <math.h>
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
        EXPECT(strstr(flame_last_error(), (substr)) != NULL, #call " msg");                   \
        EXPECT(strstr(flame_last_error(), "flame_noise_fill") != NULL, #call " names the entry point"); \
    } while (0)

static uint64_t rng = 0xD1B54A32D192ED03ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    const flame_segment *fake = (const flame_segment *)(uintptr_t)4096;   /* never dereferenced: checks run first */
    const uint32_t *sm = (const uint32_t *)(uintptr_t)8192;
    const int64_t *st = (const int64_t *)(uintptr_t)12288;
    const uint64_t seed = 1234ull | 5678ull << 32;

    /* the table and the ABI version are what they were */
    EXPECT(flame_launch_branches() == 100 && flame_abi_version() == 1, "branch table / ABI version unchanged");

    /* one defect per call */
    EXPECT_ERR(flame_noise_fill(0, NULL, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_noise_fill(0, fake, 0, 1, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_noise_fill(0, fake, -2, 1, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_noise_fill(0, fake, INT32_MIN, 1, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, 0, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, -1, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, 0x80000000ll, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, INT64_MIN, sm, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_noise_fill(FLAME_I64, fake, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_noise_fill(FLAME_I32, fake, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_noise_fill(6, fake, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_noise_fill(-1, fake, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_noise_fill(INT32_MAX, fake, 1, 1, sm, st, seed, 0, 1.0, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, 1, NULL, st, seed, 0, 1.0, NULL), FLAME_EINVAL, "streams / starts");
    EXPECT_ERR(flame_noise_fill(0, fake, 1, 1, sm, NULL, seed, 0, 1.0, NULL), FLAME_EINVAL, "streams / starts");
    for (int dt = 0; dt < 4; ++dt) {
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, -1.0, NULL), FLAME_EINVAL, "std");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, -4.9e-324, NULL), FLAME_EINVAL, "std");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, (double)NAN, NULL), FLAME_EINVAL, "std");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, (double)INFINITY, NULL), FLAME_EINVAL, "std");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, -(double)INFINITY, NULL), FLAME_EINVAL, "std");
    }
    /* an std whose fp32 rounding is infinite: refused for the dtypes that round it, not for fp64 (whose
     * call gets as far as its NULL array) */
    for (int dt = 0; dt < 3; ++dt) {
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, 0x1.ffffffp127, NULL), FLAME_EINVAL, "infinite fp32");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, st, seed, 0, 1e300, NULL), FLAME_EINVAL, "infinite fp32");
        EXPECT_ERR(flame_noise_fill(dt, fake, 1, 1, sm, NULL, seed, 0, 0x1.fffffefffffffp127, NULL), FLAME_EINVAL, "streams / starts");
    }
    EXPECT_ERR(flame_noise_fill(FLAME_F64, fake, 1, 1, sm, NULL, seed, 0, 1e300, NULL), FLAME_EINVAL, "streams / starts");

    /* 4,000 randomized calls, every one with a defect picked at random on top of random other
     * arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 4);
        int32_t n_segs = (int32_t)(next() % 5) + 1;
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        const flame_segment *segs = fake;
        const uint32_t *a = sm;
        const int64_t *b = st;
        double std = (double)(next() % 1000) / 64.0;
        switch (next() % 6) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: dtype = 4 + (int)(next() % 1000); break;
        case 4: if (next() & 1) a = NULL; else b = NULL; break;
        default: std = (next() & 1) ? -1.0 - (double)(next() % 7) : ((next() & 1) ? (double)NAN : (double)INFINITY); break;
        }
        int rc = flame_noise_fill(dtype, segs, n_segs, n_chunks, a, b, next(), (uint32_t)next(), std, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_noise_fill refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_noise_fill message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("noise abi asan OK\n");
    return 0;
}
