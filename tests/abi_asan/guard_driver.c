/* Host sanitizer run of the update guard's two entry points (flame_update_stats,
 * flame_agg_reduce_scaled): built against a copy of libflame_amd.so whose HOST code is compiled
 * with -fsanitize=address,undefined (tests/abi_asan/Makefile).  Every call carries at least
 * one invalid argument and must be refused on the host with an error code and a message, before
 * any HIP call, without a sanitizer report.  No GPU is needed. */
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
        if ((substr)[0]) EXPECT(strstr(flame_last_error(), (substr)) != NULL, #call " msg");  \
    } while (0)

static uint64_t rng = 0xD1B54A32D192ED03ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    void *fake = (void *)(uintptr_t)4096;     /* never dereferenced: checks run first */
    double *sq = (double *)fake;
    int64_t *nf = (int64_t *)fake;
    const int64_t need = flame_update_stats_scratch_bytes(100, 9);
    EXPECT(need > 0 && need % 8 == 0 && need >= 9 * 8, "scratch size");
    EXPECT(need * 100 <= 100ll * 9 * 4096, "scratch below 1 % of the bytes read");
    EXPECT(flame_update_stats_scratch_bytes(0, 9) == 0 && flame_update_stats_scratch_bytes(100, 0) == 0 &&
           flame_update_stats_scratch_bytes(-5, -5) == 0, "scratch size of invalid arguments");

    /* flame_update_stats: one defect per call */
    EXPECT_ERR(flame_update_stats(0, NULL, 1, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_stats(0, fake, 0, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 0, fake, 9, sq, nf, fake, need, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 0, sq, nf, fake, need, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, -3, sq, nf, fake, need, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, NULL, 9, sq, nf, fake, need, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_update_stats(FLAME_I64, fake, 1, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_ENOTSUP, "integer");
    EXPECT_ERR(flame_update_stats(FLAME_I32, fake, 1, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_ENOTSUP, "integer");
    EXPECT_ERR(flame_update_stats(42, fake, 1, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_stats(-1, fake, 1, 100, fake, 9, sq, nf, fake, need, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 9, NULL, nf, fake, need, NULL), FLAME_EINVAL, "output");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 9, sq, NULL, fake, need, NULL), FLAME_EINVAL, "output");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 9, sq, nf, NULL, need, NULL), FLAME_EINVAL, "scratch");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 9, sq, nf, fake, need - 8, NULL), FLAME_EINVAL, "too small");
    EXPECT_ERR(flame_update_stats(0, fake, 1, 100, fake, 9, sq, nf, fake, -1, NULL), FLAME_EINVAL, "too small");

    /* flame_agg_reduce_scaled */
    const float *f = (const float *)fake;
    const double *d = (const double *)fake;
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, NULL, 0, 1, NULL, 0, NULL, NULL, NULL, NULL, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, fake, 1, 0, fake, 1, f, d, f, d, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, fake, 1, 1, fake, -1, f, d, f, d, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, fake, 1, 1, NULL, 1, f, d, f, d, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_agg_reduce_scaled(0, FLAME_AGG_SEG_RATES, fake, 1, 1, fake, 1, f, d, f, d, NULL), FLAME_ENOTSUP,
               "SEG_RATES");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 8, fake, 1, 1, fake, 1, f, d, f, d, NULL), FLAME_EINVAL, "unknown flags");
    EXPECT_ERR(flame_agg_reduce_scaled(0, FLAME_AGG_INIT_FIRST, fake, 1, 1, NULL, 0, f, d, f, d, NULL), FLAME_EINVAL,
               "at least one client");
    EXPECT_ERR(flame_agg_reduce_scaled(FLAME_I64, 0, fake, 1, 1, fake, 1, f, d, f, d, NULL), FLAME_ENOTSUP, "integer");
    EXPECT_ERR(flame_agg_reduce_scaled(FLAME_I32, 0, fake, 1, 1, fake, 1, f, d, f, d, NULL), FLAME_ENOTSUP, "integer");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, fake, 1, 1, fake, 1, NULL, d, f, d, NULL), FLAME_EINVAL, "rate");
    EXPECT_ERR(flame_agg_reduce_scaled(FLAME_F64, 0, fake, 1, 1, fake, 1, f, NULL, f, d, NULL), FLAME_EINVAL, "rate");
    EXPECT_ERR(flame_agg_reduce_scaled(0, 0, fake, 1, 1, fake, 1, f, d, NULL, d, NULL), FLAME_EINVAL, "scale");
    EXPECT_ERR(flame_agg_reduce_scaled(FLAME_F64, 0, fake, 1, 1, fake, 1, f, d, f, NULL, NULL), FLAME_EINVAL, "scale");
    EXPECT_ERR(flame_agg_reduce_scaled(31, 0, fake, 1, 1, fake, 1, f, d, f, d, NULL), FLAME_ENOTSUP, "unknown dtype");

    /* 4,000 randomized calls of each, every one with a defect picked at random on top of random
     * (possibly also invalid) other arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 6);
        int32_t n_segs = (int32_t)(next() % 5) + 1, n_clients = (int32_t)(next() % 2000) + 1;
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        int64_t sb = flame_update_stats_scratch_bytes(n_chunks, n_clients);
        const void *segs = fake, *cl = fake;
        double *o1 = sq;
        int64_t *o2 = nf;
        void *scr = fake;
        switch (next() % 9) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = -(int32_t)(next() % 1000); break;
        case 4: cl = NULL; break;
        case 5: dtype = (next() & 1) ? 4 + (int)(next() % 2) : 6 + (int)(next() % 1000); break;
        case 6: o1 = NULL; break;
        case 7: o2 = NULL; break;
        default: if (next() & 1) scr = NULL; else sb = sb - 1 - (int64_t)(next() % (uint64_t)sb); break;
        }
        int rc = flame_update_stats(dtype, (const flame_segment *)segs, n_segs, n_chunks, (const void *const *)cl,
                                    n_clients, o1, o2, scr, sb, NULL);
        /* a random integer dtype on an otherwise single-defect call is refused too */
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_update_stats refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_update_stats message");
    }
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 4);
        unsigned flags = (unsigned)(next() % 2) | ((next() & 1) ? FLAME_AGG_XCD_MAP : 0u);
        int32_t n_segs = (int32_t)(next() % 5) + 1, n_clients = (int32_t)(next() % 2000) + 1;
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        const void *segs = fake, *cl = fake;
        const float *r32 = f, *s32 = f;
        const double *r64 = d, *s64 = d;
        switch (next() % 9) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = -1 - (int32_t)(next() % 1000); break;
        case 4: cl = NULL; break;
        case 5: dtype = 4 + (int)(next() % 1000); break;
        case 6: flags |= (next() & 1) ? FLAME_AGG_SEG_RATES : (8u << (next() % 20)); break;
        case 7: r32 = NULL; r64 = NULL; break;
        default: s32 = NULL; s64 = NULL; break;
        }
        int rc = flame_agg_reduce_scaled(dtype, flags, (const flame_segment *)segs, n_segs, n_chunks,
                                         (const void *const *)cl, n_clients, r32, r64, s32, s64, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_agg_reduce_scaled refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_agg_reduce_scaled message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("guard abi asan OK\n");
    return 0;
}
