/* Host sanitizer run of flame_update_dist / flame_update_dist_scratch_bytes: built against a copy
 * of libflame_amd.so whose HOST code is compiled with -fsanitize=address,undefined
 * (tests/abi_asan/Makefile).  Every launch call carries at least one invalid argument and
 * must be refused on the host with an error code and a message, before any HIP call, without a
 * sanitizer report.  No GPU is needed. */
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
        EXPECT(strstr(flame_last_error(), "flame_update_dist") != NULL || strstr(flame_last_error(), "n_chunks") != NULL, \
               #call " names the entry point");                                              \
    } while (0)

static uint64_t rng = 0xD1B54A32D192ED03ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    const flame_segment *fake = (const flame_segment *)(uintptr_t)4096;   /* never dereferenced: checks run first */
    const void *const *cl = (const void *const *)(uintptr_t)8192;
    double *d2 = (double *)(uintptr_t)12288;
    int64_t *nf = (int64_t *)(uintptr_t)16384;
    void *sc = (void *)(uintptr_t)20480;
    const int64_t big = (int64_t)1 << 40;

    /* the scratch size: flame_update_stats' (one pass, two instantiations), no cap on n_clients */
    for (int64_t c = 1; c <= 30000; c += (c < 200 ? 1 : 97))
        for (int32_t n = 1; n <= 5000; n += (n < 130 ? 1 : 211)) {
            const int64_t b = flame_update_dist_scratch_bytes(c, n);
            EXPECT(b == flame_update_stats_scratch_bytes(c, n) && b >= 8 * (int64_t)n, "scratch as the statistics'");
        }
    EXPECT(flame_update_dist_scratch_bytes(1, INT32_MAX) > 0, "no client cap");
    EXPECT(flame_update_dist_scratch_bytes(0, 9) == 0 && flame_update_dist_scratch_bytes(5, 0) == 0 &&
           flame_update_dist_scratch_bytes(-1, 9) == 0 && flame_update_dist_scratch_bytes(0x80000000ll, 9) == 0, "refused sizes");

    /* one defect per call */
    EXPECT_ERR(flame_update_dist(0, NULL, 1, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_dist(0, fake, 0, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_dist(0, fake, -2, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 0, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_dist(0, fake, 1, -1, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 0x80000000ll, cl, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, NULL, 9, d2, nf, sc, big, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 0, d2, nf, sc, big, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, INT32_MIN, d2, nf, sc, big, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_dist(FLAME_I64, fake, 1, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_update_dist(FLAME_I32, fake, 1, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_update_dist(6, fake, 1, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_dist(-1, fake, 1, 1, cl, 9, d2, nf, sc, big, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 9, NULL, nf, sc, big, NULL), FLAME_EINVAL, "output array");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 9, d2, NULL, sc, big, NULL), FLAME_EINVAL, "output array");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 9, d2, nf, NULL, big, NULL), FLAME_EINVAL, "scratch");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 9, d2, nf, sc, flame_update_dist_scratch_bytes(1, 9) - 1, NULL),
               FLAME_EINVAL, "too small");
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 9, d2, nf, sc, -5, NULL), FLAME_EINVAL, "too small");
    /* more clients than the Gram kernel takes are no defect here: with everything else valid but the
     * scratch size, the refusal is the scratch's */
    EXPECT_ERR(flame_update_dist(0, fake, 1, 1, cl, 100000, d2, nf, sc, 8, NULL), FLAME_EINVAL, "too small");

    /* 4,000 randomized calls, every one with a defect picked at random on top of random other
     * arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 4);
        int32_t n_segs = (int32_t)(next() % 5) + 1;
        int32_t n_clients = 1 + (int32_t)(next() % 200000);
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        int64_t sbytes = big;
        const flame_segment *segs = fake;
        const void *const *c = cl;
        double *dd = d2;
        int64_t *nn = nf;
        void *ss = sc;
        switch (next() % 9) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = -(int32_t)(next() % 1000); break;
        case 4: c = NULL; break;
        case 5: dtype = 4 + (int)(next() % 1000); break;
        case 6: if (next() & 1) dd = NULL; else nn = NULL; break;
        case 7: ss = NULL; break;
        default: sbytes = flame_update_dist_scratch_bytes(n_chunks, n_clients) - 1 - (int64_t)(next() % 4096); break;
        }
        int rc = flame_update_dist(dtype, segs, n_segs, n_chunks, c, n_clients, dd, nn, ss, sbytes, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_update_dist refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_update_dist message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("dist abi asan OK\n");
    return 0;
}
