/* Host sanitizer run of flame_update_gram / flame_update_gram_scratch_bytes /
 * flame_update_gram_max_clients: built against a copy of libflame_amd.so whose HOST code is
 * compiled with -fsanitize=address,undefined (tests/abi_asan/Makefile).  Every launch call
 * carries at least one invalid argument and must be refused on the host with an error code and a
 * message, before any HIP call, without a sanitizer report.  No GPU is needed. */
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

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    const flame_segment *fake = (const flame_segment *)(uintptr_t)4096;   /* never dereferenced: checks run first */
    const void *const *cl = (const void *const *)(uintptr_t)8192;
    double *g = (double *)(uintptr_t)12288;
    int64_t *nf = (int64_t *)(uintptr_t)16384;
    void *sc = (void *)(uintptr_t)20480;
    const int64_t big = (int64_t)1 << 40;
    const int max_n = flame_update_gram_max_clients();
    EXPECT(max_n == 1024, "max_clients");

    /* the scratch bound: at most 1 GiB everywhere, monotone in both arguments, 0 for what is refused */
    int64_t prev_c = 0;
    for (int64_t c = 1; c <= 30000; c += (c < 200 ? 1 : 97)) {
        int64_t prev_n = 0;
        for (int32_t n = 1; n <= max_n; n += (n < 130 ? 1 : 31)) {
            const int64_t b = flame_update_gram_scratch_bytes(c, n);
            EXPECT(b > 0 && b <= ((int64_t)1 << 30), "scratch within 1 GiB");
            EXPECT(b >= prev_n, "scratch monotone in n_clients");
            prev_n = b;
        }
        const int64_t at = flame_update_gram_scratch_bytes(c, max_n);
        EXPECT(at >= prev_c, "scratch monotone in n_chunks");
        prev_c = at;
    }
    EXPECT(flame_update_gram_scratch_bytes(24415, 1024) <= ((int64_t)1 << 30), "config 3 at 1,024 clients");
    EXPECT(flame_update_gram_scratch_bytes(0x7FFFFFFFll, 1024) <= ((int64_t)1 << 30), "the largest launch");
    EXPECT(flame_update_gram_scratch_bytes(0, 9) == 0 && flame_update_gram_scratch_bytes(5, 0) == 0 &&
           flame_update_gram_scratch_bytes(5, 1025) == 0 && flame_update_gram_scratch_bytes(-1, 9) == 0, "refused sizes");

    /* one defect per call */
    EXPECT_ERR(flame_update_gram(0, NULL, 1, 1, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_gram(0, fake, 0, 1, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_gram(0, fake, -2, 1, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 0, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_gram(0, fake, 1, -1, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 0x80000000ll, cl, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, NULL, 9, g, nf, sc, big, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 0, g, nf, sc, big, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, INT32_MIN, g, nf, sc, big, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, max_n + 1, g, nf, sc, big, NULL), FLAME_ENOTSUP, "n_clients");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, INT32_MAX, g, nf, sc, big, NULL), FLAME_ENOTSUP, "n_clients");
    EXPECT_ERR(flame_update_gram(FLAME_I64, fake, 1, 1, cl, 9, g, nf, sc, big, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_update_gram(FLAME_I32, fake, 1, 1, cl, 9, g, nf, sc, big, NULL), FLAME_ENOTSUP, "float dtypes only");
    EXPECT_ERR(flame_update_gram(6, fake, 1, 1, cl, 9, g, nf, sc, big, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_gram(-1, fake, 1, 1, cl, 9, g, nf, sc, big, NULL), FLAME_ENOTSUP, "unknown dtype");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 9, NULL, nf, sc, big, NULL), FLAME_EINVAL, "output array");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 9, g, NULL, sc, big, NULL), FLAME_EINVAL, "output array");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 9, g, nf, NULL, big, NULL), FLAME_EINVAL, "scratch");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 9, g, nf, sc, flame_update_gram_scratch_bytes(1, 9) - 1, NULL),
               FLAME_EINVAL, "too small");
    EXPECT_ERR(flame_update_gram(0, fake, 1, 1, cl, 9, g, nf, sc, -5, NULL), FLAME_EINVAL, "too small");

    /* 4,000 randomized calls, every one with a defect picked at random on top of random other
     * arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int dtype = (int)(next() % 4);
        int32_t n_segs = (int32_t)(next() % 5) + 1;
        int32_t n_clients = 1 + (int32_t)(next() % (uint64_t)max_n);
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        int64_t sbytes = big;
        const flame_segment *segs = fake;
        const void *const *c = cl;
        double *gg = g;
        int64_t *nn = nf;
        void *ss = sc;
        switch (next() % 10) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = -(int32_t)(next() % 1000); break;
        case 4: n_clients = max_n + 1 + (int32_t)(next() % 100000); break;
        case 5: c = NULL; break;
        case 6: dtype = 4 + (int)(next() % 1000); break;
        case 7: if (next() & 1) gg = NULL; else nn = NULL; break;
        case 8: ss = NULL; break;
        default: sbytes = flame_update_gram_scratch_bytes(n_chunks, n_clients) - 1 - (int64_t)(next() % 4096); break;
        }
        int rc = flame_update_gram(dtype, segs, n_segs, n_chunks, c, n_clients, gg, nn, ss, sbytes, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_update_gram refused");
        EXPECT(flame_last_error()[0] != 0, "randomized flame_update_gram message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("gram abi asan OK\n");
    return 0;
}
