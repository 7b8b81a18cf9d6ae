/* Host sanitizer run of flame_agg_reduce_mx: built against a copy of libflame_amd.so whose HOST
 * code is compiled with -fsanitize=address,undefined (tests/abi_asan/Makefile).  Every call
 * carries at least one invalid argument and must be refused on the host with an error code and a
 * message naming the entry point, before any HIP call, without a sanitizer report.  No GPU is
 * needed. */
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
        EXPECT(strstr(flame_last_error(), "flame_agg_reduce_mx") != NULL, #call " names the entry point"); \
        if ((substr)[0]) EXPECT(strstr(flame_last_error(), (substr)) != NULL, #call " msg");  \
    } while (0)

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(void) {
    const flame_segment *fake = (const flame_segment *)(uintptr_t)4096;   /* never dereferenced: checks run first */
    const void *const *cl = (const void *const *)(uintptr_t)8192;
    const void *const *bs = (const void *const *)(uintptr_t)20480;
    const float *r = (const float *)(uintptr_t)12288;
    const float *sc = (const float *)(uintptr_t)16384;
    const int E4 = FLAME_FP8_E4M3, E5 = FLAME_FP8_E5M2, F = FLAME_F32;
    EXPECT(flame_launch_branches() == 100, "the launch-branch table is unchanged");
    EXPECT(flame_abi_version() == 1, "the ABI version is unchanged");
    EXPECT(flame_chunk_elems(E4) == 4096 && flame_chunk_elems(E5) == 4096, "the client dtype's chunk");
    EXPECT(E4 == 10 && E5 == 11, "the next free element codes");

    /* one defect per call: the dtype pair */
    const int pairs[][2] = {{FLAME_F32, FLAME_F32}, {FLAME_BF16, FLAME_F32}, {FLAME_F16, FLAME_F32},
                            {FLAME_F64, FLAME_F32}, {FLAME_I64, FLAME_F32}, {FLAME_I32, FLAME_F32},
                            {FLAME_U8, FLAME_F32}, {FLAME_BOOL, FLAME_F32}, {12, FLAME_F32}, {-1, FLAME_F32},
                            {FLAME_FP8_E4M3, FLAME_BF16}, {FLAME_FP8_E4M3, FLAME_F16}, {FLAME_FP8_E5M2, FLAME_F64},
                            {FLAME_FP8_E5M2, FLAME_FP8_E5M2}, {FLAME_FP8_E4M3, FLAME_FP8_E5M2}, {FLAME_FP8_E4M3, -1},
                            {FLAME_FP8_E5M2, 12}};
    for (size_t i = 0; i < sizeof(pairs) / sizeof(pairs[0]); ++i) {
        char a[32], b[32];
        snprintf(a, sizeof a, "client dtype %d", pairs[i][0]);
        snprintf(b, sizeof b, "aggregate dtype %d", pairs[i][1]);
        EXPECT_ERR(flame_agg_reduce_mx(pairs[i][0], pairs[i][1], 0, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, a);
        EXPECT(strstr(flame_last_error(), b) != NULL, "the message names the aggregate dtype");
    }
    /* the tables and counts */
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, NULL, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 0, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, 0, fake, -2, 1, cl, bs, 3, r, sc, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, 0, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, -1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, 0, fake, 1, 0x80000000ll, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, 1, NULL, bs, 3, r, NULL, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, 1, cl, NULL, 3, r, NULL, NULL), FLAME_EINVAL, "block scale pointer");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, 0, fake, 1, 1, cl, NULL, 3, r, sc, NULL), FLAME_EINVAL, "block scale pointer");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, 1, cl, bs, 0, r, NULL, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0, fake, 1, 1, cl, bs, INT32_MIN, r, sc, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, 0, fake, 1, 1, cl, bs, 3, NULL, NULL, NULL), FLAME_EINVAL, "rate array");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, 0, fake, 1, 1, cl, bs, 3, NULL, sc, NULL), FLAME_EINVAL, "rate array");
    /* the flags */
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, FLAME_AGG_INIT_FIRST, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, "INIT_FIRST");
    EXPECT_ERR(flame_agg_reduce_mx(E5, F, FLAME_AGG_INIT_FIRST | FLAME_AGG_XCD_MAP, fake, 1, 1, cl, bs, 3, r, sc, NULL),
               FLAME_ENOTSUP, "INIT_FIRST");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, FLAME_AGG_SEG_RATES, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, "SEG_RATES");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 8u, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "unknown flags");
    EXPECT_ERR(flame_agg_reduce_mx(E4, F, 0x80000000u, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "unknown flags");

    /* the older reduce entry points refuse the two new codes as any unknown code (host tables that
     * pass their pointer checks; the dtype is refused before a launch) */
    for (int k = 0; k < 2; ++k) {
        const int code = k ? E5 : E4;
        EXPECT(flame_agg_reduce(code, 0, fake, 1, 1, cl, 3, r, (const double *)r, NULL) == FLAME_ENOTSUP, "flame_agg_reduce");
        EXPECT(flame_agg_reduce_scaled(code, 0, fake, 1, 1, cl, 3, r, (const double *)r, sc, (const double *)sc, NULL) ==
                   FLAME_ENOTSUP, "flame_agg_reduce_scaled");
        EXPECT(flame_agg_reduce_mixed(code, F, 0, fake, 1, 1, cl, 3, r, NULL, NULL) == FLAME_ENOTSUP, "flame_agg_reduce_mixed");
        EXPECT(flame_agg_reduce_mixed(FLAME_BF16, code, 0, fake, 1, 1, cl, 3, r, NULL, NULL) == FLAME_ENOTSUP,
               "flame_agg_reduce_mixed aggregate");
        EXPECT(flame_agg_trimmed(code, 0, fake, 1, 1, cl, 3, 1, NULL) == FLAME_ENOTSUP, "flame_agg_trimmed");
        EXPECT(flame_scale_add_chunk_elems(code) == 0, "flame_scale_add_chunk_elems");
    }

    /* 4,000 randomized calls, every one with a defect picked at random on top of random (possibly
     * also invalid) other arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int cd = (next() & 1) ? E4 : E5, ad = F;
        unsigned flags = (next() & 1) ? FLAME_AGG_XCD_MAP : 0u;
        int32_t n_segs = (int32_t)(next() % 5) + 1;
        int32_t n_clients = 1 + (int32_t)(next() % 2000);
        int64_t n_chunks = (int64_t)(next() % 100000) + 1;
        const flame_segment *segs = fake;
        const void *const *c = cl, *const *b = bs;
        const float *rates = r, *scales = (next() & 1) ? sc : NULL;
        switch (next() % 10) {
        case 0: segs = NULL; break;
        case 1: n_segs = -(int32_t)(next() % 3); break;
        case 2: n_chunks = (next() & 1) ? -(int64_t)(next() % 1000) : 0x80000000ll + (int64_t)(next() % 1000); break;
        case 3: n_clients = -(int32_t)(next() % 1000); break;
        case 4: c = NULL; break;
        case 5: cd = (int)(next() % 10); break;
        case 6: ad = 1 + (int)(next() % 1000); break;
        case 7: flags |= (next() & 1) ? (1u + (unsigned)(next() % 3)) : (8u << (next() % 20)); break;
        case 8: b = NULL; break;
        default: rates = NULL; break;
        }
        int rc = flame_agg_reduce_mx(cd, ad, flags, segs, n_segs, n_chunks, c, b, n_clients, rates, scales, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_agg_reduce_mx refused");
        EXPECT(strstr(flame_last_error(), "flame_agg_reduce_mx") != NULL, "randomized flame_agg_reduce_mx message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("mx abi asan OK\n");
    return 0;
}
