/* Host sanitizer run of flame_agg_reduce_mxfp4: built against a copy of libflame_amd.so whose HOST
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
        EXPECT(strstr(flame_last_error(), "flame_agg_reduce_mxfp4") != NULL, #call " names the entry point"); \
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
    const int E2 = FLAME_FP4_E2M1, F = FLAME_F32;
    EXPECT(flame_launch_branches() == 100, "the launch-branch table is unchanged");
    EXPECT(flame_abi_version() == 1, "the ABI version is unchanged");
    EXPECT(E2 == 12, "the next free element code");
    EXPECT(flame_chunk_elems(E2) == 8192, "the chunk: one 4,096-byte tile of packed client bytes");
    EXPECT(flame_chunk_elems(FLAME_FP8_E4M3) == 4096 && flame_chunk_elems(13) == 0, "the other codes keep theirs");

    /* one defect per call: every (client, aggregate) pair but (12, f32) */
    const int codes[] = {FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64, FLAME_I64, FLAME_I32, FLAME_U8, FLAME_BOOL,
                         FLAME_FP8_E4M3, FLAME_FP8_E5M2, FLAME_FP4_E2M1, 13, 21, -1};
    const size_t n_codes = sizeof(codes) / sizeof(codes[0]);
    for (size_t i = 0; i < n_codes; ++i)
        for (size_t j = 0; j < n_codes; ++j) {
            if (codes[i] == E2 && codes[j] == F) continue;
            char a[32], b[32];
            snprintf(a, sizeof a, "client dtype %d", codes[i]);
            snprintf(b, sizeof b, "aggregate dtype %d", codes[j]);
            EXPECT_ERR(flame_agg_reduce_mxfp4(codes[i], codes[j], 0, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, a);
            EXPECT(strstr(flame_last_error(), b) != NULL, "the message names the aggregate dtype");
        }
    /* the tables and counts */
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, NULL, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 0, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, -2, 1, cl, bs, 3, r, sc, NULL), FLAME_EINVAL, "segment");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 0, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, -1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 0x80000000ll, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "n_chunks");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, NULL, bs, 3, r, NULL, NULL), FLAME_EINVAL, "client pointer");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, NULL, 3, r, NULL, NULL), FLAME_EINVAL, "block scale pointer");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, NULL, 3, r, sc, NULL), FLAME_EINVAL, "block scale pointer");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, bs, 0, r, NULL, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, bs, INT32_MIN, r, sc, NULL), FLAME_EINVAL, "n_clients");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, bs, 3, NULL, NULL, NULL), FLAME_EINVAL, "rate array");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0, fake, 1, 1, cl, bs, 3, NULL, sc, NULL), FLAME_EINVAL, "rate array");
    /* the flags */
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, FLAME_AGG_INIT_FIRST, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, "INIT_FIRST");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, FLAME_AGG_INIT_FIRST | FLAME_AGG_XCD_MAP, fake, 1, 1, cl, bs, 3, r, sc, NULL),
               FLAME_ENOTSUP, "INIT_FIRST");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, FLAME_AGG_SEG_RATES, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_ENOTSUP, "SEG_RATES");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 8u, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "unknown flags");
    EXPECT_ERR(flame_agg_reduce_mxfp4(E2, F, 0x80000000u, fake, 1, 1, cl, bs, 3, r, NULL, NULL), FLAME_EINVAL, "unknown flags");

    /* flame_agg_reduce_mx and the older reduce entry points refuse the new code as any unknown code */
    EXPECT(flame_agg_reduce_mx(E2, F, 0, fake, 1, 1, cl, bs, 3, r, NULL, NULL) == FLAME_ENOTSUP, "flame_agg_reduce_mx");
    EXPECT(strstr(flame_last_error(), "client dtype 12") != NULL, "flame_agg_reduce_mx names the code");
    EXPECT(flame_agg_reduce_mx(FLAME_FP8_E4M3, E2, 0, fake, 1, 1, cl, bs, 3, r, NULL, NULL) == FLAME_ENOTSUP, "flame_agg_reduce_mx aggregate");
    EXPECT(flame_agg_reduce(E2, 0, fake, 1, 1, cl, 3, r, (const double *)r, NULL) == FLAME_ENOTSUP, "flame_agg_reduce");
    EXPECT(flame_agg_reduce_scaled(E2, 0, fake, 1, 1, cl, 3, r, (const double *)r, sc, (const double *)sc, NULL) ==
               FLAME_ENOTSUP, "flame_agg_reduce_scaled");
    EXPECT(flame_agg_reduce_mixed(E2, F, 0, fake, 1, 1, cl, 3, r, NULL, NULL) == FLAME_ENOTSUP, "flame_agg_reduce_mixed");
    EXPECT(flame_agg_reduce_mixed(FLAME_BF16, E2, 0, fake, 1, 1, cl, 3, r, NULL, NULL) == FLAME_ENOTSUP,
           "flame_agg_reduce_mixed aggregate");
    EXPECT(flame_agg_trimmed(E2, 0, fake, 1, 1, cl, 3, 1, NULL) == FLAME_ENOTSUP, "flame_agg_trimmed");
    EXPECT(flame_scale_add_chunk_elems(E2) == 0, "flame_scale_add_chunk_elems");

    /* 4,000 randomized calls, every one with a defect picked at random on top of random (possibly
     * also invalid) other arguments: a nonzero status and a message, nothing launched */
    for (int it = 0; it < 4000; ++it) {
        int cd = E2, ad = F;
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
        case 5: cd = (int)(next() % 12); break;
        case 6: ad = 1 + (int)(next() % 1000); break;
        case 7: flags |= (next() & 1) ? (1u + (unsigned)(next() % 3)) : (8u << (next() % 20)); break;
        case 8: b = NULL; break;
        default: rates = NULL; break;
        }
        int rc = flame_agg_reduce_mxfp4(cd, ad, flags, segs, n_segs, n_chunks, c, b, n_clients, rates, scales, NULL);
        EXPECT(rc == FLAME_EINVAL || rc == FLAME_ENOTSUP, "randomized flame_agg_reduce_mxfp4 refused");
        EXPECT(strstr(flame_last_error(), "flame_agg_reduce_mxfp4") != NULL, "randomized flame_agg_reduce_mxfp4 message");
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("mxfp4 abi asan OK\n");
    return 0;
}
