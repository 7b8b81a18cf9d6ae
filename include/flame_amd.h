/*
 * flame_amd.h -- C ABI of the MI355X-native server-side aggregation path.
 *
 * Drop-in boundary for cisco-open/flame's lib/python data plane.  Each entry
 * point replaces one PyTorch op sequence in the reference (paths relative to
 * /root/reference/lib/python/flame/):
 *
 *   flame_agg_reduce            optimizer/fedavg.py:79-104   (FedAvg.do client loop +
 *                                                             _aggregate_pytorch)
 *                               optimizer/fedbuff.py:89-97,136-157 (FedBuff.do loop +
 *                                                             _aggregate_pytorch)
 *   flame_fedopt_reduce_adapt   optimizer/fedopt.py:80-90,102-129 (FedAvg.do + _adapt_pytorch)
 *                               + fedadam.py:33-35 / fedyogi.py:34-36 / fedadagrad.py:33-35
 *   flame_fedopt_reduce_adapt_f64, flame_fedopt_chain_f64
 *                               the same statements on float64 tensors (fp64 rates, unrounded
 *                               Python-float scalars), per round and per eager queue
 *   flame_fedbuff_scale_add    optimizer/fedbuff.py:101-127 (scale_add_agg_weights), fused with
 *                               common/util.py:152-159 (delta_weights_pytorch) as used by
 *                               mode/horizontal/asyncfl/middle_aggregator.py:221-226,246
 *   flame_hier_fedbuff          a node's co-located two-level FedBuff hierarchy in one pass
 *                               (FLAME_HIER_SYNC: the synchronous FedAvg hierarchy,
 *                               syncfl/middle_aggregator.py:163-229 -> syncfl/top_aggregator.py:122-176):
 *                               per middle optimizer/fedbuff.py:89-97,136-157 (None-start
 *                               arrivals) + :101-127 (scale_add) + the delta of
 *                               mode/horizontal/asyncfl/middle_aggregator.py:221-226,246,
 *                               fed to the top's FedBuff (asyncfl/top_aggregator.py:85-109)
 *   flame_feddyn_round          optimizer/feddyn.py:90-113,125-139 (FedDyn.do: add_to_hist,
 *                               FedAvg with rate 1/len(cache), mean of the histories, cld_model)
 *   flame_elementwise           the same statements for the keys the fused kernels do not take
 *                               (int and mixed-dtype keys; fp64 outside FedOPT): optimizer/fedopt.py:102-129,
 *                               scaffold.py:141-150, feddyn.py:90-113,125-139
 *   flame_update_stats          privacy/differential_privacy.py:68-76 (the update's total norm), as
 *                               per-update sums of squares and non-finite counts on the aggregator
 *   flame_update_dist           (no reference counterpart: squared distances to a centre for the
 *                               geometric median of Pillutla et al., IEEE TSP 2022, on the same pass)
 *   flame_agg_reduce_scaled     privacy/differential_privacy.py:79-82 (torch.mul(d_w, scale)) followed
 *                               by optimizer/fedavg.py:93-104, in one pass
 *   flame_agg_reduce_mixed      optimizer/fedavg.py:93-104 with bf16 / f16 updates into an fp32 model:
 *                               `tmp = v * rate` in v's dtype, `agg += tmp` in the promoted fp32
 *   flame_agg_reduce_mx         (no reference counterpart: MXFP8 updates -- OCP e4m3fn / e5m2 elements, one
 *                               E8M0 scale per 32 -- into an fp32 model; the same statements over the
 *                               dequantized update)
 *   flame_agg_reduce_mxfp4      (no reference counterpart: MXFP4 updates -- OCP e2m1 elements, two per byte,
 *                               one E8M0 scale per 32 -- into an fp32 model; the same statements again)
 *   flame_agg_trimmed           (no reference counterpart: the coordinate-wise trimmed mean / median
 *                               of Yin et al., ICML 2018, over the same tables)
 *   flame_agg_select            (no reference counterpart: the same trimmed mean / median for any
 *                               trim count, by radix selection)
 *   flame_noise_fill            privacy/differential_privacy.py:55-61 (torch.normal(0, noise_factor)),
 *                               drawn once per round on the aggregator: Philox4x32-10 + Box-Muller
 *   flame_synth_fill            (bench/test plumbing: counter-based synthetic updates)
 *   flame_hier_resident_per_cu  (no reference counterpart: occupancy query the parameter
 *                               shard uses to size its waves, flame_amd/shard.py)
 *
 * Conventions
 *   - All pointers passed to the compute entry points are DEVICE pointers
 *     (HBM of the current HIP device) unless stated otherwise; `stream` is a
 *     hipStream_t (NULL = default stream).  Calls are asynchronous on `stream`.
 *   - Per element, clients are combined strictly in the order given (the
 *     reference's cache.iterkeys() order); each reference op is one IEEE
 *     round-to-nearest-even rounding in the tensor's dtype (no FMA), so results
 *     are bit-identical to the reference's torch-CPU arithmetic for
 *     FedAvg/FedBuff.  Only FedOPT's sqrt differs (torch-CPU's fp32 sqrt is not
 *     correctly rounded; ours is).
 *   - Return value: FLAME_OK (0) or a nonzero FLAME_E* status; the message is
 *     available from flame_last_error() (thread-local).  Nothing aborts.
 */
#ifndef FLAME_AMD_H
#define FLAME_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLAME_ABI_VERSION 1

/* status codes */
#define FLAME_OK 0
#define FLAME_EINVAL 1   /* bad argument (message in flame_last_error) */
#define FLAME_EHIP 2     /* HIP runtime error (launch / device) */
#define FLAME_ENOTSUP 3  /* dtype / variant not supported by this entry point */

/* element types (torch dtypes of the reference state_dict tensors) */
#define FLAME_F32 0
#define FLAME_BF16 1
#define FLAME_F16 2
#define FLAME_F64 3
#define FLAME_I64 4
#define FLAME_I32 5
/* 6 .. 9 are the element types only flame_elementwise takes (FLAME_U8 .. FLAME_BOOL, below).
 * MXFP8 client elements (OCP Microscaling v1.0), taken by flame_agg_reduce_mx alone: every other
 * entry point refuses them as it refuses an unknown code */
#define FLAME_FP8_E4M3 10 /* OCP e4m3fn: torch.float8_e4m3fn */
#define FLAME_FP8_E5M2 11 /* OCP e5m2:   torch.float8_e5m2 */
/* the MXFP4 client element, two per byte, taken by flame_agg_reduce_mxfp4 alone */
#define FLAME_FP4_E2M1 12 /* OCP e2m1:   torch.float4_e2m1fn_x2 (one byte = two elements) */

/* flame_agg_reduce flags */
#define FLAME_AGG_INIT_FIRST 1u  /* no base: acc = tmp(client 0) (fedbuff.py:139-140,154-155) */
#define FLAME_AGG_SEG_RATES 2u   /* rates are [n_segs][n_clients]: one rate row per segment
                                    (independent reductions -- e.g. the middle aggregators of
                                    a node, asyncfl/middle_aggregator.py:164-256 -- in one launch) */
#define FLAME_AGG_XCD_MAP 4u     /* workgroups take chunks XCD by XCD (each of the 8 XCDs, which get
                                    workgroups round-robin, streams one contiguous eighth of the
                                    chunks): faster when every client is its own tensor (rows),
                                    slower for a tiled UpdateSlab; results are identical */

/* flame_fedopt_reduce_adapt variants and flags */
#define FLAME_FEDADAM 0
#define FLAME_FEDYOGI 1
#define FLAME_FEDADAGRAD 2
#define FLAME_OPT_STATE_ZERO 1u  /* m_t, v_t were None: treat as zeros, do not read (fedopt.py:108-122) */
#define FLAME_OPT_XCD_MAP 2u     /* as FLAME_AGG_XCD_MAP, for flame_fedopt_reduce_adapt */

/* per-segment flag (flame_segment.flags) */
#define FLAME_SEG_UNALIGNED 1    /* some pointer of this segment is not 16-byte aligned */
#define FLAME_SEG_CUR_IS_AVG 2   /* flame_fedopt_reduce_adapt: `cur` IS the FedAvg result (the eager
                                    caller's current_weights alias base_weights after the round-1
                                    passthrough, eager_syncfl/top_aggregator.py:42,75 +
                                    fedopt.py:87-88): cur takes the reduced value, d = avg - avg;
                                    seg.cur is not read */

/*
 * One contiguous run of elements (typically one state_dict tensor, or one
 * dtype group of a flattened model).  Field roles by entry point:
 *
 *                 flame_agg_reduce     flame_fedopt_reduce_adapt   flame_fedbuff_scale_add
 *   out           aggregate (out)      FedAvg result (out, opt.)   base weights (in/out)
 *   in            base (in; may ==out) base weights (in)           agg_goal_weights (in)
 *   cur           -                    current weights (in)        -
 *   cur_out       -                    new current weights (out)   delta = new-old (out, opt.)
 *   m, v          -                    m_t, v_t (in/out)           -
 *
 * chunk_begin is the prefix sum over previous segments of
 * ceil(numel / flame_chunk_elems(dtype)); the grid covers n_chunks chunks.
 * client_tile_stride (reduce entry points only): 0 = every client's data for
 * the segment is contiguous; otherwise client data is TILED -- chunk c of a
 * client starts client_tile_stride bytes after chunk c-1 (e.g. a [chunks][N][chunk]
 * slab, where one workgroup reads one contiguous N x chunk region).
 * The table lives in device memory.
 */
typedef struct flame_segment {
    void *out;
    const void *in;
    const void *cur;
    void *cur_out;
    void *m;
    void *v;
    int64_t numel;
    int64_t chunk_begin;
    int64_t flags;
    int64_t client_tile_stride;
} flame_segment;

/* Library info. */
int flame_abi_version(void);
const char *flame_last_error(void);
/* Elements one workgroup covers per segment chunk for `dtype` (0 if invalid). */
int64_t flame_chunk_elems(int dtype);
/* Elements per chunk for the elementwise scale-add kernel. */
int64_t flame_scale_add_chunk_elems(int dtype);

/*
 * Weighted client reduction (FedAvg / FedBuff accumulate).
 *   clients : device array [n_segs][n_clients] of device pointers; row s holds,
 *             in iteration order, each client's data for segment s.
 *   rates32 : device [n_clients] fp32 rates (float(count/total) or
 *             float(1/sqrt(1+version-tres.version))), used for every dtype but f64.
 *   rates64 : device [n_clients] fp64 rates, used for FLAME_F64 (may be NULL otherwise).
 *             With FLAME_AGG_SEG_RATES both are [n_segs][n_clients] and segment s uses row s.
 * Per element e of each segment:
 *   acc = in[e] (or tmp_0 with FLAME_AGG_INIT_FIRST);
 *   for i: tmp = round(v_i[e] * rate_i) (ints: trunc(float(v)*rate)); acc = round(acc + tmp)
 *   out[e] = acc.
 */
int flame_agg_reduce(int dtype, unsigned flags, const flame_segment *segs, int32_t n_segs,
                     int64_t n_chunks, const void *const *clients, int32_t n_clients,
                     const float *rates32, const double *rates64, void *stream);

/*
 * flame_agg_reduce for small launches: the same metadata block (segments, then the client
 * pointer table and the rates, at byte offsets off_clients / off_r32 / off_r64 -- pass -1 for
 * the rate array the dtype does not use) is passed from HOST memory and travels to the GPU as
 * a kernel argument, so no H2D copy (a blit kernel on gfx950, ≈15 µs of GPU timeline per
 * launch) precedes the reduction.  meta_bytes <= flame_agg_argmeta_max_bytes() (3,584).
 * Semantics, flags and dtypes as flame_agg_reduce; the client and segment pointers inside
 * the block are device pointers as there.
 */
int flame_agg_reduce_argmeta(int dtype, unsigned flags, const void *host_meta, int64_t meta_bytes,
                             int32_t n_segs, int64_t n_chunks, int32_t n_clients, int64_t off_clients,
                             int64_t off_r32, int64_t off_r64, void *stream);
int64_t flame_agg_argmeta_max_bytes(void);

/*
 * Server-side update guard, part 1: per-update statistics.  Restates the norm of
 * privacy/differential_privacy.py:68-76 (torch.norm of every tensor's norm = the square root of
 * the sum of squares of all elements) on the aggregator, over the updates it actually received.
 *   segs, clients : the tables flame_agg_reduce takes; only numel, chunk_begin, flags
 *                   (FLAME_SEG_UNALIGNED) and client_tile_stride of a segment are read, so one
 *                   launch covers tensors, tiled UpdateSlab slots and misaligned views alike.
 *   sumsq         : device double [n_clients];  sumsq[i] += sum of x*x over client i's FINITE
 *                   elements of every segment (each x widened to fp64 first, every add in fp64).
 *   nonfinite     : device int64 [n_clients];   nonfinite[i] += number of NaN / +-inf elements
 *                   (they add nothing to sumsq).
 *   scratch       : device buffer of >= flame_update_stats_scratch_bytes(n_chunks, n_clients)
 *                   bytes (scratch_bytes: its size), overwritten.
 * Both outputs are accumulated into: zero them, then launch once per dtype of a model on one
 * stream.  No floating-point atomics: partial sums are combined in a fixed order, so the same
 * launch on the same data gives the same bits.  dtype FLAME_F32, FLAME_BF16, FLAME_F16 or
 * FLAME_F64 (integer dtypes: FLAME_ENOTSUP); n_clients >= 1.  Not a launch branch of
 * flame_launch_branches() (one instantiation per dtype).
 */
int flame_update_stats(int dtype, const flame_segment *segs, int32_t n_segs, int64_t n_chunks,
                       const void *const *clients, int32_t n_clients, double *sumsq, int64_t *nonfinite,
                       void *scratch, int64_t scratch_bytes, void *stream);
int64_t flame_update_stats_scratch_bytes(int64_t n_chunks, int32_t n_clients);

/*
 * Squared distances of a round's updates to a centre: what the smoothed Weiszfeld iterations of
 * the geometric median (RFA: Pillutla, Kakade, Harchaoui, "Robust Aggregation for Federated
 * Learning", IEEE Transactions on Signal Processing 70, 2022) need of the device.  flame has no
 * counterpart file.  It is flame_update_stats' pass with one subtraction per element.
 *   segs, clients : the tables flame_update_stats takes; besides numel, chunk_begin, flags and
 *                   client_tile_stride, each segment's `in` is read: the centre z of that segment,
 *                   numel contiguous elements of the segment's dtype.  FLAME_SEG_UNALIGNED on a
 *                   segment: its client views AND its centre are read element by element;
 *                   otherwise `in` is 16-byte aligned.
 *   dist2         : device double [n_clients];  dist2[i] += sum over every element e of every segment
 *                   of t(e):  t = 0 when x_i[e] is NaN or +-inf (whatever z[e] is); otherwise
 *                   d = fp64(x_i[e]) - fp64(z[e]) (one IEEE fp64 subtract), t = d * d, squared and
 *                   added as flame_update_stats does for the dtype (f32 / bf16 / f16: one fma;
 *                   f64: the square rounds, then the add).  A non-finite z[e] propagates by IEEE
 *                   arithmetic: dist2[i] becomes +inf or NaN.
 *   nonfinite     : device int64 [n_clients];  nonfinite[i] += number of NaN / +-inf elements of
 *                   x_i (non-finite centre elements are not counted).
 *   scratch       : device buffer of >= flame_update_dist_scratch_bytes(n_chunks, n_clients) bytes
 *                   (scratch_bytes: its size), overwritten.
 * With an all-zero centre (+0 or -0) dist2 is flame_update_stats' sumsq bit for bit and nonfinite
 * is equal: the two are one kernel template.  Both outputs are accumulated into: zero them, then
 * launch once per float dtype of a model on one stream.  No floating-point atomics: partial sums
 * are combined in a fixed order, so the same launch on the same data gives the same bits.  dtype
 * FLAME_F32, FLAME_BF16, FLAME_F16 or FLAME_F64 (integer dtypes: FLAME_ENOTSUP); n_clients >= 1,
 * no upper limit.  Not a launch branch of flame_launch_branches().
 */
int flame_update_dist(int dtype, const flame_segment *segs, int32_t n_segs, int64_t n_chunks,
                      const void *const *clients, int32_t n_clients, double *dist2, int64_t *nonfinite,
                      void *scratch, int64_t scratch_bytes, void *stream);
int64_t flame_update_dist_scratch_bytes(int64_t n_chunks, int32_t n_clients);

/*
 * Pairwise Gram matrix of a round's updates: what Krum / Multi-Krum (Blanchard, El Mhamdi,
 * Guerraoui, Stainer: "Machine Learning with Adversaries: Byzantine Tolerant Gradient Descent",
 * NeurIPS 2017) needs of the device.  flame has no counterpart file.
 *   segs, clients : the tables flame_update_stats takes; only numel, chunk_begin, flags
 *                   (FLAME_SEG_UNALIGNED) and client_tile_stride of a segment are read, so one
 *                   launch covers tensors, tiled UpdateSlab slots and misaligned views alike.
 *   gram          : device double [n_clients][n_clients];  gram[i][j] += sum over every element e
 *                   of every segment of s(x_i[e]) * s(x_j[e]), where s(x) is x widened to fp64 if x
 *                   is finite, else 0.0 -- flame_update_stats' sanitising, so gram[i][i] is its
 *                   sumsq[i] up to summation order.  Products of f32 / bf16 / f16 values are exact
 *                   in fp64; the accumulation (v_mfma_f64_16x16x4_f64, then fp64 adds) is the only
 *                   rounding: |error| <= (elements + 1) * 2^-53 * sum |x_i x_j| (f64 keys: + 2, one
 *                   more rounding per product).  Both triangles are written and are bitwise equal.
 *   nonfinite     : device int64 [n_clients];  nonfinite[i] += number of NaN / +-inf elements.
 *   scratch       : device buffer of >= flame_update_gram_scratch_bytes(n_chunks, n_clients) bytes
 *                   (scratch_bytes: its size), overwritten.  At most 1 GiB for every n_clients <=
 *                   1024 at any n_chunks (the chunk range of a workgroup grows with both).
 * Both outputs are accumulated into: zero them, then launch once per float dtype of a model on one
 * stream.  No floating-point atomics: partial sums are combined in a fixed order, so the same
 * launch on the same data gives the same bits.  dtype FLAME_F32, FLAME_BF16, FLAME_F16 or
 * FLAME_F64 (integer dtypes: FLAME_ENOTSUP); 1 <= n_clients <= flame_update_gram_max_clients()
 * (1024; more: FLAME_ENOTSUP).  Not a launch branch of flame_launch_branches().
 */
int flame_update_gram(int dtype, const flame_segment *segs, int32_t n_segs, int64_t n_chunks,
                      const void *const *clients, int32_t n_clients, double *gram, int64_t *nonfinite,
                      void *scratch, int64_t scratch_bytes, void *stream);
int64_t flame_update_gram_scratch_bytes(int64_t n_chunks, int32_t n_clients);
int flame_update_gram_max_clients(void);

/*
 * Server-side update guard, part 2: flame_agg_reduce with a per-client clip scale.
 *   scales32 : device [n_clients] fp32 scales (f32 / bf16 / f16); scales64: device [n_clients]
 *              fp64 scales (FLAME_F64; either may be NULL when the dtype does not use it).
 * Per element, clients in order, every op rounded once in the tensor's dtype:
 *   t1  = round(v_i[e] * scale_i)     torch.mul(d_w, scale), differential_privacy.py:79-82
 *   tmp = round(t1 * rate_i)          fedavg.py:93-104
 *   acc = round(acc + tmp)
 * scale_i == 1 reproduces flame_agg_reduce bit for bit.  Float dtypes only (FLAME_ENOTSUP
 * otherwise); flags FLAME_AGG_INIT_FIRST and FLAME_AGG_XCD_MAP (FLAME_AGG_SEG_RATES:
 * FLAME_ENOTSUP); device tables only.  Not a launch branch of flame_launch_branches().
 */
int flame_agg_reduce_scaled(int dtype, unsigned flags, const flame_segment *segs, int32_t n_segs,
                            int64_t n_chunks, const void *const *clients, int32_t n_clients,
                            const float *rates32, const double *rates64, const float *scales32,
                            const double *scales64, void *stream);

/*
 * 16-bit updates into an fp32 aggregate in one launch (optimizer/fedavg.py:93-104 when a trainer
 * sends bf16 / f16 deltas to an fp32 server model: `tmp = (v * rate)` stays in v's dtype, torch
 * computes `agg += tmp` in the promoted dtype; with scales32 the clipped round's
 * torch.mul(d_w, scale) of differential_privacy.py:79-82 comes first, as in flame_agg_reduce_scaled).
 *   client_dtype : C, FLAME_BF16 or FLAME_F16: every client tensor of every segment.
 *   agg_dtype    : FLAME_F32: every segment's in / out.
 *   segs         : chunk_begin counts chunks of flame_chunk_elems(client_dtype) = 2,048 elements
 *                  (one 4,096-byte slab tile); client_tile_stride is in client bytes.
 *   rates32      : device [n_clients]; scales32: device [n_clients], or NULL for the plain round.
 * Per element e, clients in order, no FMA:
 *   acc = in[e]                                                  (fp32)
 *   t   = round_C(f32(v_i[e]) * rate_i)
 *         with scales32: t = round_C(f32(round_C(f32(v_i[e]) * scale_i)) * rate_i)
 *   acc = round_f32(acc + f32(t))
 *   out[e] = acc
 * scale_i == 1 reproduces the plain round bit for bit.  Refusals, each before any HIP call and
 * named in flame_last_error: a pair other than (bf16 | f16, f32) is FLAME_ENOTSUP (the message
 * names both dtypes); FLAME_AGG_INIT_FIRST is FLAME_ENOTSUP (a None-start aggregate takes the
 * update's dtype in the reference, so there is no statement to restate); FLAME_AGG_SEG_RATES is
 * FLAME_ENOTSUP; any flag beyond FLAME_AGG_XCD_MAP, a NULL table or rate array, n_segs <= 0,
 * n_clients < 1 or n_chunks outside [1, 2^31) is FLAME_EINVAL.  Device tables only (no
 * kernel-argument variant).  Not a launch branch of flame_launch_branches().
 */
int flame_agg_reduce_mixed(int client_dtype, int agg_dtype, unsigned flags, const flame_segment *segs,
                           int32_t n_segs, int64_t n_chunks, const void *const *clients,
                           int32_t n_clients, const float *rates32, const float *scales32, void *stream);

/*
 * MXFP8 updates into an fp32 aggregate in one launch.  flame has no counterpart: the contract is this
 * project's own.  An update holds, per tensor, one OCP e4m3fn or e5m2 byte per element
 * and one E8M0 scale byte per block of 32 flat C-order elements (the last block may be partial), as
 * flame_amd.mx.quantize writes them.  The arguments are flame_agg_reduce_mixed's plus block_scales.
 *   client_dtype : FLAME_FP8_E4M3 or FLAME_FP8_E5M2: every client tensor of every segment.
 *   agg_dtype    : FLAME_F32: every segment's in / out.
 *   segs         : chunk_begin counts chunks of flame_chunk_elems(client_dtype) = 4,096 elements (one
 *                  4,096-byte tile: a lane owns 16 elements, half a block).  client_tile_stride must
 *                  be 0: the engine never builds a tiled MX row, and the kernel does not read the field.
 *   clients      : device array [n_segs][n_clients] of pointers to the element bytes.
 *   block_scales : device array [n_segs][n_clients] of pointers to the scale bytes,
 *                  ceil(numel / 32) each, of ANY alignment (FLAME_SEG_UNALIGNED does not speak of them);
 *                  device addresses or translated pinned-host addresses, as client rows are.
 *   rates32      : device [n_clients]; scales32: device [n_clients] clip scales, or NULL for the plain round.
 * Per element e, clients in order, no FMA:
 *   acc = in[e]                                                  (fp32)
 *   x   = f32(q_i[e]) * f32_e8m0(s_i[e / 32])                    one IEEE fp32 multiply, denormals kept;
 *         f32_e8m0(b) = 2^(b - 127) (b = 0: the fp32 subnormal 2^-127); a NaN element or scale byte 255
 *         gives NaN
 *         with scales32: x = round_f32(x * scale_i)
 *   t   = round_f32(x * rate_i)
 *   acc = round_f32(acc + t)
 *   out[e] = acc
 * x is flame_amd.mx.dequantize's value of the element, so the result is bit for bit what
 * flame_agg_reduce (with scales32: flame_agg_reduce_scaled) gives for FLAME_F32 over the
 * dequantized update.  Refusals, each before any HIP call and named in flame_last_error: a pair other
 * than (e4m3 | e5m2, f32) is FLAME_ENOTSUP (the message names both dtypes); FLAME_AGG_INIT_FIRST is
 * FLAME_ENOTSUP; FLAME_AGG_SEG_RATES is FLAME_ENOTSUP; any flag beyond FLAME_AGG_XCD_MAP, a NULL
 * table or rate array, n_segs <= 0, n_clients < 1 or n_chunks outside [1, 2^31) is FLAME_EINVAL.
 * Device tables only (no kernel-argument variant).  Not a launch branch of flame_launch_branches().
 */
int flame_agg_reduce_mx(int client_dtype, int agg_dtype, unsigned flags, const flame_segment *segs,
                        int32_t n_segs, int64_t n_chunks, const void *const *clients,
                        const void *const *block_scales, int32_t n_clients, const float *rates32,
                        const float *scales32, void *stream);

/*
 * MXFP4 updates into an fp32 aggregate in one launch (OCP Microscaling v1.0; the contract is this
 * project's own).  An update holds, per tensor, one 4-bit OCP e2m1 code per element and
 * one E8M0 scale byte per block of 32 flat C-order elements (16 bytes; the last block may be partial),
 * as flame_amd.mx.quantize(fmt="e2m1") writes them.
 *   Elements: 1 sign bit, 2 exponent bits, 1 mantissa bit.  Codes 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6;
 *             codes 8 .. 15 their negatives (code 8 is -0).  No inf, no NaN.
 *   Packing : two elements per byte: flat element 2i is the LOW nibble of byte i, element 2i + 1 the
 *             HIGH nibble (torch.float4_e2m1fn_x2's and the hardware's order).  A client pointer
 *             addresses ceil(numel / 2) bytes; with odd numel the last high nibble is padding, which
 *             the kernel never reads a meaning from (nothing after byte ceil(numel / 2) - 1 is read).
 * The arguments are flame_agg_reduce_mx's.
 *   client_dtype : FLAME_FP4_E2M1: every client tensor of every segment.
 *   agg_dtype    : FLAME_F32: every segment's in / out.
 *   segs         : chunk_begin counts chunks of flame_chunk_elems(FLAME_FP4_E2M1) = 8,192 elements (one
 *                  4,096-byte tile of client bytes: a lane owns 32 elements, one whole scale block).
 *                  client_tile_stride must be 0: a tiled MXFP4 row is refused where rows are built
 *                  (flame_amd/engine.py; the table is device memory, this entry point cannot look), and
 *                  the kernel does not read the field.  FLAME_SEG_UNALIGNED speaks of in, out and the
 *                  client byte pointers.
 *   clients      : device array [n_segs][n_clients] of pointers to the packed element bytes, of any
 *                  alignment under FLAME_SEG_UNALIGNED.
 *   block_scales : device array [n_segs][n_clients] of pointers to the scale bytes,
 *                  ceil(numel / 32) each, of ANY alignment (FLAME_SEG_UNALIGNED does not speak of them).
 *   rates32      : device [n_clients]; scales32: device [n_clients] clip scales, or NULL for the plain round.
 * Per element e, clients in order, no FMA, denormals kept:
 *   acc = in[e]                                                  (fp32)
 *   b   = q_i[e >> 1];  c = (e & 1) ? b >> 4 : b & 15
 *   x   = f32_e2m1(c) * f32_e8m0(s_i[e / 32])                    one IEEE fp32 multiply;
 *         f32_e8m0(b) = 2^(b - 127) (b = 0: the fp32 subnormal 2^-127); scale byte 255 gives NaN
 *         for every element of its block (the one way an MXFP4 update carries a NaN)
 *         with scales32: x = round_f32(x * scale_i)
 *   t   = round_f32(x * rate_i)
 *   acc = round_f32(acc + t)
 *   out[e] = acc
 * x is flame_amd.mx.dequantize's value of the element, so the result is bit for bit what
 * flame_agg_reduce (with scales32: flame_agg_reduce_scaled) gives for FLAME_F32 over the
 * dequantized update.  Refusals, each before any HIP call and named in flame_last_error: a pair other
 * than (e2m1, f32) is FLAME_ENOTSUP (the message names both dtypes); FLAME_AGG_INIT_FIRST is
 * FLAME_ENOTSUP; FLAME_AGG_SEG_RATES is FLAME_ENOTSUP; any flag beyond FLAME_AGG_XCD_MAP, a NULL
 * table or rate array, n_segs <= 0, n_clients < 1 or n_chunks outside [1, 2^31) is FLAME_EINVAL.
 * Device tables only (no kernel-argument variant).  Not a launch branch of flame_launch_branches().
 */
int flame_agg_reduce_mxfp4(int client_dtype, int agg_dtype, unsigned flags, const flame_segment *segs,
                           int32_t n_segs, int64_t n_chunks, const void *const *clients,
                           const void *const *block_scales, int32_t n_clients, const float *rates32,
                           const float *scales32, void *stream);

/*
 * Coordinate-wise trimmed mean and, at its limit, the coordinate-wise median (Yin, Chen,
 * Ramchandran, Bartlett: "Byzantine-Robust Distributed Learning: Towards Optimal Statistical
 * Rates", ICML 2018).  flame has no counterpart file: its optimizers only average.
 *   segs, clients : the tables flame_agg_reduce takes (tensors, tiled UpdateSlab slots, misaligned
 *                   views); no rates -- a weighted trimmed mean would let a liar choose its weight.
 *   trim_k        : values dropped at EACH end per element; 0 <= trim_k <= flame_agg_trimmed_max_k()
 *                   (16) and n_clients > 2 * trim_k.  trim_k = (n_clients - 1) / 2 is the median
 *                   (one value kept for odd n_clients, the mean of two for even).
 * Per element e, with x_i = v_i[e] in client order:
 *   order   -inf < .. < -0 < +0 < .. < +inf < NaN (all NaNs equal and largest, as torch.sort
 *           places them), compared on monotone integer keys, never by floating-point min / max;
 *   select  streaming in client order: `lo` keeps the trim_k smallest values seen so far, `hi` the
 *           trim_k largest of those that left `lo`; a value that leaves `hi` is kept.  The
 *           n_clients - 2 * trim_k kept values are the multiset sorted(x)[trim_k : n - trim_k];
 *   sum     each kept value widened to fp64 (exact for f32 / bf16 / f16) and added, one IEEE fp64 add
 *           each, to an accumulator that starts at +0.0, in the order the values emerge -- a
 *           function of the values and the client order only, never of the launch geometry;
 *   mean    acc / double(n_clients - 2 * trim_k), one fp64 division, rounded to the dtype (f64: as
 *           is; f32: one RNE step; bf16 / f16: two, fp64 -> fp32 -> 16 bit);
 *   out[e] = round(in[e] + mean), one add in the dtype (torch-CPU's `base += mean`); with
 *           FLAME_AGG_INIT_FIRST out[e] = mean and `in` is not read.
 * Up to trim_k NaN / +inf / -inf values per element therefore vanish; more of them on one side
 * propagate as IEEE arithmetic says.  trim_k = 0 is the unweighted mean accumulated in fp64.
 * No floating-point atomics: equal launches give equal bits.  Float dtypes only (FLAME_ENOTSUP
 * otherwise); flags FLAME_AGG_INIT_FIRST and FLAME_AGG_XCD_MAP (FLAME_AGG_SEG_RATES: FLAME_ENOTSUP);
 * device tables only.  Not a launch branch of flame_launch_branches().
 */
int flame_agg_trimmed(int dtype, unsigned flags, const flame_segment *segs, int32_t n_segs,
                      int64_t n_chunks, const void *const *clients, int32_t n_clients, int32_t trim_k,
                      void *stream);
int flame_agg_trimmed_max_k(void);

/*
 * The same trimmed mean / median for ANY trim_k, by radix selection instead of register chains
 * (DESIGN.md §2 and §4).  Tables, flags, dtypes and refusals as flame_agg_trimmed.
 *   trim_k    : 0 <= trim_k and n_clients > 2 * trim_k (FLAME_EINVAL otherwise); no cap.
 *   n_clients : at most flame_agg_select_max_clients() (65,535: the kernel counts in 16 bits);
 *               more is FLAME_ENOTSUP.
 * Per element e, with x_i = v_i[e] in client order, on the keys and the order of flame_agg_trimmed
 * (every NaN the all-ones key, -0 < +0); s = sorted(keys), k = trim_k, n = n_clients:
 *   select  lo = s[k] and hi = s[n - k - 1], found by an MSB-first radix search on the keys;
 *           c_lo = #{key <= lo} - k and c_hi = #{key >= hi} - k (both >= 1); if lo == hi,
 *           c_lo = n - 2k and there is no hi term;
 *   sum     acc starts at +0.0; for i in client order, if lo < key_i < hi: acc += widen(x_i), one
 *           IEEE fp64 add each; then acc += double(c_lo) * widen(value(lo)) and, if lo != hi,
 *           acc += double(c_hi) * widen(value(hi)): one fp64 multiply, then one fp64 add, no fma.
 *           value(all-ones key) is the quiet NaN 0x7f..f.  The kept multiset is
 *           sorted(x)[k : n - k] as for flame_agg_trimmed; the ORDER of the adds differs from the
 *           chains', so the two entry points can differ in the last bit (they agree bit for bit
 *           whenever the fp64 sum is exact).  A function of the values and the client order only,
 *           never of the launch geometry;
 *   mean, out[e] : as flame_agg_trimmed.
 * No floating-point atomics: equal launches give equal bits.  Float dtypes only (FLAME_ENOTSUP
 * otherwise); flags FLAME_AGG_INIT_FIRST and FLAME_AGG_XCD_MAP (FLAME_AGG_SEG_RATES: FLAME_ENOTSUP);
 * device tables only.  Not a launch branch of flame_launch_branches().
 */
int flame_agg_select(int dtype, unsigned flags, const flame_segment *segs, int32_t n_segs,
                     int64_t n_chunks, const void *const *clients, int32_t n_clients, int32_t trim_k,
                     void *stream);
int flame_agg_select_max_clients(void);

/*
 * Fused FedAvg + FedOPT adaptive step (dtype FLAME_F32, FLAME_BF16 or FLAME_F16; base,
 * cur, m, v, outputs and clients all of that dtype).  After the reduction above (avg kept
 * in registers, optionally written to seg.out), per element, every op rounded in dtype:
 *   d = avg - cur; m = b1*m + omb1*d;
 *   Adam: v = b2*v + omb2*(d*d);  Yogi: v = v - omb2*(d*d)*sign(v - d*d);  AdaGrad: v = v + d*d
 *   cur_out = cur + (eta*m) / (sqrt(v) + tau)
 * (a segment flagged FLAME_SEG_CUR_IS_AVG takes cur = avg, as the reference does when
 * current_weights and base_weights are one object).
 * Scalars are the roundings torch applies to the Python floats: b1 = f32(beta_1),
 * omb1 = f32(1 - beta_1), b2 = f32(beta_2), omb2 = f32(1 - beta_2), eta = f32(eta),
 * tau = f32(tau) for fp32 but dtype(tau) for bf16/fp16 (torch-CPU rounds a scalar to a
 * reduced-precision tensor's dtype before + / -).
 */
int flame_fedopt_reduce_adapt(int dtype, int variant, unsigned flags, const flame_segment *segs,
                              int32_t n_segs, int64_t n_chunks, const void *const *clients,
                              int32_t n_clients, const float *rates32, float b1, float omb1,
                              float b2, float omb2, float eta, float tau, void *stream);

/*
 * Eager FedOPT chain (FLAME_F32, FLAME_BF16 or FLAME_F16; every tensor of a segment of that
 * dtype, scalars as for flame_fedopt_reduce_adapt): the eager top aggregator's per-arrival do() calls
 * (eager_syncfl/top_aggregator.py:36-90, fedavg.py:93-104 then fedopt.py:102-129), queued and
 * run in one pass.  Per element, for each client i in order: base = base + round(w_i * r_i);
 * where step_end[i] != 0 (device array, one byte per client; client i closes a do() call) the
 * adaptive step of flame_fedopt_reduce_adapt with avg = base and the running current (the
 * first step of a segment flagged FLAME_SEG_CUR_IS_AVG takes cur = base).  Writes base to
 * seg.out, m and v in place, the final current to seg.cur_out (seg.cur is read unless the
 * segment is flagged).  FLAME_OPT_STATE_ZERO: m, v start as zeros and are not read.  Bitwise
 * equal to one flame_fedopt_reduce_adapt launch per do() call.  Replaces, per round,
 * optimizer/fedopt.py:80-90,102-129 as the eager role calls it.
 */
int flame_fedopt_chain(int dtype, int variant, unsigned flags, const flame_segment *segs, int32_t n_segs,
                       int64_t n_chunks, const void *const *clients, int32_t n_clients,
                       const float *rates32, const uint8_t *step_end, float b1, float omb1, float b2,
                       float omb2, float eta, float tau, void *stream);

/*
 * flame_fedopt_reduce_adapt with its metadata block (segments, then the [n_segs][n_clients]
 * client table at byte offset off_clients, then the fp32 rates at off_r32; at most
 * flame_agg_argmeta_max_bytes() bytes, host memory) passed as a kernel argument: no
 * device table and no H2D copy before the launch.  Small rounds only (e.g. flame's MNIST
 * model x a few trainers).  Replaces the same reference code as flame_fedopt_reduce_adapt
 * (optimizer/fedopt.py:80-90,102-129).  FLAME_EINVAL if a table lies outside the block.
 */
int flame_fedopt_reduce_adapt_argmeta(int dtype, int variant, unsigned flags, const void *host_meta,
                                      int64_t meta_bytes, int32_t n_segs, int64_t n_chunks,
                                      int32_t n_clients, int64_t off_clients, int64_t off_r32,
                                      float b1, float omb1, float b2, float omb2, float eta,
                                      float tau, void *stream);

/*
 * flame_fedopt_reduce_adapt for FLAME_F64 segments (base, cur, m, v, outputs and clients all
 * fp64; chunk_begin counts flame_chunk_elems(FLAME_F64) chunks): one launch per round for all
 * fp64 keys.  Per element the clients are reduced in order with the fp64 rates,
 * acc = round(acc + round(w_i * rates64[i])) as flame_agg_reduce does for FLAME_F64, then
 *   d = avg - cur; m = b1*m + omb1*d;
 *   Adam: v = b2*v + omb2*(d*d);  Yogi: v = v - (omb2*(d*d))*sign(v - d*d);  AdaGrad: v = v + d*d
 *   cur_out = cur + (eta*m) / (sqrt(v) + tau)
 * with every op one IEEE fp64 rounding (no FMA, denormals kept, sqrt and divide correctly
 * rounded, sign as torch.sign: NaN and +-0 give 0), and avg (if seg.out), m, v, cur_out stored.
 * Scalars are the Python floats themselves, not their fp32 roundings: torch multiplies an fp64
 * tensor by a Python scalar in double (b1 = beta_1, omb1 = 1 - beta_1, b2 = beta_2,
 * omb2 = 1 - beta_2, eta, tau).  Flags and FLAME_SEG_CUR_IS_AVG as flame_fedopt_reduce_adapt.
 * Replaces optimizer/fedopt.py:80-90,102-129 + fedadam.py:33-35 / fedyogi.py:34-36 /
 * fedadagrad.py:33-35 on float64 tensors; bitwise equal to flame_agg_reduce followed by the
 * same statements through flame_elementwise.
 */
int flame_fedopt_reduce_adapt_f64(int variant, unsigned flags, const flame_segment *segs, int32_t n_segs,
                                  int64_t n_chunks, const void *const *clients, int32_t n_clients,
                                  const double *rates64, double b1, double omb1, double b2, double omb2,
                                  double eta, double tau, void *stream);

/*
 * flame_fedopt_chain for FLAME_F64 segments (fp64 rates, scalars as for
 * flame_fedopt_reduce_adapt_f64): per element, for each client i in order
 * base = base + round(w_i * rates64[i]); where step_end[i] != 0 the adaptive step of
 * flame_fedopt_reduce_adapt_f64 with avg = base and the running current (the first step of a
 * segment flagged FLAME_SEG_CUR_IS_AVG takes cur = base; if no step closes, cur_out = base).
 * Writes base to seg.out, m and v in place, the final current to seg.cur_out.
 * FLAME_OPT_STATE_ZERO: m, v start as zeros and are not read.  Needs >= 1 client and a step_end
 * array.  Bitwise equal to one flame_fedopt_reduce_adapt_f64 launch per do() call.  Replaces,
 * per round, optimizer/fedopt.py:80-90,102-129 as the eager role
 * (eager_syncfl/top_aggregator.py:36-90) calls it on float64 tensors.
 */
int flame_fedopt_chain_f64(int variant, unsigned flags, const flame_segment *segs, int32_t n_segs,
                           int64_t n_chunks, const void *const *clients, int32_t n_clients,
                           const double *rates64, const uint8_t *step_end, double b1, double omb1,
                           double b2, double omb2, double eta, double tau, void *stream);

/*
 * FedBuff scale-add: out[e] = round(out[e] + round(in[e] / goal)); if seg.cur_out
 * is non-NULL also cur_out[e] = round(new - old) (the middle aggregator's delta).
 * Float dtypes only (the reference raises for integer tensors).
 */
int flame_fedbuff_scale_add(int dtype, const flame_segment *segs, int32_t n_segs,
                            int64_t n_chunks, int64_t goal, void *stream);

/* flame_hier_fedbuff flags */
#define FLAME_HIER_TOP_ACCUM 1u  /* the top aggregate exists (not None): start from seg.top_agg_in */
#define FLAME_HIER_TOP_APPLY 2u  /* finish with the top's scale-add into seg.top_w */
#define FLAME_HIER_MID_READONLY 4u  /* do not write w_m' back: the middles' weights are only the
                                      base of their deltas (the async middle role replaces them with
                                      the top's model at its next fetch,
                                      asyncfl/middle_aggregator.py:119-120); mid_w may then alias */
#define FLAME_HIER_SYNC 8u   /* the synchronous hierarchy (syncfl/middle_aggregator.py:163-229 feeding
                                syncfl/top_aggregator.py:122-176): per middle FedAvg from its weights,
                                a = w_m + tmp(c_{m,0}, r_{m,0}) + ..., w_m' = a, d_m = w_m' - w_m; the top
                                is a FedAvg from its weights: top = top_agg_in + tmp(d_m, top_rates[m]) in
                                order.  Needs FLAME_HIER_TOP_ACCUM, excludes FLAME_HIER_TOP_APPLY; mid_goal
                                is not read (any values) */

/* One contiguous run of elements of the hierarchy (one state_dict tensor). */
typedef struct flame_hier_segment {
    void *top_w;              /* top model weights, in/out (FLAME_HIER_TOP_APPLY) */
    const void *top_agg_in;   /* top aggregate before this batch (FLAME_HIER_TOP_ACCUM) */
    void *top_agg_out;        /* top aggregate after this batch (NULL = not stored; may == top_agg_in) */
    int64_t numel;
    int64_t chunk_begin;      /* prefix sum of ceil(numel / flame_chunk_elems(dtype)) */
    int64_t flags;            /* FLAME_SEG_UNALIGNED */
    int64_t client_tile_stride;  /* as flame_segment.client_tile_stride, shared by every arrival */
    int64_t mid_tile_stride;  /* bytes between consecutive chunks of one middle's weights (0 = each
                                 middle's weights contiguous); nonzero: every middle's weights are
                                 tiled like the arrivals (slots of one flame_amd UpdateSlab), so a
                                 chunk's middle weights form one contiguous [n_mids][chunk] block */
} flame_hier_segment;

/*
 * Co-located two-level FedBuff hierarchy (LIFL-style: n_mids middle aggregators on this
 * GPU feeding one top aggregator), one launch.  Per element, for m = 0 .. n_mids-1 (the
 * order the top receives the middles' deltas), every op rounded in dtype:
 *   a   = tmp(c_{m,0}, r_{m,0}); a = a + tmp(c_{m,i}, r_{m,i}) for i >= 1     (None-start FedBuff)
 *   w_m' = w_m + a / mid_goal[m];  d_m = w_m' - w_m;  w_m := w_m'          (scale_add + delta)
 *   top = tmp(d_0, top_rates[0]) (or top_agg_in + ...), top = top + tmp(d_m, top_rates[m])
 * then top_agg_out = top and, with FLAME_HIER_TOP_APPLY, top_w = top_w + top / top_goal.
 * tmp(v, r) = round(v * r).  Bit-identical to flame_agg_reduce (INIT_FIRST) per middle +
 * flame_fedbuff_scale_add with delta + one flame_agg_reduce per delta on the top aggregate +
 * flame_fedbuff_scale_add; the middle aggregates never reach HBM.
 *   mid_w     : device [n_segs][n_mids] pointers to each middle's weights (in/out; in only with
 *               FLAME_HIER_MID_READONLY)
 *   mid_delta : device [n_segs][n_mids] pointers for the deltas (NULL table or NULL entries:
 *               not stored)
 *   clients   : device [n_segs][n_mids][n_clients] arrival pointers, arrival order per middle
 *   mid_rates : device [n_mids][n_clients] fp32 staleness rates float(1/sqrt(1+version-v))
 *   mid_goal  : device [n_mids] float(agg_goal) of each middle; top_rates: device [n_mids]
 * dtype FLAME_F32, FLAME_BF16 or FLAME_F16.
 * With n_mids = 1, top_agg_out = NULL and no flags this is a single FedBuff aggregator's
 * scale_add (optimizer/fedbuff.py:101-127) applied straight from its queued arrivals
 * (fedbuff.py:89-97,136-157) -- the aggregate is never stored (the async top's round,
 * asyncfl/top_aggregator.py:85-110).
 */
int flame_hier_fedbuff(int dtype, unsigned flags, const flame_hier_segment *segs, int32_t n_segs,
                       int64_t n_chunks, int32_t n_mids, int32_t n_clients, const void *const *mid_w,
                       const void *const *mid_delta, const void *const *clients,
                       const float *mid_rates, const float *mid_goal, const float *top_rates,
                       float top_goal, void *stream);

/* flame_feddyn_round step flags */
#define FLAME_DYN_W 1u      /* the step has an arrival w (steps[..][0]) */
#define FLAME_DYN_AVG 2u    /* avg = avg + tmp(w, rate_avg)            (needs W) */
#define FLAME_DYN_HIN 4u    /* load the history h (steps[..][1]) */
#define FLAME_DYN_HOUT 8u   /* h' = HIN ? h + w : w, stored to steps[..][2] (needs W) */
#define FLAME_DYN_MEAN 16u  /* mean = mean + tmp(HOUT ? h' : h, rate_mean) (needs HIN or HOUT) */
/* One contiguous run of elements of a FedDyn round (one state_dict tensor). */
typedef struct flame_dyn_segment {
    void *out;                   /* the average (may == in) */
    const void *in;              /* base weights: the FedAvg start (deepcopy of cld_model) */
    void *cld;                   /* cld_model = avg + mean history (out) */
    int64_t numel;
    int64_t chunk_begin;         /* prefix sum of ceil(numel / flame_chunk_elems(dtype)) */
    int64_t flags;               /* FLAME_SEG_UNALIGNED */
    int64_t client_tile_stride;  /* arrivals: as flame_segment.client_tile_stride */
    int64_t hist_tile_stride;    /* histories: 0 = contiguous, else bytes between their chunks */
} flame_dyn_segment;
/*
 * One FedDyn server round (optimizer/feddyn.py:90-113 do() + :125-139 add_to_hist) in one
 * launch, per dtype.  steps: device [n_segs][n_steps][3] pointers (w, h_in,
 * h_out) per segment; step_flags: device [n_steps].  Per element, steps run in order with
 * mean starting at +0 (`0.0 + Σ rate*h`); every op rounds in dtype as torch-CPU does, so the
 * result is bit-identical to the reference's op sequence when the program lists the
 * arrivals in cache.iterkeys() order (AVG) and the histories in local_param_dict order
 * (MEAN).  Steps [n_phase1, n_steps) start after every earlier step's store, so they may
 * re-read a history written by a phase-1 step; within a phase no step may read another
 * step's output.  rate_avg = 1/len(cache), rate_mean = 1/len(local_param_dict) (rounded to
 * fp32 for f32/bf16/f16).  dtype FLAME_F32, FLAME_BF16, FLAME_F16 or FLAME_F64.
 */
int flame_feddyn_round(int dtype, const flame_dyn_segment *segs, int32_t n_segs, int64_t n_chunks,
                       const void *const *steps, const uint32_t *step_flags, int32_t n_steps,
                       int32_t n_phase1, double rate_avg, double rate_mean, void *stream);
/*
 * flame_elementwise: one elementwise program -- a short typed op sequence, the reference's
 * own torch statements for the keys the fused kernels do not take (int buffers such as
 * num_batches_tracked, mixed-dtype keys, fp64 / int8 / uint8 / int16 tensors):
 *   optimizer/fedopt.py:102-129 + fedadam.py:33-35 / fedyogi.py:34-36 / fedadagrad.py:33-35
 *     (FedOPT's adaptive step: d, m, v, sqrt(v) + tau, the quotient, current + ...),
 *   optimizer/scaffold.py:141-150 (c += (w * rate).to(c.dtype) for a control of another dtype),
 *   optimizer/feddyn.py:90-113,125-139 (the history / mean / cld statements of mixed keys).
 * flame_amd/elementwise.py records the statements on lazy tensors and takes every result dtype
 * from torch's own promotion (the statements run on meta tensors of the same shapes), so a
 * program only ever computes what torch-CPU would: an op whose operands are cast (FLAME_EW_CAST)
 * to its result dtype first, then
 *   fp32 / fp64: one IEEE round-to-nearest-even op (sqrt / divide correctly rounded);
 *   bf16 / fp16: the op in fp32 on the widened operands, rounded once to the dtype; a scalar
 *     is used in fp32 by MUL_S and rounded to the dtype first by ADD_S (torch-CPU's behaviour);
 *   integers: two's-complement arithmetic wrapped to the dtype's width (bool: + is a logical
 *     or, * a logical and, - is refused as torch refuses it).
 * A float -> integer FLAME_EW_CAST is defined for finite values whose truncation toward zero fits
 * the target type (a negative value does not fit FLAME_U8); for a NaN, an infinity or a value
 * outside that range the result is unspecified, as in the reference (C++ undefined behaviour).
 * An integer dtype applies ADD_S / MUL_S's scalar as an int64 wrapped to the dtype's width, so
 * the scalar must be an integer that a double and an int64 hold exactly.
 * Per element i of [0, numel): registers r[0..FLAME_EW_MAX_REGS) start undefined; ops run in
 * order.  prog (n_ops <= FLAME_EW_MAX_OPS) and bufs (n_bufs <= FLAME_EW_MAX_BUFS) are HOST
 * arrays, copied into the launch; every buffer is a contiguous DEVICE array of numel elements.
 */
#define FLAME_U8 6     /* element types only flame_elementwise takes */
#define FLAME_I8 7
#define FLAME_I16 8
#define FLAME_BOOL 9
#define FLAME_EW_LOAD 0    /* r[dst] = bufs[a][i], read as dtype */
#define FLAME_EW_STORE 1   /* bufs[a][i] = r[b], written as dtype (= r[b]'s dtype) */
#define FLAME_EW_ZERO 2    /* r[dst] = 0 (torch.zeros_like) */
#define FLAME_EW_CAST 3    /* r[dst] = r[a] (dtype b) as dtype: int -> float RNE (via fp32 for
                              bf16 / fp16, as c10 converts), float -> narrower float RNE (fp64 ->
                              bf16 / fp16 via fp32), float -> int toward zero, int -> int wrapped,
                              to bool: != 0 */
#define FLAME_EW_ADD 4     /* r[dst] = r[a] + r[b] (both already dtype) */
#define FLAME_EW_SUB 5     /* r[a] - r[b] */
#define FLAME_EW_MUL 6     /* r[a] * r[b] */
#define FLAME_EW_DIV 7     /* r[a] / r[b] (float dtype: torch's true division) */
#define FLAME_EW_ADD_S 8   /* r[a] + scalar */
#define FLAME_EW_MUL_S 9   /* r[a] * scalar */
#define FLAME_EW_SQUARE 10 /* r[a] ** 2 */
#define FLAME_EW_SIGN 11   /* torch.sign (NaN and -0 -> +0 for floats) */
#define FLAME_EW_SQRT 12   /* torch.sqrt (float dtype) */
#define FLAME_EW_MAX_OPS 64
#define FLAME_EW_MAX_REGS 32
#define FLAME_EW_MAX_BUFS 16
typedef struct flame_ew_op {
    int32_t op;      /* FLAME_EW_* */
    int32_t dtype;   /* the result's element type (LOAD / STORE: the buffer's) */
    int32_t dst;     /* register written */
    int32_t a;       /* register read (LOAD / STORE: the buffer index) */
    int32_t b;       /* second register read (STORE: the register stored; CAST: r[a]'s dtype) */
    int32_t pad;
    double scalar;   /* ADD_S / MUL_S: the Python scalar */
} flame_ew_op;
int flame_elementwise(const flame_ew_op *prog, int32_t n_ops, void *const *bufs, int32_t n_bufs,
                      int64_t numel, void *stream);
/*
 * The same program over several segments in one launch (e.g. a ResNet's BatchNorm
 * num_batches_tracked keys, which share one program): table = DEVICE [n_segs][n_bufs] buffer
 * pointers, seg_end = DEVICE [n_segs] inclusive prefix sums of the segments' element counts,
 * numel = seg_end[n_segs - 1].  prog is a HOST array as above.
 */
int flame_elementwise_segments(const flame_ew_op *prog, int32_t n_ops, void *const *table, int32_t n_bufs,
                               const int64_t *seg_end, int32_t n_segs, int64_t numel, void *stream);

/*
 * flame_hier_fedbuff for small launches: the metadata block (segments, then the mid_w,
 * mid_delta, client, mid_rates, mid_goal and top_rates tables at the given byte offsets;
 * off_mid_delta = -1 for none) is passed from HOST memory as a kernel argument instead of
 * being copied to the device first.  meta_bytes <= flame_agg_argmeta_max_bytes().
 */
int flame_hier_fedbuff_argmeta(int dtype, unsigned flags, const void *host_meta, int64_t meta_bytes,
                               int32_t n_segs, int64_t n_chunks, int32_t n_mids, int32_t n_clients,
                               int64_t off_mid_w, int64_t off_mid_delta, int64_t off_clients,
                               int64_t off_mid_rates, int64_t off_mid_goal, int64_t off_top_rates,
                               float top_goal, void *stream);

/*
 * Workgroups of the flame_hier_fedbuff launch for (dtype, n_mids, FLAME_HIER_SYNC in flags)
 * that stay resident per CU at once (hipOccupancyMaxActiveBlocksPerMultiprocessor on the
 * instantiation flame_hier_fedbuff would pick).  Its workgroups are long-lived (a chunk's
 * every arrival), so a launch of chunks not a multiple of (this x CUs) ends in a partly
 * filled last round of workgroups; flame_amd.shard sizes its waves with it.  Returns the
 * count (>= 1) or a negative FLAME_E* status (host-side query, no launch).
 */
int flame_hier_resident_per_cu(int dtype, unsigned flags, int32_t n_mids);

/*
 * Host buffers the kernels read zero-copy over PCIe (ingest; flame_amd/ingest.py).
 *   flame_host_register:   page-lock + map an existing host range (e.g. a received
 *                          channel payload or the LIFL shared-memory segment,
 *                          lib/python/flame/backend/shm.py:386-403) for device access.
 *   flame_host_unregister: undo it.
 *   flame_host_device_pointer: device address of a pinned / registered host address
 *                          (hipHostMalloc'd memory maps to itself).
 */
int flame_host_register(void *host, uint64_t nbytes);
int flame_host_unregister(void *host);
int flame_host_device_pointer(void *host, void **device);

/*
 * Fill out[0..numel) with the counter-based generator of flame_amd/synth.py:
 *   value_f32(seed, stream_id, start + j) * scale, rounded RNE to `dtype`
 *   (FLAME_F32 / FLAME_BF16 / FLAME_F16).  `out` is a device pointer.
 */
int flame_synth_fill(int dtype, void *out, int64_t numel, uint64_t seed, uint64_t stream_id,
                     int64_t start, float scale, void *stream);

/*
 * Server-side Gaussian noise: the reference's trainer-side statement
 * privacy/differential_privacy.py:55-61 (torch.normal(0, noise_factor) added to every element
 * of a trainer's delta), drawn once per round on the aggregator for the weighted average.
 * Write-only over a segment table: of each flame_segment only out, numel, chunk_begin and flags
 * (FLAME_SEG_UNALIGNED) are read.  Element e of segment s receives
 *   out[e] = round_dtype(z(seed, round, streams[s], starts[s] + e) * std)
 * where z is an fp32 unit normal, a pure function of its four arguments:
 *   bits      Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
 *             1, 2, 3", SC'11), key (seed & 0xffffffff, seed >> 32), counter (b & 0xffffffff,
 *             b >> 32, stream, round) with b = g >> 2 for global index g; the output words
 *             x0..x3 serve elements 4b .. 4b+3
 *   uniforms  u1 = RNE_f32(2 x + 1) * 2^-33 in (0, 1] from x0 (x2), the angle 2 pi k / 2^24
 *             with k = x1 >> 8 (x3 >> 8)
 *   transform Box-Muller (Box, Muller: "A note on the generation of random normal deviates",
 *             Ann. Math. Statist. 29, 1958): r = sqrt(-2 ln u1), z_even = r cos, z_odd = r sin,
 *             as explicit fp32 multiplies, adds, one divide and one correctly rounded root
 *             (no fma, no hardware log / sin / cos), restated op for op by tests/noise_ref.py
 * FLAME_F32 / FLAME_BF16 / FLAME_F16 take std rounded to fp32 and one fp32 multiply (16-bit:
 * then one RNE rounding); FLAME_F64 widens z and takes one fp64 multiply by std itself.
 *   streams : device uint32[n_segs], the key's position in the model's iteration order
 *   starts  : device int64[n_segs], >= 0 (the caller's to guarantee: the array lives in device
 *             memory), the global index of the segment's first element inside its key, so a
 *             sub-range of a key can be generated alone; a segment with starts % 4 == 0 and
 *             aligned `out` is written in 16-byte vectors, any other element by element
 * The result does not depend on the launch geometry.  Refused before any HIP call: a NULL
 * table or array, n_segs <= 0, n_chunks outside [1, 2^31), an integer (FLAME_ENOTSUP, "float
 * dtypes only") or unknown dtype, std negative, NaN or infinite (or, for the fp32-std dtypes,
 * rounding to an infinite fp32).
 */
int flame_noise_fill(int dtype, const flame_segment *segs, int32_t n_segs, int64_t n_chunks,
                     const uint32_t *streams, const int64_t *starts, uint64_t seed, uint32_t round,
                     double std, void *stream);

/*
 * Slab insert: the aggregator role's `self.cache[end] = tres` (mode/horizontal/syncfl/
 * top_aggregator.py:154-156, asyncfl/top_aggregator.py:85-87) into a tiled update slab
 * (flame_amd/slab.py).  Per entry (one state_dict key of one update): the `nbytes`
 * contiguous bytes at `src` are cut into FLAME_TILE_BYTES tiles (one reduction chunk of
 * every dtype, = flame_chunk_elems(dtype) x itemsize) and tile t is written to
 * dst + t * dst_tile_stride; the last tile may be partial (bytes past nbytes untouched).
 * dst must be 16-byte aligned, dst_tile_stride >= FLAME_TILE_BYTES and a multiple of 16
 * when the entry spans more than one tile; src may have any alignment; nbytes == 0 entries
 * are skipped.
 *   flame_slab_write    : ONE kernel launch for up to 89 entries (the table travels as a
 *                         kernel argument, no metadata H2D); src is a device pointer (or a
 *                         mapped pinned-host pointer, read over PCIe).
 *   flame_slab_write_2d : per entry one hipMemcpy2DAsync (pitch = dst_tile_stride) plus one
 *                         hipMemcpyAsync for a ragged tail, on the copy engines; for host
 *                         sources (pinned, registered or pageable).
 * Both are asynchronous on `stream`.
 */
#define FLAME_TILE_BYTES 4096
typedef struct flame_tile_copy {
    const void *src;
    void *dst;
    int64_t nbytes;
    int64_t dst_tile_stride;
} flame_tile_copy;
int flame_slab_write(const flame_tile_copy *table, int32_t n_entries, void *stream);
int flame_slab_write_2d(const flame_tile_copy *table, int32_t n_entries, void *stream);

/*
 * Launch-branch counters (test and audit support; no reference counterpart).  Every
 * host-side branch of the launch entry points above that picks a kernel instantiation
 * (dtype, variant, residency, store-group mode) has an index in [0, flame_launch_branches());
 * each successful launch increments its branch's process-wide counter.
 *   flame_launch_branch_name  : "entry/mode/dtype[/variant]", NULL outside the range
 *   flame_launch_branch_count : launches so far, -1 outside the range
 */
int32_t flame_launch_branches(void);
const char *flame_launch_branch_name(int32_t branch);
int64_t flame_launch_branch_count(int32_t branch);

#ifdef __cplusplus
}
#endif
#endif /* FLAME_AMD_H */
