// fedagg.hip -- CDNA4 (gfx950) kernels + C ABI for flame's server-side aggregation.
//
// Hot path: the weighted reduction of N client updates into
// one global model, restated from /root/reference/lib/python/flame/
//   optimizer/fedavg.py:79-104, optimizer/fedbuff.py:89-97,122-157,
//   optimizer/fedopt.py:102-129 (+ fedadam.py:33-35, fedyogi.py:34-36, fedadagrad.py:33-35).
//
// Design:
//   * HBM-read bound (≈1 flop per byte): no MFMA (the pairwise Gram kernel, update_gram_kernel, is
//     the one exception: fp64 matrix cores); every byte is read once.  LDS only holds
//     output blocks so their HBM writes go out as bursts (FedOPT, the hierarchy), or caps
//     residency at 2 workgroups per CU for long launches (HBM streams fastest there).
//   * One workgroup (256 lanes) owns one chunk of one segment; each lane owns
//     16 contiguous bytes of every client's update (dwordx4, non-temporal), so
//     every wave instruction is a 1 KiB fully-coalesced read.
//   * The client axis stays SEQUENTIAL in registers: per element the sum is
//     acc = round(acc + round(v_i * r_i)) in cache.iterkeys() order, exactly the
//     reference's torch-CPU op order -> bit-identical results.  Reordering the
//     fp32 client sum (tree / __shfl_down / split-K) breaks the 1e-6 contract
//     at N=1024, so it is not done.
//   * CU clients are unrolled per step so each lane has CU x 16 B loads in
//     flight (memory-level parallelism); client pointers and rates are
//     wave-uniform and come through the scalar cache.
//   * Built with -ffp-contract=off and explicit __f*_rn ops: no FMA contraction.
//   * Every host-side launch branch (which instantiation a launch takes) is counted
//     (flame_launch_branch_count) and pinned by a GPU oracle test.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdarg>
#include <type_traits>

#include "../../include/flame_amd.h"
#include "fastmath.h"

// One IEEE rounding per reference op, denormals kept (fastmath.h's div_rn proof and every bitwise
// test rest on it).  -ffast-math / -ffinite-math-only are refused here; the denormal mode of the
// built kernels (-fgpu-flush-denormals-to-zero sets no macro) is checked on the code object by
// tests/test_denorm_mode.py.
#if defined(__FAST_MATH__) || (defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__)
#error "fedagg.hip must not be built with -ffast-math / -ffinite-math-only"
#endif

namespace {

// Tunables, each chosen by an interleaved A/B sweep on MI355X.  The product build
// (flame_amd/build.py) passes no -D: these defaults ARE the shipped kernel.  The sweep tools
// (tools/hier_sweep.py, tools/chain_sweep.py, ...) build variants of THIS source with -DFLAME_T_*
// overrides into build/, so a sweep always measures the shipped code with one knob moved.
constexpr int kBlock = 256;          // lanes per workgroup of the reduction kernels
#ifndef FLAME_T_CLIENT_UNROLL
#define FLAME_T_CLIENT_UNROLL 8
#endif
constexpr int kClientUnroll = FLAME_T_CLIENT_UNROLL;     // clients whose loads are issued together per lane (full residency)
#ifndef FLAME_T_CLIENT_UNROLL16
#define FLAME_T_CLIENT_UNROLL16 8
#endif
constexpr int kClientUnroll16 = FLAME_T_CLIENT_UNROLL16;   // the same for 16-bit dtypes (8 elements per lane vector)
// flame_agg_reduce, launches of >= kLoMinClients clients over >= kLoMinChunks chunks: 2 workgroups
// per CU (kLoLds of dynamic LDS, unused) with a client unroll of 3 (16-bit: 4) -- fewer loads in
// flight read HBM faster (C3: 14.90 -> 14.18 ms, 99 % of a region probe at that residency;
// profiles/r03ze_c3_sweep.log, r03zf_c3_sweep.log, r03zf_c3_bf16_sweep.log)
#ifndef FLAME_T_LO_UNROLL
#define FLAME_T_LO_UNROLL 3
#endif
constexpr int kLoUnroll = FLAME_T_LO_UNROLL;
#ifndef FLAME_T_LO_UNROLL16
#define FLAME_T_LO_UNROLL16 4
#endif
constexpr int kLoUnroll16 = FLAME_T_LO_UNROLL16;
#ifndef FLAME_T_LO_LDS
#define FLAME_T_LO_LDS 65536
#endif
constexpr int kLoLds = FLAME_T_LO_LDS;
// Below kLoBurstMaxClients clients the low-residency launch also holds kLoWGC chunks' outputs per
// workgroup in LDS and stores them in one burst: the short client streams of such rounds pay for
// every interleaved store.  Tiled slab, one process, bitwise (tools/kernel_sweep.py,
// profiles/r05s_lo_wgc_*.log, r05t_lo_wgc_*.log): fp32 x 25M, 64 clients 0.964 -> 0.909 ms, 128
// 1.843 -> 1.797, 256 3.594 -> 3.546, 512 equal, 1,024 +0.8 %; bf16 x 50M, 64 clients 1.028 ->
// 0.969 ms, 256 3.647 -> 3.621.  (A kernel-argument launch never holds 512 clients' pointers, so
// its low-residency launches always burst.)
#ifndef FLAME_T_LO_WGC
#define FLAME_T_LO_WGC 8
#endif
constexpr int kLoWGC = FLAME_T_LO_WGC;
#ifndef FLAME_T_LO_BURST_MAX_CLIENTS
#define FLAME_T_LO_BURST_MAX_CLIENTS 512
#endif
constexpr int kLoBurstMaxClients = FLAME_T_LO_BURST_MAX_CLIENTS;
// the dynamic LDS that, beside the kLoWGC chunks' held outputs (4 KiB each), still makes kLoLds per workgroup
constexpr int kLoHeld = kLoWGC > 1 ? kLoWGC * 4096 : 0;
constexpr int kLoDynLds = kLoLds > kLoHeld ? kLoLds - kLoHeld : 0;
#ifndef FLAME_T_LO_MIN_CLIENTS
#define FLAME_T_LO_MIN_CLIENTS 64
#endif
constexpr int kLoMinClients = FLAME_T_LO_MIN_CLIENTS;    // 64 x 100M fp32: 4.04 -> 3.90 ms (profiles/r03zn_c64_lomin.log)
#ifndef FLAME_T_LO_MIN_CHUNKS
#define FLAME_T_LO_MIN_CHUNKS 4096
#endif
constexpr int64_t kLoMinChunks = FLAME_T_LO_MIN_CHUNKS;
// FedOPT (fp32, >= 8 x 256 x kOptWGC chunks): kOptWGC chunks per workgroup, their avg/m/v/cur
// blocks held in LDS (16 KiB per chunk -> 2 workgroups per CU) and stored in one burst at the end,
// client unroll kOptUnroll (profiles/r02_fedopt_wgc_sweep.log, r03zf_c4_sweep.log, r03zg_c4_sweep.log)
#ifndef FLAME_T_OPT_WGC
#define FLAME_T_OPT_WGC 4
#endif
constexpr int kOptWGC = FLAME_T_OPT_WGC;
#ifndef FLAME_T_OPT_UNROLL
#define FLAME_T_OPT_UNROLL 3
#endif
constexpr int kOptUnroll = FLAME_T_OPT_UNROLL;
// hierarchy kernel: register store groups of kHB middles (16-bit client unroll kHierUnroll16);
// launches of >= kHLdsMinMids middles hold store groups of kHBL middles in LDS (4 KiB each per
// workgroup, 2 workgroups per CU) with a 16-bit unroll of kHierLdsUnroll16 (C5 shard 20.99 ->
// 19.51 ms, profiles/r02_hier_lds_sweep.log); one middle over >= 64 arrivals and >= 4,096 chunks
// (a FedBuff aggregator's fused scale_add): low residency, unroll 3 (profiles/r03zv_fedbuff_*.log)
#ifndef FLAME_T_HB
#define FLAME_T_HB 8
#endif
constexpr int kHB = FLAME_T_HB;
#ifndef FLAME_T_HIER_UNROLL16
#define FLAME_T_HIER_UNROLL16 4
#endif
constexpr int kHierUnroll16 = FLAME_T_HIER_UNROLL16;
#ifndef FLAME_T_HBL
#define FLAME_T_HBL 16
#endif
constexpr int kHBL = FLAME_T_HBL;
#ifndef FLAME_T_HIER_LDS_UNROLL16
#define FLAME_T_HIER_LDS_UNROLL16 6
#endif
constexpr int kHierLdsUnroll16 = FLAME_T_HIER_LDS_UNROLL16;
#ifndef FLAME_T_HLDS_MIN_MIDS
#define FLAME_T_HLDS_MIN_MIDS 16
#endif
constexpr int kHLdsMinMids = FLAME_T_HLDS_MIN_MIDS;
#ifndef FLAME_T_HLO_UNROLL
#define FLAME_T_HLO_UNROLL 3
#endif
constexpr int kHLoUnroll = FLAME_T_HLO_UNROLL;
#ifndef FLAME_T_HLO_MIN_CLIENTS
#define FLAME_T_HLO_MIN_CLIENTS 64
#endif
constexpr int kHLoMinClients = FLAME_T_HLO_MIN_CLIENTS;
#ifndef FLAME_T_HLO_MIN_CHUNKS
#define FLAME_T_HLO_MIN_CHUNKS 4096
#endif
constexpr int64_t kHLoMinChunks = FLAME_T_HLO_MIN_CHUNKS;
#ifndef FLAME_T_HLO_LDS_F32
#define FLAME_T_HLO_LDS_F32 65536
#endif
constexpr int kHLoLdsF32 = FLAME_T_HLO_LDS_F32;    // 2 workgroups per CU
#ifndef FLAME_T_HLO_LDS16
#define FLAME_T_HLO_LDS16 53248
#endif
constexpr int kHLoLds16 = FLAME_T_HLO_LDS16;     // 3 workgroups per CU
#ifndef FLAME_T_DYN_UNROLL
#define FLAME_T_DYN_UNROLL 4
#endif
constexpr int kDynUnroll = FLAME_T_DYN_UNROLL;
#ifndef FLAME_T_CHAIN_UNROLL
#define FLAME_T_CHAIN_UNROLL 16
#endif
constexpr int kChainUnroll = FLAME_T_CHAIN_UNROLL;     // eager FedOPT chain: client loads in flight per lane
#ifndef FLAME_T_CHAIN_UNROLL16
#define FLAME_T_CHAIN_UNROLL16 8
#endif
constexpr int kChainUnroll16 = FLAME_T_CHAIN_UNROLL16;
// fp32 chain: 16 client loads in flight per lane at 3 workgroups per CU (dynamic LDS as the cap):
// 1.453 -> 1.358 ms per 64 x 25M round against 8 at full residency, one process, bitwise
// (profiles/r05g_chain_ab.log); 16-bit chains keep 8 at full residency
#ifndef FLAME_T_CHAIN_LDS
#define FLAME_T_CHAIN_LDS 53248
#endif
constexpr int kChainLds = FLAME_T_CHAIN_LDS;           // dynamic LDS per fp32 workgroup (a residency cap)
// bf16 FedOPT step (adapt_vec) and eager-chain arrivals: two elements per packed fp32 instruction,
// one instruction per bf16 rounding, v_sqrt_f32 / v_rcp_f32 where the bf16 rounding absorbs their
// ulp; 0 = the generic per-element path (same bits, for A/B builds)
#ifndef FLAME_T_BF16_PACKED
#define FLAME_T_BF16_PACKED 1
#endif
constexpr bool kBf16Packed = FLAME_T_BF16_PACKED != 0;
// the same for fp16 (two elements per fp32 instruction, a pair rounded by one v_cvt_pk_f16_f32 and
// widened back by two converts); 0 = the generic per-element path
#ifndef FLAME_T_F16_PACKED
#define FLAME_T_F16_PACKED 1
#endif
constexpr bool kF16Packed = FLAME_T_F16_PACKED != 0;
// fp16 root: v_sqrt_f32 under the fp16 rounding (1; tools/fp_probe.py finds it equal to the
// correctly rounded root's on every finite fp16 v, and the step's denominator on every v for every
// tau it draws, profiles/r06l_fp_probe.log) or flame_fm::sqrt_rn, then the rounding (0).  The
// quotient stays flame_fm::div_rn: num * v_rcp_f32 differs on 10,528 fp16 pairs (ties of subnormal
// results, where an fp16 quotient has too few bits for the midpoint argument)
#ifndef FLAME_T_F16_HWROOT
#define FLAME_T_F16_HWROOT 1
#endif
constexpr bool kF16HwRoot = FLAME_T_F16_HWROOT != 0;
// fp16 eager chain (full, aligned chunks): base / current / m / v held as packed fp16 pairs, every
// fp16-by-fp16 op one v_pk_add_f16 / v_pk_mul_f16, every scalar product two v_fma_mix_f32 and a
// v_cvt_pk_f16_f32 (1; fedopt_chain_body_f16), or the fp32-register step (0); same bits
#ifndef FLAME_T_F16_NATIVE
#define FLAME_T_F16_NATIVE 1
#endif
constexpr bool kF16Native = FLAME_T_F16_NATIVE != 0;
// ... and its root: v_sqrt_f16 on the packed pair (1; tools/fp_probe.py: equal to the correctly
// rounded fp16 root on every fp16 v >= +0) or v_sqrt_f32 on the widened halves (0)
#ifndef FLAME_T_F16_HSQRT
#define FLAME_T_F16_HSQRT 1
#endif
constexpr bool kF16HalfRoot = FLAME_T_F16_HSQRT != 0;
// the 16-bit steps' fast-path admission (adapt_vec_half): 1 = only what their root / quotient need --
// v in [+0, 2^78] for both, and for fp16 (flame_fm::div_rn) a finite |num|: every nonzero finite
// fp16 value is >= 2^-24, inside div_rn's range, and the bf16 quotient num * v_rcp_f32 matches on
// every non-NaN bf16 num (tools/fp_probe.py) -- so a bf16 m decaying through [2^-133, 2^-85]
// (a weight whose average stops moving) no longer sends its lane down the general path;
// 0 = the fp32 step's admission (flame_fm::admits), for A/B builds
#ifndef FLAME_T_HALF_ADMIT
#define FLAME_T_HALF_ADMIT 1
#endif
constexpr bool kHalfAdmit = FLAME_T_HALF_ADMIT != 0;
// FedYogi's (1 - beta_2) d^2 * sign(v - d^2): sign as one ordered compare + bit-select (1) or as
// torch writes it, two compares and an integer difference (0); same bits
#ifndef FLAME_T_YOGI_SIGN
#define FLAME_T_YOGI_SIGN 1
#endif
constexpr bool kYogiSelect = FLAME_T_YOGI_SIGN != 0;
constexpr int kEwBlock = 256;  // elementwise kernels (scale-add, synth)

thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(FLAME_EHIP, "%s: %s", what, hipGetErrorString(e));
    g_err[0] = 0;
    return FLAME_OK;
}

// ---------------------------------------------------------------- rounding helpers
__device__ __forceinline__ float bf16_round(float x) {
    // RNE fp32 -> bf16 -> fp32 (v_cvt_pk_bf16_f32 on gfx950)
    return static_cast<float>(static_cast<__bf16>(x));
}
__device__ __forceinline__ float bf16_to_f32(uint16_t b) {
    return __uint_as_float(static_cast<uint32_t>(b) << 16);
}
__device__ __forceinline__ uint16_t f32_to_bf16_exact(float x) {  // x already bf16-representable
    return static_cast<uint16_t>(__float_as_uint(x) >> 16);
}
// The same rounding with the result left where fp32 wants it (bits = bf16 << 16): ONE
// v_cvt_pk_bf16_f32 whose low half converts +0, instead of the convert into the low half and the
// shift up that bf16_round compiles to -- the same instruction, so the same bits (NaNs included).
// Never applied to a transcendental's result: gfx950 needs a wait state before a VALU reads a
// v_sqrt / v_rcp / v_rsq result, and the compiler does not insert it ahead of inline asm (those
// roundings use bf16_round).
__device__ __forceinline__ float bf16_rnd1(float x) {
    float r;
    asm("v_cvt_pk_bf16_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}
using f2 = __attribute__((ext_vector_type(2))) float;    // v_pk_{mul,add,fma}_f32 operands
__device__ __forceinline__ f2 bf16_rnd2(f2 x) { return f2{bf16_rnd1(x.x), bf16_rnd1(x.y)}; }
__device__ __forceinline__ f2 splat2(float x) { return f2{x, x}; }
// The empty asm pins x as an fp32 VGPR value: without it the backend folds
// fptrunc(fmul(a, r)) into v_fma_mixlo_f16, which rounds the exact product to
// fp16 ONCE, while torch rounds the fp32 product to fp16 (two roundings; they
// differ for an fp32 rate).
__device__ __forceinline__ float f16_round(float x) {
    asm volatile("" : "+v"(x));
    return static_cast<float>(static_cast<_Float16>(x));
}
__device__ __forceinline__ float f16_to_f32(uint16_t h) {
    _Float16 v;
    __builtin_memcpy(&v, &h, 2);
    return static_cast<float>(v);
}
__device__ __forceinline__ uint16_t f32_to_f16_bits(float x) {
    asm volatile("" : "+v"(x));
    _Float16 v = static_cast<_Float16>(x);
    uint16_t h;
    __builtin_memcpy(&h, &v, 2);
    return h;
}
// A pair RNE-rounded to fp16 and widened back: ONE v_cvt_pk_f16_f32 (the same conversion as
// f16_round's v_cvt_f16_f32, per half; inline asm, so the backend cannot fold a product into a
// single-rounding v_fma_mix) and two exact widening converts (the high half by SDWA).  Never
// applied to a transcendental's result (see bf16_rnd1).
__device__ __forceinline__ f2 f16_rnd2(f2 x) {
    uint32_t p;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(p) : "v"(x.x), "v"(x.y));
    return f2{f16_to_f32(static_cast<uint16_t>(p)), f16_to_f32(static_cast<uint16_t>(p >> 16))};
}

// fp16 pairs kept packed (the fp16 eager chain, FLAME_T_F16_NATIVE).  An op on two fp16 values
// rounded once to fp16 (v_pk_add_f16 / v_pk_mul_f16) equals torch-CPU's op in fp32 rounded to fp16:
// a product of two 11-bit significands is exact in fp32, and for a sum, square root or quotient
// fp32's 24 bits are >= 2p + 2 for p = 11, so rounding to fp32 first never changes the fp16
// rounding (Figueroa's double-rounding theorem).  A Python-scalar operand (beta, eta, a rate) is
// fp32 (24 bits), so those products go through fp32: smul_h2.
using h2 = __attribute__((ext_vector_type(2))) _Float16;
using us2 = __attribute__((ext_vector_type(2))) unsigned short;
__device__ __forceinline__ h2 h2_of(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ uint32_t u_of(h2 h) { return __builtin_bit_cast(uint32_t, h); }
__device__ __forceinline__ f2 widen_h2(uint32_t u) {
    const h2 h = h2_of(u);
    return f2{static_cast<float>(h.x), static_cast<float>(h.y)};
}
// RN16(RN32(s * x)) of a pair: two v_fma_mix_f32 (a half widened exactly inside the instruction;
// s * x + neg(0) = s * x + (-0) rounded once is the fp32 product, signed zeros included) and one v_cvt_pk_f16_f32 --
// instead of two widening converts, a v_pk_mul_f32, the rounding and two more widening converts.
// (lo, hi: the two fp32 products before the fp16 rounding)
__device__ __forceinline__ uint32_t smul_h2(float s, uint32_t x, float& lo, float& hi) {
    uint32_t r;
    asm("v_fma_mix_f32 %0, %1, %2, neg(0) op_sel_hi:[0,1,0]" : "=v"(lo) : "s"(s), "v"(x));
    asm("v_fma_mix_f32 %0, %1, %2, neg(0) op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(hi) : "s"(s), "v"(x));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ uint32_t smul_h2(float s, uint32_t x) {
    float lo, hi;
    return smul_h2(s, x, lo, hi);
}
// flame_fm::div_rn(num, den) with the numerator an fp16 half of x (HI: the high one): q0 = y * num
// as one v_fma_mix_f32 (the widening inside it), the residual's -num folded the same way by the
// compiler -- the same four roundings as div_rn on the widened value.  y is rcp_rn's fma result,
// never a v_rcp_f32 result, so no transcendental feeds the inline asm.
template <int HI>
__device__ __forceinline__ float div_rn_h(uint32_t x, float den) {
    const float y = flame_fm::rcp_rn(den);
    float q0;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, neg(0) op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(q0) : "v"(y), "v"(x));
    else asm("v_fma_mix_f32 %0, %1, %2, neg(0) op_sel_hi:[0,1,0]" : "=v"(q0) : "v"(y), "v"(x));
    const float a = static_cast<float>(HI ? h2_of(x).y : h2_of(x).x);
    const float rn = __builtin_fmaf(den, q0, -a);
    return __builtin_fmaf(-rn, y, q0);
}
// RN16 of an fp32 pair, packed (never on a transcendental's result, see bf16_rnd1)
__device__ __forceinline__ uint32_t pk_h2(f2 x) {
    uint32_t r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(x.x), "v"(x.y));
    return r;
}
// torch.sign of an fp16 pair as FedYogi's t * sign(x) uses it: +-1 for a nonzero x, +0 for +-0.
// x + 0 turns -0 into +0; x * 65504 * 65504 carries the smallest subnormal (2^-24) past 1 and
// overflows the rest to inf; the clamp to [-1, 1] keeps +-1 / +0.  A NaN x clamps to +1 (minNum),
// not to torch's 0.  With torch's 0 v's new value is always a NaN there: a NaN x = v - d^2 means v
// or d^2 is a NaN (t * sign is then NaN either way) or v = d^2 = +inf, where t = (1 - beta_2) * inf
// is a NaN or +-inf and t * 0 a NaN.  With +1 it is v - t: a NaN too for t = NaN or +inf, but +inf
// for t = -inf, which a beta_2 above 1 gives (tests/test_gpu_fedopt_sweep16.py found it).  So this
// is torch's result only while 1 - beta_2 >= 0: fedopt_chain_kernel keeps FedYogi off the packed
// body otherwise.
__device__ __forceinline__ h2 sign_h2(h2 x) {
    const h2 z = x + h2{0, 0};
    const h2 big = (z * h2{65504, 65504}) * h2{65504, 65504};
    return __builtin_elementwise_max(__builtin_elementwise_min(big, h2{1, 1}), h2{-1, -1});
}

// ---------------------------------------------------------------- dtype traits
// T: storage type; A: register accumulator type; EPT: elements per 16-byte lane vector.
// tmp(v, r) = the reference's `tmp = (v * rate).to(v.dtype)`; add(a, t) = `agg += tmp`;
// mulr(a, r) = one more product on a value already in the dtype (the float dtypes; the scaled
// reduction's `torch.mul(d_w, scale)` followed by the rate).
template <int DT> struct Tr;

template <> struct Tr<FLAME_F32> {
    using T = float; using A = float; static constexpr int EPT = 4;
    __device__ static A ld(T x) { return x; }
    __device__ static T st(A a) { return a; }
    __device__ static A tmp(T v, float r, double) { return __fmul_rn(v, r); }
    __device__ static A mulr(A a, float r, double) { return __fmul_rn(a, r); }
    __device__ static A add(A a, A t) { return __fadd_rn(a, t); }
};
template <> struct Tr<FLAME_BF16> {
    using T = uint16_t; using A = float; static constexpr int EPT = 8;
    __device__ static A ld(T x) { return bf16_to_f32(x); }
    __device__ static T st(A a) { return f32_to_bf16_exact(a); }
    __device__ static A tmp(T v, float r, double) { return bf16_round(__fmul_rn(bf16_to_f32(v), r)); }
    __device__ static A mulr(A a, float r, double) { return bf16_round(__fmul_rn(a, r)); }
    __device__ static A add(A a, A t) { return bf16_round(__fadd_rn(a, t)); }
};
template <> struct Tr<FLAME_F16> {
    using T = uint16_t; using A = float; static constexpr int EPT = 8;
    __device__ static A ld(T x) { return f16_to_f32(x); }
    __device__ static T st(A a) { return f32_to_f16_bits(a); }
    __device__ static A tmp(T v, float r, double) { return f16_round(__fmul_rn(f16_to_f32(v), r)); }
    __device__ static A mulr(A a, float r, double) { return f16_round(__fmul_rn(a, r)); }
    __device__ static A add(A a, A t) { return f16_round(__fadd_rn(a, t)); }
};
template <> struct Tr<FLAME_F64> {
    using T = double; using A = double; static constexpr int EPT = 2;
    __device__ static A ld(T x) { return x; }
    __device__ static T st(A a) { return a; }
    __device__ static A tmp(T v, float, double r) { return __dmul_rn(v, r); }
    __device__ static A mulr(A a, float, double r) { return __dmul_rn(a, r); }
    __device__ static A add(A a, A t) { return __dadd_rn(a, t); }
};
// int tensors: torch promotes int * python-float to fp32, then .to(int) truncates (fedavg.py:93-102)
template <> struct Tr<FLAME_I64> {
    using T = int64_t; using A = int64_t; static constexpr int EPT = 2;
    __device__ static A ld(T x) { return x; }
    __device__ static T st(A a) { return a; }
    __device__ static A tmp(T v, float r, double) { return static_cast<int64_t>(__fmul_rn(static_cast<float>(v), r)); }
    __device__ static A add(A a, A t) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(t)); }
};
template <> struct Tr<FLAME_I32> {
    using T = int32_t; using A = int32_t; static constexpr int EPT = 4;
    __device__ static A ld(T x) { return x; }
    __device__ static T st(A a) { return a; }
    __device__ static A tmp(T v, float r, double) { return static_cast<int32_t>(__fmul_rn(static_cast<float>(v), r)); }
    __device__ static A add(A a, A t) { return static_cast<int32_t>(static_cast<uint32_t>(a) + static_cast<uint32_t>(t)); }
};

// A chunk is one slab tile: each of the kBlock lanes owns one 16-byte vector of it.
template <int DT> constexpr int64_t chunk_elems() { return static_cast<int64_t>(kBlock) * Tr<DT>::EPT; }
template <int DT> constexpr bool chunk_is_tile() { return chunk_elems<DT>() * sizeof(typename Tr<DT>::T) == FLAME_TILE_BYTES; }
static_assert(chunk_is_tile<FLAME_F32>() && chunk_is_tile<FLAME_BF16>() && chunk_is_tile<FLAME_F16>() &&
              chunk_is_tile<FLAME_F64>() && chunk_is_tile<FLAME_I64>() && chunk_is_tile<FLAME_I32>(),
              "a chunk of every dtype is FLAME_TILE_BYTES bytes");

// ---------------------------------------------------------------- memory helpers
// All device data is accessed through address_space(1) (global) pointers so the
// compiler emits global_load/store (vmcnt only) instead of flat_* (which also
// count on lgkmcnt and would serialise against the scalar pointer/rate loads).
struct alignas(16) V16 { uint32_t w[4]; };
using u4 = __attribute__((ext_vector_type(4))) uint32_t;
template <typename T> using gptr = __attribute__((address_space(1))) T*;
template <typename T> using gcptr = const __attribute__((address_space(1))) T*;

template <typename T> __device__ __forceinline__ gcptr<T> G(const T* p) { return (gcptr<T>)(p); }
template <typename T> __device__ __forceinline__ gptr<T> G(T* p) { return (gptr<T>)(p); }

// Client updates are read exactly once: non-temporal loads.
__device__ __forceinline__ V16 ld_nt(const void* p) {
    u4 x = __builtin_nontemporal_load(G(reinterpret_cast<const u4*>(p)));
    V16 r; r.w[0] = x[0]; r.w[1] = x[1]; r.w[2] = x[2]; r.w[3] = x[3];
    return r;
}
__device__ __forceinline__ V16 ld_v(const void* p) {
    u4 x = *G(reinterpret_cast<const u4*>(p));
    V16 r; r.w[0] = x[0]; r.w[1] = x[1]; r.w[2] = x[2]; r.w[3] = x[3];
    return r;
}
// Output stores are write-through (sc0 sc1 nt): measured +2 % on config 3 and +4 % on
// 64-client bf16 against plain / nt stores, whose dirty L2 lines are written back
// interleaved with the client read stream (profiles/r01_scan5_*.log).  Inline asm
// because no builtin sets sc0/sc1; `s_nop 1` covers the store-data hazard.
__device__ __forceinline__ void st_v(void* p, const V16& v) {
    u4 x = {v.w[0], v.w[1], v.w[2], v.w[3]};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt\n\ts_nop 1" :: "v"(p), "v"(x) : "memory");
}
// A plain (write-back) vector store: the slab insert, whose tiles are read again soon.
__device__ __forceinline__ void st_plain(void* p, const V16& v) {
    u4 x = {v.w[0], v.w[1], v.w[2], v.w[3]};
    *G(reinterpret_cast<u4*>(p)) = x;
}
template <typename T> __device__ __forceinline__ T ld1(const T* p) { return *G(p); }
template <typename T> __device__ __forceinline__ void st1(T* p, T x) { *G(p) = x; }
template <typename T, int EPT>
__device__ __forceinline__ void unpack(const V16& v, T (&x)[EPT]) {
    static_assert(sizeof(T) * EPT == 16, "lane vector is 16 bytes");
    __builtin_memcpy(x, v.w, 16);
}
template <typename T, int EPT>
__device__ __forceinline__ V16 pack(const T (&x)[EPT]) {
    V16 v;
    __builtin_memcpy(v.w, x, 16);
    return v;
}

// Wave-uniform segment lookup: largest s with segs[s].chunk_begin <= chunk.
template <typename SEG>
__device__ __forceinline__ int find_segment(const SEG* __restrict__ segs, int n_segs, int64_t chunk) {
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk_begin <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The opening of every chunked kernel.  A workgroup owns chunk `chunk` of the launch: kBlock x EPT
// elements of segment s (any of the three segment structs), of which a lane owns EPT, one 16-byte
// vector (MXFP8 / mixed: one client vector), at elements e0 .. e0 + EPT - 1.  Each member is evaluated
// where it is called and kernels copy sg out: the listings depend on both (profiles/lane_isa_diff.log).
template <typename SEG, int EPT>
struct LaneChunk {
    static constexpr int64_t CE = static_cast<int64_t>(kBlock) * EPT;      // elements per chunk
    int s;              // the segment's index (wave-uniform)
    SEG sg;             // its table entry
    int64_t chunk;
    int64_t e0;         // the lane's first element
    __device__ __forceinline__ LaneChunk(const SEG* segs, int n_segs, int64_t chunk_)
        : s(find_segment(segs, n_segs, chunk_)), sg(segs[s]), chunk(chunk_),
          e0((chunk - sg.chunk_begin) * CE + static_cast<int64_t>(threadIdx.x) * EPT) {}
    // the lane has an element inside the segment
    __device__ __forceinline__ bool live() const { return e0 < sg.numel; }
    // the lane's vector is whole and aligned: 16-byte accesses; else element-wise with bounds
    __device__ __forceinline__ bool vec() const { return (e0 + EPT <= sg.numel) && !(sg.flags & FLAME_SEG_UNALIGNED); }
    // the segment's row of a table of n pointers per segment
    __device__ __forceinline__ const uint64_t* row(const uint64_t* __restrict__ t, int64_t n) const { return t + s * n; }
    // byte offset of the lane's first element (of `esize` bytes) inside a row's data: contiguous
    // (stride 0) or tiled, the segment's chunks `stride` bytes apart (a slab)
    __device__ __forceinline__ int64_t offset(int64_t stride, int64_t esize) const {
        const int64_t cl = chunk - sg.chunk_begin;
        const int64_t lane_elem = static_cast<int64_t>(threadIdx.x) * EPT;
        if (stride) return cl * stride + lane_elem * esize;
        return (cl * CE + lane_elem) * esize;
    }
};

// One lane's elements between memory and registers (EPT x sizeof(T) is one 16-byte vector, or
// several: the fp32 base of the mixed and MXFP8 kernels).  VEC: vector accesses (nt: read once);
// else element by element inside [e0, numel), zeros loaded beyond it.
template <bool VEC, bool NT = false, typename T, int EPT>
__device__ __forceinline__ void lane_load(const T* p, T (&x)[EPT], int64_t e0, int64_t numel) {
    constexpr int PER = 16 / sizeof(T);
    static_assert(EPT % PER == 0, "whole 16-byte vectors");
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < EPT; q += PER) {
            const V16 v = NT ? ld_nt(p + q) : ld_v(p + q);
            __builtin_memcpy(x + q, v.w, 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) x[j] = (e0 + j < numel) ? ld1(p + j) : T(0);
    }
}
template <bool VEC, typename T, int EPT>
__device__ __forceinline__ void lane_store(T* p, const T (&x)[EPT], int64_t e0, int64_t numel) {
    constexpr int PER = 16 / sizeof(T);
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < EPT; q += PER) {
            V16 v;
            __builtin_memcpy(v.w, x + q, 16);
            st_v(p + q, v);
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j)
            if (e0 + j < numel) st1(p + j, x[j]);
    }
}

// ---------------------------------------------------------------- reduction core
// Reduce clients [0, n) into acc for the lane's slots (LaneChunk).  VEC as in lane_load.  SCALED (flame_agg_reduce_scaled
// only; a template parameter, so no other kernel carries the branch): client i's value is first
// multiplied by its clip scale, tmp = round(round(v * scale_i) * rate_i).
// AD (flame_agg_reduce_mixed only; DT everywhere else): the accumulator's dtype where it differs from
// the clients' -- tmp is still formed and rounded in DT, the sum is AD's.
template <int DT, int CU, bool VEC, bool SCALED = false, int AD = DT>
__device__ __forceinline__ void reduce_clients(typename Tr<AD>::A (&acc)[Tr<DT>::EPT], bool init_first,
                                               const uint64_t* __restrict__ cp, int n,
                                               const float* __restrict__ r32, const double* __restrict__ r64,
                                               int64_t e0, int64_t numel, int64_t coff,
                                               const float* __restrict__ s32 = nullptr,
                                               const double* __restrict__ s64 = nullptr) {
    using X = Tr<DT>;
    using T = typename X::T;
    constexpr int EPT = X::EPT;
    int i = 0;
    auto rate32 = [&](int c) -> float { if constexpr (DT == FLAME_F64) return 0.f; else return r32[c]; };
    auto rate64 = [&](int c) -> double { if constexpr (DT == FLAME_F64) return r64[c]; else return 0.0; };
    auto load_client = [&](int c, T (&x)[EPT]) {
        lane_load<VEC, true>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(cp[c]) + coff), x, e0, numel);
    };
    // tmp of client c's element: the rate product, after the scale product when SCALED
    auto tmp_of = [&](int c, const float r, const double rd, T xv) {
        if constexpr (SCALED) {
            if constexpr (DT == FLAME_F64) return X::mulr(X::tmp(xv, 0.f, s64[c]), r, rd);
            else return X::mulr(X::tmp(xv, s32[c], 0.0), r, rd);
        } else {
            (void)c;
            return X::tmp(xv, r, rd);
        }
    };
    auto combine = [&](int c, const T (&x)[EPT]) {
        const float r = rate32(c);
        const double rd = rate64(c);
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = Tr<AD>::add(acc[j], tmp_of(c, r, rd, x[j]));
    };
    if (init_first && n > 0) {
        T x[EPT];
        load_client(0, x);
        const float r = rate32(0);
        const double rd = rate64(0);
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = tmp_of(0, r, rd, x[j]);
        i = 1;
    }
    for (; i + CU <= n; i += CU) {
        T x[CU][EPT];
#pragma unroll
        for (int u = 0; u < CU; ++u) load_client(i + u, x[u]);
#pragma unroll
        for (int u = 0; u < CU; ++u) combine(i + u, x[u]);
    }
    for (; i < n; ++i) {
        T x[EPT];
        load_client(i, x);
        combine(i, x);
    }
}

// One chunk of one segment: acc = base (or client 0), reduce every client in order.
// Full, aligned chunks hand their output vector back (ov / op) so the caller can
// store it; tails and misaligned views store element-wise here.
template <int DT, int CU, bool SCALED = false>
__device__ __forceinline__ bool reduce_chunk(const flame_segment* __restrict__ segs, int n_segs,
                                             const uint64_t* __restrict__ clients, int n_clients,
                                             const float* __restrict__ r32, const double* __restrict__ r64,
                                             unsigned flags, int64_t chunk, V16& ov,
                                             typename Tr<DT>::T*& op, const float* __restrict__ s32 = nullptr,
                                             const double* __restrict__ s64 = nullptr) {
    using X = Tr<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return false;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(T));
    const bool init_first = (flags & FLAME_AGG_INIT_FIRST) != 0;
    if (flags & FLAME_AGG_SEG_RATES) {  // one rate row per segment
        if (r32) r32 += static_cast<int64_t>(lc.s) * n_clients;
        if (r64) r64 += static_cast<int64_t>(lc.s) * n_clients;
    }
    const bool vec = lc.vec();
    A acc[EPT];
    const T* bp = reinterpret_cast<const T*>(sg.in) + e0;
    op = reinterpret_cast<T*>(sg.out) + e0;
    if (vec) {
        if (!init_first) {
            T b[EPT];
            unpack<T, EPT>(ld_v(bp), b);
#pragma unroll
            for (int j = 0; j < EPT; ++j) acc[j] = X::ld(b[j]);
        }
        reduce_clients<DT, CU, true, SCALED>(acc, init_first, cp, n_clients, r32, r64, e0, sg.numel, coff, s32, s64);
        T o[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) o[j] = X::st(acc[j]);
        ov = pack<T, EPT>(o);
        return true;
    }
    if (!init_first) {
#pragma unroll
        for (int j = 0; j < EPT; ++j)
            acc[j] = X::ld((e0 + j < sg.numel) ? ld1(bp + j) : T(0));
    }
    reduce_clients<DT, 1, false, SCALED>(acc, init_first, cp, n_clients, r32, r64, e0, sg.numel, coff, s32, s64);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (e0 + j < sg.numel) st1(op + j, X::st(acc[j]));
    return false;
}

// Workgroup slot of block b when the 8 XCDs (dispatched round-robin) each take one
// contiguous eighth of the slots (FLAME_AGG_XCD_MAP / FLAME_OPT_XCD_MAP): a bijection.
__device__ __forceinline__ int64_t xcd_slot(int64_t b, int64_t n) {
    const int64_t q = n / 8, r = n % 8, x = b % 8;
    return x * q + (x < r ? x : r) + b / 8;
}
// The workgroup's slot: that map where the launch's flag bit asks for it, else launch order.
__device__ __forceinline__ int64_t wg_slot(unsigned xcd_map) {
    return xcd_map ? xcd_slot(blockIdx.x, gridDim.x) : blockIdx.x;
}

// G chunks per workgroup (G = 1: chunk = workgroup slot, in launch order or the XCD-contiguous
// map).  G > 1: the workgroup reduces chunks slot*G .. slot*G+G-1 one after another, holds their
// full output vectors in LDS and stores them in one burst at the end.
template <int DT, int CU, int G>
__device__ __forceinline__ void agg_reduce_body(const flame_segment* __restrict__ segs, int n_segs,
                                                const uint64_t* __restrict__ clients, int n_clients,
                                                const float* __restrict__ r32, const double* __restrict__ r64,
                                                unsigned flags, int64_t n_chunks) {
    using T = typename Tr<DT>::T;
    const int64_t slot = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if constexpr (G == 1) {
        if (slot >= n_chunks) return;
        V16 ov;
        T* op;
        if (reduce_chunk<DT, CU>(segs, n_segs, clients, n_clients, r32, r64, flags, slot, ov, op)) st_v(op, ov);
    } else {
        static_assert(G <= 32 && G * kBlock * sizeof(V16) <= 128 * 1024, "agg_reduce_body: G chunks' outputs exceed the LDS");
        __shared__ V16 held[G][kBlock];
        unsigned pending = 0;
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            const int64_t chunk = slot * G + g;
            if (chunk >= n_chunks) break;
            V16 ov;
            T* op;
            if (reduce_chunk<DT, CU>(segs, n_segs, clients, n_clients, r32, r64, flags, chunk, ov, op)) {
                held[g][threadIdx.x] = ov;
                pending |= 1u << g;
            }
        }
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            if (!(pending >> g & 1u)) continue;
            // (through LaneChunk the f16 instantiation swaps two registers: profiles/lane_isa_diff.log)
            const int64_t chunk = slot * G + g;
            const flame_segment& sg = segs[find_segment(segs, n_segs, chunk)];
            T* op = reinterpret_cast<T*>(sg.out) + (chunk - sg.chunk_begin) * chunk_elems<DT>() +
                    static_cast<int64_t>(threadIdx.x) * Tr<DT>::EPT;
            st_v(op, held[g][threadIdx.x]);
        }
    }
}

template <int DT, int CU, int G>
__global__ __launch_bounds__(kBlock) void agg_reduce_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                            const uint64_t* __restrict__ clients, int n_clients,
                                                            const float* __restrict__ r32,
                                                            const double* __restrict__ r64, unsigned flags,
                                                            int64_t n_chunks) {
    agg_reduce_body<DT, CU, G>(segs, n_segs, clients, n_clients, r32, r64, flags, n_chunks);
}

// Small launches (few segments x few hundred clients): the whole metadata block travels as a
// kernel argument.  A separate H2D copy of a few KB is a blit kernel on gfx950 that the launch
// stream must run before the reduction (≈15 µs of GPU timeline per launch, measured on
// config 2: 0.171 -> 0.157 ms per step without it); kernel arguments reach the GPU with the
// dispatch itself and are read through the scalar cache like the device-resident table.
constexpr int kArgMetaWords = 448;          // 3,584 B: kernel arguments are limited to 4 KiB
struct ArgMeta { uint64_t w[kArgMetaWords]; };

template <int DT, int CU, int G>
__global__ __launch_bounds__(kBlock) void agg_reduce_kernel_argmeta(const ArgMeta meta, int n_segs, int n_clients,
                                                                    int off_clients, int off_r32, int off_r64,
                                                                    unsigned flags, int64_t n_chunks) {
    // `meta` is the first kernel argument: read it in place in the kernarg segment (scalar
    // loads) -- naming the by-value parameter would copy 3.5 KB into every lane's scratch
    (void)sizeof(meta);
    const uint64_t* w = (const uint64_t*)__builtin_amdgcn_kernarg_segment_ptr();
    agg_reduce_body<DT, CU, G>(reinterpret_cast<const flame_segment*>(w), n_segs, w + off_clients, n_clients,
                            off_r32 >= 0 ? reinterpret_cast<const float*>(w + off_r32) : nullptr,
                            off_r64 >= 0 ? reinterpret_cast<const double*>(w + off_r64) : nullptr, flags, n_chunks);
}

// ---------------------------------------------------------------- scaled reduction (update guard)
// flame_agg_reduce with a per-client clip scale in front of the rate (differential_privacy.py:79-82
// then fedavg.py:93-104).  Its own kernel family, one chunk per workgroup at full residency: the
// SCALED template argument keeps the extra product out of every other instantiation.
template <int DT, int CU>
__global__ __launch_bounds__(kBlock) void agg_reduce_scaled_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                                   const uint64_t* __restrict__ clients, int n_clients,
                                                                   const float* __restrict__ r32,
                                                                   const double* __restrict__ r64,
                                                                   const float* __restrict__ s32,
                                                                   const double* __restrict__ s64, unsigned flags,
                                                                   int64_t n_chunks) {
    using T = typename Tr<DT>::T;
    const int64_t slot = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (slot >= n_chunks) return;
    V16 ov;
    T* op;
    if (reduce_chunk<DT, CU, true>(segs, n_segs, clients, n_clients, r32, r64, flags, slot, ov, op, s32, s64))
        st_v(op, ov);
}

// ---------------------------------------------------------------- 16-bit updates into an fp32 aggregate
// flame_agg_reduce_mixed: bf16 / f16 client values (CD) summed into an fp32 base, the reference's
// `tmp = (v * rate)` in v's dtype and `agg += tmp` in the promoted one (fedavg.py:93-104).  The
// chunk is the clients': 2,048 elements, one 16-byte client vector per lane and client, eight fp32
// accumulators per lane, two 16-byte vectors of in / out.  One chunk per workgroup at full
// residency; SCALED as in agg_reduce_scaled_kernel.
template <int CD, int CU, bool SCALED>
__global__ __launch_bounds__(kBlock) void agg_reduce_mixed_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                                  const uint64_t* __restrict__ clients, int n_clients,
                                                                  const float* __restrict__ r32,
                                                                  const float* __restrict__ s32, unsigned flags,
                                                                  int64_t n_chunks) {
    static_assert(CD == FLAME_BF16 || CD == FLAME_F16, "16-bit clients, one client vector per lane");
    constexpr int EPT = Tr<CD>::EPT;        // 8 client values = 2 fp32 vectors of 4
    const int64_t chunk = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (chunk >= n_chunks) return;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(typename Tr<CD>::T));
    const float* bp = reinterpret_cast<const float*>(sg.in) + e0;
    float* op = reinterpret_cast<float*>(sg.out) + e0;
    float acc[EPT];
    if (lc.vec()) {       // (either arm through lane_load / lane_store moves registers: profiles/lane_isa_diff.log)
        float b[2][4];
        unpack<float, 4>(ld_v(bp), b[0]);
        unpack<float, 4>(ld_v(bp + 4), b[1]);
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = b[j / 4][j % 4];
        reduce_clients<CD, CU, true, SCALED, FLAME_F32>(acc, false, cp, n_clients, r32, nullptr, e0, sg.numel, coff, s32);
#pragma unroll
        for (int j = 0; j < EPT; ++j) b[j / 4][j % 4] = acc[j];
        st_v(op, pack<float, 4>(b[0]));
        st_v(op + 4, pack<float, 4>(b[1]));
        return;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = (e0 + j < sg.numel) ? ld1(bp + j) : 0.f;
    reduce_clients<CD, 1, false, SCALED, FLAME_F32>(acc, false, cp, n_clients, r32, nullptr, e0, sg.numel, coff, s32);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (e0 + j < sg.numel) st1(op + j, acc[j]);
}

// ---------------------------------------------------------------- MXFP8 updates into an fp32 aggregate
// flame_agg_reduce_mx: OCP e4m3fn / e5m2 client bytes (CD) with one E8M0 scale byte per 32 elements
// (OCP Microscaling v1.0), summed into an fp32 base.  An element's value is f32(q) * f32(scale), ONE
// fp32 multiply with denormals kept -- mx.dequantize's statement -- and from there the fp32
// reduction's own ops (Tr<FLAME_F32>), so the result is flame_agg_reduce[_scaled]'s over the
// dequantized update bit for bit.  The chunk is the clients': 4,096 elements (one 4,096-byte tile),
// a lane owns 16 of them = one 16-byte client vector, half a scale block, 16 fp32 accumulators and
// four 16-byte vectors of in / out.  A lane reads its block's scale byte itself, one byte load per
// client beside the vector load (two neighbouring lanes read the same byte; a wave's 32 bytes are
// one request).  One chunk per workgroup; 168 VGPRs (186 with SCALED) make that three workgroups per
// CU, not the 16-bit kernel's full residency.  SCALED as in agg_reduce_scaled_kernel.
#ifndef FLAME_T_CLIENT_UNROLL_MX
#define FLAME_T_CLIENT_UNROLL_MX 8
#endif
constexpr int kClientUnrollMx = FLAME_T_CLIENT_UNROLL_MX;   // clients whose loads are in flight per lane
// element decode: v_cvt_pk_f32_fp8 / _bf8 (1; OCP formats on gfx950 -- tests/test_gpu_mx.py runs all
// 256 x 256 (element, scale) pairs of both formats through it) or integer ALU (0; same bits, for A/B builds)
#ifndef FLAME_T_MX_HWCVT
#define FLAME_T_MX_HWCVT 1
#endif
constexpr bool kMxHwCvt = FLAME_T_MX_HWCVT != 0;
constexpr int kMxBlock = 32;         // elements per scale byte
constexpr int kMxEPT = 16;           // elements per lane: one 16-byte client vector

template <int CD> struct Mx;
template <> struct Mx<FLAME_FP8_E4M3> {
    // the four bytes of w, lowest first
    __device__ static void dec4(uint32_t w, float (&x)[4]) {
        if constexpr (kMxHwCvt) {
            const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), false);
            const f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), true);
            x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t b = (w >> (8 * j)) & 0xFFu, sign = (b & 0x80u) << 24, ex = (b >> 3) & 0xFu, man = b & 7u;
                uint32_t bits;
                if (ex == 15u && man == 7u) bits = 0x7FC00000u;                                 // the one NaN
                else if (ex == 0u) bits = __float_as_uint(static_cast<float>(man) * 0x1p-9f);   // subnormal: man * 2^-9, exact
                else bits = ((ex + 120u) << 23) | (man << 20);
                x[j] = __uint_as_float(bits | sign);
            }
        }
    }
};
template <> struct Mx<FLAME_FP8_E5M2> {
    __device__ static void dec4(uint32_t w, float (&x)[4]) {
        if constexpr (kMxHwCvt) {
            const f2 lo = __builtin_amdgcn_cvt_pk_f32_bf8(static_cast<int>(w), false);
            const f2 hi = __builtin_amdgcn_cvt_pk_f32_bf8(static_cast<int>(w), true);
            x[0] = lo.x; x[1] = lo.y; x[2] = hi.x; x[3] = hi.y;
        } else {
            // e5m2 is fp16's high byte: widen exactly
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = f16_to_f32(static_cast<uint16_t>(((w >> (8 * j)) & 0xFFu) << 8));
        }
    }
};
// E8M0: 2^(byte - 127); byte 0 is the fp32 subnormal 2^-127, byte 255 a NaN
__device__ __forceinline__ float e8m0_to_f32(uint32_t byte) {
    return __uint_as_float(byte == 255u ? 0x7FC00000u : byte == 0u ? 0x00400000u : byte << 23);
}

// reduce_clients' sibling: clients [0, n) of one lane's 16 elements into acc.  VEC: the client vector
// whole and aligned; else element by element with bounds, the scale index per element.
template <int CD, int CU, bool VEC, bool SCALED>
__device__ __forceinline__ void reduce_clients_mx(float (&acc)[kMxEPT], const uint64_t* __restrict__ cp,
                                                  const uint64_t* __restrict__ bsp, int n,
                                                  const float* __restrict__ r32, const float* __restrict__ s32,
                                                  int64_t e0, int64_t numel) {
    using F = Tr<FLAME_F32>;
    struct Ld { V16 q; uint32_t sb[VEC ? 1 : kMxEPT]; };
    auto load_client = [&](int c, Ld& l) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(cp[c]) + e0;
        const uint8_t* sp = reinterpret_cast<const uint8_t*>(bsp[c]);
        if constexpr (VEC) {
            l.q = ld_nt(p);
            l.sb[0] = ld1(sp + e0 / kMxBlock);
        } else {
            uint8_t b[kMxEPT];
#pragma unroll
            for (int j = 0; j < kMxEPT; ++j) {
                const bool in = e0 + j < numel;
                b[j] = in ? ld1(p + j) : uint8_t(0);
                l.sb[j] = in ? ld1(sp + (e0 + j) / kMxBlock) : 127u;
            }
            l.q = pack<uint8_t, kMxEPT>(b);
        }
    };
    auto combine = [&](int c, const Ld& l) {
        const float r = r32[c];
        float x[kMxEPT];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float d[4];
            Mx<CD>::dec4(l.q.w[w], d);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[4 * w + j] = d[j];
        }
#pragma unroll
        for (int j = 0; j < kMxEPT; ++j) {
            float v = __fmul_rn(x[j], e8m0_to_f32(l.sb[VEC ? 0 : j]));     // the update's value: one fp32 multiply
            if constexpr (SCALED) v = F::tmp(v, s32[c], 0.0);
            acc[j] = F::add(acc[j], F::tmp(v, r, 0.0));
        }
    };
    int i = 0;
    for (; i + CU <= n; i += CU) {
        Ld l[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) load_client(i + u, l[u]);
#pragma unroll
        for (int u = 0; u < CU; ++u) combine(i + u, l[u]);
    }
    for (; i < n; ++i) {
        Ld l;
        load_client(i, l);
        combine(i, l);
    }
}

template <int CD, int CU, bool SCALED>
__global__ __launch_bounds__(kBlock) void agg_reduce_mx_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                               const uint64_t* __restrict__ clients,
                                                               const uint64_t* __restrict__ block_scales, int n_clients,
                                                               const float* __restrict__ r32,
                                                               const float* __restrict__ s32, unsigned flags,
                                                               int64_t n_chunks) {
    static_assert(CD == FLAME_FP8_E4M3 || CD == FLAME_FP8_E5M2, "8-bit clients, one client vector per lane");
    constexpr int EPT = kMxEPT;             // 16 client bytes = 4 fp32 vectors of 4
    static_assert(kBlock * EPT == FLAME_TILE_BYTES && kMxBlock % EPT == 0, "a chunk is one tile; a lane stays inside one block");
    const int64_t chunk = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (chunk >= n_chunks) return;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const uint64_t* bsp = lc.row(block_scales, n_clients);
    const float* bp = reinterpret_cast<const float*>(sg.in) + e0;
    float* op = reinterpret_cast<float*>(sg.out) + e0;
    float acc[EPT];
    if (lc.vec()) {       // (the element-wise arm below through lane_load / lane_store moves registers: profiles/lane_isa_diff.log)
        lane_load<true>(bp, acc, e0, sg.numel);
        reduce_clients_mx<CD, CU, true, SCALED>(acc, cp, bsp, n_clients, r32, s32, e0, sg.numel);
        lane_store<true>(op, acc, e0, sg.numel);
        return;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = (e0 + j < sg.numel) ? ld1(bp + j) : 0.f;
    reduce_clients_mx<CD, 1, false, SCALED>(acc, cp, bsp, n_clients, r32, s32, e0, sg.numel);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (e0 + j < sg.numel) st1(op + j, acc[j]);
}

// ---------------------------------------------------------------- MXFP4 updates into an fp32 aggregate
// flame_agg_reduce_mxfp4: OCP e2m1 client nibbles, two per byte (flat element 2i the low nibble of
// byte i, 2i + 1 the high one), with one E8M0 scale byte per 32 elements, summed into an fp32 base.
// An element's value is f32_e2m1(code) * f32(scale), ONE fp32 multiply with denormals kept --
// mx.dequantize's statement -- and from there Tr<FLAME_F32>'s ops, as in the MXFP8 kernel.  The chunk
// is 8,192 elements (one 4,096-byte tile of client bytes): a lane owns 32 of them = one 16-byte client
// vector, exactly one scale block (no two lanes share a scale byte, and a lane's elements never
// straddle two), 32 fp32 accumulators and eight 16-byte vectors of in / out.  A segment starts a
// block, so e0 is a multiple of 32 on the element-wise arm as well: one scale byte per lane and
// client on both arms.  Register figures and residency: DESIGN.md §4.
#ifndef FLAME_T_CLIENT_UNROLL_MXFP4
#define FLAME_T_CLIENT_UNROLL_MXFP4 4
#endif
constexpr int kClientUnrollMx4 = FLAME_T_CLIENT_UNROLL_MXFP4;   // clients whose loads are in flight per lane
// element decode: v_cvt_scalef32_pk_f32_fp4, which decodes two nibbles and scales them in one instruction
// (1; tests/test_gpu_mxfp4.py runs all 256 x 256 (packed byte, scale byte) pairs through it: subnormal
// products, overflow, scale bytes 0 and 255, both zeros) or integer ALU and two fp32 products (0; same
// bits, for A/B builds)
#ifndef FLAME_T_MXFP4_HWCVT
#define FLAME_T_MXFP4_HWCVT 1
#endif
constexpr bool kMx4HwCvt = FLAME_T_MXFP4_HWCVT != 0;
constexpr int kMx4EPT = 32;          // elements per lane: one 16-byte client vector, one whole scale block

// The values of the eight nibbles of w (lowest first) times the block scale sf = f32_e8m0(byte).
// Hardware arm: byte k of w per instruction, low nibble first; the scale operand is sf itself.
// Integer arm: the code's three magnitude bits at fp32 bits 24..22 are e2m1's value times 2^-126
// (exponent field 0 is the fp32 subnormal 0 or 2^-127 = 0.5 * 2^-126, fields 1..3 carry 1 .. 6), so
// one exact product by 2^126 gives the element and the second is the contract's single rounding.
__device__ __forceinline__ void mxfp4_val8(uint32_t w, float sf, float (&x)[8]) {
    if constexpr (kMx4HwCvt) {
        const f2 b0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 0);
        const f2 b1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 1);
        const f2 b2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 2);
        const f2 b3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sf, 3);
        x[0] = b0.x; x[1] = b0.y; x[2] = b1.x; x[3] = b1.y; x[4] = b2.x; x[5] = b2.y; x[6] = b3.x; x[7] = b3.y;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t c = w >> (4 * k);
            const float q = __fmul_rn(__uint_as_float(((c & 7u) << 22) | ((c & 8u) << 28)), 0x1p126f);   // exact
            x[k] = __fmul_rn(q, sf);                                  // the update's value: one rounding
        }
    }
}

// reduce_clients_mx's sibling: clients [0, n) of one lane's kMx4EPT elements into acc.  VEC: the lane's
// client bytes whole and aligned; else byte by byte with bounds (a byte is read when its low nibble is
// an element; an odd numel's pad nibble lands in an accumulator that is never stored).
template <int CU, bool VEC, bool SCALED>
__device__ __forceinline__ void reduce_clients_mxfp4(float (&acc)[kMx4EPT], const uint64_t* __restrict__ cp,
                                                     const uint64_t* __restrict__ bsp, int n,
                                                     const float* __restrict__ r32, const float* __restrict__ s32,
                                                     int64_t e0, int64_t numel) {
    using F = Tr<FLAME_F32>;
    constexpr int NW = kMx4EPT / 8;          // 32-bit words of client nibbles per lane
    struct Ld { uint32_t q[NW]; uint32_t sb; };
    auto load_client = [&](int c, Ld& l) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(cp[c]) + (e0 >> 1);
        l.sb = ld1(reinterpret_cast<const uint8_t*>(bsp[c]) + e0 / kMxBlock);
        if constexpr (VEC) {
            const V16 v = ld_nt(p);
#pragma unroll
            for (int w = 0; w < NW; ++w) l.q[w] = v.w[w];
        } else {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                uint32_t q = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e0 + 8 * w + 2 * j < numel) q |= static_cast<uint32_t>(ld1(p + 4 * w + j)) << (8 * j);
                l.q[w] = q;
            }
        }
    };
    auto combine = [&](int c, const Ld& l) {
        const float r = r32[c];
        const float sf = e8m0_to_f32(l.sb);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            float x[8];
            mxfp4_val8(l.q[w], sf, x);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float v = x[k];
                if constexpr (SCALED) v = F::tmp(v, s32[c], 0.0);
                acc[8 * w + k] = F::add(acc[8 * w + k], F::tmp(v, r, 0.0));
            }
        }
    };
    int i = 0;
    for (; i + CU <= n; i += CU) {
        Ld l[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) load_client(i + u, l[u]);
#pragma unroll
        for (int u = 0; u < CU; ++u) combine(i + u, l[u]);
    }
    for (; i < n; ++i) {
        Ld l;
        load_client(i, l);
        combine(i, l);
    }
}

template <int CU, bool SCALED>
__global__ __launch_bounds__(kBlock) void agg_reduce_mxfp4_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                                  const uint64_t* __restrict__ clients,
                                                                  const uint64_t* __restrict__ block_scales, int n_clients,
                                                                  const float* __restrict__ r32,
                                                                  const float* __restrict__ s32, unsigned flags,
                                                                  int64_t n_chunks) {
    constexpr int EPT = kMx4EPT;            // 32 nibbles = 16 client bytes = 8 fp32 vectors of 4
    static_assert(EPT == kMxBlock && kBlock * EPT / 2 == FLAME_TILE_BYTES,
                  "a lane owns one block; a chunk is one tile of client bytes");
    const int64_t chunk = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (chunk >= n_chunks) return;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const uint64_t* bsp = lc.row(block_scales, n_clients);
    const float* bp = reinterpret_cast<const float*>(sg.in) + e0;
    float* op = reinterpret_cast<float*>(sg.out) + e0;
    float acc[EPT];
    if (lc.vec()) {
        lane_load<true>(bp, acc, e0, sg.numel);
        reduce_clients_mxfp4<CU, true, SCALED>(acc, cp, bsp, n_clients, r32, s32, e0, sg.numel);
        lane_store<true>(op, acc, e0, sg.numel);
        return;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = (e0 + j < sg.numel) ? ld1(bp + j) : 0.f;
    reduce_clients_mxfp4<1, false, SCALED>(acc, cp, bsp, n_clients, r32, s32, e0, sg.numel);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (e0 + j < sg.numel) st1(op + j, acc[j]);
}

// ---------------------------------------------------------------- trimmed mean / median
// Coordinate-wise trimmed mean (Yin et al., ICML 2018; flame has no counterpart file): per element
// the k smallest and the k largest of the n client values are dropped, the other n - 2k are summed
// in fp64 and divided (DESIGN.md §2 is the contract).  The order is -inf < .. < -0 < +0 < .. < +inf
// < NaN, taken on monotone integer keys -- never a floating-point min / max, whose minNum drops a
// NaN and duplicates its partner.  Selection streams over the clients in cache order: `lo` holds
// the k smallest keys seen so far, `hi` the k largest of what left `lo`; what leaves `hi` is kept.
// Both are sorted chains in registers, indexed only by unrolled constants.  A chain of capacity KT
// serves any k <= KT without a branch: stages j >= k start as pass-throughs (lo[j] the smallest
// key: min keeps it, max hands the arrival on unchanged; hi[j] the largest), stages j < k start
// full of the opposite extreme, so every stage is one integer min and one max per value.  (A
// wave-uniform `if (j < k)` per stage was built first: the merge behind each branch cost a third
// VALU op, a v_mov, per stage and value, and four more instructions per stage -- DESIGN.md §4.)  The
// client loop is peeled into its three phases (arrivals < k fill lo, arrivals < 2k fill hi, the
// rest emit), so the extremes the chains start with only ever fall out while nothing is kept: no
// sentinel is told apart from data.  The host picks the smallest instantiated KT >= k.
constexpr int kTrimMaxK = 16;
template <int V> using ic_ = std::integral_constant<int, V>;    // a phase as a compile-time argument
#ifndef FLAME_T_TRIM_UNROLL
#define FLAME_T_TRIM_UNROLL 8
#endif
#ifndef FLAME_T_TRIM_UNROLL_DEEP
#define FLAME_T_TRIM_UNROLL_DEEP 4
#endif
// client loads in flight per lane: fewer for the deep chains, which are VALU-bound
template <int KT> constexpr int trim_unroll() { return KT >= 8 ? FLAME_T_TRIM_UNROLL_DEEP : FLAME_T_TRIM_UNROLL; }

// Key traits.  R: one register's worth of keys (two 16-bit keys packed for bf16 / f16), NR of them
// per 16-byte lane vector.  keys(): the lane vector as keys, every NaN the all-ones key.
// add(): the keys decoded, widened to fp64 (exact) and added to the lane's accumulators; the
// all-ones key decodes to the quiet NaN 0x7f..f by the same inverse map as every other key.
template <int DT> struct TrimK;
template <> struct TrimK<FLAME_F32> {
    using R = uint32_t; static constexpr int NR = 4;
    __device__ static R lowest() { return 0u; }
    __device__ static R highest() { return ~0u; }
    __device__ static R kmin(R a, R b) { return a < b ? a : b; }
    __device__ static R kmax(R a, R b) { return a < b ? b : a; }
    __device__ static void keys(const V16& v, R (&k)[NR]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const uint32_t u = v.w[i];
            const uint32_t m = static_cast<uint32_t>(static_cast<int32_t>(u) >> 31) | 0x80000000u;
            k[i] = (u & 0x7FFFFFFFu) > 0x7F800000u ? ~0u : (u ^ m);
        }
    }
    __device__ static void add(const R (&k)[NR], double (&acc)[4]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const uint32_t m = ~static_cast<uint32_t>(static_cast<int32_t>(k[i]) >> 31) | 0x80000000u;
            acc[i] = __dadd_rn(acc[i], static_cast<double>(__uint_as_float(k[i] ^ m)));
        }
    }
};
template <> struct TrimK<FLAME_F64> {
    using R = uint64_t; static constexpr int NR = 2;
    __device__ static R lowest() { return 0ull; }
    __device__ static R highest() { return ~0ull; }
    __device__ static R kmin(R a, R b) { return a < b ? a : b; }
    __device__ static R kmax(R a, R b) { return a < b ? b : a; }
    __device__ static void keys(const V16& v, R (&k)[NR]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const uint64_t u = static_cast<uint64_t>(v.w[2 * i]) | (static_cast<uint64_t>(v.w[2 * i + 1]) << 32);
            const uint64_t m = static_cast<uint64_t>(static_cast<int64_t>(u) >> 63) | 0x8000000000000000ull;
            k[i] = (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? ~0ull : (u ^ m);
        }
    }
    __device__ static void add(const R (&k)[NR], double (&acc)[2]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const uint64_t m = ~static_cast<uint64_t>(static_cast<int64_t>(k[i]) >> 63) | 0x8000000000000000ull;
            acc[i] = __dadd_rn(acc[i], __longlong_as_double(static_cast<long long>(k[i] ^ m)));
        }
    }
};
// bf16 / f16: the same map on 16 bits, two keys per register (v_pk_min_u16 / v_pk_max_u16)
using ss2 = __attribute__((ext_vector_type(2))) short;
template <int DT> struct TrimK16 {
    using R = us2; static constexpr int NR = 4;
    static constexpr unsigned short kInf = DT == FLAME_BF16 ? 0x7F80 : 0x7C00;
    __device__ static R lowest() { return us2{0, 0}; }
    __device__ static R highest() { return us2{0xFFFF, 0xFFFF}; }
    __device__ static R kmin(R a, R b) { return __builtin_elementwise_min(a, b); }
    __device__ static R kmax(R a, R b) { return __builtin_elementwise_max(a, b); }
    __device__ static void keys(const V16& v, R (&k)[NR]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const us2 u = __builtin_bit_cast(us2, v.w[i]);
            const us2 m = __builtin_bit_cast(us2, __builtin_bit_cast(ss2, u) >> 15) | us2{0x8000, 0x8000};
            const us2 a = u & us2{0x7FFF, 0x7FFF};
            // a > inf <=> min(a, inf + 1) - min(a, inf) == 1; 0 - that is the all-ones mask of a NaN
            const us2 nan = us2{0, 0} - (__builtin_elementwise_min(a, us2{kInf + 1, kInf + 1}) -
                                         __builtin_elementwise_min(a, us2{kInf, kInf}));
            k[i] = (u ^ m) | nan;
        }
    }
    __device__ static void add(const R (&k)[NR], double (&acc)[8]) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const us2 m = ~__builtin_bit_cast(us2, __builtin_bit_cast(ss2, k[i]) >> 15) | us2{0x8000, 0x8000};
            const us2 h = k[i] ^ m;
            acc[2 * i] = __dadd_rn(acc[2 * i], static_cast<double>(Tr<DT>::ld(h.x)));
            acc[2 * i + 1] = __dadd_rn(acc[2 * i + 1], static_cast<double>(Tr<DT>::ld(h.y)));
        }
    }
};
template <> struct TrimK<FLAME_BF16> : TrimK16<FLAME_BF16> {};
template <> struct TrimK<FLAME_F16> : TrimK16<FLAME_F16> {};

// mean64 rounded to the dtype: f64 keeps it, f32 one RNE step, bf16 / f16 two (fp64 -> fp32 -> 16 bit)
template <int DT> __device__ __forceinline__ typename Tr<DT>::A trim_round(double m) {
    if constexpr (DT == FLAME_F64) return m;
    else if constexpr (DT == FLAME_F32) return __double2float_rn(m);
    else if constexpr (DT == FLAME_BF16) return bf16_round(__double2float_rn(m));
    else return f16_round(__double2float_rn(m));
}

// Clients [0, n) of one lane vector through the chains; acc takes the n - 2k kept values in the
// order they emerge.  VEC as in reduce_clients.
template <int DT, int KT, int CU, bool VEC>
__device__ __forceinline__ void trimmed_clients(double (&acc)[Tr<DT>::EPT], const uint64_t* __restrict__ cp, int n, int k,
                                                int64_t e0, int64_t numel, int64_t coff) {
    using X = Tr<DT>;
    using T = typename X::T;
    using K = TrimK<DT>;
    using R = typename K::R;
    constexpr int EPT = X::EPT, NR = K::NR;
    R lo[KT][NR], hi[KT][NR];
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            lo[j][r] = j < k ? K::highest() : K::lowest();
            hi[j][r] = j < k ? K::lowest() : K::highest();
        }
    auto load_client = [&](int c) -> V16 {
        T x[EPT];
        lane_load<VEC, true>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(cp[c]) + coff), x, e0, numel);
        return pack<T, EPT>(x);
    };
    // PHASE 0: into lo; 1: what leaves lo into hi; 2: what leaves hi is kept
    auto arrive = [&](auto phase, const V16& v) {
        constexpr int PHASE = decltype(phase)::value;
        R x[NR];
        K::keys(v, x);
#pragma unroll
        for (int j = 0; j < KT; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const R a = lo[j][r];
                lo[j][r] = K::kmin(a, x[r]);
                x[r] = K::kmax(a, x[r]);
            }
        if constexpr (PHASE >= 1) {
#pragma unroll
            for (int j = 0; j < KT; ++j)
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const R a = hi[j][r];
                    hi[j][r] = K::kmax(a, x[r]);
                    x[r] = K::kmin(a, x[r]);
                }
        }
        if constexpr (PHASE == 2) K::add(x, acc);
    };
    auto run = [&](auto phase, int i, int end) {
        for (; i + CU <= end; i += CU) {
            V16 v[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) v[u] = load_client(i + u);
#pragma unroll
            for (int u = 0; u < CU; ++u) arrive(phase, v[u]);
        }
        for (; i < end; ++i) arrive(phase, load_client(i));
    };
    run(ic_<0>{}, 0, k);
    run(ic_<1>{}, k, 2 * k);
    run(ic_<2>{}, 2 * k, n);
}

template <int DT, int KT>
__global__ __launch_bounds__(kBlock) void agg_trimmed_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                             const uint64_t* __restrict__ clients, int n_clients,
                                                             int trim_k, unsigned flags, int64_t n_chunks) {
    using X = Tr<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    const int64_t chunk = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (chunk >= n_chunks) return;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;
    const flame_segment& sg = lc.sg;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(T));
    const bool init_first = (flags & FLAME_AGG_INIT_FIRST) != 0;
    const bool vec = lc.vec();
    const double kept = static_cast<double>(n_clients - 2 * trim_k);
    const T* bp = reinterpret_cast<const T*>(sg.in) + lc.e0;
    T* op = reinterpret_cast<T*>(sg.out) + lc.e0;
    double acc[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = 0.0;
    // out = base + mean, one add in the dtype (torch-CPU's `base += mean`); INIT_FIRST: the mean.  (As one
    // function shared with agg_select_kernel both kernels' registers move: profiles/lane_isa_diff.log)
    auto result = [&](double a, T b) -> T {
        const A mean = trim_round<DT>(a / kept);
        return X::st(init_first ? mean : X::add(X::ld(b), mean));
    };
    if (vec) {
        trimmed_clients<DT, KT, trim_unroll<KT>(), true>(acc, cp, n_clients, trim_k, lc.e0, sg.numel, coff);
        T b[EPT], o[EPT];
        if (!init_first) unpack<T, EPT>(ld_v(bp), b);
#pragma unroll
        for (int j = 0; j < EPT; ++j) o[j] = result(acc[j], init_first ? T(0) : b[j]);
        st_v(op, pack<T, EPT>(o));
        return;
    }
    trimmed_clients<DT, KT, 1, false>(acc, cp, n_clients, trim_k, lc.e0, sg.numel, coff);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (lc.e0 + j < sg.numel) st1(op + j, result(acc[j], init_first ? T(0) : ld1(bp + j)));
}

// ---------------------------------------------------------------- trimmed mean / median by radix selection
// The same statement for any k (flame_agg_select; DESIGN.md §2 is the contract): the chains above
// hold 2k keys per element in registers and stop at k = 16.  Here a lane finds, per element, the
// two order statistics lo = sorted[k] and hi = sorted[n - k - 1] by an MSB-first radix search on the
// same integer keys, 4 bits per pass: every pass re-reads the chunk's n x 4 KiB (ordinary cached
// loads) and counts, per element, the digits of the keys that carry the prefix found so far; the
// digit at which the running count crosses the rank extends the prefix.  The counters are
// lane-private histograms in LDS, [bin][lane] with dword stride (bank = lane: no conflict, no
// atomic, no barrier), one array per element of the group so that the group's read-modify-writes
// are independent; a dword packs the count for lo's prefix (low half) and for hi's (high half),
// so a key costs one read-modify-write per element and a median's two ranks, whose prefixes
// agree almost to the end, share it.  16-bit counts bound n_clients by 65,535.  A group is 4
// elements (2 for f64): 4 arrays x 16 bins x 256 lanes x 4 B = 64 KiB; bf16 / f16 search their 8
// elements as two groups one after the other.  The last pass (nontemporal loads) adds the values
// strictly between lo and hi in client order and counts the ties at both ends; what the kept
// multiset holds of lo and hi enters as count x value.  Nothing depends on the launch geometry.
constexpr int kSelectMaxClients = 65535;
constexpr int kSelBins = 16;                     // 4-bit digits
#ifndef FLAME_T_SEL_UNROLL
#define FLAME_T_SEL_UNROLL 8
#endif

// The keys of TrimK<DT> one per register, and a key decoded and widened to fp64 (exact).
template <int DT> struct SelK {
    using U = std::conditional_t<DT == FLAME_F64, uint64_t, uint32_t>;
    static constexpr int BITS = DT == FLAME_F64 ? 64 : DT == FLAME_F32 ? 32 : 16;
    static constexpr int EPT = Tr<DT>::EPT;
    static constexpr int GE = EPT < 4 ? EPT : 4;     // elements searched side by side
    __device__ static void keys(const V16& v, U (&k)[EPT]) {
        using K = TrimK<DT>;
        typename K::R r[K::NR];
        K::keys(v, r);
        if constexpr (BITS == 16) {
#pragma unroll
            for (int i = 0; i < K::NR; ++i) {
                k[2 * i] = r[i].x;
                k[2 * i + 1] = r[i].y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < K::NR; ++i) k[i] = r[i];
        }
    }
    __device__ static double value(U k) {
        if constexpr (DT == FLAME_F64) {
            const uint64_t m = ~static_cast<uint64_t>(static_cast<int64_t>(k) >> 63) | 0x8000000000000000ull;
            return __longlong_as_double(static_cast<long long>(k ^ m));
        } else if constexpr (DT == FLAME_F32) {
            const uint32_t m = ~static_cast<uint32_t>(static_cast<int32_t>(k) >> 31) | 0x80000000u;
            return static_cast<double>(__uint_as_float(k ^ m));
        } else {
            const uint32_t m = (k & 0x8000u) ? 0x8000u : 0xFFFFu;
            return static_cast<double>(Tr<DT>::ld(static_cast<uint16_t>(k ^ m)));
        }
    }
};

// One lane vector of every client through the search and the summing pass; acc leaves as the fp64
// sum of the kept multiset.  h[j]: this lane's column of element j's histogram.  VEC as in
// reduce_clients.
template <int DT, bool VEC>
__device__ __forceinline__ void select_clients(double (&acc)[Tr<DT>::EPT], uint32_t* const (&h)[4],
                                               const uint64_t* __restrict__ cp, int n, int k, int64_t e0, int64_t numel,
                                               int64_t coff) {
    using X = Tr<DT>;
    using T = typename X::T;
    using S = SelK<DT>;
    using U = typename S::U;
    constexpr int EPT = X::EPT, GE = S::GE, NG = EPT / GE, CU = FLAME_T_SEL_UNROLL;
    auto load_client = [&](int c, auto last) -> V16 {
        T x[EPT];
        lane_load<VEC, decltype(last)::value != 0>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(cp[c]) + coff), x,
                                                   e0, numel);
        return pack<T, EPT>(x);
    };
    auto each_client = [&](auto last, auto&& f) {
        int i = 0;
        for (; i + CU <= n; i += CU) {
            V16 v[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) v[u] = load_client(i + u, last);
#pragma unroll
            for (int u = 0; u < CU; ++u) f(v[u]);
        }
        for (; i < n; ++i) f(load_client(i, last));
    };
    U klo[EPT], khi[EPT];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        U ulo[GE], uhi[GE];                          // the prefixes found so far, right-aligned
        uint32_t rlo[GE], rhi[GE];                   // the ranks among the keys that carry them
#pragma unroll
        for (int j = 0; j < GE; ++j) {
            ulo[j] = uhi[j] = 0;
            rlo[j] = static_cast<uint32_t>(k);
            rhi[j] = static_cast<uint32_t>(n - k - 1);
        }
#pragma unroll 1
        for (int shift = S::BITS - 4; shift >= 0; shift -= 4) {
#pragma unroll
            for (int b = 0; b < kSelBins; ++b)
#pragma unroll
                for (int j = 0; j < GE; ++j) h[j][b * kBlock] = 0u;
            each_client(ic_<0>{}, [&](const V16& v) {
                U key[EPT];
                S::keys(v, key);
#pragma unroll
                for (int j = 0; j < GE; ++j) {
                    const U hb = key[g * GE + j] >> shift;
                    const uint32_t d = static_cast<uint32_t>(hb) & (kSelBins - 1);
                    const U up = hb >> 4;
                    h[j][d * kBlock] += (up == ulo[j] ? 1u : 0u) | (up == uhi[j] ? 0x10000u : 0u);
                }
            });
            // the digit: the number of bins whose running count stays at or below the rank
#pragma unroll
            for (int j = 0; j < GE; ++j) {
                uint32_t cl = 0, ch = 0, dl = 0, dh = 0, bl = 0, bh = 0;
#pragma unroll
                for (int b = 0; b < kSelBins; ++b) {
                    const uint32_t w = h[j][b * kBlock];
                    cl += w & 0xFFFFu;
                    ch += w >> 16;
                    const bool tl = cl <= rlo[j], th = ch <= rhi[j];
                    dl += tl;
                    dh += th;
                    bl = tl ? cl : bl;
                    bh = th ? ch : bh;
                }
                ulo[j] = (ulo[j] << 4) | dl;
                uhi[j] = (uhi[j] << 4) | dh;
                rlo[j] -= bl;
                rhi[j] -= bh;
            }
        }
#pragma unroll
        for (int j = 0; j < GE; ++j) {
            klo[g * GE + j] = ulo[j];
            khi[g * GE + j] = uhi[j];
        }
    }
    // the summing pass: strictly-inside values in client order; the ties at lo and hi are counted
    uint32_t nle[EPT], nge[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) nle[j] = nge[j] = 0;
    each_client(ic_<1>{}, [&](const V16& v) {
        U key[EPT];
        S::keys(v, key);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            nle[j] += key[j] <= klo[j];
            nge[j] += key[j] >= khi[j];
            const double s = __dadd_rn(acc[j], S::value(key[j]));
            acc[j] = (klo[j] < key[j] && key[j] < khi[j]) ? s : acc[j];
        }
    });
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const bool one = klo[j] == khi[j];
        const double c_lo = static_cast<double>(one ? static_cast<uint32_t>(n - 2 * k) : nle[j] - static_cast<uint32_t>(k));
        const double c_hi = static_cast<double>(nge[j] - static_cast<uint32_t>(k));
        acc[j] = __dadd_rn(acc[j], __dmul_rn(c_lo, S::value(klo[j])));
        const double t = __dadd_rn(acc[j], __dmul_rn(c_hi, S::value(khi[j])));
        acc[j] = one ? acc[j] : t;
    }
}

template <int DT>
__global__ __launch_bounds__(kBlock) void agg_select_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                            const uint64_t* __restrict__ clients, int n_clients,
                                                            int trim_k, unsigned flags, int64_t n_chunks) {
    using X = Tr<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    __shared__ uint32_t h0[kSelBins * kBlock], h1[kSelBins * kBlock], h2[kSelBins * kBlock], h3[kSelBins * kBlock];
    static_assert(4 * sizeof(h0) <= 64 * 1024, "agg_select_kernel: the histograms exceed 64 KiB");
    const int64_t chunk = wg_slot(flags & FLAME_AGG_XCD_MAP);
    if (chunk >= n_chunks) return;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;                          // no barrier below: the histograms are lane-private
    const flame_segment& sg = lc.sg;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(T));
    const bool init_first = (flags & FLAME_AGG_INIT_FIRST) != 0;
    const bool vec = lc.vec();
    const double kept = static_cast<double>(n_clients - 2 * trim_k);
    const T* bp = reinterpret_cast<const T*>(sg.in) + lc.e0;
    T* op = reinterpret_cast<T*>(sg.out) + lc.e0;
    uint32_t* const h[4] = {h0 + threadIdx.x, h1 + threadIdx.x, h2 + threadIdx.x, h3 + threadIdx.x};
    double acc[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = 0.0;
    auto result = [&](double a, T b) -> T {          // as agg_trimmed_kernel's
        const A mean = trim_round<DT>(a / kept);
        return X::st(init_first ? mean : X::add(X::ld(b), mean));
    };
    if (vec) {
        select_clients<DT, true>(acc, h, cp, n_clients, trim_k, lc.e0, sg.numel, coff);
        T b[EPT], o[EPT];
        if (!init_first) unpack<T, EPT>(ld_v(bp), b);
#pragma unroll
        for (int j = 0; j < EPT; ++j) o[j] = result(acc[j], init_first ? T(0) : b[j]);
        st_v(op, pack<T, EPT>(o));
        return;
    }
    select_clients<DT, false>(acc, h, cp, n_clients, trim_k, lc.e0, sg.numel, coff);
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (lc.e0 + j < sg.numel) st1(op + j, result(acc[j], init_first ? T(0) : ld1(bp + j)));
}

// ---------------------------------------------------------------- update statistics (update guard)
// Per client: the sum of squares of its finite elements and the count of its non-finite ones, over
// every segment (differential_privacy.py:68-76 is the norm this feeds).  The only kernel that
// reduces ALONG an update.  A workgroup owns kStatR consecutive chunks; clients are the outer loop,
// so a lane carries one fp64 accumulator per client across its kStatR x 16 bytes and the workgroup
// reduces once per client: lane partials, a wave reduction (lanes 32, 16, .. 1 apart), the four
// wave sums added in wave order, one partial per (client, workgroup) into the caller's scratch.
// update_stats_finish_kernel adds a client's partials in a fixed order.  No floating-point atomic
// anywhere, so equal launches give equal bits.  Every element is widened to fp64 before the square
// (exact for f32 / bf16 / f16, so their square-and-add is one fma without changing a bit; fp64
// squares round once, then add).
#ifndef FLAME_T_STAT_R
#define FLAME_T_STAT_R 8
#endif
constexpr int kStatR = FLAME_T_STAT_R;           // consecutive chunks per workgroup
#ifndef FLAME_T_STAT_UNROLL
#define FLAME_T_STAT_UNROLL 8
#endif
constexpr int kStatUnroll = FLAME_T_STAT_UNROLL; // chunk loads in flight per lane
#ifndef FLAME_T_STAT_CB
#define FLAME_T_STAT_CB 8
#endif
constexpr int kStatCB = FLAME_T_STAT_CB;         // clients a lane accumulates side by side (their loads issued together)
constexpr int kStatBatch = 64;                   // clients whose wave sums share the LDS block
static_assert(kStatCB >= 1 && kStatBatch % kStatCB == 0, "the LDS block holds whole client groups");
constexpr int kWaves = kBlock / 64;
constexpr int64_t kChunkBytes = 4096;            // one chunk of every dtype (= FLAME_TILE_BYTES)
static_assert(kWaves == 4, "the statistics kernels add four wave sums");

// CEN (flame_update_dist): the term is the square of x - z, one fp64 subtract of the widened
// values, and stays 0 for a non-finite x whatever z is; a non-finite z propagates.  With z = +-0
// the subtract returns x (or a zero), so every bit below is the statistics'.
template <int DT, bool CEN>
__device__ __forceinline__ void stat_elem(typename Tr<DT>::T x, typename Tr<DT>::T z, double& acc, unsigned& bad) {
    if constexpr (DT == FLAME_F64) {
        const bool nf = !__builtin_isfinite(x);
        const double d = CEN ? __dsub_rn(x, z) : x;
        acc = __dadd_rn(acc, nf ? 0.0 : __dmul_rn(d, d));
        bad += nf;
    } else {
        const float f = Tr<DT>::ld(x);
        const bool nf = !__builtin_isfinite(f);
        double d = static_cast<double>(nf ? 0.0f : f);
        if constexpr (CEN) d = nf ? 0.0 : __dsub_rn(d, static_cast<double>(Tr<DT>::ld(z)));
        acc = __builtin_fma(d, d, acc);      // d * d is exact in fp64: the same bits as multiply, then add
        bad += nf;                           // (CEN: d has up to 53 bits, the fma rounds once)
    }
}
template <int DT, bool CEN>
__device__ __forceinline__ void stat_vec(const V16& v, const V16& zv, double& acc, unsigned& bad) {
    using T = typename Tr<DT>::T;
    T x[Tr<DT>::EPT], z[Tr<DT>::EPT];
    unpack<T, Tr<DT>::EPT>(v, x);
    unpack<T, Tr<DT>::EPT>(CEN ? zv : v, z);
#pragma unroll
    for (int j = 0; j < Tr<DT>::EPT; ++j) stat_elem<DT, CEN>(x[j], z[j], acc, bad);
}
// lane 0 receives the wave's sum, always added in the same order
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = __dadd_rn(x, __shfl_down(x, d, 64));
    return x;
}

// One pass of a workgroup over its chunks [c0, c1) for NC clients (cfirst ..): per chunk the NC
// clients' vectors are loaded together (on a tiled slab they are one contiguous NC x 4 KiB run),
// CU chunks per step.  All bounds are workgroup-uniform.  CEN: the segment's centre (segs[s].in,
// contiguous, numel elements) is read beside them, once per chunk and client group -- after the
// first group out of L2, which a workgroup's kStatR x 4 KiB never leave between groups.
template <int DT, int NC, int CU, bool CEN>
__device__ __forceinline__ void stat_pass(const flame_segment* __restrict__ segs, int n_segs, int s0, int64_t c0,
                                          int64_t c1, const uint64_t* __restrict__ clients, int n_clients, int cfirst,
                                          double (&acc)[NC], unsigned (&bad)[NC]) {
    using T = typename Tr<DT>::T;
    constexpr int EPT = Tr<DT>::EPT;
    constexpr int64_t CE = chunk_elems<DT>();
    static_assert(CE * sizeof(T) == kChunkBytes, "a chunk is 4 KiB of every dtype");
    const int64_t lane_elem = static_cast<int64_t>(threadIdx.x) * EPT;
    int64_t chunk = c0;
    // the segments that meet [c0, c1), in order
#pragma unroll 1
    for (int s = s0; s < n_segs && chunk < c1; ++s) {
        const int64_t numel = segs[s].numel, begin = segs[s].chunk_begin;
        if (numel <= 0) continue;
        int64_t end = begin + (numel + CE - 1) / CE;
        if (end > c1) end = c1;
        if (chunk < begin) chunk = begin;
        if (chunk >= end) continue;
        const int64_t tstride = segs[s].client_tile_stride;
        const int64_t step = tstride ? tstride : kChunkBytes;
        int64_t cl = chunk - begin;
        const int64_t cle = end - begin;
        // whole, aligned chunks take the vector path; the tail chunk and misaligned views go
        // element by element with bounds
        int64_t clf = (segs[s].flags & FLAME_SEG_UNALIGNED) ? cl : numel / CE;
        if (clf > cle) clf = cle;
        const uint64_t* cp = clients + static_cast<int64_t>(s) * n_clients + cfirst;
        const int64_t loff = lane_elem * static_cast<int64_t>(sizeof(T));
        const char* q[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) q[k] = reinterpret_cast<const char*>(cp[k]) + cl * step + loff;
        // the centre's bytes for this lane: chunk cl of the segment is at zb + cl * 4 KiB
        const char* const zb = CEN ? static_cast<const char*>(segs[s].in) + loff : nullptr;
        int64_t off = 0;
        for (; cl + CU <= clf; cl += CU, off += CU * step) {
            V16 x[CU][NC], z[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                if constexpr (CEN) z[u] = ld_v(zb + (cl + u) * kChunkBytes);
#pragma unroll
                for (int k = 0; k < NC; ++k) x[u][k] = ld_nt(q[k] + off + u * step);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u)
#pragma unroll
                for (int k = 0; k < NC; ++k) stat_vec<DT, CEN>(x[u][k], z[u], acc[k], bad[k]);
        }
        for (; cl < clf; ++cl, off += step) {
            V16 x[NC], z;
            if constexpr (CEN) z = ld_v(zb + cl * kChunkBytes);
#pragma unroll
            for (int k = 0; k < NC; ++k) x[k] = ld_nt(q[k] + off);
#pragma unroll
            for (int k = 0; k < NC; ++k) stat_vec<DT, CEN>(x[k], z, acc[k], bad[k]);
        }
        for (; cl < cle; ++cl, off += step) {
            const int64_t e = cl * CE + lane_elem;
            T z[EPT];
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                z[j] = (CEN && e + j < numel) ? ld1(reinterpret_cast<const T*>(zb + cl * kChunkBytes) + j) : T();
#pragma unroll
            for (int k = 0; k < NC; ++k)
#pragma unroll
                for (int j = 0; j < EPT; ++j)
                    if (e + j < numel)
                        stat_elem<DT, CEN>(ld1(reinterpret_cast<const T*>(q[k] + off) + j), z[j], acc[k], bad[k]);
        }
        chunk = end;
    }
}

template <int DT, bool CEN>
__global__ __launch_bounds__(kBlock) void update_stats_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                              const uint64_t* __restrict__ clients, int n_clients,
                                                              int64_t n_chunks, int64_t n_wg,
                                                              double* __restrict__ scratch,
                                                              unsigned long long* __restrict__ nonfinite) {
    __shared__ double wsum[kWaves][kStatBatch];
    const int64_t c0 = static_cast<int64_t>(blockIdx.x) * kStatR;
    const int64_t c1 = c0 + kStatR < n_chunks ? c0 + kStatR : n_chunks;
    const int s0 = find_segment(segs, n_segs, c0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // one client's lane partials -> its wave sums in LDS, its non-finite count added to the output
    auto commit = [&](int ci, int c, double acc, unsigned bad) {
        acc = wave_sum(acc);
        if (lane == 0) wsum[wave][ci] = acc;
        if (__any(bad != 0)) {          // rare: integer counts may use an atomic
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) bad += __shfl_down(bad, d, 64);
            if (lane == 0) atomicAdd(nonfinite + c, static_cast<unsigned long long>(bad));
        }
    };
#pragma unroll 1
    for (int cb = 0; cb < n_clients; cb += kStatBatch) {
        const int nb = n_clients - cb < kStatBatch ? n_clients - cb : kStatBatch;
        int ci = 0;
        if constexpr (kStatCB > 1) {
#pragma unroll 1
            for (; ci + kStatCB <= nb; ci += kStatCB) {
                double acc[kStatCB];
                unsigned bad[kStatCB];
#pragma unroll
                for (int k = 0; k < kStatCB; ++k) acc[k] = 0.0, bad[k] = 0;
                stat_pass<DT, kStatCB, (kStatUnroll / kStatCB > 1 ? kStatUnroll / kStatCB : 1), CEN>(
                    segs, n_segs, s0, c0, c1, clients, n_clients, cb + ci, acc, bad);
#pragma unroll
                for (int k = 0; k < kStatCB; ++k) commit(ci + k, cb + ci + k, acc[k], bad[k]);
            }
        }
#pragma unroll 1
        for (; ci < nb; ++ci) {         // the clients left over, one at a time
            double acc[1] = {0.0};
            unsigned bad[1] = {0};
            stat_pass<DT, 1, kStatUnroll, CEN>(segs, n_segs, s0, c0, c1, clients, n_clients, cb + ci, acc, bad);
            commit(ci, cb + ci, acc[0], bad[0]);
        }
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < nb) {
            const int t_ci = threadIdx.x;
            const double t = __dadd_rn(__dadd_rn(__dadd_rn(wsum[0][t_ci], wsum[1][t_ci]), wsum[2][t_ci]), wsum[3][t_ci]);
            st1(scratch + static_cast<int64_t>(cb + t_ci) * n_wg + blockIdx.x, t);
        }
        __syncthreads();
    }
}

// sumsq[c] += the n_wg partials of client c: lane t adds partials t, t + 256, .. in index order,
// then the same wave and workgroup order as above
__global__ __launch_bounds__(kBlock) void update_stats_finish_kernel(const double* __restrict__ scratch, int64_t n_wg,
                                                                     double* __restrict__ sumsq) {
    __shared__ double wsum[kWaves];
    const double* row = scratch + static_cast<int64_t>(blockIdx.x) * n_wg;
    double acc = 0.0;
    for (int64_t w = threadIdx.x; w < n_wg; w += kBlock) acc = __dadd_rn(acc, ld1(row + w));
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = __dadd_rn(__dadd_rn(__dadd_rn(wsum[0], wsum[1]), wsum[2]), wsum[3]);
        st1(sumsq + blockIdx.x, __dadd_rn(ld1(sumsq + blockIdx.x), t));
    }
}

// ---------------------------------------------------------------- pairwise Gram (Multi-Krum)
// G[i][j] = sum over every element of s(x_i) * s(x_j), s = stat_elem's sanitising (finite ? x : 0,
// widened to fp64), on the fp64 matrix cores: v_mfma_f64_16x16x4_f64.  Clients go in blocks of 16
// and tiles of kGramTile = 64.  A workgroup owns one tile pair (I <= J) over a range of chunks;
// wave w owns the 16-client row block 16 w of tile I against the four column blocks of tile J: four
// double4 accumulators.  Lane (c = lane & 15, g = lane >> 4) loads 16 bytes of client c at byte
// 64 t + 16 g of the chunk, t = 0 .. 63: EPT elements, hence EPT k-steps whose k index is g -- A is
// A[row = lane & 15][k = lane >> 4], B is B[k = lane >> 4][col = lane & 15], one double per lane,
// so a client's vector is the A operand of its row block and the B operand of its column block
// with no lane movement, and on a diagonal block they are the same registers.  The k order is the
// same for every pair of clients, which is all a dot product needs.  Clients past n_clients and
// elements past numel enter as 0.0 and are never read.  fp32 x fp32, bf16 x bf16 and fp16 x fp16
// products are exact in fp64: the accumulation is the only rounding.
// The C/D map of the f64 instruction is col = lane & 15, row = (lane >> 4) + 4 * reg (NOT the f32
// map); gram_finish_kernel is the only place that reads it.  Each workgroup stores its 64 x 64
// partial in register order (16 doubles per lane, coalesced) into the caller's scratch; the finish
// kernel adds a tile pair's partials in a fixed order and writes both triangles from the upper one.
// No floating-point atomic anywhere.  The non-finite count is taken by the diagonal workgroups
// (each client's elements pass there exactly once as an A operand).
constexpr int kGramTile = 64;                    // clients per tile: 4 waves x 16 rows, 4 column blocks
constexpr int kGramMaxClients = 1024;
constexpr int kGramPart = kGramTile * kGramTile; // doubles per partial
#ifndef FLAME_T_GRAM_MIN_R
#define FLAME_T_GRAM_MIN_R 4
#endif
constexpr int64_t kGramMinR = FLAME_T_GRAM_MIN_R;       // fewest chunks per workgroup (a 32 KiB partial each)
#ifndef FLAME_T_GRAM_TARGET_WG
#define FLAME_T_GRAM_TARGET_WG 2048
#endif
constexpr int64_t kGramTargetWG = FLAME_T_GRAM_TARGET_WG; // workgroups a launch aims at (8 per CU)
#ifndef FLAME_T_GRAM_UNROLL
#define FLAME_T_GRAM_UNROLL 2
#endif
constexpr int kGramUnroll = FLAME_T_GRAM_UNROLL;         // 64-byte steps whose loads are issued together
static_assert(64 % kGramUnroll == 0, "a chunk is 64 steps of 64 bytes");
using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int64_t gram_tiles(int n_clients) { return (n_clients + kGramTile - 1) / kGramTile; }
constexpr int64_t gram_pairs(int n_clients) { return gram_tiles(n_clients) * (gram_tiles(n_clients) + 1) / 2; }
// chunks per workgroup: at least kGramMinR, and so many that pairs x ranges stays near kGramTargetWG
inline int64_t gram_range(int64_t n_chunks, int n_clients) {
    const int64_t r = (n_chunks * gram_pairs(n_clients) + kGramTargetWG - 1) / kGramTargetWG;
    return r > kGramMinR ? r : kGramMinR;
}

// 16 bytes of one client: the vector load, or (tail chunk, misaligned view) element loads with
// bounds, zero bits past numel; no load at all for a client past the table (p == nullptr)
template <int DT>
__device__ __forceinline__ V16 gram_load(const char* p, bool vec, int64_t e, int64_t numel) {
    using T = typename Tr<DT>::T;
    constexpr int EPT = Tr<DT>::EPT;
    V16 r;
    r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0;
    if (p == nullptr) return r;
    if (vec) return ld_nt(p);
    T x[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) x[j] = e + j < numel ? ld1(reinterpret_cast<const T*>(p) + j) : T(0);
    return pack<T, EPT>(x);
}
// sanitise (finite ? x : 0), count, widen
template <int DT>
__device__ __forceinline__ void gram_widen(const V16& v, double (&d)[Tr<DT>::EPT], unsigned& bad) {
    using T = typename Tr<DT>::T;
    constexpr int EPT = Tr<DT>::EPT;
    T x[EPT];
    unpack<T, EPT>(v, x);
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        if constexpr (DT == FLAME_F64) {
            const bool nf = !__builtin_isfinite(x[j]);
            d[j] = nf ? 0.0 : x[j];
            bad += nf;
        } else {
            const float f = Tr<DT>::ld(x[j]);
            const bool nf = !__builtin_isfinite(f);
            d[j] = static_cast<double>(nf ? 0.0f : f);
            bad += nf;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(kBlock) void update_gram_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                             const uint64_t* __restrict__ clients, int n_clients,
                                                             int64_t n_chunks, int64_t range, int n_pairs,
                                                             double* __restrict__ scratch,
                                                             unsigned long long* __restrict__ nonfinite) {
    using T = typename Tr<DT>::T;
    constexpr int EPT = Tr<DT>::EPT;
    constexpr int64_t CE = chunk_elems<DT>();
    static_assert(CE * sizeof(T) == kChunkBytes, "a chunk is 4 KiB of every dtype");
    // tile pair (I <= J) of this workgroup: pairs are numbered row by row of the upper triangle
    const int tiles = static_cast<int>(gram_tiles(n_clients));
    int I = 0, rem = blockIdx.x;
    while (rem >= tiles - I) rem -= tiles - I, ++I;
    const int J = I + rem;
    const bool diag = I == J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * range;
    const int64_t c1 = c0 + range < n_chunks ? c0 + range : n_chunks;
    const int arow = I * kGramTile + 16 * wave + c;          // this lane's A client
    const bool wave_on = I * kGramTile + 16 * wave < n_clients;          // wave-uniform
    int nb = (n_clients - J * kGramTile + 15) / 16;          // column blocks of tile J that hold clients
    if (nb > 4) nb = 4;
    d4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
    unsigned bad = 0;
    if (wave_on) {
        int64_t chunk = c0;
#pragma unroll 1
        for (int s = find_segment(segs, n_segs, c0); s < n_segs && chunk < c1; ++s) {
            const int64_t numel = segs[s].numel, begin = segs[s].chunk_begin;
            if (numel <= 0) continue;
            int64_t end = begin + (numel + CE - 1) / CE;
            if (end > c1) end = c1;
            if (chunk < begin) chunk = begin;
            if (chunk >= end) continue;
            const int64_t tstride = segs[s].client_tile_stride;
            const int64_t step = tstride ? tstride : kChunkBytes;
            const int64_t full = (segs[s].flags & FLAME_SEG_UNALIGNED) ? 0 : numel / CE;   // chunks [0, full) are whole and aligned
            const uint64_t* cp = clients + static_cast<int64_t>(s) * n_clients;
            const char* pa = arow < n_clients ? reinterpret_cast<const char*>(ld1(cp + arow)) : nullptr;
            const char* pb[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = J * kGramTile + 16 * b + c;
                pb[b] = (b < nb && col < n_clients) ? reinterpret_cast<const char*>(ld1(cp + col)) : nullptr;
            }
#pragma unroll 1
            for (int64_t cl = chunk - begin; cl < end - begin; ++cl) {
                const bool vec = cl < full;                   // workgroup-uniform
                const int64_t coff = cl * step + 16 * g;
                const int64_t e0 = cl * CE + g * EPT;
#pragma unroll 1
                for (int t = 0; t < 64; t += kGramUnroll) {
                    V16 ra[kGramUnroll], rb[kGramUnroll][4];
#pragma unroll
                    for (int u = 0; u < kGramUnroll; ++u) {
                        const int64_t off = coff + 64 * (t + u);
                        const int64_t e = e0 + 4 * EPT * (t + u);
                        ra[u] = gram_load<DT>(pa ? pa + off : nullptr, vec, e, numel);
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (b < nb && !(diag && b == wave)) rb[u][b] = gram_load<DT>(pb[b] ? pb[b] + off : nullptr, vec, e, numel);
                    }
#pragma unroll
                    for (int u = 0; u < kGramUnroll; ++u) {
                        double da[EPT];
                        gram_widen<DT>(ra[u], da, bad);
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            if (b >= nb) continue;            // wave-uniform
                            if (diag && b == wave) {          // wave-uniform: A and B are the same registers
#pragma unroll
                                for (int j = 0; j < EPT; ++j)
                                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[j], da[j], acc[b], 0, 0, 0);
                            } else {
                                double db[EPT];
                                unsigned ignored = 0;
                                gram_widen<DT>(rb[u][b], db, ignored);
#pragma unroll
                                for (int j = 0; j < EPT; ++j)
                                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[j], db[j], acc[b], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            chunk = end;
        }
    }
    // the partial, in register order: entry k = 4 b + reg of lane `threadIdx.x`
    double* part = scratch + (static_cast<int64_t>(blockIdx.y) * n_pairs + blockIdx.x) * kGramPart;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) st1(part + (4 * b + r) * kBlock + threadIdx.x, acc[b][r]);
    if (diag && __any(bad != 0)) {      // rare: integer counts may use an atomic
        bad += __shfl_xor(bad, 16, 64);          // the four lanes of a client
        bad += __shfl_xor(bad, 32, 64);
        if (g == 0 && bad != 0 && arow < n_clients) atomicAdd(nonfinite + arow, static_cast<unsigned long long>(bad));
    }
}

// gram[i][j] (and [j][i]) += a tile pair's partials.  A workgroup owns 64 consecutive entries of
// the pair's 4,096 (blockIdx.y); wave s adds the partials of ranges s, s + 4, .. in index order (a
// wave's load is 512 contiguous bytes), then the four wave sums are added in wave order: a fixed
// order whatever the launch, and one workgroup per pair no longer walks every partial alone (64 x
// 25M fp32 has one pair and 2,035 partials).  Entry e = 256 k + t is what lane t of the Gram
// workgroup held as k = 4 b + reg: row 16 (t >> 6) + ((t & 63) >> 4) + 4 reg and column
// 16 b + (t & 15) of the tile pair -- the f64 instruction's C/D map.  A diagonal tile writes from
// its upper triangle only, so both triangles are the same bits.
constexpr int kGramFinishSplit = kGramPart / 64;     // workgroups per tile pair
__global__ __launch_bounds__(kBlock) void gram_finish_kernel(const double* __restrict__ scratch, int64_t n_ranges,
                                                             int n_pairs, int n_clients, double* __restrict__ gram) {
    __shared__ double wsum[kWaves][64];
    const int tiles = static_cast<int>(gram_tiles(n_clients));
    int I = 0, rem = blockIdx.x;
    while (rem >= tiles - I) rem -= tiles - I, ++I;
    const int J = I + rem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = static_cast<int>(blockIdx.y) * 64 + lane;
    const int64_t stride = static_cast<int64_t>(n_pairs) * kGramPart;
    const double* p = scratch + static_cast<int64_t>(blockIdx.x) * kGramPart + e;
    double sum = 0.0;
#pragma unroll 8
    for (int64_t r = wave; r < n_ranges; r += kWaves) sum = __dadd_rn(sum, ld1(p + r * stride));
    wsum[wave][lane] = sum;
    __syncthreads();
    if (wave != 0) return;
    const int k = e >> 8, t = e & 255;
    const int i = I * kGramTile + 16 * (t >> 6) + ((t & 63) >> 4) + 4 * (k & 3);
    const int j = J * kGramTile + 16 * (k >> 2) + (t & 15);
    if (i >= n_clients || j >= n_clients || i > j) return;
    const double total = __dadd_rn(__dadd_rn(__dadd_rn(wsum[0][lane], wsum[1][lane]), wsum[2][lane]), wsum[3][lane]);
    double* up = gram + static_cast<int64_t>(i) * n_clients + j;
    const double v = __dadd_rn(ld1(up), total);
    st1(up, v);
    if (i != j) st1(gram + static_cast<int64_t>(j) * n_clients + i, v);
}

// ---------------------------------------------------------------- fused FedOPT (fp32)
__device__ __forceinline__ float sign_f(float x) {  // torch.sign: NaN -> 0, -0 -> 0
    if constexpr (kYogiSelect) {
        // +-1 with x's sign where x is ordered and nonzero (one v_cmp_lg_f32 + one v_bfi_b32),
        // else +0: the same value as the integer difference below, in 3 instructions instead of 6
        return __builtin_islessgreater(x, 0.0f) ? __builtin_copysignf(1.0f, x) : 0.0f;
    } else {
        return static_cast<float>((0.0f < x) - (x < 0.0f));
    }
}

// Per-dtype rounding after each reference op (identity for fp32; RNE to bf16 / fp16).
template <int DT> __device__ __forceinline__ float rnd(float x) {
    if constexpr (DT == FLAME_BF16) return bf16_round(x);
    else if constexpr (DT == FLAME_F16) return f16_round(x);
    else return x;
}

// fedopt.py:106-129 (+ the _delta_v variants) up to the square root: d, the new m and v, and
// the numerator eta * m, each torch op rounded in the tensor's dtype.
template <int DT, int VARIANT>
__device__ __forceinline__ void adapt_moments(float avg, float cur, float& m, float& v, float& num, float b1,
                                              float omb1, float b2, float omb2, float eta) {
    const float d = rnd<DT>(__fsub_rn(avg, cur));
    const float mn = rnd<DT>(__fadd_rn(rnd<DT>(__fmul_rn(b1, m)), rnd<DT>(__fmul_rn(omb1, d))));
    const float d2 = rnd<DT>(__fmul_rn(d, d));
    float vn;
    if constexpr (VARIANT == FLAME_FEDADAM) {
        vn = rnd<DT>(__fadd_rn(rnd<DT>(__fmul_rn(b2, v)), rnd<DT>(__fmul_rn(omb2, d2))));
    } else if constexpr (VARIANT == FLAME_FEDYOGI) {
        const float t = rnd<DT>(__fmul_rn(omb2, d2));
        vn = rnd<DT>(__fsub_rn(v, rnd<DT>(__fmul_rn(t, sign_f(rnd<DT>(__fsub_rn(v, d2)))))));
    } else {
        vn = rnd<DT>(__fadd_rn(v, d2));
    }
    m = mn;
    v = vn;
    num = rnd<DT>(__fmul_rn(eta, mn));
}

// One element of fedopt.py:106-129, each torch op rounded in the tensor's dtype.  `tau` arrives
// pre-rounded to the dtype for bf16/fp16 (torch-CPU rounds a Python scalar to a reduced-precision
// tensor's dtype before + and -, not before * and /).  The general correctly rounded sqrt and
// divide (__builtin_sqrtf is correctly rounded; the __fsqrt_rn builtin lowers to the 1-ulp
// v_sqrt_f32): the scalar tail path, and adapt_vec's fallback.
template <int DT, int VARIANT>
__device__ __forceinline__ void adapt_elem(float avg, float cur, float& m, float& v, float& cur_out,
                                           float b1, float omb1, float b2, float omb2, float eta, float tau) {
    float num;
    adapt_moments<DT, VARIANT>(avg, cur, m, v, num, b1, omb1, b2, omb2, eta);
    const float den = rnd<DT>(__fadd_rn(rnd<DT>(__builtin_sqrtf(v)), tau));
    cur_out = rnd<DT>(__fadd_rn(cur, rnd<DT>(__fdiv_rn(num, den))));
}

// A lane's EPT elements of one adaptive step (cur_is_avg: current IS the average, d = 0).  When
// the lane's operands are all in the range fastmath.h admits -- v in [+0, 2^78], eta*m = +-0 or
// 2^-85 <= |.| <= 2^100, tau in [2^-20, 2^38] (so sqrt(v) + tau is in [2^-20, 2^40]) -- the
// square root and the divide take flame_fm::sqrt_rn / div_rn (rsq / rcp seeds, packed fma), else
// the general sequences.  Both give the same m, v and current (tools/fp_probe.py), so which one a
// lane takes never shows in the results.
// bf16 (a lane's 8 elements as 4 pairs): adapt_vec's op sequence with every fp32 op on a pair
// (v_pk_mul_f32 / v_pk_add_f32) and every bf16 rounding one instruction (bf16_rnd1).  Admitted
// lanes take v_sqrt_f32 and num * v_rcp_f32(den) for the correctly rounded root and quotient: both
// are within 2 fp32 ulps of the exact value, and the exact root of a bf16 v, and the exact quotient
// of two bf16 values, are never within 2^-18 (relative) of a bf16 rounding midpoint (8-bit
// significands), so the bf16 rounding of either equals the bf16 rounding of the correctly rounded
// fp32 value (v_sqrt_f32 flushes a subnormal v to a zero root, but den = RN(RN(root) + tau) = tau
// for both roots there).  tools/fp_probe.py checks the root on every normal bf16 v, den on every
// admitted v and the quotient on every admitted (num, den) pair.
// fp16: the same sequence with f16_rnd2 (one v_cvt_pk_f16_f32 + two widening converts per pair).
// An fp16 significand has 11 bits, too many for the midpoint argument; the exhaustive fp16 probe
// of tools/fp_probe.py finds v_sqrt_f32 exact under the fp16 rounding on every finite v (so the
// root takes it, FLAME_T_F16_HWROOT) but num * v_rcp_f32 not (the quotient stays div_rn).
// The pair rounding (inline asm: never on a transcendental's result) and the single rounding the
// compiler builds (safe on one) of the 16-bit dtypes.
template <int DT> __device__ __forceinline__ f2 hrnd2(f2 x) {
    if constexpr (DT == FLAME_BF16) return bf16_rnd2(x);
    else return f16_rnd2(x);
}
template <int DT> __device__ __forceinline__ float hrnd1(float x) {
    if constexpr (DT == FLAME_BF16) return bf16_round(x);
    else return f16_round(x);
}

template <int DT, int VARIANT>
__device__ __forceinline__ void adapt_vec_half(const float (&avg)[8], const float (&cur)[8], bool cur_is_avg,
                                               float (&m)[8], float (&v)[8], float (&cur_out)[8], float b1,
                                               float omb1, float b2, float omb2, float eta, float tau) {
    float c[8], num[8];
#pragma unroll
    for (int p = 0; p < 8; p += 2) {
        const f2 a = {avg[p], avg[p + 1]};
        const f2 cc = cur_is_avg ? a : f2{cur[p], cur[p + 1]};
        const f2 d = hrnd2<DT>(a - cc);
        const f2 mn = hrnd2<DT>(hrnd2<DT>(splat2(b1) * f2{m[p], m[p + 1]}) + hrnd2<DT>(splat2(omb1) * d));
        const f2 d2 = hrnd2<DT>(d * d);
        const f2 vo = {v[p], v[p + 1]};
        f2 vn;
        if constexpr (VARIANT == FLAME_FEDADAM) {
            vn = hrnd2<DT>(hrnd2<DT>(splat2(b2) * vo) + hrnd2<DT>(splat2(omb2) * d2));
        } else if constexpr (VARIANT == FLAME_FEDYOGI) {
            const f2 t = hrnd2<DT>(splat2(omb2) * d2);
            const f2 x = hrnd2<DT>(vo - d2);
            // t * sign(x) needs no rounding of its own: t is in the dtype and the sign +-1 or +0, so
            // the product is +-t or +-0 exactly (a NaN stays a NaN; its payload bits are not pinned)
            vn = hrnd2<DT>(vo - t * f2{sign_f(x.x), sign_f(x.y)});
        } else {
            vn = hrnd2<DT>(vo + d2);
        }
        const f2 nm = hrnd2<DT>(splat2(eta) * mn);
        c[p] = cc.x;
        c[p + 1] = cc.y;
        m[p] = mn.x;
        m[p + 1] = mn.y;
        v[p] = vn.x;
        v[p + 1] = vn.y;
        num[p] = nm.x;
        num[p + 1] = nm.y;
    }
    bool adm;
    if constexpr (!kHalfAdmit) adm = flame_fm::admits<8>(v, num);
    else if constexpr (DT == FLAME_BF16) adm = flame_fm::admits_v<8>(v);
    else adm = flame_fm::admits_v<8>(v) & flame_fm::admits_finite<8>(num) & (tau <= 0x1p15f);  // den finite in fp16
    const bool ok = (tau >= 0x1p-20f) & (tau <= 0x1p38f) & adm;
    if (ok) {
        constexpr bool hw_root = DT == FLAME_BF16 || kF16HwRoot;
        constexpr bool hw_div = DT == FLAME_BF16;
#pragma unroll
        for (int p = 0; p < 8; p += 2) {
            // the roots' rounding through hrnd1: a v_sqrt_f32 / v_rsq_f32 result never feeds inline asm
            f2 s, q;
            if constexpr (hw_root) {
                s = f2{hrnd1<DT>(__builtin_amdgcn_sqrtf(v[p])), hrnd1<DT>(__builtin_amdgcn_sqrtf(v[p + 1]))};
            } else {
                s = f2{hrnd1<DT>(flame_fm::sqrt_rn(v[p])), hrnd1<DT>(flame_fm::sqrt_rn(v[p + 1]))};
            }
            const f2 den = hrnd2<DT>(s + splat2(tau));
            if constexpr (hw_div) {
                q = hrnd2<DT>(f2{num[p], num[p + 1]} * f2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)});
            } else {
                q = hrnd2<DT>(f2{flame_fm::div_rn(num[p], den.x), flame_fm::div_rn(num[p + 1], den.y)});
            }
            const f2 co = hrnd2<DT>(f2{c[p], c[p + 1]} + q);
            cur_out[p] = co.x;
            cur_out[p + 1] = co.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float den = hrnd1<DT>(__fadd_rn(hrnd1<DT>(__builtin_sqrtf(v[j])), tau));
            cur_out[j] = hrnd1<DT>(__fadd_rn(c[j], hrnd1<DT>(__fdiv_rn(num[j], den))));
        }
    }
}

template <int DT, int VARIANT, int EPT>
__device__ __forceinline__ void adapt_vec(const float (&avg)[EPT], const float (&cur)[EPT], bool cur_is_avg,
                                          float (&m)[EPT], float (&v)[EPT], float (&cur_out)[EPT], float b1,
                                          float omb1, float b2, float omb2, float eta, float tau) {
    if constexpr (EPT == 8 && ((DT == FLAME_BF16 && kBf16Packed) || (DT == FLAME_F16 && kF16Packed))) {
        adapt_vec_half<DT, VARIANT>(avg, cur, cur_is_avg, m, v, cur_out, b1, omb1, b2, omb2, eta, tau);
        return;
    }
    float c[EPT], num[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        c[j] = cur_is_avg ? avg[j] : cur[j];
        adapt_moments<DT, VARIANT>(avg[j], c[j], m[j], v[j], num[j], b1, omb1, b2, omb2, eta);
    }
    const bool ok = (tau >= 0x1p-20f) & (tau <= 0x1p38f) & flame_fm::admits<EPT>(v, num);
    if (ok) {         // per lane (exec-masked; a wave whose lanes all agree runs one side only)
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const float den = rnd<DT>(__fadd_rn(rnd<DT>(flame_fm::sqrt_rn(v[j])), tau));
            cur_out[j] = rnd<DT>(__fadd_rn(c[j], rnd<DT>(flame_fm::div_rn(num[j], den))));
        }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const float den = rnd<DT>(__fadd_rn(rnd<DT>(__builtin_sqrtf(v[j])), tau));
            cur_out[j] = rnd<DT>(__fadd_rn(c[j], rnd<DT>(__fdiv_rn(num[j], den))));
        }
    }
}

// One chunk of a FedOPT round.  held != nullptr: a full-vector chunk leaves its avg / m / v /
// cur blocks in LDS (held[o * kBlock + lane], o = avg, m, v, cur) for the caller
// to store, and returns true; otherwise everything is stored here and it returns false.
template <int DT, int VARIANT, int CU>
__device__ __forceinline__ bool fedopt_chunk(const flame_segment* __restrict__ segs, int n_segs, int64_t chunk,
                                             const uint64_t* __restrict__ clients, int n_clients,
                                             const float* __restrict__ r32, unsigned flags, float b1,
                                             float omb1, float b2, float omb2, float eta, float tau,
                                             V16* held) {
    using X = Tr<DT>;
    using T = typename X::T;
    constexpr int EPT = X::EPT;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return false;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(T));
    const bool zero_state = (flags & FLAME_OPT_STATE_ZERO) != 0;
    const bool cur_avg = (sg.flags & FLAME_SEG_CUR_IS_AVG) != 0;   // cur IS the FedAvg result
    const bool vec = lc.vec();
    float acc[EPT];
    const T* base = reinterpret_cast<const T*>(sg.in) + e0;
    const T* curp = reinterpret_cast<const T*>(sg.cur) + e0;
    T* mp = reinterpret_cast<T*>(sg.m) + e0;
    T* vp = reinterpret_cast<T*>(sg.v) + e0;
    T* ap = sg.out ? reinterpret_cast<T*>(sg.out) + e0 : nullptr;
    T* cop = reinterpret_cast<T*>(sg.cur_out) + e0;
    if (vec) {
        T b[EPT];
        unpack<T, EPT>(ld_v(base), b);
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = X::ld(b[j]);
        reduce_clients<DT, CU, true>(acc, false, cp, n_clients, r32, nullptr, e0, sg.numel, coff);
        // A one-trip loop on purpose: written as straight-line code with an early return the step
        // compiles to a different schedule, measured 2 % slower on config 4 (DESIGN.md §4,
        // profiles/vpt_isa_diff.log); with the loop the listing is the one that was tuned.
#pragma unroll
        for (int once = 0; once < 1; ++once) {
            T cur_t[EPT], m_t[EPT], v_t[EPT], avg_o[EPT], m_o[EPT], v_o[EPT], c_o[EPT];
            if (!cur_avg) unpack<T, EPT>(ld_v(curp), cur_t);
            if (!zero_state) {
                unpack<T, EPT>(ld_v(mp), m_t);
                unpack<T, EPT>(ld_v(vp), v_t);
            }
            float cf[EPT], mf[EPT], vf[EPT], co[EPT];
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                cf[j] = cur_avg ? 0.f : X::ld(cur_t[j]);
                mf[j] = zero_state ? 0.f : X::ld(m_t[j]);
                vf[j] = zero_state ? 0.f : X::ld(v_t[j]);
            }
            adapt_vec<DT, VARIANT, EPT>(acc, cf, cur_avg, mf, vf, co, b1, omb1, b2, omb2, eta, tau);
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                avg_o[j] = X::st(acc[j]);
                m_o[j] = X::st(mf[j]);
                v_o[j] = X::st(vf[j]);
                c_o[j] = X::st(co[j]);
            }
            if (held) {
                V16* h = held + threadIdx.x;
                h[0 * kBlock] = pack<T, EPT>(avg_o);
                h[1 * kBlock] = pack<T, EPT>(m_o);
                h[2 * kBlock] = pack<T, EPT>(v_o);
                h[3 * kBlock] = pack<T, EPT>(c_o);
                continue;
            }
            if (ap) st_v(ap, pack<T, EPT>(avg_o));
            st_v(mp, pack<T, EPT>(m_o));
            st_v(vp, pack<T, EPT>(v_o));
            st_v(cop, pack<T, EPT>(c_o));
        }
        return held != nullptr;
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j)
            acc[j] = (e0 + j < sg.numel) ? X::ld(ld1(base + j)) : 0.f;
        reduce_clients<DT, 1, false>(acc, false, cp, n_clients, r32, nullptr, e0, sg.numel, coff);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if (e0 + j >= sg.numel) continue;
            float mj = zero_state ? 0.f : X::ld(ld1(mp + j)), vj = zero_state ? 0.f : X::ld(ld1(vp + j)), cj;
            adapt_elem<DT, VARIANT>(acc[j], cur_avg ? acc[j] : X::ld(ld1(curp + j)), mj, vj, cj, b1, omb1,
                                    b2, omb2, eta, tau);
            if (ap) st1(ap + j, X::st(acc[j]));
            st1(mp + j, X::st(mj));
            st1(vp + j, X::st(vj));
            st1(cop + j, X::st(cj));
        }
    }
    return false;
}

// G = 1: one chunk per workgroup, stored as computed.  G > 1: G consecutive chunks per
// workgroup, their outputs held in LDS and stored together at the end (kOptWGC).
template <int DT, int VARIANT, int CU, int G>
__device__ __forceinline__ void fedopt_body(const flame_segment* __restrict__ segs, int n_segs,
                                            const uint64_t* __restrict__ clients, int n_clients,
                                            const float* __restrict__ r32, unsigned flags, float b1,
                                            float omb1, float b2, float omb2, float eta, float tau,
                                            int64_t n_chunks) {
    const int64_t wg = wg_slot(flags & FLAME_OPT_XCD_MAP);
    if constexpr (G == 1) {
        (void)n_chunks;
        fedopt_chunk<DT, VARIANT, CU>(segs, n_segs, wg, clients, n_clients, r32, flags, b1, omb1, b2,
                                      omb2, eta, tau, nullptr);
    } else {
        using T = typename Tr<DT>::T;
        static_assert(G * 4 * kBlock * sizeof(V16) <= 160 * 1024, "kOptWGC: outputs exceed the LDS");
        __shared__ V16 held[G * 4 * kBlock];
        unsigned pending = 0;
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            const int64_t chunk = wg * G + g;
            if (chunk >= n_chunks) break;
            if (fedopt_chunk<DT, VARIANT, CU>(segs, n_segs, chunk, clients, n_clients, r32, flags, b1, omb1, b2, omb2,
                                              eta, tau, held + g * 4 * kBlock))
                pending |= 1u << g;
        }
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            if (!(pending >> g & 1u)) continue;
            const LaneChunk<flame_segment, Tr<DT>::EPT> lc(segs, n_segs, wg * G + g);
            const flame_segment sg = lc.sg;
            const int64_t e0 = lc.e0;
            T* outs[4] = {sg.out ? reinterpret_cast<T*>(sg.out) + e0 : nullptr, reinterpret_cast<T*>(sg.m) + e0,
                          reinterpret_cast<T*>(sg.v) + e0, reinterpret_cast<T*>(sg.cur_out) + e0};
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (!outs[o]) continue;
                st_v(outs[o], held[(g * 4 + o) * kBlock + threadIdx.x]);
            }
        }
    }
}

template <int DT, int VARIANT, int CU, int G>
__global__ __launch_bounds__(kBlock) void fedopt_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                        const uint64_t* __restrict__ clients, int n_clients,
                                                        const float* __restrict__ r32, unsigned flags, float b1,
                                                        float omb1, float b2, float omb2, float eta, float tau,
                                                        int64_t n_chunks) {
    fedopt_body<DT, VARIANT, CU, G>(segs, n_segs, clients, n_clients, r32, flags, b1, omb1, b2, omb2, eta, tau,
                                    n_chunks);
}

// The same with the metadata block as a kernel argument, read in place (flame_fedopt_reduce_adapt_argmeta;
// see agg_reduce_kernel_argmeta).  Word offsets: client table at off_clients, fp32 rates at off_r32.
template <int DT, int VARIANT, int CU, int G>
__global__ __launch_bounds__(kBlock) void fedopt_kernel_argmeta(const ArgMeta meta, int n_segs, int n_clients,
                                                                int off_clients, int off_r32, unsigned flags,
                                                                float b1, float omb1, float b2, float omb2,
                                                                float eta, float tau, int64_t n_chunks) {
    (void)sizeof(meta);
    const uint64_t* w = (const uint64_t*)__builtin_amdgcn_kernarg_segment_ptr();
    fedopt_body<DT, VARIANT, CU, G>(reinterpret_cast<const flame_segment*>(w), n_segs, w + off_clients, n_clients,
                                    off_r32 >= 0 ? reinterpret_cast<const float*>(w + off_r32) : nullptr, flags,
                                    b1, omb1, b2, omb2, eta, tau, n_chunks);
}

// ---------------------------------------------------------------- eager FedOPT chain
// The eager top aggregator's round (eager_syncfl/top_aggregator.py:36-90) calls do() once per
// arrival: FedAvg of that arrival into the round's base (fedavg.py:93-104), then one adaptive
// step from the optimizer's state (fedopt.py:102-129).  This kernel runs a queue of such calls in
// one pass.  Per element, for each client i in arrival order:
//   b = b + tmp(w_i, r_i)
//   where client i closes a do() call (step_end[i] != 0): d = b - c, m / v / c updated as
//   adapt_elem (c = b for the first step when the segment is flagged FLAME_SEG_CUR_IS_AVG:
//   current_weights IS the base right after the round-1 passthrough).
// Base, current, m and v are read once and base, m, v and the new current written once, instead
// of every arrival's launch reading and writing all four.  Bitwise equal to those launches: every
// value held in registers between steps is already rounded to the dtype (each op rounds), so it
// equals what the per-arrival launches store and reload.
// step_end[i] through a SCALAR load: the aligned dword holding byte i (never outside the page
// that holds it), so the per-step test is an s_load + scalar branch, not a vector byte load whose
// s_waitcnt vmcnt(0) would also wait for the batch's client loads in flight.
__device__ __forceinline__ bool step_ends(const uint8_t* __restrict__ step_end, int i) {
    using kptr = const __attribute__((address_space(4))) uint32_t*;    // constant: scalar loads
    const uintptr_t a = reinterpret_cast<uintptr_t>(step_end) + static_cast<uintptr_t>(i);
    const uint32_t w = *reinterpret_cast<kptr>(a & ~static_cast<uintptr_t>(3));
    return ((w >> ((a & 3u) * 8u)) & 0xffu) != 0u;
}

// VEC: the workgroup's whole chunk is inside the segment and aligned, so every lane's loads are
// unconditional 16-byte vectors and the batch's loads are waited for one by one
// (s_waitcnt vmcnt(CU - 1 - u)) instead of all at once.
template <int DT, int VARIANT, int CU, bool VEC>
__device__ __forceinline__ void fedopt_chain_body(const flame_segment& sg, int64_t e0, const uint64_t* __restrict__ cp,
                                                  int64_t coff, int n_clients, const float* __restrict__ r32,
                                                  const uint8_t* __restrict__ step_end, unsigned flags, float b1,
                                                  float omb1, float b2, float omb2, float eta, float tau) {
    using X = Tr<DT>;
    using T = typename X::T;
    constexpr int EPT = X::EPT;
    const int nv = VEC ? EPT : static_cast<int>(sg.numel - e0 < EPT ? sg.numel - e0 : EPT);   // (not lane_load: lane_isa_diff.log)
    bool aliased = (sg.flags & FLAME_SEG_CUR_IS_AVG) != 0;
    const bool zero_state = (flags & FLAME_OPT_STATE_ZERO) != 0;
    const T* bp = reinterpret_cast<const T*>(sg.in) + e0;
    const T* curp = reinterpret_cast<const T*>(sg.cur) + e0;
    T* mp = reinterpret_cast<T*>(sg.m) + e0;
    T* vp = reinterpret_cast<T*>(sg.v) + e0;
    auto load_t = [&](const T* p, T (&x)[EPT], bool nt) {
        if constexpr (VEC) {
            unpack<T, EPT>(nt ? ld_nt(p) : ld_v(p), x);
        } else {
#pragma unroll
            for (int j = 0; j < EPT; ++j) x[j] = j < nv ? ld1(p + j) : T(0);
        }
    };
    auto load_f = [&](const T* p, float (&x)[EPT]) {
        T t[EPT];
        load_t(p, t, false);
#pragma unroll
        for (int j = 0; j < EPT; ++j) x[j] = X::ld(t[j]);
    };
    float b[EPT], c[EPT] = {}, m[EPT], v[EPT];
    load_f(bp, b);
    if (!aliased) load_f(curp, c);
    if (zero_state) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) m[j] = v[j] = 0.f;
    } else {
        load_f(mp, m);
        load_f(vp, v);
    }
    auto load_client = [&](int i, T (&x)[EPT]) {
        load_t(reinterpret_cast<const T*>(reinterpret_cast<const char*>(cp[i]) + coff), x, true);
    };
    auto arrive = [&](const T (&x)[EPT], float r, bool ends) {
        if constexpr ((DT == FLAME_BF16 && kBf16Packed) || (DT == FLAME_F16 && kF16Packed)) {
#pragma unroll
            for (int j = 0; j < EPT; j += 2) {     // X::add(b, X::tmp(x, r)) on pairs
                const f2 t = hrnd2<DT>(f2{X::ld(x[j]), X::ld(x[j + 1])} * splat2(r));
                const f2 s = hrnd2<DT>(f2{b[j], b[j + 1]} + t);
                b[j] = s.x;
                b[j + 1] = s.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < EPT; ++j) b[j] = X::add(b[j], X::tmp(x[j], r, 0.0));
        }
        if (ends) {     // uniform: one do() call ends here
            if (__builtin_expect(aliased, 0)) {   // the first step after the passthrough: current IS base
#pragma unroll
                for (int j = 0; j < EPT; ++j) c[j] = b[j];
                aliased = false;
            }
            adapt_vec<DT, VARIANT, EPT>(b, c, false, m, v, c, b1, omb1, b2, omb2, eta, tau);
        }
    };
    auto load_batch = [&](int i0, T (&x)[CU][EPT], float (&rr)[CU], bool (&ends)[CU]) {
#pragma unroll
        for (int u = 0; u < CU; ++u) load_client(i0 + u, x[u]);
#pragma unroll
        for (int u = 0; u < CU; ++u) {     // the batch's scalar loads issued together, one wait
            rr[u] = r32[i0 + u];
            ends[u] = step_ends(step_end, i0 + u);
        }
    };
    auto run_batch = [&](const T (&x)[CU][EPT], const float (&rr)[CU], const bool (&ends)[CU]) {
#pragma unroll
        for (int u = 0; u < CU; ++u) arrive(x[u], rr[u], ends[u]);
    };
    int i = 0;
    // (Two register batches -- the next batch's loads issued before this one's steps -- run no
    // faster: 1.294 vs 1.287 ms at 8 loads per batch, 1.457 at 12, 3.40 at 16 (two 64-register
    // batches); one process, bitwise, profiles/r05k_chain_pipe_ab.log.  Nor do two or four
    // chunks per lane -- twice / four times the independent step chains: 1.38-1.44 vs 1.378 ms,
    // profiles/r05o_chain_ev_ab.log -- nor 2 / 3 / 4 chunks per workgroup with their outputs burst
    // from LDS: 1.386 / 1.417 / 1.372 vs 1.370 ms, profiles/r05w_chain_wgc_ab.log.  Three resident
    // workgroups of the plain batch loop already overlap one another's loads and arithmetic.)
    for (; i + CU <= n_clients; i += CU) {
        T x[CU][EPT];
        float rr[CU];
        bool ends[CU];
        load_batch(i, x, rr, ends);
        run_batch(x, rr, ends);
    }
    for (; i < n_clients; ++i) {
        T x[EPT];
        load_client(i, x);
        arrive(x, r32[i], step_ends(step_end, i));
    }
    if (aliased) {             // no step closed: current is still the base
#pragma unroll
        for (int j = 0; j < EPT; ++j) c[j] = b[j];
    }
    T* outs[4] = {reinterpret_cast<T*>(sg.out) + e0, mp, vp, reinterpret_cast<T*>(sg.cur_out) + e0};
    const float* vals[4] = {b, m, v, c};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        T t[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) t[j] = X::st(vals[o][j]);
        if constexpr (VEC) {
            st_v(outs[o], pack<T, EPT>(t));
        } else {
            for (int j = 0; j < nv; ++j) st1(outs[o] + j, t[j]);
        }
    }
}

// fedopt_chain_body for an fp16 model on a full, aligned chunk: the same per-arrival accumulate and
// per-call step (fedopt.py:102-129, each torch op rounded to fp16), with the lane's 8 elements held
// as 4 packed pairs.  An op whose operands are both fp16 is one packed fp16 instruction (same bits
// as fp32-then-fp16, see h2 above); a product with a Python scalar is smul_h2; the root and the
// quotient widen their operands and take v_sqrt_f32 / flame_fm::div_rn as adapt_vec_half does
// (same admission: v in [+0, 65504] per half, a finite numerator, tau in [2^-20, 2^15]); a lane
// outside it takes the general sequence per element.
template <int VARIANT, int CU>
__device__ __forceinline__ void fedopt_chain_body_f16(const flame_segment& sg, int64_t e0, const uint64_t* __restrict__ cp,
                                                      int64_t coff, int n_clients, const float* __restrict__ r32,
                                                      const uint8_t* __restrict__ step_end, unsigned flags, float b1,
                                                      float omb1, float b2, float omb2, float eta, float tau) {
    bool aliased = (sg.flags & FLAME_SEG_CUR_IS_AVG) != 0;
    const bool zero_state = (flags & FLAME_OPT_STATE_ZERO) != 0;
    const uint16_t* bp = reinterpret_cast<const uint16_t*>(sg.in) + e0;
    const uint16_t* curp = reinterpret_cast<const uint16_t*>(sg.cur) + e0;
    uint16_t* mp = reinterpret_cast<uint16_t*>(sg.m) + e0;
    uint16_t* vp = reinterpret_cast<uint16_t*>(sg.v) + e0;
    uint32_t b[4], c[4] = {}, m[4] = {}, v[4] = {};
    auto ld4 = [](const void* p, uint32_t (&x)[4]) {
        const V16 t = ld_v(p);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = t.w[q];
    };
    ld4(bp, b);
    if (!aliased) ld4(curp, c);
    if (!zero_state) {
        ld4(mp, m);
        ld4(vp, v);
    }
    const h2 tau2 = {static_cast<_Float16>(tau), static_cast<_Float16>(tau)};   // tau is fp16-exact
    const bool tau_ok = (tau >= 0x1p-20f) & (tau <= 0x1p15f);                   // den in [2^-20, 65504]
    auto adapt = [&]() {
        uint32_t num[4];
        us2 vmax = {0, 0};
        bool fin = true;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const h2 d = h2_of(b[p]) - h2_of(c[p]);
            const h2 mn = h2_of(smul_h2(b1, m[p])) + h2_of(smul_h2(omb1, u_of(d)));
            const h2 d2 = d * d;
            const h2 vo = h2_of(v[p]);
            h2 vn;
            if constexpr (VARIANT == FLAME_FEDADAM) {
                vn = h2_of(smul_h2(b2, v[p])) + h2_of(smul_h2(omb2, u_of(d2)));
            } else if constexpr (VARIANT == FLAME_FEDYOGI) {
                const h2 t = h2_of(smul_h2(omb2, u_of(d2)));
                vn = vo - t * sign_h2(vo - d2);      // t * (+-1 or +0) is exact (omb2 >= 0, see sign_h2)
            } else {
                vn = vo + d2;
            }
            m[p] = u_of(mn);
            v[p] = u_of(vn);
            float plo, phi;
            num[p] = smul_h2(eta, m[p], plo, phi);
            vmax = __builtin_elementwise_max(vmax, __builtin_bit_cast(us2, v[p]));
            // compares (lane masks), not fmaxf: an fmaxf of an inline-asm result costs a
            // canonicalizing max first
            fin &= (__builtin_fabsf(plo) < 65520.f) & (__builtin_fabsf(phi) < 65520.f);
        }
        // v's halves in [+0, 65504] (a sign, an inf or a NaN is above 0x7bff); every numerator
        // finite: its fp32 product below 65520, the fp16 overflow threshold (a NaN product fails the
        // compare: that lane takes the general sequence, which gives the same NaN)
        const bool ok = tau_ok & (max(vmax.x, vmax.y) <= 0x7bffu) & fin;
        if (ok) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                h2 s;
                if constexpr (kF16HalfRoot) {
                    s = __builtin_elementwise_sqrt(h2_of(v[p]));      // v_sqrt_f16 (tools/fp_probe.py)
                } else {
                    const f2 vv = widen_h2(v[p]);
                    s = h2{static_cast<_Float16>(__builtin_amdgcn_sqrtf(vv.x)),
                           static_cast<_Float16>(__builtin_amdgcn_sqrtf(vv.y))};
                }
                const f2 den = widen_h2(u_of(s + tau2));
                const f2 q = {div_rn_h<0>(num[p], den.x), div_rn_h<1>(num[p], den.y)};
                c[p] = u_of(h2_of(c[p]) + h2_of(pk_h2(q)));
            }
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const f2 vv = widen_h2(v[p]), cc = widen_h2(c[p]), nn = widen_h2(num[p]);
                float co[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float den = f16_round(__fadd_rn(f16_round(__builtin_sqrtf(vv[h])), tau));
                    co[h] = f16_round(__fadd_rn(cc[h], f16_round(__fdiv_rn(nn[h], den))));
                }
                c[p] = u_of(h2{static_cast<_Float16>(co[0]), static_cast<_Float16>(co[1])});   // exact
            }
        }
    };
    auto arrive = [&](const V16& x, float r, bool ends) {
#pragma unroll
        for (int p = 0; p < 4; ++p) b[p] = u_of(h2_of(b[p]) + h2_of(smul_h2(r, x.w[p])));
        if (ends) {     // uniform: one do() call ends here
            if (__builtin_expect(aliased, 0)) {   // the first step after the passthrough: current IS base
#pragma unroll
                for (int p = 0; p < 4; ++p) c[p] = b[p];
                aliased = false;
            }
            adapt();
        }
    };
    auto client = [&](int i) { return reinterpret_cast<const char*>(cp[i]) + coff; };
    int i = 0;
    for (; i + CU <= n_clients; i += CU) {
        V16 x[CU];
        float rr[CU];
        bool ends[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) x[u] = ld_nt(client(i + u));
#pragma unroll
        for (int u = 0; u < CU; ++u) {
            rr[u] = r32[i + u];
            ends[u] = step_ends(step_end, i + u);
        }
#pragma unroll
        for (int u = 0; u < CU; ++u) arrive(x[u], rr[u], ends[u]);
    }
    for (; i < n_clients; ++i) arrive(ld_nt(client(i)), r32[i], step_ends(step_end, i));
    if (aliased) {             // no step closed: current is still the base
#pragma unroll
        for (int p = 0; p < 4; ++p) c[p] = b[p];
    }
    auto st4 = [](void* p, const uint32_t (&x)[4]) {
        V16 t;
#pragma unroll
        for (int q = 0; q < 4; ++q) t.w[q] = x[q];
        st_v(p, t);
    };
    st4(reinterpret_cast<uint16_t*>(sg.out) + e0, b);
    st4(mp, m);
    st4(vp, v);
    st4(reinterpret_cast<uint16_t*>(sg.cur_out) + e0, c);
}

template <int DT, int VARIANT, int CU>
__global__ __launch_bounds__(kBlock) void fedopt_chain_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                              const uint64_t* __restrict__ clients, int n_clients,
                                                              const float* __restrict__ r32,
                                                              const uint8_t* __restrict__ step_end, unsigned flags,
                                                              float b1, float omb1, float b2, float omb2, float eta,
                                                              float tau) {
    const LaneChunk<flame_segment, Tr<DT>::EPT> lc(segs, n_segs, blockIdx.x);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(typename Tr<DT>::T));
    bool full = (lc.chunk - sg.chunk_begin) * lc.CE + lc.CE <= sg.numel && !(sg.flags & FLAME_SEG_UNALIGNED);   // workgroup-uniform (on the copy: lane_isa_diff.log)
    // the packed fp16 body's FedYogi sign is torch's only while 1 - beta_2 >= 0 (sign_h2): a beta_2
    // above 1 takes the per-element body for every chunk (a kernel argument: uniform)
    if constexpr (DT == FLAME_F16 && kF16Native && VARIANT == FLAME_FEDYOGI) full &= !(omb2 < 0.f);
    if (full) {
        if constexpr (DT == FLAME_F16 && kF16Native)
            fedopt_chain_body_f16<VARIANT, CU>(sg, e0, cp, coff, n_clients, r32, step_end, flags, b1, omb1, b2, omb2,
                                               eta, tau);
        else
            fedopt_chain_body<DT, VARIANT, CU, true>(sg, e0, cp, coff, n_clients, r32, step_end, flags, b1, omb1, b2,
                                                     omb2, eta, tau);
    } else
        fedopt_chain_body<DT, VARIANT, 1, false>(sg, e0, cp, coff, n_clients, r32, step_end, flags, b1, omb1, b2,
                                                 omb2, eta, tau);
}

// ---------------------------------------------------------------- FedOPT, fp64 keys
// fedopt.py:102-129 (+ the _delta_v variants) for a key whose base, current, m, v and updates
// are all fp64.  Bodies of their own: the fp32-typed ones above round into a 16- or 32-bit dtype
// after every op and pick fp32 fast paths, none of which applies here.  Every torch op is one
// IEEE fp64 rounding (no fma: -ffp-contract=off), denormals kept; the scalars are the Python
// floats themselves (torch multiplies an fp64 tensor by a Python scalar in double, so none of
// them passes through fp32); the root and the quotient are flame_fm::dsqrt_rn / ddiv_rn.  Op for
// op what ew_kernel's FLAME_F64 arms compute for the same statements, so which of the two a key
// takes never shows in its bits.
struct Hyper64 { double b1, omb1, b2, omb2, eta, tau; };

__device__ __forceinline__ double sign_d(double x) {      // torch.sign: NaN -> 0, -0 -> 0
    return static_cast<double>((0.0 < x) - (x < 0.0));
}

template <int VARIANT>
__device__ __forceinline__ void adapt_elem_f64(double avg, double cur, double& m, double& v, double& cur_out,
                                               const Hyper64& h) {
    const double d = __dsub_rn(avg, cur);
    const double mn = __dadd_rn(__dmul_rn(m, h.b1), __dmul_rn(d, h.omb1));
    const double d2 = __dmul_rn(d, d);
    double vn;
    if constexpr (VARIANT == FLAME_FEDADAM) {
        vn = __dadd_rn(__dmul_rn(v, h.b2), __dmul_rn(d2, h.omb2));
    } else if constexpr (VARIANT == FLAME_FEDYOGI) {
        vn = __dsub_rn(v, __dmul_rn(__dmul_rn(d2, h.omb2), sign_d(__dsub_rn(v, d2))));
    } else {
        vn = __dadd_rn(v, d2);
    }
    m = mn;
    v = vn;
    const double den = __dadd_rn(flame_fm::dsqrt_rn(vn), h.tau);
    cur_out = __dadd_rn(cur, flame_fm::ddiv_rn(__dmul_rn(mn, h.eta), den));
}

// One chunk of an fp64 FedOPT round (fedopt_chunk's layout: a lane owns one 16-byte vector, two
// doubles): the clients reduced in order with the fp64 rates (reduce_clients, the arithmetic of
// agg_reduce_kernel<FLAME_F64>), then the step, then avg (if seg.out), m, v and cur_out stored.
template <int VARIANT, int CU>
__device__ __forceinline__ void fedopt_chunk_f64(const flame_segment* __restrict__ segs, int n_segs, int64_t chunk,
                                                 const uint64_t* __restrict__ clients, int n_clients,
                                                 const double* __restrict__ r64, unsigned flags, const Hyper64& h) {
    constexpr int DT = FLAME_F64;
    constexpr int EPT = Tr<DT>::EPT;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, chunk);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(double));
    const bool zero_state = (flags & FLAME_OPT_STATE_ZERO) != 0;
    const bool cur_avg = (sg.flags & FLAME_SEG_CUR_IS_AVG) != 0;   // cur IS the FedAvg result
    const bool vec = lc.vec();
    double acc[EPT];
    const double* base = reinterpret_cast<const double*>(sg.in) + e0;
    const double* curp = reinterpret_cast<const double*>(sg.cur) + e0;
    double* mp = reinterpret_cast<double*>(sg.m) + e0;
    double* vp = reinterpret_cast<double*>(sg.v) + e0;
    double* ap = sg.out ? reinterpret_cast<double*>(sg.out) + e0 : nullptr;
    double* cop = reinterpret_cast<double*>(sg.cur_out) + e0;
    if (vec) {
        unpack<double, EPT>(ld_v(base), acc);
        reduce_clients<DT, CU, true>(acc, false, cp, n_clients, nullptr, r64, e0, sg.numel, coff);
        double c[EPT], m[EPT], vv[EPT], co[EPT];
        if (!cur_avg) unpack<double, EPT>(ld_v(curp), c);
        if (!zero_state) {
            unpack<double, EPT>(ld_v(mp), m);
            unpack<double, EPT>(ld_v(vp), vv);
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if (cur_avg) c[j] = acc[j];
            if (zero_state) m[j] = vv[j] = 0.0;
            adapt_elem_f64<VARIANT>(acc[j], c[j], m[j], vv[j], co[j], h);
        }
        if (ap) st_v(ap, pack<double, EPT>(acc));
        st_v(mp, pack<double, EPT>(m));
        st_v(vp, pack<double, EPT>(vv));
        st_v(cop, pack<double, EPT>(co));
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = (e0 + j < sg.numel) ? ld1(base + j) : 0.0;
        reduce_clients<DT, 1, false>(acc, false, cp, n_clients, nullptr, r64, e0, sg.numel, coff);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if (e0 + j >= sg.numel) continue;
            double mj = zero_state ? 0.0 : ld1(mp + j), vj = zero_state ? 0.0 : ld1(vp + j), cj;
            adapt_elem_f64<VARIANT>(acc[j], cur_avg ? acc[j] : ld1(curp + j), mj, vj, cj, h);
            if (ap) st1(ap + j, acc[j]);
            st1(mp + j, mj);
            st1(vp + j, vj);
            st1(cop + j, cj);
        }
    }
}

template <int VARIANT, int CU>
__global__ __launch_bounds__(kBlock) void fedopt_kernel_f64(const flame_segment* __restrict__ segs, int n_segs,
                                                            const uint64_t* __restrict__ clients, int n_clients,
                                                            const double* __restrict__ r64, unsigned flags,
                                                            const Hyper64 h, int64_t n_chunks) {
    const int64_t chunk = wg_slot(flags & FLAME_OPT_XCD_MAP);
    if (chunk >= n_chunks) return;
    fedopt_chunk_f64<VARIANT, CU>(segs, n_segs, chunk, clients, n_clients, r64, flags, h);
}

// fedopt_chain_body for an fp64 model: per arrival base = base + round(w_i * r_i) with the fp64
// rate, the step of adapt_elem_f64 wherever a do() call closes.  What stays in registers between
// steps is what the per-call launches would store and reload (every op rounds to fp64).
template <int VARIANT, int CU, bool VEC>
__device__ __forceinline__ void fedopt_chain_body_f64(const flame_segment& sg, int64_t e0,
                                                      const uint64_t* __restrict__ cp, int64_t coff, int n_clients,
                                                      const double* __restrict__ r64,
                                                      const uint8_t* __restrict__ step_end, unsigned flags,
                                                      const Hyper64& h) {
    using X = Tr<FLAME_F64>;
    constexpr int EPT = X::EPT;
    const int nv = VEC ? EPT : static_cast<int>(sg.numel - e0 < EPT ? sg.numel - e0 : EPT);   // (not lane_load: lane_isa_diff.log)
    bool aliased = (sg.flags & FLAME_SEG_CUR_IS_AVG) != 0;
    const bool zero_state = (flags & FLAME_OPT_STATE_ZERO) != 0;
    const double* bp = reinterpret_cast<const double*>(sg.in) + e0;
    const double* curp = reinterpret_cast<const double*>(sg.cur) + e0;
    double* mp = reinterpret_cast<double*>(sg.m) + e0;
    double* vp = reinterpret_cast<double*>(sg.v) + e0;
    auto load = [&](const double* p, double (&x)[EPT], bool nt) {
        if constexpr (VEC) {
            unpack<double, EPT>(nt ? ld_nt(p) : ld_v(p), x);
        } else {
#pragma unroll
            for (int j = 0; j < EPT; ++j) x[j] = j < nv ? ld1(p + j) : 0.0;
        }
    };
    auto store = [&](double* p, const double (&x)[EPT]) {
        if constexpr (VEC) {
            st_v(p, pack<double, EPT>(x));
        } else {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (j < nv) st1(p + j, x[j]);
        }
    };
    double b[EPT], c[EPT] = {}, m[EPT] = {}, v[EPT] = {};
    load(bp, b, false);
    if (!aliased) load(curp, c, false);
    if (!zero_state) {
        load(mp, m, false);
        load(vp, v, false);
    }
    auto load_client = [&](int i, double (&x)[EPT]) {
        load(reinterpret_cast<const double*>(reinterpret_cast<const char*>(cp[i]) + coff), x, true);
    };
    auto arrive = [&](const double (&x)[EPT], double r, bool ends) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) b[j] = X::add(b[j], X::tmp(x[j], 0.f, r));
        if (ends) {     // uniform: one do() call ends here
            if (__builtin_expect(aliased, 0)) {   // the first step after the passthrough: current IS base
#pragma unroll
                for (int j = 0; j < EPT; ++j) c[j] = b[j];
                aliased = false;
            }
#pragma unroll
            for (int j = 0; j < EPT; ++j) adapt_elem_f64<VARIANT>(b[j], c[j], m[j], v[j], c[j], h);
        }
    };
    int i = 0;
    for (; i + CU <= n_clients; i += CU) {
        double x[CU][EPT], rr[CU];
        bool ends[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) load_client(i + u, x[u]);
#pragma unroll
        for (int u = 0; u < CU; ++u) {     // the batch's scalar loads issued together, one wait
            rr[u] = r64[i + u];
            ends[u] = step_ends(step_end, i + u);
        }
#pragma unroll
        for (int u = 0; u < CU; ++u) arrive(x[u], rr[u], ends[u]);
    }
    for (; i < n_clients; ++i) {
        double x[EPT];
        load_client(i, x);
        arrive(x, r64[i], step_ends(step_end, i));
    }
    if (aliased) {             // no step closed: current is still the base
#pragma unroll
        for (int j = 0; j < EPT; ++j) c[j] = b[j];
    }
    store(reinterpret_cast<double*>(sg.out) + e0, b);
    store(mp, m);
    store(vp, v);
    store(reinterpret_cast<double*>(sg.cur_out) + e0, c);
}

template <int VARIANT, int CU>
__global__ __launch_bounds__(kBlock) void fedopt_chain_kernel_f64(const flame_segment* __restrict__ segs, int n_segs,
                                                                  const uint64_t* __restrict__ clients,
                                                                  int n_clients, const double* __restrict__ r64,
                                                                  const uint8_t* __restrict__ step_end,
                                                                  unsigned flags, const Hyper64 h) {
    const LaneChunk<flame_segment, Tr<FLAME_F64>::EPT> lc(segs, n_segs, blockIdx.x);
    if (!lc.live()) return;
    const uint64_t* cp = lc.row(clients, n_clients);
    const int64_t coff = lc.offset(lc.sg.client_tile_stride, sizeof(double));
    if ((lc.chunk - lc.sg.chunk_begin) * lc.CE + lc.CE <= lc.sg.numel && !(lc.sg.flags & FLAME_SEG_UNALIGNED))   // as fedopt_chain_kernel
        fedopt_chain_body_f64<VARIANT, CU, true>(lc.sg, lc.e0, cp, coff, n_clients, r64, step_end, flags, h);
    else
        fedopt_chain_body_f64<VARIANT, 1, false>(lc.sg, lc.e0, cp, coff, n_clients, r64, step_end, flags, h);
}

// ---------------------------------------------------------------- FedBuff scale-add (+delta)
template <int DT> struct SA;
template <> struct SA<FLAME_F32> {
    using T = float; static constexpr int EPT = 4;
    __device__ static void op(T& b, T a, float g, double, T* d) {
        const float nb = __fadd_rn(b, __fdiv_rn(a, g));
        if (d) *d = __fsub_rn(nb, b);
        b = nb;
    }
};
template <> struct SA<FLAME_F64> {
    using T = double; static constexpr int EPT = 2;
    __device__ static void op(T& b, T a, float, double g, T* d) {
        const double nb = __dadd_rn(b, __ddiv_rn(a, g));
        if (d) *d = __dsub_rn(nb, b);
        b = nb;
    }
};
template <> struct SA<FLAME_BF16> {
    using T = uint16_t; static constexpr int EPT = 8;
    __device__ static void op(T& b, T a, float g, double, T* d) {
        const float bo = bf16_to_f32(b);
        const float q = bf16_round(__fdiv_rn(bf16_to_f32(a), g));
        const float nb = bf16_round(__fadd_rn(bo, q));
        if (d) *d = f32_to_bf16_exact(bf16_round(__fsub_rn(nb, bo)));
        b = f32_to_bf16_exact(nb);
    }
};
template <> struct SA<FLAME_F16> {
    using T = uint16_t; static constexpr int EPT = 8;
    __device__ static void op(T& b, T a, float g, double, T* d) {
        const float bo = f16_to_f32(b);
        const float q = f16_round(__fdiv_rn(f16_to_f32(a), g));
        const float nb = f16_round(__fadd_rn(bo, q));
        if (d) *d = f32_to_f16_bits(__fsub_rn(nb, bo));
        b = f32_to_f16_bits(nb);
    }
};

template <int DT>
__global__ __launch_bounds__(kEwBlock) void scale_add_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                           float gf, double gd) {
    using S = SA<DT>;
    using T = typename S::T;
    constexpr int EPT = S::EPT;
    static_assert(kEwBlock == kBlock, "LaneChunk's chunk is kBlock lanes");
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, blockIdx.x);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    T* bp = reinterpret_cast<T*>(sg.out) + e0;
    const T* ap = reinterpret_cast<const T*>(sg.in) + e0;
    T* dp = sg.cur_out ? reinterpret_cast<T*>(sg.cur_out) + e0 : nullptr;
    if (lc.vec()) {
        T b[EPT], a[EPT], d[EPT];
        unpack<T, EPT>(ld_v(bp), b);
        unpack<T, EPT>(ld_v(ap), a);
#pragma unroll
        for (int j = 0; j < EPT; ++j) S::op(b[j], a[j], gf, gd, dp ? &d[j] : nullptr);
        st_v(bp, pack<T, EPT>(b));
        if (dp) st_v(dp, pack<T, EPT>(d));
    } else {
        for (int j = 0; j < EPT; ++j) {
            if (e0 + j >= sg.numel) break;
            T b = ld1(bp + j), d;
            S::op(b, ld1(ap + j), gf, gd, dp ? &d : nullptr);
            st1(bp + j, b);
            if (dp) st1(dp + j, d);
        }
    }
}

// ---------------------------------------------------------------- co-located FedBuff hierarchy
// One pass over a node's whole two-level asynchronous hierarchy:
// for each middle m in the order the top receives their deltas --
//   agg_m  = FedBuff None-start reduce of its C queued arrivals      (fedbuff.py:89-97,136-157)
//   w_m'   = w_m + agg_m / goal_m,  delta_m = w_m' - w_m             (fedbuff.py:122-127,
//                                     asyncfl/middle_aggregator.py:221-226,246, common/util.py:152-159)
//   top    = tmp(delta_m, rate_m) [None start] or top + tmp(...)     (fedbuff.py:96,136-157, top role)
// then top_w += top / top_goal (fedbuff.py:122-127).  Every op rounds in the tensor's
// dtype exactly as the separate launches do, so results are bit-identical to them; the
// middle aggregates and deltas never touch HBM (deltas are stored only if asked for).
// SYNC (FLAME_HIER_SYNC): the synchronous hierarchy instead (syncfl/middle_aggregator.py:163-229,
// syncfl/top_aggregator.py:122-176): each middle's FedAvg starts from its weights,
//   a = w_m + tmp(c_{m,0}, r_{m,0}) + ...;  w_m' = a;  d_m = w_m' - w_m
// and the top's FedAvg adds tmp(d_m, top_rates[m]) to the top weights (top_agg_in).
template <int DT> __device__ __forceinline__ float rnd(float x);
// The element-wise hierarchy (segment tails, misaligned views): the same op sequence as the
// vector paths, one element at a time.
template <int DT, bool SYNC, typename MP>
__device__ __forceinline__ void hier_tail(const flame_hier_segment& sg, int64_t e0, int64_t coff,
                                          const uint64_t* __restrict__ wrow, const uint64_t* __restrict__ drow,
                                          const uint64_t* __restrict__ crow, MP mid_ptr, int n_mids, int n_clients,
                                          const float* __restrict__ mid_rates, const float* __restrict__ mid_goal,
                                          const float* __restrict__ top_rates, float top_goal, unsigned flags) {
    using X = Tr<DT>;
    using S = SA<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    (void)wrow;
    A top[EPT];
    bool have_top = (flags & FLAME_HIER_TOP_ACCUM) != 0;
    const T* tin = reinterpret_cast<const T*>(sg.top_agg_in) + e0;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (have_top && e0 + j < sg.numel) top[j] = X::ld(ld1(tin + j));
#pragma unroll 1
    for (int m = 0; m < n_mids; ++m) {
        A acc[EPT];
        T* wp = mid_ptr(m);
        if constexpr (SYNC) {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                acc[j] = (e0 + j < sg.numel) ? X::ld(ld1(wp + j)) : A(0);
        }
        reduce_clients<DT, 1, false>(acc, !SYNC, crow + static_cast<int64_t>(m) * n_clients, n_clients,
                                     mid_rates + static_cast<int64_t>(m) * n_clients, nullptr, e0, sg.numel, coff);
        T* dp = (drow && drow[m]) ? reinterpret_cast<T*>(drow[m]) + e0 : nullptr;
        const float g = mid_goal[m], rt = top_rates[m];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if (e0 + j >= sg.numel) continue;
            T w = ld1(wp + j), d;
            if constexpr (SYNC) {
                const T wn = X::st(acc[j]);
                d = X::st(rnd<DT>(__fsub_rn(X::ld(wn), X::ld(w))));
                w = wn;
            } else {
                S::op(w, X::st(acc[j]), g, static_cast<double>(g), &d);
            }
            if (!(flags & FLAME_HIER_MID_READONLY)) st1(wp + j, w);
            if (dp) st1(dp + j, d);
            const A t = X::tmp(d, rt, 0.0);
            top[j] = have_top ? X::add(top[j], t) : t;
        }
        have_top = true;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        if (e0 + j >= sg.numel) continue;
        const T t = X::st(top[j]);
        if (sg.top_agg_out) st1(reinterpret_cast<T*>(sg.top_agg_out) + e0 + j, t);
        if (flags & FLAME_HIER_TOP_APPLY) {
            T* gp = reinterpret_cast<T*>(sg.top_w) + e0 + j;
            T gw = ld1(gp);
            S::op(gw, t, top_goal, static_cast<double>(top_goal), nullptr);
            st1(gp, gw);
        }
    }
}

// (HL instantiations: the middle loop stays rolled -- its group lives in LDS, not registers)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <int DT, int CU, bool SYNC, int HB, bool HL>
__device__ __forceinline__ void hier_fedbuff_body(const flame_hier_segment* __restrict__ segs, int n_segs,
                                                  int n_mids, int n_clients, const uint64_t* __restrict__ mid_w,
                                                  const uint64_t* __restrict__ mid_delta,
                                                  const uint64_t* __restrict__ clients,
                                                  const float* __restrict__ mid_rates,
                                                  const float* __restrict__ mid_goal,
                                                  const float* __restrict__ top_rates, float top_goal,
                                                  unsigned flags) {
    using X = Tr<DT>;
    using S = SA<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    const LaneChunk<flame_hier_segment, EPT> lc(segs, n_segs, blockIdx.x);
    if (!lc.live()) return;
    const flame_hier_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const int64_t coff = lc.offset(sg.client_tile_stride, sizeof(T));
    const uint64_t* wrow = lc.row(mid_w, n_mids);
    const uint64_t* drow = mid_delta ? lc.row(mid_delta, n_mids) : nullptr;
    const uint64_t* crow = clients + static_cast<int64_t>(lc.s) * n_mids * n_clients;
    const bool vec = lc.vec();
    // inside every middle's weights, contiguous or tiled (not lc.offset: profiles/lane_isa_diff.log)
    const int64_t woff = sg.mid_tile_stride
        ? (lc.chunk - sg.chunk_begin) * sg.mid_tile_stride + static_cast<int64_t>(threadIdx.x) * EPT * sizeof(T)
        : e0 * static_cast<int64_t>(sizeof(T));
    auto mid_ptr = [&](int m) { return reinterpret_cast<T*>(reinterpret_cast<char*>(wrow[m]) + woff); };
    A top[EPT];
    bool have_top = (flags & FLAME_HIER_TOP_ACCUM) != 0;
    const T* tin = reinterpret_cast<const T*>(sg.top_agg_in) + e0;
    if (vec) {
        if (have_top) {
            T b[EPT];
            unpack<T, EPT>(ld_v(tin), b);
#pragma unroll
            for (int j = 0; j < EPT; ++j) top[j] = X::ld(b[j]);
        }
        // middles in groups of HB: a group's middle-weight stores are issued together after its
        // reductions (1 = store each middle's weights right after its reduction).  HL: the group's
        // weights wait in LDS (lane-private slots, no barrier) rather than in registers -- long
        // store bursts at 2 workgroups per CU
        __shared__ V16 held[HL ? HB * kBlock : 1];
#pragma unroll 1
        for (int m0 = 0; m0 < n_mids; m0 += HB) {
            V16 pend[HL ? 1 : HB];
            const int nb = n_mids - m0 < HB ? n_mids - m0 : HB;   // middles in this group
#pragma unroll
            for (int u = 0; u < HB; ++u) {
            const int m = m0 + u;
            if (HB > 1 && m >= n_mids) break;
            T* wp = mid_ptr(m);
            A acc[EPT];
            T wo[EPT];
            if constexpr (SYNC) {     // FedAvg starts from the middle's weights (deepcopy(self.weights))
                unpack<T, EPT>(ld_v(wp), wo);
#pragma unroll
                for (int j = 0; j < EPT; ++j) acc[j] = X::ld(wo[j]);
            }
            reduce_clients<DT, CU, true>(acc, !SYNC, crow + static_cast<int64_t>(m) * n_clients, n_clients,
                                         mid_rates + static_cast<int64_t>(m) * n_clients, nullptr, e0, sg.numel,
                                         coff);
            T* dp = (drow && drow[m]) ? reinterpret_cast<T*>(drow[m]) + e0 : nullptr;
            const float g = mid_goal[m], rt = top_rates[m];
            // A one-trip loop on purpose (as in fedopt_chunk): without it the group loop compiles to
            // another schedule, measured 0.4 % slower on config 5 (profiles/vpt_isa_diff.log)
#pragma unroll
            for (int once = 0; once < 1; ++once) {
                T w[EPT], d[EPT];
                if constexpr (SYNC) {
#pragma unroll
                    for (int j = 0; j < EPT; ++j) {
                        w[j] = X::st(acc[j]);
                        d[j] = X::st(rnd<DT>(__fsub_rn(X::ld(w[j]), X::ld(wo[j]))));
                        top[j] = X::add(top[j], X::tmp(d[j], rt, 0.0));
                    }
                } else {
                    unpack<T, EPT>(ld_v(wp), w);
#pragma unroll
                    for (int j = 0; j < EPT; ++j) {
                        S::op(w[j], X::st(acc[j]), g, static_cast<double>(g), &d[j]);
                        const A t = X::tmp(d[j], rt, 0.0);
                        top[j] = have_top ? X::add(top[j], t) : t;
                    }
                }
                if constexpr (HL) held[u * kBlock + threadIdx.x] = pack<T, EPT>(w);
                else pend[u] = pack<T, EPT>(w);
                if (dp) st_v(dp, pack<T, EPT>(d));
            }
            have_top = true;
            }
            if (!(flags & FLAME_HIER_MID_READONLY)) {
#pragma unroll
                for (int u = 0; u < HB; ++u) {
                    if (u >= nb) break;
                    T* wp = mid_ptr(m0 + u);       // re-read from the (scalar) pointer table
                    V16 pv;
                    if constexpr (HL) pv = held[u * kBlock + threadIdx.x];
                    else pv = pend[u];
                    st_v(wp, pv);
                }
            }
        }
        T o[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) o[j] = X::st(top[j]);
        if (sg.top_agg_out) st_v(reinterpret_cast<T*>(sg.top_agg_out) + e0, pack<T, EPT>(o));
        if (flags & FLAME_HIER_TOP_APPLY) {
            T* gp = reinterpret_cast<T*>(sg.top_w) + e0;
            T gw[EPT];
            unpack<T, EPT>(ld_v(gp), gw);
#pragma unroll
            for (int j = 0; j < EPT; ++j) S::op(gw[j], o[j], top_goal, static_cast<double>(top_goal), nullptr);
            st_v(gp, pack<T, EPT>(gw));
        }
        return;
    }
    hier_tail<DT, SYNC>(sg, e0, coff, wrow, drow, crow, mid_ptr, n_mids, n_clients, mid_rates, mid_goal, top_rates,
                        top_goal, flags);
}

template <int DT, int CU, bool SYNC, int HB, bool HL>
__global__ __launch_bounds__(kBlock) void hier_fedbuff_kernel(const flame_hier_segment* __restrict__ segs, int n_segs,
                                                    int n_mids, int n_clients, const uint64_t* __restrict__ mid_w,
                                                    const uint64_t* __restrict__ mid_delta,
                                                    const uint64_t* __restrict__ clients,
                                                    const float* __restrict__ mid_rates,
                                                    const float* __restrict__ mid_goal,
                                                    const float* __restrict__ top_rates, float top_goal,
                                                    unsigned flags) {
    hier_fedbuff_body<DT, CU, SYNC, HB, HL>(segs, n_segs, n_mids, n_clients, mid_w, mid_delta, clients, mid_rates, mid_goal,
                                    top_rates, top_goal, flags);
}

// The same with the metadata block in the kernel arguments (small launches, e.g. a single
// FedBuff aggregator's fused scale_add); word offsets into the block, -1 = no delta table.
template <int DT, int CU, bool SYNC, int HB, bool HL>
__global__ __launch_bounds__(kBlock) void hier_fedbuff_kernel_argmeta(const ArgMeta meta, int n_segs, int n_mids, int n_clients,
                                                            int o_mid_w, int o_mid_delta, int o_clients,
                                                            int o_mid_rates, int o_mid_goal, int o_top_rates,
                                                            float top_goal, unsigned flags) {
    (void)sizeof(meta);     // read in place in the kernarg segment (see agg_reduce_kernel_argmeta)
    const uint64_t* w = (const uint64_t*)__builtin_amdgcn_kernarg_segment_ptr();
    hier_fedbuff_body<DT, CU, SYNC, HB, HL>(reinterpret_cast<const flame_hier_segment*>(w), n_segs, n_mids, n_clients,
                                    w + o_mid_w, o_mid_delta >= 0 ? w + o_mid_delta : nullptr, w + o_clients,
                                    reinterpret_cast<const float*>(w + o_mid_rates),
                                    reinterpret_cast<const float*>(w + o_mid_goal),
                                    reinterpret_cast<const float*>(w + o_top_rates), top_goal, flags);
}
#pragma clang diagnostic pop

// ---------------------------------------------------------------- FedDyn server round
// One pass over a FedDyn aggregation round (optimizer/feddyn.py:90-113,125-139), driven
// by a host-built step program.  Per element, in step order (every op rounded in dtype):
//   W:    load the arrival w (tiled or contiguous, like flame_agg_reduce's clients)
//   HIN:  load a history h (contiguous)
//   AVG:  avg = avg + tmp(w, r_avg)                           (FedAvg, rate 1/len(cache))
//   HOUT: h' = HIN ? h + w : w, stored to h_out               (add_to_hist)
//   MEAN: mean = mean + tmp(HOUT ? h' : h, r_mean), mean0 = +0 (0.0 + Σ rate*h)
// then out = avg, cld = avg + mean.  Steps [0, n_phase1) run before [n_phase1, n_steps);
// batched loads never cross that boundary, so a phase-2 step may re-read what a phase-1
// step stored (history order != arrival order).
template <int DT, int CU, bool VEC>
__device__ __forceinline__ void feddyn_chunk(const flame_dyn_segment& sg, const uint64_t* __restrict__ row,
                                             const uint32_t* __restrict__ sflags, int n_steps, int n_phase1,
                                             float ra32, float rm32, double ra64, double rm64, int64_t e0,
                                             int64_t coff, int64_t hoff) {
    using X = Tr<DT>;
    using T = typename X::T;
    using A = typename X::A;
    constexpr int EPT = X::EPT;
    const int64_t ooff = e0 * static_cast<int64_t>(sizeof(T));   // base / average / cld: contiguous
    auto load = [&](uint64_t base, int64_t off, T (&x)[EPT]) {
        lane_load<VEC, true>(reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + off), x, e0, sg.numel);
    };
    auto store = [&](void* base, int64_t off, const T (&x)[EPT]) {
        lane_store<VEC>(reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off), x, e0, sg.numel);
    };
    A avg[EPT], mean[EPT];
    {
        T b[EPT];
        load(reinterpret_cast<uint64_t>(sg.in), ooff, b);
#pragma unroll
        for (int j = 0; j < EPT; ++j) { avg[j] = X::ld(b[j]); mean[j] = A(0); }
    }
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
        const int end = phase ? n_steps : n_phase1;
#pragma unroll 1
        for (int k = phase ? n_phase1 : 0; k < end; k += CU) {
            const int nb = (end - k < CU) ? end - k : CU;
            T w[CU][EPT], h[CU][EPT];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                if (u >= nb) break;
                const uint32_t f = sflags[k + u];
                const uint64_t* p = row + static_cast<int64_t>(k + u) * 3;
                if (f & FLAME_DYN_W) load(p[0], coff, w[u]);
                if (f & FLAME_DYN_HIN) load(p[1], hoff, h[u]);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                if (u >= nb) break;
                const uint32_t f = sflags[k + u];
                if (f & FLAME_DYN_AVG) {
#pragma unroll
                    for (int j = 0; j < EPT; ++j) avg[j] = X::add(avg[j], X::tmp(w[u][j], ra32, ra64));
                }
                if (f & FLAME_DYN_HOUT) {
                    if (f & FLAME_DYN_HIN) {
#pragma unroll
                        for (int j = 0; j < EPT; ++j) h[u][j] = X::st(X::add(X::ld(h[u][j]), X::ld(w[u][j])));
                    } else {
#pragma unroll
                        for (int j = 0; j < EPT; ++j) h[u][j] = w[u][j];
                    }
                    store(reinterpret_cast<void*>(row[static_cast<int64_t>(k + u) * 3 + 2]), hoff, h[u]);
                }
                if (f & FLAME_DYN_MEAN) {
#pragma unroll
                    for (int j = 0; j < EPT; ++j) mean[j] = X::add(mean[j], X::tmp(h[u][j], rm32, rm64));
                }
            }
        }
    }
    T o[EPT], c[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) { o[j] = X::st(avg[j]); c[j] = X::st(X::add(avg[j], mean[j])); }
    store(sg.out, ooff, o);
    store(sg.cld, ooff, c);
}

template <int DT, int CU>
__global__ __launch_bounds__(kBlock) void feddyn_kernel(const flame_dyn_segment* __restrict__ segs, int n_segs,
                                                        const uint64_t* __restrict__ steps,
                                                        const uint32_t* __restrict__ sflags, int n_steps,
                                                        int n_phase1, float ra32, float rm32, double ra64,
                                                        double rm64) {
    using X = Tr<DT>;
    constexpr int EPT = X::EPT;
    // XCD-contiguous chunk map: 512 x 12M fp32 -0.7 % (cache order) / -1.4 % (other order)
    // (profiles/r02_feddyn_xcd_sweep.log)
    const LaneChunk<flame_dyn_segment, EPT> lc(segs, n_segs, xcd_slot(blockIdx.x, gridDim.x));
    if (!lc.live()) return;
    const int64_t coff = lc.offset(lc.sg.client_tile_stride, sizeof(typename X::T));
    // histories: contiguous, or tiled like the arrivals (a FedDyn history store in the slab layout); not
    // lc.offset: profiles/lane_isa_diff.log
    const int64_t hoff = lc.sg.hist_tile_stride
        ? (lc.chunk - lc.sg.chunk_begin) * lc.sg.hist_tile_stride + static_cast<int64_t>(threadIdx.x) * EPT * static_cast<int64_t>(sizeof(typename X::T))
        : lc.e0 * static_cast<int64_t>(sizeof(typename X::T));
    const uint64_t* row = steps + static_cast<int64_t>(lc.s) * n_steps * 3;
    if (lc.vec())
        feddyn_chunk<DT, CU, true>(lc.sg, row, sflags, n_steps, n_phase1, ra32, rm32, ra64, rm64, lc.e0, coff, hoff);
    else
        feddyn_chunk<DT, 1, false>(lc.sg, row, sflags, n_steps, n_phase1, ra32, rm32, ra64, rm64, lc.e0, coff, hoff);
}

// ---------------------------------------------------------------- synthetic generator
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <int DT>
__global__ __launch_bounds__(kEwBlock) void synth_kernel(void* out, int64_t numel, uint64_t ck, int64_t start, float scale) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kEwBlock;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * kEwBlock + threadIdx.x; j < numel; j += stride) {
        const uint64_t h = mix64(ck + static_cast<uint64_t>(start + j) * 0x9E3779B97F4A7C15ull);
        const int32_t s = static_cast<int32_t>((h & 0xFFFFu) + ((h >> 16) & 0xFFFFu) + ((h >> 32) & 0xFFFFu) + (h >> 48)) - 131070;
        const float x = __fmul_rn(static_cast<float>(s), scale);
        if constexpr (DT == FLAME_F32) st1(reinterpret_cast<float*>(out) + j, x);
        else if constexpr (DT == FLAME_BF16) st1(reinterpret_cast<uint16_t*>(out) + j, f32_to_bf16_exact(bf16_round(x)));
        else st1(reinterpret_cast<uint16_t*>(out) + j, f32_to_f16_bits(x));
    }
}

// ---------------------------------------------------------------- server-side Gaussian noise
// flame's DifferentialPrivacy adds torch.normal(0, noise_factor) to every element of a trainer's
// delta (privacy/differential_privacy.py:55-61); here the aggregator draws the noise of the whole
// round once ("the noise contract").  The generator is a pure function of
// (seed, round, stream, index): Philox4x32-10 (Salmon et al., SC'11) gives four words per block b,
// counter (b lo, b hi, stream, round), key (seed lo, seed hi); (x0, x1) and (x2, x3) each give two
// unit normals by Box-Muller.  Every floating-point step is ONE fp32 operation written as an
// intrinsic -- no fma, no hardware log / sin / cos, no device libm -- in the order
// tests/noise_ref.py restates them in numpy float32, so the two agree bit for bit.  (The root is
// __builtin_sqrtf, which is correctly rounded; the __fsqrt_rn builtin lowers to the 1-ulp v_sqrt_f32.)
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = static_cast<uint32_t>(p1); c[2] = n2; c[3] = static_cast<uint32_t>(p0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// -2 ln u for u in (0, 1]: u = 2^e m with m in (sqrt(1/2), sqrt 2], ln m = 2 atanh(s), s = f / (2 + f),
// f = m - 1 (exact), the series to s^11; e ln 2 with ln 2 split so that e * HI is exact
__device__ __forceinline__ float noise_neg2ln(float u) {
    const uint32_t bits = __float_as_uint(u);
    int e = static_cast<int>(bits >> 23) - 127;
    float m = __uint_as_float((bits & 0x7FFFFFu) | 0x3F800000u);
    if (m > 0x1.6a09e6p+0f) { m = __fmul_rn(m, 0.5f); e += 1; }
    const float f = __fadd_rn(m, -1.0f);
    const float s = __fdiv_rn(f, __fadd_rn(f, 2.0f));
    const float z = __fmul_rn(s, s);
    float p = 0x1.745d18p-4f;
    p = __fadd_rn(__fmul_rn(p, z), 0x1.c71c72p-4f);
    p = __fadd_rn(__fmul_rn(p, z), 0x1.24924ap-3f);
    p = __fadd_rn(__fmul_rn(p, z), 0x1.99999ap-3f);
    p = __fadd_rn(__fmul_rn(p, z), 0x1.555556p-2f);
    p = __fmul_rn(p, z);
    const float t = __fadd_rn(s, s);
    const float lg = __fadd_rn(t, __fmul_rn(t, p));
    const float ef = static_cast<float>(e);
    const float ln = __fadd_rn(__fmul_rn(ef, 0x1.62e4p-1f), __fadd_rn(lg, __fmul_rn(ef, 0x1.7f7d1cp-20f)));
    return __fmul_rn(-2.0f, ln);
}

// (cos, sin) of 2 pi k / 2^24: the octant from the integer, the angle inside it mirrored onto
// [0, pi/4], the Taylor polynomials to phi^9 / phi^10 there
__device__ __forceinline__ void noise_sincos(uint32_t k, float& co, float& si) {
    const uint32_t o = k >> 21, j = k & 0x1FFFFFu;
    const uint32_t jj = (o & 1u) ? 0x200000u - j : j;
    const float phi = __fmul_rn(static_cast<float>(jj), 0x1.921fb6p-22f);
    const float z = __fmul_rn(phi, phi);
    float ps = 0x1.71de3ap-19f;
    ps = __fadd_rn(__fmul_rn(ps, z), -0x1.a01a02p-13f);
    ps = __fadd_rn(__fmul_rn(ps, z), 0x1.111112p-7f);
    ps = __fadd_rn(__fmul_rn(ps, z), -0x1.555556p-3f);
    const float s = __fadd_rn(phi, __fmul_rn(__fmul_rn(phi, z), ps));
    float pc = -0x1.27e4fcp-22f;
    pc = __fadd_rn(__fmul_rn(pc, z), 0x1.a01a02p-16f);
    pc = __fadd_rn(__fmul_rn(pc, z), -0x1.6c16c2p-10f);
    pc = __fadd_rn(__fmul_rn(pc, z), 0x1.555556p-5f);
    pc = __fadd_rn(__fmul_rn(pc, z), -0x1p-1f);
    const float c = __fadd_rn(1.0f, __fmul_rn(z, pc));
    const bool swap = ((o + 1u) >> 1) & 1u, cneg = ((o + 2u) >> 2) & 1u, sneg = o >> 2;
    const float c0 = swap ? s : c, s0 = swap ? c : s;
    co = __uint_as_float(__float_as_uint(c0) ^ (cneg ? 0x80000000u : 0u));
    si = __uint_as_float(__float_as_uint(s0) ^ (sneg ? 0x80000000u : 0u));
}

// two unit normals from two words: u1 = RNE_f32(2 xu + 1) * 2^-33 in (0, 1] (the 33-bit odd integer as
// an exact 16-bit high part and an exact 17-bit low part: the one rounding is the add's), k = xk >> 8
__device__ __forceinline__ void noise_pair(uint32_t xu, uint32_t xk, float& ze, float& zo) {
    const uint64_t v = 2ull * xu + 1ull;
    const float hi = static_cast<float>(static_cast<uint32_t>(v >> 17));
    const float lo = static_cast<float>(static_cast<uint32_t>(v & 0x1FFFFu));
    const float u = __fmul_rn(__fadd_rn(__fmul_rn(hi, 131072.0f), lo), 0x1p-33f);
    const float r = __builtin_sqrtf(noise_neg2ln(u));
    float co, si;
    noise_sincos(xk >> 8, co, si);
    ze = __fmul_rn(r, co);
    zo = __fmul_rn(r, si);
}

// the four unit normals of block b of key `stream` in round `round`
__device__ __forceinline__ void noise_block(uint32_t k0, uint32_t k1, uint32_t round, uint32_t stream, uint64_t b,
                                            float (&z)[4]) {
    uint32_t c[4] = {static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32), stream, round};
    philox4x32_10(c, k0, k1);
    noise_pair(c[0], c[1], z[0], z[1]);
    noise_pair(c[2], c[3], z[2], z[3]);
}

// noise[e] = round_dtype(z * std): f32 / bf16 / f16 one fp32 product by the fp32 std (16-bit: then one
// RNE rounding); f64 widens z and takes one fp64 product by the double
template <int DT>
__device__ __forceinline__ typename Tr<DT>::T noise_value(float z, float std32, double std64) {
    if constexpr (DT == FLAME_F64) return __dmul_rn(static_cast<double>(z), std64);
    else if constexpr (DT == FLAME_F32) return __fmul_rn(z, std32);
    else if constexpr (DT == FLAME_BF16) return f32_to_bf16_exact(bf16_round(__fmul_rn(z, std32)));
    else return f32_to_f16_bits(__fmul_rn(z, std32));
}

// Write-only fill over a segment table (only out, numel, chunk_begin and flags are read); element e
// of segment s is the generator's value at global index starts[s] + e of key streams[s].  A lane
// covers EPT consecutive elements; an aligned segment with starts % 4 == 0 stores them as one
// 16-byte vector (whole Philox blocks), anything else element by element.  The value of an element
// depends on (seed, round, stream, index) alone, never on the launch geometry.
template <int DT>
__global__ __launch_bounds__(kBlock) void noise_fill_kernel(const flame_segment* __restrict__ segs, int n_segs,
                                                          const uint32_t* __restrict__ streams,
                                                          const int64_t* __restrict__ starts, uint32_t k0, uint32_t k1,
                                                          uint32_t round, float std32, double std64) {
    using T = typename Tr<DT>::T;
    constexpr int EPT = Tr<DT>::EPT;
    const LaneChunk<flame_segment, EPT> lc(segs, n_segs, blockIdx.x);
    if (!lc.live()) return;
    const flame_segment sg = lc.sg;
    const int64_t e0 = lc.e0;
    const uint32_t stream = streams[lc.s];
    const uint64_t start = static_cast<uint64_t>(starts[lc.s]);
    const uint64_t g0 = start + static_cast<uint64_t>(e0);
    T* op = reinterpret_cast<T*>(sg.out) + e0;
    float z[4];
    if (lc.vec() && !(start & 3u)) {
        T x[EPT];
        if constexpr (EPT >= 4) {
#pragma unroll
            for (int q = 0; q < EPT / 4; ++q) {
                noise_block(k0, k1, round, stream, (g0 >> 2) + q, z);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * q + j] = noise_value<DT>(z[j], std32, std64);
            }
        } else {            // f64: half a block per lane
            noise_block(k0, k1, round, stream, g0 >> 2, z);
            const bool up = g0 & 2u;
            x[0] = noise_value<DT>(up ? z[2] : z[0], std32, std64);
            x[1] = noise_value<DT>(up ? z[3] : z[1], std32, std64);
        }
        st_v(op, pack<T, EPT>(x));
        return;
    }
    uint64_t have = ~0ull;
    for (int j = 0; j < EPT; ++j) {
        if (e0 + j >= sg.numel) break;
        const uint64_t g = g0 + static_cast<uint64_t>(j);
        if ((g >> 2) != have) {
            have = g >> 2;
            noise_block(k0, k1, round, stream, have, z);
        }
        const uint32_t l = static_cast<uint32_t>(g) & 3u;
        const float zl = l == 0 ? z[0] : l == 1 ? z[1] : l == 2 ? z[2] : z[3];
        st1(op + j, noise_value<DT>(zl, std32, std64));
    }
}

// ---------------------------------------------------------------- slab insert (tiling copy)
// The role's `self.cache[end] = tres` (syncfl/top_aggregator.py:154-156) lands one update
// in a slab slot: each key's contiguous bytes are cut into 4 KiB tiles (one reduction
// chunk of any dtype) written `dst_tile_stride` apart (the slab's capacity x 4 KiB).  One
// workgroup copies kSlabTPW tiles, every lane 16 B of each (all its loads issued before its
// stores); the entry table rides in the kernel arguments, so an insert is ONE launch and no
// H2D of metadata.
// 2 tiles per workgroup (1-8 within noise) and plain stores (measured best of the store policies,
// profiles/r03b_slab_sweep.log)
constexpr int kSlabTPW = 2;
struct SlabEntry { const uint8_t* src; uint8_t* dst; int64_t nbytes; int64_t stride; int64_t tile_begin; };
constexpr int kSlabMaxEntries = static_cast<int>(sizeof(ArgMeta) / sizeof(SlabEntry));
static_assert(FLAME_TILE_BYTES == kBlock * 16, "a slab tile is one 16-byte vector per lane");

__global__ __launch_bounds__(kBlock) void slab_write_kernel(const ArgMeta meta, int n_entries, int64_t n_tiles) {
    (void)sizeof(meta);
    const SlabEntry* ents = (const SlabEntry*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x;
    V16 v[kSlabTPW];
    uint8_t* dp[kSlabTPW];
    int kind[kSlabTPW];   // 0 none, 1 vector, 2 bytes
#pragma unroll
    for (int j = 0; j < kSlabTPW; ++j) {
        const int64_t tile = static_cast<int64_t>(blockIdx.x) * kSlabTPW + j;
        kind[j] = 0;
        dp[j] = nullptr;
        if (tile >= n_tiles) continue;
        int lo = 0, hi = n_entries - 1;           // wave-uniform: last entry with tile_begin <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ents[mid].tile_begin <= tile) lo = mid; else hi = mid - 1;
        }
        const SlabEntry& e = ents[lo];
        const int64_t t = tile - e.tile_begin;
        const int64_t off = t * FLAME_TILE_BYTES + lane * 16;
        if (off >= e.nbytes) continue;
        dp[j] = e.dst + t * e.stride + lane * 16;
        const uint8_t* sp = e.src + off;
        const int sh = static_cast<int>(reinterpret_cast<uintptr_t>(sp) & 15);   // uniform per entry
        if (off + 16 <= e.nbytes && sh == 0) {
            v[j] = ld_nt(sp);
            kind[j] = 1;
        } else if (off + 16 <= e.nbytes) {
            // misaligned source (e.g. tensor bytes inside a channel payload): two aligned loads
            // and a byte funnel shift.  The second 16-byte block starts before the entry's last
            // byte, so it never leaves that byte's (4 KiB-aligned) page.
            const uint8_t* ab = sp - sh;
            const V16 lo = ld_nt(ab), hi = ld_nt(ab + 16);
            const uint32_t w[8] = {lo.w[0], lo.w[1], lo.w[2], lo.w[3], hi.w[0], hi.w[1], hi.w[2], hi.w[3]};
            const unsigned r = static_cast<unsigned>(sh & 3);
#define FLAME_SLAB_FUNNEL(Q) \
    for (int i = 0; i < 4; ++i) v[j].w[i] = __builtin_amdgcn_alignbyte(w[i + (Q) + 1], w[i + (Q)], r);
            switch (sh >> 2) {
            case 0: FLAME_SLAB_FUNNEL(0) break;
            case 1: FLAME_SLAB_FUNNEL(1) break;
            case 2: FLAME_SLAB_FUNNEL(2) break;
            default: FLAME_SLAB_FUNNEL(3) break;
            }
#undef FLAME_SLAB_FUNNEL
            kind[j] = 1;
        } else {                                  // ragged tail
            const int nb = static_cast<int>(e.nbytes - off < 16 ? e.nbytes - off : 16);
            for (int b = 0; b < nb; ++b) st1(dp[j] + b, ld1(sp + b));
            kind[j] = 2;
        }
    }
#pragma unroll
    for (int j = 0; j < kSlabTPW; ++j)
        if (kind[j] == 1) st_plain(dp[j], v[j]);
}

// ---------------------------------------------------------------- elementwise programs
// flame_elementwise (include/flame_amd.h): the reference's torch statements for keys the fused
// kernels do not take -- an int buffer (num_batches_tracked), a mixed-dtype or fp64 key -- as a
// short typed op list read from the kernel arguments in place (scalar loads; every wave takes the
// same switch arm).  A register holds a double (every fp32 / bf16 / fp16 value is exact in one)
// or an int64.  Such keys are small, so the registers may live in scratch.
struct EwArgs {
    flame_ew_op ops[FLAME_EW_MAX_OPS];
    void* bufs[FLAME_EW_MAX_BUFS];       // one segment: the buffers
    void* const* table;                  // segments: device [n_segs][n_bufs] buffers (else NULL)
    const int64_t* seg_end;              // segments: device [n_segs] inclusive element prefix sums
    int64_t numel;
    int32_t n_ops, n_segs, n_bufs;
};
union EwVal {
    double f;
    int64_t i;
};

__host__ __device__ __forceinline__ bool ew_float(int dt) { return dt >= FLAME_F32 && dt <= FLAME_F64; }
// an fp32 result into a 32-bit-or-narrower float dtype (torch's opmath result, rounded once)
__device__ __forceinline__ double ew_rnd32(float x, int dt) {
    if (dt == FLAME_BF16) return bf16_round(x);
    if (dt == FLAME_F16) return f16_round(x);
    return x;
}
// an int64 wrapped to the integer dtype's width (two's complement, as torch's int ops wrap)
__device__ __forceinline__ int64_t ew_wrap(int64_t x, int dt) {
    switch (dt) {
    case FLAME_I32: return static_cast<int32_t>(static_cast<uint32_t>(x));
    case FLAME_I16: return static_cast<int16_t>(static_cast<uint16_t>(x));
    case FLAME_I8: return static_cast<int8_t>(static_cast<uint8_t>(x));
    case FLAME_U8: return static_cast<uint8_t>(x);
    case FLAME_BOOL: return x != 0;
    default: return x;
    }
}
__device__ __forceinline__ EwVal ew_load(const void* p, int64_t i, int dt) {
    EwVal v;
    switch (dt) {
    case FLAME_F32: v.f = ld1(static_cast<const float*>(p) + i); break;
    case FLAME_BF16: v.f = bf16_to_f32(ld1(static_cast<const uint16_t*>(p) + i)); break;
    case FLAME_F16: v.f = f16_to_f32(ld1(static_cast<const uint16_t*>(p) + i)); break;
    case FLAME_F64: v.f = ld1(static_cast<const double*>(p) + i); break;
    case FLAME_I64: v.i = ld1(static_cast<const int64_t*>(p) + i); break;
    case FLAME_I32: v.i = ld1(static_cast<const int32_t*>(p) + i); break;
    case FLAME_I16: v.i = ld1(static_cast<const int16_t*>(p) + i); break;
    case FLAME_I8: v.i = ld1(static_cast<const int8_t*>(p) + i); break;
    default: v.i = ld1(static_cast<const uint8_t*>(p) + i); break;        // U8, BOOL
    }
    return v;
}
__device__ __forceinline__ void ew_store(void* p, int64_t i, int dt, EwVal v) {
    switch (dt) {
    case FLAME_F32: st1(static_cast<float*>(p) + i, static_cast<float>(v.f)); break;
    case FLAME_BF16: st1(static_cast<uint16_t*>(p) + i, f32_to_bf16_exact(static_cast<float>(v.f))); break;
    case FLAME_F16: st1(static_cast<uint16_t*>(p) + i, f32_to_f16_bits(static_cast<float>(v.f))); break;
    case FLAME_F64: st1(static_cast<double*>(p) + i, v.f); break;
    case FLAME_I64: st1(static_cast<int64_t*>(p) + i, v.i); break;
    case FLAME_I32: st1(static_cast<int32_t*>(p) + i, static_cast<int32_t>(v.i)); break;
    case FLAME_I16: st1(static_cast<int16_t*>(p) + i, static_cast<int16_t>(v.i)); break;
    case FLAME_I8: st1(static_cast<int8_t*>(p) + i, static_cast<int8_t>(v.i)); break;
    default: st1(static_cast<uint8_t*>(p) + i, static_cast<uint8_t>(v.i)); break;
    }
}
// CAST from dtype s to dtype t (c10's conversions: an int or an fp64 value reaches bf16 / fp16
// through fp32; a float reaches an int toward zero)
__device__ __forceinline__ EwVal ew_cast(EwVal x, int s, int t) {
    EwVal r;
    if (ew_float(t)) {
        if (t == FLAME_F64) r.f = ew_float(s) ? x.f : __ll2double_rn(x.i);
        else {
            const float f = ew_float(s) ? (s == FLAME_F64 ? __double2float_rn(x.f) : static_cast<float>(x.f))
                                        : __ll2float_rn(x.i);
            r.f = ew_rnd32(f, t);
        }
    } else if (t == FLAME_BOOL) {
        r.i = ew_float(s) ? (x.f != 0.0) : (x.i != 0);
    } else {
        r.i = ew_wrap(ew_float(s) ? __double2ll_rz(x.f) : x.i, t);
    }
    return r;
}
// a binary op in dtype dt on two values of dt (fp32 opmath for bf16 / fp16, as torch-CPU)
template <int OP>
__device__ __forceinline__ EwVal ew_bin(EwVal a, EwVal b, int dt) {
    EwVal r;
    if (dt == FLAME_F64) {
        r.f = OP == FLAME_EW_ADD ? __dadd_rn(a.f, b.f) : OP == FLAME_EW_SUB ? __dsub_rn(a.f, b.f)
            : OP == FLAME_EW_MUL ? __dmul_rn(a.f, b.f) : flame_fm::ddiv_rn(a.f, b.f);
    } else if (ew_float(dt)) {
        const float x = static_cast<float>(a.f), y = static_cast<float>(b.f);
        r.f = ew_rnd32(OP == FLAME_EW_ADD ? __fadd_rn(x, y) : OP == FLAME_EW_SUB ? __fsub_rn(x, y)
                       : OP == FLAME_EW_MUL ? __fmul_rn(x, y) : __fdiv_rn(x, y), dt);
    } else {
        const uint64_t x = static_cast<uint64_t>(a.i), y = static_cast<uint64_t>(b.i);
        r.i = ew_wrap(static_cast<int64_t>(OP == FLAME_EW_ADD ? x + y : OP == FLAME_EW_SUB ? x - y : x * y), dt);
    }
    return r;
}

// (The registers live in a private array, which the dynamic indexing puts in scratch; held in LDS
// instead, [register][lane], a 25M-element fp64 FedAdam step ran slower: 1.520 vs 1.407 ms,
// profiles/r06zh_ew_fp64_lds.log.)
// One op of a program on one element (registers r, the element's buffers and index).
__device__ __forceinline__ void ew_step(const flame_ew_op& o, EwVal* r, void* const* bufs, int64_t i) {
    const int dt = o.dtype;
    switch (o.op) {
    case FLAME_EW_LOAD: r[o.dst] = ew_load(bufs[o.a], i, dt); break;
    case FLAME_EW_STORE: ew_store(bufs[o.a], i, dt, r[o.b]); break;
    case FLAME_EW_ZERO: if (ew_float(dt)) r[o.dst].f = 0.0; else r[o.dst].i = 0; break;
    case FLAME_EW_CAST: r[o.dst] = ew_cast(r[o.a], o.b, dt); break;
    case FLAME_EW_ADD: r[o.dst] = ew_bin<FLAME_EW_ADD>(r[o.a], r[o.b], dt); break;
    case FLAME_EW_SUB: r[o.dst] = ew_bin<FLAME_EW_SUB>(r[o.a], r[o.b], dt); break;
    case FLAME_EW_MUL: r[o.dst] = ew_bin<FLAME_EW_MUL>(r[o.a], r[o.b], dt); break;
    case FLAME_EW_DIV: r[o.dst] = ew_bin<FLAME_EW_DIV>(r[o.a], r[o.b], dt); break;
    case FLAME_EW_ADD_S:
    case FLAME_EW_MUL_S: {
        EwVal s;
        if (dt == FLAME_F64) s.f = o.scalar;
        else if (ew_float(dt)) {
            // torch-CPU: a Python scalar multiplies a float tensor in fp32 (opmath) but is
            // rounded to a bf16 / fp16 tensor's dtype before it is added
            const float sf = __double2float_rn(o.scalar);
            s.f = o.op == FLAME_EW_ADD_S ? ew_rnd32(sf, dt) : sf;
        } else {
            s.i = __double2ll_rz(o.scalar);
        }
        r[o.dst] = o.op == FLAME_EW_ADD_S ? ew_bin<FLAME_EW_ADD>(r[o.a], s, dt) : ew_bin<FLAME_EW_MUL>(r[o.a], s, dt);
        break;
    }
    case FLAME_EW_SQUARE: r[o.dst] = ew_bin<FLAME_EW_MUL>(r[o.a], r[o.a], dt); break;
    case FLAME_EW_SIGN: {
        EwVal v = r[o.a];
        if (ew_float(dt)) v.f = static_cast<double>((0.0 < v.f) - (v.f < 0.0));   // NaN, -0 -> +0
        else v.i = (v.i > 0) - (v.i < 0);
        r[o.dst] = v;
        break;
    }
    case FLAME_EW_SQRT: {
        EwVal v = r[o.a];
        if (dt == FLAME_F64) v.f = flame_fm::dsqrt_rn(v.f);
        else v.f = ew_rnd32(__builtin_sqrtf(static_cast<float>(v.f)), dt);   // correctly rounded
        r[o.dst] = v;
        break;
    }
    default: break;
    }
}

// One element per lane per pass over the program: two or four (the op fetch and dispatch paid
// once for several) ran slower, 1.616 / 1.757 vs 1.411 ms per 25M-element fp64 FedAdam step
// (profiles/r06zi_ew_fp64_ilp.log) -- more registers in scratch; so did registers in LDS (1.520).
__global__ __launch_bounds__(kEwBlock) void ew_kernel(EwArgs args) {
    (void)sizeof(args);      // read in place from the kernarg segment (see agg_reduce_kernel_argmeta)
    const EwArgs* P = (const EwArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t numel = P->numel;
    const int n_ops = P->n_ops;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    void* const* table = P->table;
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < numel; g += stride) {
        // the element's segment (several keys of one program in one launch) and index in it
        int64_t i = g;
        void* const* bufs = P->bufs;
        if (table) {
            int lo = 0, hi = P->n_segs - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (P->seg_end[mid] > g) hi = mid; else lo = mid + 1;
            }
            i = g - (lo ? P->seg_end[lo - 1] : 0);
            bufs = table + static_cast<int64_t>(lo) * P->n_bufs;
        }
        EwVal r[FLAME_EW_MAX_REGS];
        for (int k = 0; k < n_ops; ++k) ew_step(P->ops[k], r, bufs, i);
    }
}

// ---------------------------------------------------------------- launch-branch counters
// Every host-side launch branch of the C ABI has an index; a successful launch counts it, so
// tests can assert which instantiation a call took and that every branch is reached by an
// oracle test (tests/test_gpu_zz_launch_branches.py).
//
// The host side from here to flame_feddyn_round:
//   * the branch table: the BR_* bases and kBranchRows, one row per family; branch_name() looks a
//     name up in it.  A new family takes the next free base, a row and a larger BR_COUNT (rows
//     that do not tile [0, BR_COUNT) do not compile).
//   * dispatch<VALUES...>(): a runtime dtype / variant / mode becomes a std::integral_constant,
//     so the fan-out over template arguments is written once per family.
//   * the shared argument checks (check_chunks, check_variant, check_flags, load_argmeta, inside).
//   * per family (agg, fedopt, hier) one pick_*(), the only rule that chooses an instantiation --
//     the device-table entry point, the kernel-argument one and flame_hier_resident_per_cu all
//     call it -- and one launch_*(), templated on where the metadata comes from.
enum : int {
    BR_AGG = 0, BR_AGG_LO = 6, BR_AGG_ARG = 9, BR_OPT = 15, BR_OPT_MULTI = 24, BR_OPT_ARG = 27, BR_SA = 36,
    BR_HIER_REG = 40, BR_HIER_LDS = 46, BR_HIER_LO = 52, BR_HIER_ARG = 55, BR_DYN = 61, BR_AGG_ARG_LO = 65,
    BR_HIER_ARG_LO = 68, BR_OPT_ARG_MULTI = 71, BR_HIER_ARG_LDS = 74, BR_CHAIN = 80, BR_AGG_LOB = 89, BR_EW = 92,
    BR_EW_SEG = 93, BR_OPT_F64 = 94, BR_CHAIN_F64 = 97, BR_COUNT = 100
};
std::atomic<long long> g_launches[BR_COUNT];

// How a branch's offset from its family's base becomes the rest of its name (dt = FLAME_F32 ..
// FLAME_I32): BK_DT offset = dt, BK_DT_VARIANT dt * 3 + variant, BK_DT_SYNC dt * 2 + sync
// (fedbuff / sync), BK_VARIANT variant, BK_NONE the prefix alone
enum BranchKey : int { BK_NONE, BK_DT, BK_DT_VARIANT, BK_DT_SYNC, BK_VARIANT };
struct BranchRow {
    int base, count;
    BranchKey key;
    const char* prefix;
    const char* suffix = "";
};
constexpr BranchRow kBranchRows[] = {
    {BR_AGG, 6, BK_DT, "flame_agg_reduce"},                        // full residency
    {BR_AGG_LO, 3, BK_DT, "flame_agg_reduce/lo"},                  // f32, bf16, f16: 2 workgroups per CU
    {BR_AGG_ARG, 6, BK_DT, "flame_agg_reduce_argmeta"},
    {BR_OPT, 9, BK_DT_VARIANT, "flame_fedopt_reduce_adapt"},       // f32, bf16, f16: one chunk per workgroup
    {BR_OPT_MULTI, 3, BK_VARIANT, "flame_fedopt_reduce_adapt/multi/f32"},      // kOptWGC chunks per workgroup
    {BR_OPT_ARG, 9, BK_DT_VARIANT, "flame_fedopt_reduce_adapt_argmeta"},
    {BR_SA, 4, BK_DT, "flame_fedbuff_scale_add"},                  // f32, bf16, f16, f64
    {BR_HIER_REG, 6, BK_DT_SYNC, "flame_hier_fedbuff/reg"},        // register store groups
    {BR_HIER_LDS, 6, BK_DT_SYNC, "flame_hier_fedbuff/lds"},        // LDS store groups (>= kHLdsMinMids middles)
    {BR_HIER_LO, 3, BK_DT, "flame_hier_fedbuff/lo", "/fedbuff"},   // one middle over a long launch, low residency
    {BR_HIER_ARG, 6, BK_DT_SYNC, "flame_hier_fedbuff_argmeta"},
    {BR_DYN, 4, BK_DT, "flame_feddyn_round"},                      // f32, bf16, f16, f64
    {BR_AGG_ARG_LO, 3, BK_DT, "flame_agg_reduce_argmeta/lo_burst"},
    {BR_HIER_ARG_LO, 3, BK_DT, "flame_hier_fedbuff_argmeta/lo", "/fedbuff"},
    {BR_OPT_ARG_MULTI, 3, BK_VARIANT, "flame_fedopt_reduce_adapt_argmeta/multi/f32"},
    {BR_HIER_ARG_LDS, 6, BK_DT_SYNC, "flame_hier_fedbuff_argmeta/lds"},
    {BR_CHAIN, 9, BK_DT_VARIANT, "flame_fedopt_chain"},            // f32, bf16, f16
    {BR_AGG_LOB, 3, BK_DT, "flame_agg_reduce/lo_burst"},           // low residency, LDS-held output bursts
    {BR_EW, 1, BK_NONE, "flame_elementwise"},
    {BR_EW_SEG, 1, BK_NONE, "flame_elementwise_segments"},
    {BR_OPT_F64, 3, BK_VARIANT, "flame_fedopt_reduce_adapt/f64"},
    {BR_CHAIN_F64, 3, BK_VARIANT, "flame_fedopt_chain/f64"},
};
constexpr bool branch_rows_tile() {
    int next = 0;
    for (const BranchRow& r : kBranchRows) {
        if (r.base != next || r.count < 1) return false;      // a gap, an overlap or rows out of index order
        next += r.count;
    }
    return next == BR_COUNT;
}
static_assert(branch_rows_tile(), "kBranchRows must tile [0, BR_COUNT) in index order, without gap or overlap");

const char* branch_name(int i) {
    static const char* const dts[6] = {"f32", "bf16", "f16", "f64", "i64", "i32"};
    static const char* const var[3] = {"fedadam", "fedyogi", "fedadagrad"};
    static char names[BR_COUNT][64];
    static const bool once = [] {
        for (const BranchRow& r : kBranchRows)
            for (int o = 0; o < r.count; ++o) {
                char* n = names[r.base + o];
                const size_t z = sizeof(names[0]);
                switch (r.key) {
                case BK_NONE: snprintf(n, z, "%s", r.prefix); break;
                case BK_DT: snprintf(n, z, "%s/%s%s", r.prefix, dts[o], r.suffix); break;
                case BK_DT_VARIANT: snprintf(n, z, "%s/%s/%s", r.prefix, dts[o / 3], var[o % 3]); break;
                case BK_DT_SYNC: snprintf(n, z, "%s/%s/%s", r.prefix, dts[o / 2], o % 2 ? "sync" : "fedbuff"); break;
                case BK_VARIANT: snprintf(n, z, "%s/%s", r.prefix, var[o]); break;
                }
            }
        return true;
    }();
    (void)once;
    return (i >= 0 && i < BR_COUNT) ? names[i] : nullptr;
}

// check_launch + count the branch on success
int launched(int br, const char* what) {
    const int rc = check_launch(what);
    if (rc == FLAME_OK) g_launches[br].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

// ---------------------------------------------------------------- compile-time dispatch
// Calls f(std::integral_constant<int, V>{}) for the V of VALUES that equals v; false when none
// does.  Inlines to the if-chain a switch would give.  A left fold: the compiler expands it, and
// so instantiates the kernels, in the order VALUES are written.
template <int V> using ic = std::integral_constant<int, V>;
template <int... VALUES, typename F>
inline bool dispatch(int v, F&& f) {
    return (... || (v == VALUES && (f(ic<VALUES>{}), true)));
}
template <typename F> inline bool dispatch_variant(int variant, F&& f) {
    return dispatch<FLAME_FEDADAM, FLAME_FEDYOGI, FLAME_FEDADAGRAD>(variant, f);
}
constexpr bool is16(int dt) { return dt == FLAME_BF16 || dt == FLAME_F16; }
constexpr bool is_f32_or_16(int dt) { return dt == FLAME_F32 || is16(dt); }

// ---------------------------------------------------------------- shared argument checks
int check_chunks(int64_t n_chunks) {
    if (n_chunks <= 0 || n_chunks > 0x7FFFFFFFll) return set_err(FLAME_EINVAL, "n_chunks out of range: %lld", (long long)n_chunks);
    return FLAME_OK;
}
int check_variant(const char* who, int variant) {
    if (variant < FLAME_FEDADAM || variant > FLAME_FEDADAGRAD) return set_err(FLAME_ENOTSUP, "%s: unknown variant %d", who, variant);
    return FLAME_OK;
}
int check_flags(const char* who, unsigned flags, unsigned allowed) {
    if (flags & ~allowed) return set_err(FLAME_EINVAL, "%s: unknown flags 0x%x", who, flags);
    return FLAME_OK;
}
// The table entry points outside the launch-branch table name themselves in every refusal
int need_segs(const char* who, const flame_segment* segs, int32_t n_segs) {
    if (!segs || n_segs <= 0) return set_err(FLAME_EINVAL, "%s: segment table is NULL or n_segs <= 0", who);
    return FLAME_OK;
}
int need_clients(const char* who, const void* clients) {
    if (!clients) return set_err(FLAME_EINVAL, "%s: client pointer table is NULL", who);
    return FLAME_OK;
}
int no_int_dtype(const char* who, int dtype) {
    if (dtype == FLAME_I64 || dtype == FLAME_I32)
        return set_err(FLAME_ENOTSUP, "%s: integer dtype %d not supported (float dtypes only)", who, dtype);
    return FLAME_OK;
}
int float_dtype(const char* who, int dtype) {
    if (int rc = no_int_dtype(who, dtype)) return rc;
    if (dtype < FLAME_F32 || dtype > FLAME_F64) return set_err(FLAME_ENOTSUP, "%s: unknown dtype %d", who, dtype);
    return FLAME_OK;
}
int no_seg_rates(const char* who, unsigned flags) {
    if (flags & FLAME_AGG_SEG_RATES) return set_err(FLAME_ENOTSUP, "%s: FLAME_AGG_SEG_RATES is not supported", who);
    return FLAME_OK;
}
int need_scratch(const char* who, const void* scratch, int64_t bytes, int64_t need) {
    if (!scratch || bytes < need)
        return set_err(FLAME_EINVAL, "%s: scratch buffer is NULL or too small (%lld bytes, %lld needed)", who,
                       static_cast<long long>(bytes), static_cast<long long>(need));
    return FLAME_OK;
}

int validate(const flame_segment* segs, int32_t n_segs, int64_t n_chunks, int32_t n_clients, const void* clients) {
    if (!segs || n_segs <= 0) return set_err(FLAME_EINVAL, "segment table is NULL or n_segs <= 0");
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_clients < 0) return set_err(FLAME_EINVAL, "n_clients < 0");
    if (n_clients > 0 && !clients) return set_err(FLAME_EINVAL, "client pointer table is NULL");
    return FLAME_OK;
}

// The kernel-argument entry points: the caller's metadata block, checked and copied into the
// ArgMeta the launch passes by value; a table of `bytes` at byte offset `off` lies inside it
int load_argmeta(const char* who, const void* host_meta, int64_t meta_bytes, ArgMeta& m) {
    if (!host_meta || meta_bytes <= 0 || meta_bytes % 8 || meta_bytes > static_cast<int64_t>(sizeof(ArgMeta)))
        return set_err(FLAME_EINVAL, "%s: metadata block must be 8..%d bytes, a multiple of 8", who,
                       static_cast<int>(sizeof(ArgMeta)));
    std::memcpy(m.w, host_meta, static_cast<size_t>(meta_bytes));
    return FLAME_OK;
}

bool inside(int64_t meta_bytes, int64_t off, int64_t bytes) { return off >= 0 && off % 8 == 0 && off + bytes <= meta_bytes; }

// ---------------------------------------------------------------- flame_agg_reduce[_argmeta]
// Where a launch's metadata comes from: tables in device memory, or word offsets into the ArgMeta
// that travels as the first kernel argument
struct AggTables { const flame_segment* segs; const uint64_t* clients; const float* r32; const double* r64; };
struct AggArgMeta { const ArgMeta* m; int oc, o32, o64; };
constexpr unsigned kAggFlags = FLAME_AGG_INIT_FIRST | FLAME_AGG_SEG_RATES | FLAME_AGG_XCD_MAP;

int check_agg_flags(const char* who, unsigned flags, int32_t n_clients) {
    if ((flags & FLAME_AGG_INIT_FIRST) && n_clients < 1)
        return set_err(FLAME_EINVAL, "FLAME_AGG_INIT_FIRST needs at least one client");
    return check_flags(who, flags, kAggFlags);
}

enum AggMode : int {
    AGG_FULL,  // one chunk per workgroup, full residency
    AGG_LO,    // long-lived workgroups over many chunks: two per CU, fewer loads in flight per lane
    AGG_LOB    // the same with kLoWGC chunks' outputs held in LDS and stored in bursts
};
int pick_agg(int dtype, int32_t n_clients, int64_t n_chunks, bool argmeta) {
    // f64 / integers have no low-residency instantiation: the general launch
    if (!is_f32_or_16(dtype) || n_clients < kLoMinClients || n_chunks < kLoMinChunks) return AGG_FULL;
    // the kernel-argument block cannot hold enough clients to need the plain instantiation
    static_assert((kArgMetaWords - 10) < kLoBurstMaxClients,
                  "a kernel-argument launch can hold kLoBurstMaxClients clients: it needs the plain instantiation too");
    return (argmeta || n_clients < kLoBurstMaxClients) ? AGG_LOB : AGG_LO;
}
constexpr bool agg_exists(int dt, int mode, bool argmeta) {
    return mode == AGG_FULL || (is_f32_or_16(dt) && !(argmeta && mode == AGG_LO));
}
constexpr int agg_branch(int mode, bool argmeta) {
    if (argmeta) return mode == AGG_FULL ? BR_AGG_ARG : BR_AGG_ARG_LO;
    return mode == AGG_FULL ? BR_AGG : mode == AGG_LO ? BR_AGG_LO : BR_AGG_LOB;
}
template <int DT, int MODE> struct AggInst {
    static constexpr int CU = MODE != AGG_FULL ? (is16(DT) ? kLoUnroll16 : kLoUnroll)
                              : (DT == FLAME_I64 || DT == FLAME_I32) ? 4 : is16(DT) ? kClientUnroll16 : kClientUnroll;
    static constexpr int G = MODE == AGG_LOB ? kLoWGC : 1;       // chunks per workgroup
    static constexpr int LDS = MODE == AGG_LOB ? kLoDynLds : MODE == AGG_LO ? kLoLds : 0;   // a residency cap
};

template <typename SRC>
inline int launch_agg(const char* who, int dtype, unsigned flags, const SRC& src, int32_t n_segs, int32_t n_clients,
                      int64_t n_chunks, void* stream) {
    constexpr bool kArg = std::is_same<SRC, AggArgMeta>::value;
    const int mode = pick_agg(dtype, n_clients, n_chunks, kArg);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bool known = false;
    dispatch<AGG_LOB, AGG_LO, AGG_FULL>(mode, [&](auto md) {
        known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64, FLAME_I64, FLAME_I32>(dtype, [&](auto dt) {
            constexpr int DT = decltype(dt)::value, MODE = decltype(md)::value;
            if constexpr (agg_exists(DT, MODE, kArg)) {
                using I = AggInst<DT, MODE>;
                const dim3 grid(static_cast<unsigned>((n_chunks + I::G - 1) / I::G)), block(kBlock);
                if constexpr (kArg)
                    hipLaunchKernelGGL((agg_reduce_kernel_argmeta<DT, I::CU, I::G>), grid, block, I::LDS, st, *src.m,
                                       n_segs, n_clients, src.oc, src.o32, src.o64, flags, n_chunks);
                else
                    hipLaunchKernelGGL((agg_reduce_kernel<DT, I::CU, I::G>), grid, block, I::LDS, st, src.segs, n_segs,
                                       src.clients, n_clients, src.r32, src.r64, flags, n_chunks);
            }
        });
    });
    if (!known) return set_err(FLAME_ENOTSUP, "%s: unsupported dtype %d", who, dtype);
    return launched(agg_branch(mode, kArg) + dtype, who);
}

// ---------------------------------------------------------------- flame_fedopt_reduce_adapt[_argmeta]
struct Hyper32 { float b1, omb1, b2, omb2, eta, tau; };
struct OptTables { const flame_segment* segs; const uint64_t* clients; const float* r32; };
struct OptArgMeta { const ArgMeta* m; int oc, o32; };
constexpr unsigned kOptFlags = FLAME_OPT_STATE_ZERO | FLAME_OPT_XCD_MAP;

// kOptWGC chunks per workgroup (outputs held in LDS) for fp32 launches big enough to fill the
// GPU several times over; one chunk per workgroup otherwise
bool pick_opt(int dtype, int64_t n_chunks) { return dtype == FLAME_F32 && n_chunks >= 8ll * 256 * kOptWGC; }
template <int DT, bool MULTI> struct OptInst {
    static constexpr int CU = MULTI ? kOptUnroll : is16(DT) ? kClientUnroll16 : kClientUnroll;
    static constexpr int G = MULTI ? kOptWGC : 1;
};

// the caller has checked the variant
template <typename SRC>
inline int launch_opt(const char* who, int dtype, int variant, unsigned flags, const SRC& src, int32_t n_segs,
                      int32_t n_clients, int64_t n_chunks, const Hyper32& h, void* stream) {
    constexpr bool kArg = std::is_same<SRC, OptArgMeta>::value;
    const bool multi = pick_opt(dtype, n_chunks);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) {
        dispatch<1, 0>(multi, [&](auto mu) {
            dispatch_variant(variant, [&](auto vr) {
                constexpr int DT = decltype(dt)::value, V = decltype(vr)::value;
                constexpr bool MULTI = decltype(mu)::value != 0;
                if constexpr (!MULTI || DT == FLAME_F32) {
                    using I = OptInst<DT, MULTI>;
                    const dim3 grid(static_cast<unsigned>((n_chunks + I::G - 1) / I::G)), block(kBlock);
                    if constexpr (kArg)
                        hipLaunchKernelGGL((fedopt_kernel_argmeta<DT, V, I::CU, I::G>), grid, block, 0, st, *src.m, n_segs,
                                           n_clients, src.oc, src.o32, flags, h.b1, h.omb1, h.b2, h.omb2, h.eta, h.tau,
                                           n_chunks);
                    else
                        hipLaunchKernelGGL((fedopt_kernel<DT, V, I::CU, I::G>), grid, block, 0, st, src.segs, n_segs,
                                           src.clients, n_clients, src.r32, flags, h.b1, h.omb1, h.b2, h.omb2, h.eta,
                                           h.tau, n_chunks);
                }
            });
        });
    });
    if (!known) return set_err(FLAME_ENOTSUP, "%s: dtype %d not supported (f32, bf16, f16)", who, dtype);
    if (multi) return launched((kArg ? BR_OPT_ARG_MULTI : BR_OPT_MULTI) + variant, who);
    return launched((kArg ? BR_OPT_ARG : BR_OPT) + dtype * 3 + variant, who);
}

// ---------------------------------------------------------------- flame_hier_fedbuff[_argmeta]
struct HierTables {
    const flame_hier_segment* segs;
    const uint64_t *mid_w, *mid_delta, *clients;
    const float *mid_rates, *mid_goal, *top_rates;
};
struct HierArgMeta { const ArgMeta* m; int ow, od, oc, orr, og, ot; };

int check_hier_flags(const char* who, unsigned flags, float top_goal) {
    if (int rc = check_flags(who, flags, FLAME_HIER_TOP_ACCUM | FLAME_HIER_TOP_APPLY | FLAME_HIER_MID_READONLY | FLAME_HIER_SYNC))
        return rc;
    if ((flags & FLAME_HIER_SYNC) && ((flags & FLAME_HIER_TOP_APPLY) || !(flags & FLAME_HIER_TOP_ACCUM)))
        return set_err(FLAME_EINVAL, "%s: FLAME_HIER_SYNC needs FLAME_HIER_TOP_ACCUM (the top's FedAvg starts from "
                                     "its weights) and no FLAME_HIER_TOP_APPLY", who);
    if ((flags & FLAME_HIER_TOP_APPLY) && top_goal == 0.f) return set_err(FLAME_EINVAL, "top agg_goal must be nonzero");
    return FLAME_OK;
}

// Many middles (config 5: 64 per GPU): LDS-held store groups.  One middle over a long launch
// (a FedBuff aggregator's fused scale_add / a middle's scale_add + delta over >= 64 queued
// arrivals): fewer workgroups per CU, fewer loads in flight -- fp32 2 per CU, 16-bit 3 per CU,
// unroll 3 (64 x 25M: 1.058 -> 0.989 ms fp32, 0.533 -> 0.509 ms bf16; tools/fedbuff_sweep.py,
// profiles/r03zv_fedbuff_*.log).  Otherwise (small hierarchies): register groups, full residency.
struct HierPick { bool lds, lo, sync; };
HierPick pick_hier(unsigned flags, int32_t n_mids, int32_t n_clients, int64_t n_chunks) {
    HierPick p;
    p.sync = (flags & FLAME_HIER_SYNC) != 0;
    p.lds = n_mids >= kHLdsMinMids;
    p.lo = !p.lds && !p.sync && n_mids == 1 && n_clients >= kHLoMinClients && n_chunks >= kHLoMinChunks;
    return p;
}
int hier_branch(const HierPick& p, bool argmeta, int dtype) {
    if (p.lo) return (argmeta ? BR_HIER_ARG_LO : BR_HIER_LO) + dtype;
    const int base = p.lds ? (argmeta ? BR_HIER_ARG_LDS : BR_HIER_LDS) : (argmeta ? BR_HIER_ARG : BR_HIER_REG);
    return base + dtype * 2 + p.sync;
}
template <int DT_, bool LDS_, bool LO, bool SYNC_> struct HierInst {
    static constexpr int DT = DT_;
    static constexpr bool SYNC = SYNC_;
    static constexpr int CU = LO ? kHLoUnroll : !is16(DT) ? kClientUnroll : LDS_ ? kHierLdsUnroll16 : kHierUnroll16;
    static constexpr int HB = LDS_ ? kHBL : kHB;        // middles per store group
    static constexpr bool HL = LDS_;                    // store groups held in LDS
    static constexpr int LDS = !LO ? 0 : is16(DT) ? kHLoLds16 : kHLoLdsF32;   // a residency cap
};
// Calls f(HierInst<...>{}) for the instantiation p selects; false for a dtype without kernels
template <typename F>
inline bool dispatch_hier(int dtype, const HierPick& p, F&& f) {
    return dispatch<FLAME_F32, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (p.lds) {
            if (p.sync) f(HierInst<DT, true, false, true>{});
            else f(HierInst<DT, true, false, false>{});
        } else if (p.lo) {
            f(HierInst<DT, false, true, false>{});
        } else {
            if (p.sync) f(HierInst<DT, false, false, true>{});
            else f(HierInst<DT, false, false, false>{});
        }
    });
}

template <typename SRC>
inline int launch_hier(const char* who, int dtype, unsigned flags, const SRC& src, int32_t n_segs, int64_t n_chunks,
                       int32_t n_mids, int32_t n_clients, float top_goal, void* stream) {
    constexpr bool kArg = std::is_same<SRC, HierArgMeta>::value;
    const HierPick p = pick_hier(flags, n_mids, n_clients, n_chunks);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    const bool known = dispatch_hier(dtype, p, [&](auto inst) {
        using I = decltype(inst);
        if constexpr (kArg)
            hipLaunchKernelGGL((hier_fedbuff_kernel_argmeta<I::DT, I::CU, I::SYNC, I::HB, I::HL>), grid, block, I::LDS, st,
                               *src.m, n_segs, n_mids, n_clients, src.ow, src.od, src.oc, src.orr, src.og, src.ot,
                               top_goal, flags);
        else
            hipLaunchKernelGGL((hier_fedbuff_kernel<I::DT, I::CU, I::SYNC, I::HB, I::HL>), grid, block, I::LDS, st,
                               src.segs, n_segs, n_mids, n_clients, src.mid_w, src.mid_delta, src.clients, src.mid_rates,
                               src.mid_goal, src.top_rates, top_goal, flags);
    });
    if (!known) return set_err(FLAME_ENOTSUP, "%s: dtype %d not supported (f32, bf16, f16)", who, dtype);
    return launched(hier_branch(p, kArg, dtype), who);
}

}  // namespace

// ==================================================================== C ABI
extern "C" {

int flame_abi_version(void) { return FLAME_ABI_VERSION; }

const char* flame_last_error(void) { return g_err; }

int64_t flame_chunk_elems(int dtype) {
    int64_t n = 0;
    dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64, FLAME_I64, FLAME_I32>(
        dtype, [&](auto dt) { n = chunk_elems<decltype(dt)::value>(); });
    if (dtype == FLAME_FP8_E4M3 || dtype == FLAME_FP8_E5M2) n = static_cast<int64_t>(kBlock) * kMxEPT;   // flame_agg_reduce_mx only
    if (dtype == FLAME_FP4_E2M1) n = static_cast<int64_t>(kBlock) * kMx4EPT;                              // flame_agg_reduce_mxfp4 only
    return n;
}

int64_t flame_scale_add_chunk_elems(int dtype) {
    int64_t n = 0;
    dispatch<FLAME_F32, FLAME_F64, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) { n = kEwBlock * SA<decltype(dt)::value>::EPT; });
    return n;
}

int flame_agg_reduce(int dtype, unsigned flags, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                     const void* const* clients, int32_t n_clients, const float* rates32, const double* rates64,
                     void* stream) {
    const char* const who = "flame_agg_reduce";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (int rc = check_agg_flags(who, flags, n_clients)) return rc;
    if (dtype == FLAME_F64 ? (n_clients > 0 && !rates64) : (n_clients > 0 && !rates32))
        return set_err(FLAME_EINVAL, "rate array is NULL");
    const AggTables src{segs, reinterpret_cast<const uint64_t*>(clients), rates32, rates64};
    return launch_agg(who, dtype, flags, src, n_segs, n_clients, n_chunks, stream);
}

int flame_agg_reduce_argmeta(int dtype, unsigned flags, const void* host_meta, int64_t meta_bytes, int32_t n_segs,
                             int64_t n_chunks, int32_t n_clients, int64_t off_clients, int64_t off_r32,
                             int64_t off_r64, void* stream) {
    const char* const who = "flame_agg_reduce_argmeta";
    ArgMeta m;
    if (int rc = load_argmeta(who, host_meta, meta_bytes, m)) return rc;
    if (n_segs <= 0 || n_clients < 0) return set_err(FLAME_EINVAL, "%s: n_segs <= 0 or n_clients < 0", who);
    if (int rc = check_chunks(n_chunks)) return rc;
    if (int rc = check_agg_flags(who, flags, n_clients)) return rc;
    const int64_t rows = (flags & FLAME_AGG_SEG_RATES) ? n_segs : 1;
    if (static_cast<int64_t>(n_segs) * static_cast<int64_t>(sizeof(flame_segment)) > meta_bytes ||
        !inside(meta_bytes, off_clients, static_cast<int64_t>(n_segs) * n_clients * 8))
        return set_err(FLAME_EINVAL, "%s: segment / client table outside the metadata block", who);
    const bool f64 = dtype == FLAME_F64;
    if (n_clients > 0 && !(f64 ? inside(meta_bytes, off_r64, rows * n_clients * 8) : inside(meta_bytes, off_r32, rows * n_clients * 4)))
        return set_err(FLAME_EINVAL, "%s: rate array outside the metadata block", who);
    const AggArgMeta src{&m, static_cast<int>(off_clients / 8), (!f64 && n_clients > 0) ? static_cast<int>(off_r32 / 8) : -1,
                         (f64 && n_clients > 0) ? static_cast<int>(off_r64 / 8) : -1};
    return launch_agg(who, dtype, flags, src, n_segs, n_clients, n_chunks, stream);
}

int64_t flame_agg_argmeta_max_bytes(void) { return static_cast<int64_t>(sizeof(ArgMeta)); }

// The update guard's two entry points stand outside the launch-branch table, as flame_slab_write
// and flame_synth_fill do: one instantiation per dtype, nothing to pick.
int flame_agg_reduce_scaled(int dtype, unsigned flags, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                            const void* const* clients, int32_t n_clients, const float* rates32,
                            const double* rates64, const float* scales32, const double* scales64, void* stream) {
    const char* const who = "flame_agg_reduce_scaled";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_agg_flags(who, flags, n_clients)) return rc;
    if (int rc = no_int_dtype(who, dtype)) return rc;
    const bool f64 = dtype == FLAME_F64;
    if (n_clients > 0 && !(f64 ? rates64 : static_cast<const void*>(rates32))) return set_err(FLAME_EINVAL, "%s: rate array is NULL", who);
    if (n_clients > 0 && !(f64 ? scales64 : static_cast<const void*>(scales32))) return set_err(FLAME_EINVAL, "%s: scale array is NULL", who);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        constexpr int CU = is16(DT) ? kClientUnroll16 : kClientUnroll;
        hipLaunchKernelGGL((agg_reduce_scaled_kernel<DT, CU>), dim3(static_cast<unsigned>(n_chunks)), dim3(kBlock), 0, st, segs,
                           n_segs, reinterpret_cast<const uint64_t*>(clients), n_clients, rates32, rates64, scales32,
                           scales64, flags, n_chunks);
    });
    if (!known) return set_err(FLAME_ENOTSUP, "%s: unknown dtype %d", who, dtype);
    return check_launch(who);
}

// 16-bit updates into an fp32 aggregate: outside the launch-branch table as well, one
// instantiation per client dtype and SCALED.  Every refusal comes before the first HIP call.
int flame_agg_reduce_mixed(int client_dtype, int agg_dtype, unsigned flags, const flame_segment* segs, int32_t n_segs,
                           int64_t n_chunks, const void* const* clients, int32_t n_clients, const float* rates32,
                           const float* scales32, void* stream) {
    const char* const who = "flame_agg_reduce_mixed";
    if (!is16(client_dtype) || agg_dtype != FLAME_F32)
        return set_err(FLAME_ENOTSUP, "%s: client dtype %d into aggregate dtype %d is not supported (bf16 or f16 into f32 only)",
                       who, client_dtype, agg_dtype);
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return set_err(rc, "%s: n_chunks out of range: %lld", who, (long long)n_chunks);
    if (n_clients < 1) return set_err(FLAME_EINVAL, "%s: n_clients < 1", who);
    if (int rc = need_clients(who, clients)) return rc;
    if (!rates32) return set_err(FLAME_EINVAL, "%s: rate array is NULL", who);
    if (flags & FLAME_AGG_INIT_FIRST)
        return set_err(FLAME_ENOTSUP, "%s: FLAME_AGG_INIT_FIRST is not supported (a None-start aggregate takes the update's dtype)", who);
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_flags(who, flags, FLAME_AGG_XCD_MAP)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint64_t* cl = reinterpret_cast<const uint64_t*>(clients);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    dispatch<FLAME_BF16, FLAME_F16>(client_dtype, [&](auto dt) {
        constexpr int CD = decltype(dt)::value;
        if (scales32)
            hipLaunchKernelGGL((agg_reduce_mixed_kernel<CD, kClientUnroll16, true>), grid, block, 0, st, segs, n_segs, cl,
                               n_clients, rates32, scales32, flags, n_chunks);
        else
            hipLaunchKernelGGL((agg_reduce_mixed_kernel<CD, kClientUnroll16, false>), grid, block, 0, st, segs, n_segs, cl,
                               n_clients, rates32, scales32, flags, n_chunks);
    });
    return check_launch(who);
}

// MXFP8 updates into an fp32 aggregate: flame_agg_reduce_mixed's arguments plus the table of scale
// byte pointers.  Outside the launch-branch table, one instantiation per element format and SCALED;
// every refusal comes before the first HIP call.
int flame_agg_reduce_mx(int client_dtype, int agg_dtype, unsigned flags, const flame_segment* segs, int32_t n_segs,
                        int64_t n_chunks, const void* const* clients, const void* const* block_scales, int32_t n_clients,
                        const float* rates32, const float* scales32, void* stream) {
    const char* const who = "flame_agg_reduce_mx";
    if ((client_dtype != FLAME_FP8_E4M3 && client_dtype != FLAME_FP8_E5M2) || agg_dtype != FLAME_F32)
        return set_err(FLAME_ENOTSUP, "%s: client dtype %d into aggregate dtype %d is not supported (fp8 e4m3 or e5m2 into f32 only)",
                       who, client_dtype, agg_dtype);
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return set_err(rc, "%s: n_chunks out of range: %lld", who, (long long)n_chunks);
    if (n_clients < 1) return set_err(FLAME_EINVAL, "%s: n_clients < 1", who);
    if (int rc = need_clients(who, clients)) return rc;
    if (!block_scales) return set_err(FLAME_EINVAL, "%s: block scale pointer table is NULL", who);
    if (!rates32) return set_err(FLAME_EINVAL, "%s: rate array is NULL", who);
    if (flags & FLAME_AGG_INIT_FIRST)
        return set_err(FLAME_ENOTSUP, "%s: FLAME_AGG_INIT_FIRST is not supported (an MX update has no aggregate dtype of its own)", who);
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_flags(who, flags, FLAME_AGG_XCD_MAP)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint64_t* cl = reinterpret_cast<const uint64_t*>(clients);
    const uint64_t* bs = reinterpret_cast<const uint64_t*>(block_scales);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    dispatch<FLAME_FP8_E4M3, FLAME_FP8_E5M2>(client_dtype, [&](auto dt) {
        constexpr int CD = decltype(dt)::value;
        if (scales32)
            hipLaunchKernelGGL((agg_reduce_mx_kernel<CD, kClientUnrollMx, true>), grid, block, 0, st, segs, n_segs, cl, bs,
                               n_clients, rates32, scales32, flags, n_chunks);
        else
            hipLaunchKernelGGL((agg_reduce_mx_kernel<CD, kClientUnrollMx, false>), grid, block, 0, st, segs, n_segs, cl, bs,
                               n_clients, rates32, scales32, flags, n_chunks);
    });
    return check_launch(who);
}

// MXFP4 updates into an fp32 aggregate: flame_agg_reduce_mx's arguments, its own entry point (that one
// keeps refusing every code but its two).  One instantiation per SCALED; every refusal comes before
// the first HIP call.  The segment table lives in device memory, so client_tile_stride cannot be
// looked at here: the kernel does not read the field (engine.py never builds a tiled MX row).
int flame_agg_reduce_mxfp4(int client_dtype, int agg_dtype, unsigned flags, const flame_segment* segs, int32_t n_segs,
                           int64_t n_chunks, const void* const* clients, const void* const* block_scales,
                           int32_t n_clients, const float* rates32, const float* scales32, void* stream) {
    const char* const who = "flame_agg_reduce_mxfp4";
    if (client_dtype != FLAME_FP4_E2M1 || agg_dtype != FLAME_F32)
        return set_err(FLAME_ENOTSUP, "%s: client dtype %d into aggregate dtype %d is not supported (fp4 e2m1 into f32 only)",
                       who, client_dtype, agg_dtype);
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return set_err(rc, "%s: n_chunks out of range: %lld", who, (long long)n_chunks);
    if (n_clients < 1) return set_err(FLAME_EINVAL, "%s: n_clients < 1", who);
    if (int rc = need_clients(who, clients)) return rc;
    if (!block_scales) return set_err(FLAME_EINVAL, "%s: block scale pointer table is NULL", who);
    if (!rates32) return set_err(FLAME_EINVAL, "%s: rate array is NULL", who);
    if (flags & FLAME_AGG_INIT_FIRST)
        return set_err(FLAME_ENOTSUP, "%s: FLAME_AGG_INIT_FIRST is not supported (an MX update has no aggregate dtype of its own)", who);
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_flags(who, flags, FLAME_AGG_XCD_MAP)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint64_t* cl = reinterpret_cast<const uint64_t*>(clients);
    const uint64_t* bs = reinterpret_cast<const uint64_t*>(block_scales);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    if (scales32)
        hipLaunchKernelGGL((agg_reduce_mxfp4_kernel<kClientUnrollMx4, true>), grid, block, 0, st, segs, n_segs, cl, bs,
                           n_clients, rates32, scales32, flags, n_chunks);
    else
        hipLaunchKernelGGL((agg_reduce_mxfp4_kernel<kClientUnrollMx4, false>), grid, block, 0, st, segs, n_segs, cl, bs,
                           n_clients, rates32, scales32, flags, n_chunks);
    return check_launch(who);
}

// The trimmed mean stands outside the launch-branch table too: the chain capacity follows from
// trim_k alone (the smallest instantiated KT >= trim_k), nothing else is picked.
int flame_agg_trimmed_max_k(void) { return kTrimMaxK; }

int flame_agg_trimmed(int dtype, unsigned flags, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                      const void* const* clients, int32_t n_clients, int32_t trim_k, void* stream) {
    const char* const who = "flame_agg_trimmed";
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return rc;
    if (int rc = need_clients(who, clients)) return rc;
    if (trim_k < 0 || trim_k > kTrimMaxK)
        return set_err(trim_k < 0 ? FLAME_EINVAL : FLAME_ENOTSUP, "%s: trim_k %d outside [0, %d] (flame_agg_trimmed_max_k)", who,
                       trim_k, kTrimMaxK);
    if (n_clients <= 2 * trim_k)
        return set_err(FLAME_EINVAL, "%s: n_clients %d must exceed 2 * trim_k = %d", who, n_clients, 2 * trim_k);
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_flags(who, flags, FLAME_AGG_INIT_FIRST | FLAME_AGG_XCD_MAP)) return rc;
    if (int rc = float_dtype(who, dtype)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    constexpr int kCaps[] = {1, 2, 3, 4, 6, 8, 12, 16};      // a round pays for KT stages, not for trim_k
    static_assert(kCaps[7] == kTrimMaxK, "the capacities end at kTrimMaxK");
    int kt = kTrimMaxK;
    for (int i = 7; i >= 0; --i)
        if (kCaps[i] >= trim_k) kt = kCaps[i];
    dispatch<1, 2, 3, 4, 6, 8, 12, 16>(kt, [&](auto cap) {
        dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
            hipLaunchKernelGGL((agg_trimmed_kernel<decltype(dt)::value, decltype(cap)::value>),
                               dim3(static_cast<unsigned>(n_chunks)), dim3(kBlock), 0, st, segs, n_segs,
                               reinterpret_cast<const uint64_t*>(clients), n_clients, trim_k, flags, n_chunks);
        });
    });
    return check_launch(who);
}

// The selection by radix passes: one instantiation per dtype, any trim_k; the client count is
// bounded by the histograms' 16-bit counters.
int flame_agg_select_max_clients(void) { return kSelectMaxClients; }

int flame_agg_select(int dtype, unsigned flags, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                     const void* const* clients, int32_t n_clients, int32_t trim_k, void* stream) {
    const char* const who = "flame_agg_select";
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return rc;
    if (int rc = need_clients(who, clients)) return rc;
    if (trim_k < 0) return set_err(FLAME_EINVAL, "%s: trim_k %d is negative", who, trim_k);
    if (n_clients > kSelectMaxClients)
        return set_err(FLAME_ENOTSUP, "%s: n_clients %d exceeds %d (flame_agg_select_max_clients)", who, n_clients,
                       kSelectMaxClients);
    if (static_cast<int64_t>(n_clients) <= 2 * static_cast<int64_t>(trim_k))
        return set_err(FLAME_EINVAL, "%s: n_clients %d must exceed 2 * trim_k = %lld", who, n_clients,
                       2 * static_cast<long long>(trim_k));
    if (int rc = no_seg_rates(who, flags)) return rc;
    if (int rc = check_flags(who, flags, FLAME_AGG_INIT_FIRST | FLAME_AGG_XCD_MAP)) return rc;
    if (int rc = float_dtype(who, dtype)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((agg_select_kernel<decltype(dt)::value>), dim3(static_cast<unsigned>(n_chunks)), dim3(kBlock), 0,
                           st, segs, n_segs, reinterpret_cast<const uint64_t*>(clients), n_clients, trim_k, flags, n_chunks);
    });
    return check_launch(who);
}

int64_t flame_update_stats_scratch_bytes(int64_t n_chunks, int32_t n_clients) {
    if (n_chunks <= 0 || n_chunks > 0x7FFFFFFFll || n_clients <= 0) return 0;
    return (n_chunks + kStatR - 1) / kStatR * static_cast<int64_t>(n_clients) * static_cast<int64_t>(sizeof(double));
}

// flame_update_stats and flame_update_dist are the two instantiations of one pass (CEN: with a
// centre); they share every check, the scratch layout and the finish kernel.
static int launch_stats(const char* who, bool cen, int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                        const void* const* clients, int32_t n_clients, double* sums, int64_t* nonfinite, void* scratch,
                        int64_t scratch_bytes, void* stream) {
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_clients <= 0) return set_err(FLAME_EINVAL, "%s: n_clients <= 0", who);
    if (int rc = need_clients(who, clients)) return rc;
    if (int rc = float_dtype(who, dtype)) return rc;
    if (!sums || !nonfinite) return set_err(FLAME_EINVAL, "%s: output array is NULL", who);
    if (int rc = need_scratch(who, scratch, scratch_bytes, flame_update_stats_scratch_bytes(n_chunks, n_clients))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_wg = (n_chunks + kStatR - 1) / kStatR;
    dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        hipLaunchKernelGGL((cen ? update_stats_kernel<DT, true> : update_stats_kernel<DT, false>),
                           dim3(static_cast<unsigned>(n_wg)), dim3(kBlock), 0, st, segs, n_segs,
                           reinterpret_cast<const uint64_t*>(clients), n_clients, n_chunks, n_wg,
                           static_cast<double*>(scratch), reinterpret_cast<unsigned long long*>(nonfinite));
    });
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(update_stats_finish_kernel, dim3(static_cast<unsigned>(n_clients)), dim3(kBlock), 0, st,
                       static_cast<const double*>(scratch), n_wg, sums);
    return check_launch(who);
}

int flame_update_stats(int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                       const void* const* clients, int32_t n_clients, double* sumsq, int64_t* nonfinite,
                       void* scratch, int64_t scratch_bytes, void* stream) {
    return launch_stats("flame_update_stats", false, dtype, segs, n_segs, n_chunks, clients, n_clients, sumsq, nonfinite,
                        scratch, scratch_bytes, stream);
}

// The distances to a centre (RFA): the same pass with segs[s].in read as the centre of segment s.
int64_t flame_update_dist_scratch_bytes(int64_t n_chunks, int32_t n_clients) {
    return flame_update_stats_scratch_bytes(n_chunks, n_clients);
}

int flame_update_dist(int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                      const void* const* clients, int32_t n_clients, double* dist2, int64_t* nonfinite,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    return launch_stats("flame_update_dist", true, dtype, segs, n_segs, n_chunks, clients, n_clients, dist2, nonfinite,
                        scratch, scratch_bytes, stream);
}

// The Gram stands outside the launch-branch table as the statistics do: one instantiation per dtype.
int flame_update_gram_max_clients(void) { return kGramMaxClients; }

// An upper bound of what a launch writes (pairs x ranges partials), monotone in both arguments:
// ranges <= ceil(n_chunks / kGramMinR) and pairs x ranges <= kGramTargetWG + pairs (gram_range).
int64_t flame_update_gram_scratch_bytes(int64_t n_chunks, int32_t n_clients) {
    if (n_chunks <= 0 || n_chunks > 0x7FFFFFFFll || n_clients <= 0 || n_clients > kGramMaxClients) return 0;
    const int64_t pairs = gram_pairs(n_clients);
    const int64_t a = (n_chunks + kGramMinR - 1) / kGramMinR * pairs, b = kGramTargetWG + pairs;
    return (a < b ? a : b) * kGramPart * static_cast<int64_t>(sizeof(double));
}

int flame_update_gram(int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                      const void* const* clients, int32_t n_clients, double* gram, int64_t* nonfinite,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    const char* const who = "flame_update_gram";
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_clients <= 0) return set_err(FLAME_EINVAL, "%s: n_clients <= 0", who);
    if (n_clients > kGramMaxClients)
        return set_err(FLAME_ENOTSUP, "%s: n_clients %d exceeds %d (flame_update_gram_max_clients)", who, n_clients,
                       kGramMaxClients);
    if (int rc = need_clients(who, clients)) return rc;
    if (int rc = float_dtype(who, dtype)) return rc;
    if (!gram || !nonfinite) return set_err(FLAME_EINVAL, "%s: output array is NULL", who);
    if (int rc = need_scratch(who, scratch, scratch_bytes, flame_update_gram_scratch_bytes(n_chunks, n_clients))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t range = gram_range(n_chunks, n_clients);
    const int64_t n_ranges = (n_chunks + range - 1) / range;
    const int n_pairs = static_cast<int>(gram_pairs(n_clients));
    dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((update_gram_kernel<decltype(dt)::value>),
                           dim3(static_cast<unsigned>(n_pairs), static_cast<unsigned>(n_ranges)), dim3(kBlock), 0, st, segs,
                           n_segs, reinterpret_cast<const uint64_t*>(clients), n_clients, n_chunks, range, n_pairs,
                           static_cast<double*>(scratch), reinterpret_cast<unsigned long long*>(nonfinite));
    });
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(gram_finish_kernel, dim3(static_cast<unsigned>(n_pairs), kGramFinishSplit), dim3(kBlock), 0, st,
                       static_cast<const double*>(scratch), n_ranges, n_pairs, n_clients, gram);
    return check_launch(who);
}

int flame_fedopt_reduce_adapt(int dtype, int variant, unsigned flags, const flame_segment* segs, int32_t n_segs,
                              int64_t n_chunks, const void* const* clients, int32_t n_clients,
                              const float* rates32, float b1, float omb1, float b2, float omb2, float eta,
                              float tau, void* stream) {
    const char* const who = "flame_fedopt_reduce_adapt";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (n_clients > 0 && !rates32) return set_err(FLAME_EINVAL, "rate array is NULL");
    if (int rc = check_variant(who, variant)) return rc;
    if (int rc = check_flags(who, flags, kOptFlags)) return rc;
    const OptTables src{segs, reinterpret_cast<const uint64_t*>(clients), rates32};
    return launch_opt(who, dtype, variant, flags, src, n_segs, n_clients, n_chunks, Hyper32{b1, omb1, b2, omb2, eta, tau},
                      stream);
}

int flame_fedopt_chain(int dtype, int variant, unsigned flags, const flame_segment* segs, int32_t n_segs,
                       int64_t n_chunks, const void* const* clients, int32_t n_clients, const float* rates32,
                       const uint8_t* step_end, float b1, float omb1, float b2, float omb2, float eta, float tau,
                       void* stream) {
    const char* const who = "flame_fedopt_chain";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (n_clients < 1 || !rates32 || !step_end)
        return set_err(FLAME_EINVAL, "%s: needs >= 1 client, a rate array and a step_end array", who);
    if (int rc = check_variant(who, variant)) return rc;
    if (int rc = check_flags(who, flags, FLAME_OPT_STATE_ZERO)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    auto cl = reinterpret_cast<const uint64_t*>(clients);
    const bool known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) {
        dispatch_variant(variant, [&](auto vr) {
            constexpr int DT = decltype(dt)::value, V = decltype(vr)::value;
            constexpr int CU = is16(DT) ? kChainUnroll16 : kChainUnroll;
            hipLaunchKernelGGL((fedopt_chain_kernel<DT, V, CU>), grid, block, DT == FLAME_F32 ? kChainLds : 0, st, segs,
                               n_segs, cl, n_clients, rates32, step_end, flags, b1, omb1, b2, omb2, eta, tau);
        });
    });
    if (!known) return set_err(FLAME_ENOTSUP, "%s: dtype %d not supported (f32, bf16, f16)", who, dtype);
    return launched(BR_CHAIN + dtype * 3 + variant, who);
}

int flame_fedopt_reduce_adapt_f64(int variant, unsigned flags, const flame_segment* segs, int32_t n_segs,
                                  int64_t n_chunks, const void* const* clients, int32_t n_clients,
                                  const double* rates64, double b1, double omb1, double b2, double omb2, double eta,
                                  double tau, void* stream) {
    const char* const who = "flame_fedopt_reduce_adapt_f64";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (n_clients > 0 && !rates64) return set_err(FLAME_EINVAL, "rate array is NULL");
    if (int rc = check_variant(who, variant)) return rc;
    if (int rc = check_flags(who, flags, kOptFlags)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    auto cl = reinterpret_cast<const uint64_t*>(clients);
    const Hyper64 h{b1, omb1, b2, omb2, eta, tau};
    dispatch_variant(variant, [&](auto vr) {
        hipLaunchKernelGGL((fedopt_kernel_f64<decltype(vr)::value, kClientUnroll>), grid, block, 0, st, segs, n_segs, cl,
                           n_clients, rates64, flags, h, n_chunks);
    });
    return launched(BR_OPT_F64 + variant, who);
}

int flame_fedopt_chain_f64(int variant, unsigned flags, const flame_segment* segs, int32_t n_segs, int64_t n_chunks,
                           const void* const* clients, int32_t n_clients, const double* rates64,
                           const uint8_t* step_end, double b1, double omb1, double b2, double omb2, double eta,
                           double tau, void* stream) {
    const char* const who = "flame_fedopt_chain_f64";
    if (int rc = validate(segs, n_segs, n_chunks, n_clients, clients)) return rc;
    if (n_clients < 1 || !rates64 || !step_end)
        return set_err(FLAME_EINVAL, "%s: needs >= 1 client, a rate array and a step_end array", who);
    if (int rc = check_variant(who, variant)) return rc;
    if (int rc = check_flags(who, flags, FLAME_OPT_STATE_ZERO)) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    auto cl = reinterpret_cast<const uint64_t*>(clients);
    const Hyper64 h{b1, omb1, b2, omb2, eta, tau};
    dispatch_variant(variant, [&](auto vr) {
        hipLaunchKernelGGL((fedopt_chain_kernel_f64<decltype(vr)::value, kClientUnroll>), grid, block, 0, st, segs, n_segs,
                           cl, n_clients, rates64, step_end, flags, h);
    });
    return launched(BR_CHAIN_F64 + variant, who);
}

int flame_fedopt_reduce_adapt_argmeta(int dtype, int variant, unsigned flags, const void* host_meta,
                                      int64_t meta_bytes, int32_t n_segs, int64_t n_chunks, int32_t n_clients,
                                      int64_t off_clients, int64_t off_r32, float b1, float omb1, float b2,
                                      float omb2, float eta, float tau, void* stream) {
    const char* const who = "flame_fedopt_reduce_adapt_argmeta";
    ArgMeta m;
    if (int rc = load_argmeta(who, host_meta, meta_bytes, m)) return rc;
    if (n_segs <= 0 || n_clients < 0) return set_err(FLAME_EINVAL, "%s: n_segs <= 0 or n_clients < 0", who);
    if (int rc = check_chunks(n_chunks)) return rc;
    if (int rc = check_flags(who, flags, kOptFlags)) return rc;
    if (int rc = check_variant(who, variant)) return rc;
    if (static_cast<int64_t>(n_segs) * static_cast<int64_t>(sizeof(flame_segment)) > meta_bytes ||
        !inside(meta_bytes, off_clients, static_cast<int64_t>(n_segs) * n_clients * 8) ||
        (n_clients > 0 && !inside(meta_bytes, off_r32, static_cast<int64_t>(n_clients) * 4)))
        return set_err(FLAME_EINVAL, "%s: a table lies outside the metadata block", who);
    const OptArgMeta src{&m, static_cast<int>(off_clients / 8), n_clients > 0 ? static_cast<int>(off_r32 / 8) : -1};
    return launch_opt(who, dtype, variant, flags, src, n_segs, n_clients, n_chunks, Hyper32{b1, omb1, b2, omb2, eta, tau},
                      stream);
}

int flame_fedbuff_scale_add(int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks, int64_t goal,
                            void* stream) {
    if (int rc = validate(segs, n_segs, n_chunks, 0, nullptr)) return rc;
    if (goal == 0) return set_err(FLAME_EINVAL, "agg_goal must be nonzero");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kEwBlock);
    const float gf = static_cast<float>(goal);
    const double gd = static_cast<double>(goal);
    const bool known = dispatch<FLAME_F32, FLAME_F64, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((scale_add_kernel<decltype(dt)::value>), grid, block, 0, st, segs, n_segs, gf, gd);
    });
    if (!known)
        return set_err(FLAME_ENOTSUP, "flame_fedbuff_scale_add: dtype %d not supported (integer tensors raise in the reference)", dtype);
    return launched(BR_SA + dtype, "flame_fedbuff_scale_add");
}

int flame_hier_fedbuff(int dtype, unsigned flags, const flame_hier_segment* segs, int32_t n_segs, int64_t n_chunks,
                       int32_t n_mids, int32_t n_clients, const void* const* mid_w, const void* const* mid_delta,
                       const void* const* clients, const float* mid_rates, const float* mid_goal,
                       const float* top_rates, float top_goal, void* stream) {
    const char* const who = "flame_hier_fedbuff";
    if (!segs || n_segs <= 0) return set_err(FLAME_EINVAL, "segment table is NULL or n_segs <= 0");
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_mids < 1 || n_clients < 1) return set_err(FLAME_EINVAL, "%s: need >= 1 middle and >= 1 arrival per middle", who);
    if (!mid_w || !clients || !mid_rates || !mid_goal || !top_rates) return set_err(FLAME_EINVAL, "%s: NULL table", who);
    if (int rc = check_hier_flags(who, flags, top_goal)) return rc;
    const HierTables src{segs, reinterpret_cast<const uint64_t*>(mid_w), reinterpret_cast<const uint64_t*>(mid_delta),
                         reinterpret_cast<const uint64_t*>(clients), mid_rates, mid_goal, top_rates};
    return launch_hier(who, dtype, flags, src, n_segs, n_chunks, n_mids, n_clients, top_goal, stream);
}

int flame_hier_fedbuff_argmeta(int dtype, unsigned flags, const void* host_meta, int64_t meta_bytes, int32_t n_segs,
                               int64_t n_chunks, int32_t n_mids, int32_t n_clients, int64_t off_mid_w,
                               int64_t off_mid_delta, int64_t off_clients, int64_t off_mid_rates,
                               int64_t off_mid_goal, int64_t off_top_rates, float top_goal, void* stream) {
    const char* const who = "flame_hier_fedbuff_argmeta";
    ArgMeta m;
    if (int rc = load_argmeta(who, host_meta, meta_bytes, m)) return rc;
    if (n_segs <= 0) return set_err(FLAME_EINVAL, "segment table is empty");
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_mids < 1 || n_clients < 1) return set_err(FLAME_EINVAL, "%s: need >= 1 middle and >= 1 arrival per middle", who);
    if (int rc = check_hier_flags(who, flags, top_goal)) return rc;
    const int64_t S = n_segs, M = n_mids, C = n_clients;
    if (S * static_cast<int64_t>(sizeof(flame_hier_segment)) > meta_bytes || !inside(meta_bytes, off_mid_w, S * M * 8) ||
        (off_mid_delta >= 0 && !inside(meta_bytes, off_mid_delta, S * M * 8)) ||
        !inside(meta_bytes, off_clients, S * M * C * 8) || !inside(meta_bytes, off_mid_rates, M * C * 4) ||
        !inside(meta_bytes, off_mid_goal, M * 4) || !inside(meta_bytes, off_top_rates, M * 4))
        return set_err(FLAME_EINVAL, "%s: a table lies outside the metadata block", who);
    const HierArgMeta src{&m, static_cast<int>(off_mid_w / 8), off_mid_delta >= 0 ? static_cast<int>(off_mid_delta / 8) : -1,
                          static_cast<int>(off_clients / 8), static_cast<int>(off_mid_rates / 8),
                          static_cast<int>(off_mid_goal / 8), static_cast<int>(off_top_rates / 8)};
    return launch_hier(who, dtype, flags, src, n_segs, n_chunks, n_mids, n_clients, top_goal, stream);
}

int flame_hier_resident_per_cu(int dtype, unsigned flags, int32_t n_mids) {
    if (n_mids < 1) return -set_err(FLAME_EINVAL, "flame_hier_resident_per_cu: n_mids < 1");
    // the one-middle low-residency launch aside, which depends on the launch size
    HierPick p = pick_hier(flags, n_mids, 0, 0);
    p.lo = false;
    const void* f = nullptr;
    const bool known = dispatch_hier(dtype, p, [&](auto inst) {
        using I = decltype(inst);
        f = reinterpret_cast<const void*>(hier_fedbuff_kernel<I::DT, I::CU, I::SYNC, I::HB, I::HL>);
    });
    if (!known)
        return -set_err(FLAME_ENOTSUP, "flame_hier_resident_per_cu: dtype %d not supported (f32, bf16, f16)", dtype);
    int blocks = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, f, kBlock, 0);
    if (e != hipSuccess) return -set_err(FLAME_EHIP, "hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e));
    return blocks < 1 ? 1 : blocks;
}

int flame_feddyn_round(int dtype, const flame_dyn_segment* segs, int32_t n_segs, int64_t n_chunks,
                       const void* const* steps, const uint32_t* step_flags, int32_t n_steps, int32_t n_phase1,
                       double rate_avg, double rate_mean, void* stream) {
    if (!segs || n_segs <= 0) return set_err(FLAME_EINVAL, "segment table is NULL or n_segs <= 0");
    if (int rc = check_chunks(n_chunks)) return rc;
    if (n_steps < 1 || !steps) return set_err(FLAME_EINVAL, "flame_feddyn_round: empty step program");
    if (n_steps > 0 && !step_flags) return set_err(FLAME_EINVAL, "flame_feddyn_round: step flag array is NULL");
    if (n_phase1 < 0 || n_phase1 > n_steps)
        return set_err(FLAME_EINVAL, "flame_feddyn_round: n_phase1 %d outside [0, %d]", n_phase1, n_steps);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    auto sp = reinterpret_cast<const uint64_t*>(steps);
    // torch rounds the Python-float rates to the tensor's opmath type: fp32, fp64 for f64 tensors
    const float ra32 = static_cast<float>(rate_avg), rm32 = static_cast<float>(rate_mean);
    const bool known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((feddyn_kernel<decltype(dt)::value, kDynUnroll>), grid, block, 0, st, segs, n_segs, sp, step_flags,
                           n_steps, n_phase1, ra32, rm32, rate_avg, rate_mean);
    });
    if (!known) return set_err(FLAME_ENOTSUP, "flame_feddyn_round: dtype %d not supported (f32, bf16, f16, f64)", dtype);
    return launched(BR_DYN + dtype, "flame_feddyn_round");
}

int flame_host_register(void* host, uint64_t nbytes) {
    if (!host || nbytes == 0) return set_err(FLAME_EINVAL, "flame_host_register: empty range");
    hipError_t e = hipHostRegister(host, static_cast<size_t>(nbytes), hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) return set_err(FLAME_EHIP, "hipHostRegister: %s", hipGetErrorString(e));
    return FLAME_OK;
}

int flame_host_unregister(void* host) {
    if (!host) return set_err(FLAME_EINVAL, "flame_host_unregister: NULL");
    hipError_t e = hipHostUnregister(host);
    if (e != hipSuccess) return set_err(FLAME_EHIP, "hipHostUnregister: %s", hipGetErrorString(e));
    return FLAME_OK;
}

int flame_host_device_pointer(void* host, void** device) {
    if (!host || !device) return set_err(FLAME_EINVAL, "flame_host_device_pointer: NULL");
    hipError_t e = hipHostGetDevicePointer(device, host, 0);
    if (e != hipSuccess) return set_err(FLAME_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    return FLAME_OK;
}

int flame_synth_fill(int dtype, void* out, int64_t numel, uint64_t seed, uint64_t stream_id, int64_t start,
                     float scale, void* stream) {
    if (numel < 0 || (numel > 0 && !out)) return set_err(FLAME_EINVAL, "flame_synth_fill: bad buffer");
    if (numel == 0) return FLAME_OK;
    const uint64_t ck = mix64((seed * 0x9E3779B97F4A7C15ull) ^ ((stream_id + 1ull) * 0xD1B54A32D192ED03ull));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t blocks = (numel + kEwBlock - 1) / kEwBlock;
    if (blocks > 8192) blocks = 8192;
    const dim3 grid(static_cast<unsigned>(blocks)), block(kEwBlock);
    const bool known = dispatch<FLAME_F32, FLAME_BF16, FLAME_F16>(dtype, [&](auto dt) {
        hipLaunchKernelGGL(synth_kernel<decltype(dt)::value>, grid, block, 0, st, out, numel, ck, start, scale);
    });
    if (!known) return set_err(FLAME_ENOTSUP, "flame_synth_fill: dtype %d not supported", dtype);
    return check_launch("flame_synth_fill");
}

// Outside the launch-branch table, as flame_update_stats and flame_synth_fill are: one instantiation
// per dtype, nothing to pick.
int flame_noise_fill(int dtype, const flame_segment* segs, int32_t n_segs, int64_t n_chunks, const uint32_t* streams,
                     const int64_t* starts, uint64_t seed, uint32_t round, double std, void* stream) {
    const char* const who = "flame_noise_fill";
    if (int rc = need_segs(who, segs, n_segs)) return rc;
    if (n_chunks <= 0 || n_chunks > 0x7FFFFFFFll)
        return set_err(FLAME_EINVAL, "%s: n_chunks out of range: %lld", who, (long long)n_chunks);
    if (dtype == FLAME_I64 || dtype == FLAME_I32)
        return set_err(FLAME_ENOTSUP, "%s: float dtypes only (integer and bool tensors get no noise), got dtype %d", who, dtype);
    if (dtype != FLAME_F32 && dtype != FLAME_BF16 && dtype != FLAME_F16 && dtype != FLAME_F64)
        return set_err(FLAME_ENOTSUP, "%s: unknown dtype %d", who, dtype);
    if (!(std >= 0.0) || std > 1.7976931348623157e308)
        return set_err(FLAME_EINVAL, "%s: std must be a finite number >= 0, got %g", who, std);
    if (dtype != FLAME_F64 && std >= 0x1.ffffffp127)       // FLT_MAX + half an ulp: rounds to an infinite fp32
        return set_err(FLAME_EINVAL, "%s: std %g rounds to an infinite fp32", who, std);
    if (!streams || !starts) return set_err(FLAME_EINVAL, "%s: the streams / starts array is NULL", who);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    const float std32 = dtype == FLAME_F64 ? 0.f : static_cast<float>(std);
    dispatch<FLAME_F32, FLAME_BF16, FLAME_F16, FLAME_F64>(dtype, [&](auto dt) {
        hipLaunchKernelGGL((noise_fill_kernel<decltype(dt)::value>), grid, block, 0, st, segs, n_segs, streams, starts, k0,
                           k1, round, std32, std);
    });
    return check_launch(who);
}

static int ew_check(const flame_ew_op* prog, int32_t n_ops, void* const* bufs, int32_t n_bufs, int64_t numel);

int flame_elementwise(const flame_ew_op* prog, int32_t n_ops, void* const* bufs, int32_t n_bufs, int64_t numel,
                      void* stream) {
    if (n_bufs < 0 || n_bufs > FLAME_EW_MAX_BUFS || (n_bufs > 0 && !bufs))
        return set_err(FLAME_EINVAL, "flame_elementwise: n_bufs %d outside [0, %d] or NULL table", n_bufs, FLAME_EW_MAX_BUFS);
    const int rc = ew_check(prog, n_ops, bufs, n_bufs, numel);
    if (rc != FLAME_OK) return rc;
    if (numel == 0 || n_ops == 0) return FLAME_OK;
    EwArgs a{};
    for (int32_t k = 0; k < n_ops; ++k) a.ops[k] = prog[k];
    for (int32_t k = 0; k < n_bufs; ++k) a.bufs[k] = bufs[k];
    a.numel = numel;
    a.n_ops = n_ops;
    int64_t blocks = (numel + kEwBlock - 1) / kEwBlock;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(ew_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kEwBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return launched(BR_EW, "flame_elementwise");
}

int flame_elementwise_segments(const flame_ew_op* prog, int32_t n_ops, void* const* table, int32_t n_bufs,
                               const int64_t* seg_end, int32_t n_segs, int64_t numel, void* stream) {
    if (n_bufs < 0 || n_bufs > FLAME_EW_MAX_BUFS)
        return set_err(FLAME_EINVAL, "flame_elementwise_segments: n_bufs %d outside [0, %d]", n_bufs, FLAME_EW_MAX_BUFS);
    if (n_segs <= 0 || !table || !seg_end)
        return set_err(FLAME_EINVAL, "flame_elementwise_segments: n_segs <= 0 or a NULL table");
    const int rc = ew_check(prog, n_ops, nullptr, n_bufs, numel);      // the buffers live on the device
    if (rc != FLAME_OK) return rc;
    if (numel == 0 || n_ops == 0) return FLAME_OK;
    EwArgs a{};
    for (int32_t k = 0; k < n_ops; ++k) a.ops[k] = prog[k];
    a.table = table;
    a.seg_end = seg_end;
    a.numel = numel;
    a.n_ops = n_ops;
    a.n_segs = n_segs;
    a.n_bufs = n_bufs;
    int64_t blocks = (numel + kEwBlock - 1) / kEwBlock;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(ew_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kEwBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return launched(BR_EW_SEG, "flame_elementwise_segments");
}

// the host-side check of a program (both entry points): every register defined before it is read,
// in the dtype the reading op says; every buffer it names present (bufs NULL: the segments'
// buffers are on the device, only the index is checked); an op / dtype the kernel knows
static int ew_check(const flame_ew_op* prog, int32_t n_ops, void* const* bufs, int32_t n_bufs, int64_t numel) {
    if (n_ops < 0 || n_ops > FLAME_EW_MAX_OPS || (n_ops > 0 && !prog))
        return set_err(FLAME_EINVAL, "flame_elementwise: n_ops %d outside [0, %d] or NULL program", n_ops, FLAME_EW_MAX_OPS);
    if (numel < 0) return set_err(FLAME_EINVAL, "flame_elementwise: numel < 0");
    // host-side check of the program: every register defined before it is read, in the dtype the
    // reading op says; every buffer it names present; an op / dtype the kernel knows
    int rdt[FLAME_EW_MAX_REGS];
    for (int k = 0; k < FLAME_EW_MAX_REGS; ++k) rdt[k] = -1;
    auto reg = [](int x) { return x >= 0 && x < FLAME_EW_MAX_REGS; };
    for (int32_t k = 0; k < n_ops; ++k) {
        const flame_ew_op& o = prog[k];
        const int dt = o.dtype;
        if (dt < FLAME_F32 || dt > FLAME_BOOL) return set_err(FLAME_EINVAL, "flame_elementwise: op %d: dtype %d", k, dt);
        auto bad = [&](const char* why) { return set_err(FLAME_EINVAL, "flame_elementwise: op %d (%d): %s", k, o.op, why); };
        switch (o.op) {
        case FLAME_EW_LOAD:
            if (!reg(o.dst) || o.a < 0 || o.a >= n_bufs || (bufs && numel > 0 && !bufs[o.a])) return bad("bad register or buffer");
            rdt[o.dst] = dt;
            break;
        case FLAME_EW_STORE:
            if (!reg(o.b) || o.a < 0 || o.a >= n_bufs || (bufs && numel > 0 && !bufs[o.a])) return bad("bad register or buffer");
            if (rdt[o.b] != dt) return bad("stored register is not of the buffer's dtype");
            break;
        case FLAME_EW_ZERO:
            if (!reg(o.dst)) return bad("bad register");
            rdt[o.dst] = dt;
            break;
        case FLAME_EW_CAST:
            if (!reg(o.dst) || !reg(o.a) || rdt[o.a] < 0 || rdt[o.a] != o.b) return bad("source register undefined or not of dtype b");
            rdt[o.dst] = dt;
            break;
        case FLAME_EW_ADD: case FLAME_EW_SUB: case FLAME_EW_MUL: case FLAME_EW_DIV:
            if (!reg(o.dst) || !reg(o.a) || !reg(o.b) || rdt[o.a] != dt || rdt[o.b] != dt) return bad("operand not of the op's dtype");
            if (o.op == FLAME_EW_DIV && !ew_float(dt)) return bad("division in an integer dtype");
            // bool: torch's + is a logical or, * a logical and (the sum / product != 0); - raises
            if (dt == FLAME_BOOL && o.op == FLAME_EW_SUB) return bad("subtraction in bool");
            rdt[o.dst] = dt;
            break;
        case FLAME_EW_ADD_S: case FLAME_EW_MUL_S: case FLAME_EW_SQUARE: case FLAME_EW_SIGN: case FLAME_EW_SQRT:
            if (!reg(o.dst) || !reg(o.a) || rdt[o.a] != dt) return bad("operand not of the op's dtype");
            if (o.op == FLAME_EW_SQRT && !ew_float(dt)) return bad("sqrt in an integer dtype");
            if (dt == FLAME_BOOL && (o.op == FLAME_EW_ADD_S || o.op == FLAME_EW_MUL_S))
                return bad("a scalar op in bool");
            rdt[o.dst] = dt;
            break;
        default: return bad("unknown op");
        }
    }
    return FLAME_OK;
}

static int check_tile_copies(const flame_tile_copy* t, int32_t n, const char* who) {
    if (n < 0 || (n > 0 && !t)) return set_err(FLAME_EINVAL, "%s: NULL table or n_entries < 0", who);
    for (int32_t i = 0; i < n; ++i) {
        if (t[i].nbytes < 0) return set_err(FLAME_EINVAL, "%s: entry %d: nbytes < 0", who, i);
        if (t[i].nbytes == 0) continue;
        if (!t[i].src || !t[i].dst) return set_err(FLAME_EINVAL, "%s: entry %d: NULL pointer", who, i);
        if (reinterpret_cast<uintptr_t>(t[i].dst) % 16)
            return set_err(FLAME_EINVAL, "%s: entry %d: dst not 16-byte aligned", who, i);
        if (t[i].nbytes > FLAME_TILE_BYTES && (t[i].dst_tile_stride < FLAME_TILE_BYTES || t[i].dst_tile_stride % 16))
            return set_err(FLAME_EINVAL, "%s: entry %d: dst_tile_stride %lld must be >= %d and a multiple of 16", who,
                           i, static_cast<long long>(t[i].dst_tile_stride), FLAME_TILE_BYTES);
    }
    return FLAME_OK;
}

int flame_slab_write(const flame_tile_copy* table, int32_t n_entries, void* stream) {
    int rc = check_tile_copies(table, n_entries, "flame_slab_write");
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    g_err[0] = 0;
    int32_t i = 0;
    while (i < n_entries) {           // up to kSlabMaxEntries keys per launch (one launch for most models)
        ArgMeta m;
        SlabEntry* ents = reinterpret_cast<SlabEntry*>(m.w);
        int n = 0;
        int64_t tiles = 0;
        for (; i < n_entries && n < kSlabMaxEntries; ++i) {
            if (table[i].nbytes == 0) continue;
            ents[n] = SlabEntry{static_cast<const uint8_t*>(table[i].src), static_cast<uint8_t*>(table[i].dst),
                                table[i].nbytes, table[i].dst_tile_stride, tiles};
            tiles += (table[i].nbytes + FLAME_TILE_BYTES - 1) / FLAME_TILE_BYTES;
            ++n;
        }
        if (n == 0) break;
        const int64_t blocks = (tiles + kSlabTPW - 1) / kSlabTPW;
        if (blocks > 0x7FFFFFFFll) return set_err(FLAME_EINVAL, "flame_slab_write: %lld tiles", (long long)tiles);
        hipLaunchKernelGGL(slab_write_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, m, n, tiles);
        rc = check_launch("flame_slab_write");
        if (rc) return rc;
    }
    return FLAME_OK;
}

int flame_slab_write_2d(const flame_tile_copy* table, int32_t n_entries, void* stream) {
    int rc = check_tile_copies(table, n_entries, "flame_slab_write_2d");
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int32_t i = 0; i < n_entries; ++i) {
        const flame_tile_copy& t = table[i];
        if (t.nbytes == 0) continue;
        const int64_t full = t.nbytes / FLAME_TILE_BYTES, rem = t.nbytes % FLAME_TILE_BYTES;
        hipError_t e = hipSuccess;
        if (full)
            e = hipMemcpy2DAsync(t.dst, static_cast<size_t>(t.dst_tile_stride), t.src, FLAME_TILE_BYTES,
                                 FLAME_TILE_BYTES, static_cast<size_t>(full), hipMemcpyDefault, st);
        if (e == hipSuccess && rem)
            e = hipMemcpyAsync(static_cast<uint8_t*>(t.dst) + full * t.dst_tile_stride,
                               static_cast<const uint8_t*>(t.src) + full * FLAME_TILE_BYTES, static_cast<size_t>(rem),
                               hipMemcpyDefault, st);
        if (e != hipSuccess) return set_err(FLAME_EHIP, "flame_slab_write_2d: entry %d: %s", i, hipGetErrorString(e));
    }
    g_err[0] = 0;
    return FLAME_OK;
}

int32_t flame_launch_branches(void) { return BR_COUNT; }

const char* flame_launch_branch_name(int32_t branch) { return branch_name(branch); }

int64_t flame_launch_branch_count(int32_t branch) {
    if (branch < 0 || branch >= BR_COUNT) return -1;
    return g_launches[branch].load(std::memory_order_relaxed);
}

}  // extern "C"
