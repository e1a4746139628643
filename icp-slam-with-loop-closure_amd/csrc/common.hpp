// common.hpp — shared helpers of the slamhip C-ABI (error state, launch checks).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "slamhip.h"

// Timing-only ablation switches remove work from the ICP kernel and give
// WRONG results (DESIGN.md section 3.1 cycle budget).  A product build refuses
// them: only a build that also defines SLAM_TIMING_ONLY (tools/ab_build.sh
// A/B libraries under ab/, never the in-tree libslamhip.so) may set them.
#if !defined(SLAM_TIMING_ONLY) && (defined(SLAM_ABL_SUMS) || defined(SLAM_ABL_GROUP) || defined(SLAM_ABL_CERT) || \
                                   defined(SLAM_ABL_STAGE2X) || defined(SLAM_NO_WINX) || defined(SLAM_KABSCH_ALL))
#error "SLAM_ABL_* / SLAM_NO_WINX / SLAM_KABSCH_ALL are timing-only ablations: define SLAM_TIMING_ONLY as well (A/B builds only)"
#endif
#if defined(SLAM_TIMING_ONLY) && defined(SLAMHIP_PRODUCT_BUILD)
#error "SLAM_TIMING_ONLY in a product build"
#endif

namespace slamhip {

// Thread-local message of the last failing call (slam_last_error()).
inline char* last_error_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int ok() {
    last_error_buf()[0] = 0;
    return SLAM_OK;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SLAM_EHIP, "%s: %s", what, hipGetErrorString(e));
    return ok();
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// 3x3 SE(2) matrix with the last row implicit [0, 0, 1].
struct SE2 {
    double m00, m01, m02, m10, m11, m12;
};

__device__ __forceinline__ SE2 load_se2(const double* p) {
    SE2 t;
    t.m00 = p[0]; t.m01 = p[1]; t.m02 = p[2];
    t.m10 = p[3]; t.m11 = p[4]; t.m12 = p[5];
    return t;
}

__device__ __forceinline__ void store_se2(double* p, const SE2& t) {
    p[0] = t.m00; p[1] = t.m01; p[2] = t.m02;
    p[3] = t.m10; p[4] = t.m11; p[5] = t.m12;
    // the constant row from registers set here: as a hoisted constant the
    // zero pair was the ICP kernel's only VGPR spill
    double z = 0.0, one = 1.0;
    asm volatile("" : "+v"(z), "+v"(one));
    p[6] = z;     p[7] = z;     p[8] = one;
}

// A @ B for SE(2) matrices with NumPy/OpenBLAS dgemm rounding: every entry is
// the k = 0, 1, 2 FMA chain fma(a2, b2, fma(a1, b1, a0 * b0)) (verified bit
// for bit against numpy 2.2 / OpenBLAS 0.3.29 in the build container).  With
// B's last row [0, 0, 1] the k = 2 term is +0 (columns 0, 1) or a2 (column 2).
__device__ __forceinline__ SE2 se2_mul(const SE2& a, const SE2& b) {
    SE2 c;
    c.m00 = fma(a.m02, 0.0, fma(a.m01, b.m10, a.m00 * b.m00));
    c.m01 = fma(a.m02, 0.0, fma(a.m01, b.m11, a.m00 * b.m01));
    c.m02 = fma(a.m02, 1.0, fma(a.m01, b.m12, a.m00 * b.m02));
    c.m10 = fma(a.m12, 0.0, fma(a.m11, b.m10, a.m10 * b.m00));
    c.m11 = fma(a.m12, 0.0, fma(a.m11, b.m11, a.m10 * b.m01));
    c.m12 = fma(a.m12, 1.0, fma(a.m11, b.m12, a.m10 * b.m02));
    return c;
}

// A double moved between lanes of a 16-lane row by DPP (both halves).
template <int CTRL>
__device__ __forceinline__ double dpp_row(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(b & 0xffffffff), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// Lane `lane`'s double (lane wave-uniform) through SGPRs.
__device__ __forceinline__ double readlane_d(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(b & 0xffffffff), lane);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(b >> 32), lane);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// All-lane sum of a wave64 without LDS: pairs and quads by DPP quad_perm,
// quads of a 16-lane row by DPP row_ror 12 / 8 (lane 0 of each row then holds
// the row sum), the four rows combined as (r0+r1)+(r2+r3) by row swaps.  Lane 0
// holds the result (other lanes may differ in rounding; callers use lane 0).
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_row<0xB1>(v);    // xor 1
    v += dpp_row<0x4E>(v);    // xor 2
    v += dpp_row<0x12C>(v);   // row_ror 12
    v += dpp_row<0x128>(v);   // row_ror 8
    // rows: (r0 + r1) in rows 0-1, (r2 + r3) in rows 2-3 (gfx950 v_permlane16_swap),
    // then the halves (v_permlane32_swap): lane 0 holds (r0 + r1) + (r2 + r3)
    const long long b = __double_as_longlong(v);
    const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(b), static_cast<unsigned>(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(b >> 32), static_cast<unsigned>(b >> 32),
                                                     false, false);
    v = __longlong_as_double((static_cast<long long>(hi[0]) << 32) | lo[0]) +
        __longlong_as_double((static_cast<long long>(hi[1]) << 32) | lo[1]);
    const long long c = __double_as_longlong(v);
    const auto lo2 = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(c), static_cast<unsigned>(c), false, false);
    const auto hi2 = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(c >> 32), static_cast<unsigned>(c >> 32),
                                                      false, false);
    return __longlong_as_double((static_cast<long long>(hi2[0]) << 32) | lo2[0]) +
           __longlong_as_double((static_cast<long long>(hi2[1]) << 32) | lo2[1]);
}

// Deterministic block all-reduce of NV doubles; `red` is LDS scratch of
// WAVES * NV doubles.  Every thread returns identical bits (fixed wave order).
template <int NV, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    }
    __syncthreads();
    if constexpr (WAVES <= 8) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = red[k];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += red[w * NV + k];
            v[k] = s;
        }
    } else {
        // 16-wave workgroups: lane w reads wave w's partials and the wave sums
        // them with the DPP tree (fixed order; NV registers instead of WAVES*NV)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = lane < WAVES ? red[lane * NV + k] : 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = readlane_d(wave_sum(v[k]), 0);
    }
}

// ---------------------------------------------------------------------------
// Order-free sums.  A term x with |x| <= B (one of n terms) is split onto two
// fixed grids chosen from (B, n) alone: h1 = (x + M1) - M1 is x rounded to a
// multiple of u1 = ulp(M1) (exact: x + M1 stays inside M1's binade), the
// remainder r = x - h1 is exact, and h2 = (r + M2) - M2 rounds r to u2 =
// ulp(M2).  Every partial sum of h1 values (multiples of u1, bounded by
// 2^53 u1) and of h2 values is exact, so the two totals are the same bits for
// ANY summation order: any workgroup shape, query layout or split of a pair
// over workgroups.  The dropped remainder is <= u2 / 2 per term, ~2^-70 of n B
// (far below a naive fp64 sum's rounding).  Valid while n B < 2^900.
// ---------------------------------------------------------------------------
struct RsumGrid {
    double m1, m2;
};

__device__ __forceinline__ RsumGrid rsum_grid(double bound, int n) {
    int e;
    (void)frexp(fmin(fmax(bound, 0x1p-900), 0x1p+900) * static_cast<double>(n), &e);   // n B < 2^e
    e += 2;                                                                           // |x| <= 2^(e-2) / n
    const int lg = 32 - __clz(max(n - 1, 1));                                         // n <= 2^lg
    RsumGrid g;
    g.m1 = ldexp(1.5, e);
    g.m2 = ldexp(1.5, e - 53 + lg + 2);   // |r| <= 2^(e-53) <= 2^(e2-2) / n
    return g;
}

__device__ __forceinline__ void rsum_add(double x, const RsumGrid& g, double& s1, double& s2) {
#ifdef SLAM_ABL_SUMS
    s1 += x;   // ablation build (timing only): plain sums
    return;
#endif
    const double h1 = (x + g.m1) - g.m1;
    const double r = x - h1;
    const double h2 = (r + g.m2) - g.m2;
    s1 += h1;
    s2 += h2;
}

// v_permlane{16,32}_swap on doubles (both 32-bit halves): for a pair (a, b)
// a + b afterwards is a's sum over the two swapped lane sets in one half (rows)
// and b's in the other.
__device__ __forceinline__ void swap32_d(double& a, double& b) {
    const long long x = __double_as_longlong(a), y = __double_as_longlong(b);
    const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(x), static_cast<unsigned>(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(x >> 32), static_cast<unsigned>(y >> 32),
                                                     false, false);
    a = __longlong_as_double((static_cast<long long>(hi[0]) << 32) | lo[0]);
    b = __longlong_as_double((static_cast<long long>(hi[1]) << 32) | lo[1]);
}
__device__ __forceinline__ void swap16_d(double& a, double& b) {
    const long long x = __double_as_longlong(a), y = __double_as_longlong(b);
    const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(x), static_cast<unsigned>(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(x >> 32), static_cast<unsigned>(y >> 32),
                                                     false, false);
    a = __longlong_as_double((static_cast<long long>(hi[0]) << 32) | lo[0]);
    b = __longlong_as_double((static_cast<long long>(hi[1]) << 32) | lo[1]);
}

// Sum over the 16 lanes of each row; every lane of the row gets it.
__device__ __forceinline__ double row_sum_d(double v) {
    v += dpp_row<0xB1>(v);    // xor 1
    v += dpp_row<0x4E>(v);    // xor 2
    v += dpp_row<0x12C>(v);   // row_ror 12
    v += dpp_row<0x128>(v);   // row_ror 8
    return v;
}

// Block all-reduce of 16 per-thread values whose partial sums are all EXACT
// (rsum_add grids), so the reduction order is free and chosen for cost: a
// reduce-scatter over the wave halves and row pairs (permlane swaps: 16 -> 8
// -> 4 values per lane), row sums of the remaining 4, one LDS slot per value
// and wave, and lane q (< 16) of every wave sums value q over the waves.
// `slab` is LDS of WAVES * 16 doubles; one barrier.  Returns value q in lane
// q (readlane_d(ret, q) makes it uniform).
template <int WAVES>
__device__ __forceinline__ double block_sum_exact16(double (&v)[16], double* slab) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {   // lanes 0-31: v[2j] summed over l, l+32; lanes 32-63: v[2j+1]
        swap32_d(v[2 * j], v[2 * j + 1]);
        v[j] = v[2 * j] + v[2 * j + 1];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // row r holds v[4i + {0, 2, 1, 3}[r]] summed over l, l+16, l+32, l+48
        swap16_d(v[2 * i], v[2 * i + 1]);
        v[i] = v[2 * i] + v[2 * i + 1];
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int row = lane >> 4;
    const int q0 = ((row & 1) << 1) | (row >> 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double s = row_sum_d(v[i]);
        if ((lane & 15) == 0) slab[wave * 16 + 4 * i + q0] = s;
    }
    __syncthreads();
    double t = 0.0;
    if (lane < 16) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += slab[w * 16 + lane];
    }
    return t;
}

// The wave-level form of block_sum_exact16: the 16 values summed over this
// wave's 64 lanes (exact partial sums, so the order is free), value q returned
// in lane q < 16 — no LDS, no barrier.
__device__ __forceinline__ double wave_sum_exact16(double (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        swap32_d(v[2 * j], v[2 * j + 1]);
        v[j] = v[2 * j] + v[2 * j + 1];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        swap16_d(v[2 * i], v[2 * i + 1]);
        v[i] = v[2 * i] + v[2 * i + 1];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = row_sum_d(v[i]);   // row r, register i: value 4 i + q0(r)
    const int lane = threadIdx.x & 63;
    const int q = lane & 15, q0 = q & 3;
    const int src = 16 * (((q0 & 1) << 1) | (q0 >> 1));   // the row holding value q (q0 is an involution)
    const double t0 = __shfl(v[0], src, 64), t1 = __shfl(v[1], src, 64);
    const double t2 = __shfl(v[2], src, 64), t3 = __shfl(v[3], src, 64);
    const int i = q >> 2;
    return i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3;
}

// popcount(x) + acc in one instruction: left to itself the compiler counts every
// dword into a register of its own and adds them up as a tree (8 + 7
// instructions for a 32-byte descriptor instead of 8)
__device__ __forceinline__ uint32_t bcnt(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// A float's bits as an int of the same order (sign-magnitude -> two's
// complement, an involution; -0 < +0, no NaN inputs), and back.
__device__ __forceinline__ int f2ord(float f) {
    const int i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float ord2f(int o) { return __int_as_float(o ^ ((o >> 31) & 0x7fffffff)); }

// An int moved between lanes by DPP (bound_ctrl: an invalid source lane reads 0): the step of the integer
// reductions here and of wave_reduce_i (icp_kernels.hip).
#define SLAM_DPPI(v, ctrl) __builtin_amdgcn_mov_dpp((v), (ctrl), 0xF, 0xF, true)

// Signed maxima of 8 per-lane values over the wave's 64 lanes in ONE
// reduce-scatter (the integer form of wave_sum_exact16; max is exact, so the
// order is free): v_permlane32_swap on pairs (8 -> 4 registers: lanes 0-31
// hold the even value over l, l+32, lanes 32-63 the odd one), v_permlane16_swap
// (4 -> 2: row r of register i holds value 4 i + {0, 2, 1, 3}[r] over the four
// rows), 4 DPP steps within the rows of the two survivors, and one v_readlane
// per value: the results are wave-uniform (SGPRs).
__device__ __forceinline__ void wave_max8_i32(int (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const auto p = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(v[2 * j]),
                                                        static_cast<unsigned>(v[2 * j + 1]), false, false);
        v[j] = max(static_cast<int>(p[0]), static_cast<int>(p[1]));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const auto p = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(v[2 * i]),
                                                        static_cast<unsigned>(v[2 * i + 1]), false, false);
        v[i] = max(static_cast<int>(p[0]), static_cast<int>(p[1]));
    }
    int x0 = v[0], x1 = v[1];
    x0 = max(x0, SLAM_DPPI(x0, 0xB1));    // quad_perm [1,0,3,2]
    x1 = max(x1, SLAM_DPPI(x1, 0xB1));
    x0 = max(x0, SLAM_DPPI(x0, 0x4E));    // quad_perm [2,3,0,1]
    x1 = max(x1, SLAM_DPPI(x1, 0x4E));
    x0 = max(x0, SLAM_DPPI(x0, 0x124));   // row_ror:4
    x1 = max(x1, SLAM_DPPI(x1, 0x124));
    x0 = max(x0, SLAM_DPPI(x0, 0x128));   // row_ror:8
    x1 = max(x1, SLAM_DPPI(x1, 0x128));
    v[0] = __builtin_amdgcn_readlane(x0, 0);
    v[2] = __builtin_amdgcn_readlane(x0, 16);
    v[1] = __builtin_amdgcn_readlane(x0, 32);
    v[3] = __builtin_amdgcn_readlane(x0, 48);
    v[4] = __builtin_amdgcn_readlane(x1, 0);
    v[6] = __builtin_amdgcn_readlane(x1, 16);
    v[5] = __builtin_amdgcn_readlane(x1, 32);
    v[7] = __builtin_amdgcn_readlane(x1, 48);
}

// Bounds of a 64-query group's active lanes for the ICP group search: the box
// of their fp32 points, their largest M2 (non-negative or +inf: its bits order
// as they are) and the intersection [wlo, whi) of their windows [ws, ws +
// kwin).  All seven reduce as signed maxima of ordered 32-bit keys (the minima
// complemented) in one wave_max8_i32; an inactive lane contributes each key's
// identity (+-inf, 0, an empty intersection), so the results are the bits of
// seven separate min / max reductions.  Wave-uniform; the key mapping is undone
// on the scalar side.  At least one lane is active.
struct GroupBounds {
    float bx0, bx1, by0, by1, gM2;
    int wlo, whi;
};
__device__ __forceinline__ GroupBounds wave_group_bounds(bool act, float qx, float qy, float M2, int ws, int kwin) {
    const int ox = f2ord(qx), oy = f2ord(qy);
    constexpr int kLo = static_cast<int>(0x807fffffu);   // f2ord(-inf): below every finite key
    int v[8];
    v[0] = act ? ~ox : kLo;           // ~f2ord(x) is decreasing in x, ~f2ord(+inf) = f2ord(-inf)
    v[1] = act ? ox : kLo;
    v[2] = act ? ~oy : kLo;
    v[3] = act ? oy : kLo;
    v[4] = act ? __float_as_int(M2) : 0;
    v[5] = act ? ws : 0;
    v[6] = act ? 0xffff - (ws + kwin) : 0;
    v[7] = 0;
    wave_max8_i32(v);
    GroupBounds g;
    g.bx0 = ord2f(~v[0]);
    g.bx1 = ord2f(v[1]);
    g.by0 = ord2f(~v[2]);
    g.by1 = ord2f(v[3]);
    g.gM2 = __int_as_float(v[4]);
    g.wlo = v[5];
    g.whi = 0xffff - v[6];
    return g;
}

}  // namespace slamhip
