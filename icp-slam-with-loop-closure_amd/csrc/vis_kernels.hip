// vis_kernels.hip — per-edge verification of scan-pair transforms by visibility
// for gfx950 (MI355X).  include/slamhip.h states the rule; tests/vis_ref.py
// restates it.
//
// vis_tables_kernel: one 256-thread workgroup per scan.  The sector centres and
// the scan's table pass through LDS; a point's sector is the first maximum of
// (c_k x) + (s_k y) over the S centres (the plain S-step loop, every lane reading
// the same LDS address: a broadcast), and its r2 goes into the table with a
// 64-bit unsigned LDS atomic min on the bit pattern: non-negative doubles order
// as their bits do, so the minimum is exact and order-free.
//
// vis_check_kernel: one 256-thread workgroup per edge, both directions.  The two
// scans' tables are square-rooted once into LDS (IEEE sqrt is monotone: the
// minimum of the roots is the root of the minimum, and +inf stays +inf); a lane
// maps its point, finds its sector with the same loop and walks the 2W + 1
// entries around it.  The agreeing and conflicting points are counted by ballot
// and popcount per wave and added up as integers in a fixed order.  No
// floating-point atomics, no exchange between workgroups: the counts do not
// depend on the launch shape.  The status flags are plain stores of 1.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kVisBlock = 256;
constexpr int kVisWaves = kVisBlock / 64;
constexpr int kVisMaxS = 1024;
constexpr int kVisBadScan = 1, kVisBadEdge = 2;
constexpr unsigned long long kVisInfBits = 0x7ff0000000000000ull;

__device__ int g_vis_bad_scan;   // nonzero: a launch since slam_vis_status met a scan with bad offsets
__device__ int g_vis_bad_edge;   // nonzero: ... an edge that names a scan outside [0, n_scans) or one with bad offsets

// The first maximum of (c_k x) + (s_k y) over the S centres in LDS.  A NaN never exceeds the running best, so a
// point that is not finite gets sector 0.
__device__ __forceinline__ int vis_sector(const double2* dir, int S, double x, double y) {
    int best_k = 0;
    double best = (dir[0].x * x) + (dir[0].y * y);
#pragma unroll 4
    for (int k = 1; k < S; ++k) {
        const double2 d = dir[k];   // one address for the wave: a broadcast
        const double v = (d.x * x) + (d.y * y);
        const bool gt = v > best;   // the smallest k among equal maxima stays
        best = gt ? v : best;
        best_k = gt ? k : best_k;
    }
    return best_k;
}

__global__ __launch_bounds__(kVisBlock) void vis_tables_kernel(const double* __restrict__ pts,
                                                               const int64_t* __restrict__ scan_off, int64_t P,
                                                               const double* __restrict__ dirs, int32_t S,
                                                               double* __restrict__ out_r2) {
    __shared__ double2 dir[kVisMaxS];
    __shared__ unsigned long long tab[kVisMaxS];
    const int tid = threadIdx.x;
    const int64_t scan = blockIdx.x;
    for (int k = tid; k < S; k += kVisBlock) {
        dir[k] = make_double2(dirs[2 * k], dirs[2 * k + 1]);
        tab[k] = kVisInfBits;
    }
    int64_t p0 = scan_off[scan], p1 = scan_off[scan + 1];
    if (p0 < 0 || p1 < p0 || p1 > P) {   // uniform: nothing is read through bad offsets, the row stays +inf
        if (tid == 0) g_vis_bad_scan = 1;
        p1 = p0 = 0;
    }
    __syncthreads();
    const double2* Q = reinterpret_cast<const double2*>(pts);
    for (int64_t p = p0 + tid; p < p1; p += kVisBlock) {
        const double2 q = Q[p];
        const double r2 = (q.x * q.x) + (q.y * q.y);
        if (!(r2 < INFINITY)) continue;   // not finite (NaN included): no part
        const int k = vis_sector(dir, S, q.x, q.y);
        atomicMin(&tab[k], static_cast<unsigned long long>(__double_as_longlong(r2)));   // r2 >= +0: bits order as values
    }
    __syncthreads();
    for (int k = tid; k < S; k += kVisBlock)
        out_r2[scan * S + k] = __longlong_as_double(static_cast<long long>(tab[k]));
}

struct VisArgs {
    const double* pts;
    const int64_t* scan_off;
    const double* dirs;
    const double* tables;
    const int32_t* src;
    const int32_t* dst;
    const double* tf;
    int64_t P;
    int32_t n_scans, S, W;
    double margin;
    int32_t* out;
};

// One direction: the points [p0, p1) through M against the rooted table `root`.  `agree` and `conflict` are
// this WAVE's counts, the same in all its lanes.
__device__ __forceinline__ void vis_direction(const VisArgs& A, const double2* dir, const double* root, int64_t p0,
                                              int64_t p1, const SE2& M, int& agree, int& conflict) {
    const int S = A.S, W = A.W;
    const double2* Q = reinterpret_cast<const double2*>(A.pts);
    const int64_t n = p1 - p0;
    const int64_t rounds = (n + kVisBlock - 1) / kVisBlock;
    int na = 0, nc = 0;
    for (int64_t r = 0; r < rounds; ++r) {   // every lane of the wave takes every round: the ballots are whole
        const int64_t i = r * kVisBlock + threadIdx.x;
        bool ag = false, cf = false;
        if (i < n) {
            const double2 p = Q[p0 + i];
            const double qx = ((M.m00 * p.x) + (M.m01 * p.y)) + M.m02;
            const double qy = ((M.m10 * p.x) + (M.m11 * p.y)) + M.m12;
            const double rq = sqrt((qx * qx) + (qy * qy));
            const int k = vis_sector(dir, S, qx, qy);
            bool all_seen = true;
            double lo = INFINITY;
            int j = k - W;
            j += j < 0 ? S : 0;   // W < S: one wrap at most
            for (int w = -W; w <= W; ++w) {
                const double re = root[j];
                j = j + 1 == S ? 0 : j + 1;
                const bool seen = re < INFINITY;
                all_seen = all_seen && seen;
                ag = ag || (seen && fabs(re - rq) <= A.margin);
                lo = re < lo ? re : lo;
            }
            cf = !ag && all_seen && rq + A.margin < lo;
        }
        na += __popcll(__ballot(ag));
        nc += __popcll(__ballot(cf));
    }
    agree = na;
    conflict = nc;
}

__global__ __launch_bounds__(kVisBlock) void vis_check_kernel(const VisArgs A) {
    __shared__ double2 dir[kVisMaxS];
    __shared__ double root[2][kVisMaxS];   // [0]: the destination's table, [1]: the source's, square-rooted
    __shared__ int cnt[kVisWaves][4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int S = A.S;
    const int64_t si = A.src[b], di = A.dst[b];
    int64_t s0 = 0, s1 = 0, d0 = 0, d1 = 0;
    bool bad = si < 0 || si >= A.n_scans || di < 0 || di >= A.n_scans;
    if (!bad) {
        s0 = A.scan_off[si];
        s1 = A.scan_off[si + 1];
        d0 = A.scan_off[di];
        d1 = A.scan_off[di + 1];
        bad = s0 < 0 || s1 < s0 || s1 > A.P || d0 < 0 || d1 < d0 || d1 > A.P || s1 - s0 > 0x7fffffffll ||
              d1 - d0 > 0x7fffffffll;
    }
    if (bad) {   // uniform: the edge is not computed and nothing is read through its indices
        if (tid == 0) g_vis_bad_edge = 1;
        if (tid < 6) A.out[6 * b + tid] = -1;
        return;
    }
    for (int k = tid; k < S; k += kVisBlock) {
        dir[k] = make_double2(A.dirs[2 * k], A.dirs[2 * k + 1]);
        root[0][k] = sqrt(A.tables[di * S + k]);
        root[1][k] = sqrt(A.tables[si * S + k]);
    }
    __syncthreads();
    const SE2 T = load_se2(A.tf + 9 * b);
    SE2 R;   // the rigid inverse: the transposed rotation, -(R^T t)
    R.m00 = T.m00;
    R.m01 = T.m10;
    R.m10 = T.m01;
    R.m11 = T.m11;
    R.m02 = -((T.m00 * T.m02) + (T.m10 * T.m12));
    R.m12 = -((T.m01 * T.m02) + (T.m11 * T.m12));
    int a0, c0, a1, c1;
    vis_direction(A, dir, root[0], s0, s1, T, a0, c0);
    vis_direction(A, dir, root[1], d0, d1, R, a1, c1);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        cnt[wave][0] = a0;
        cnt[wave][1] = c0;
        cnt[wave][2] = a1;
        cnt[wave][3] = c1;
    }
    __syncthreads();
    if (tid < 4) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kVisWaves; ++w) s += cnt[w][tid];
        A.out[6 * b + (tid < 2 ? tid : tid + 1)] = s;   // agree0 conflict0 . agree1 conflict1 .
    }
    if (tid == 4) A.out[6 * b + 2] = static_cast<int32_t>(s1 - s0);
    if (tid == 5) A.out[6 * b + 5] = static_cast<int32_t>(d1 - d0);
}

static int vis_read_clear(int* total) {
    int a = 0, b = 0;
    if (hipMemcpyFromSymbol(&a, HIP_SYMBOL(g_vis_bad_scan), sizeof(int)) != hipSuccess ||
        hipMemcpyFromSymbol(&b, HIP_SYMBOL(g_vis_bad_edge), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "vis status: read");
    const int zero = 0;
    if (a && hipMemcpyToSymbol(HIP_SYMBOL(g_vis_bad_scan), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "vis status: clear");
    if (b && hipMemcpyToSymbol(HIP_SYMBOL(g_vis_bad_edge), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "vis status: clear");
    *total = (a ? kVisBadScan : 0) | (b ? kVisBadEdge : 0);
    return SLAM_OK;
}

static int vis_sectors_ok(const char* what, int32_t S) {
    if (S < 3 || S > kVisMaxS) return fail(SLAM_EINVAL, "%s: S = %d outside 3..%d", what, S, kVisMaxS);
    return SLAM_OK;
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_vis_tables_f64(const double* pts, const int64_t* scan_off, int32_t n_scans, int64_t P, const double* dirs,
                        int32_t S, double* out_r2, void* stream) {
    if (!pts || !scan_off || !dirs || !out_r2) return fail(SLAM_EINVAL, "vis tables: null array");
    if (n_scans < 0 || P < 0)
        return fail(SLAM_EINVAL, "vis tables: n_scans = %d, P = %lld: negative", n_scans, static_cast<long long>(P));
    if (const int rc = vis_sectors_ok("vis tables", S)) return rc;
    if (reinterpret_cast<uintptr_t>(pts) % 16) return fail(SLAM_EINVAL, "vis tables: points not 16-byte aligned");
    if (n_scans == 0) return ok();
    hipLaunchKernelGGL(vis_tables_kernel, dim3(static_cast<unsigned>(n_scans)), dim3(kVisBlock), 0, as_stream(stream),
                       pts, scan_off, P, dirs, S, out_r2);
    return check_launch("vis tables kernel");
}

int slam_vis_check_f64(const double* pts, const int64_t* scan_off, int32_t n_scans, int64_t P, const double* dirs,
                       int32_t S, const double* tables, const int32_t* src, const int32_t* dst, const double* tf,
                       int32_t B, double margin, int32_t W, int32_t* out_counts, void* stream) {
    if (!pts || !scan_off || !dirs || !tables || !src || !dst || !tf || !out_counts)
        return fail(SLAM_EINVAL, "vis check: null array");
    if (n_scans < 0 || P < 0 || B < 0)
        return fail(SLAM_EINVAL, "vis check: B = %d, n_scans = %d, P = %lld: negative", B, n_scans,
                    static_cast<long long>(P));
    if (const int rc = vis_sectors_ok("vis check", S)) return rc;
    if (W < 0 || W > (S - 1) / 2) return fail(SLAM_EINVAL, "vis check: W = %d: 0 <= W and 2 W + 1 <= S = %d expected", W, S);
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(SLAM_EINVAL, "vis check: a negative or non-finite margin");
    if (reinterpret_cast<uintptr_t>(pts) % 16) return fail(SLAM_EINVAL, "vis check: points not 16-byte aligned");
    if (B == 0) return ok();
    VisArgs A;
    A.pts = pts;
    A.scan_off = scan_off;
    A.dirs = dirs;
    A.tables = tables;
    A.src = src;
    A.dst = dst;
    A.tf = tf;
    A.P = P;
    A.n_scans = n_scans;
    A.S = S;
    A.W = W;
    A.margin = margin;
    A.out = out_counts;
    hipLaunchKernelGGL(vis_check_kernel, dim3(static_cast<unsigned>(B)), dim3(kVisBlock), 0, as_stream(stream), A);
    return check_launch("vis check kernel");
}

int slam_vis_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "vis status: stream sync");
    int st = 0;
    if (const int rc = vis_read_clear(&st)) return rc;
    if (st == 0) return ok();
    return fail(SLAM_EINVAL, "vis:%s%s", st & kVisBadScan ? " a scan's offsets descend or leave [0, P];" : "",
                st & kVisBadEdge ? " an edge names a scan outside [0, n_scans) or one with bad offsets (its counts "
                                   "are -1);"
                                 : "");
}

}  // extern "C"
