// plicp_kernels.hip — point-to-line refinement of ICP edges for gfx950 (MI355X).
// include/slamhip.h states the rule; tests/plicp_ref.py restates it.
//
// plicp_normals_kernel: one 256-thread workgroup per scan, one thread per point
// (a strided loop above 256 points), one launch for all scans.  A thread walks at
// most K neighbours to each side of its point; the reads stay in L1 / L2.  A scan
// with bad offsets writes nothing: the output is zeroed in front of the launch.
//
// plicp_pair_kernel<QPT>: one 256-thread workgroup per pair, every iteration on
// chip.  Lane t keeps the transformed queries t + 256 q, q < QPT, with their best
// squared distance and index in registers.  The destination scan streams through
// one fixed LDS tile of 2,048 double2 (32 KiB) in ascending order; every lane
// reads a candidate at the same address (an LDS broadcast) and keeps (best, j)
// under a strict <, so the first index wins a tie as in np.argmin.  No cap on
// the destination's size and no dynamic LDS.  The matched normal is one gather
// per inlier, the eleven sums (H, g, e and the inlier count) go through
// block_sum, whose result is the same bits in every thread: each thread solves
// the 3x3 system and updates its own copy of T, so T is never handed on.  No
// exchange between workgroups, no spin wait, no atomics: the status flags are
// plain stores of 1.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kPlBlock = 256;
constexpr int kPlWaves = kPlBlock / 64;
constexpr int kPlTile = 2048;          // destination points per LDS tile
constexpr int kPlMaxQuery = 8192;      // source points per pair at most: 32 per lane
constexpr int kPlSums = 11;            // H00 H01 H02 H11 H12 H22 g0 g1 g2 e m
constexpr int kPlBadScan = 1, kPlBadPair = 2;

__device__ int g_plicp_bad_scan;   // nonzero: a launch since slam_plicp_status met a scan with bad offsets
__device__ int g_plicp_bad_pair;   // nonzero: ... a pair outside its launch's bounds

__global__ __launch_bounds__(kPlBlock) void plicp_normals_kernel(const double* __restrict__ pts,
                                                                 const int64_t* __restrict__ scan_off, int64_t P,
                                                                 int32_t K, double rho2, double ctol,
                                                                 double* __restrict__ normals) {
    const int64_t p0 = scan_off[blockIdx.x], p1 = scan_off[blockIdx.x + 1];
    if (p0 < 0 || p1 < p0 || p1 > P) {   // uniform: nothing is read or written through bad offsets
        if (threadIdx.x == 0) g_plicp_bad_scan = 1;
        return;
    }
    const double2* Q = reinterpret_cast<const double2*>(pts) + p0;
    const int64_t n = p1 - p0;
    for (int64_t j = threadIdx.x; j < n; j += kPlBlock) {
        const double2 qj = Q[j];
        int64_t l = j, r = j;
        while (l > 0 && j - l < K) {
            const double2 c = Q[l - 1];
            const double dx = c.x - qj.x, dy = c.y - qj.y;
            if (!((dx * dx) + (dy * dy) <= rho2)) break;
            --l;
        }
        while (r < n - 1 && r - j < K) {
            const double2 c = Q[r + 1];
            const double dx = c.x - qj.x, dy = c.y - qj.y;
            if (!((dx * dx) + (dy * dy) <= rho2)) break;
            ++r;
        }
        double nx = 0.0, ny = 0.0;
        if (r - l >= 2) {
            const double2 ql = Q[l], qr = Q[r];
            const double tx = qr.x - ql.x, ty = qr.y - ql.y;
            const double L2 = (tx * tx) + (ty * ty);
            if (L2 > 0.0 && L2 < INFINITY) {
                const double L = sqrt(L2);
                const double ax = -ty / L, ay = tx / L;
                const double off = (ax * (qj.x - ql.x)) + (ay * (qj.y - ql.y));
                if (fabs(off) <= ctol) {
                    nx = ax;
                    ny = ay;
                }
            }
        }
        reinterpret_cast<double2*>(normals)[p0 + j] = make_double2(nx, ny);
    }
}

struct PlicpArgs {
    const double* pts;
    const int64_t* scan_off;
    const double* normals;
    const int32_t* src;
    const int32_t* dst;
    const double* init;
    int64_t P;
    int32_t S;
    int32_t min_inliers, max_iters, max_n1, match_stride;
    double max_dist2, eps_t, eps_r, pivot_tol;
    double* out_tf;
    double* out_err;
    double* out_obs;
    int32_t* out_inliers;
    int32_t* out_iters;
    int32_t* out_status;
    int32_t* out_match;
};

__device__ __forceinline__ void plicp_row(double (&s)[kPlSums], double a0, double a1, double a2, double r) {
    s[0] += a0 * a0;
    s[1] += a0 * a1;
    s[2] += a0 * a2;
    s[3] += a1 * a1;
    s[4] += a1 * a2;
    s[5] += a2 * a2;
    s[6] += a0 * r;
    s[7] += a1 * r;
    s[8] += a2 * r;
    s[9] += r * r;
}

__device__ __forceinline__ bool plicp_bad_pivot(double d, double hkk, double tol) {
    return !(fabs(d) < INFINITY) || d <= tol * hkk;   // not finite (NaN included) or too small
}

template <int QPT>
__global__ __launch_bounds__(kPlBlock) void plicp_pair_kernel(const PlicpArgs A) {
    __shared__ double2 tile[kPlTile];
    __shared__ double red[kPlWaves * kPlSums];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t si = A.src[b], di = A.dst[b];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    SE2 T = load_se2(A.init + 9 * b);
    int64_t s0 = 0, s1 = 0, d0 = 0, d1 = 0;
    bool bad = si < 0 || si >= A.S || di < 0 || di >= A.S;
    if (!bad) {
        s0 = A.scan_off[si];
        s1 = A.scan_off[si + 1];
        d0 = A.scan_off[di];
        d1 = A.scan_off[di + 1];
        bad = s0 < 0 || s1 < s0 || s1 > A.P || d0 < 0 || d1 < d0 || d1 > A.P || s1 - s0 > A.max_n1 ||
              s1 - s0 > static_cast<int64_t>(QPT) * kPlBlock || d1 - d0 > 0x7fffffffll ||
              (A.out_match && s1 - s0 > A.match_stride);
    }
    if (bad) {   // uniform: the pair is not computed and nothing is read through its indices
        if (tid == 0) {
            g_plicp_bad_pair = 1;
            store_se2(A.out_tf + 9 * b, T);
            A.out_err[b] = nan;
            A.out_obs[b] = nan;
            A.out_inliers[b] = 0;
            A.out_iters[b] = 0;
            A.out_status[b] = -1;
        }
        if (A.out_match)
            for (int i = tid; i < A.match_stride; i += kPlBlock) A.out_match[b * A.match_stride + i] = -1;
        return;
    }
    const int n1 = static_cast<int>(s1 - s0);
    const int n2 = static_cast<int>(d1 - d0);
    const double2* Ps = reinterpret_cast<const double2*>(A.pts) + s0;
    const double2* Qd = reinterpret_cast<const double2*>(A.pts) + d0;
    const double2* Nd = reinterpret_cast<const double2*>(A.normals) + d0;

    double xq[QPT], yq[QPT], best[QPT];
    int bj[QPT];
    int it = 0, status = 0, m = 0;
    double err = nan, obs = nan;
    for (;;) {
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const int i = q * kPlBlock + tid;
            xq[q] = nan;   // a slot past the scan: every distance is NaN and never below best
            yq[q] = nan;
            if (i < n1) {
                const double2 p = Ps[i];
                xq[q] = ((T.m00 * p.x) + (T.m01 * p.y)) + T.m02;
                yq[q] = ((T.m10 * p.x) + (T.m11 * p.y)) + T.m12;
            }
            best[q] = inf;
            bj[q] = 0;
        }
        for (int base = 0; base < n2; base += kPlTile) {
            const int cnt = min(kPlTile, n2 - base);
            __syncthreads();   // the previous tile (and the sums' scratch) is done with
            for (int k = tid; k < cnt; k += kPlBlock) tile[k] = Qd[base + k];
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {
                const double2 c = tile[k];   // one address for the wave: a broadcast
#pragma unroll
                for (int q = 0; q < QPT; ++q) {
                    const double dx = xq[q] - c.x, dy = yq[q] - c.y;
                    const double d = (dx * dx) + (dy * dy);
                    const bool lt = d < best[q];
                    best[q] = lt ? d : best[q];
                    bj[q] = lt ? base + k : bj[q];
                }
            }
        }
        double s[kPlSums];
#pragma unroll
        for (int k = 0; k < kPlSums; ++k) s[k] = 0.0;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const bool in = q * kPlBlock + tid < n1 && best[q] <= A.max_dist2;
            if (in) {
                const double2 c = Qd[bj[q]];
                const double2 nn = Nd[bj[q]];
                const double ex = xq[q] - c.x, ey = yq[q] - c.y;
                if (nn.x != 0.0 || nn.y != 0.0) {
                    plicp_row(s, nn.x, nn.y, (nn.y * xq[q]) - (nn.x * yq[q]), (nn.x * ex) + (nn.y * ey));
                } else {
                    plicp_row(s, 1.0, 0.0, -yq[q], ex);
                    plicp_row(s, 0.0, 1.0, xq[q], ey);
                }
                s[10] += 1.0;
            } else {
                bj[q] = -1;
            }
        }
        __syncthreads();   // every wave has left the tile loop: red is free
        block_sum<kPlSums, kPlWaves>(s, red);
        const double H00 = s[0], H01 = s[1], H02 = s[2], H11 = s[3], H12 = s[4], H22 = s[5];
        m = static_cast<int>(s[10]);
        err = s[9] / s[10];
        const double h = (H00 + H11) / 2.0;
        const double q2 = (h * h) - ((H00 * H11) - (H01 * H01));
        const double qq = sqrt(q2 > 0.0 ? q2 : 0.0);
        obs = (h - qq) / (h + qq);
        if (m < A.min_inliers) {
            status = 3;
            break;
        }
        status = 2;
        const double dd0 = H00;
        if (plicp_bad_pivot(dd0, H00, A.pivot_tol)) break;
        const double l10 = H01 / dd0, l20 = H02 / dd0;
        const double dd1 = H11 - (l10 * H01);
        if (plicp_bad_pivot(dd1, H11, A.pivot_tol)) break;
        const double u = H12 - (l20 * H01);
        const double l21 = u / dd1;
        const double dd2 = (H22 - (l20 * H02)) - (l21 * u);
        if (plicp_bad_pivot(dd2, H22, A.pivot_tol)) break;
        const double z0 = -s[6];
        const double z1 = -s[7] - (l10 * z0);
        const double z2 = (-s[8] - (l20 * z0)) - (l21 * z1);
        const double dth = z2 / dd2;
        const double dy = (z1 / dd1) - (l21 * dth);
        const double dx = ((z0 / dd0) - (l10 * dy)) - (l20 * dth);
        const double c = cos(dth), sn = sin(dth);
        SE2 Tn;
        Tn.m00 = (c * T.m00) - (sn * T.m10);
        Tn.m01 = (c * T.m01) - (sn * T.m11);
        Tn.m02 = ((c * T.m02) - (sn * T.m12)) + dx;
        Tn.m10 = (sn * T.m00) + (c * T.m10);
        Tn.m11 = (sn * T.m01) + (c * T.m11);
        Tn.m12 = ((sn * T.m02) + (c * T.m12)) + dy;
        T = Tn;
        ++it;
        if (fabs(dx) < A.eps_t && fabs(dy) < A.eps_t && fabs(dth) < A.eps_r) {
            status = 0;
            break;
        }
        if (it == A.max_iters) {
            status = 1;
            break;
        }
    }
    if (tid == 0) {
        store_se2(A.out_tf + 9 * b, T);
        A.out_err[b] = err;
        A.out_obs[b] = obs;
        A.out_inliers[b] = m;
        A.out_iters[b] = it;
        A.out_status[b] = status;
    }
    if (A.out_match) {
        int32_t* row = A.out_match + b * A.match_stride;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const int i = q * kPlBlock + tid;
            if (i < n1) row[i] = bj[q];
        }
        for (int i = n1 + tid; i < A.match_stride; i += kPlBlock) row[i] = -1;
    }
}

static bool plicp_tol_ok(double v) { return v >= 0.0 && std::isfinite(v); }

static int plicp_read_clear(int* total) {
    int a = 0, b = 0;
    if (hipMemcpyFromSymbol(&a, HIP_SYMBOL(g_plicp_bad_scan), sizeof(int)) != hipSuccess ||
        hipMemcpyFromSymbol(&b, HIP_SYMBOL(g_plicp_bad_pair), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "plicp status: read");
    const int zero = 0;
    if (a && hipMemcpyToSymbol(HIP_SYMBOL(g_plicp_bad_scan), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "plicp status: clear");
    if (b && hipMemcpyToSymbol(HIP_SYMBOL(g_plicp_bad_pair), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "plicp status: clear");
    *total = (a ? kPlBadScan : 0) | (b ? kPlBadPair : 0);
    return SLAM_OK;
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_plicp_normals_f64(const double* pts, const int64_t* scan_off, int32_t S, int64_t P, int32_t K, double rho2,
                           double ctol, double* out_normals, void* stream) {
    if (!pts || !scan_off || !out_normals) return fail(SLAM_EINVAL, "plicp normals: null array");
    if (S < 0 || P < 0) return fail(SLAM_EINVAL, "plicp normals: S = %d, P = %lld: negative", S, static_cast<long long>(P));
    if (K < 1) return fail(SLAM_EINVAL, "plicp normals: K = %d < 1", K);
    if (!plicp_tol_ok(rho2) || !plicp_tol_ok(ctol))
        return fail(SLAM_EINVAL, "plicp normals: a negative or non-finite tolerance");
    if (reinterpret_cast<uintptr_t>(pts) % 16 || reinterpret_cast<uintptr_t>(out_normals) % 16)
        return fail(SLAM_EINVAL, "plicp normals: points or normals not 16-byte aligned");
    if (S == 0 || P == 0) return ok();
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(out_normals, 0, static_cast<size_t>(P) * 16, st) != hipSuccess)
        return fail(SLAM_EHIP, "plicp normals: memset");
    hipLaunchKernelGGL(plicp_normals_kernel, dim3(static_cast<unsigned>(S)), dim3(kPlBlock), 0, st, pts, scan_off, P, K,
                       rho2, ctol, out_normals);
    return check_launch("plicp normals kernel");
}

int slam_plicp_batch_f64(const double* pts, const int64_t* scan_off, int32_t S, int64_t P, const double* normals,
                         const int32_t* src_scan, const int32_t* dst_scan, const double* init, int32_t B,
                         double max_dist2, int32_t min_inliers, int32_t max_iters, double eps_t, double eps_r,
                         double pivot_tol, int32_t max_n1, double* out_tf, double* out_err, double* out_obs,
                         int32_t* out_inliers, int32_t* out_iters, int32_t* out_status, int32_t* out_match,
                         int32_t match_stride, void* stream) {
    if (!pts || !scan_off || !normals || !src_scan || !dst_scan || !init || !out_tf || !out_err || !out_obs ||
        !out_inliers || !out_iters || !out_status)
        return fail(SLAM_EINVAL, "plicp: null array");
    if (B < 0 || S < 0 || P < 0)
        return fail(SLAM_EINVAL, "plicp: B = %d, S = %d, P = %lld: negative", B, S, static_cast<long long>(P));
    if (max_iters < 1) return fail(SLAM_EINVAL, "plicp: max_iters = %d < 1", max_iters);
    if (!plicp_tol_ok(max_dist2) || !plicp_tol_ok(eps_t) || !plicp_tol_ok(eps_r) || !plicp_tol_ok(pivot_tol))
        return fail(SLAM_EINVAL, "plicp: a negative or non-finite tolerance");
    if (max_n1 < 0) return fail(SLAM_EINVAL, "plicp: max_n1 = %d < 0", max_n1);
    if (max_n1 > kPlMaxQuery)
        return fail(SLAM_ETOOBIG, "plicp: a source scan of %d points, above %d", max_n1, kPlMaxQuery);
    if (out_match && match_stride < max_n1)
        return fail(SLAM_EINVAL, "plicp: match stride %d below max_n1 = %d", match_stride, max_n1);
    if (reinterpret_cast<uintptr_t>(pts) % 16 || reinterpret_cast<uintptr_t>(normals) % 16)
        return fail(SLAM_EINVAL, "plicp: points or normals not 16-byte aligned");
    if (B == 0) return ok();
    PlicpArgs A;
    A.pts = pts;
    A.scan_off = scan_off;
    A.normals = normals;
    A.src = src_scan;
    A.dst = dst_scan;
    A.init = init;
    A.P = P;
    A.S = S;
    A.min_inliers = min_inliers;
    A.max_iters = max_iters;
    A.max_n1 = max_n1;
    A.match_stride = out_match ? match_stride : 0;
    A.max_dist2 = max_dist2;
    A.eps_t = eps_t;
    A.eps_r = eps_r;
    A.pivot_tol = pivot_tol;
    A.out_tf = out_tf;
    A.out_err = out_err;
    A.out_obs = out_obs;
    A.out_inliers = out_inliers;
    A.out_iters = out_iters;
    A.out_status = out_status;
    A.out_match = out_match;
    hipStream_t st = as_stream(stream);
    const int qpt = (max_n1 + kPlBlock - 1) / kPlBlock;   // queries per lane: the smallest instance that holds them
#define SLAM_PLICP_LAUNCH(q) hipLaunchKernelGGL(plicp_pair_kernel<q>, dim3(static_cast<unsigned>(B)), dim3(kPlBlock), 0, st, A)
    if (qpt <= 1) SLAM_PLICP_LAUNCH(1);
    else if (qpt <= 2) SLAM_PLICP_LAUNCH(2);
    else if (qpt <= 5) SLAM_PLICP_LAUNCH(5);
    else if (qpt <= 8) SLAM_PLICP_LAUNCH(8);
    else if (qpt <= 16) SLAM_PLICP_LAUNCH(16);
    else SLAM_PLICP_LAUNCH(32);
#undef SLAM_PLICP_LAUNCH
    return check_launch("plicp pair kernel");
}

int slam_plicp_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "plicp status: stream sync");
    int st = 0;
    if (const int rc = plicp_read_clear(&st)) return rc;
    if (st == 0) return ok();
    return fail(SLAM_EINVAL, "plicp:%s%s", st & kPlBadScan ? " a scan's offsets descend or leave [0, P];" : "",
                st & kPlBadPair ? " a pair names a scan outside [0, S), has bad offsets or exceeds max_n1 / the match "
                                  "stride (its out_status is -1);"
                                : "");
}

}  // extern "C"
