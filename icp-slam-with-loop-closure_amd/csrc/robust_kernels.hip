// robust_kernels.hip — robust loss kernels for the Gauss-Newton solve, by
// per-edge reweighting (iteratively reweighted least squares), gfx950.
//
// The GN kernels (gn_kernels.hip) read one scalar weight per edge, w[e], and
// minimise sum_e w[e] |e_e|^2.  A robust loss rho(s) of the weighted squared
// residual s_e = info_e |e_e|^2 is minimised by the same iteration when w is
// rewritten before every step as w[e] = info_e rho'(s_e) at the current poses.
// This file is that rewrite and nothing else: ONE launch of one thread per
// edge in front of the unchanged iteration.  It restates the residual of
// gn_kernels.hip's linearize_edge (same operations in the same order; the
// build does not contract, so the two agree bit for bit on the same device):
//
//   z   = (tf[2], tf[5], atan2(tf[3], tf[0]))
//   e_t = Rz^T (Ri^T (tj - ti) - tz),   e_th = wrap_pi(thj - thi - thz)
//
// ratio r(s) = rho'(s) and cost rho(s), c2 = c^2 (gnc-gm: c2 = mu c^2):
//   huber    r = 1 (s <= c2), c / sqrt(s)         rho = s, 2 c sqrt(s) - c2
//   cauchy   r = 1 / (1 + s / c2)                 rho = c2 log1p(s / c2)
//   gm       r = (c2 / (c2 + s))^2                rho = c2 s / (c2 + s)
//   dcs      r = sg^2, sg = min(1, 2 c2 / (c2 + s))
//                                                 rho = s (sg = 1), c2 (3 s - c2) / (c2 + s)
// (the DCS cost is the integral of its ratio; the switch-variable form
// sg^2 s + c2 (1 - sg)^2 is the constant c2 past the kink: DESIGN.md 3.13).
// An edge with robust_mask[e] == 0 keeps r = 1 and adds s to the cost.
//
// The cost and the largest masked s leave the launch as one partial per
// workgroup (fixed summation order, no atomics); the host adds the partials.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace slamhip {

constexpr int kRobustBlock = 256;   // threads (edges) per workgroup, one cost / max partial each

__device__ __forceinline__ double robust_wrap_pi(double a) {
    return a - 2.0 * M_PI * floor((a + M_PI) / (2.0 * M_PI));
}

// |e|^2 of edge e as linearize_edge forms it (ev[0]^2 + ev[1]^2 + ev[2]^2)
__device__ __forceinline__ double robust_edge_sq(const double* __restrict__ poses, const int32_t* __restrict__ ea,
                                                 const int32_t* __restrict__ eb, const double* __restrict__ tf, int e) {
    const int i = ea[e], j = eb[e];
    const double* t = tf + 9 * static_cast<int64_t>(e);
    const double zx = t[2], zy = t[5], zt = atan2(t[3], t[0]);
    const double xi = poses[3 * i], yi = poses[3 * i + 1], ti = poses[3 * i + 2];
    const double xj = poses[3 * j], yj = poses[3 * j + 1], tj = poses[3 * j + 2];
    double si, ci, sz, cz;
    sincos(ti, &si, &ci);
    sincos(zt, &sz, &cz);
    const double dx = xj - xi, dy = yj - yi;
    const double ux = ci * dx + si * dy, uy = -si * dx + ci * dy;   // Ri^T (tj - ti)
    const double vx = ux - zx, vy = uy - zy;
    const double e0 = cz * vx + sz * vy;
    const double e1 = -sz * vx + cz * vy;
    const double e2 = robust_wrap_pi(tj - ti - zt);
    return e0 * e0 + e1 * e1 + e2 * e2;
}

// r(s) and rho(s) of one loss; c2 already carries gnc-gm's mu
__device__ __forceinline__ void robust_loss(int loss, double s, double c, double c2, double& r, double& rho) {
    switch (loss) {
    case SLAM_LOSS_HUBER:
        if (s <= c2) {
            r = 1.0;
            rho = s;
        } else {
            const double q = sqrt(s);
            r = c / q;
            rho = 2.0 * c * q - c2;
        }
        break;
    case SLAM_LOSS_CAUCHY: {
        const double u = s / c2;
        r = 1.0 / (1.0 + u);
        rho = c2 * log1p(u);
        break;
    }
    case SLAM_LOSS_DCS: {
        const double sg = fmin(1.0, (2.0 * c2) / (c2 + s));
        r = sg * sg;
        rho = sg < 1.0 ? (c2 * (3.0 * s - c2)) / (c2 + s) : s;
        break;
    }
    case SLAM_LOSS_GM:
    case SLAM_LOSS_GNC_GM: {
        const double q = c2 / (c2 + s);
        r = q * q;
        rho = (c2 * s) / (c2 + s);
        break;
    }
    default:   // unreachable: the entry point refuses any other loss; such an edge keeps r = 1
        break;
    }
}

// Largest of the workgroup's values (all >= 0): max is exact, so any order.
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int w = 1; w < kRobustBlock / 64; ++w) m = fmax(m, red[w]);
    return m;
}

__global__ __launch_bounds__(kRobustBlock) void gn_robust_weights_kernel(
    const double* __restrict__ poses, const int32_t* __restrict__ ea, const int32_t* __restrict__ eb,
    const double* __restrict__ tf, const double* __restrict__ info, const uint8_t* __restrict__ robust_mask, int32_t E,
    int32_t loss, double c, double c2, double* __restrict__ w_out, double* __restrict__ s_out,
    double* __restrict__ ratio_out, double* __restrict__ cost_partials, double* __restrict__ smax_partials) {
    __shared__ double red[kRobustBlock / 64];
    __shared__ double redm[kRobustBlock / 64];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    double cost = 0.0, smax = 0.0;
    if (e < E) {
        const double we = info[e];
        const double s = we * robust_edge_sq(poses, ea, eb, tf, e);
        double r = 1.0, rho = s;
        if (robust_mask[e]) {
            robust_loss(loss, s, c, c2, r, rho);
            smax = s;
        }
        w_out[e] = we * r;
        s_out[e] = s;
        ratio_out[e] = r;
        cost = rho;
    }
    double v[1] = {cost};
    block_sum<1, kRobustBlock / 64>(v, red);
    const double m = block_max(smax, redm);
    if (threadIdx.x == 0) {
        cost_partials[blockIdx.x] = v[0];
        smax_partials[blockIdx.x] = m;
    }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

static_assert(kRobustBlock == SLAM_GN_ROBUST_BLOCK, "the header's partial count");

int slam_gn_robust_weights_f64(const double* poses, const int32_t* ea, const int32_t* eb, const double* tf,
                               const double* info, const uint8_t* robust_mask, int32_t E, int32_t loss, double c,
                               double mu, double* w_out, double* s_out, double* ratio_out, double* cost_partials,
                               double* smax_partials, void* stream) {
    if (E < 0) return fail(SLAM_EINVAL, "gn robust: E=%d", E);
    if (loss < SLAM_LOSS_HUBER || loss > SLAM_LOSS_GNC_GM)
        return fail(SLAM_EINVAL, "gn robust: unknown loss %d (huber 0, cauchy 1, gm 2, dcs 3, gnc-gm 4)", loss);
    if (!std::isfinite(c) || !(c > 0.0)) return fail(SLAM_EINVAL, "gn robust: scale c=%g is not finite and positive", c);
    if (!std::isfinite(mu) || !(mu >= 1.0)) return fail(SLAM_EINVAL, "gn robust: mu=%g is not finite and >= 1", mu);
    if (!poses || !ea || !eb || !tf || !info || !robust_mask || !w_out || !s_out || !ratio_out || !cost_partials ||
        !smax_partials)
        return fail(SLAM_EINVAL, "gn robust: null array argument");
    if (E == 0) return ok();
    double c2 = c * c;
    if (loss == SLAM_LOSS_GNC_GM) c2 = mu * c2;
    hipLaunchKernelGGL(gn_robust_weights_kernel, dim3((E + kRobustBlock - 1) / kRobustBlock), dim3(kRobustBlock), 0,
                       as_stream(stream), poses, ea, eb, tf, info, robust_mask, E, loss, c, c2, w_out, s_out,
                       ratio_out, cost_partials, smax_partials);
    return check_launch("gn robust weights kernel");
}

}  // extern "C"
