// loc_kernels.hip — localisation of scans in a finished occupancy grid for
// gfx950 (MI355X).  include/slamhip.h states the three definitions;
// tests/loc_ref.py restates them in NumPy.  The reference has no counterpart.
//
// Field (integers only): F[r][c] = min(d_cap^2, squared cell distance to the
// nearest occupied cell), uint16.  loc_col_kernel: one thread per (column, band
// of 128 rows), a down sweep and an up sweep of the capped vertical distance g,
// each started d_cap rows outside the band with g = d_cap (an occupied cell
// further away cannot matter under the cap), adjacent columns on adjacent lanes.
// loc_row_kernel: one workgroup per (row, 256 columns), g^2 of the columns
// within d_cap of the tile in LDS (d_cap outside the grid), every thread takes
// the minimum of g^2 + dx^2 over |dx| <= d_cap: conflict-free LDS reads.
//
// Search: B queries (scan, centre) against ONE table shared by all of them, a
// copy of F with a border of d_cap^2, ny step rows and nx step columns wide, made
// per call by loc_table_kernel (uint16, or uint8 when d_cap <= 15 and the caller
// asks for it).  A query cell is clamped in fp64 into the range from which every
// shift stays inside the bordered table, and a clamped cell reads only border:
// no bounds test in the gather loop, no int32 overflow for far-away points.
// loc_search_kernel<R, T>: one workgroup per (query, angle), the angle's cells
// in LDS, each thread owns R shifts with adjacent i on adjacent lanes, the point
// loop reads the cell from LDS as a broadcast and gathers R table entries.
// Costs are int32 sums, so the order is free; the minimum, ties to the smallest
// flat index, is an atomic min of the 64-bit key cost << 32 | flat.
//
// Refinement: loc_refine_kernel, one 256-thread workgroup per query, every
// iteration on chip.  Thread t takes the points t, t + 256, ... in ascending
// order, reads the four field cells around each (L2 hits: the map is shared),
// and adds its rows to eleven sums; block_sum (common.hpp) then adds the
// threads' sums in its fixed tree, and every thread solves the 3x3 system on the
// same bits.  The launch shape is fixed, so the order of the sums is too.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kLocBlock = 256;
constexpr int kLocWaves = kLocBlock / 64;
constexpr int kLocBand = 128;     // rows per thread of the column pass
constexpr int kLocMaxCap = 255;   // d_cap^2 <= 65,025 fits uint16
constexpr int kLocMaxR = 8;       // shifts per thread and pass
constexpr int kLocTile = 4096;    // query cells per LDS tile (16 KiB)
constexpr int kLocSums = 11;      // H00 H01 H02 H11 H12 H22 g0 g1 g2 e m

__device__ int g_loc_bad_query;   // nonzero: a launch since slam_loc_status met a query outside its bounds

// ---------------------------------------------------------------------------------- field

__global__ __launch_bounds__(kLocBlock) void loc_col_kernel(const int8_t* __restrict__ grid, int32_t H, int32_t W,
                                                            int32_t occ_min, int32_t d_cap, uint8_t* __restrict__ g) {
    const int32_t c = blockIdx.x * kLocBlock + threadIdx.x;
    if (c >= W) return;
    const int32_t r0 = blockIdx.y * kLocBand;
    const int32_t r1 = min(H, r0 + kLocBand);
    int32_t d = d_cap;
    for (int32_t r = max(0, r0 - d_cap); r < r1; ++r) {
        const int64_t at = static_cast<int64_t>(r) * W + c;
        d = static_cast<int32_t>(grid[at]) > occ_min ? 0 : min(d + 1, d_cap);
        if (r >= r0) g[at] = static_cast<uint8_t>(d);
    }
    d = d_cap;
    for (int32_t r = min(H, r1 + d_cap) - 1; r >= r0; --r) {
        const int64_t at = static_cast<int64_t>(r) * W + c;
        d = static_cast<int32_t>(grid[at]) > occ_min ? 0 : min(d + 1, d_cap);
        if (r < r1) g[at] = static_cast<uint8_t>(min(static_cast<int32_t>(g[at]), d));   // this thread's own store
    }
}

__global__ __launch_bounds__(kLocBlock) void loc_row_kernel(const uint8_t* __restrict__ g, int32_t H, int32_t W,
                                                            int32_t d_cap, uint16_t* __restrict__ F) {
    __shared__ int32_t sq[kLocBlock + 2 * kLocMaxCap];
    const int32_t c0 = blockIdx.x * kLocBlock;
    const int64_t row = static_cast<int64_t>(blockIdx.y) * W;
    const int tid = threadIdx.x;
    for (int32_t k = tid; k < kLocBlock + 2 * d_cap; k += kLocBlock) {
        const int32_t col = c0 - d_cap + k;
        const int32_t v = col >= 0 && col < W ? static_cast<int32_t>(g[row + col]) : d_cap;
        sq[k] = v * v;
    }
    __syncthreads();
    const int32_t c = c0 + tid;
    if (c >= W) return;
    int32_t best = d_cap * d_cap;
    for (int32_t dx = -d_cap; dx <= d_cap; ++dx) best = min(best, sq[tid + d_cap + dx] + dx * dx);
    F[row + c] = static_cast<uint16_t>(best);
}

// --------------------------------------------------------------------------------- search

struct LocGeom {
    int32_t H, W, px, py, wp, hp, step, cap2;   // grid, border columns / rows, bordered size, shift step, d_cap^2
    double min_x, min_y, cw;
};

template <typename T>
__global__ __launch_bounds__(kLocBlock) void loc_table_kernel(const uint16_t* __restrict__ F, LocGeom g,
                                                              T* __restrict__ table) {
    const int64_t cells = static_cast<int64_t>(g.wp) * g.hp;
    for (int64_t at = static_cast<int64_t>(blockIdx.x) * kLocBlock + threadIdx.x; at < cells;
         at += static_cast<int64_t>(gridDim.x) * kLocBlock) {
        const int32_t r = static_cast<int32_t>(at / g.wp) - g.py;
        const int32_t c = static_cast<int32_t>(at % g.wp) - g.px;
        const int32_t v = r >= 0 && r < g.H && c >= 0 && c < g.W ? F[static_cast<int64_t>(r) * g.W + c] : g.cap2;
        table[at] = static_cast<T>(v);
    }
}

// floor((p - o) / cw) clamped to [lo, hi] in fp64 (a NaN gives lo), then int.
__device__ __forceinline__ int32_t loc_cell(double p, double o, double cw, double lo, double hi) {
    const double f = floor((p - o) / cw);
    return static_cast<int32_t>(fmin(fmax(f, lo), hi));
}

__device__ __forceinline__ unsigned long long loc_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor(static_cast<unsigned>(v), off, 64);
        const unsigned hi = __shfl_xor(static_cast<unsigned>(v >> 32), off, 64);
        const unsigned long long w = (static_cast<unsigned long long>(hi) << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

struct LocSearchArgs {
    const double2* pts;
    const int64_t* scan_off;
    const int32_t* q_scan;
    const double* centre;
    const double* rot;
    int64_t P;
    int32_t S, max_n, n_theta, nx, ny;
    unsigned long long* keys;
    int32_t* out_costs;
};

// The query's scan, or false (uniform) when the query is outside the launch's bounds.
__device__ __forceinline__ bool loc_query_scan(const int64_t* scan_off, int32_t s, int32_t S, int64_t P, int32_t max_n,
                                               int64_t* q0, int64_t* n) {
    if (s < 0 || s >= S) return false;
    const int64_t a = scan_off[s], b = scan_off[s + 1];
    if (a < 0 || b < a || b > P || b - a > max_n) return false;
    *q0 = a;
    *n = b - a;
    return true;
}

template <int R, typename T>
__global__ __launch_bounds__(kLocBlock) void loc_search_kernel(const LocSearchArgs A, const LocGeom g,
                                                               const T* __restrict__ table) {
    __shared__ int32_t cell[kLocTile];
    __shared__ unsigned long long red[kLocWaves];
    const int b = blockIdx.x / A.n_theta;
    const int k = blockIdx.x - b * A.n_theta;
    const int tid = threadIdx.x;
    int64_t q0 = 0, n = 0;
    if (!loc_query_scan(A.scan_off, A.q_scan[b], A.S, A.P, A.max_n, &q0, &n)) {
        if (tid == 0) g_loc_bad_query = 1;   // the key stays all ones: loc_best_kernel writes -1
        return;
    }
    const int32_t nx = A.nx, ny = A.ny;
    const double c = A.rot[2 * (static_cast<int64_t>(b) * A.n_theta + k)];
    const double sn = A.rot[2 * (static_cast<int64_t>(b) * A.n_theta + k) + 1];
    const double x0 = A.centre[3 * b + 1], y0 = A.centre[3 * b + 2];
    const int32_t nshift = nx * ny;
    const int32_t hx = nx / 2, hy = ny / 2;
    // the cells from which every shift stays inside the bordered table; a cell
    // clamped to either end has all its shifts in the border (outside the grid)
    const double xlo = static_cast<double>(hx) * g.step - g.px;
    const double xhi = (static_cast<double>(g.W) - 1 + g.px) - static_cast<double>(nx - 1 - hx) * g.step;
    const double ylo = static_cast<double>(hy) * g.step - g.py;
    const double yhi = (static_cast<double>(g.H) - 1 + g.py) - static_cast<double>(ny - 1 - hy) * g.step;
    unsigned long long best = ~0ull;

    for (int32_t s0 = 0; s0 < nshift; s0 += kLocBlock * R) {
        int32_t off[R], acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int32_t u = s0 + r * kLocBlock + tid;
            const int32_t j = u / nx, i = u - j * nx;
            off[r] = u < nshift ? ((j - hy) * g.wp + (i - hx)) * g.step : 0;   // an idle slot re-reads the cell itself
            acc[r] = 0;
        }
        for (int64_t t0 = 0; t0 < n; t0 += kLocTile) {
            const int32_t m = static_cast<int32_t>(n - t0 < kLocTile ? n - t0 : kLocTile);
            __syncthreads();
            for (int32_t p = tid; p < m; p += kLocBlock) {
                const double2 q = A.pts[q0 + t0 + p];
                const double X = (c * q.x - sn * q.y) + x0;
                const double Y = (sn * q.x + c * q.y) + y0;
                const int32_t ix = loc_cell(X, g.min_x, g.cw, xlo, xhi);
                const int32_t iy = loc_cell(Y, g.min_y, g.cw, ylo, yhi);
                cell[p] = (iy + g.py) * g.wp + ix + g.px;
            }
            __syncthreads();
            // two points per trip: eight, with all their gathers in flight at once, ran no faster (DESIGN.md
            // section 3.12: the loop is bound by the cache lines a wave's gather touches, not by latency)
#pragma unroll 2
            for (int32_t p = 0; p < m; ++p) {
                const int32_t base = cell[p];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] += static_cast<int32_t>(table[static_cast<uint32_t>(base + off[r])]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int32_t u = s0 + r * kLocBlock + tid;
            if (u < nshift) {
                const int64_t flat = static_cast<int64_t>(k) * nshift + u;   // < 2^31 (host check)
                if (A.out_costs) A.out_costs[static_cast<int64_t>(b) * A.n_theta * nshift + flat] = acc[r];
                const unsigned long long key =
                    (static_cast<unsigned long long>(static_cast<uint32_t>(acc[r])) << 32) | static_cast<uint32_t>(flat);
                best = key < best ? key : best;
            }
        }
    }
    best = loc_wave_min(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kLocWaves; ++w) best = red[w] < best ? red[w] : best;
        atomicMin(&A.keys[b], best);
    }
}

__global__ void loc_best_kernel(const unsigned long long* __restrict__ keys, int32_t B, int32_t nx, int32_t ny,
                                int32_t* __restrict__ out_best) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long key = keys[b];
    if (key == ~0ull) {   // a query outside its bounds
        out_best[4 * b] = out_best[4 * b + 1] = out_best[4 * b + 2] = out_best[4 * b + 3] = -1;
        return;
    }
    const int32_t flat = static_cast<int32_t>(static_cast<uint32_t>(key));
    const int32_t nshift = nx * ny;
    const int32_t k = flat / nshift, rem = flat - k * nshift;
    out_best[4 * b] = static_cast<int32_t>(key >> 32);
    out_best[4 * b + 1] = k;
    out_best[4 * b + 2] = rem / nx;
    out_best[4 * b + 3] = rem % nx;
}

template <typename T>
using LocSearchFn = void (*)(const LocSearchArgs, const LocGeom, const T*);

template <typename T, int... I>
static LocSearchFn<T> loc_search_instance(int r, std::integer_sequence<int, I...>) {
    static const LocSearchFn<T> table[] = {loc_search_kernel<I + 1, T>...};
    return table[r - 1];
}

// Entry width of the search table on this host thread (slam_loc_set_table).
inline int& loc_table_width() {
    static thread_local int w = 2;
    return w;
}

static bool loc_pos(double v) { return v > 0.0 && std::isfinite(v); }

// Validates the shape and fills the table geometry; 0 or SLAM_EINVAL.
static int loc_shape(int32_t B, int32_t H, int32_t W, double min_x, double min_y, double cw, int32_t d_cap,
                     int32_t n_theta, int32_t ny, int32_t nx, int32_t step, LocGeom* g, int64_t* key_bytes) {
    if (B <= 0) return fail(SLAM_EINVAL, "loc: B = %d <= 0", B);
    if (H <= 0 || W <= 0) return fail(SLAM_EINVAL, "loc: a grid of %d x %d cells", H, W);
    if (d_cap < 1 || d_cap > kLocMaxCap) return fail(SLAM_EINVAL, "loc: d_cap = %d outside 1..%d", d_cap, kLocMaxCap);
    if (!loc_pos(cw) || !std::isfinite(min_x) || !std::isfinite(min_y))
        return fail(SLAM_EINVAL, "loc: cell_width must be positive, the origin finite");
    if (n_theta <= 0 || nx <= 0 || ny <= 0 || step <= 0)
        return fail(SLAM_EINVAL, "loc: n_theta = %d, nx = %d, ny = %d, step = %d must be positive", n_theta, nx, ny, step);
    const int64_t volume = static_cast<int64_t>(n_theta) * ny * nx;
    if (static_cast<int64_t>(ny) * nx > (1ll << 30) || volume >= (1ll << 31))
        return fail(SLAM_EINVAL, "loc: cost volume of %d x %d x %d entries does not fit 31 bits", n_theta, ny, nx);
    if (static_cast<int64_t>(B) * n_theta >= (1ll << 31))
        return fail(SLAM_EINVAL, "loc: %d queries x %d angles exceed the launch grid", B, n_theta);
    const int64_t px = static_cast<int64_t>(nx) * step, py = static_cast<int64_t>(ny) * step;
    const int64_t wp = W + 2 * px, hp = H + 2 * py;
    if (wp * hp >= (1ll << 31))
        return fail(SLAM_EINVAL, "loc: bordered table of %lld x %lld cells does not fit 31 bits",
                    static_cast<long long>(hp), static_cast<long long>(wp));
    g->H = H;
    g->W = W;
    g->px = static_cast<int32_t>(px);
    g->py = static_cast<int32_t>(py);
    g->wp = static_cast<int32_t>(wp);
    g->hp = static_cast<int32_t>(hp);
    g->step = step;
    g->cap2 = d_cap * d_cap;
    g->min_x = min_x;
    g->min_y = min_y;
    g->cw = cw;
    *key_bytes = (8 * static_cast<int64_t>(B) + 255) / 256 * 256;
    return SLAM_OK;
}

// ----------------------------------------------------------------------------- refinement

struct LocRefineArgs {
    const double2* pts;
    const int64_t* scan_off;
    const int32_t* q_scan;
    const double* init;
    const uint16_t* F;
    int64_t P;
    int32_t S, max_n, H, W, cap2, max_iters;
    double min_x, min_y, cw, eps_t, eps_r, min_inlier_frac, pivot_tol;
    double* out_pose;
    double* out_rms;
    int32_t* out_inliers;
    int32_t* out_iters;
    int32_t* out_status;
};

__device__ __forceinline__ bool loc_bad_pivot(double d, double hkk, double tol) {
    return !(fabs(d) < INFINITY) || d <= tol * hkk;   // not finite (NaN included) or too small
}

__global__ __launch_bounds__(kLocBlock) void loc_refine_kernel(const LocRefineArgs A) {
    __shared__ double red[kLocWaves * kLocSums];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double th = A.init[3 * b], x = A.init[3 * b + 1], y = A.init[3 * b + 2];
    int64_t q0 = 0, n = 0;
    if (!loc_query_scan(A.scan_off, A.q_scan[b], A.S, A.P, A.max_n, &q0, &n)) {   // uniform
        if (tid == 0) {
            g_loc_bad_query = 1;
            A.out_pose[3 * b] = th;
            A.out_pose[3 * b + 1] = x;
            A.out_pose[3 * b + 2] = y;
            A.out_rms[b] = nan;
            A.out_inliers[b] = 0;
            A.out_iters[b] = 0;
            A.out_status[b] = -1;
        }
        return;
    }
    const double2* Ps = A.pts + q0;
    const uint16_t* __restrict__ F = A.F;
    const int32_t W = A.W;
    const double cw = A.cw;
    const double umax = static_cast<double>(W) - 2.0, vmax = static_cast<double>(A.H) - 2.0;
    int it = 0, status = 0, m = 0;
    double rms = nan;
    for (;;) {
        const double c = cos(th), sn = sin(th);
        double s[kLocSums];
#pragma unroll
        for (int k = 0; k < kLocSums; ++k) s[k] = 0.0;
        for (int64_t i = tid; i < n; i += kLocBlock) {
            const double2 p = Ps[i];
            const double gx = ((c * p.x) - (sn * p.y)) + x;
            const double gy = ((sn * p.x) + (c * p.y)) + y;
            const double u = ((gx - A.min_x) / cw) - 0.5;
            const double v = ((gy - A.min_y) / cw) - 0.5;
            const double fu = floor(u), fv = floor(v);
            if (!(fu >= 0.0 && fu <= umax && fv >= 0.0 && fv <= vmax)) continue;   // a cell outside the grid (or NaN)
            const int32_t i0 = static_cast<int32_t>(fu), j0 = static_cast<int32_t>(fv);
            const int64_t at = static_cast<int64_t>(j0) * W + i0;
            const int32_t f00 = F[at], f10 = F[at + 1], f01 = F[at + W], f11 = F[at + W + 1];
            if (f00 == A.cap2 && f10 == A.cap2 && f01 == A.cap2 && f11 == A.cap2) continue;
            const double a = u - fu, bb = v - fv;
            const double a1 = 1.0 - a, b1 = 1.0 - bb;
            const double D00 = sqrt(static_cast<double>(f00)) * cw, D10 = sqrt(static_cast<double>(f10)) * cw;
            const double D01 = sqrt(static_cast<double>(f01)) * cw, D11 = sqrt(static_cast<double>(f11)) * cw;
            const double r = (b1 * ((a1 * D00) + (a * D10))) + (bb * ((a1 * D01) + (a * D11)));
            const double jx = ((b1 * (D10 - D00)) + (bb * (D11 - D01))) / cw;
            const double jy = ((a1 * (D01 - D00)) + (a * (D11 - D10))) / cw;
            const double jt = (jx * ((-sn * p.x) - (c * p.y))) + (jy * ((c * p.x) - (sn * p.y)));
            s[0] += jx * jx;
            s[1] += jx * jy;
            s[2] += jx * jt;
            s[3] += jy * jy;
            s[4] += jy * jt;
            s[5] += jt * jt;
            s[6] += jx * r;
            s[7] += jy * r;
            s[8] += jt * r;
            s[9] += r * r;
            s[10] += 1.0;
        }
        __syncthreads();   // every wave is done with the previous iteration's red
        block_sum<kLocSums, kLocWaves>(s, red);
        const double H00 = s[0], H01 = s[1], H02 = s[2], H11 = s[3], H12 = s[4], H22 = s[5];
        m = static_cast<int>(s[10]);
        rms = sqrt(s[9] / s[10]);
        if (m == 0 || s[10] < A.min_inlier_frac * static_cast<double>(n)) {
            status = 3;
            break;
        }
        status = 2;
        const double dd0 = H00;
        if (loc_bad_pivot(dd0, H00, A.pivot_tol)) break;
        const double l10 = H01 / dd0, l20 = H02 / dd0;
        const double dd1 = H11 - (l10 * H01);
        if (loc_bad_pivot(dd1, H11, A.pivot_tol)) break;
        const double uu = H12 - (l20 * H01);
        const double l21 = uu / dd1;
        const double dd2 = (H22 - (l20 * H02)) - (l21 * uu);
        if (loc_bad_pivot(dd2, H22, A.pivot_tol)) break;
        const double z0 = -s[6];
        const double z1 = -s[7] - (l10 * z0);
        const double z2 = (-s[8] - (l20 * z0)) - (l21 * z1);
        const double dth = z2 / dd2;
        const double dy = (z1 / dd1) - (l21 * dth);
        const double dx = ((z0 / dd0) - (l10 * dy)) - (l20 * dth);
        x = x + dx;
        y = y + dy;
        th = th + dth;
        ++it;
        if (sqrt((dx * dx) + (dy * dy)) < A.eps_t && fabs(dth) < A.eps_r) {
            status = 0;
            break;
        }
        if (it == A.max_iters) {
            status = 1;
            break;
        }
    }
    if (tid == 0) {
        A.out_pose[3 * b] = th;
        A.out_pose[3 * b + 1] = x;
        A.out_pose[3 * b + 2] = y;
        A.out_rms[b] = rms;
        A.out_inliers[b] = m;
        A.out_iters[b] = it;
        A.out_status[b] = status;
    }
}

static bool loc_tol_ok(double v) { return v >= 0.0 && std::isfinite(v); }

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int64_t slam_loc_field_work_size(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return fail(SLAM_EINVAL, "loc field: a grid of %d x %d cells", H, W);
    ok();
    return (static_cast<int64_t>(H) * W + 255) / 256 * 256;   // bytes: the capped vertical distances
}

int slam_loc_field(const int8_t* grid, int32_t H, int32_t W, int32_t occ_min, int32_t d_cap, uint16_t* out_field,
                   void* work, void* stream) {
    if (H <= 0 || W <= 0) return fail(SLAM_EINVAL, "loc field: a grid of %d x %d cells", H, W);
    if (d_cap < 1 || d_cap > kLocMaxCap)
        return fail(SLAM_EINVAL, "loc field: d_cap = %d outside 1..%d", d_cap, kLocMaxCap);
    if (occ_min < -128 || occ_min > 127) return fail(SLAM_EINVAL, "loc field: occ_min = %d outside int8", occ_min);
    if (H > 65535) return fail(SLAM_EINVAL, "loc field: H = %d exceeds the launch grid", H);
    if (!grid || !out_field || !work) return fail(SLAM_EINVAL, "loc field: null array");
    hipStream_t st = as_stream(stream);
    uint8_t* g = reinterpret_cast<uint8_t*>(work);
    const unsigned bx = static_cast<unsigned>((W + kLocBlock - 1) / kLocBlock);
    hipLaunchKernelGGL(loc_col_kernel, dim3(bx, static_cast<unsigned>((H + kLocBand - 1) / kLocBand)), dim3(kLocBlock),
                       0, st, grid, H, W, occ_min, d_cap, g);
    hipLaunchKernelGGL(loc_row_kernel, dim3(bx, static_cast<unsigned>(H)), dim3(kLocBlock), 0, st, g, H, W, d_cap,
                       out_field);
    return check_launch("loc field kernels");
}

int64_t slam_loc_search_work_size(int32_t B, int32_t H, int32_t W, int32_t n_theta, int32_t ny, int32_t nx,
                                  int32_t step) {
    // bytes: best keys (u64 / query) | the bordered table ((H + 2 ny step) x (W + 2 nx step) entries of 2 bytes)
    LocGeom g;
    int64_t key_bytes;
    if (loc_shape(B, H, W, 0.0, 0.0, 1.0, 1, n_theta, ny, nx, step, &g, &key_bytes) != SLAM_OK) return SLAM_EINVAL;
    ok();
    return key_bytes + (2 * static_cast<int64_t>(g.wp) * g.hp + 255) / 256 * 256;
}

int slam_loc_search(const uint16_t* field, int32_t H, int32_t W, double min_x, double min_y, double cell_width,
                    int32_t d_cap, const double* pts, const int64_t* scan_off, int32_t S, int64_t P,
                    const int32_t* q_scan, const double* centre, const double* rot, int32_t B, int32_t max_n,
                    int32_t n_theta, int32_t nx, int32_t ny, int32_t step, int32_t* out_best, int32_t* out_costs,
                    void* work, void* stream) {
    LocGeom g;
    int64_t key_bytes;
    if (loc_shape(B, H, W, min_x, min_y, cell_width, d_cap, n_theta, ny, nx, step, &g, &key_bytes) != SLAM_OK)
        return SLAM_EINVAL;
    if (S < 0 || P < 0 || max_n < 0)
        return fail(SLAM_EINVAL, "loc: S = %d, P = %lld, max_n = %d: negative", S, static_cast<long long>(P), max_n);
    if (static_cast<int64_t>(max_n) * g.cap2 >= (1ll << 31))
        return fail(SLAM_EINVAL, "loc: a scan of %d points at d_cap = %d: its cost does not fit 31 bits", max_n, d_cap);
    if (!field || !pts || !scan_off || !q_scan || !centre || !rot || !out_best || !work)
        return fail(SLAM_EINVAL, "loc: null array");
    if (reinterpret_cast<uintptr_t>(pts) % 16 || reinterpret_cast<uintptr_t>(work) % 8)
        return fail(SLAM_EINVAL, "loc: points not 16-byte or work not 8-byte aligned");
    hipStream_t st = as_stream(stream);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(work);
    void* table = reinterpret_cast<uint8_t*>(work) + key_bytes;
    if (hipMemsetAsync(keys, 0xff, static_cast<size_t>(key_bytes), st) != hipSuccess)
        return fail(SLAM_EHIP, "loc: workspace clear");
    const bool bytes = loc_table_width() == 1 && g.cap2 <= 255;
    const int64_t cells = static_cast<int64_t>(g.wp) * g.hp;
    const unsigned tb = static_cast<unsigned>(std::min<int64_t>((cells + kLocBlock - 1) / kLocBlock, 4096));
    if (bytes)
        hipLaunchKernelGGL(loc_table_kernel<uint8_t>, dim3(tb), dim3(kLocBlock), 0, st, field, g,
                           reinterpret_cast<uint8_t*>(table));
    else
        hipLaunchKernelGGL(loc_table_kernel<uint16_t>, dim3(tb), dim3(kLocBlock), 0, st, field, g,
                           reinterpret_cast<uint16_t*>(table));
    LocSearchArgs A;
    A.pts = reinterpret_cast<const double2*>(pts);
    A.scan_off = scan_off;
    A.q_scan = q_scan;
    A.centre = centre;
    A.rot = rot;
    A.P = P;
    A.S = S;
    A.max_n = max_n;
    A.n_theta = n_theta;
    A.nx = nx;
    A.ny = ny;
    A.keys = keys;
    A.out_costs = out_costs;
    // passes of at most kLocBlock * kLocMaxR shifts, spread evenly over them
    const int64_t nshift = static_cast<int64_t>(ny) * nx;
    const int64_t passes = (nshift + kLocBlock * kLocMaxR - 1) / (kLocBlock * kLocMaxR);
    const int R = static_cast<int>((nshift + kLocBlock * passes - 1) / (kLocBlock * passes));
    const dim3 grid(static_cast<unsigned>(B) * static_cast<unsigned>(n_theta));
    if (bytes)
        hipLaunchKernelGGL(loc_search_instance<uint8_t>(R, std::make_integer_sequence<int, kLocMaxR>()), grid,
                           dim3(kLocBlock), 0, st, A, g, reinterpret_cast<const uint8_t*>(table));
    else
        hipLaunchKernelGGL(loc_search_instance<uint16_t>(R, std::make_integer_sequence<int, kLocMaxR>()), grid,
                           dim3(kLocBlock), 0, st, A, g, reinterpret_cast<const uint16_t*>(table));
    hipLaunchKernelGGL(loc_best_kernel, dim3((B + 255) / 256), dim3(256), 0, st, keys, B, nx, ny, out_best);
    return check_launch("loc search kernels");
}

int slam_loc_set_table(int width) {
    if (width != 1 && width != 2) return fail(SLAM_EINVAL, "loc: table entry width %d (1 or 2)", width);
    loc_table_width() = width;
    return ok();
}

int slam_loc_refine_f64(const uint16_t* field, int32_t H, int32_t W, double min_x, double min_y, double cell_width,
                        int32_t d_cap, const double* pts, const int64_t* scan_off, int32_t S, int64_t P,
                        const int32_t* q_scan, const double* init, int32_t B, int32_t max_n, int32_t max_iters,
                        double eps_t, double eps_r, double min_inlier_frac, double pivot_tol, double* out_pose,
                        double* out_rms, int32_t* out_inliers, int32_t* out_iters, int32_t* out_status, void* stream) {
    if (B < 0 || S < 0 || P < 0 || max_n < 0)
        return fail(SLAM_EINVAL, "loc refine: B = %d, S = %d, P = %lld, max_n = %d: negative", B, S,
                    static_cast<long long>(P), max_n);
    if (H <= 0 || W <= 0) return fail(SLAM_EINVAL, "loc refine: a grid of %d x %d cells", H, W);
    if (d_cap < 1 || d_cap > kLocMaxCap)
        return fail(SLAM_EINVAL, "loc refine: d_cap = %d outside 1..%d", d_cap, kLocMaxCap);
    if (!loc_pos(cell_width) || !std::isfinite(min_x) || !std::isfinite(min_y))
        return fail(SLAM_EINVAL, "loc refine: cell_width must be positive, the origin finite");
    if (max_iters < 1) return fail(SLAM_EINVAL, "loc refine: max_iters = %d < 1", max_iters);
    if (!loc_tol_ok(eps_t) || !loc_tol_ok(eps_r) || !loc_tol_ok(pivot_tol) || !loc_tol_ok(min_inlier_frac) ||
        min_inlier_frac > 1.0)
        return fail(SLAM_EINVAL, "loc refine: a negative or non-finite tolerance, or min_inlier_frac above 1");
    if (!field || !pts || !scan_off || !q_scan || !init || !out_pose || !out_rms || !out_inliers || !out_iters ||
        !out_status)
        return fail(SLAM_EINVAL, "loc refine: null array");
    if (reinterpret_cast<uintptr_t>(pts) % 16) return fail(SLAM_EINVAL, "loc refine: points not 16-byte aligned");
    if (B == 0) return ok();
    LocRefineArgs A;
    A.pts = reinterpret_cast<const double2*>(pts);
    A.scan_off = scan_off;
    A.q_scan = q_scan;
    A.init = init;
    A.F = field;
    A.P = P;
    A.S = S;
    A.max_n = max_n;
    A.H = H;
    A.W = W;
    A.cap2 = d_cap * d_cap;
    A.max_iters = max_iters;
    A.min_x = min_x;
    A.min_y = min_y;
    A.cw = cell_width;
    A.eps_t = eps_t;
    A.eps_r = eps_r;
    A.min_inlier_frac = min_inlier_frac;
    A.pivot_tol = pivot_tol;
    A.out_pose = out_pose;
    A.out_rms = out_rms;
    A.out_inliers = out_inliers;
    A.out_iters = out_iters;
    A.out_status = out_status;
    hipLaunchKernelGGL(loc_refine_kernel, dim3(static_cast<unsigned>(B)), dim3(kLocBlock), 0, as_stream(stream), A);
    return check_launch("loc refine kernel");
}

int slam_loc_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "loc status: stream sync");
    int bad = 0;
    if (hipMemcpyFromSymbol(&bad, HIP_SYMBOL(g_loc_bad_query), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "loc status: read");
    const int zero = 0;
    if (bad && hipMemcpyToSymbol(HIP_SYMBOL(g_loc_bad_query), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "loc status: clear");
    if (!bad) return ok();
    return fail(SLAM_EINVAL, "loc: a query names a scan outside [0, S), one whose offsets descend or leave [0, P], or "
                             "one of more than max_n points (its best row / status is -1)");
}

}  // extern "C"
