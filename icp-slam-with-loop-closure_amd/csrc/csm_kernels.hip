// csm_kernels.hip — batched correlative scan matcher for gfx950 (MI355X).
//
// Brute-force, single-resolution correlative scan matching (Olson 2009) of B
// scan pairs: an initial guess for loop-closure ICP that does not depend on
// the two scans sharing a heading.  The reference (cohnt/ICP-SLAM-with-Loop-
// Closure) has no counterpart: it starts every loop-closure ICP from identity.
//
// Per pair: the reference scan is rasterised into a uint8 look-up table L
// (2 on a cell that holds a point, 1 on its 8 neighbours, 0 elsewhere); for
// every angle bin the query scan is rotated, shifted to the search centre and
// binned to cells; the score of (angle k, shift j, i) is the sum of L over the
// query cells moved by the shift.  Only integers are summed, so the result is
// the same for any summation order, workgroup split or GPU; the best score,
// ties to the smallest flat index (k ny + j) nx + i, is an atomic max of the
// 64-bit key score << 32 | ~flat.
//
// The table lives in the caller's workspace with a zero border of nx columns
// (nx + 4 on the right) and ny rows on every side.  A query cell is clamped
// (in fp64, before the conversion to int) into the range from which every
// shift of the window stays inside the bordered table, and a clamped cell
// reads only border: no bounds test in the gather loop, no int32 overflow for
// far-away points.
//
// Kernels: csm_raster_kernel (one workgroup per pair; launched twice, first
// every 1, then every 2: plain byte stores, no atomics, no store-order
// dependence), csm_score_kernel<R, W> (one workgroup per (pair, angle): query
// cells of the angle in LDS, each thread owns R slots of W shifts with
// adjacent i on adjacent lanes, the point loop reads the cell from LDS as a
// broadcast and gathers R table bytes (W = 1) or dwords (W = 4, the default;
// DESIGN.md section 3.5 has the A/B), csm_best_kernel (unpacks the keys).

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <utility>

#include "common.hpp"

namespace slamhip {

constexpr int kCsmBlock = 256;
constexpr int kCsmMaxR = 16;      // slots per thread and pass, byte gathers (1 shift per slot)
constexpr int kCsmMaxR4 = 8;      // the same, dword gathers (4 shifts per slot)
constexpr int kCsmTile = 4096;    // query cells per LDS tile (16 KiB)

struct CsmGeom {
    int32_t G, px, py, wp;   // cells per side, border columns / rows, bordered row length
    int64_t tbl;             // bytes per pair's bordered table (multiple of 256)
    double o, res;           // grid origin -(G / 2) res, cell width
};

// floor((p - o) / res) clamped to [lo, hi] in fp64 (a NaN gives lo), then int.
__device__ __forceinline__ int32_t csm_cell(double p, double o, double res, double lo, double hi) {
    const double f = floor((p - o) / res);
    return static_cast<int32_t>(fmin(fmax(f, lo), hi));
}

__global__ __launch_bounds__(kCsmBlock) void csm_raster_kernel(const double2* __restrict__ pts,
                                                               const int64_t* __restrict__ scan_off,
                                                               const int32_t* __restrict__ dst_scan, CsmGeom g,
                                                               uint8_t* __restrict__ tables, int32_t value) {
    const int b = blockIdx.x;
    const int s = dst_scan[b];
    uint8_t* L = tables + static_cast<int64_t>(b) * g.tbl;
    const int32_t G = g.G;
    for (int64_t j = scan_off[s] + threadIdx.x; j < scan_off[s + 1]; j += kCsmBlock) {
        const double2 p = pts[j];
        // cells below -1 or above G mark nothing inside the grid
        const int32_t cx = csm_cell(p.x, g.o, g.res, -2.0, G + 1.0);
        const int32_t cy = csm_cell(p.y, g.o, g.res, -2.0, G + 1.0);
        if (value == 2) {
            if (cx >= 0 && cx < G && cy >= 0 && cy < G) L[(cy + g.py) * g.wp + cx + g.px] = 2;
        } else {
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t x = cx + dx, y = cy + dy;
                    if (x >= 0 && x < G && y >= 0 && y < G) L[(y + g.py) * g.wp + x + g.px] = 1;
                }
        }
    }
}

__device__ __forceinline__ unsigned long long csm_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor(static_cast<unsigned>(v), off, 64);
        const unsigned hi = __shfl_xor(static_cast<unsigned>(v >> 32), off, 64);
        const unsigned long long w = (static_cast<unsigned long long>(hi) << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// One workgroup per (pair b, angle k).  A thread owns R slots per pass, a slot
// being W shifts with adjacent i of one window row: W = 1 gathers one table
// byte per slot and point; W = 4 gathers the 4 adjacent bytes as one (unaligned)
// dword and adds them as packed 16-bit pairs, widened to int32 after every LDS
// tile (4,096 points x 2 < 2^16).  Cells of a slot past the window's last
// column are read (the border is 4 columns wider on the right) and dropped.
template <int R, int W>
__global__ __launch_bounds__(kCsmBlock) void csm_score_kernel(
    const double2* __restrict__ pts, const int64_t* __restrict__ scan_off, const int32_t* __restrict__ src_scan,
    const double* __restrict__ centre, const double* __restrict__ rot, int32_t n_theta, int32_t nx, int32_t ny,
    CsmGeom g, const uint8_t* __restrict__ tables, unsigned long long* __restrict__ keys,
    int32_t* __restrict__ out_scores) {
    static_assert(W == 1 || W == 4, "slot width");
    __shared__ int32_t cell[kCsmTile];
    __shared__ unsigned long long red[kCsmBlock / 64];
    const int b = blockIdx.x / n_theta;
    const int k = blockIdx.x - b * n_theta;
    const int tid = threadIdx.x;
    const int s = src_scan[b];
    const int64_t q0 = scan_off[s];
    const int64_t n = scan_off[s + 1] - q0;
    const double c = rot[2 * (static_cast<int64_t>(b) * n_theta + k)];
    const double sn = rot[2 * (static_cast<int64_t>(b) * n_theta + k) + 1];
    const double tx0 = centre[3 * b + 1], ty0 = centre[3 * b + 2];
    const uint8_t* __restrict__ L = tables + static_cast<int64_t>(b) * g.tbl;
    const int32_t nshift = nx * ny;
    const int32_t row_slots = (nx + W - 1) / W, nslot = ny * row_slots;
    const int32_t hx = nx / 2, hy = ny / 2;
    // the cells from which every shift stays inside the bordered table; a cell
    // clamped to either end has all its shifts in the border (outside the grid)
    const double xlo = hx - g.px, xhi = (g.G - 1 + g.px) - (nx - 1 - hx);
    const double ylo = hy - g.py, yhi = (g.G - 1 + g.py) - (ny - 1 - hy);
    unsigned long long best = 0;

    for (int32_t s0 = 0; s0 < nslot; s0 += kCsmBlock * R) {
        int32_t off[R], acc[R][W];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int32_t u = s0 + r * kCsmBlock + tid;
            const int32_t j = u / row_slots, i = W * (u - j * row_slots);
            off[r] = u < nslot ? (j - hy) * g.wp + (i - hx) : 0;   // an idle slot re-reads the cell itself
#pragma unroll
            for (int t = 0; t < W; ++t) acc[r][t] = 0;
        }
        for (int64_t t0 = 0; t0 < n; t0 += kCsmTile) {
            const int32_t m = static_cast<int32_t>(n - t0 < kCsmTile ? n - t0 : kCsmTile);
            __syncthreads();
            for (int32_t p = tid; p < m; p += kCsmBlock) {
                const double2 q = pts[q0 + t0 + p];
                const double X = (c * q.x - sn * q.y) + tx0;
                const double Y = (sn * q.x + c * q.y) + ty0;
                const int32_t ix = csm_cell(X, g.o, g.res, xlo, xhi);
                const int32_t iy = csm_cell(Y, g.o, g.res, ylo, yhi);
                cell[p] = (iy + g.py) * g.wp + ix + g.px;
            }
            __syncthreads();
            if constexpr (W == 1) {
#pragma unroll 2
                for (int32_t p = 0; p < m; ++p) {
                    const int32_t base = cell[p];
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][0] += L[static_cast<uint32_t>(base + off[r])];
                }
            } else {
                uint32_t even[R], odd[R];   // cells i, i + 2 and i + 1, i + 3 as 16-bit pairs
#pragma unroll
                for (int r = 0; r < R; ++r) even[r] = odd[r] = 0;
#pragma unroll 2
                for (int32_t p = 0; p < m; ++p) {
                    const int32_t base = cell[p];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        uint32_t w;
                        __builtin_memcpy(&w, L + static_cast<uint32_t>(base + off[r]), 4);
                        even[r] += w & 0x00ff00ffu;
                        odd[r] += (w >> 8) & 0x00ff00ffu;
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    acc[r][0] += even[r] & 0xffffu;
                    acc[r][1] += odd[r] & 0xffffu;
                    acc[r][2] += even[r] >> 16;
                    acc[r][3] += odd[r] >> 16;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int32_t u = s0 + r * kCsmBlock + tid;
            const int32_t j = u / row_slots, i0 = W * (u - j * row_slots);
#pragma unroll
            for (int t = 0; t < W; ++t) {
                if (u < nslot && i0 + t < nx) {
                    const int64_t flat = static_cast<int64_t>(k) * nshift + j * nx + i0 + t;   // < 2^31 (host check)
                    if (out_scores) out_scores[static_cast<int64_t>(b) * n_theta * nshift + flat] = acc[r][t];
                    const unsigned long long key =
                        (static_cast<unsigned long long>(static_cast<uint32_t>(acc[r][t])) << 32) |
                        (0xffffffffu - static_cast<uint32_t>(flat));
                    best = key > best ? key : best;
                }
            }
        }
    }
    best = csm_wave_max(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kCsmBlock / 64; ++w) best = red[w] > best ? red[w] : best;
        atomicMax(&keys[b], best);
    }
}

__global__ void csm_best_kernel(const unsigned long long* __restrict__ keys, int32_t B, int32_t nx, int32_t ny,
                                int32_t* __restrict__ out_best) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long key = keys[b];
    const int32_t flat = static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(key));
    const int32_t nshift = nx * ny;
    const int32_t k = flat / nshift, rem = flat - k * nshift;
    out_best[4 * b] = static_cast<int32_t>(key >> 32);
    out_best[4 * b + 1] = k;
    out_best[4 * b + 2] = rem / nx;
    out_best[4 * b + 3] = rem % nx;
}

using CsmScoreFn = void (*)(const double2*, const int64_t*, const int32_t*, const double*, const double*, int32_t,
                            int32_t, int32_t, CsmGeom, const uint8_t*, unsigned long long*, int32_t*);

template <int W, int... I>
static CsmScoreFn csm_score_instance(int r, std::integer_sequence<int, I...>) {
    static const CsmScoreFn table[] = {csm_score_kernel<I + 1, W>...};
    return table[r - 1];
}

// Gather width of the score kernel on this host thread (slam_csm_set_gather).
inline int& csm_gather_width() {
    static thread_local int w = 4;
    return w;
}

// Validates the shape and fills the table geometry; 0 or SLAM_EINVAL.
static int csm_shape(int32_t B, double res, int32_t G, int32_t n_theta, int32_t ny, int32_t nx, CsmGeom* g,
                     int64_t* key_bytes) {
    if (B <= 0) return fail(SLAM_EINVAL, "csm: B = %d <= 0", B);
    if (G <= 0 || (G & 1)) return fail(SLAM_EINVAL, "csm: G = %d must be positive and even", G);
    if (!(res > 0.0) || !std::isfinite(res)) return fail(SLAM_EINVAL, "csm: res must be a positive finite number");
    if (n_theta <= 0 || nx <= 0 || ny <= 0)
        return fail(SLAM_EINVAL, "csm: n_theta = %d, nx = %d, ny = %d must be positive", n_theta, nx, ny);
    const int64_t volume = static_cast<int64_t>(n_theta) * ny * nx;
    if (static_cast<int64_t>(ny) * nx > (1ll << 30) || volume >= (1ll << 31))
        return fail(SLAM_EINVAL, "csm: score volume of %d x %d x %d entries does not fit 31 bits", n_theta, ny, nx);
    if (static_cast<int64_t>(B) * n_theta >= (1ll << 31))
        return fail(SLAM_EINVAL, "csm: %d pairs x %d angles exceed the launch grid", B, n_theta);
    const int64_t wp = static_cast<int64_t>(G) + 2 * static_cast<int64_t>(nx) + 4;   // + 4: the dword gathers' overhang
    const int64_t hp = static_cast<int64_t>(G) + 2 * static_cast<int64_t>(ny);
    if (wp * hp >= (1ll << 31))
        return fail(SLAM_EINVAL, "csm: bordered table of %lld x %lld cells does not fit 31 bits",
                    static_cast<long long>(hp), static_cast<long long>(wp));
    g->G = G;
    g->px = nx;
    g->py = ny;
    g->wp = static_cast<int32_t>(wp);
    g->tbl = (wp * hp + 255) / 256 * 256;
    g->res = res;
    g->o = -static_cast<double>(G / 2) * res;
    *key_bytes = (8 * static_cast<int64_t>(B) + 255) / 256 * 256;
    return SLAM_OK;
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int64_t slam_csm_work_size(int32_t B, int32_t G, int32_t n_theta, int32_t ny, int32_t nx) {
    // bytes: best keys (u64 / pair) | bordered tables ((G + 2 ny) x (G + 2 nx + 4) bytes / pair)
    CsmGeom g;
    int64_t key_bytes;
    if (csm_shape(B, 1.0, G, n_theta, ny, nx, &g, &key_bytes) != SLAM_OK) return SLAM_EINVAL;
    ok();
    return key_bytes + static_cast<int64_t>(B) * g.tbl;
}

int slam_csm_batch(const double* pts, const int64_t* scan_off, const int32_t* src_scan, const int32_t* dst_scan,
                   const double* centre, const double* rot, int32_t B, double res, int32_t G, int32_t n_theta,
                   int32_t nx, int32_t ny, int32_t* out_best, int32_t* out_scores, void* work, void* stream) {
    if (!pts || !scan_off || !src_scan || !dst_scan || !centre || !rot || !out_best || !work)
        return fail(SLAM_EINVAL, "csm: null array");
    CsmGeom g;
    int64_t key_bytes;
    if (csm_shape(B, res, G, n_theta, ny, nx, &g, &key_bytes) != SLAM_OK) return SLAM_EINVAL;
    hipStream_t st = as_stream(stream);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(work);
    uint8_t* tables = reinterpret_cast<uint8_t*>(work) + key_bytes;
    const hipError_t e = hipMemsetAsync(work, 0, static_cast<size_t>(key_bytes + static_cast<int64_t>(B) * g.tbl), st);
    if (e != hipSuccess) return fail(SLAM_EHIP, "csm workspace clear: %s", hipGetErrorString(e));
    const double2* p2 = reinterpret_cast<const double2*>(pts);
    for (int32_t value = 1; value <= 2; ++value)
        hipLaunchKernelGGL(csm_raster_kernel, dim3(B), dim3(kCsmBlock), 0, st, p2, scan_off, dst_scan, g, tables,
                           value);
    // passes of at most kCsmBlock * max_r slots (1 or 4 shifts each), the slots spread evenly over them
    const int W = csm_gather_width();
    const int max_r = W == 4 ? kCsmMaxR4 : kCsmMaxR;
    const int64_t nslot = static_cast<int64_t>(ny) * ((nx + W - 1) / W);
    const int64_t passes = (nslot + kCsmBlock * max_r - 1) / (kCsmBlock * max_r);
    const int R = static_cast<int>((nslot + kCsmBlock * passes - 1) / (kCsmBlock * passes));
    const CsmScoreFn score = W == 4 ? csm_score_instance<4>(R, std::make_integer_sequence<int, kCsmMaxR4>())
                                    : csm_score_instance<1>(R, std::make_integer_sequence<int, kCsmMaxR>());
    hipLaunchKernelGGL(score, dim3(static_cast<unsigned>(B) * static_cast<unsigned>(n_theta)), dim3(kCsmBlock), 0, st,
                       p2, scan_off, src_scan, centre, rot, n_theta, nx, ny, g, tables, keys, out_scores);
    hipLaunchKernelGGL(csm_best_kernel, dim3((B + 255) / 256), dim3(256), 0, st, keys, B, nx, ny, out_best);
    return check_launch("csm kernels");
}

int slam_csm_set_gather(int width) {
    if (width != 1 && width != 4) return fail(SLAM_EINVAL, "csm: gather width %d (1 or 4)", width);
    csm_gather_width() = width;
    return ok();
}

}  // extern "C"
