// lcd_kernels.hip — proximity loop-closure candidates for gfx950 (MI355X).
//
// The candidate search of the reference's detect_proximity
// (src/loop_closure_detection.py:12-24): for every pose i the nearest pose j
// among those at least min_dist_along_path further along the path, i.e.
//     start[i] + np.argmin(cdist(xy, xy)[i, start[i]:])
// The reference (and the drop-in's host path) builds the whole N x N fp64
// matrix for it, 20 GB at 50,000 poses; here the rows are scanned in
// registers and nothing quadratic in N is stored.
//
// Rule (include/slamhip.h states it): dx = x_i - x_j, dy = y_i - y_j,
// s = (dx dx) + (dy dy) with three roundings (no FMA contraction), d = sqrt(s)
// correctly rounded; the answer is the smallest j in [start[i], N) whose d is
// minimal.  Ties are ties of the ROUNDED square roots: two different s may
// round to one d, and then the earlier j wins although its s is larger.
//
// lcd_scan_kernel: workgroup (row block of 256 rows) x (column chunk).  A lane
// owns kLcdRows = 1 row (x, y, start and (best_s, best_d, best_j) in
// registers; two rows per lane, sharing each column read, measured 8 % slower:
// profiles/lcd_shape_ab.txt); the chunk's column (x, y) pairs pass through LDS
// in tiles of 1,024 and are read as broadcasts (every lane the same address).
// A column is screened on s: only when s drops below the lane's best_s is the
// square root taken, and best_j moves only when the
// rounded d drops too.  sqrt is monotonic, so a column with s >= best_s has
// d >= best_d and, coming later, cannot win; lowering best_s on a tie of d is
// safe for the same reason.  A workgroup whose chunk lies left of every start
// of its rows returns at once (the triangular half of the tiles), tiles left
// of them are skipped, and tiles right of every start of a wave's rows take
// the loop without the `j >= start` test.  Every row writes one (d, j) partial
// per chunk that holds one of its columns.
//
// lcd_merge_kernel: one lane per row takes the partials in chunk order, a
// later chunk winning only with a strictly smaller d: lexicographic on (d, j).
// No floating-point atomics, nothing depends on the launch shape.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kLcdBlock = 256;
constexpr int kLcdRows = 1;         // rows per lane
constexpr int kLcdTile = 1024;      // columns per LDS tile (16 KiB)
constexpr int kLcdBatch = 4;        // columns read from LDS ahead of their use (divides kLcdTile)
constexpr int kLcdMaxChunks = 16;   // partials per row: the workspace is linear in N

struct LcdBest {
    double s, d;
    int32_t j;
};

// Column j with s < b.s.
__device__ __forceinline__ void lcd_take(LcdBest& b, double s, int32_t j) {
    const double d = sqrt(s);   // correctly rounded (no fast-math in this build)
    if (d < b.d) {
        b.d = d;
        b.j = j;
    }
    b.s = s;
}

__device__ __forceinline__ int32_t lcd_start(const int32_t* __restrict__ start, int64_t i, int32_t N) {
    return min(max(start[i], 0), N - 1);   // the contract is 0 <= start < N; never index outside on a bad one
}

template <bool MASKED>
__device__ __forceinline__ void lcd_scan_tile(const double2* col, int32_t m, int32_t t0, const double (&x)[kLcdRows],
                                              const double (&y)[kLcdRows], const int32_t (&st)[kLcdRows],
                                              LcdBest (&best)[kLcdRows]) {
    // kLcdBatch columns are read before any is used: the rare branch into
    // lcd_take keeps the compiler from moving a read above it
    for (int32_t k = 0; k < m; k += kLcdBatch) {
        double2 p[kLcdBatch];
#pragma unroll
        for (int u = 0; u < kLcdBatch; ++u) p[u] = col[k + u];
#pragma unroll
        for (int u = 0; u < kLcdBatch; ++u) {
            const int32_t j = t0 + k + u;
#pragma unroll
            for (int r = 0; r < kLcdRows; ++r) {
                const double dx = x[r] - p[u].x, dy = y[r] - p[u].y;
                const double s = (dx * dx) + (dy * dy);   // NaN for the tile's padding: never below best_s
                if ((!MASKED || j >= st[r]) && s < best[r].s) lcd_take(best[r], s, j);
            }
        }
    }
}

__global__ __launch_bounds__(kLcdBlock) void lcd_scan_kernel(const double* __restrict__ poses, int32_t N,
                                                             const int32_t* __restrict__ start, int32_t n_rows,
                                                             int32_t chunk, double* __restrict__ part_d,
                                                             int32_t* __restrict__ part_j) {
    __shared__ double2 col[kLcdTile];
    __shared__ int32_t first;   // smallest start of the workgroup's rows
    const int tid = threadIdx.x;
    const int32_t c0 = static_cast<int32_t>(blockIdx.y) * chunk;   // < N
    const int32_t c1 = static_cast<int32_t>(min(static_cast<int64_t>(N), static_cast<int64_t>(c0) + chunk));
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * (kLcdBlock * kLcdRows) + tid;

    double x[kLcdRows], y[kLcdRows];
    int32_t st[kLcdRows];
    bool valid[kLcdRows];
    LcdBest best[kLcdRows];
    if (tid == 0) first = N;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kLcdRows; ++r) {
        const int64_t i = row0 + r * kLcdBlock;
        valid[r] = i < n_rows;
        // a row past the end computes against (0, 0) from column 0 and writes nothing
        st[r] = valid[r] ? lcd_start(start, i, N) : 0;
        x[r] = valid[r] ? poses[3 * i] : 0.0;
        y[r] = valid[r] ? poses[3 * i + 1] : 0.0;
        best[r].s = best[r].d = __builtin_huge_val();
        best[r].j = max(st[r], c0);   // all distances infinite: argmin's first column
        if (valid[r]) atomicMin(&first, st[r]);
    }
    __syncthreads();
    const int32_t lo = first;
    if (lo >= c1) return;   // the whole chunk lies left of every row's start (uniform)

    int32_t t0 = c0 + (max(lo, c0) - c0) / kLcdTile * kLcdTile;
    for (; t0 < c1; t0 += kLcdTile) {
        const int32_t m = min(kLcdTile, c1 - t0);
        __syncthreads();
        const int32_t m_pad = (m + kLcdBatch - 1) / kLcdBatch * kLcdBatch;   // <= kLcdTile
        for (int32_t k = tid; k < m_pad; k += kLcdBlock) {
            const int64_t j = static_cast<int64_t>(t0) + k;
            const double nan = __builtin_nan("");
            col[k] = k < m ? make_double2(poses[3 * j], poses[3 * j + 1]) : make_double2(nan, nan);
        }
        __syncthreads();
        bool open = true;
#pragma unroll
        for (int r = 0; r < kLcdRows; ++r) open = open && st[r] <= t0;
        if (__all(open))
            lcd_scan_tile<false>(col, m, t0, x, y, st, best);
        else
            lcd_scan_tile<true>(col, m, t0, x, y, st, best);
    }
#pragma unroll
    for (int r = 0; r < kLcdRows; ++r) {
        const int64_t i = row0 + r * kLcdBlock;
        if (valid[r] && st[r] < c1) {
            const int64_t at = static_cast<int64_t>(blockIdx.y) * N + i;
            part_d[at] = best[r].d;
            part_j[at] = best[r].j;
        }
    }
}

__global__ __launch_bounds__(kLcdBlock) void lcd_merge_kernel(const int32_t* __restrict__ start, int32_t n_rows,
                                                              int32_t N, int32_t chunk, int32_t n_chunks,
                                                              const double* __restrict__ part_d,
                                                              const int32_t* __restrict__ part_j,
                                                              int32_t* __restrict__ out_j, double* __restrict__ out_d) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kLcdBlock + threadIdx.x;
    if (i >= n_rows) return;
    int32_t c = lcd_start(start, i, N) / chunk;   // the first chunk the scan wrote for this row
    double d = part_d[static_cast<int64_t>(c) * N + i];
    int32_t j = part_j[static_cast<int64_t>(c) * N + i];
    for (++c; c < n_chunks; ++c) {
        const double dc = part_d[static_cast<int64_t>(c) * N + i];
        if (dc < d) {   // chunks ascend in j: an equal d keeps the earlier column
            d = dc;
            j = part_j[static_cast<int64_t>(c) * N + i];
        }
    }
    out_j[i] = j;
    out_d[i] = d;
}

// Column chunk: at most kLcdMaxChunks chunks of whole tiles.
static void lcd_shape(int32_t N, int32_t* chunk, int32_t* n_chunks) {
    const int64_t per = (static_cast<int64_t>(N) + kLcdMaxChunks - 1) / kLcdMaxChunks;
    const int64_t w = (per + kLcdTile - 1) / kLcdTile * kLcdTile;
    *chunk = static_cast<int32_t>(w);
    *n_chunks = static_cast<int32_t>((static_cast<int64_t>(N) + w - 1) / w);
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int64_t slam_lcd_work_size(int32_t N) {
    // bytes: partial d (f64 [n_chunks][N]) | partial j (i32 [n_chunks][N]), at most 16 x 12 bytes per pose
    if (N <= 0) return fail(SLAM_EINVAL, "lcd: N = %d <= 0", N);
    int32_t chunk, n_chunks;
    lcd_shape(N, &chunk, &n_chunks);
    ok();
    return (static_cast<int64_t>(n_chunks) * N * 12 + 255) / 256 * 256;
}

int slam_lcd_nearest_f64(const double* poses, int32_t N, const int32_t* start, int32_t n_rows, int32_t* out_j,
                         double* out_d, void* work, void* stream) {
    if (!poses || !start || !out_j || !out_d || !work) return fail(SLAM_EINVAL, "lcd: null array");
    if (N <= 0) return fail(SLAM_EINVAL, "lcd: N = %d <= 0", N);
    if (n_rows < 0 || n_rows > N) return fail(SLAM_EINVAL, "lcd: n_rows = %d outside [0, N = %d]", n_rows, N);
    if (n_rows == 0) return ok();
    int32_t chunk, n_chunks;
    lcd_shape(N, &chunk, &n_chunks);
    double* part_d = reinterpret_cast<double*>(work);
    int32_t* part_j = reinterpret_cast<int32_t*>(part_d + static_cast<int64_t>(n_chunks) * N);
    hipStream_t st = as_stream(stream);
    const unsigned row_blocks = static_cast<unsigned>((static_cast<int64_t>(n_rows) + kLcdBlock * kLcdRows - 1) /
                                                      (kLcdBlock * kLcdRows));
    hipLaunchKernelGGL(lcd_scan_kernel, dim3(row_blocks, static_cast<unsigned>(n_chunks)), dim3(kLcdBlock), 0, st,
                       poses, N, start, n_rows, chunk, part_d, part_j);
    hipLaunchKernelGGL(lcd_merge_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(n_rows) + kLcdBlock - 1) /
                                                                    kLcdBlock)),
                       dim3(kLcdBlock), 0, st, start, n_rows, N, chunk, n_chunks, part_d, part_j, out_j, out_d);
    return check_launch("lcd kernels");
}

}  // extern "C"
