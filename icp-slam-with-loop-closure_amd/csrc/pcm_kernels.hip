// pcm_kernels.hip — loop-closure verification by pairwise consistency for gfx950
// (MI355X).  include/slamhip.h states the rule; tests/pcm_ref.py restates it.
//
// pcm_prepare_kernel: one thread per closure l = (a, b, Z): V = X[a], D = (V Z)
// inv(X[b]), Di = inv(D), U = inv(V) D, twelve doubles stored as twelve arrays of
// L in `work`.  An index outside [0, N) raises the status flag and its closure
// gets NaNs: it is never read through and every comparison with it is false.
//
// pcm_pair_kernel: a 256-thread workgroup per tile of 256 columns and 256 rows.
// Lane = column m with its twelve doubles and (a, b) in registers; the row l is
// wave-uniform (scalar loads).  Every thread evaluates the canonical pair
// (min(l, m), max(l, m)): E = (U_lo Di_hi) V_lo, so bit (l, m) and bit (m, l) come
// from the same arithmetic and both triangles are written without atomics.  The
// wave's 64 verdicts are one __ballot and one 8-byte store per row (4 bytes
// where the row's last word is the wave's first).
//
// pcm_degree_kernel: one wave per row sums the popcounts of its words.
//
// pcm_peel_kernel<K>: ONE workgroup of 1,024 threads.  Thread t owns closures
// t + 1024 k, k < K, as packed keys degree << 16 | (65535 - index) in REGISTERS
// and an alive mask of K bits: no LDS array and no global scratch is sized by L.
// A step is a block minimum of the alive keys (DPP wave minimum, one LDS slot per
// wave, one barrier), then the removed closure's bit row: a wave's slot k lies in
// two words of it, lane k loads that pair (two loads a thread, whatever K is) and
// v_readlane hands it to the wave, which decrements.  Only integers decide
// anything.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kPcmBlock = 256;        // pair kernel: columns per workgroup (the column tile)
constexpr int kPcmRows = 256;         // pair kernel: rows per workgroup
constexpr int kPcmPeelBlock = 1024;   // peel kernel: its one workgroup
constexpr int kPcmMaxSlots = 64;      // closures per peel thread at most
constexpr int kPcmMaxL = kPcmPeelBlock * kPcmMaxSlots;   // 65,536: index and degree fit 16 bits
constexpr int kPcmBadIndex = 1;

static thread_local int t_pcm_slots = 0;   // slam_pcm_set_peel_slots
__device__ int g_pcm_status;               // kPcmBadIndex of the launches since slam_pcm_status

struct Rigid {   // an SE(2) element (c, s, x, y)
    double c, s, x, y;
};

__device__ __forceinline__ Rigid pcm_mul(const Rigid& A, const Rigid& B) {
    Rigid r;
    r.c = (A.c * B.c) - (A.s * B.s);
    r.s = (A.s * B.c) + (A.c * B.s);
    r.x = ((A.c * B.x) - (A.s * B.y)) + A.x;
    r.y = ((A.s * B.x) + (A.c * B.y)) + A.y;
    return r;
}

__device__ __forceinline__ Rigid pcm_inv(const Rigid& A) {
    Rigid r;
    r.c = A.c;
    r.s = -A.s;
    r.x = -((A.c * A.x) + (A.s * A.y));
    r.y = (A.s * A.x) - (A.c * A.y);
    return r;
}

__device__ __forceinline__ Rigid pcm_load(const double* __restrict__ p, int64_t stride, int64_t i) {
    Rigid r;
    r.c = p[i];
    r.s = p[stride + i];
    r.x = p[2 * stride + i];
    r.y = p[3 * stride + i];
    return r;
}

__device__ __forceinline__ void pcm_store(double* __restrict__ p, int64_t stride, int64_t i, const Rigid& r) {
    p[i] = r.c;
    p[stride + i] = r.s;
    p[2 * stride + i] = r.x;
    p[3 * stride + i] = r.y;
}

__device__ __forceinline__ Rigid pcm_pick(bool first, const Rigid& p, const Rigid& q) {
    Rigid r;
    r.c = first ? p.c : q.c;
    r.s = first ? p.s : q.s;
    r.x = first ? p.x : q.x;
    r.y = first ? p.y : q.y;
    return r;
}

__global__ __launch_bounds__(kPcmBlock) void pcm_prepare_kernel(const double* __restrict__ X, int32_t N,
                                                                const int32_t* __restrict__ a,
                                                                const int32_t* __restrict__ b,
                                                                const double* __restrict__ Z, int32_t L,
                                                                double* __restrict__ work) {
    const int64_t l = static_cast<int64_t>(blockIdx.x) * kPcmBlock + threadIdx.x;
    if (l >= L) return;
    const int32_t ia = a[l], ib = b[l];
    Rigid V, U, Di;
    if (ia < 0 || ia >= N || ib < 0 || ib >= N) {   // flagged, and never an index outside
        atomicOr(&g_pcm_status, kPcmBadIndex);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        V.c = V.s = V.x = V.y = nan;
        U = V;
        Di = V;
    } else {
        V = pcm_load(X + 4 * static_cast<int64_t>(ia), 1, 0);
        const Rigid Xb = pcm_load(X + 4 * static_cast<int64_t>(ib), 1, 0);
        const Rigid Zl = pcm_load(Z + 4 * l, 1, 0);
        const Rigid D = pcm_mul(pcm_mul(V, Zl), pcm_inv(Xb));
        Di = pcm_inv(D);
        U = pcm_mul(pcm_inv(V), D);
    }
    pcm_store(work, L, l, V);
    pcm_store(work + 4 * static_cast<int64_t>(L), L, l, U);
    pcm_store(work + 8 * static_cast<int64_t>(L), L, l, Di);
}

struct __attribute__((packed, aligned(4))) PcmWordPair {   // two words of a bit row: 4-byte aligned where W is odd
    uint32_t lo, hi;
};

__global__ __launch_bounds__(kPcmBlock) void pcm_pair_kernel(const double* __restrict__ work,
                                                             const int32_t* __restrict__ a,
                                                             const int32_t* __restrict__ b, int32_t L, int32_t W,
                                                             double tt0, double ttd, double tr0, double trd,
                                                             uint32_t* __restrict__ adj) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int32_t m0 = static_cast<int32_t>(blockIdx.x) * kPcmBlock + wave * 64;   // the wave's first column
    if (m0 >= L) return;   // the whole wave: no barrier below
    const int32_t m = m0 + lane;
    const int64_t mc = min(m, L - 1);   // a lane past the end repeats the last column, its verdict is dropped
    const double* Vp = work;
    const double* Up = work + 4 * static_cast<int64_t>(L);
    const double* Dp = work + 8 * static_cast<int64_t>(L);
    const Rigid Vm = pcm_load(Vp, L, mc), Um = pcm_load(Up, L, mc), Dm = pcm_load(Dp, L, mc);
    const int64_t am = a[mc], bm = b[mc];
    const double bt0 = tt0 * tt0, btd = ttd * ttd, br0 = tr0 * tr0, brd = trd * trd;
    const int32_t w0 = m0 >> 5;              // < W
    const bool two = w0 + 1 < W;
    const int32_t l0 = static_cast<int32_t>(blockIdx.y) * kPcmRows;
    const int32_t l1 = min(L, l0 + kPcmRows);
    for (int32_t l = l0; l < l1; ++l) {   // wave-uniform
        const Rigid Vl = pcm_load(Vp, L, l), Ul = pcm_load(Up, L, l), Dl = pcm_load(Dp, L, l);
        const int64_t al = a[l], bl = b[l];
        const bool lo = l < m;   // the pair is (l, m), else (m, l)
        const Rigid A = pcm_pick(lo, Ul, Um), B = pcm_pick(lo, Dm, Dl), C = pcm_pick(lo, Vl, Vm);
        const Rigid E = pcm_mul(pcm_mul(A, B), C);
        const int64_t da = al - am, db = bl - bm;
        const double n = static_cast<double>((da < 0 ? -da : da) + (db < 0 ? -db : db));
        const double dt = (E.x * E.x) + (E.y * E.y);
        const double omc = 1.0 - E.c;
        const double dr = (E.s * E.s) + (omc * omc);
        const bool ok = m < L && m != l && dt <= bt0 + (btd * n) && dr <= br0 + (brd * n);
        const unsigned long long bits = __ballot(ok);
        if (lane == 0) {
            uint32_t* row = adj + static_cast<int64_t>(l) * W + w0;
            if (two) {
                PcmWordPair p;
                p.lo = static_cast<uint32_t>(bits);
                p.hi = static_cast<uint32_t>(bits >> 32);
                *reinterpret_cast<PcmWordPair*>(row) = p;
            } else {
                *row = static_cast<uint32_t>(bits);
            }
        }
    }
}

__global__ __launch_bounds__(kPcmBlock) void pcm_degree_kernel(const uint32_t* __restrict__ adj, int32_t L, int32_t W,
                                                               int32_t* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int64_t l = static_cast<int64_t>(blockIdx.x) * (kPcmBlock / 64) + (threadIdx.x >> 6);
    if (l >= L) return;   // the whole wave
    const uint32_t* row = adj + l * W;
    uint32_t c = 0;
    for (int32_t w = lane; w < W; w += 64) c = bcnt(row[w], c);
    for (int off = 32; off; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) deg[l] = static_cast<int32_t>(c);
}

// Minimum over the wave's 64 lanes, wave-uniform.  Every lane is active.
__device__ __forceinline__ uint32_t pcm_wave_min(uint32_t v) {
    int x = static_cast<int>(v);
    x = static_cast<int>(min(static_cast<uint32_t>(x), static_cast<uint32_t>(SLAM_DPPI(x, 0xB1))));    // quad_perm [1,0,3,2]
    x = static_cast<int>(min(static_cast<uint32_t>(x), static_cast<uint32_t>(SLAM_DPPI(x, 0x4E))));    // quad_perm [2,3,0,1]
    x = static_cast<int>(min(static_cast<uint32_t>(x), static_cast<uint32_t>(SLAM_DPPI(x, 0x124))));   // row_ror:4
    x = static_cast<int>(min(static_cast<uint32_t>(x), static_cast<uint32_t>(SLAM_DPPI(x, 0x128))));   // row_ror:8
    const uint32_t a = static_cast<uint32_t>(__builtin_amdgcn_readlane(x, 0));
    const uint32_t b = static_cast<uint32_t>(__builtin_amdgcn_readlane(x, 16));
    const uint32_t c = static_cast<uint32_t>(__builtin_amdgcn_readlane(x, 32));
    const uint32_t d = static_cast<uint32_t>(__builtin_amdgcn_readlane(x, 48));
    return min(min(a, b), min(c, d));
}

template <int K>
__global__ __launch_bounds__(kPcmPeelBlock) void pcm_peel_kernel(const uint32_t* __restrict__ adj,
                                                                 const int32_t* __restrict__ deg, int32_t L,
                                                                 int32_t W, int32_t min_size,
                                                                 int32_t* __restrict__ out_order,
                                                                 uint8_t* __restrict__ out_keep,
                                                                 int32_t* __restrict__ out_steps) {
    constexpr int kWaves = kPcmPeelBlock / 64;
    __shared__ uint32_t slot[2][kWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    uint32_t key[K];               // closure tid + 1024 k: degree << 16 | (65535 - index)
    unsigned long long live = 0;   // bit k: that closure is alive
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int32_t m = tid + kPcmPeelBlock * k;
        key[k] = 0xFFFFFFFFu;
        if (m < L) {
            key[k] = (static_cast<uint32_t>(deg[m]) << 16) | static_cast<uint32_t>(65535 - m);
            live |= 1ull << k;
        }
    }
    int32_t alive = L, step = 0;
    int par = 0;
    while (alive > 1) {
        uint32_t best = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < K; ++k)   // a dead slot counts as all ones, without a condition register per slot
            best = min(best, key[k] | ((static_cast<uint32_t>(live >> k) & 1u) - 1u));
        best = pcm_wave_min(best);
        if (lane == 0) slot[par][wave] = best;
        __syncthreads();   // the only barrier of a step: the slots alternate
        best = pcm_wave_min(slot[par][lane & (kWaves - 1)]);
        par ^= 1;
        const int32_t d = static_cast<int32_t>(best >> 16);
        const int32_t r = 65535 - static_cast<int32_t>(best & 0xFFFFu);   // < L: taken from an alive key
        if (d == alive - 1) break;   // lowest degree, highest index; a clique when it touches everyone alive
        if ((r & (kPcmPeelBlock - 1)) == tid) {
            live &= ~(1ull << (r >> 10));
            out_order[r] = step;
        }
        // Slot k of this wave's lanes lies in words 2 wave + 32 k (lanes 0-31) and the next one (lanes 32-63) of
        // row r: lane k loads slot k's pair, two loads a thread whatever K is, and a v_readlane hands them out.
        const uint32_t* row = adj + static_cast<int64_t>(r) * W;
        const int32_t wi = 2 * wave + 32 * lane;
        const uint32_t lo = lane < K && wi < W ? row[wi] : 0u;
        const uint32_t hi = lane < K && wi + 1 < W ? row[wi + 1] : 0u;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t wl = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lo), k));
            const uint32_t wh = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hi), k));
            const uint32_t w = lane & 32 ? wh : wl;
            key[k] -= ((w >> (lane & 31)) & static_cast<uint32_t>(live >> k) & 1u) << 16;
        }
        --alive;
        ++step;
    }
    const bool kept = alive >= min_size;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int32_t m = tid + kPcmPeelBlock * k;
        if (m < L) {
            const bool on = (live >> k) & 1ull;
            if (on) out_order[m] = -1;
            out_keep[m] = on && kept ? 1 : 0;
        }
    }
    if (tid == 0) *out_steps = step;
}

static int pcm_check_L(int32_t L) {
    if (L < 0) return fail(SLAM_EINVAL, "pcm: L = %d < 0", L);
    if (L > kPcmMaxL) return fail(SLAM_ETOOBIG, "pcm: L = %d closures, above %d", L, kPcmMaxL);
    return SLAM_OK;
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int64_t slam_pcm_work_size(int32_t L) {
    // bytes: V, U, Di of every closure as twelve arrays of L doubles
    if (const int rc = pcm_check_L(L)) return rc;
    ok();
    return (static_cast<int64_t>(L) * 96 + 255) / 256 * 256;
}

int slam_pcm_adjacency_f64(const double* X, int32_t N, const int32_t* a, const int32_t* b, const double* Z, int32_t L,
                           double trans_tol, double trans_drift, double rot_tol, double rot_drift, uint32_t* out_adj,
                           int32_t* out_deg, void* work, void* stream) {
    if (!X || !a || !b || !Z || !out_adj || !out_deg || !work) return fail(SLAM_EINVAL, "pcm: null array");
    if (N <= 0) return fail(SLAM_EINVAL, "pcm: N = %d <= 0", N);
    if (const int rc = pcm_check_L(L)) return rc;
    if (!(trans_tol >= 0 && trans_drift >= 0 && rot_tol >= 0 && rot_drift >= 0))
        return fail(SLAM_EINVAL, "pcm: a negative (or NaN) tolerance");
    if (reinterpret_cast<uintptr_t>(work) % 8) return fail(SLAM_EINVAL, "pcm: work not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out_adj) % 4) return fail(SLAM_EINVAL, "pcm: adjacency not 4-byte aligned");
    if (L == 0) return ok();
    hipStream_t st = as_stream(stream);
    const int32_t W = (L + 31) / 32;
    const unsigned tiles = static_cast<unsigned>((L + kPcmBlock - 1) / kPcmBlock);
    double* wk = static_cast<double*>(work);
    hipLaunchKernelGGL(pcm_prepare_kernel, dim3(tiles), dim3(kPcmBlock), 0, st, X, N, a, b, Z, L, wk);
    hipLaunchKernelGGL(pcm_pair_kernel, dim3(tiles, static_cast<unsigned>((L + kPcmRows - 1) / kPcmRows)),
                       dim3(kPcmBlock), 0, st, wk, a, b, L, W, trans_tol, trans_drift, rot_tol, rot_drift, out_adj);
    hipLaunchKernelGGL(pcm_degree_kernel, dim3(static_cast<unsigned>((L + kPcmBlock / 64 - 1) / (kPcmBlock / 64))),
                       dim3(kPcmBlock), 0, st, out_adj, L, W, out_deg);
    return check_launch("pcm adjacency kernels");
}

int slam_pcm_select(const uint32_t* adj, const int32_t* deg, int32_t L, int32_t min_size, int32_t* out_order,
                    uint8_t* out_keep, int32_t* out_steps, void* stream) {
    if (!adj || !deg || !out_order || !out_keep || !out_steps) return fail(SLAM_EINVAL, "pcm: null array");
    if (const int rc = pcm_check_L(L)) return rc;
    if (min_size < 0) return fail(SLAM_EINVAL, "pcm: min_size = %d < 0", min_size);
    int slots = 1;
    while (slots * kPcmPeelBlock < L) slots *= 4;
    if (t_pcm_slots > slots) slots = t_pcm_slots;
    if (L == 0) return ok();
    hipStream_t st = as_stream(stream);
    const int32_t W = (L + 31) / 32;
#define SLAM_PCM_PEEL(k)                                                                                        \
    hipLaunchKernelGGL(pcm_peel_kernel<k>, dim3(1), dim3(kPcmPeelBlock), 0, st, adj, deg, L, W, min_size, out_order, \
                       out_keep, out_steps)
    switch (slots) {
        case 1: SLAM_PCM_PEEL(1); break;
        case 4: SLAM_PCM_PEEL(4); break;
        case 16: SLAM_PCM_PEEL(16); break;
        default: SLAM_PCM_PEEL(64); break;
    }
#undef SLAM_PCM_PEEL
    return check_launch("pcm peel kernel");
}

int slam_pcm_set_peel_slots(int slots) {
    if (slots != 0 && slots != 1 && slots != 4 && slots != 16 && slots != 64)
        return fail(SLAM_EINVAL, "pcm: peel slots %d (0 automatic, 1, 4, 16 or 64)", slots);
    t_pcm_slots = slots;
    return ok();
}

int slam_pcm_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "pcm status: stream sync");
    int st = 0;
    if (hipMemcpyFromSymbol(&st, HIP_SYMBOL(g_pcm_status), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "pcm status: read");
    if (st == 0) return ok();
    const int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pcm_status), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "pcm status: clear");
    return fail(SLAM_EINVAL, "pcm: a closure index outside [0, N)");
}

}  // extern "C"
