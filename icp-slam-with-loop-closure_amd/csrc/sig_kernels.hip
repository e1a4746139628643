// sig_kernels.hip — rotation-invariant scan signatures for gfx950 (MI355X):
// loop-closure candidates from the scans themselves (no pose nearness, no
// camera).  include/slamhip.h states the rule; tests/sig_ref.py restates it.
//
// sig_build_kernel: one 256-thread workgroup per scan.  A point's ring is the
// count of ring edges at or below r2 = (x x) + (y y), minus one; its sector the
// first maximum of (c_s x) + (s_s y) over the S sector centres (no atan2; the
// host-made tables pass through LDS).  The bit goes into the scan's S masks
// with an integer LDS atomicOr; the ring counts and n are taken from the
// finished masks.  Order-free, no floating-point atomics.
//
// sig_scan_kernel: one WAVE per row i and column chunk, lanes = shifts.  Lane k
// keeps row i's masks rotated by its own shift in registers, rot[t] =
// sig_i[(t - k) mod S], so that d(i, j, k) = sum_t popcount(rot[t] ^ sig_j[t])
// reads column j's masks at wave-uniform addresses: scalar loads, one xor and
// one accumulating popcount per mask and lane, no LDS and no barrier in the
// loop.  Shifts 64..127 (S > 64) are a second pass over the same registers,
// rot[(t + S - 64) mod S].  Columns come in tiles of 64: each lane screens one
// column with the ring-count bound (8 four-byte sums of absolute differences),
// the survivors' ballot is walked bit by bit, a wave minimum of the key
// d << 8 | k gives (d_ij, k_ij), and a candidate is inserted into the row's
// sorted top-K list, one slot per lane, with a ballot and a lane shift.  Every
// (row, chunk) writes a partial list of K entries and a count.
//
// sig_merge_kernel: 16 lanes per row insert the partials in chunk order into
// the same sorted list: lexicographic on (d, j).  Only integers decide anything:
// the result does not depend on the launch shape or on the screen.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

#pragma clang fp contract(off)

namespace slamhip {

constexpr int kSigBlock = 256;
constexpr int kSigRings = 32;
constexpr int kSigMaxS = 128;
constexpr int kSigMaxK = 16;
constexpr int kSigTile = 64;          // columns per screen step: one per lane
constexpr int kSigMinChunk = 256;     // columns per chunk at least (whole tiles)
constexpr int kSigMaxChunks = 16;     // partials per row: the workspace is linear in N
constexpr int kSigBadStart = 1, kSigBadScan = 2;
constexpr unsigned long long kSigEmpty = ~0ull;

static thread_local int t_sig_screen = 1;   // slam_sig_set_screen
__device__ int g_sig_status;   // kSigBadStart | kSigBadScan of the launches since slam_sig_status

__global__ __launch_bounds__(kSigBlock) void sig_build_kernel(const double* __restrict__ pts,
                                                              const int64_t* __restrict__ scan_off, int64_t P,
                                                              const double* __restrict__ dirs,
                                                              const double* __restrict__ edges2, int32_t S,
                                                              uint32_t* __restrict__ sig, uint8_t* __restrict__ ring,
                                                              int32_t* __restrict__ n_out) {
    __shared__ double2 dir[kSigMaxS];
    __shared__ double edge[kSigRings + 1];
    __shared__ uint32_t mask[kSigMaxS];
    __shared__ uint32_t rcount[kSigRings];
    const int tid = threadIdx.x;
    const int64_t scan = blockIdx.x;
    if (tid < S) {
        dir[tid] = make_double2(dirs[2 * tid], dirs[2 * tid + 1]);
        mask[tid] = 0;
    }
    if (tid <= kSigRings) edge[tid] = edges2[tid];
    int64_t p0 = scan_off[scan], p1 = scan_off[scan + 1];
    if (p0 < 0 || p1 < p0 || p1 > P) {   // uniform: nothing is read through bad offsets, the signature stays empty
        if (tid == 0) atomicOr(&g_sig_status, kSigBadScan);
        p1 = p0 = 0;
    }
    __syncthreads();
    for (int64_t p = p0 + tid; p < p1; p += kSigBlock) {
        const double x = pts[2 * p], y = pts[2 * p + 1];
        const double r2 = (x * x) + (y * y);
        int r = -1;   // edges nondecreasing: the count of edges <= r2 is the ring's upper edge index
#pragma unroll
        for (int k = 0; k <= kSigRings; ++k) r += edge[k] <= r2 ? 1 : 0;
        if (r < 0 || r >= kSigRings) continue;   // outside every ring (or NaN)
        int best_s = 0;
        double best = (dir[0].x * x) + (dir[0].y * y);
        for (int s = 1; s < S; ++s) {
            const double v = (dir[s].x * x) + (dir[s].y * y);
            if (v > best) {   // the smallest s among equal maxima stays
                best = v;
                best_s = s;
            }
        }
        atomicOr(&mask[best_s], 1u << r);
    }
    __syncthreads();
    if (tid < S) sig[scan * S + tid] = mask[tid];
    if (tid < kSigRings) {
        uint32_t c = 0;
        for (int s = 0; s < S; ++s) c += (mask[s] >> tid) & 1u;
        rcount[tid] = c;
        ring[scan * kSigRings + tid] = static_cast<uint8_t>(c);   // c <= S <= 128
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t n = 0;
        for (int r = 0; r < kSigRings; ++r) n += rcount[r];
        n_out[scan] = static_cast<int32_t>(n);
    }
}

// Minimum over the wave's 64 lanes, wave-uniform.  Every lane is active.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
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

// A row's sorted list, slot l in lane l of a 16-lane group (key = d << 32 | j ascending, kSigEmpty when unused):
// entry (x, xk) goes to its place and the larger entries move up one lane, the last one out.  x is the same in
// all 16 lanes of a group and differs from every key held; inserting kSigEmpty changes nothing.  Every lane of
// the wave takes part.
__device__ __forceinline__ void sig_insert(unsigned long long& key, int32_t& kk, unsigned long long x, int32_t xk) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = __ballot(key < x);   // the list is sorted: a prefix of each group
    const int pos = __popcll((below >> (lane & 48)) & 0xffffull);
    const unsigned long long pkey = __shfl_up(key, 1, 16);
    const int32_t pk = __shfl_up(kk, 1, 16);
    const int l = lane & 15;
    if (l == pos) {
        key = x;
        kk = xk;
    } else if (l > pos) {
        key = pkey;
        kk = pk;
    }
}

__device__ __forceinline__ int32_t sig_start(const int32_t* __restrict__ start, int64_t i, int32_t N) {
    const int32_t st = start[i];
    if (st < 0 || st > N) {   // flagged, and never an index outside
        atomicOr(&g_sig_status, kSigBadStart);
        return N;
    }
    return st;
}

template <int S>
__global__ __launch_bounds__(kSigBlock) void sig_scan_kernel(const uint32_t* __restrict__ sig,
                                                             const uint8_t* __restrict__ ring,
                                                             const int32_t* __restrict__ n_bits, int32_t N,
                                                             const int32_t* __restrict__ start, int32_t n_rows,
                                                             int32_t num, int32_t den, int32_t K, int32_t screen,
                                                             int32_t chunk, unsigned long long* __restrict__ part_key,
                                                             int32_t* __restrict__ part_k,
                                                             int32_t* __restrict__ part_count) {
    constexpr int kPasses = (S + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (kSigBlock / 64) + wave;
    if (i >= n_rows) return;   // the whole wave: no barrier below
    const int32_t c0 = static_cast<int32_t>(blockIdx.y) * chunk;   // < N, a multiple of kSigTile
    const int32_t c1 = static_cast<int32_t>(min(static_cast<int64_t>(N), static_cast<int64_t>(c0) + chunk));
    const int32_t st = __builtin_amdgcn_readfirstlane(sig_start(start, i, N));

    unsigned long long key = kSigEmpty;   // lane l (mod 16): slot l of the row's list
    int32_t kk = -1;
    int32_t count = 0;
    if (st < c1) {
        // lane = shift: rot[t] = sig_i[(t - lane) mod S]
        uint32_t rot[S];
        const uint32_t* si = sig + i * S;
        const int back = (S - lane % S) % S;
#pragma unroll
        for (int t = 0; t < S; ++t) rot[t] = si[(t + back) % S];
        uint32_t ri[8];
        const uint32_t* rp = reinterpret_cast<const uint32_t*>(ring + i * kSigRings);
#pragma unroll
        for (int w = 0; w < 8; ++w) ri[w] = rp[w];
        const int64_t ni = n_bits[i];
        const int64_t lnum = num, lden = den;

        for (int32_t t0 = c0 + (max(st, c0) - c0) / kSigTile * kSigTile; t0 < c1; t0 += kSigTile) {
            // screen: lane = column
            const int32_t jl = t0 + lane;
            const bool in = jl >= st && jl < c1;
            const int32_t jc = in ? jl : static_cast<int32_t>(i);   // a lane outside reads the row itself
            const uint4* rq = reinterpret_cast<const uint4*>(ring + static_cast<int64_t>(jc) * kSigRings);
            const uint4 a = rq[0], b = rq[1];
            const int32_t nj = n_bits[jc];
            uint32_t lb = __builtin_amdgcn_sad_u8(ri[0], a.x, 0u);
            lb = __builtin_amdgcn_sad_u8(ri[1], a.y, lb);
            lb = __builtin_amdgcn_sad_u8(ri[2], a.z, lb);
            lb = __builtin_amdgcn_sad_u8(ri[3], a.w, lb);
            lb = __builtin_amdgcn_sad_u8(ri[4], b.x, lb);
            lb = __builtin_amdgcn_sad_u8(ri[5], b.y, lb);
            lb = __builtin_amdgcn_sad_u8(ri[6], b.z, lb);
            lb = __builtin_amdgcn_sad_u8(ri[7], b.w, lb);
            const bool pass = in && (!screen || static_cast<int64_t>(lb) * lden <= lnum * (ni + nj));
            unsigned long long todo = __ballot(pass);
            while (todo) {
                const int bit = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int32_t j = t0 + bit;
                const int64_t nij = ni + __builtin_amdgcn_readlane(nj, bit);
                const uint32_t* sj = sig + static_cast<int64_t>(j) * S;   // wave-uniform: scalar loads
                uint32_t dp[kPasses] = {};   // pass p: shift lane + 64 p; each mask of the column is read once
#pragma unroll
                for (int t = 0; t < S; ++t) {
                    const uint32_t m = sj[t];
#pragma unroll
                    for (int p = 0; p < kPasses; ++p) dp[p] = bcnt(rot[(t + S - 64 * p) % S] ^ m, dp[p]);
                }
                uint32_t best = 0xFFFFFFFFu;
#pragma unroll
                for (int p = 0; p < kPasses; ++p) {
                    const int k = lane + 64 * p;
                    best = min(best, k < S ? (dp[p] << 8) | static_cast<uint32_t>(k) : 0xFFFFFFFFu);
                }
                best = wave_min_u32(best);   // d <= 32 S = 4,096 and k < 128: 20 bits
                const int64_t d = best >> 8;
                if (d * lden <= lnum * nij) {   // uniform
                    ++count;
                    sig_insert(key, kk, (static_cast<unsigned long long>(d) << 32) | static_cast<uint32_t>(j),
                               static_cast<int32_t>(best & 255u));
                }
            }
        }
    }
    const int64_t at = static_cast<int64_t>(blockIdx.y) * N + i;
    if (lane < K) {
        part_key[at * K + lane] = key;
        part_k[at * K + lane] = kk;
    }
    if (lane == 0) part_count[at] = count;
}

__global__ __launch_bounds__(kSigBlock) void sig_merge_kernel(int32_t n_rows, int32_t N, int32_t K, int32_t n_chunks,
                                                              const unsigned long long* __restrict__ part_key,
                                                              const int32_t* __restrict__ part_k,
                                                              const int32_t* __restrict__ part_count,
                                                              int32_t* __restrict__ out_j, int32_t* __restrict__ out_d,
                                                              int32_t* __restrict__ out_k,
                                                              int32_t* __restrict__ out_count) {
    const int l = threadIdx.x & 15;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kSigBlock / 16) + (threadIdx.x >> 4);
    const int64_t i = min(row, static_cast<int64_t>(n_rows) - 1);   // a group past the end repeats the last row, writes nothing
    unsigned long long key = kSigEmpty;
    int32_t kk = -1;
    int32_t count = 0;
    for (int32_t c = 0; c < n_chunks; ++c) {   // chunks ascend in j, each list ascends in (d, j)
        const int64_t at = static_cast<int64_t>(c) * N + i;
        count += part_count[at];
        for (int32_t e = 0; e < K; ++e) sig_insert(key, kk, part_key[at * K + e], part_k[at * K + e]);
    }
    if (row >= n_rows) return;
    if (l < K) {
        const bool used = key != kSigEmpty;
        out_j[row * K + l] = used ? static_cast<int32_t>(key & 0xFFFFFFFFull) : -1;
        out_d[row * K + l] = used ? static_cast<int32_t>(key >> 32) : -1;
        out_k[row * K + l] = used ? kk : -1;
    }
    if (l == 0) out_count[row] = count;
}

// Column chunk: at most kSigMaxChunks chunks of whole tiles, kSigMinChunk columns at least.
static void sig_shape(int32_t N, int32_t* chunk, int32_t* n_chunks) {
    const int64_t per = (static_cast<int64_t>(N) + kSigMaxChunks - 1) / kSigMaxChunks;
    int64_t w = (per + kSigTile - 1) / kSigTile * kSigTile;
    if (w < kSigMinChunk) w = kSigMinChunk;
    *chunk = static_cast<int32_t>(w);
    *n_chunks = static_cast<int32_t>((static_cast<int64_t>(N) + w - 1) / w);
}

static bool sig_bad_S(int32_t S) { return S < 8 || S > kSigMaxS || S % 8; }

using SigScanFn = decltype(&sig_scan_kernel<64>);

static SigScanFn sig_scan_fn(int32_t S) {
    switch (S) {
#define SLAM_SIG_CASE(s) \
    case s:              \
        return sig_scan_kernel<s>;
        SLAM_SIG_CASE(8) SLAM_SIG_CASE(16) SLAM_SIG_CASE(24) SLAM_SIG_CASE(32) SLAM_SIG_CASE(40) SLAM_SIG_CASE(48)
        SLAM_SIG_CASE(56) SLAM_SIG_CASE(64) SLAM_SIG_CASE(72) SLAM_SIG_CASE(80) SLAM_SIG_CASE(88) SLAM_SIG_CASE(96)
        SLAM_SIG_CASE(104) SLAM_SIG_CASE(112) SLAM_SIG_CASE(120) SLAM_SIG_CASE(128)
#undef SLAM_SIG_CASE
    }
    return nullptr;
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_sig_build(const double* pts, const int64_t* scan_off, int32_t N, int64_t P, const double* dirs,
                   const double* edges2, int32_t S, uint32_t* sig, uint8_t* ring, int32_t* n_bits, void* stream) {
    if (!pts || !scan_off || !dirs || !edges2 || !sig || !ring || !n_bits) return fail(SLAM_EINVAL, "sig: null array");
    if (N < 0) return fail(SLAM_EINVAL, "sig: N = %d < 0", N);
    if (P < 0) return fail(SLAM_EINVAL, "sig: P = %lld < 0", static_cast<long long>(P));
    if (sig_bad_S(S)) return fail(SLAM_EINVAL, "sig: S = %d (a multiple of 8 in 8..%d)", S, kSigMaxS);
    if (reinterpret_cast<uintptr_t>(ring) % 16) return fail(SLAM_EINVAL, "sig: ring counts not 16-byte aligned");
    if (N == 0) return ok();
    hipLaunchKernelGGL(sig_build_kernel, dim3(static_cast<unsigned>(N)), dim3(kSigBlock), 0, as_stream(stream), pts,
                       scan_off, P, dirs, edges2, S, sig, ring, n_bits);
    return check_launch("sig build kernel");
}

int64_t slam_sig_work_size(int32_t N, int32_t S, int32_t K) {
    // bytes per chunk and scan: K keys (u64) | K shifts (i32) | one count (i32); at most 16 x 196 per scan
    if (N <= 0) return fail(SLAM_EINVAL, "sig: N = %d <= 0", N);
    if (sig_bad_S(S)) return fail(SLAM_EINVAL, "sig: S = %d (a multiple of 8 in 8..%d)", S, kSigMaxS);
    if (K < 1 || K > kSigMaxK) return fail(SLAM_EINVAL, "sig: K = %d outside 1..%d", K, kSigMaxK);
    int32_t chunk, n_chunks;
    sig_shape(N, &chunk, &n_chunks);
    ok();
    return (static_cast<int64_t>(n_chunks) * N * (12 * K + 4) + 255) / 256 * 256;
}

int slam_sig_match(const uint32_t* sig, const uint8_t* ring, const int32_t* n_bits, int32_t N, int32_t S,
                   const int32_t* start, int32_t n_rows, int32_t num, int32_t den, int32_t K, int32_t* out_j,
                   int32_t* out_d, int32_t* out_k, int32_t* out_count, void* work, void* stream) {
    if (!sig || !ring || !n_bits || !start || !out_j || !out_d || !out_k || !out_count || !work)
        return fail(SLAM_EINVAL, "sig: null array");
    if (N <= 0) return fail(SLAM_EINVAL, "sig: N = %d <= 0", N);
    if (sig_bad_S(S)) return fail(SLAM_EINVAL, "sig: S = %d (a multiple of 8 in 8..%d)", S, kSigMaxS);
    if (K < 1 || K > kSigMaxK) return fail(SLAM_EINVAL, "sig: K = %d outside 1..%d", K, kSigMaxK);
    if (num < 0 || den < 1 || num > den)
        return fail(SLAM_EINVAL, "sig: threshold %d / %d (0 <= num <= den, den >= 1)", num, den);
    if (n_rows < 0 || n_rows > N) return fail(SLAM_EINVAL, "sig: n_rows = %d outside [0, N = %d]", n_rows, N);
    if (reinterpret_cast<uintptr_t>(ring) % 16) return fail(SLAM_EINVAL, "sig: ring counts not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(work) % 8) return fail(SLAM_EINVAL, "sig: work not 8-byte aligned");
    if (n_rows == 0) return ok();
    int32_t chunk, n_chunks;
    sig_shape(N, &chunk, &n_chunks);
    const int64_t slots = static_cast<int64_t>(n_chunks) * N * K;
    unsigned long long* part_key = reinterpret_cast<unsigned long long*>(work);
    int32_t* part_k = reinterpret_cast<int32_t*>(part_key + slots);
    int32_t* part_count = part_k + slots;
    hipStream_t st = as_stream(stream);
    const unsigned row_blocks = static_cast<unsigned>((static_cast<int64_t>(n_rows) + kSigBlock / 64 - 1) /
                                                      (kSigBlock / 64));
    hipLaunchKernelGGL(sig_scan_fn(S), dim3(row_blocks, static_cast<unsigned>(n_chunks)), dim3(kSigBlock), 0, st, sig,
                       ring, n_bits, N, start, n_rows, num, den, K, t_sig_screen, chunk, part_key, part_k, part_count);
    hipLaunchKernelGGL(sig_merge_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(n_rows) + kSigBlock / 16 - 1) /
                                                                    (kSigBlock / 16))),
                       dim3(kSigBlock), 0, st, n_rows, N, K, n_chunks, part_key, part_k, part_count, out_j, out_d,
                       out_k, out_count);
    return check_launch("sig match kernels");
}

int slam_sig_set_screen(int on) {
    if (on != 0 && on != 1) return fail(SLAM_EINVAL, "sig: screen %d (0 off, 1 on)", on);
    t_sig_screen = on;
    return ok();
}

int slam_sig_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "sig status: stream sync");
    int st = 0;
    if (hipMemcpyFromSymbol(&st, HIP_SYMBOL(g_sig_status), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "sig status: read");
    if (st == 0) return ok();
    const int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_sig_status), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "sig status: clear");
    if (st & kSigBadScan) return fail(SLAM_EINVAL, "sig: scan offsets descend or leave [0, P]");
    return fail(SLAM_EINVAL, "sig: a start outside [0, N]");
}

}  // extern "C"
