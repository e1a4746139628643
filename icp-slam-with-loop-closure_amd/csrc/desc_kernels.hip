// desc_kernels.hip — batched matching of 32-byte binary descriptors (ORB) for
// gfx950 (MI355X): the hot loop of the reference's image loop-closure detector.
//
// The reference's detect_images_direct_similarity
// (src/loop_closure_detection.py:81-163) calls matchify (:61-79) for every
// image pair (i, j >= start[i]): a brute-force match of about 500 x 500
// descriptors, the `n_matches` best matches summed into one score.  Here one
// 256-thread workgroup matches one pair; include/slamhip.h states the rule.
//
// desc_pass: the lanes own the query descriptors (8 dwords each in registers,
// kDescQ = 2 per lane and pass: 512 queries a pass), the train descriptors pass
// through LDS in tiles of 256 and are read as broadcasts (every lane the same
// address, two 16-byte reads per descriptor).  A distance is 8 x (xor +
// accumulating popcount) for `hamming`, and |q|^2 + |t|^2 - 2 q.t with 8
// unsigned 4 x 8-bit dot products for `l2` (|t|^2 is computed once per tile
// load), all in exact integers.  Inside a tile the lane keeps the minimum of
// the packed key d << 8 | k (k the index in the tile), and after the tile the
// key's d replaces the lane's best only when strictly smaller: tiles and k
// ascend, so the smallest index among equal d wins with no extra work.
// `hamming`'s cross-check runs the same pass with the roles swapped (bwd[b] in
// LDS): no cross-lane reduction, no atomics on distances.  The alternative,
// one pass with an LDS atomicMin of the packed key d << 12 | a per distance
// (slam_desc_set_bwd(1)), gives the same bits; DESIGN.md section 3.7 has the
// A/B that chose the swapped pass.
//
// Selection: `hamming` counts its cross-checked matches in a 257-bin LDS
// histogram (integer atomics); an exclusive prefix over the bins gives what
// every bin contributes to the n_matches smallest, and the score
// sum d * taken[d] is an exact integer.  `l2`, and `hamming` when the rows are
// asked for, takes the n_matches smallest of the packed 64-bit key (d, a) in
// n_matches rounds of a block-wide minimum; lane 0 writes the rows and adds the
// summands left to right.  Only integers decide anything and no result depends
// on the workgroup order or the launch shape.  No floating-point atomics.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace slamhip {

constexpr int kDescBlock = 256;
constexpr int kDescQ = 2;          // query descriptors per lane and pass
constexpr int kDescTile = 256;     // train descriptors per LDS tile (8 KiB); the packed key holds 8 index bits
constexpr int kDescUnroll = 4;     // train descriptors read from LDS ahead of their use
constexpr int kDescMaxN = 4096;    // descriptors per image (the LDS result arrays)
constexpr uint32_t kDescNone = 0xFFFFFFFFu;
constexpr int kDescBadIndex = 1, kDescTooBig = 2;

static thread_local int t_desc_bwd = 0;   // slam_desc_set_bwd
__device__ int g_desc_status;   // kDescBadIndex | kDescTooBig of the launches since slam_desc_status

struct Desc {
    uint4 lo, hi;
};

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t acc) {
    return __builtin_amdgcn_udot4(a, b, acc, false);
}

__device__ __forceinline__ uint32_t desc_norm(const Desc& v) {
    uint32_t s = dot4(v.lo.x, v.lo.x, 0);
    s = dot4(v.lo.y, v.lo.y, s);
    s = dot4(v.lo.z, v.lo.z, s);
    s = dot4(v.lo.w, v.lo.w, s);
    s = dot4(v.hi.x, v.hi.x, s);
    s = dot4(v.hi.y, v.hi.y, s);
    s = dot4(v.hi.z, v.hi.z, s);
    return dot4(v.hi.w, v.hi.w, s);
}

// qt = |q|^2 + |t|^2 for l2 (unused for hamming)
template <int METRIC>
__device__ __forceinline__ uint32_t desc_dist(const Desc& q, const Desc& t, uint32_t qt) {
    if (METRIC == 0) {
        uint32_t d = bcnt(q.lo.x ^ t.lo.x, 0);
        d = bcnt(q.lo.y ^ t.lo.y, d);
        d = bcnt(q.lo.z ^ t.lo.z, d);
        d = bcnt(q.lo.w ^ t.lo.w, d);
        d = bcnt(q.hi.x ^ t.hi.x, d);
        d = bcnt(q.hi.y ^ t.hi.y, d);
        d = bcnt(q.hi.z ^ t.hi.z, d);
        return bcnt(q.hi.w ^ t.hi.w, d);
    }
    uint32_t s = dot4(q.lo.x, t.lo.x, 0);
    s = dot4(q.lo.y, t.lo.y, s);
    s = dot4(q.lo.z, t.lo.z, s);
    s = dot4(q.lo.w, t.lo.w, s);
    s = dot4(q.hi.x, t.hi.x, s);
    s = dot4(q.hi.y, t.hi.y, s);
    s = dot4(q.hi.z, t.hi.z, s);
    s = dot4(q.hi.w, t.hi.w, s);
    return qt - 2u * s;   // sum (q - t)^2 >= 0, at most 32 * 255^2 = 2,080,800
}

struct DescLds {
    uint4 tile[2 * kDescTile];
    uint32_t tnorm[kDescTile];
    uint32_t fd[kDescMaxN];    // d(a, fwd[a]); kDescNone once a is known not to be a match
    uint16_t fb[kDescMaxN];    // fwd[a]
    uint32_t ba[kDescMaxN];    // hamming: bwd[b] in the low 12 bits (above them d(bwd[b], b) when atomics made it)
    uint32_t hist[257];
    uint32_t wsum[4];
    unsigned long long wmin[2][4];
    uint32_t score, count;
};

template <int METRIC, bool ATOM, int NQ, int U>
__device__ __forceinline__ void desc_scan_some(DescLds& s, int t0, int k0, const Desc (&q)[kDescQ],
                                               const uint32_t (&qn)[kDescQ], const uint32_t (&qidx)[kDescQ],
                                               uint32_t (&key)[kDescQ]) {
    // all U descriptors are read before the first is used: the LDS latency is paid once per U
    Desc t[U];
    uint32_t tn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        t[u].lo = s.tile[2 * (k0 + u)];
        t[u].hi = s.tile[2 * (k0 + u) + 1];
        tn[u] = METRIC ? s.tnorm[k0 + u] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            const uint32_t d = desc_dist<METRIC>(q[r], t[u], qn[r] + tn[u]);
            key[r] = min(key[r], (d << 8) | static_cast<uint32_t>(k0 + u));
            // the A/B alternative for bwd: every distance goes to its train descriptor's packed (d, a) minimum
            if (ATOM && qidx[r] != kDescNone) atomicMin(&s.ba[t0 + k0 + u], (d << 12) | qidx[r]);
        }
    }
}

template <int METRIC, bool ATOM, int NQ>
__device__ __forceinline__ void desc_scan_tile(DescLds& s, int t0, int m, const Desc (&q)[kDescQ],
                                               const uint32_t (&qn)[kDescQ], const uint32_t (&qidx)[kDescQ],
                                               uint32_t (&key)[kDescQ]) {
    int k = 0;
    for (; k + kDescUnroll <= m; k += kDescUnroll)
        desc_scan_some<METRIC, ATOM, NQ, kDescUnroll>(s, t0, k, q, qn, qidx, key);
    for (; k < m; ++k) desc_scan_some<METRIC, ATOM, NQ, 1>(s, t0, k, q, qn, qidx, key);
}

// For every query descriptor i < nQ the smallest train index with the least
// distance, into out_i[i], and that distance into out_d[i] (when not null).
// nQ, nT in 1..kDescMaxN; every thread of the workgroup calls it.
template <int METRIC, bool ATOM>
__device__ __forceinline__ void desc_pass(DescLds& s, const uint4* __restrict__ Q, int nQ, const uint4* __restrict__ T,
                                          int nT, uint32_t* out_d, uint16_t* out_i16, uint32_t* out_i32) {
    const int tid = threadIdx.x;
    const int wave0 = tid & ~63;
    for (int q0 = 0; q0 < nQ; q0 += kDescBlock * kDescQ) {
        Desc q[kDescQ];
        uint32_t qn[kDescQ], qidx[kDescQ], best_d[kDescQ], best_i[kDescQ];
#pragma unroll
        for (int r = 0; r < kDescQ; ++r) {
            const int i = q0 + r * kDescBlock + tid;
            const uint4 z = make_uint4(0, 0, 0, 0);
            q[r].lo = i < nQ ? Q[2 * i] : z;   // a lane past the end matches zeros and writes nothing
            q[r].hi = i < nQ ? Q[2 * i + 1] : z;
            qn[r] = METRIC ? desc_norm(q[r]) : 0u;
            qidx[r] = i < nQ ? static_cast<uint32_t>(i) : kDescNone;
            best_d[r] = kDescNone;
            best_i[r] = 0;
        }
        const bool one = q0 + wave0 < nQ;                // wave-uniform: this wave holds a query
        const bool two = q0 + kDescBlock + wave0 < nQ;   // ... and one in its second slot
        for (int t0 = 0; t0 < nT; t0 += kDescTile) {
            const int m = min(kDescTile, nT - t0);
            __syncthreads();   // the previous tile's readers are done
            if (tid < m) {
                Desc t;
                t.lo = T[2 * (t0 + tid)];
                t.hi = T[2 * (t0 + tid) + 1];
                s.tile[2 * tid] = t.lo;
                s.tile[2 * tid + 1] = t.hi;
                if (METRIC) s.tnorm[tid] = desc_norm(t);
            }
            __syncthreads();
            if (!one) continue;
            uint32_t key[kDescQ];
#pragma unroll
            for (int r = 0; r < kDescQ; ++r) key[r] = kDescNone;
            if (two)
                desc_scan_tile<METRIC, ATOM, kDescQ>(s, t0, m, q, qn, qidx, key);
            else
                desc_scan_tile<METRIC, ATOM, 1>(s, t0, m, q, qn, qidx, key);
#pragma unroll
            for (int r = 0; r < kDescQ; ++r) {
                const uint32_t d = key[r] >> 8;   // d < 2^21: a key that saw a descriptor is never kDescNone
                if (key[r] != kDescNone && d < best_d[r]) {
                    best_d[r] = d;
                    best_i[r] = static_cast<uint32_t>(t0) + (key[r] & 255u);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kDescQ; ++r) {
            const int i = q0 + r * kDescBlock + tid;
            if (i < nQ) {
                if (out_d) out_d[i] = best_d[r];
                if (out_i16) out_i16[i] = static_cast<uint16_t>(best_i[r]);
                if (out_i32) out_i32[i] = best_i[r];
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

template <int METRIC, bool ATOM>
__global__ __launch_bounds__(kDescBlock) void desc_match_kernel(const uint8_t* __restrict__ desc,
                                                                const int64_t* __restrict__ img_off, int32_t M,
                                                                const int32_t* __restrict__ qi,
                                                                const int32_t* __restrict__ ti, int32_t n_matches,
                                                                double* __restrict__ out_score,
                                                                int32_t* __restrict__ out_count,
                                                                int32_t* __restrict__ out_matches) {
    __shared__ DescLds s;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int32_t* rows = out_matches ? out_matches + b * n_matches * 3 : nullptr;
    const int32_t iq = qi[b], it = ti[b];

    // the pair's own bounds (all uniform): nothing is read through a bad index
    int bad = 0;
    int64_t a0 = 0, b0 = 0, nA64 = 0, nB64 = 0;
    if (iq < 0 || iq >= M || it < 0 || it >= M) {
        bad = kDescBadIndex;
    } else {
        a0 = img_off[iq];
        nA64 = img_off[iq + 1] - a0;
        b0 = img_off[it];
        nB64 = img_off[it + 1] - b0;
        if (a0 < 0 || b0 < 0 || nA64 < 0 || nB64 < 0)
            bad = kDescBadIndex;
        else if (nA64 > kDescMaxN || nB64 > kDescMaxN)
            bad = kDescTooBig;
    }
    if (bad) {
        if (tid == 0) {
            atomicOr(&g_desc_status, bad);
            out_score[b] = __builtin_nan("");
            out_count[b] = -1;
        }
        if (rows)
            for (int i = tid; i < 3 * n_matches; i += kDescBlock) rows[i] = -1;
        return;
    }
    const int nA = static_cast<int>(nA64), nB = static_cast<int>(nB64);
    const uint4* A = reinterpret_cast<const uint4*>(desc + a0 * 32);
    const uint4* Bd = reinterpret_cast<const uint4*>(desc + b0 * 32);

    // forward, and for hamming the same pass with the roles swapped (one copy of the code)
    const int count0 = nA > 0 && nB > 0 ? nA : 0;
    int count = count0;
    if (ATOM) {
        for (int i = tid; i < nB; i += kDescBlock) s.ba[i] = kDescNone;   // desc_pass starts with a barrier
        if (count0 > 0) desc_pass<METRIC, true>(s, A, nA, Bd, nB, s.fd, s.fb, nullptr);
    } else {
#pragma unroll 1
        for (int dir = 0; dir < (METRIC == 0 ? 2 : 1) && count0 > 0; ++dir)
            desc_pass<METRIC, false>(s, dir ? Bd : A, dir ? nB : nA, dir ? A : Bd, dir ? nA : nB,
                                     dir ? nullptr : s.fd, dir ? nullptr : s.fb, dir ? s.ba : nullptr);
    }
    if (METRIC == 0 && count > 0) {
        for (int i = tid; i < 257; i += kDescBlock) s.hist[i] = 0;
        if (tid == 0) s.score = 0;
        __syncthreads();
        for (int a = tid; a < nA; a += kDescBlock) {
            if ((s.ba[s.fb[a]] & 4095u) == static_cast<uint32_t>(a))
                atomicAdd(&s.hist[s.fd[a]], 1u);
            else
                s.fd[a] = kDescNone;
        }
        __syncthreads();
        // exclusive prefix over bins 0..255 (lane = bin); bin 256 comes last
        const uint32_t h = s.hist[tid];
        uint32_t inc = h;
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) s.wsum[wave] = inc;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) base += s.wsum[w];
            total += s.wsum[w];
        }
        const uint32_t excl = base + inc - h;
        const uint32_t want = static_cast<uint32_t>(n_matches);
        const uint32_t taken = excl >= want ? 0u : min(h, want - excl);
        if (taken) atomicAdd(&s.score, static_cast<uint32_t>(tid) * taken);
        if (tid == 0) {
            const uint32_t h256 = s.hist[256];
            const uint32_t t256 = total >= want ? 0u : min(h256, want - total);
            if (t256) atomicAdd(&s.score, 256u * t256);
            s.count = total + h256;
        }
        __syncthreads();
        count = static_cast<int>(s.count);
    }

    if (count < n_matches) {
        if (tid == 0) {
            out_score[b] = __builtin_huge_val();
            out_count[b] = count;
        }
        if (rows)
            for (int i = tid; i < 3 * n_matches; i += kDescBlock) rows[i] = -1;
        return;
    }
    if (METRIC == 0 && !rows) {
        if (tid == 0) {
            out_score[b] = static_cast<double>(s.score);
            out_count[b] = count;
        }
        return;
    }

    // the n_matches smallest (d, a), one block-wide minimum per round
    unsigned long long lo = 0;
    double sum = 0.0;
    for (int r = 0; r < n_matches; ++r) {
        unsigned long long best = ~0ull;
        for (int a = tid; a < nA; a += kDescBlock) {
            const uint32_t d = s.fd[a];
            const unsigned long long key = (static_cast<unsigned long long>(d) << 32) | static_cast<uint32_t>(a);
            if (d != kDescNone && key >= lo && key < best) best = key;
        }
        best = wave_min_u64(best);
        if ((tid & 63) == 0) s.wmin[r & 1][tid >> 6] = best;
        __syncthreads();   // one barrier per round: the slots alternate
        best = s.wmin[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const unsigned long long v = s.wmin[r & 1][w];
            best = v < best ? v : best;
        }
        lo = best + 1;
        if (tid == 0) {
            const uint32_t a = static_cast<uint32_t>(best), d = static_cast<uint32_t>(best >> 32);
            if (rows) {
                rows[3 * r] = static_cast<int32_t>(a);
                rows[3 * r + 1] = s.fb[a];
                rows[3 * r + 2] = static_cast<int32_t>(d);
            }
            // l2: the float32 square root (the fp64 root rounded to float32 is the same float for every
            // d <= 2,080,800: tests/test_desc.py)
            const double root = static_cast<float>(sqrt(static_cast<double>(d)));
            sum += METRIC ? root : static_cast<double>(d);
        }
    }
    if (tid == 0) {
        out_score[b] = sum;
        out_count[b] = count;
    }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int64_t slam_desc_work_size(int32_t B, int32_t max_n, int32_t n_matches) {
    // every intermediate of a pair lives in its workgroup's LDS: the buffer is a fixed, reserved 256 bytes
    if (B < 0) return fail(SLAM_EINVAL, "desc: B = %d < 0", B);
    if (max_n < 0) return fail(SLAM_EINVAL, "desc: max_n = %d < 0", max_n);
    if (max_n > kDescMaxN) return fail(SLAM_ETOOBIG, "desc: %d descriptors in an image, at most %d", max_n, kDescMaxN);
    if (n_matches < 1 || n_matches > 256) return fail(SLAM_EINVAL, "desc: n_matches = %d outside 1..256", n_matches);
    ok();
    return 256;
}

int slam_desc_match_batch(const uint8_t* desc, const int64_t* img_off, int32_t M, const int32_t* qi,
                          const int32_t* ti, int32_t B, int32_t metric, int32_t n_matches, double* out_score,
                          int32_t* out_count, int32_t* out_matches, void* work, void* stream) {
    if (!desc || !img_off || !qi || !ti || !out_score || !out_count || !work)
        return fail(SLAM_EINVAL, "desc: null array");
    if (reinterpret_cast<uintptr_t>(desc) % 16) return fail(SLAM_EINVAL, "desc: descriptors not 16-byte aligned");
    if (B < 0) return fail(SLAM_EINVAL, "desc: B = %d < 0", B);
    if (M <= 0) return fail(SLAM_EINVAL, "desc: M = %d <= 0", M);
    if (metric != 0 && metric != 1) return fail(SLAM_EINVAL, "desc: unknown metric %d (0 hamming, 1 l2)", metric);
    if (n_matches < 1 || n_matches > 256) return fail(SLAM_EINVAL, "desc: n_matches = %d outside 1..256", n_matches);
    if (B == 0) return ok();
    auto fn = metric == 1 ? desc_match_kernel<1, false>
                          : (t_desc_bwd == 1 ? desc_match_kernel<0, true> : desc_match_kernel<0, false>);
    hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(B)), dim3(kDescBlock), 0, as_stream(stream), desc, img_off, M,
                       qi, ti, n_matches, out_score, out_count, out_matches);
    return check_launch("desc match kernel");
}

int slam_desc_set_bwd(int mode) {
    if (mode != 0 && mode != 1) return fail(SLAM_EINVAL, "desc: bwd mode %d (0 swapped pass, 1 LDS atomics)", mode);
    t_desc_bwd = mode;
    return ok();
}

int slam_desc_status(void* stream) {
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return fail(SLAM_EHIP, "desc status: stream sync");
    int st = 0;
    if (hipMemcpyFromSymbol(&st, HIP_SYMBOL(g_desc_status), sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "desc status: read");
    if (st == 0) return ok();
    const int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_desc_status), &zero, sizeof(int)) != hipSuccess)
        return fail(SLAM_EHIP, "desc status: clear");
    if (st & kDescBadIndex)
        return fail(SLAM_EINVAL, "desc: a pair names an image outside [0, M) or its offsets descend");
    return fail(SLAM_ETOOBIG, "desc: an image holds more than %d descriptors", kDescMaxN);
}

}  // extern "C"
