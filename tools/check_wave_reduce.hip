// Check of wave_group_bounds (csrc/common.hpp), the fused reduction of the ICP
// group search, against a serial loop on the host: one workgroup of 64 lanes,
// every (active-lane set, value pattern) case in turn.  Prints one line
// "check_wave_reduce: N cases, M mismatches" and exits 0 only for M == 0.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Iinclude -Iicp-slam-with-loop-closure_amd/csrc
//         tools/check_wave_reduce.hip -o tools/check_wave_reduce
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"

constexpr int kWinT = 4;       // the kernel's window (sub-chunks)
constexpr int kNsubT = 136;    // 1081 candidates: window starts in [0, nsub - kWin]

struct Lane {
    float qx, qy, m2;
    int ws, act;
};

__global__ void check_kernel(const Lane* in, int ncases, uint32_t* out) {
    const int lane = threadIdx.x;
    for (int c = 0; c < ncases; ++c) {
        const Lane l = in[c * 64 + lane];
        const slamhip::GroupBounds g = slamhip::wave_group_bounds(l.act != 0, l.qx, l.qy, l.m2, l.ws, kWinT);
        uint32_t* o = out + (static_cast<size_t>(c) * 64 + lane) * 7;
        o[0] = __float_as_uint(g.bx0);
        o[1] = __float_as_uint(g.bx1);
        o[2] = __float_as_uint(g.by0);
        o[3] = __float_as_uint(g.by1);
        o[4] = __float_as_uint(g.gM2);
        o[5] = static_cast<uint32_t>(g.wlo);
        o[6] = static_cast<uint32_t>(g.whi);
    }
}

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// a before b in the order of the reals, -0 before +0
static bool before(float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }

int main() {
    std::vector<std::vector<int>> sets;
    sets.push_back({});
    sets.push_back({0});
    sets.push_back({63});
    sets.push_back({3, 21, 40, 62});   // one lane in each 16-lane row
    {
        std::vector<int> row;
        for (int l = 16; l < 32; ++l) row.push_back(l);
        sets.push_back(row);
    }
    sets.push_back({31, 32});
    {
        std::vector<int> all;
        for (int l = 0; l < 64; ++l) all.push_back(l);
        sets.push_back(all);
    }
    constexpr int kPatterns = 5;
    const int ncases = static_cast<int>(sets.size()) * kPatterns;
    std::vector<Lane> in(static_cast<size_t>(ncases) * 64);
    uint32_t rng = 12345u;
    auto rnd = [&]() {
        rng = rng * 1664525u + 1013904223u;
        return static_cast<float>(rng >> 8) * (1.0f / 16777216.0f);   // [0, 1)
    };
    for (int s = 0; s < static_cast<int>(sets.size()); ++s) {
        for (int p = 0; p < kPatterns; ++p) {
            Lane* L = in.data() + static_cast<size_t>(s * kPatterns + p) * 64;
            for (int l = 0; l < 64; ++l) {
                Lane& q = L[l];
                q.act = 0;
                switch (p) {
                    case 0:   // both signs, all different
                        q.qx = 20.0f * rnd() - 10.0f;
                        q.qy = 20.0f * rnd() - 10.0f;
                        q.m2 = 4.0f * rnd();
                        q.ws = static_cast<int>(rnd() * (kNsubT - kWinT + 1));
                        break;
                    case 1:   // signed zeros only
                        q.qx = (l & 1) ? -0.0f : 0.0f;
                        q.qy = (l & 2) ? 0.0f : -0.0f;
                        q.m2 = 0.0f;
                        q.ws = 0;
                        break;
                    case 2:   // equal values in several lanes, windows at both ends
                        q.qx = static_cast<float>(l % 4) - 1.5f;
                        q.qy = -static_cast<float>(l % 3);
                        q.m2 = static_cast<float>(l % 5) * 0.25f;
                        q.ws = (l % 2) ? kNsubT - kWinT : 0;
                        break;
                    case 3:   // the largest finite float, +inf as M2
                        q.qx = (l % 7 == 0) ? FLT_MAX : (l % 7 == 3) ? -FLT_MAX : 3.0f * rnd();
                        q.qy = (l % 5 == 1) ? -FLT_MAX : (l % 5 == 4) ? FLT_MAX : -3.0f * rnd();
                        q.m2 = (l % 9 == 0) ? INFINITY : (l % 9 == 5) ? FLT_MAX : rnd();
                        q.ws = kNsubT - kWinT;
                        break;
                    default:   // negative coordinates only, overlapping windows
                        q.qx = -1.0f - rnd();
                        q.qy = -100.0f * rnd() - 1e-30f;
                        q.m2 = 1e-30f * rnd();
                        q.ws = 60 + l % 3;
                        break;
                }
            }
            for (int l : sets[s]) L[l].act = 1;
        }
    }
    Lane* din = nullptr;
    uint32_t* dout = nullptr;
    const size_t nout = static_cast<size_t>(ncases) * 64 * 7;
    if (hipMalloc(&din, in.size() * sizeof(Lane)) != hipSuccess || hipMalloc(&dout, nout * 4) != hipSuccess ||
        hipMemcpy(din, in.data(), in.size() * sizeof(Lane), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dout, 0xee, nout * 4) != hipSuccess) {
        printf("check_wave_reduce: HIP set-up failed\n");
        return 2;
    }
    check_kernel<<<1, 64>>>(din, ncases, dout);
    std::vector<uint32_t> out(nout);
    const hipError_t e = hipMemcpy(out.data(), dout, nout * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        printf("check_wave_reduce: %s\n", hipGetErrorString(e));
        return 2;
    }
    int bad = 0;
    for (int c = 0; c < ncases; ++c) {
        const Lane* L = in.data() + static_cast<size_t>(c) * 64;
        float bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY, gm2 = 0.0f;
        int wlo = 0, wend = 0xffff;   // [max ws, min (ws + kWin)) over the active lanes
        for (int l = 0; l < 64; ++l) {
            if (!L[l].act) continue;
            if (before(L[l].qx, bx0)) bx0 = L[l].qx;
            if (before(bx1, L[l].qx)) bx1 = L[l].qx;
            if (before(L[l].qy, by0)) by0 = L[l].qy;
            if (before(by1, L[l].qy)) by1 = L[l].qy;
            if (L[l].m2 > gm2) gm2 = L[l].m2;
            if (L[l].ws > wlo) wlo = L[l].ws;
            if (L[l].ws + kWinT < wend) wend = L[l].ws + kWinT;
        }
        const uint32_t want[7] = {bits(bx0), bits(bx1), bits(by0), bits(by1), bits(gm2),
                                  static_cast<uint32_t>(wlo), static_cast<uint32_t>(wend)};
        for (int l = 0; l < 64; ++l) {
            for (int q = 0; q < 7; ++q) {
                const uint32_t got = out[(static_cast<size_t>(c) * 64 + l) * 7 + q];
                if (got != want[q]) {
                    if (bad < 10)
                        fprintf(stderr, "case %d (set %d pattern %d) lane %d value %d: got %08x want %08x\n", c,
                                c / kPatterns, c % kPatterns, l, q, got, want[q]);
                    ++bad;
                }
            }
        }
    }
    printf("check_wave_reduce: %d cases, %d mismatches\n", ncases, bad);
    (void)hipFree(din);
    (void)hipFree(dout);
    return bad == 0 ? 0 : 1;
}
