// compares the library's wave_max_f32 (cpk_device_common.inl: v_max_f32 with DPP operands, no LDS) with a plain
// __shfl_xor reduction, one wave, pattern by pattern: the maximum in each of the 64 lanes in turn, all -inf, ties, a -inf
// half-wave (either half), one NaN lane (both must return the largest non-NaN value).  Every lane's result is compared:
// the value is wave-uniform.  Prints one line; exit status 1 on a mismatch.
// hipcc --offload-arch=gfx950 -I cpecan_amd/csrc -I include -o wave_max_check tools/wave_max_check.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cpecan_internal.h"
#define NEG_INF (-__builtin_huge_val())
#include "cpk_device_common.inl"

__device__ __forceinline__ float shuffle_max_f32(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__global__ void k(const float *in, float *outNew, float *outRef, int nPat) {
    const int lane = threadIdx.x;
    for (int p = 0; p < nPat; p++) {
        const float v = in[p * 64 + lane];
        outNew[p * 64 + lane] = wave_max_f32(v);
        outRef[p * 64 + lane] = shuffle_max_f32(v);
    }
}

int main() {
    const float inf = INFINITY;
    std::vector<float> in;
    std::vector<float> want;  // what both reductions must return
    auto add = [&](const float (&v)[64], float w) {
        in.insert(in.end(), v, v + 64);
        want.push_back(w);
    };
    float v[64];
    for (int at = 0; at < 64; at++) {  // the maximum in each lane in turn, the others distinct and below it
        for (int i = 0; i < 64; i++) v[i] = -1000.0f - 3.5f * (float)((i * 37) & 63);
        v[at] = 7.25f;
        add(v, 7.25f);
    }
    for (int i = 0; i < 64; i++) v[i] = -inf;
    add(v, -inf);
    for (int i = 0; i < 64; i++) v[i] = -2.0f - (float)(i % 3);  // ties: the maximum in 22 lanes
    add(v, -2.0f);
    for (int i = 0; i < 64; i++) v[i] = -5.5f;  // ... and in all of them
    add(v, -5.5f);
    for (int half = 0; half < 2; half++) {  // a -inf half-wave
        for (int i = 0; i < 64; i++) v[i] = (i < 32) == (half == 0) ? -inf : -40.0f - (float)i;
        add(v, half == 0 ? -72.0f : -40.0f);
    }
    for (int at : {0, 15, 16, 31, 32, 47, 63}) {  // one NaN lane, at row borders too
        for (int i = 0; i < 64; i++) v[i] = -300.0f + (float)((i * 11) & 63);
        float w = -inf;
        v[at] = NAN;
        for (int i = 0; i < 64; i++)
            if (i != at && v[i] > w) w = v[i];
        add(v, w);
    }
    const int nPat = (int)want.size();
    const size_t bytes = in.size() * sizeof(float);
    float *dIn, *dNew, *dRef;
    if (hipMalloc(&dIn, bytes) != hipSuccess || hipMalloc(&dNew, bytes) != hipSuccess || hipMalloc(&dRef, bytes) != hipSuccess) {
        printf("wave_max_check: no device memory\n");
        return 2;
    }
    hipMemcpy(dIn, in.data(), bytes, hipMemcpyHostToDevice);
    hipMemset(dNew, 0, bytes);
    hipMemset(dRef, 0, bytes);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dIn, dNew, dRef, nPat);
    std::vector<float> gotNew(in.size()), gotRef(in.size());
    if (hipMemcpy(gotNew.data(), dNew, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(gotRef.data(), dRef, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("wave_max_check: the kernel did not run\n");
        return 2;
    }
    int bad = 0, firstPat = -1, firstLane = -1;
    for (int p = 0; p < nPat; p++)
        for (int i = 0; i < 64; i++) {
            const float a = gotNew[p * 64 + i], b = gotRef[p * 64 + i], w = want[p];
            if (memcmp(&a, &w, 4) != 0 || memcmp(&b, &w, 4) != 0) {
                if (!bad) firstPat = p, firstLane = i;
                bad++;
            }
        }
    if (bad) {
        printf("wave_max_check: MISMATCH in %d of %d results, first at pattern %d lane %d: dpp %g shuffle %g expected %g\n", bad,
               nPat * 64, firstPat, firstLane, gotNew[firstPat * 64 + firstLane], gotRef[firstPat * 64 + firstLane], want[firstPat]);
        return 1;
    }
    printf("wave_max_check: ok, %d patterns x 64 lanes: dpp == shuffle == expected\n", nPat);
    return 0;
}
