// expf_ulps.hip -- the error of the device expf against float64 exp on the host, over every float32 in [-17, -2^-24] and at 0: the one number of the
// edge softmax's bound that cannot be derived (tests/edge_reference.py EXP_ULPS).  Stand-alone:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tests/studies/expf_ulps.hip -o expf_ulps && ./expf_ulps
// The arguments run through their bit patterns in batches; the device writes expf(x), the host compares with exp((double) x) and prints the largest
// error in units of the last place of the float32 nearest the exact value, the argument that attains it, and how many results were not the correctly
// rounded one.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define TRY(e)                                                                                          \
    do {                                                                                                \
        hipError_t s_ = (e);                                                                            \
        if (s_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(s_)); return 2; }              \
    } while (0)

__global__ void k_expf(uint32_t first, uint32_t n, float *out)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = expf(__uint_as_float(first + i));
}

static float as_float(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

int main()
{
    const uint32_t lo = as_bits(-ldexpf(1.0f, -24)), hi = as_bits(-17.0f);      // negative floats: the bit pattern grows with the magnitude
    const uint32_t batch = 1u << 24;
    float *d = nullptr;
    TRY(hipMalloc(&d, sizeof(float) * batch));
    std::vector<float> h(batch);
    double worst = 0.0;
    float worst_x = 0.0f;
    uint64_t total = 0, misrounded = 0;
    auto judge = [&](float x, float got) {
        const double want = exp((double)x);
        const double ulp = ldexp(1.0, ilogb(want) - 23);              // every exact value here is normal in float32 (exp(-17) = 4.1e-8)
        const double err = fabs((double)got - want) / ulp;
        if (err > worst) { worst = err; worst_x = x; }
        if (got != (float)want) misrounded++;
        total++;
    };
    for (uint64_t first = lo; first <= hi; first += batch) {
        const uint32_t n = (uint32_t)((uint64_t)hi - first + 1 < batch ? (uint64_t)hi - first + 1 : batch);
        hipLaunchKernelGGL(k_expf, dim3(4096), dim3(256), 0, 0, (uint32_t)first, n, d);
        TRY(hipGetLastError());
        TRY(hipMemcpy(h.data(), d, sizeof(float) * n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) judge(as_float((uint32_t)first + i), h[i]);
    }
    hipLaunchKernelGGL(k_expf, dim3(1), dim3(64), 0, 0, 0u, 1u, d);    // x = +0
    TRY(hipGetLastError());
    TRY(hipMemcpy(h.data(), d, sizeof(float), hipMemcpyDeviceToHost));
    judge(0.0f, h[0]);
    printf("expf(0) = %.9g\n", h[0]);
    TRY(hipFree(d));
    printf("arguments: %llu (every float32 in [-17, -2^-24] and 0)\n", (unsigned long long)total);
    printf("largest error: %.6f ulps at x = %.9g (bits 0x%08x)\n", worst, worst_x, as_bits(worst_x));
    printf("not correctly rounded: %llu\n", (unsigned long long)misrounded);
    return 0;
}
