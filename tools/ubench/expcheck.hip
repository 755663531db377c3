// The shipped exp / exp10 (wt::exp_k / wt::exp10_k with the product's constant table, wt_tables.hpp) against OCML's on
// the device, bit for bit.
//   hipcc --offload-arch=gfx950 -O3 -I ics-wt-physicsengine_amd/csrc -o tools/scratch/expcheck tools/ubench/expcheck.hip && tools/scratch/expcheck
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <cmath>
#include "wt_tables.hpp"

__global__ void chk(const double *x, int n, int which, unsigned long long *mism, double *worst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = which ? wt::exp10_k(wt::kp_of(wt::default_ktab()), x[i]) : wt::exp_k(wt::kt_of(wt::default_ktab()), x[i]);
    const double b = which ? exp10(x[i]) : exp(x[i]);
    if (__double_as_longlong(a) != __double_as_longlong(b) && !(a != a && b != b)) { atomicAdd(mism, 1ull); worst[which] = x[i]; }
}

int main()
{
    const int n = 1 << 22;
    std::vector<double> h(n);
    double *d; unsigned long long *m; double *w;
    hipMalloc(&d, n * sizeof(double)); hipMalloc(&m, 8); hipMalloc(&w, 16);
    struct { double lo, hi; const char *name; int which; } cases[] = {
        {-14.5, 0.5, "exp10 on [-14.5, 0.5] (H = 10^-pH)", 1}, {-400, 400, "exp10 on [-400, 400]", 1},
        {-3.0, 3.0, "exp on [-3, 3] (Arrhenius exponent)", 0}, {-800, 800, "exp on [-800, 800]", 0}};
    uint64_t s = 88172645463325252ull;
    for (auto &c : cases) {
        for (int i = 0; i < n; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; h[i] = c.lo + (c.hi - c.lo) * ((s >> 11) * (1.0 / 9007199254740992.0)); }
        h[0] = c.lo; h[1] = c.hi; h[2] = 0.0; h[3] = -0.0; h[4] = NAN; h[5] = INFINITY; h[6] = -INFINITY; h[7] = 1e300; h[8] = -1e300;
        hipMemcpy(d, h.data(), n * sizeof(double), hipMemcpyHostToDevice);
        hipMemset(m, 0, 8);
        hipLaunchKernelGGL(chk, dim3(n / 256), dim3(256), 0, 0, d, n, c.which, m, w);
        unsigned long long mm; double ww[2];
        hipMemcpy(&mm, m, 8, hipMemcpyDeviceToHost); hipMemcpy(ww, w, 16, hipMemcpyDeviceToHost);
        printf("%-42s %d samples: %llu mismatches vs OCML%s\n", c.name, n, mm, mm ? "" : " (bit-identical)");
        if (mm) printf("   e.g. x = %.17g\n", ww[c.which]);
    }
    return 0;
}
