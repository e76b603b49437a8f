// one probe: what v_mfma_f32_16x16x4_f32 does with subnormal operands, accumulators and results, beside fmaf on the same values
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
typedef float floatx4 __attribute__((ext_vector_type(4)));
struct Case { float a, b, c; int terms; };   // terms: 1 = only k = 0 carries a * b, 4 = every k
__global__ void probe(const Case* cs, int n, float* out_mfma, float* out_fma) {
    const int lane = threadIdx.x & 63, g = lane >> 4;
    for (int i = 0; i < n; ++i) {
        const Case c = cs[i];
        const bool on = c.terms == 4 || g == 0;
        floatx4 acc = {c.c, c.c, c.c, c.c};
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(on ? c.a : 0.0f, on ? c.b : 0.0f, acc, 0, 0, 0);
        if (lane == 0) {
            out_mfma[i] = acc[0];
            float f = c.c;
            for (int t = 0; t < c.terms; ++t) f = fmaf(c.a, c.b, f);
            out_fma[i] = f;
        }
    }
}
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main() {
    const Case cs[] = {
        {ldexpf(1, -149), 1.0f, 0.0f, 1},               // subnormal operand (smallest)
        {ldexpf(1, -127), 1.0f, 0.0f, 1},               // subnormal operand (largest power of two)
        {1.0f, ldexpf(3, -140), 0.0f, 1},               // subnormal as the other operand
        {ldexpf(1, -149), ldexpf(1, 23), 0.0f, 1},      // subnormal operand, normal result 2^-126
        {ldexpf(1, -100), ldexpf(1, -40), 0.0f, 1},     // normal operands, subnormal result 2^-140
        {ldexpf(1, -100), ldexpf(1, -49), 0.0f, 1},     // normal operands, result 2^-149
        {ldexpf(1, -100), ldexpf(1, -50), 0.0f, 1},     // normal operands, result 2^-150 (half the smallest subnormal: ties to even -> 0)
        {0.0f, 0.0f, ldexpf(1, -149), 1},               // subnormal accumulator, nothing added
        {0.0f, 0.0f, ldexpf(5, -130), 1},               // subnormal accumulator, nothing added
        {ldexpf(1, -126), 1.0f, -ldexpf(1, -127), 1},   // normal + subnormal accumulator -> subnormal 2^-127
        {ldexpf(1, -128), 1.0f, 0.0f, 4},               // four subnormal terms -> normal 2^-126
        {ldexpf(1, -126), 1.0f, 0.0f, 1},               // smallest normal, for comparison
    };
    const int n = sizeof(cs) / sizeof(cs[0]);
    Case* d_cs; float *d_m, *d_f;
    if (hipMalloc(&d_cs, sizeof(cs)) || hipMalloc(&d_m, n * 4) || hipMalloc(&d_f, n * 4)) return 2;
    if (hipMemcpy(d_cs, cs, sizeof(cs), hipMemcpyHostToDevice)) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d_cs, n, d_m, d_f);
    float m[n], f[n];
    if (hipDeviceSynchronize() || hipMemcpy(m, d_m, n * 4, hipMemcpyDeviceToHost) || hipMemcpy(f, d_f, n * 4, hipMemcpyDeviceToHost)) return 3;
    for (int i = 0; i < n; ++i) {
        double exact = (double)cs[i].c + cs[i].terms * ((double)cs[i].a * (double)cs[i].b);
        printf("PROBE a=%08x b=%08x c=%08x terms=%d  exact %.6a  mfma %08x (%.6a)  fmaf %08x (%.6a)\n", bits(cs[i].a), bits(cs[i].b), bits(cs[i].c),
               cs[i].terms, exact, bits(m[i]), (double)m[i], bits(f[i]), (double)f[i]);
    }
    return 0;
}
