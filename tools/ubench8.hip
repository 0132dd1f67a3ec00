// Throughput of fp64 VALU work on the whole device (the freqz kernels' inner loops; MI355X_MICROARCH.md gives fp32 and transcendental
// issue costs but none for fp64): v_fma_f64 in 8 independent chains per lane, and sincospi(double) of ocml, each over 1024 blocks of
// 256 threads x 8 waves per SIMD. Prints lane-operations per second and, from the clock, cycles per wave-instruction per SIMD.
// hipcc --offload-arch=gfx950 -O3 -o tools/ubench8 tools/ubench8.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#define IT 4096
__global__ void __launch_bounds__(256) fma64(double* out, double c) {
    double a[8];
    for (int i = 0; i < 8; ++i) a[i] = threadIdx.x * 1e-3 + i;
    for (int it = 0; it < IT; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = fma(a[i], c, 1e-7);
    }
    double s = 0;
    for (int i = 0; i < 8; ++i) s += a[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
__global__ void __launch_bounds__(256) sincos64(double* out, double c) {
    double x = threadIdx.x * 1e-3, s = 0;
    for (int it = 0; it < IT / 16; ++it) {
        double sn, cs;
        sincospi(x, &sn, &cs);
        s += sn * cs;
        x = fma(x, c, 1e-9);
    }
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
int main() {
    int dev = 0, cus = 0, clk = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, dev);           // kHz
    const int blocks = cus * 8;                                                       // 8 waves per SIMD (4 SIMDs, 4 waves per block)
    double* d;
    (void)hipMalloc(&d, (size_t)blocks * 256 * 8);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int mode = 0; mode < 2; ++mode) {
        float best = 1e30f;
        for (int r = 0; r < 20; ++r) {
            (void)hipEventRecord(e0, 0);
            if (mode == 0) hipLaunchKernelGGL(fma64, dim3(blocks), dim3(256), 0, 0, d, 0.999999);
            else hipLaunchKernelGGL(sincos64, dim3(blocks), dim3(256), 0, 0, d, 1.0000001);
            (void)hipEventRecord(e1, 0);
            (void)hipEventSynchronize(e1);
            float ms;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (r >= 5 && ms < best) best = ms;
        }
        const double ops = (double)blocks * 256 * (mode == 0 ? 8.0 * IT : IT / 16.0);
        const double per_s = ops / (best * 1e-3);
        // wave-instructions per SIMD per cycle -> cycles per wave64 instruction (or per sincospi call) on one SIMD
        const double cyc = (best * 1e-3) * clk * 1e3 * (cus * 4) / (ops / 64);
        printf("%-10s %8.3f ms  %10.3e lane-ops/s  %6.2f cycles per wave64 %s per SIMD (clock attr %d MHz, %d CUs)\n", mode ? "sincospi" : "v_fma_f64",
               best, per_s, cyc, mode ? "call" : "instruction", clk / 1000, cus);
    }
    return 0;
}
