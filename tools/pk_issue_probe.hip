// pk_issue_probe.hip -- does a packed f32 VALU instruction (v_pk_mul_f32 / v_pk_add_f32) hold the vector pipe of gfx950 for one
// pass, like v_mul_f32 / v_add_f32, or for two?  ("Packed pairs in the rounds of the register solver".)
//
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize tools/pk_issue_probe.hip -o pk_issue_probe
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize --cuda-device-only -S tools/pk_issue_probe.hip -o pk_issue_probe.s
//
// Two kernels in the launch shape of the headline step kernel: 768 workgroups x 512 threads, registers capped for six waves per
// SIMD, and enough LDS per workgroup that exactly three of them share a CU -- so every SIMD of a 256-CU device holds six waves
// for the whole launch.  Each lane carries eight accumulator pairs through a long unrolled stream of a = a * m + c with
// -ffp-contract=off (a multiply and an add, individually rounded): one kernel on float2 vector types (8 v_pk_mul_f32 +
// 8 v_pk_add_f32 per pass over the accumulators), the other on the same sixteen floats one by one (16 v_mul_f32 + 16 v_add_f32;
// -fno-slp-vectorize keeps the compiler from pairing them again).  Same values, and both store their accumulators: the two
// result buffers must be equal bit for bit.
//
// Reported per kernel: the time of a launch (one event pair over LAUNCHES launches), the clock (the shader cycles wave 0 of
// workgroup 0 spent in the stream by s_memtime, against the 100 MHz s_memrealtime), and from both the VALU instructions issued
// per cycle per SIMD over the launch.  A pipe that takes a wave's instruction for four cycles issues 0.25 per cycle.  (Wave 0's
// own cycles say nothing about the rate: the oldest wave of a SIMD is issued first and is done long before the launch is.)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef float pk2 __attribute__((ext_vector_type(2)));

constexpr int WGS = 768, THREADS = 512, PAIRS = 8, PASSES = 2048, LAUNCHES = 8;
constexpr int LDS_WORDS = 12 * 1024;      // 48 KB: three workgroups per CU (160 KB), never four

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Stamp { unsigned long long cycles, ticks; };

// (the LDS block only sets the residency; one word of it is written and read, so that it is allocated)
#define PROBE_HEAD \
    __shared__ unsigned pad[LDS_WORDS]; \
    const unsigned gid = blockIdx.x * THREADS + threadIdx.x; \
    if (threadIdx.x == 0) pad[blockIdx.x % LDS_WORDS] = gid; \
    __syncthreads(); \
    const unsigned seed = (pad[blockIdx.x % LDS_WORDS] + threadIdx.x) & 63u;      /* = gid & 63, through the LDS word */ \
    const unsigned long long t0 = __builtin_readcyclecounter(), w0 = wall_clock64()
#define PROBE_TAIL \
    const unsigned long long t1 = __builtin_readcyclecounter(), w1 = wall_clock64(); \
    if (gid == 0) { st->cycles = t1 - t0; st->ticks = w1 - w0; }

__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(6, 6)))
void probe_packed(const float *__restrict__ in, float *__restrict__ out, Stamp *st) {
    PROBE_HEAD;
    pk2 a[PAIRS];
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) a[k] = pk2{in[2 * k] + (float)seed, in[2 * k + 1]};
    const pk2 m = {in[16], in[17]}, c = {in[18], in[19]};
#pragma unroll 4
    for (int i = 0; i < PASSES; ++i) {
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) a[k] = a[k] * m;
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) a[k] = a[k] + c;
    }
    PROBE_TAIL;
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) { out[(size_t)gid * 16 + 2 * k] = a[k].x; out[(size_t)gid * 16 + 2 * k + 1] = a[k].y; }
}

__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(6, 6)))
void probe_scalar(const float *__restrict__ in, float *__restrict__ out, Stamp *st) {
    PROBE_HEAD;
    float a[2 * PAIRS];
#pragma unroll
    for (int k = 0; k < PAIRS; ++k) { a[2 * k] = in[2 * k] + (float)seed; a[2 * k + 1] = in[2 * k + 1]; }
    const float mx = in[16], my = in[17], cx = in[18], cy = in[19];
#pragma unroll 4
    for (int i = 0; i < PASSES; ++i) {
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) { a[2 * k] = a[2 * k] * mx; a[2 * k + 1] = a[2 * k + 1] * my; }
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) { a[2 * k] = a[2 * k] + cx; a[2 * k + 1] = a[2 * k + 1] + cy; }
    }
    PROBE_TAIL;
#pragma unroll
    for (int k = 0; k < 2 * PAIRS; ++k) out[(size_t)gid * 16 + k] = a[k];
}

template <class K>
static int run(const char *name, K kernel, int instPerPass, const float *dIn, float *dOut, Stamp *dSt, std::vector<float> &res, int simds) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(kernel, dim3(WGS), dim3(THREADS), 0, 0, dIn, dOut, dSt);      // warm-up: code object loaded, clocks up
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    for (int l = 0; l < LAUNCHES; ++l) hipLaunchKernelGGL(kernel, dim3(WGS), dim3(THREADS), 0, 0, dIn, dOut, dSt);
    CHECK(hipEventRecord(e1));
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
    float ms = 0.0f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    Stamp st;
    CHECK(hipMemcpy(&st, dSt, sizeof st, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(res.data(), dOut, res.size() * sizeof(float), hipMemcpyDeviceToHost));
    const double perWave = (double)instPerPass * PASSES;                  // VALU instructions of the stream, per wave
    const double wavesPerSimd = (double)WGS * (THREADS / 64) / simds;
    const double mhz = st.ticks ? (double)st.cycles / ((double)st.ticks / 100.0) : 0.0;
    const double launchMs = ms / LAUNCHES;
    printf("%-7s %d VALU per pass, %.0f per wave, %.2f waves per SIMD | %.4f ms per launch (%d launches, %.3f ms) | "
           "wave 0: %llu cycles in %llu ticks of 100 MHz -> %.0f MHz | VALU per cycle per SIMD: %.4f (%.2f cycles each)\n",
           name, instPerPass, perWave, wavesPerSimd, launchMs, LAUNCHES, ms, st.cycles, st.ticks, mhz,
           wavesPerSimd * perWave / (launchMs * 1e-3 * mhz * 1e6), launchMs * 1e-3 * mhz * 1e6 / (wavesPerSimd * perWave));
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int simds = prop.multiProcessorCount * 4;
    printf("%s, %d CUs, %d SIMDs\n", prop.gcnArchName, prop.multiProcessorCount, simds);
    float hIn[20];
    for (int k = 0; k < 16; ++k) hIn[k] = 0.5f + 0.03125f * (float)k;
    hIn[16] = 0.99902344f; hIn[17] = 0.99804688f; hIn[18] = 0.0009765625f; hIn[19] = 0.001953125f;
    const size_t n = (size_t)WGS * THREADS * 16;
    float *dIn, *dOutP, *dOutS;
    Stamp *dSt;
    CHECK(hipMalloc(&dIn, sizeof hIn)); CHECK(hipMalloc(&dOutP, n * sizeof(float))); CHECK(hipMalloc(&dOutS, n * sizeof(float)));
    CHECK(hipMalloc(&dSt, sizeof(Stamp)));
    CHECK(hipMemcpy(dIn, hIn, sizeof hIn, hipMemcpyHostToDevice));
    std::vector<float> rp(n), rs(n);
    if (run("packed", probe_packed, 2 * PAIRS, dIn, dOutP, dSt, rp, simds)) return 1;
    if (run("scalar", probe_scalar, 4 * PAIRS, dIn, dOutS, dSt, rs, simds)) return 1;
    const bool same = memcmp(rp.data(), rs.data(), n * sizeof(float)) == 0;
    printf("results of the two kernels: %s (lane 1: %.9g %.9g)\n", same ? "bit-identical" : "DIFFERENT", rp[16], rp[17]);
    return same ? 0 : 2;
}
