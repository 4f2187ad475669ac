// swap_calib.hip -- issue cost of a per-lane exchange of two VGPRs (gfx950): v_swap_b32 and
// v_pk_mov_b32 ... op_sel:[1,0], beside v_fma_f32 (2 cycles) and v_min_f32 (4 cycles) as anchors.
//
// DEVELOPER TOOL (tests/tools), in the manner of valu_calib.hip: not part of the product.  Build + run:
//     hipcc --offload-arch=gfx950 -O2 -o swap_calib tests/tools/swap_calib.hip && timeout -k 10 120 ./swap_calib
//
// Every class: 256-thread workgroups, 8 per CU (8 waves per SIMD); each wave runs ITER iterations of a
// block of 64 instructions of the class over 8 independent register pairs and stamps s_memtime around
// the loop.  Reported: shader cycles per wave64 instruction per SIMD = the median wave's cycles /
// (instructions per wave x 8), with all lanes active, the even lanes only, and lanes 0-31 only.
// First it checks what the two exchange instructions do to the lanes inside and outside exec.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int ITER = 512;
constexpr int PER_BLOCK = 64;
constexpr int WPS = 8;          // waves per SIMD

struct Out { unsigned long long cycles; unsigned long long realtime; };

#define REP8(S) S S S S S S S S

// exec_mode: 0 all lanes, 1 even lanes, 2 lanes 0-31
__device__ __forceinline__ void set_exec(int exec_mode)
{
    if (exec_mode == 1) asm volatile("s_mov_b32 exec_lo, 0x55555555\n\ts_mov_b32 exec_hi, 0x55555555");
    else if (exec_mode == 2) asm volatile("s_mov_b64 exec, 0x00000000ffffffff");
}

#define PROLOGUE                                                                                  \
    const float s0 = seed[threadIdx.x & 7];                                                       \
    float a0 = s0, a1 = s0 + 1.f, a2 = s0 + 2.f, a3 = s0 + 3.f, a4 = s0 + 4.f, a5 = s0 + 5.f, a6 = s0 + 6.f, a7 = s0 + 7.f, \
          a8 = s0 + 8.f, a9 = s0 + 9.f, a10 = s0 + 10.f, a11 = s0 + 11.f, a12 = s0 + 12.f, a13 = s0 + 13.f, a14 = s0 + 14.f, a15 = s0 + 15.f; \
    v2f p0 = {a0, a1}, p1 = {a2, a3}, p2 = {a4, a5}, p3 = {a6, a7}, p4 = {a8, a9}, p5 = {a10, a11}, p6 = {a12, a13}, p7 = {a14, a15}; \
    const float x = seed[8], y = seed[9];                                                         \
    (void)x; (void)y;                                                                             \
    __syncthreads();                                                                              \
    unsigned long long t0, t1, r0, r1;                                                            \
    asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(r0), "=s"(t0) :: "memory"); \
    set_exec(exec_mode);

#define EPILOGUE                                                                                  \
    asm volatile("s_mov_b64 exec, -1");                                                           \
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1), "=s"(r1) :: "memory"); \
    if ((threadIdx.x & 63) == 0) {                                                                \
        const int w = blockIdx.x * 4 + (threadIdx.x >> 6);                                        \
        out[w].cycles = t1 - t0;                                                                  \
        out[w].realtime = r1 - r0;                                                                \
    }                                                                                             \
    sink[blockIdx.x * 256 + threadIdx.x] = p0.x + p0.y + p1.x + p1.y + p2.x + p2.y + p3.x + p3.y + p4.x + p4.y + p5.x + p5.y + p6.x + p6.y + p7.x + p7.y \
        + a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + a8 + a9 + a10 + a11 + a12 + a13 + a14 + a15;

#define PAIRS "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7)
#define ACCS "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)

#define DEF_KERNEL(NAME, BODY)                                                                    \
    __global__ __launch_bounds__(256) void NAME(const float* seed, float* sink, Out* out, int exec_mode) \
    {                                                                                             \
        PROLOGUE                                                                                  \
        for (int i = 0; i < ITER; ++i) { BODY; }                                                  \
        EPILOGUE                                                                                  \
    }

// anchors: 8 accumulators, 8 x 8 instructions
#define BODY_FMA asm volatile(REP8("v_fma_f32 %0, %8, %9, %0\n\t v_fma_f32 %1, %8, %9, %1\n\t v_fma_f32 %2, %8, %9, %2\n\t v_fma_f32 %3, %8, %9, %3\n\t" \
                                   "v_fma_f32 %4, %8, %9, %4\n\t v_fma_f32 %5, %8, %9, %5\n\t v_fma_f32 %6, %8, %9, %6\n\t v_fma_f32 %7, %8, %9, %7\n\t") \
                              : ACCS : "v"(x), "v"(y))
#define BODY_MIN asm volatile(REP8("v_min_f32 %0, %8, %0\n\t v_min_f32 %1, %8, %1\n\t v_min_f32 %2, %8, %2\n\t v_min_f32 %3, %8, %3\n\t" \
                                   "v_min_f32 %4, %8, %4\n\t v_min_f32 %5, %8, %5\n\t v_min_f32 %6, %8, %6\n\t v_min_f32 %7, %8, %7\n\t") \
                              : ACCS : "v"(x))
// the exchanges: 8 pairs of registers
#define BODY_SWAP asm volatile(REP8("v_swap_b32 %0, %1\n\t v_swap_b32 %2, %3\n\t v_swap_b32 %4, %5\n\t v_swap_b32 %6, %7\n\t" \
                                    "v_swap_b32 %8, %9\n\t v_swap_b32 %10, %11\n\t v_swap_b32 %12, %13\n\t v_swap_b32 %14, %15\n\t") \
                               : ACCS, "+v"(a8), "+v"(a9), "+v"(a10), "+v"(a11), "+v"(a12), "+v"(a13), "+v"(a14), "+v"(a15))
#define PKMOV(n) "v_pk_mov_b32 %" #n ", %" #n ", %" #n " op_sel:[1,0]\n\t"
#define BODY_PKMOV asm volatile(REP8(PKMOV(0) PKMOV(1) PKMOV(2) PKMOV(3) PKMOV(4) PKMOV(5) PKMOV(6) PKMOV(7)) : PAIRS)

DEF_KERNEL(calib_v_fma_f32, BODY_FMA)
DEF_KERNEL(calib_v_min_f32, BODY_MIN)
DEF_KERNEL(calib_v_swap_b32, BODY_SWAP)
DEF_KERNEL(calib_v_pk_mov_b32, BODY_PKMOV)

// what the two instructions do: lane l holds (l, 100 + l); exec = even lanes
__global__ __launch_bounds__(64) void check_exchange(float* res)
{
    const int l = threadIdx.x;
    float a = (float)l, b = 100.f + (float)l;
    v2f p = {(float)l, 100.f + (float)l};
    asm volatile("s_mov_b32 exec_lo, 0x55555555\n\ts_mov_b32 exec_hi, 0x55555555\n\t"
                 "v_swap_b32 %0, %1\n\t"
                 "v_pk_mov_b32 %2, %2, %2 op_sel:[1,0]\n\t"
                 "s_mov_b64 exec, -1"
                 : "+v"(a), "+v"(b), "+v"(p));
    res[l] = a; res[64 + l] = b; res[128 + l] = p.x; res[192 + l] = p.y;
}

typedef void (*kern_t)(const float*, float*, Out*, int);
struct Case { const char* name; kern_t k; };

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("# device %s, %d CUs, clock %d kHz\n", prop.gcnArchName, cus, prop.clockRate);
    float h_seed[16];
    for (int i = 0; i < 16; ++i) h_seed[i] = 1.0f + 0.001f * i;
    float *d_seed, *d_sink, *d_res;
    Out* d_out;
    const int grid = cus * WPS;
    CK(hipMalloc(&d_seed, sizeof h_seed));
    CK(hipMalloc(&d_sink, (size_t)grid * 256 * 4));
    CK(hipMalloc(&d_out, (size_t)grid * 4 * sizeof(Out)));
    CK(hipMalloc(&d_res, 256 * 4));
    CK(hipMemcpy(d_seed, h_seed, sizeof h_seed, hipMemcpyHostToDevice));

    hipLaunchKernelGGL(check_exchange, dim3(1), dim3(64), 0, nullptr, d_res);
    float r[256];
    CK(hipMemcpy(r, d_res, sizeof r, hipMemcpyDeviceToHost));
    bool swap_ok = true, pk_ok = true;
    for (int l = 0; l < 64; ++l) {
        const bool on = (l & 1) == 0;
        const float lo = on ? 100.f + l : (float)l, hi = on ? (float)l : 100.f + l;
        swap_ok &= r[l] == lo && r[64 + l] == hi;
        pk_ok &= r[128 + l] == lo && r[192 + l] == hi;
    }
    printf("# exchange under exec = even lanes: v_swap_b32 %s, v_pk_mov_b32 op_sel:[1,0] %s\n",
           swap_ok ? "exchanges the active lanes only" : "DOES NOT", pk_ok ? "exchanges the active lanes only" : "DOES NOT");

    const Case cases[] = {{"v_fma_f32", calib_v_fma_f32}, {"v_min_f32", calib_v_min_f32}, {"v_swap_b32", calib_v_swap_b32},
                          {"v_pk_mov_b32 op_sel:[1,0]", calib_v_pk_mov_b32}};
    static const char* en[3] = {"all", "even", "lo32"};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("%-28s %6s %5s %13s %12s %10s %10s\n", "class", "w/SIMD", "exec", "cyc/inst/SIMD", "wall-based", "clock GHz", "wall us");
    for (const Case& c : cases)
        for (int em = 0; em < 3; ++em) {
            for (int rep = 0; rep < 3; ++rep) {      // the last repetition is reported (warm clocks)
                CK(hipEventRecord(e0, nullptr));
                hipLaunchKernelGGL(c.k, dim3(grid), dim3(256), 0, nullptr, d_seed, d_sink, d_out, em);
                CK(hipEventRecord(e1, nullptr));
                CK(hipEventSynchronize(e1));
            }
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            std::vector<Out> h((size_t)grid * 4);
            CK(hipMemcpy(h.data(), d_out, h.size() * sizeof(Out), hipMemcpyDeviceToHost));
            std::vector<double> cyc, clk;
            for (const Out& o : h) { cyc.push_back((double)o.cycles); clk.push_back((double)o.cycles / ((double)o.realtime * 10.0)); }
            std::sort(cyc.begin(), cyc.end());
            std::sort(clk.begin(), clk.end());
            const double med = cyc[cyc.size() / 2], ghz = clk[clk.size() / 2];   // s_memrealtime ticks at 100 MHz
            const double insts = (double)ITER * PER_BLOCK;
            printf("%-28s %6d %5s %13.3f %12.3f %10.3f %10.1f\n", c.name, WPS, en[em], med / (insts * WPS),
                   ms * 1e-3 * ghz * 1e9 / (insts * WPS), ghz, ms * 1e3);
        }
    return 0;
}
