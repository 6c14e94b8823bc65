// Micro-benchmark behind the launch shape of unary_f64_kernel (csrc/expr.hip): the same Float64 -> Float64 map over 10^8 rows in
// several access patterns (A: 16 bytes per lane, one load in flight, 4 / 8 / 16 workgroups per CU, non-temporal or plain stores;
// B: two or four loads in flight per lane; C: the stack machine's pattern, four 8-byte rows per lane), median of 20 launches.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/unary_kernel_bench.hip -o tools/unary_kernel_bench
// Results: profiles/unary/kernel_variants.txt.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
#include <cstdint>
#include <cmath>
typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
template <int F> __device__ __forceinline__ u64 f(u64 w) {
    if (F == 0) return w & 0x7fffffffffffffffull;
    if (F == 1) return (u64)__double_as_longlong(sin(__longlong_as_double((long long)w)));
    return (u64)__double_as_longlong(__longlong_as_double((long long)w) * 2.0);
}
template <int F, bool NT>
__global__ void __launch_bounds__(256) kA(const u64 *__restrict__ in, u64 *__restrict__ out, int64_t pairs, int64_t n) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, first = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const u64x2 *in2 = (const u64x2 *)in; u64x2 *out2 = (u64x2 *)out;
    for (int64_t j = first; j < pairs; j += stride) {
        u64x2 v = __builtin_nontemporal_load(in2 + j);
        v.x = f<F>(v.x); v.y = f<F>(v.y);
        if (NT) __builtin_nontemporal_store(v, out2 + j); else out2[j] = v;
    }
    for (int64_t j = 2 * pairs + first; j < n; j += stride) out[j] = f<F>(in[j]);
}
template <int F, int U>
__global__ void __launch_bounds__(256) kB(const u64 *__restrict__ in, u64 *__restrict__ out, int64_t pairs, int64_t n) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, first = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const u64x2 *in2 = (const u64x2 *)in; u64x2 *out2 = (u64x2 *)out;
    int64_t j = first;
    for (; j + (U - 1) * stride < pairs; j += U * stride) {
        u64x2 v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = __builtin_nontemporal_load(in2 + j + k * stride);
#pragma unroll
        for (int k = 0; k < U; ++k) { v[k].x = f<F>(v[k].x); v[k].y = f<F>(v[k].y); __builtin_nontemporal_store(v[k], out2 + j + k * stride); }
    }
    for (; j < pairs; j += stride) { u64x2 v = __builtin_nontemporal_load(in2 + j); v.x = f<F>(v.x); v.y = f<F>(v.y); __builtin_nontemporal_store(v, out2 + j); }
    for (int64_t t = 2 * pairs + first; t < n; t += stride) out[t] = f<F>(in[t]);
}
// the stack machine's access pattern: a wave walks 256-row chunks, a lane owns rows chunk + r*64 + lane (8-byte accesses)
template <int F>
__global__ void __launch_bounds__(256) kC(const u64 *__restrict__ in, u64 *__restrict__ out, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (n + 255) / 256, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t c = wave; c < n_chunks; c += n_waves) {
        const int64_t row0 = c * 256 + lane;
        u64 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = __builtin_nontemporal_load(in + std::min<int64_t>(row0 + r * 64, n - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) if (row0 + r * 64 < n) __builtin_nontemporal_store(f<F>(v[r]), out + row0 + r * 64);
    }
}
int main() {
    const int64_t n = 100000000;
    hipDeviceProp_t p; CK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    u64 *in, *out; CK(hipMalloc(&in, n * 8)); CK(hipMalloc(&out, n * 8));
    std::vector<double> h(n); for (int64_t i = 0; i < n; ++i) h[i] = double((i * 2654435761u) % 200001) / 1000.0 - 100.0;
    CK(hipMemcpy(in, h.data(), n * 8, hipMemcpyHostToDevice));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto grid = [&](int64_t items, int bpc) { int64_t need = (items + 255) / 256, cap = int64_t(cus) * bpc; return (unsigned)std::min(need, cap); };
    auto timeit = [&](const char *name, auto launch) {
        std::vector<float> t;
        for (int i = 0; i < 25; ++i) { (void)hipEventRecord(a); launch(); (void)hipEventRecord(b); (void)hipEventSynchronize(b); float ms; (void)hipEventElapsedTime(&ms, a, b); if (i >= 5) t.push_back(ms); }
        std::sort(t.begin(), t.end());
        printf("%-44s median %.4f min %.4f max %.4f ms\n", name, t[t.size() / 2], t.front(), t.back());
    };
    for (int round = 0; round < 2; ++round) {
    printf("cus %d round %d\n", cus, round);
    timeit("A abs 16B 1 pair/iter nt-store 8 blk/CU", [&] { kA<0, true><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("A sin (same)", [&] { kA<1, true><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("A mul2 (same)", [&] { kA<2, true><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("A abs plain store", [&] { kA<0, false><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("A abs 16 blk/CU", [&] { kA<0, true><<<grid(n / 2, 16), 256>>>(in, out, n / 2, n); });
    timeit("A abs 4 blk/CU", [&] { kA<0, true><<<grid(n / 2, 4), 256>>>(in, out, n / 2, n); });
    timeit("B abs unroll 2", [&] { kB<0, 2><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("B abs unroll 4", [&] { kB<0, 4><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("B sin unroll 2", [&] { kB<1, 2><<<grid(n / 2, 8), 256>>>(in, out, n / 2, n); });
    timeit("C abs stack-machine pattern 8B x4", [&] { kC<0><<<grid((n + 3) / 4, 8), 256>>>(in, out, n); });
    timeit("C mul2 stack-machine pattern 8B x4", [&] { kC<2><<<grid((n + 3) / 4, 8), 256>>>(in, out, n); });
    }
    CK(hipDeviceSynchronize());
    return 0;
}
