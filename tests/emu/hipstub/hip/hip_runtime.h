// Stand-in for <hip/hip_runtime.h>: what parsnp_amd/csrc/engine/gapalign_hip.hip needs to compile and run for the HOST
// (tests/emu/gap_emu.cpp includes that file unchanged, with this directory first on the include path).  Device memory is
// host memory, a stream runs at once, and a launch runs its workgroups one after the other: the lanes of a workgroup are
// fibers that switch only where the device's lanes meet -- __syncthreads, the wave barrier, shuffles and ballots
// (gap_emu.cpp holds the scheduler).  Only launches of 256 threads run; any other launch is an error (see gap_emu.cpp).
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>

#define __global__
#define __device__
#define __host__
#define __constant__
#define __shared__
#define __launch_bounds__(...)
#define __align__(n) alignas(n)
#define HIP_SYMBOL(x) (&(x))

struct gap_emu_idx { unsigned x, y, z; };
extern gap_emu_idx threadIdx, blockIdx;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };

namespace {      // the dynamic LDS of the kernels (`extern __shared__` at block scope names these): one workgroup runs at a time
alignas(16) uint8_t rows_lds[160 * 1024];
alignas(16) uint8_t long_lds[160 * 1024];
}

// ---- the scheduler's side (gap_emu.cpp)
enum { GAP_EMU_WAVE = 1, GAP_EMU_BLOCK = 2 };
void gap_emu_yield(int kind);                    // this lane waits for its wavefront / its workgroup
uint32_t* gap_emu_exchange();                    // 64 words of this lane's wavefront for the shuffle in flight (flips per call)
int gap_emu_lane_live(int lane);                 // the lane of this wavefront has not returned from the kernel
int gap_emu_launch(unsigned blocks, unsigned threads, const std::function<void()>& body);

// ---- lane intrinsics
inline unsigned __lane_id() { return threadIdx.x & 63u; }
template <class T> inline T gap_emu_shfl_from(T v, int src) {
    static_assert(sizeof(T) == 4, "32-bit shuffles");
    uint32_t* x = gap_emu_exchange();
    uint32_t w; memcpy(&w, &v, 4);
    x[threadIdx.x & 63u] = w;
    gap_emu_yield(GAP_EMU_WAVE);
    if (src < 0 || src > 63 || !gap_emu_lane_live(src)) return v;
    w = x[src]; T r; memcpy(&r, &w, 4);
    return r;
}
template <class T> inline T __shfl(T v, int src, int = 64) { return gap_emu_shfl_from(v, src); }
template <class T> inline T __shfl_xor(T v, int d, int = 64) { return gap_emu_shfl_from(v, (int)(threadIdx.x & 63u) ^ d); }
template <class T> inline T __shfl_up(T v, int d, int = 64) { const int l = (int)(threadIdx.x & 63u); return gap_emu_shfl_from(v, l - d < 0 ? l : l - d); }
inline unsigned long long __ballot(int pred) {
    uint32_t* x = gap_emu_exchange();
    x[threadIdx.x & 63u] = pred ? 1u : 0u;
    gap_emu_yield(GAP_EMU_WAVE);
    unsigned long long m = 0;
    for (int l = 0; l < 64; l++) if (gap_emu_lane_live(l) && x[l]) m |= 1ull << l;
    return m;
}
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline float __int_as_float(int v) { float f; memcpy(&f, &v, 4); return f; }
inline int __float_as_int(float f) { int v; memcpy(&v, &f, 4); return v; }
inline void __syncthreads() { gap_emu_yield(GAP_EMU_BLOCK); }
inline void __threadfence_block() {}
inline long long clock64() { return 0; }
#define __builtin_amdgcn_s_waitcnt(x) ((void)0)
#define __builtin_amdgcn_wave_barrier() gap_emu_yield(GAP_EMU_WAVE)
#define __builtin_amdgcn_readfirstlane(x) (x)      // every use is of a value the lanes hold alike (gapalign_hip.hip: uni)
template <class T> inline T atomicAdd(T* p, T v) { const T old = *p; *p = old + v; return old; }      // one lane runs at a time

// ---- the runtime
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum { hipStreamNonBlocking = 1, hipHostMallocMapped = 2, hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef void* hipStream_t;
struct gap_emu_event { double t; };
typedef gap_emu_event* hipEvent_t;
struct hipDeviceProp_t { int multiProcessorCount; };
extern hipError_t gap_emu_last_error;

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : (e == hipErrorOutOfMemory ? "out of memory" : "invalid value (the emulation runs launches of 256 threads only)"); }
inline hipError_t hipGetLastError() { const hipError_t e = gap_emu_last_error; gap_emu_last_error = hipSuccess; return e; }
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) { const char* e = getenv("PM_GAP_EMU_CUS"); p->multiProcessorCount = e && atoi(e) > 0 ? atoi(e) : 256; return hipSuccess; }
// device memory comes back filled with 0xCD: what a kernel reads before it has written it shows in the rows
inline hipError_t hipMalloc(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 1); if (!*p) return hipErrorOutOfMemory; memset(*p, 0xCD, bytes); return hipSuccess; }
template <class T> inline hipError_t hipMalloc(T** p, size_t bytes) { return hipMalloc((void**)p, bytes); }
inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
inline hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (void*)1; return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
inline hipError_t hipMemcpyToSymbol(void* sym, const void* s, size_t n) { memcpy(sym, s, n); return hipSuccess; }
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
inline double gap_emu_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = new gap_emu_event{0}; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->t = gap_emu_now(); return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { *ms = (float)((b->t - a->t) * 1e3); return hipSuccess; }
template <class K, class... A>
inline void hipLaunchKernelGGL(K kernel, dim3 grid, dim3 block, size_t, hipStream_t, A... args) {
    gap_emu_last_error = gap_emu_launch(grid.x, block.x, [=]() { kernel(args...); });
}
