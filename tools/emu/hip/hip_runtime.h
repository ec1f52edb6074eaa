// TEST HARNESS (tools/emu): a tiny single-threaded SIMT emulator that lets the unmodified kernel sources under
// atracdenc_amd/csrc be compiled for the host and stepped through lane by lane on a machine without a GPU. It is NOT part
// of the product and is never shipped in libat3hip.so. Two test modules produce results with it,
// tests/test_kernels_simt_harness.py (the encoders) and tests/test_decoders_simt_harness.py (the decoders and the resampler):
// they are the parity gate of the GPU-less suite, and the run_emu*.py scripts next to this directory are their drivers. No
// benchmark number is produced with it.
//
// Model: one workgroup at a time; each work-item is a ucontext fiber; __syncthreads() yields to a
// round-robin scheduler. __shared__ becomes `static` (one workgroup alive at a time).
//
// Checks a GPU run does not make:
//   * EMU_STRICT=1 (with the -O0 build): a cross-lane exchange reached from two different calls aborts (emu_runtime.cpp).
//   * LDS is filled with 0xCD before every workgroup, every device allocation with 0xCD when it is made.
//   * EMU_FENCE=high|low (read when the library loads; off by default): hipMalloc maps every allocation with an inaccessible
//     page directly after it (high; the size is rounded up to 4 bytes only) or directly before it (low), hipFree unmaps it.
//     A kernel that reads or writes one word outside a buffer ends the process with a signal. Host build only.
//     Under `high` an allocation is therefore aligned to 4 bytes only, where hipMalloc gives 256: alignment is given up on
//     purpose, since a buffer that ends at the page cannot also begin on a 16-byte boundary for every size. The float4 /
//     int4 of this header are plain structs and the strict build is -O0, so no access here needs more; a kernel that
//     comes to rely on a wider alignment of a device buffer would trap under `high` without being wrong.
//   * EMU_ORDER=reverse (off by default): the scheduler visits the wavefronts of a workgroup in descending order (lanes
//     inside a wavefront stay ascending: the hardware runs them in lockstep and the sources rely on it). A missing
//     __syncthreads() between a low-numbered producer wavefront and a high-numbered consumer shows in one of the two
//     orders; results must have identical bits in both.
//   * EMU_STREAMS=lazy | lazy:SEED (read when the library loads; off by default): deferred streams. Unset, every launch, copy
//     and fill runs at its call, in program order, and events and waits do nothing: a wait between two streams can be missing
//     and nothing shows. With the mode on, each stream made here, the null stream and every foreign handle is a FIFO of
//     operations (launch, memcpy_async, memset_async, event record, stream wait), executed in a legal order that is not
//     program order:
//       - launch arguments are evaluated at the call and held by value (emu_launch_by_value, in every mode);
//       - hipEventRecord queues a record; hipStreamWaitEvent takes the event's latest record AT THE CALL and is runnable once
//         that record has executed: a later record of the event does not move it, an event never recorded holds nobody up;
//       - hipStreamSynchronize(s) runs s dry and, transitively, whatever its waits need - nothing else; hipEventSynchronize
//         runs up to the record taken at the call; hipDeviceSynchronize, hipFree and hipHostFree run everything;
//         hipStreamDestroy runs that stream dry;
//       - blocking hipMemcpy / hipMemset run at once, behind the streams made WITHOUT hipStreamNonBlocking and the null stream,
//         and wait for no non-blocking stream (a caller's handle counts as non-blocking); the null stream and the blocking
//         streams run each other dry before either takes an operation;
//       - host memory: a host-to-device hipMemcpyAsync from memory that is not hipHostMalloc's is staged at the call, a
//         device-to-host one into such memory is complete, with all ahead of it on its stream, when the call returns; copies
//         from or to hipHostMalloc ranges (tracked) are deferred like a launch.
//     `lazy` executes nothing until a host-blocking call forces it. `lazy:SEED` also runs, before every enqueue, a seeded random
//     number of runnable operations of one seeded random stream, so streams run ahead of and fall behind each other. A wait
//     whose record sits behind a wait for the asking stream aborts with both streams and the event named; operations still
//     queued at exit are reported on stderr; EMU_STREAMS_LOG=<file> records each operation when it executes. EMU_TRACE lines are
//     written at the call in every mode. extern "C" emu_caller_stream_create / _destroy / _sync and emu_caller_copy give a
//     Python driver a caller's stream with a deferred copy on it (tools/emu/run_emu_streams.py); tests/host/
//     emu_streams_selftest.cpp shows on toy programs that each missing wait changes a result. LIMITS: the mode explores
//     ORDERS of whole operations - kernels never overlap, nothing has a duration - and knows nothing of hardware queues,
//     priorities or which schedule a device would really take; a clean run says that the waits suffice for the orders it
//     took (one for `lazy`, one per seed), not for all legal ones.
#pragma once
#define AT3_EMU_HOST 1
#include <ucontext.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <tuple>
#include <vector>

using std::isfinite;

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct float2 {
    float x, y;
};
struct float4 {
    float x, y, z, w;
};
static inline float2 make_float2(float x, float y) { float2 r; r.x = x; r.y = y; return r; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }


struct uint2 {
    unsigned x, y;
};
struct uint4 {
    unsigned x, y, z, w;
};
static inline uint2 make_uint2(unsigned x, unsigned y) { uint2 r; r.x = x; r.y = y; return r; }
struct int4 {
    int x, y, z, w;
};
static inline int4 make_int4(int x, int y, int z, int w) { int4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

extern dim3 threadIdx, blockIdx, blockDim, gridDim;

#define __global__
#define __device__
#define __host__
// every __shared__ object lands in one section that the scheduler poisons before each workgroup starts: a kernel that
// reads LDS it has not written sees 0xCD bytes here, not the zeros (or the previous workgroup's values) a plain static holds
#define __shared__ static __attribute__((section("emu_lds")))
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__

void emu_syncthreads();
#define __syncthreads() emu_syncthreads()

static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline unsigned int __umul24(unsigned int a, unsigned int b) { return (a & 0xffffffu) * (b & 0xffffffu); }
static inline int min(int a, int b) { return b < a ? b : a; }
// float -> int as the hardware converts (v_rndne_f32 + v_cvt_i32_f32): round to nearest even, NaN -> 0, saturation at
// INT_MIN / INT_MAX. (x86's cvtss2si answers INT_MIN for a NaN and for every value out of range: the harness must not.)
static inline int emu_cvt_i32_f32(float f) { return f != f ? 0 : f >= 2147483648.0f ? INT32_MAX : f <= -2147483648.0f ? INT32_MIN : (int)f; }
static inline int __float2int_rn(float f) { return emu_cvt_i32_f32(nearbyintf(f)); }
static inline int __float2int_rz(float f) { return emu_cvt_i32_f32(f); }
static inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
template <typename T, typename U> static inline T atomicAdd(T* p, U v) { T o = *p; *p = o + (T)v; return o; }
template <typename T> static inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
template <typename T> static inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }

typedef int hipError_t;
template <typename F> static inline int hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, F, int, size_t) { *n = 3; return 0; }
enum { hipSuccess = 0, hipErrorUnknown = 1 };
typedef void* hipStream_t;
typedef struct emu_event* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };

static inline const char* hipGetErrorString(hipError_t) { return "emu error"; }
static inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
static inline hipError_t hipSetDevice(int) { return hipSuccess; }
static inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
// Streams, events and everything queued on them are out of line (emu_runtime.cpp): every stream and event is an object of its
// own, and with EMU_TRACE=<file> in the environment when the library loads each of these calls appends one line to that file
// (streams and events by their ordinal in creation order, byte counts, launch geometry; never a pointer). A stream handle that
// was not made here - a caller's - is traced as `caller`. tools/emu/run_emu_trace.py pins the host code's call sequence with it.
// The priority range is 0 (lowest) .. -1, so that a trace tells a low-priority stream from a high-priority one.
#define hipStreamNonBlocking 1
#define hipEventDisableTiming 2
static inline hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s);
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags);
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipDeviceSynchronize();
hipError_t hipEventCreate(hipEvent_t* e);
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned);
static inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
// device allocations: poisoned with 0xCD, and under EMU_FENCE placed against a guard page (emu_runtime.cpp)
// (C linkage: tools/emu/run_emu_decode.py allocates exactly-sized caller buffers with them, which the product's own
// allocations, padded by dev_alloc, are not)
extern "C" void* emu_device_alloc(size_t n);
extern "C" void emu_device_free(void* p);
extern "C" void emu_fail_alloc_after(long n);   // n more allocations succeed, the later ones are refused (n < 0: none is)
hipError_t hipMalloc(void** p, size_t n);
#define hipHostMallocDefault 0u
hipError_t hipHostMalloc(void** p, size_t n, unsigned);   // (EMU_STREAMS tracks these ranges: copies from or to them are deferred)
hipError_t hipHostFree(void* p);
hipError_t hipFree(void* p);
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t st);
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st);
hipError_t hipMemset(void* d, int v, size_t n);
struct hipDeviceProp_t { int multiProcessorCount; size_t maxSharedMemoryPerMultiProcessor; };
static inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) { p->multiProcessorCount = 4; p->maxSharedMemoryPerMultiProcessor = 160u * 1024u; return hipSuccess; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipDeviceGetPCIBusId(char* id, int len, int) { if (len > 0) id[0] = 0; return hipErrorUnknown; }

// ---- wave-level (64 lanes) cross-lane primitives: implemented with a wave-wide rendezvous ----
unsigned emu_wave_exchange(unsigned value, unsigned* all64);   // deposit `value`, returns active mask lo; all64 = values
unsigned long long emu_ballot(bool pred);
#define __ballot(pred) emu_ballot(pred)
int emu_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl);
int emu_bpermute(int addr, int v);
#define __builtin_amdgcn_ds_bpermute(addr, v) emu_bpermute((int)(addr), (int)(v))
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) emu_update_dpp((int)(old), (int)(src), (ctrl), (rm), (bm), (bc))
int emu_readlane(int v, int lane);
#define __builtin_amdgcn_readlane(v, lane) emu_readlane((int)(v), (lane))
static inline __attribute__((always_inline)) float __shfl(float v, int lane, int = 64) { float r; int i; memcpy(&i, &v, 4); i = emu_readlane(i, lane); memcpy(&r, &i, 4); return r; }
static inline __attribute__((always_inline)) float __shfl_xor(float v, int mask, int = 64) { return __shfl(v, (int)((threadIdx.x & 63u) ^ (unsigned)mask)); }
// v_permlane32_swap / v_permlane16_swap (gfx950): returns {a', b'}
typedef int emu_int2 __attribute__((ext_vector_type(2)));
static inline __attribute__((always_inline)) emu_int2 __builtin_amdgcn_permlane32_swap(int a, int b, bool, bool)
{
    const int ln = (int)(threadIdx.x & 63u);
    const int pa = emu_bpermute(4 * (ln ^ 32), a), pb = emu_bpermute(4 * (ln ^ 32), b);
    emu_int2 r;
    if (ln < 32) { r[0] = a; r[1] = pa; } else { r[0] = pb; r[1] = b; }
    return r;
}
static inline __attribute__((always_inline)) emu_int2 __builtin_amdgcn_permlane16_swap(int a, int b, bool, bool)
{
    const int ln = (int)(threadIdx.x & 63u);
    const int pa = emu_bpermute(4 * (ln ^ 16), a), pb = emu_bpermute(4 * (ln ^ 16), b);
    emu_int2 r;
    if ((ln & 16) == 0) { r[0] = a; r[1] = pa; } else { r[0] = pb; r[1] = b; }
    return r;
}
void emu_wave_barrier();
#define __builtin_amdgcn_wave_barrier() emu_wave_barrier()
#define __builtin_amdgcn_fence(order, scope) ((void)0)
static inline unsigned __builtin_amdgcn_readfirstlane(unsigned v) { return v; }
#define __builtin_amdgcn_s_setprio(x) ((void)0)
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
static inline unsigned long long __builtin_amdgcn_s_memtime() { return 0ull; }
static inline unsigned long long __builtin_amdgcn_s_memrealtime() { return 0ull; }
static inline unsigned __builtin_amdgcn_mbcnt_lo(unsigned mask, unsigned v) { const unsigned ln = threadIdx.x & 63u; return v + (unsigned)__builtin_popcount(mask & (ln >= 32 ? 0xffffffffu : ((1u << ln) - 1u))); }
static inline unsigned __builtin_amdgcn_mbcnt_hi(unsigned mask, unsigned v) { const unsigned ln = threadIdx.x & 63u; return v + (ln > 32 ? (unsigned)__builtin_popcount(mask & ((1u << (ln - 32)) - 1u)) : 0u); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }

void emu_launch(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const std::function<void()>& body);
// The arguments are evaluated and converted to the kernel's parameter types when the launch is called and travel by value: under
// EMU_STREAMS the body runs later, when the caller's locals are gone. (`kernel` may be a parenthesised template name.)
template <typename... P, typename... A>
static inline void emu_launch_by_value(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, void (*kernel)(P...), A&&... args)
{
    std::tuple<std::decay_t<P>...> held(std::forward<A>(args)...);
    emu_launch(name, grid, block, lds_bytes, stream, [kernel, held]() { std::apply(kernel, held); });
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
    emu_launch_by_value(#kernel, (grid), (block), (shmem), (stream), kernel, ##__VA_ARGS__)
