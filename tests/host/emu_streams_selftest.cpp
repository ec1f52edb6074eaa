// TEST HARNESS self-test (no product code): toy stream programs for the SIMT harness's deferred-stream mode (EMU_STREAMS,
// tools/emu/hip/hip_runtime.h). Each pattern runs in an unguarded form, whose result depends on the order in which the queued
// operations execute, and in a guarded one, whose result does not. The program prints one line `name form value` per run;
// tests/test_emu_streams_selftest.py runs it eagerly, under `lazy` and under seeds, and compares the lines: the unguarded
// forms are the proof that the mode can show a missing wait, the guarded ones that it shows nothing where nothing is missing.
// An unguarded form races on memory the program owns and nothing more. `--leave-queued` ends with operations still queued.
#include "hip/hip_runtime.h"

#include <cinttypes>

extern "C" size_t emu_streams_queued();

__global__ void k_fill(int* p, int n, int v)
{
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) p[i] = v;
}
__global__ void k_copy(int* dst, const int* src, int n)
{
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) dst[i] = src[i];
}

namespace {
constexpr int N = 96;        // one and a half wavefronts, two workgroups
constexpr int ROUNDS = 16;   // repetitions of a pattern: a seeded schedule may happen to keep program order in some of them

void fill(hipStream_t s, int* p, int v) { hipLaunchKernelGGL(k_fill, dim3(2), dim3(64), 0, s, p, N, v); }
void copy(hipStream_t s, int* d, const int* src) { hipLaunchKernelGGL(k_copy, dim3(2), dim3(64), 0, s, d, src, N); }

uint64_t digest(const int* p, int n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int i = 0; i < n; ++i) h = (h ^ (uint32_t)p[i]) * 0x100000001b3ull;
    return h;
}
void report(const char* name, bool guarded, uint64_t v) { printf("%s %s %016" PRIx64 "\n", name, guarded ? "guarded" : "unguarded", v); }

int* dev(int n, int v)
{
    int* p = nullptr;
    if (hipMalloc((void**)&p, sizeof(int) * (size_t)n) != hipSuccess) abort();
    hipMemset(p, 0, sizeof(int) * (size_t)n);
    for (int i = 0; i < n; ++i) p[i] = v;   // (harness memory is host memory)
    return p;
}
hipStream_t stream(bool non_blocking = true)
{
    hipStream_t s;
    if (non_blocking) hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    else hipStreamCreate(&s);
    return s;
}

// 1. a producer kernel on one stream, its consumer on another
void producer_consumer(bool guarded)
{
    hipStream_t a = stream(), b = stream();
    hipEvent_t e[ROUNDS];
    int* buf = dev(N * ROUNDS, 0);
    int* out = dev(N * ROUNDS, -1);
    for (int r = 0; r < ROUNDS; ++r) {
        hipEventCreateWithFlags(&e[r], hipEventDisableTiming);
        fill(a, buf + r * N, r + 1);
        if (guarded) { hipEventRecord(e[r], a); hipStreamWaitEvent(b, e[r], 0); }
        copy(b, out + r * N, buf + r * N);
    }
    hipStreamSynchronize(b);
    report("producer_consumer", guarded, digest(out, N * ROUNDS));
    hipStreamSynchronize(a);
    for (int r = 0; r < ROUNDS; ++r) hipEventDestroy(e[r]);
    hipStreamDestroy(a); hipStreamDestroy(b);
    hipFree(buf); hipFree(out);
}

// 2. write after read on a two-slot buffer, three queued rounds: the producer's round r may overwrite slot r % 2 only when the
// consumer has read round r - 2 from it. Both forms order the reads behind the writes; the unguarded one lacks the way back.
void two_slots(bool guarded)
{
    uint64_t h = 0;
    for (int rep = 0; rep < ROUNDS; ++rep) {
        hipStream_t p = stream(), c = stream();
        hipEvent_t filled[3], consumed[3];
        int* slot = dev(N * 2, 0);
        int* out = dev(N * 3, -1);
        for (int r = 0; r < 3; ++r) {
            hipEventCreateWithFlags(&filled[r], hipEventDisableTiming);
            hipEventCreateWithFlags(&consumed[r], hipEventDisableTiming);
            if (guarded && r >= 2) hipStreamWaitEvent(p, consumed[r - 2], 0);
            fill(p, slot + (r % 2) * N, 100 * rep + r + 1);
            hipEventRecord(filled[r], p);
            hipStreamWaitEvent(c, filled[r], 0);
            copy(c, out + r * N, slot + (r % 2) * N);
            hipEventRecord(consumed[r], c);
        }
        hipStreamSynchronize(p);   // the producer is asked first: whatever lets it run ahead, it does
        hipStreamSynchronize(c);
        h = h * 31 + digest(out, N * 3);
        for (int r = 0; r < 3; ++r) { hipEventDestroy(filled[r]); hipEventDestroy(consumed[r]); }
        hipStreamDestroy(p); hipStreamDestroy(c);
        hipFree(slot); hipFree(out);
    }
    report("two_slots", guarded, h);
}

// 3. the host overwrites the source of a queued host-to-device copy before it waits for the stream: a page-locked source is read
// when the copy executes (unguarded), a pageable one when the call is made (guarded)
void host_source(bool pageable)
{
    hipStream_t s = stream();
    int* h = nullptr;
    if (pageable) h = (int*)malloc(sizeof(int) * N);
    else hipHostMalloc((void**)&h, sizeof(int) * N, hipHostMallocDefault);
    int* d = dev(N, 0);
    for (int i = 0; i < N; ++i) h[i] = 1;
    hipMemcpyAsync(d, h, sizeof(int) * N, hipMemcpyHostToDevice, s);
    for (int i = 0; i < N; ++i) h[i] = 2;
    hipStreamSynchronize(s);
    report("host_source", pageable, digest(d, N));
    // and the way back: into pageable memory the copy is complete when the call returns, with the kernel ahead of it
    int* back = (int*)malloc(sizeof(int) * N);
    for (int i = 0; i < N; ++i) back[i] = -1;
    fill(s, d, 9);
    hipMemcpyAsync(back, d, sizeof(int) * N, hipMemcpyDeviceToHost, s);
    report(pageable ? "pageable_d2h_complete_at_return_2" : "pageable_d2h_complete_at_return_1", true, digest(back, N));
    hipStreamSynchronize(s);
    free(back);
    if (pageable) free(h); else hipHostFree(h);
    hipStreamDestroy(s);
    hipFree(d);
}

// 4. a wait takes the record that was the event's latest when the wait was called: a later record of the same event does not
// move it, and an event that was never recorded holds nobody up
void wait_then_rerecord()
{
    hipStream_t a = stream(), b = stream();
    hipEvent_t e, never;
    hipEventCreateWithFlags(&e, hipEventDisableTiming);
    hipEventCreateWithFlags(&never, hipEventDisableTiming);
    int* first = dev(N, 0);
    int* second = dev(N, 0);
    int* out = dev(N * 2, -1);
    fill(a, first, 1);
    hipEventRecord(e, a);
    hipStreamWaitEvent(b, e, 0);
    hipStreamWaitEvent(b, never, 0);
    fill(a, second, 2);
    hipEventRecord(e, a);            // behind the wait: not what b waits for
    copy(b, out, first);
    hipStreamSynchronize(b);
    hipEventRecord(never, a);
    report("wait_before_rerecord_first", true, digest(out, N));   // ordered by the wait: 1 in every mode
    // `second` is not ordered against b: under `lazy` stream a has run as far as the first record and no further
    printf("wait_before_rerecord_left_on_a count %zu\n", emu_streams_queued());
    hipStreamSynchronize(a);
    hipEventSynchronize(e);
    report("wait_before_rerecord_second", true, digest(second, N));
    hipEventDestroy(e); hipEventDestroy(never);
    hipStreamDestroy(a); hipStreamDestroy(b);
    hipFree(first); hipFree(second); hipFree(out);
}

// 5. a blocking hipMemcpy waits for no non-blocking stream (unguarded); it does wait for a stream made without the flag, and a
// stream that was synchronised has nothing left (both guarded)
void blocking_copy(int form)
{
    hipStream_t s = stream(form != 1);
    int* d = dev(N, 0);
    int h[N];
    fill(s, d, 5);
    if (form == 2) hipStreamSynchronize(s);
    hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    report(form == 0 ? "blocking_copy_nonblocking_stream" : form == 1 ? "blocking_copy_blocking_stream" : "blocking_copy_after_sync", form != 0, digest(h, N));
    hipStreamSynchronize(s);
    hipStreamDestroy(s);
    hipFree(d);
}

// 6. launch arguments are evaluated when the launch is called
void arguments_by_value()
{
    hipStream_t s = stream();
    int* d = dev(N, 0);
    {
        int v = 3;
        int* p = d;
        fill(s, p, v);
        v = 4; p = nullptr;
        (void)v; (void)p;
    }
    hipStreamSynchronize(s);
    report("arguments_by_value", true, digest(d, N));
    hipStreamDestroy(s);
    hipFree(d);
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--leave-queued")) {
        hipStream_t s = stream();
        int* d = dev(N, 0);
        fill(s, d, 1);
        printf("left queued %zu\n", emu_streams_queued());
        return 0;
    }
    for (int g = 0; g < 2; ++g) {
        producer_consumer(g != 0);
        two_slots(g != 0);
        host_source(g != 0);
    }
    wait_then_rerecord();
    for (int form = 0; form < 3; ++form) blocking_copy(form);
    arguments_by_value();
    printf("SELFTEST DONE\n");
    return 0;
}
