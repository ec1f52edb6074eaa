// DEVELOPMENT HARNESS ONLY - see hip/hip_runtime.h in this directory.
#include "hip/hip_runtime.h"
#include <dlfcn.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdarg>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
// k_alloc_pack's harness-only counters (at3_k_alloc.hpp: AT3_STAT)
extern "C" { unsigned long long g_alloc_stats[16] = {0}; }

dim3 threadIdx, blockIdx, blockDim, gridDim;

extern "C" char __start_emu_lds[] __attribute__((weak)), __stop_emu_lds[] __attribute__((weak));

namespace {
struct Fiber {
    ucontext_t ctx;
    char* stack = nullptr;
    bool done = false;
    const char* wait = "";   // what the work-item waits in, and where it was called from (deadlock report)
    void* wait_pc = nullptr;
    void* hist[16] = {};   // the last call sites, newest at hist_n % 16
    unsigned long long hist_n = 0;
};
constexpr size_t kStack = 256 * 1024;
std::vector<Fiber> g_fibers;
struct FiberStacks {   // (defined behind g_fibers: runs before the vector goes, so a leak check at exit sees the product's leaks only)
    ~FiberStacks() { for (Fiber& f : g_fibers) free(f.stack); }
} g_fiber_stacks;
ucontext_t g_main;
const std::function<void()>* g_body = nullptr;
int g_cur = -1;
unsigned g_nthr = 0;

// block barrier state
unsigned g_live = 0, g_bar_arrived = 0, g_bar_gen = 0;
// per-wave rendezvous state
struct Wave {
    unsigned live = 0, arrived = 0, gen = 0;
    unsigned slot[64];
    void* site[64];
    bool present[64];
    unsigned snap[64];
    bool snap_present[64];
};
std::vector<Wave> g_waves;

// EMU_FENCE: 0 off, 1 high (guard page directly after the allocation), 2 low (directly before it)
int fence_mode()
{
    static const int mode = [] {
        const char* e = getenv("EMU_FENCE");
        if (!e || !*e) return 0;
        if (!strcmp(e, "high")) return 1;
        if (!strcmp(e, "low")) return 2;
        fprintf(stderr, "emu: EMU_FENCE must be high or low, not '%s'\n", e);
        abort();
    }();
    return mode;
}
// EMU_ORDER=reverse: the wavefronts of a workgroup are visited in descending order
bool reverse_order()
{
    static const bool rev = [] {
        const char* e = getenv("EMU_ORDER");
        if (!e || !*e) return false;
        if (!strcmp(e, "reverse")) return true;
        fprintf(stderr, "emu: EMU_ORDER must be reverse, not '%s'\n", e);
        abort();
    }();
    return rev;
}
struct Mapping {
    void* base;
    size_t bytes;
};
std::map<void*, Mapping> g_fenced;   // allocation -> its mapping (guard page included)
std::mutex g_fenced_mu;

void yield_to_scheduler() { swapcontext(&g_fibers[g_cur].ctx, &g_main); }

void trampoline()
{
    (*g_body)();
    Fiber& f = g_fibers[g_cur];
    f.done = true;
    --g_live;
    Wave& w = g_waves[g_cur / 64];
    --w.live;
    // a finished work-item no longer takes part in barriers: release waiters if it was the last one missing
    if (g_live > 0 && g_bar_arrived == g_live) { g_bar_arrived = 0; ++g_bar_gen; }
    if (w.live > 0 && w.arrived == w.live) {
        memcpy(w.snap, w.slot, sizeof(w.slot)); memcpy(w.snap_present, w.present, sizeof(w.present));
        memset(w.present, 0, sizeof(w.present)); w.arrived = 0; ++w.gen;
    }
    swapcontext(&f.ctx, &g_main);
}
}  // namespace

// emu_fail_alloc_after(n): n more device allocations succeed, every later one is refused (n < 0: none is). A stand-alone
// program walks the *_create paths that destroy a half-made context with it (tests/host/test_host_shim_s16.cpp).
static long g_allocs_left = -1;
extern "C" void emu_fail_alloc_after(long n) { g_allocs_left = n; }

void* emu_device_alloc(size_t n)
{
    if (g_allocs_left == 0) return nullptr;
    if (g_allocs_left > 0) --g_allocs_left;
    const int mode = fence_mode();
    if (mode == 0) {
        void* p = malloc(n);
        if (p) memset(p, 0xCD, n);
        return p;
    }
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    const size_t body = mode == 1 ? (n + 3) / 4 * 4 : n;   // high: a word past the request is the guard page already
    const size_t body_pages = (body + page - 1) / page * page + (body == 0 ? page : 0);
    char* base = (char*)mmap(nullptr, body_pages + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == (char*)MAP_FAILED) return nullptr;
    char* guard = mode == 1 ? base + body_pages : base;
    char* first = mode == 1 ? base : base + page;
    memset(first, 0xCD, body_pages);
    if (mprotect(guard, page, PROT_NONE) != 0) { munmap(base, body_pages + page); return nullptr; }
    void* p = mode == 1 ? (void*)(guard - body) : (void*)first;
    std::lock_guard<std::mutex> lock(g_fenced_mu);
    g_fenced[p] = Mapping{base, body_pages + page};
    return p;
}

void emu_device_free(void* p)
{
    if (!p) return;
    if (fence_mode() == 0) { free(p); return; }
    std::lock_guard<std::mutex> lock(g_fenced_mu);
    auto it = g_fenced.find(p);
    if (it == g_fenced.end()) { fprintf(stderr, "emu: hipFree of %p, which hipMalloc did not return\n", p); abort(); }
    munmap(it->second.base, it->second.bytes);
    g_fenced.erase(it);
}

// ---- streams, events, copies: objects of their own, and the EMU_TRACE call trace (hip/hip_runtime.h) ----
struct emu_event {
    int ordinal;
    unsigned long long last_rec;   // (EMU_STREAMS) the most recent record of this event that was called, 0: none yet
};
namespace {
std::mutex g_trace_mu;
std::map<void*, int> g_streams;       // the streams made here -> ordinal in creation order
std::map<void*, size_t> g_alloc_bytes;   // (traced runs only) what hipFree gives back
int g_n_streams = 0, g_n_events = 0;

FILE* trace_file()
{
    static FILE* f = [] {
        const char* e = getenv("EMU_TRACE");
        return (e && *e) ? fopen(e, "a") : (FILE*)nullptr;
    }();
    return f;
}
void trace(const char* fmt, ...)
{
    FILE* f = trace_file();
    if (!f) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    fputc('\n', f);
    fflush(f);
}
std::string sname(hipStream_t s)
{
    std::lock_guard<std::mutex> lock(g_trace_mu);
    auto it = g_streams.find(s);
    return it == g_streams.end() ? std::string(s ? "caller" : "null") : "s" + std::to_string(it->second);
}
std::string ename(hipEvent_t e) { return e ? "e" + std::to_string(e->ordinal) : std::string("null"); }
const char* kname(hipMemcpyKind k) { return k == hipMemcpyHostToDevice ? "h2d" : k == hipMemcpyDeviceToHost ? "d2h" : "d2d"; }

// ---- EMU_STREAMS=lazy | lazy:SEED: every stream is a queue, executed in a legal order that is not program order ----
// (hip/hip_runtime.h has the semantics.) One lock guards all of it; an operation's body never calls back into the runtime.
struct StreamsMode {
    int mode = 0;   // 0 eager (today's behaviour), 1 lazy, 2 lazy with a seeded scheduler
    unsigned long long rng = 0;
};
const StreamsMode& streams_mode_init()
{
    static const StreamsMode m = [] {
        StreamsMode r;
        const char* e = getenv("EMU_STREAMS");
        if (!e || !*e) return r;
        if (!strcmp(e, "lazy")) { r.mode = 1; return r; }
        char* end = nullptr;
        if (!strncmp(e, "lazy:", 5) && e[5]) {
            r.rng = strtoull(e + 5, &end, 10) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
            if (end && !*end) { r.mode = 2; return r; }
        }
        fprintf(stderr, "emu: EMU_STREAMS must be lazy or lazy:SEED, not '%s'\n", e);
        abort();
    }();
    return m;
}
unsigned long long g_rng = 0;
unsigned rnd(unsigned n)   // splitmix64
{
    unsigned long long z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 16) % n;
}
struct Op {
    enum Kind { WORK, RECORD, WAIT } kind;
    std::function<void()> run;        // WORK: a launch, a copy or a fill
    unsigned long long rec = 0;       // RECORD: its id; WAIT: the record captured when the wait was called (never 0 in a queue)
    std::string what;                 // as the trace line names it
};
struct Queue {
    std::deque<Op> ops;
    bool blocking = false;   // made without hipStreamNonBlocking, or the null stream: a blocking hipMemcpy / hipMemset waits for it
    bool forcing = false;    // its head wait is being served further up the call stack
    std::string name;
};
std::recursive_mutex g_lazy_mu;
std::map<void*, Queue> g_queues;                     // stream handle (nullptr: the null stream) -> queue, made on first use
std::map<unsigned long long, void*> g_pending_recs;  // records that are queued and have not executed -> their stream
unsigned long long g_n_recs = 0;
std::map<char*, size_t> g_pinned;                    // the hipHostMalloc ranges

int lazy_mode()
{
    static const int mode = [] { const StreamsMode& m = streams_mode_init(); g_rng = m.rng; return m.mode; }();
    return mode;
}
FILE* order_log()   // EMU_STREAMS_LOG=<file>: one line per operation when it executes, i.e. the order that was explored
{
    static FILE* f = [] {
        const char* e = getenv("EMU_STREAMS_LOG");
        return (e && *e) ? fopen(e, "a") : (FILE*)nullptr;
    }();
    return f;
}
Queue& queue_of(hipStream_t s)
{
    auto it = g_queues.find(s);
    if (it != g_queues.end()) return it->second;
    Queue& q = g_queues[s];
    q.name = sname(s);
    q.blocking = s == nullptr;   // a caller's stream counts as non-blocking: nothing waits for it that was not told to
    return q;
}
bool pinned(const void* p, size_t n)
{
    auto it = g_pinned.upper_bound((char*)p);
    if (it == g_pinned.begin()) return false;
    --it;
    return (char*)p + n <= it->first + it->second;
}
void force_record(unsigned long long rec, const Queue& for_q);
// executes the head of q; a head that waits for a record still queued runs that record's stream first, as far as the record
void step(Queue& q)
{
    Op& head = q.ops.front();
    if (head.kind == Op::WAIT && g_pending_recs.count(head.rec)) {
        q.forcing = true;
        force_record(head.rec, q);
        q.forcing = false;
    }
    Op op = std::move(q.ops.front());
    q.ops.pop_front();
    if (FILE* f = order_log()) { fprintf(f, "run %s: %s\n", q.name.c_str(), op.what.c_str()); fflush(f); }
    if (op.kind == Op::WORK) op.run();
    else if (op.kind == Op::RECORD) g_pending_recs.erase(op.rec);
}
void force_record(unsigned long long rec, const Queue& for_q)
{
    auto it = g_pending_recs.find(rec);
    if (it == g_pending_recs.end()) return;
    Queue& q = g_queues[it->second];
    if (q.forcing) {   // the record sits behind a wait that (transitively) waits for the asking stream: it can never execute
        fprintf(stderr, "emu: deadlock: stream %s waits (%s) for a record on stream %s, which itself waits for stream %s\n", for_q.name.c_str(),
                for_q.ops.empty() ? "host" : for_q.ops.front().what.c_str(), q.name.c_str(), for_q.name.c_str());
        abort();
    }
    while (g_pending_recs.count(rec)) step(q);
}
void drain(Queue& q) { while (!q.ops.empty()) step(q); }
void drain_all()
{
    for (bool any = true; any;) {
        any = false;
        for (auto& kv : g_queues) if (!kv.second.ops.empty()) { drain(kv.second); any = true; }
    }
}
void drain_blocking()
{
    for (auto& kv : g_queues) if (kv.second.blocking) drain(kv.second);
}
// lazy:SEED, before every enqueue: a random number of runnable operations from random streams
void scheduler_turn()
{
    if (lazy_mode() != 2) return;
    // (fewer on average than are queued, and all of one turn from one stream: streams fall behind and run ahead of each other,
    // where a turn that kept up with the host would all but restore program order)
    static const unsigned burst[8] = {0, 0, 0, 0, 1, 1, 2, 9};
    unsigned n = burst[rnd(8)];
    if (n == 0) return;
    auto ready = [](const Queue& q) { return !q.ops.empty() && !(q.ops.front().kind == Op::WAIT && g_pending_recs.count(q.ops.front().rec)); };
    std::vector<Queue*> all;
    for (auto& kv : g_queues) if (ready(kv.second)) all.push_back(&kv.second);
    if (all.empty()) return;
    Queue& q = *all[rnd((unsigned)all.size())];
    for (; n > 0 && ready(q); --n) step(q);
}
void enqueue(hipStream_t s, Op op)
{
    scheduler_turn();
    Queue& q = queue_of(s);
    // the null stream and the blocking streams order themselves against each other: (a legal order) each runs dry before the
    // other takes an operation
    if (s == nullptr) drain_blocking();
    else if (q.blocking) { auto it = g_queues.find(nullptr); if (it != g_queues.end()) drain(it->second); }
    q.ops.push_back(std::move(op));
}
void enqueue_work(hipStream_t s, std::string what, std::function<void()> run)
{
    Op op;
    op.kind = Op::WORK; op.run = std::move(run); op.what = std::move(what);
    enqueue(s, std::move(op));
}
struct ExitReport {
    ~ExitReport()
    {
        if (!lazy_mode()) return;
        for (auto& kv : g_queues)
            if (!kv.second.ops.empty())
                fprintf(stderr, "emu: at exit stream %s still holds %zu operations, the first one: %s\n", kv.second.name.c_str(), kv.second.ops.size(), kv.second.ops.front().what.c_str());
    }
} g_exit_report;
#define LAZY_LOCK std::lock_guard<std::recursive_mutex> lazy_lock(g_lazy_mu)

hipError_t make_stream(hipStream_t* s, unsigned flags, const int* priority)
{
    *s = malloc(8);
    if (!*s) return hipErrorUnknown;
    int n;
    {
        std::lock_guard<std::mutex> lock(g_trace_mu);
        n = g_streams[*s] = g_n_streams++;
    }
    if (lazy_mode()) { LAZY_LOCK; queue_of(*s).blocking = !(flags & hipStreamNonBlocking); }
    if (priority) trace("stream_create s%d flags=%u priority=%d", n, flags, *priority);
    else trace("stream_create s%d flags=%u priority=default", n, flags);
    return hipSuccess;
}
}  // namespace

hipError_t hipStreamCreate(hipStream_t* s) { return make_stream(s, 0, nullptr); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return make_stream(s, flags, nullptr); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) { return make_stream(s, flags, &priority); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    trace("stream_destroy %s", sname(s).c_str());
    if (lazy_mode()) { LAZY_LOCK; auto it = g_queues.find(s); if (it != g_queues.end()) { drain(it->second); g_queues.erase(it); } }
    std::lock_guard<std::mutex> lock(g_trace_mu);
    if (g_streams.erase(s)) free(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    trace("stream_sync %s", sname(s).c_str());
    if (lazy_mode()) { LAZY_LOCK; drain(queue_of(s)); if (s == nullptr) drain_blocking(); }
    return hipSuccess;
}
hipError_t hipDeviceSynchronize()
{
    trace("device_sync");
    if (lazy_mode()) { LAZY_LOCK; drain_all(); }
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    *e = (hipEvent_t)malloc(sizeof(emu_event));
    if (!*e) return hipErrorUnknown;
    {
        std::lock_guard<std::mutex> lock(g_trace_mu);
        (*e)->ordinal = g_n_events++;
        (*e)->last_rec = 0;
    }
    trace("event_create %s flags=%u", ename(*e).c_str(), flags);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { trace("event_destroy %s", ename(e).c_str()); free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    trace("event_record %s %s", ename(e).c_str(), sname(s).c_str());
    if (lazy_mode()) {
        LAZY_LOCK;
        Op op;
        op.kind = Op::RECORD; op.rec = ++g_n_recs; op.what = "event_record " + ename(e);
        enqueue(s, std::move(op));
        g_pending_recs[g_n_recs] = s;
        e->last_rec = g_n_recs;
    }
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    trace("event_sync %s", ename(e).c_str());
    if (lazy_mode()) { LAZY_LOCK; static const Queue host = [] { Queue q; q.name = "host"; return q; }(); force_record(e->last_rec, host); }
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    trace("stream_wait %s %s", sname(s).c_str(), ename(e).c_str());
    if (lazy_mode() && e->last_rec) {   // (a wait for an event that was never recorded is no operation)
        LAZY_LOCK;
        Op op;
        op.kind = Op::WAIT; op.rec = e->last_rec; op.what = "stream_wait " + ename(e);
        enqueue(s, std::move(op));
    }
    return hipSuccess;
}

hipError_t hipMalloc(void** p, size_t n)
{
    *p = emu_device_alloc(n);
    if (trace_file()) {
        trace("malloc %zu", n);
        std::lock_guard<std::mutex> lock(g_trace_mu);
        if (*p) g_alloc_bytes[*p] = n;
    }
    return *p ? hipSuccess : hipErrorUnknown;
}
hipError_t hipFree(void* p)
{
    if (trace_file()) {
        size_t n = 0;
        {
            std::lock_guard<std::mutex> lock(g_trace_mu);
            auto it = g_alloc_bytes.find(p);
            if (it != g_alloc_bytes.end()) { n = it->second; g_alloc_bytes.erase(it); }
        }
        trace("free %zu", n);
    }
    if (lazy_mode()) { LAZY_LOCK; drain_all(); }
    emu_device_free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind kind)
{
    trace("memcpy %s %zu", kname(kind), n);
    if (lazy_mode()) { LAZY_LOCK; drain_blocking(); }   // and for no non-blocking stream
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n)
{
    if (lazy_mode()) { LAZY_LOCK; drain_blocking(); }
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t st)
{
    trace("memcpy_async %s %zu %s", kname(kind), n, sname(st).c_str());
    if (lazy_mode()) {
        LAZY_LOCK;
        const std::string what = std::string("memcpy_async ") + kname(kind) + " " + std::to_string(n);
        if (kind == hipMemcpyHostToDevice && !pinned(s, n)) {   // pageable source: staged when the call is made
            auto snap = std::make_shared<std::vector<char>>((const char*)s, (const char*)s + n);
            enqueue_work(st, what + " (pageable, staged at the call)", [d, snap, n] { memcpy(d, snap->data(), n); });
        } else if (kind == hipMemcpyDeviceToHost && !pinned(d, n)) {   // pageable destination: done when the call returns
            enqueue_work(st, what + " (pageable, complete at the call)", [d, s, n] { memcpy(d, s, n); });
            drain(queue_of(st));
        } else {
            enqueue_work(st, what, [d, s, n] { memcpy(d, s, n); });
        }
        return hipSuccess;
    }
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st)
{
    trace("memset_async %zu %s", n, sname(st).c_str());
    if (lazy_mode()) { LAZY_LOCK; enqueue_work(st, "memset_async " + std::to_string(n), [d, v, n] { memset(d, v, n); }); return hipSuccess; }
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned)
{
    *p = malloc(n);
    if (*p && lazy_mode()) { LAZY_LOCK; g_pinned[(char*)*p] = n; }
    return *p ? hipSuccess : hipErrorUnknown;
}
hipError_t hipHostFree(void* p)
{
    if (lazy_mode()) { LAZY_LOCK; drain_all(); g_pinned.erase((char*)p); }
    free(p);
    return hipSuccess;
}

// A caller's side of a stream, for a Python driver (tools/emu/run_emu_streams.py): a stream the engines did not make (traced
// as `caller`), a copy queued on it that is deferred whatever memory it touches (the caller's producer), and its waits.
extern "C" int emu_streams_mode() { return lazy_mode(); }
extern "C" void* emu_caller_stream_create() { return malloc(8); }
extern "C" void emu_caller_stream_destroy(void* s)
{
    if (lazy_mode()) { LAZY_LOCK; auto it = g_queues.find(s); if (it != g_queues.end()) { drain(it->second); g_queues.erase(it); } }
    free(s);
}
extern "C" void emu_caller_copy(void* d, const void* s, size_t n, void* stream)
{
    if (lazy_mode()) { LAZY_LOCK; enqueue_work(stream, "caller copy " + std::to_string(n), [d, s, n] { memcpy(d, s, n); }); return; }
    memcpy(d, s, n);
}
extern "C" void emu_caller_stream_sync(void* stream)
{
    if (lazy_mode()) { LAZY_LOCK; drain(queue_of(stream)); }
}
extern "C" size_t emu_streams_queued()   // operations that have not executed yet, over all streams
{
    size_t n = 0;
    if (lazy_mode()) { LAZY_LOCK; for (auto& kv : g_queues) n += kv.second.ops.size(); }
    return n;
}

#define EMU_WAIT(what) do { Fiber& f_ = g_fibers[g_cur]; f_.wait = what; f_.wait_pc = __builtin_return_address(0); f_.hist[++f_.hist_n % 16] = f_.wait_pc; } while (0)

__attribute__((noinline)) void emu_syncthreads()
{
    EMU_WAIT("__syncthreads");
    const unsigned gen = g_bar_gen;
    if (++g_bar_arrived == g_live) { g_bar_arrived = 0; ++g_bar_gen; return; }
    while (g_bar_gen == gen) yield_to_scheduler();
}

// All live lanes of the wave that reach this point exchange one 32-bit value.
unsigned emu_wave_exchange(unsigned value, unsigned* all64)
{
    Wave& w = g_waves[g_cur / 64];
    const int lane = g_cur % 64;
    w.slot[lane] = value;
    w.present[lane] = true;
    w.site[lane] = g_fibers[g_cur].wait_pc;
    const unsigned gen = w.gen;
    if (++w.arrived == w.live) {
        // every lane of a rendezvous must come from the same call: lanes that meet from two different ones have
        // taken different paths through code this harness can only run convergently
        // (EMU_STRICT=1, for -O0 builds: an optimiser may duplicate one call into two places)
        static const bool strict = getenv("EMU_STRICT") != nullptr;
        for (int i = 0; strict && i < 64; ++i)
            if (w.present[i] && w.site[i] != w.site[lane]) {
                Dl_info di;
                const bool ok = dladdr(w.site[lane], &di) != 0;
                char* base = ok ? (char*)di.dli_fbase : (char*)0;
                fprintf(stderr, "emu: divergent rendezvous: lane %d called from +0x%zx, lane %d from +0x%zx\n", lane, (size_t)((char*)w.site[lane] - base), i, (size_t)((char*)w.site[i] - base));
                abort();
            }
        memcpy(w.snap, w.slot, sizeof(w.slot)); memcpy(w.snap_present, w.present, sizeof(w.present));
        memset(w.present, 0, sizeof(w.present)); w.arrived = 0; ++w.gen;
    } else {
        while (w.gen == gen) yield_to_scheduler();
    }
    for (int i = 0; i < 64; ++i) all64[i] = w.snap_present[i] ? w.snap[i] : 0u;
    return 0;
}

__attribute__((noinline)) void emu_wave_barrier()
{
    EMU_WAIT("wave_sync");
    unsigned all[64];
    emu_wave_exchange(0u, all);
}

__attribute__((noinline)) unsigned long long emu_ballot(bool pred)
{
    EMU_WAIT("ballot");
    unsigned all[64];
    emu_wave_exchange(pred ? 1u : 0u, all);
    unsigned long long m = 0;
    for (int i = 0; i < 64; ++i) if (all[i]) m |= 1ull << i;
    return m;
}

__attribute__((noinline)) int emu_readlane(int v, int lane)
{
    EMU_WAIT("readlane");
    unsigned all[64];
    emu_wave_exchange((unsigned)v, all);
    return (int)all[lane & 63];
}

__attribute__((noinline)) int emu_bpermute(int addr, int v)
{
    EMU_WAIT("bpermute");
    unsigned all[64];
    emu_wave_exchange((unsigned)v, all);
    return (int)all[(addr >> 2) & 63];
}

__attribute__((noinline)) int emu_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl)
{
    EMU_WAIT("dpp");
    unsigned all[64];
    emu_wave_exchange((unsigned)src, all);
    const int lane = g_cur % 64, row = lane / 16, pos = lane % 16;
    if (!((row_mask >> row) & 1) || !((bank_mask >> (pos / 4)) & 1)) return old;
    int srcpos = -1;  // position within the row, -1 = invalid
    if (ctrl >= 0x101 && ctrl <= 0x10F) { srcpos = pos + (ctrl - 0x100); if (srcpos > 15) srcpos = -1; }       // row_shl
    else if (ctrl >= 0x111 && ctrl <= 0x11F) { srcpos = pos - (ctrl - 0x110); }                                 // row_shr
    else if (ctrl >= 0x121 && ctrl <= 0x12F) { srcpos = (pos - (ctrl - 0x120) + 16) % 16; }                     // row_ror
    else if (ctrl == 0x140) { srcpos = 15 - pos; }                                                               // row_mirror
    else if (ctrl == 0x141) { srcpos = (pos & 8) | (7 - (pos & 7)); }                                            // row_half_mirror
    else if (ctrl == 0x142) { if (row == 0) return old; return (int)all[row * 16 - 1]; }                         // row_bcast:15 (lane 15 of the previous row)
    else if (ctrl == 0x143) { if (row < 2) return old; return (int)all[31]; }                                   // row_bcast:31
    else if (ctrl == 0x138) { if (lane == 0) return bound_ctrl ? 0 : old; return (int)all[lane - 1]; }          // wave_shr:1
    else if (ctrl < 0x100) { srcpos = (pos & ~3) | ((ctrl >> (2 * (pos & 3))) & 3); }                            // quad_perm
    else { fprintf(stderr, "emu: unsupported dpp ctrl 0x%x\n", ctrl); abort(); }
    if (srcpos < 0) return bound_ctrl ? 0 : old;
    return (int)all[row * 16 + srcpos];
}

static void run_kernel(const char* name, dim3 grid, dim3 block, const std::function<void()>& body);

void emu_launch(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const std::function<void()>& body)
{
    trace("launch %s grid=(%u,%u,%u) block=(%u,%u,%u) lds=%zu %s", name, grid.x, grid.y, grid.z, block.x, block.y, block.z, lds_bytes, sname(stream).c_str());
    if (lazy_mode()) {
        LAZY_LOCK;
        enqueue_work(stream, std::string("launch ") + name, [name, grid, block, body] { run_kernel(name, grid, block, body); });
        return;
    }
    run_kernel(name, grid, block, body);
}

static void run_kernel(const char* name, dim3 grid, dim3 block, const std::function<void()>& body)
{
    // one kernel at a time: the scheduler's state is global, and a host program may launch from several threads
    static std::mutex launch_mu;
    std::lock_guard<std::mutex> launch_lock(launch_mu);
    const unsigned nthr = block.x * block.y * block.z;
    if (g_fibers.size() < nthr) {
        const size_t old = g_fibers.size();
        g_fibers.resize(nthr);
        for (size_t i = old; i < nthr; ++i) g_fibers[i].stack = (char*)malloc(kStack);
    }
    g_body = &body;
    g_nthr = nthr;
    blockDim = block;
    gridDim = grid;
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx) {
                blockIdx = dim3(bx, by, bz);
                if (&__start_emu_lds[0] != nullptr && &__stop_emu_lds[0] > &__start_emu_lds[0]) memset(__start_emu_lds, 0xCD, (size_t)(__stop_emu_lds - __start_emu_lds));
                g_live = nthr; g_bar_arrived = 0;
                g_waves.assign((nthr + 63) / 64, Wave());
                for (unsigned t = 0; t < nthr; ++t) {
                    Fiber& f = g_fibers[t];
                    f.done = false; f.hist_n = 0;
                    g_waves[t / 64].live++;
                    getcontext(&f.ctx);
                    f.ctx.uc_stack.ss_sp = f.stack;
                    f.ctx.uc_stack.ss_size = kStack;
                    f.ctx.uc_link = &g_main;
                    makecontext(&f.ctx, trampoline, 0);
                }
                for (auto& w : g_waves) { memset(w.present, 0, sizeof(w.present)); }
                unsigned alive = nthr;
                unsigned long long spins = 0;
                while (alive) {
                    alive = 0;
                    const unsigned nwaves = (nthr + 63) / 64;
                    for (unsigned wi = 0; wi < nwaves; ++wi) {
                        const unsigned wv = reverse_order() ? nwaves - 1 - wi : wi;
                        for (unsigned t = wv * 64; t < nthr && t < (wv + 1) * 64; ++t) {
                            Fiber& f = g_fibers[t];
                            if (f.done) continue;
                            g_cur = (int)t;
                            threadIdx = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
                            swapcontext(&g_main, &f.ctx);
                            if (!f.done) ++alive;
                        }
                    }
                    if (++spins > 300000ull) { fprintf(stderr, "emu: deadlock (divergent barrier?) in %s, workgroup %u of %u\n", name, bx, grid.x);
                        for (unsigned t = 0; t < nthr; ++t)
                            if (!g_fibers[t].done) {
                                Dl_info di;   // offset in the shared object: addr2line -e <lib> <offset>
                                const bool ok = dladdr(g_fibers[t].wait_pc, &di) != 0;
                                fprintf(stderr, "  work-item %u waits in %s called from +0x%zx; %llu rendezvous so far, the last ones from", t, g_fibers[t].wait, ok ? (size_t)((char*)g_fibers[t].wait_pc - (char*)di.dli_fbase) : (size_t)g_fibers[t].wait_pc, g_fibers[t].hist_n);
                                for (unsigned h = 0; h < 16 && h < g_fibers[t].hist_n; ++h)
                                    fprintf(stderr, " +0x%zx", (size_t)((char*)g_fibers[t].hist[(g_fibers[t].hist_n - h) % 16] - (ok ? (char*)di.dli_fbase : (char*)0)));
                                fprintf(stderr, "\n");
                            }
                        abort();
                    }
                }
            }
}
