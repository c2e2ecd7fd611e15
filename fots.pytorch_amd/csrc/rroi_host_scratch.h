// rroi_host_scratch.h -- host side, part 2 of 3: the scratch arena of the reference-ABI launchers (LauncherArena,
// ScratchLease, launcher_scratch).  Included by rroi_align_hip.hip inside its anonymous namespace.
#pragma once

// ------------------------------------------------------------------------------------
// Scratch of the reference-ABI launchers.  Their signatures carry no workspace, so the library keeps
// one buffer per (device, stream), grown on demand and reused: calls on one stream are ordered, so the
// next call may overwrite what the previous one left.  No allocator round trip per call, and a call
// whose buffer exists enqueues kernels only -- it can be captured into a HIP graph.
// Lifetime and locking rules:
//   * a buffer that has been handed out WHILE ITS STREAM WAS CAPTURING is baked into a graph: it is PINNED and from
//     then on GRAPH-EXCLUSIVE -- never freed (not by a later, larger call, not by the least-recently-used eviction,
//     not by rroi_align_release_launcher_scratch()) and never handed out again: later eager calls on that stream get
//     a buffer of their own (a second table entry), later captures take stream-ordered memory that their graph owns.
//     So a replay of the graph -- on whatever stream -- shares its scratch with nothing but itself;
//   * a call made while capturing that finds no unpinned buffer of its stream (or one that is too small) takes
//     stream-ordered memory for that call alone: the graph owns it;
//   * locks: the TABLE lock covers look-up, creation and eviction only; every entry has its OWN lock, taken before
//     the table lock is dropped and held until the caller has ENQUEUED its launches (ScratchLease) -- so only callers
//     of the same (device, stream) entry serialise, and a second thread sharing the stream cannot free, in stream
//     order and ahead of those launches, a buffer that the first thread is about to launch on.  Lock order: table,
//     then entry; a lease holder never takes the table lock.
// ------------------------------------------------------------------------------------
struct LauncherArena {
    bool used = false;
    int device = 0;
    hipStream_t stream = nullptr;
    void* ptr = nullptr;
    size_t bytes = 0;
    unsigned long long last_use = 0;
    bool pinned = false;   // handed out during a stream capture: a graph replays with this address
    unsigned long long capture_id = 0;   // ... the capture that pinned it: later calls of the SAME capture may reuse it
    std::mutex in_use;     // held by the lease of the call that is enqueuing on this buffer
};
constexpr int kMaxArenas = 64;   // pinned entries keep their slot for the life of the process (documented in the header)
std::mutex g_table_mutex;
LauncherArena g_arenas[kMaxArenas];
unsigned long long g_arena_clock = 0;
std::atomic<unsigned long long> g_transient_calls{0};

// A buffer of at least `bytes` for launches on `stream`, held under its entry's lock until give_back().
struct ScratchLease {
    std::unique_lock<std::mutex> lock;   // the entry's (empty for a transient buffer)
    void* ptr = nullptr;
    bool transient = false;   // the buffer belongs to this call alone: give_back() returns it in stream order
    hipError_t err = hipSuccess;
    hipError_t give_back(hipStream_t stream)
    {
        hipError_t e = hipSuccess;
        if (transient && ptr) e = hipFreeAsync(ptr, stream);
        ptr = nullptr;
        if (lock.owns_lock()) lock.unlock();
        return e;
    }
};

ScratchLease launcher_scratch(hipStream_t stream, size_t bytes)
{
    ScratchLease L;
    int dev = 0;
    if ((L.err = hipGetDevice(&dev)) != hipSuccess) return L;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long cap_id = 0;
    const bool capturing = hipStreamGetCaptureInfo(stream, &cap, &cap_id) == hipSuccess && cap != hipStreamCaptureStatusNone;
    auto take_transient = [&]() {
        L.err = hipMallocAsync(&L.ptr, bytes, stream);
        L.transient = L.err == hipSuccess;
        if (!L.transient) L.ptr = nullptr;
        g_transient_calls.fetch_add(1, std::memory_order_relaxed);
    };
    std::unique_lock<std::mutex> table(g_table_mutex);
    LauncherArena* a = nullptr;
    std::unique_lock<std::mutex> mine;
    for (;;) {
        // the stream's own entry: the one THIS capture pinned earlier (a second launcher call inside one capture reuses
        // it instead of taking mem-alloc nodes), else its unpinned one (a pinned one belongs to its graph)
        a = nullptr;
        for (LauncherArena& e : g_arenas)
            if (e.used && e.device == dev && e.stream == stream && capturing && e.pinned && e.capture_id == cap_id && e.bytes >= bytes)
                a = &e;
        if (!a)
            for (LauncherArena& e : g_arenas)
                if (e.used && !e.pinned && e.device == dev && e.stream == stream) a = &e;
        if (!a) break;
        mine = std::unique_lock<std::mutex>(a->in_use, std::try_to_lock);
        if (mine.owns_lock()) break;
        // another thread is enqueuing on this entry: wait for it WITHOUT the table lock (holding it stalled
        // every other stream's look-up), then look the entry up again -- it may have grown, been pinned or evicted
        table.unlock();
        { std::lock_guard<std::mutex> wait(a->in_use); }   // (the entries are static: the mutex outlives any eviction)
        table.lock();
    }
    if (a) {
        if (a->bytes >= bytes) {
            a->last_use = ++g_arena_clock;
            if (capturing && !a->pinned) {             // this graph's from now on
                a->pinned = true;
                a->capture_id = cap_id;
            }
            L.ptr = a->ptr;
            L.lock = std::move(mine);
            return L;
        }
        if (capturing) {   // too small, and the graph owns what it allocates: the entry stays as it is
            mine.unlock();
            table.unlock();
            take_transient();
            return L;
        }
        // grow: the old buffer goes back in stream order, behind the launches that still use it (every user held
        // this entry's lock until its launches were enqueued, so none of them can come after this free)
        if ((L.err = hipFreeAsync(a->ptr, stream)) != hipSuccess) return L;
        a->ptr = nullptr;
        a->bytes = 0;
        void* p = nullptr;
        if ((L.err = hipMallocAsync(&p, bytes, stream)) != hipSuccess) {
            a->used = false;
            return L;
        }
        a->ptr = p;
        a->bytes = bytes;
        a->last_use = ++g_arena_clock;
        L.ptr = p;
        L.lock = std::move(mine);
        return L;
    }
    if (capturing) {   // nothing cached for this stream: the graph owns what it allocates
        table.unlock();
        take_transient();
        return L;
    }
    // a new entry: a free slot, or the least recently used buffer that no graph holds and nobody is enqueuing on
    LauncherArena* slot = nullptr;
    for (LauncherArena& e : g_arenas)
        if (!e.used && !slot) slot = &e;
    if (slot) {
        mine = std::unique_lock<std::mutex>(slot->in_use);
    } else {
        LauncherArena* lru = nullptr;
        for (LauncherArena& e : g_arenas)
            if (!e.pinned && (!lru || e.last_use < lru->last_use)) lru = &e;
        if (lru) mine = std::unique_lock<std::mutex>(lru->in_use, std::try_to_lock);
        if (!lru || !mine.owns_lock()) {   // every entry is pinned (or the candidate is busy): nothing to cache in
            table.unlock();
            take_transient();
            return L;
        }
        int cur = dev;   // (its stream may be gone: a synchronous free)
        (void)hipSetDevice(lru->device);
        (void)hipFree(lru->ptr);
        (void)hipSetDevice(cur);
        lru->used = false;
        slot = lru;
    }
    void* p = nullptr;
    if ((L.err = hipMallocAsync(&p, bytes, stream)) != hipSuccess) return L;
    slot->used = true;
    slot->device = dev;
    slot->stream = stream;
    slot->ptr = p;
    slot->bytes = bytes;
    slot->pinned = false;
    slot->last_use = ++g_arena_clock;
    L.ptr = p;
    L.lock = std::move(mine);
    return L;
}
