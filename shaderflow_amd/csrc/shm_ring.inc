// shm_ring.inc — cross-process frame queue of the sharded export (included by capi_readout.hip; no reference equivalent, SURVEY.md §8e).
//
// One process per GPU. A sink (ffmpeg's stdin, a file) takes ONE byte stream, so one process owns it — but nothing forces the
// frames of the other ranks through that process' GPU and its single PCIe link: every rank copies its finished frames over its
// OWN link into a POSIX shared-memory segment (registered with HIP, so the copy engine writes it directly), and a writer thread
// in the sink's process hands the frames to the file descriptor in frame order. Per rank the segment holds a ring of `slots`
// frames with two counters — frames published by the producer, frames consumed by the writer — both only ever incremented, each
// written by one side (single producer, single consumer per ring): plain acquire/release atomics, no lock crosses a process.
//
//   segment = header | rank 0: slots x frame | rank 1: slots x frame | …
//
// The producer side keeps turbopipe's structure (exporting.py:147-171): copy stream + fence on the render stream + a thread that
// publishes a frame when its copy has landed; sfx_shm_push blocks while the rank's ring is full (back-pressure from the sink).

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

struct ShmHeader {
    std::atomic<uint64_t> magic;                 // set last by the creator (release); others wait for it
    uint64_t frame_bytes, frame_stride, slots, world, data_offset;
    std::atomic<uint32_t> failed;                // any side may raise it: everybody stops waiting
    struct alignas(64) Counters { std::atomic<uint64_t> produced; char pad0[56]; std::atomic<uint64_t> consumed; char pad1[56]; } rank[64];
};
static const uint64_t SHM_MAGIC = 0x5346585f53484d31ull;           // "SFX_SHM1"

struct ShmRing : Object {
    Context* ctx;
    std::string name;
    int rank, world, slots;
    size_t frame_bytes, frame_stride, mapped_bytes;
    bool owner, registered = false, unlinked = false;
    ShmHeader* header = nullptr;
    char* base = nullptr;
    // producer: the publisher thread waits for a pushed frame on the host, copies it on an engine lane (two in flight: lane_pump on
    // EngineLanes, capi_readout.hip) and publishes it when it has landed
    std::vector<hipEvent_t> ready;               // per slot: recorded on the render stream when the slot's frame is complete
    std::vector<const void*> sources;            // per slot: where the frame lives on the device
    EngineLanes lanes;
    void* bounce = nullptr;                      // pinned staging when the segment cannot be registered for DMA
    ptrdiff_t dma_delta = 0;                     // registered slots: device-visible address minus host address
    uint64_t pushed = 0;
    std::atomic<int> copy_error{0};              // raised by the publisher thread, read by sfx_shm_push
    std::thread publisher;
    std::mutex mutex;
    std::condition_variable wake, idle;
    uint64_t queued = 0, published = 0;
    bool stop = false;
    // consumer (the sink's process)
    std::thread writer;
    std::vector<int32_t> order_rank, order_count;
    int fd = -1, io_error = 0;
    bool draining = false;
};

static char* shm_slot(ShmRing* r, int rank, uint64_t frame) {
    return r->base + r->header->data_offset + ((uint64_t)rank*r->slots + frame % r->slots)*r->frame_stride;
}

// how long one side waits while NOTHING moves anywhere in the group before it gives up: SHADERFLOW_SHM_TIMEOUT seconds, default 120.
// The clock restarts whenever any rank's produced or consumed counter advances: rank r's own `consumed` stands still while the writer
// drains the runs of the other ranks ((world-1) x batch frames of sink time — minutes with a slow encoder behind the pipe), and that
// is a healthy export, not a dead one (ADVICE round 3). A dead peer is caught at once by the `failed` flag, not by this clock.
static double shm_patience() {
    static const double seconds = [] { const char* e = getenv("SHADERFLOW_SHM_TIMEOUT"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 120.0; }();
    return seconds;
}

static uint64_t shm_progress(const ShmHeader* header) {
    uint64_t sum = 0;
    const uint64_t world = header->world <= 64 ? header->world : 64;
    for (uint64_t k = 0; k < world; k++) sum += header->rank[k].produced.load(std::memory_order_relaxed) + header->rank[k].consumed.load(std::memory_order_relaxed);
    return sum;
}

// waits (sleeping) until `ready()`; false when the other side failed or nothing in the group moved for `seconds`
// (`global_progress` false: a plain deadline — segment set-up, before the counters mean anything)
template <class F> static bool shm_wait(ShmRing* r, F ready, double seconds = shm_patience(), bool global_progress = true) {
    auto start = std::chrono::steady_clock::now();
    uint64_t seen = (global_progress && r->header) ? shm_progress(r->header) : 0;
    for (unsigned spins = 0; !ready(); spins++) {
        if (r->header && r->header->failed.load(std::memory_order_acquire)) return false;
        if (spins < 64) { std::this_thread::yield(); continue; }
        std::this_thread::sleep_for(std::chrono::microseconds(spins < 2000 ? 50 : 500));
        if ((spins & 255) == 0) {
            if (global_progress && r->header) {
                const uint64_t now = shm_progress(r->header);
                if (now != seen) { seen = now; start = std::chrono::steady_clock::now(); }
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count() > seconds) return false;
        }
    }
    return true;
}

static void shm_publisher(ShmRing* r) {
    hipSetDevice(r->ctx->device);
    struct Hooks {                                                   // (a job is a frame's number)
        ShmRing* r;
        uint64_t issued = 0;
        int slot(uint64_t frame) const { return (int)(frame % r->slots); }
        char* target(uint64_t frame) const { return r->bounce ? (char*)r->bounce + (size_t)slot(frame)*r->frame_stride : shm_slot(r, r->rank, frame) + r->dma_delta; }
        bool take(uint64_t& frame, bool sleep) {
            std::unique_lock<std::mutex> lock(r->mutex);
            if (sleep) r->wake.wait(lock, [&] { return r->stop || issued < r->queued; });
            if (issued >= r->queued) return false;
            frame = issued++;
            return true;
        }
        bool ready(uint64_t frame) {                                 // the frame is complete on the render stream (false: its event reports an error — the ring fails)
            const bool rendered = wait_frame_ready(r->ready[slot(frame)]);
            r->lanes.resolve(r->ctx, target(frame), r->sources[slot(frame)]);
            return rendered;
        }
        LaneIssue issue(int lane, uint64_t frame) { return r->lanes.issue(lane, target(frame), r->sources[slot(frame)], r->frame_bytes) ? LaneIssue::issued : LaneIssue::failed; }
        void landed(uint64_t frame, bool ok) {
            if (ok) {
                if (r->bounce) memcpy(shm_slot(r, r->rank, frame), (char*)r->bounce + (frame % r->slots)*r->frame_stride, r->frame_bytes);
                r->header->rank[r->rank].produced.store(frame + 1, std::memory_order_release);
            } else {                                                 // the copy failed: the slot does not hold the frame — never publish it
                r->copy_error = 1;
                r->header->failed.store(1, std::memory_order_release);
            }
            { std::lock_guard<std::mutex> lock(r->mutex); r->published = frame + 1; }   // (failed: local bookkeeping only — nobody waits for it for ever)
            r->idle.notify_all();
        }
        bool failed(uint64_t) {                                      // the ring has failed for every rank: the thread ends
            r->copy_error = 1;
            r->header->failed.store(1, std::memory_order_release);  // everybody stops waiting for this rank's frames
            { std::lock_guard<std::mutex> lock(r->mutex); r->published = r->queued; }
            r->idle.notify_all();
            return false;
        }
    } hooks{r};
    // no early reports: `produced` is a counter that must rise in frame order, so frames are published strictly in issue order
    lane_pump<uint64_t>(r->lanes, 2, false, hooks);
}

static void shm_writer(ShmRing* r) {
    std::vector<uint64_t> taken(r->world, 0);
    for (size_t k = 0; k < r->order_rank.size() && !r->io_error; k++) {
        const int from = r->order_rank[k];
        for (int n = 0; n < r->order_count[k]; n++) {
            const uint64_t frame = taken[from];
            auto& counters = r->header->rank[from];
            if (!shm_wait(r, [&] { return counters.produced.load(std::memory_order_acquire) > frame; })) { r->io_error = ETIMEDOUT; break; }
            const char* p = shm_slot(r, from, frame);
            size_t left = r->fd >= 0 ? r->frame_bytes : 0;           // no sink (a benchmark, a freewheeling run): consume and discard
            while (left > 0) {
                ssize_t w = ::write(r->fd, p, left);
                if (w < 0) { if (errno == EINTR) continue; r->io_error = errno; break; }
                p += w; left -= (size_t)w;
            }
            if (r->io_error) break;
            taken[from] = frame + 1;
            counters.consumed.store(frame + 1, std::memory_order_release);
        }
    }
    if (r->io_error) r->header->failed.store(1, std::memory_order_release);
}

extern "C" int sfx_shm_create(sfx_handle h, const char* name, int rank, int world, size_t frame_bytes, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, h);
    if (!out || !name || name[0] != '/' || rank < 0 || world < 1 || world > 64 || rank >= world || slots < 1 || frame_bytes == 0)
        return fail(SFX_E_INVALID, "shared frame ring '%s': rank %d of %d, %d slots of %zu bytes", name ? name : "(null)", rank, world, slots, frame_bytes);
    USE_DEVICE(c);
    ShmRing* r = new ShmRing();
    r->magic = MAGIC_SHM; r->ctx = c; r->name = name; r->rank = rank; r->world = world; r->slots = slots;
    r->frame_bytes = frame_bytes; r->frame_stride = (frame_bytes + 4095) & ~(size_t)4095; r->owner = (rank == 0);
    const size_t data_offset = (sizeof(ShmHeader) + 4095) & ~(size_t)4095;
    r->mapped_bytes = data_offset + (size_t)world*slots*r->frame_stride;
    auto bail = [&](int code, const char* what) { const int e = errno; if (r->base) munmap(r->base, r->mapped_bytes); if (r->owner) shm_unlink(name); delete r; return fail(code, "shared frame ring '%s': %s: %s", name, what, strerror(e)); };
    int fd = -1;
    if (r->owner) {
        shm_unlink(name);                                             // a stale segment of a crashed run
        fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0) return bail(SFX_E_IO, "shm_open");
        if (ftruncate(fd, (off_t)r->mapped_bytes) != 0) { close(fd); return bail(SFX_E_IO, "ftruncate (is /dev/shm large enough?)"); }
    } else {
        const auto start = std::chrono::steady_clock::now();
        struct stat st;
        for (;;) {                                                    // the creator may still be on its way
            fd = shm_open(name, O_RDWR, 0600);
            if (fd >= 0 && fstat(fd, &st) == 0 && (size_t)st.st_size >= r->mapped_bytes) break;
            if (fd >= 0) { close(fd); fd = -1; }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count() > 120.0) { errno = ETIMEDOUT; return bail(SFX_E_IO, "waiting for rank 0 to create the segment"); }
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
    }
    void* mapped = mmap(nullptr, r->mapped_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (mapped == MAP_FAILED) return bail(SFX_E_IO, "mmap");
    r->base = (char*)mapped;
    r->header = (ShmHeader*)mapped;
    if (r->owner) {
        r->header->frame_bytes = frame_bytes; r->header->frame_stride = r->frame_stride; r->header->slots = slots; r->header->world = world;
        r->header->data_offset = data_offset;
        r->header->failed.store(0);
        for (int k = 0; k < 64; k++) { r->header->rank[k].produced.store(0); r->header->rank[k].consumed.store(0); }
        r->header->magic.store(SHM_MAGIC, std::memory_order_release);
    } else {
        const bool ready = shm_wait(r, [&] { return r->header->magic.load(std::memory_order_acquire) == SHM_MAGIC; }, 120.0, false);
        if (!ready || r->header->frame_bytes != frame_bytes || r->header->slots != (uint64_t)slots || r->header->world != (uint64_t)world) {
            errno = EPROTO; return bail(SFX_E_INVALID, "the segment was created for another geometry");
        }
    }
    // the rank's own slots become a DMA target; without registration (refused for this mapping) copies stage through a pinned buffer
    char* mine = shm_slot(r, rank, 0);
    if (hipHostRegister(mine, (size_t)slots*r->frame_stride, hipHostRegisterDefault) == hipSuccess) {
        r->registered = true;
        void* device_view = nullptr;                                  // the address the copy engines know the registered pages by
        if (hipHostGetDevicePointer(&device_view, mine, 0) == hipSuccess && device_view) r->dma_delta = (char*)device_view - mine;
        else (void)hipGetLastError();
    } else {
        (void)hipGetLastError();
        if (hipHostMalloc(&r->bounce, (size_t)slots*r->frame_stride, hipHostMallocDefault) != hipSuccess) { errno = ENOMEM; return bail(SFX_E_HIP, "neither hipHostRegister nor a pinned staging buffer"); }
    }
    r->ready.resize(slots); r->sources.assign(slots, nullptr);
    bool ok = true;
    for (int k = 0; k < slots && ok; k++) ok = hipEventCreateWithFlags(&r->ready[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) { errno = EIO; return bail(SFX_E_HIP, "event creation"); }
    r->publisher = std::thread(shm_publisher, r);
    c->readouts.push_back({r, [](void* ring) {
        ShmRing* q = (ShmRing*)ring;
        std::unique_lock<std::mutex> lock(q->mutex);
        q->idle.wait(lock, [&] { return q->published >= q->queued; });
    }});
    *out = handle_of(r);
    return SFX_OK;
}

extern "C" int sfx_shm_push(sfx_handle h, const void* device_ptr) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r || !device_ptr) return fail(SFX_E_INVALID, "invalid shared frame ring or pointer");
    USE_DEVICE(r->ctx);
    const uint64_t frame = r->pushed;
    auto& counters = r->header->rank[r->rank];
    // a slot is free again when the writer has consumed the frame that last lived in it
    if (!shm_wait(r, [&] { return frame < counters.consumed.load(std::memory_order_acquire) + (uint64_t)r->slots; }))
        return fail(SFX_E_IO, "shared frame ring: the sink stopped consuming frames (the writer or a peer failed, or nothing moved in the group for %.0f s)", shm_patience());
    if (r->copy_error) return fail(SFX_E_HIP, "shared frame ring: neither HSA nor HIP accepted the read-out copy");
    r->sources[frame % r->slots] = device_ptr;
    HIP_TRY(hipEventRecord(r->ready[frame % r->slots], r->ctx->stream));     // the frame is complete on the render stream when this event is
    r->pushed = frame + 1;
    {
        std::lock_guard<std::mutex> lock(r->mutex);
        r->queued = r->pushed;
    }
    r->wake.notify_one();
    return SFX_OK;
}

// every frame pushed so far has left its device buffer (which may be rendered into again) and is visible to the writer
extern "C" int sfx_shm_flush(sfx_handle h) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r) return fail(SFX_E_INVALID, "invalid shared frame ring");
    std::unique_lock<std::mutex> lock(r->mutex);
    r->idle.wait(lock, [&] { return r->published >= r->queued; });
    return SFX_OK;
}

// the first `frames` frames this rank pushed have left their device buffers (which may be rendered into again)
extern "C" int sfx_shm_wait(sfx_handle h, int64_t frames) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r || frames < 0 || (uint64_t)frames > r->pushed) return fail(SFX_E_INVALID, "invalid shared frame ring, or waiting for frames that were never pushed");
    std::unique_lock<std::mutex> lock(r->mutex);
    r->idle.wait(lock, [&] { return r->published >= (uint64_t)frames; });
    return SFX_OK;
}

extern "C" int sfx_shm_drain(sfx_handle h, int fd, const int32_t* ranks, const int32_t* counts, int runs) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r || !r->owner || r->draining || runs < 0 || (runs > 0 && (!ranks || !counts))) return fail(SFX_E_INVALID, "shared frame ring: only its creator drains it, once");
    for (int k = 0; k < runs; k++) if (ranks[k] < 0 || ranks[k] >= r->world || counts[k] < 0) return fail(SFX_E_INVALID, "shared frame ring: run %d names rank %d / %d frames", k, ranks[k], counts[k]);
    r->order_rank.assign(ranks, ranks + runs); r->order_count.assign(counts, counts + runs);
    r->fd = fd; r->draining = true;
    r->writer = std::thread(shm_writer, r);
    return SFX_OK;
}

// any rank, any time: tells every process of the group to stop waiting (a producer raised, the export is being torn down)
extern "C" int sfx_shm_abort(sfx_handle h) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r) return fail(SFX_E_INVALID, "invalid shared frame ring");
    r->header->failed.store(1, std::memory_order_release);
    return SFX_OK;
}

// rank 0, once every rank has mapped the segment: removes its NAME, so that no crash can leave gigabytes of tmpfs behind (the
// memory lives until the last process unmaps it)
extern "C" int sfx_shm_unlink(sfx_handle h) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r || !r->owner) return fail(SFX_E_INVALID, "shared frame ring: only its creator unlinks it");
    if (!r->unlinked) { shm_unlink(r->name.c_str()); r->unlinked = true; }
    return SFX_OK;
}

extern "C" int sfx_shm_drain_wait(sfx_handle h) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r) return fail(SFX_E_INVALID, "invalid shared frame ring");
    if (r->writer.joinable()) r->writer.join();
    return r->io_error ? fail(SFX_E_IO, "shared frame ring: writing to the sink failed: %s", strerror(r->io_error)) : SFX_OK;
}

extern "C" int sfx_shm_destroy(sfx_handle h) {
    ShmRing* r = get<ShmRing>(h, MAGIC_SHM);
    if (!r) return fail(SFX_E_INVALID, "invalid shared frame ring");
    hipSetDevice(r->ctx->device);
    {
        std::lock_guard<std::mutex> lock(r->mutex);
        r->stop = true;
    }
    r->wake.notify_all();
    if (r->publisher.joinable()) r->publisher.join();
    if (r->writer.joinable()) { r->header->failed.store(1, std::memory_order_release); r->writer.join(); }
    r->lanes.release();
    readouts_forget(r->ctx, r);
    if (r->registered) hipHostUnregister(shm_slot(r, r->rank, 0));
    if (r->bounce) hipHostFree(r->bounce);
    for (auto& e : r->ready) hipEventDestroy(e);
    munmap(r->base, r->mapped_bytes);
    if (r->owner && !r->unlinked) shm_unlink(r->name.c_str());
    r->magic = 0;
    delete r;
    return SFX_OK;
}
