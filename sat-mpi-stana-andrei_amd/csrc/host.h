// host.h -- the host-side layer the solver translation units share (dpll.hip,
// dpll_scan.hip, dp.hip, resolution.hip, cdcl.hip, resolution_batch.hip,
// dp_batch.hip): the error-propagating SATMI_TRY, a CU's LDS size, the alignment
// and carving of layouts, the cached device facts, the grow-only device and
// pinned buffers, the workspace pool with its lease and the stream a workspace
// owns, event-pair timing, capture-then-replay of a repeated launch segment,
// the dense variable index, and the DPLL launches' per-stream state (the check
// of host arrays is batch_keys.h, what the batched entry points share besides
// is batch_host.h).  Host code only; device helpers are in common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace satmi {

#define SATMI_TRY(x)                     \
    do {                                 \
        int _rc = (x);                   \
        if (_rc != SATMI_OK) return _rc; \
    } while (0)

// A refused argument, under the entry point's name `who`.
inline int fail_arg(const char *who, const char *what) {
    set_error(std::string(who) + ": " + what);
    return SATMI_ERR_ARG;
}

constexpr uint32_t LDS_PER_CU = 160u * 1024u;   // bytes of LDS a CU's workgroups share

// Layout builders place their arrays on 16-byte boundaries.
template <class U>
constexpr U align16(U x) { return (x + 15u) & ~(U)15u; }

// Offsets of the arrays of one block, each 256-byte aligned; `at` ends as its size.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t off = at;
        at += (bytes + 255) & ~(size_t)255;
        return off;
    }
};

// ---------------------------------------------------------------- device facts
// What the launch paths ask about the current device, queried once per device.
struct DeviceFacts {
    int cus = 256;               // compute units
    double ticks_per_s = 1e8;    // s_memrealtime ticks per second (the constant wall clock)
};
inline int device_facts(DeviceFacts *out, int *dev_out = nullptr) {
    static std::mutex mu;
    static std::vector<std::pair<bool, DeviceFacts>> known;
    int dev = 0;
    SATMI_HIP(hipGetDevice(&dev));
    if (dev_out) *dev_out = dev;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)known.size() <= dev) known.resize(dev + 1);
    auto &k = known[dev];
    if (!k.first) {
        int cus = 0, khz = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            k.second.cus = cus;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
            k.second.ticks_per_s = (double)khz * 1000.0;
        k.first = true;
    }
    *out = k.second;
    return SATMI_OK;
}

// ---------------------------------------------------------------- device buffer
// Who ran out of device memory and what the caller can do about it.
struct OomText {
    const char *entry, *remedy;
};

// Grow-only device memory.  Three ways to get room, for three lifetimes:
//   reserve  frees first and allocates exactly what is asked (contents lost):
//            the lowest peak, for gigabyte candidate buffers and arenas;
//   move_to  allocates exactly `want`, fills it, keeps a prefix by a copy on
//            `s`, and frees the old buffer once `s` has drained;
//   grow     move_to with half as much again, for buffers that grow step by step.
// With `oom`, a request beyond the free device memory is SATMI_ERR_NOMEM with
// that text; without, it is whatever hipMalloc answers.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    int reserve(size_t bytes, const OomText *oom = nullptr) {
        if (bytes <= cap) return SATMI_OK;
        release();
        const size_t want = std::max<size_t>(bytes, 256);
        SATMI_TRY(alloc(&p, want, oom));
        cap = want;
        return SATMI_OK;
    }
    int move_to(size_t want, hipStream_t s, const OomText *oom, size_t keep = 0, int fill = -1) {
        void *np = nullptr;
        SATMI_TRY(alloc(&np, want, oom));
        if (fill >= 0) SATMI_HIP(hipMemsetAsync(np, fill, want, s));
        if (p && keep) SATMI_HIP(hipMemcpyAsync(np, p, std::min(keep, cap), hipMemcpyDeviceToDevice, s));
        if (p) {
            SATMI_HIP(hipStreamSynchronize(s));   // the old buffer is no longer read
            (void)hipFree(p);
        }
        p = np;
        cap = want;
        return SATMI_OK;
    }
    int grow(size_t bytes, hipStream_t s, const OomText *oom, size_t keep = 0, int fill = -1) {
        return bytes <= cap ? SATMI_OK : move_to(std::max<size_t>(bytes + bytes / 2, 256), s, oom, keep, fill);
    }
    template <class T>
    T *as() const { return (T *)p; }

private:
    static int alloc(void **np, size_t want, const OomText *oom) {
        size_t free_b = 0, total_b = 0;
        if (oom && hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b) {
            set_error(std::string(oom->entry) + ": out of device memory (" + std::to_string(want >> 20) +
                      " MiB wanted, " + std::to_string(free_b >> 20) + " MiB free); " + oom->remedy);
            return SATMI_ERR_NOMEM;
        }
        SATMI_HIP(hipMalloc(np, want));
        return SATMI_OK;
    }
};

// Grow-only pinned host memory (contents lost on regrowth): a call's inputs
// are gathered here and sent in one copy (a copy from pageable memory is staged
// synchronously, one per array), and small results come back through it.
// `reserve` allocates exactly what is asked, `grow` half as much again.
struct PinBuf {
    unsigned char *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    int reserve(size_t bytes, unsigned flags = hipHostMallocDefault) {
        if (bytes <= cap) return SATMI_OK;
        release();
        const size_t want = std::max<size_t>(bytes, 4096);
        SATMI_HIP(hipHostMalloc((void **)&p, want, flags));
        cap = want;
        return SATMI_OK;
    }
    int grow(size_t bytes) { return bytes <= cap ? SATMI_OK : reserve(bytes + bytes / 2); }
};

// ---------------------------------------------------------------- workspace pool
// The device state of one call of a solver (a workspace W: its buffers, a
// non-blocking stream, pinned words), kept between calls in a process-wide
// pool: a call takes a free workspace of its device or makes one, and returns
// it when done, so concurrent calls from any number of host threads each own
// one and the number of workspaces is the peak number of concurrent calls.
// W has `int dev`, `hipStream_t stream` and `bool open()` (creates the stream
// and whatever else a fresh workspace needs): it derives from WorkStream.
struct WorkStream {
    int dev = 0;
    hipStream_t stream = nullptr;
    WorkStream() = default;
    WorkStream(const WorkStream &) = delete;
    WorkStream &operator=(const WorkStream &) = delete;
    // a base's destructor runs after the members of the workspace went: its
    // graph, events and buffers are gone before their stream
    ~WorkStream() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool open() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess; }
};

template <class W>
struct Pool {
    static Pool &get() {
        static Pool *p = new Pool;   // never destroyed: no hipFree after the runtime's teardown
        return *p;
    }
    W *acquire(int dev) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < free_list.size(); ++i)
                if (free_list[i]->dev == dev) {
                    W *w = free_list[i];
                    free_list.erase(free_list.begin() + (long)i);
                    return w;
                }
        }
        W *w = new W;
        w->dev = dev;
        if (!w->open()) {
            delete w;
            return nullptr;
        }
        return w;
    }
    void release(W *w) {
        std::lock_guard<std::mutex> g(mu);
        free_list.push_back(w);
    }
    // Free every idle workspace; calls in flight keep theirs.
    void trim() {
        std::vector<W *> idle;
        {
            std::lock_guard<std::mutex> g(mu);
            idle.swap(free_list);
        }
        for (W *w : idle) destroy(w);
    }
    static void destroy(W *w) {
        (void)hipStreamSynchronize(w->stream);
        delete w;
    }

private:
    std::mutex mu;
    std::vector<W *> free_list;
};

// A call's hold on a workspace: back to the pool after a call that set `ok`,
// destroyed (once its stream drained) after one that failed part-way and may
// have left device state that the next call would trust.
template <class W>
struct Lease {
    W *w;
    bool ok = false;
    ~Lease() {
        if (!w) return;
        if (ok) Pool<W>::get().release(w);
        else Pool<W>::destroy(w);
    }
};

// ---------------------------------------------------------------- event-pair timing
// Times launches on one stream: begin() / end() bracket them, total() sums.
// The pairs are kept between calls (reset() starts a call's count afresh); a
// failure is SATMI_ERR_HIP under the caller's name `who`.
struct EventTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    EventTimer() = default;
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer() {
        for (auto &e : ev) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    }
    int begin(hipStream_t s, const char *who) {
        if (used == ev.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
                if (a) (void)hipEventDestroy(a);
                set_error(std::string(who) + ": hipEventCreate failed");
                return SATMI_ERR_HIP;
            }
            ev.push_back({a, b});
        }
        return record(ev[used].first, s, who);
    }
    int end(hipStream_t s, const char *who) { return record(ev[used++].second, s, who); }
    void reset() { used = 0; }
    double total() const {   // after the stream drained
        double ms = 0.0;
        for (size_t i = 0; i < used; ++i) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ev[i].first, ev[i].second) == hipSuccess) ms += t;
        }
        return ms;
    }

private:
    static int record(hipEvent_t e, hipStream_t s, const char *who) {
        const hipError_t rc = hipEventRecord(e, s);
        return rc == hipSuccess ? SATMI_OK : hip_fail(rc, (std::string(who) + ": hipEventRecord").c_str());
    }
};

// ---------------------------------------------------------------- graph replay
// A segment of launches that a workspace enqueues again and again with the
// same arguments: the first time it is enqueued plainly and its key (the bytes
// of everything its launches read from the host: build it as a zero-initialised
// struct, so padding compares equal) is remembered; the second time the same
// key comes it is captured into a HIP graph, and from then on replayed with one
// launch.  `enqueue` puts the segment on the stream and returns a SATMI_* code.
struct ReplayGraph {
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned char> key;
    ReplayGraph() = default;
    ReplayGraph(const ReplayGraph &) = delete;
    ReplayGraph &operator=(const ReplayGraph &) = delete;
    ~ReplayGraph() { reset(); }
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
        key.clear();
    }
    template <class Key, class F>
    int run(hipStream_t s, const Key &k, F &&enqueue) {
        static_assert(std::is_trivially_copyable<Key>::value, "a key is compared as bytes");
        const bool same = key.size() == sizeof(Key) && std::memcmp(key.data(), &k, sizeof(Key)) == 0;
        if (same && exec) {
            SATMI_HIP(hipGraphLaunch(exec, s));
        } else if (same) {
            hipGraph_t graph = nullptr;
            SATMI_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue();
            const hipError_t ec = hipStreamEndCapture(s, &graph);
            if (rc != SATMI_OK || ec != hipSuccess) {
                if (graph) (void)hipGraphDestroy(graph);
                reset();
                if (rc != SATMI_OK) return rc;
                SATMI_HIP(ec);
            }
            const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            SATMI_HIP(ei);
            SATMI_HIP(hipGraphLaunch(exec, s));
        } else {   // remember the segment: captured if it comes again
            reset();
            key.assign((const unsigned char *)&k, (const unsigned char *)&k + sizeof(Key));
            return enqueue();
        }
        return SATMI_OK;
    }
};

// ---------------------------------------------------------------- dense variable index
// Numbers the variables that occur in the checked literals lits[lo .. hi) of a
// formula (batch_keys.h: none is 0 or INT32_MIN, `maxvar` is their largest
// variable), in ascending order of their ids: var2dense[v] = index or -1,
// dense2var[index] = v.
inline void dense_var_index(const int32_t *lits, int64_t lo, int64_t hi, int maxvar,
                            std::vector<int32_t> *var2dense, std::vector<int32_t> *dense2var) {
    var2dense->assign((size_t)maxvar + 1, -1);
    dense2var->clear();
    for (int64_t i = lo; i < hi; ++i) (*var2dense)[std::abs(lits[i])] = 1;
    for (int v = 1; v <= maxvar; ++v)
        if ((*var2dense)[v] >= 0) {
            (*var2dense)[v] = (int32_t)dense2var->size();
            dense2var->push_back(v);
        }
}

// ---------------------------------------------------------------- DPLL stream state
// What the DPLL launches keep per (device, stream); dpll.hip owns the map and
// looks a stream's state up once per launch.  Each stream has its own work
// counter, so batches launched on different streams (a pipelined caller
// overlapping one batch's tail with the next batch) never share a queue.
// Launches on one stream are ordered, and its state belongs to whoever is
// launching on it: a scratch buffer is only replaced after the stream drained.
struct DpllStream {
    hipStream_t stream = nullptr;
    uint32_t *counter = nullptr;   // work counter + launch span (common.h), 256 B
    DevBuf occ;                    // incremental scan kernel: occurrence lists / snapshot overflow per wave
    DevBuf split;                  // branch splitting: head, slot pool, donation stacks
    DevBuf arena;                  // wide general kernel: per-wave HBM arenas
    uint32_t split_epoch = 0;      // the launch tag of the slot states
    bool split_last = false;       // the stream's last DPLL launch split (its statistics are valid)

    int scratch(DevBuf &b, size_t bytes) {
        if (bytes <= b.cap) return SATMI_OK;
        if (b.p) SATMI_HIP(hipStreamSynchronize(stream));
        return b.reserve(bytes);
    }
    // >= bytes of splitting scratch and the next launch tag (distinct per
    // launch on the stream); marks the launch as one that split
    int split_scratch(size_t bytes, uint32_t *epoch) {
        if (bytes > split.cap) {
            SATMI_TRY(scratch(split, bytes));
            // fresh memory: no stale state may carry the next tags
            const hipError_t e = hipMemsetAsync(split.p, 0, split.cap, stream);
            if (e != hipSuccess) {
                split.release();
                return hip_fail(e, "branch-splitting scratch: hipMemsetAsync");
            }
        }
        split_epoch = (split_epoch + 1u) & 0x0FFFFFFFu;
        if (split_epoch == 0u) split_epoch = 1u;
        *epoch = split_epoch;
        split_last = true;
        return SATMI_OK;
    }
};

}  // namespace satmi
