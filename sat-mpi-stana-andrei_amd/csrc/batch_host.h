// batch_host.h -- the device-side pieces the batched entry points share: the
// staging of one carved block (dpll.hip, cdcl.hip), and for the entry points
// with a persistent grid (resolution_batch.hip, dp_batch.hip, check.hip) the
// workspace a call leases, the grid's size and the dynamic-LDS attribute.
// Blocks are carved with host.h's Carve; the launch sequences differ.
#pragma once
#include "batch_keys.h"
#include "host.h"

namespace satmi {

// One device block carved with Carve, and the stream its copies go on.
struct Staged {
    unsigned char *base;
    hipStream_t stream;
    template <class T>
    T *at(size_t off) const { return (T *)(base + off); }
    int up(size_t off, const void *src, size_t bytes) const {
        if (bytes) SATMI_HIP(hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, stream));
        return SATMI_OK;
    }
    int down(void *dst, size_t off, size_t bytes) const {   // a null `dst` is an output the caller does not want
        if (dst && bytes) SATMI_HIP(hipMemcpyAsync(dst, base + off, bytes, hipMemcpyDeviceToHost, stream));
        return SATMI_OK;
    }
};

// A call's device state, kept between calls in the workspace pool (host.h; one
// pool per entry point: each derives its own empty type).  Nothing in it is
// trusted by the next call, so it goes back to the pool whatever the outcome.
struct BatchWork : WorkStream {
    DevBuf up, out;     // the inputs, one upload; the outputs, zeroed, one copy back
    DevBuf keys_out, rec_off;   // record: the keys the kernel keeps; where each formula's go (Davis-Putnam)
    PinBuf up_h, out_h;
    void drop_large_record() {   // its keys are not kept in the pool past a large recorded batch
        if (keys_out.cap > ((size_t)64 << 20)) keys_out.release();
    }
};

// Workgroups of a persistent grid over B formulas: as many as the CUs hold --
// by LDS (`lds_bytes` dynamic and `lds_slack` static per workgroup), by a CU's
// 32 wave slots, and 16 at the most -- capped by the test knob `dbg_grid` (0 = none).
inline int batch_grid(const DeviceFacts &facts, size_t lds_bytes, size_t lds_slack, int threads, int B, int dbg_grid) {
    const int waves = threads / 64;
    const int per_cu =
        (int)std::max<size_t>(1, std::min<size_t>({LDS_PER_CU / (lds_bytes + lds_slack), (size_t)(32 / waves), 16}));
    const int grid = (int)std::min<int64_t>(B, (int64_t)facts.cus * per_cu);
    return dbg_grid > 0 ? std::min(grid, dbg_grid) : grid;
}

// More than 48 KiB of dynamic LDS has to be allowed per kernel.
inline int batch_allow_lds(const void *kernel, size_t lds_bytes) {
    if (lds_bytes > 48 * 1024)
        SATMI_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return SATMI_OK;
}

}  // namespace satmi
