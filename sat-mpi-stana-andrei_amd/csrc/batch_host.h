// batch_host.h -- the launch-side pieces the two batched entry points
// (resolution_batch.hip, dp_batch.hip) share: the workspace a call leases, the
// persistent grid's size, the dynamic-LDS attribute (its blocks are carved with
// host.h's Carve).
// The launch sequences differ (Davis-Putnam launches twice when it records).
#pragma once
#include "batch_keys.h"
#include "host.h"

namespace satmi {

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
