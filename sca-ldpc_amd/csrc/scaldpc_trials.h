// Where a Monte-Carlo call's trial indices come from.  Every generator kernel is lane = slot of the call and forms the global
// trial index of its slot, the value the Philox counter carries; nothing after the generators knows trial indices.
//   TrialRange   slot b is trial first + b                (the contiguous entries: scaldpc_mc_*_run*)
//   TrialList    slot b is trial ids[b], a device array   (the list entries: scaldpc_mc_*_at*)
// The generators take either through a template parameter of their body, so both forms are one text.  `live` says that slot b
// exists (b < batch): the lanes of a ragged last tile read nothing of the list.  A live lane's read is 8 bytes, consecutive
// lanes consecutive addresses: one coalesced 512-B load per wave.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "scaldpc_common.h"

namespace scaldpc {

struct TrialRange {
    long first;
    __device__ __forceinline__ unsigned long long trial(long b, bool) const { return (unsigned long long)(first + b); }
};

struct TrialList {
    const long long *__restrict__ ids;
    __device__ __forceinline__ unsigned long long trial(long b, bool live) const { return live ? (unsigned long long)ids[b] : 0ull; }
};

// The host's view, handed down from an entry point to its launches: a first index, or the HOST list of an _at entry (listed;
// ids may then be null, which the argument checks refuse).
struct TrialSrc {
    int64_t first;
    const int64_t *ids;
    bool listed;
    static TrialSrc range(int64_t first) { return TrialSrc{first, nullptr, false}; }
    static TrialSrc list(const int64_t *ids) { return TrialSrc{0, ids, true}; }
};

// The refusals every entry shares: a negative first index; a null list; a negative entry, named by position and value.
// Writes the reason to msg and returns false.  batch must have been checked positive before a list is looked at.
inline bool trials_ok(const TrialSrc &ts, int batch, char *msg, size_t len)
{
    if (!ts.listed) {
        if (ts.first < 0) {
            snprintf(msg, len, "first_trial must not be negative");
            return false;
        }
        return true;
    }
    if (!ts.ids) {
        snprintf(msg, len, "trial_ids is NULL");
        return false;
    }
    for (int i = 0; i < batch; i++)
        if (ts.ids[i] < 0) {
            snprintf(msg, len, "trial_ids[%d] = %lld is negative", i, (long long)ts.ids[i]);
            return false;
        }
    return true;
}

// The same on the device, as the generator launches take it: the first index, or (ids) the device copy of the list.
struct DeviceTrials {
    long first = 0;
    const long long *ids = nullptr;
};

// A call's trials for its launches.  A list (always a HOST array) is copied on stream s into `block`, a buffer the handle owns
// (released by destroy, counted by scaldpc_debug_live_blocks); every Monte-Carlo entry drains s before it returns.
inline int stage_trials(Buf<long long> &block, const TrialSrc &ts, int batch, hipStream_t s, DeviceTrials *out)
{
    *out = DeviceTrials{(long)ts.first, nullptr};
    if (!ts.listed) return 0;
    SC_TRY(block.ensure((size_t)batch));
    SC_HIP(hipMemcpyAsync(block, ts.ids, sizeof(long long) * (size_t)batch, hipMemcpyHostToDevice, s));
    out->ids = block;
    return 0;
}

}  // namespace scaldpc
