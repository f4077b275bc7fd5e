// nr_defer_policy.h — when a cached draw may leave its framebuffer and depth stores pending (deferred stores,
// nr_common.h DeferredStores).  Plain C++ with no HIP dependency: tests/test_defer_policy.py compiles it with
// the host compiler and walks the patterns below.
//
// Every cached batch that runs k_keys_idx leaves one record, whether it stored its values itself or left them
// pending.  A record ends in one of two ways:
//   superseded  both halves (colour, depth) were overwritten by clears before anything read them: the stores
//               served no result;
//   needed      something used the buffers first.  If the batch had deferred, a resolve kernel ran: a second
//               pass over the index and the records, which costs more than the stores it had saved.
// In automatic mode a batch defers only after `threshold` records in a row ended superseded.  A needed record
// resets the run; one that had deferred also doubles the threshold (up to THRESHOLD_MAX, never shrinking within a
// context).  So a caller who uses the buffers every frame never defers; one who uses them every N-th frame (N
// above the threshold) resolves after runs of N whose deferred share falls off geometrically: the k-th resolve
// comes only after a run of 2^k superseded records, and once the threshold has passed N there are none.
#pragma once

namespace nrdefer {

constexpr unsigned THRESHOLD_START = 2;
constexpr unsigned THRESHOLD_MAX = 1024;

struct Policy {
    unsigned run = 0;                        // consecutive records that ended superseded, never needed
    unsigned threshold = THRESHOLD_START;    // run length from which a batch defers
    // May the next cached batch defer (automatic mode)?
    bool allows() const { return run >= threshold; }
    // A record went away with both halves dead and neither ever needed (the batch had stored or not).
    void superseded() {
        if (run < ~0u) ++run;
    }
    // A record's values were needed (once per record, at its first use).  deferred: the batch had left them
    // pending, so a resolve kernel ran.
    void needed(bool deferred) {
        run = 0;
        if (deferred) threshold = threshold >= THRESHOLD_MAX / 2 ? THRESHOLD_MAX : threshold * 2;
    }
};

}  // namespace nrdefer
