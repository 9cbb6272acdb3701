// Kernels whose workgroups WAIT for each other inside a launch (the register-resident fp64 Sinkhorn: the row slabs of a pair; the
// clustered fp64 layer tail: the four workgroups of a 16-row block) are admitted ONE LAUNCH AT A TIME per device, whatever stream
// they are on: a waiting workgroup holds its CU, and partly resident groups of several launches can fill the chip with waiters
// whose partners find no slot (measured with the Sinkhorn: four streams, every spin ran into its bound - sinkhorn_f64.hip).
// Such launches are only made through a CoopGroup: a run of launches on ONE stream (a forward, or one per-op call) that holds its
// device's chain locked while it enqueues them - only the ENQUEUE of exact-mode forwards is serialised per device, a millisecond of
// host time.  Before its first waiting launch the group waits for the event of the previous group that made one, unless that group
// was on the same stream (launches on one stream are ordered already); when it closes it records ONE event behind its last waiting
// launch (an event per launch cost ~3 us of gap each in the kernel trace: 18 clustered layer launches per one-pair forward).  The
// group asks once whether its stream is being captured into a graph; if so it is not chained() (an event wait on foreign work
// cannot be captured): the Sinkhorn launches unchained, the clustered layer tail is not used at all (its flags count launches: a
// replay would meet them already set).
// The chain is per PROCESS (one process per GPU is the model): two processes that run such launches on one device are
// not ordered against each other - a starved launch then runs into its spin bound (seconds) and the call is refused through the range
// status, never answered wrongly; MDGAT_F64_LAYER_FUSION=2 keeps the layer tails out of it.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "common.hpp"

struct CoopChain {
    std::mutex m;
    hipEvent_t ev = nullptr;                   // behind the last waiting launch of the previous group that made one
    hipStream_t last_stream = nullptr;         // that group's stream (only compared, never used: it may be gone)
    bool has_last = false;
    unsigned long long epoch = 0;              // launches of the clustered layer tail so far (its flags carry it)
    unsigned long long* cluster_flags = nullptr;
};

class CoopGroup {
    CoopChain* c_ = nullptr;
    std::unique_lock<std::mutex> lock_;        // (released after the destructor's body: the group is neither copied nor moved)
    hipStream_t s_ = nullptr;
    bool chained_ = false, admitted_ = false;

public:
    ~CoopGroup() {
        if (!admitted_) return;
        (void)hipEventRecord(c_->ev, s_);
        c_->last_stream = s_;
        c_->has_last = true;
    }
    // Locks the chain of device `dev` (the current one) for launches on `s`; after an error the group does nothing but unlock.
    int open(int dev, hipStream_t s) {
        static CoopChain chains[MDGAT_MAX_DEVICES];
        if (dev < 0 || dev >= MDGAT_MAX_DEVICES) { mdgat_set_error("launch chain: device %d out of range", dev); return MDGAT_ERR_BAD_ARG; }
        c_ = &chains[dev];
        lock_ = std::unique_lock<std::mutex>(c_->m);
        s_ = s;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(s, &st);
        chained_ = st == hipStreamCaptureStatusNone;
        if (chained_ && !c_->ev) return mdgat_check_hip(hipEventCreateWithFlags(&c_->ev, hipEventDisableTiming), "launch chain: hipEventCreate");
        return MDGAT_OK;
    }
    bool chained() const { return chained_; }
    hipStream_t stream() const { return s_; }
    CoopChain& chain() { return *c_; }
    // Before every waiting launch (nothing to do under capture or after the first).
    int admit() {
        if (!chained_ || admitted_) return MDGAT_OK;
        admitted_ = true;
        if (!c_->has_last || c_->last_stream == s_) return MDGAT_OK;
        return mdgat_check_hip(hipStreamWaitEvent(s_, c_->ev, 0), "launch chain: wait for the previous group");
    }
};
