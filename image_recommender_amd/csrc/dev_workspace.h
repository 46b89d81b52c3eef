// dev_workspace.h — the per-device workspace scheme of the entry points that own no index
// (knn_kmeans.hip, vlad.hip).  One workspace per device, shared by every call on it: calls hold
// `mu` while they enqueue, and a call on another stream than the previous one first waits for that
// call's event.  It lives as long as the process (never deleted: its buffers go with the process).
// Host code; not part of the public ABI.
#pragma once

#include <map>
#include <mutex>

#include "knn_index.h"

namespace imgrec {

// what a workspace derives from; its own members are the DevBufs its launches share
struct StreamHandoff {
    std::mutex mu;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    // around a call's launches on `st`, `mu` held
    int begin(hipStream_t st) {
        if (!done) KNN_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (used && last != st) KNN_HIP(hipStreamWaitEvent(st, done, 0));
        return KNN_OK;
    }
    int end(hipStream_t st) {
        KNN_HIP(hipEventRecord(done, st));
        last = st;
        used = true;
        return KNN_OK;
    }
};

template <class W>
W* per_device(int device) {
    static std::mutex mu;
    static std::map<int, W*> all;
    std::lock_guard<std::mutex> lk(mu);
    W*& w = all[device];
    if (!w) w = new W();
    return w;
}

// a stream of the call's own: drained, then destroyed
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
};

inline int have_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) KNN_FAIL(KNN_ENOSYS, "no HIP device visible");
    return KNN_OK;
}

}  // namespace imgrec
