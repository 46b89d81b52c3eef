// dev_workspace.h — the per-device workspace scheme of the entry points that own no index
// (knn_kmeans.hip, vlad.hip, vladenc.hip).  One workspace per device, shared by every call on it:
// calls hold `mu` while they enqueue, and a call on another stream than the previous one first waits
// for that call's event (HandoffOp); on_workspace is that sequence around a call's body.  A
// workspace lives as long as the process (never deleted: its buffers go with the process).
// Host code; not part of the public ABI.
#pragma once

#include <map>
#include <mutex>

#include "knn_index.h"

namespace imgrec {

// what a workspace derives from; its own members are the DevBufs its launches share.  The fence
// is eager and makes its event on first use.
struct StreamHandoff {
    std::mutex mu;
    Fence<HipStreams> fence;
};
// one call's launches on the caller's stream: begin(st) ... finish(rc) (stream_fence.h OpScope; the
// device is the caller's current one)
struct HandoffOp : OpScope<HipStreams> {
    explicit HandoffOp(StreamHandoff* w) : OpScope(w->mu, -1, w->fence, nullptr) {}
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

// One call on the current device's workspace W, on the caller's stream: the lock, the hand-off from
// the previous call's stream, body(w) (its launches on st; an int code), the fence's end.  When the
// body fails, the scope's destructor still closes the fence over what it enqueued (stream_fence.h).
template <class W, class Body>
int on_workspace(hipStream_t st, Body body) {
    int device = 0;
    KNN_HIP(hipGetDevice(&device));
    W* w = per_device<W>(device);
    HandoffOp op(w);
    int rc = op.begin(st);
    if (rc == KNN_OK) rc = body(w);
    return op.finish(rc);
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
