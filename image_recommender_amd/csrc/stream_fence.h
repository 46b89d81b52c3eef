// stream_fence.h — the one keeper of the ordering contract of include/imgrec_knn.h: operations of
// one owner (an index, a per-device workspace) on mixed streams are always ordered, host forms
// synchronise, and two operations never use the owner's workspace concurrently.  Plain C++17 with
// no HIP include: the stream API is a policy of static functions that return 0 or the API's own
// error value, in the shape of HipStreams (knn_index.h): Stream and Event handles ({} = none),
// create_event / destroy_event, record, wait, sync_stream, sync_device, clear_error (forget the
// API's sticky last error), fail(e, call) (set the error text, return the error code) and
// DeviceScope(device) (set the device, then restore it).  The host check
// (tests/fuzz/stream_fence_check.cpp) drives the same code over a policy that logs every call.
#pragma once

#include <mutex>
#include <optional>

namespace imgrec {

// What the owner's last operation left behind.  Eager (the default): an asynchronous operation
// records the event on its stream as its last enqueued step, and the next operation on ANOTHER
// stream waits for that event; nothing depends on the old stream afterwards (it may be destroyed).
// Lazy (opt-in, knn_set_fence_mode): nothing is recorded while the stream stays the same; the event
// is recorded on the remembered stream only when a different stream arrives, so back-to-back
// operations on one stream pay no record (~5.7 us of idle GPU each on MI355X, profiles/r03/), but
// the remembered stream MUST outlive the next call (recording on a destroyed stream is a use after
// free, not a guaranteed error).  A lazy record that does report an error falls back to a
// device-wide synchronisation instead of wedging the owner.  Host forms leave no fence.
template <typename P>
class Fence {
public:
    using Stream = typename P::Stream;
    Fence() = default;
    Fence(const Fence&) = delete;
    Fence& operator=(const Fence&) = delete;
    ~Fence() { if (ev_) P::destroy_event(ev_); }

    bool lazy = false;
    bool set = false;           // an operation on `stream` may still run
    bool recorded = false;      // the event already marks its end
    Stream stream{};

    // the event, made on first use (an index makes it when it is created)
    int create() { return ev_ ? 0 : check(P::create_event(&ev_), "hipEventCreateWithFlags(&fence, hipEventDisableTiming)"); }
    // before an operation enqueues on st
    int begin(Stream st) {
        if (const int rc = create()) return rc;
        if (!set || stream == st) return 0;
        if (!recorded) {
            if (P::record(ev_, stream) != 0) {
                P::clear_error();
                set = false;
                return check(P::sync_device(), "hipDeviceSynchronize()");
            }
            recorded = true;
        }
        return check(P::wait(st, ev_), "hipStreamWaitEvent(st, fence, 0)");
    }
    // after an asynchronous operation's last enqueued step on st (end_raw: the API's own error
    // value and no error text, for the scope's clean-up)
    int end_raw(Stream st) {
        stream = st;
        set = true;
        const int e = lazy ? 0 : P::record(ev_, st);
        recorded = !lazy && e == 0;
        return e;
    }
    int end(Stream st) { return check(end_raw(st), "hipEventRecord(fence, st)"); }
    // after a host form (its stream drained before returning): nothing to wait for
    void end_synced() { set = recorded = false; }

private:
    static int check(int e, const char* call) { return e == 0 ? 0 : P::fail(e, call); }
    typename P::Event ev_{};
};

// One operation on an owner: holds the owner's lock and device from construction to destruction,
// begins on a stream (the caller's for *_device forms, the owner's own for host forms) and is
// finished with the operation's result code.  A scope that never begins only locks and sets the
// device.  A scope left begun but unfinished (an error exit: finish(rc != 0), or a return before
// it) still closes the fence, so what the failed call enqueued stays ordered before the next
// operation: the device form ends on its stream as for success, best effort; the host form
// synchronises its stream (no copy into the caller's memory stays in flight) and clears the fence.
// That clean-up never touches the error text: the caller sees the original failure.
template <typename P>
class OpScope {
public:
    using Stream = typename P::Stream;
    OpScope(std::mutex& mu, int device, Fence<P>& fence, Stream own) : lk_(mu), fence_(fence), own_(own) {
        if (device >= 0) dev_.emplace(device);
    }
    ~OpScope() {
        if (!begun_) return;
        if (!host_ && fence_.end_raw(st_) != 0) P::clear_error();
        if (host_) (void)P::sync_stream(st_), fence_.end_synced();
    }
    int begin(Stream st, bool host = false) {      // device form, on the caller's stream
        st_ = st;
        host_ = host;
        const int rc = fence_.begin(st);
        begun_ = rc == 0;
        return rc;
    }
    int begin_host() { return begin(own_, true); }  // host form, on the owner's own stream
    Stream stream() const { return st_; }
    // Success: the device form ends on its stream; the host form synchronises its stream (unless
    // `synced`: the body's last step already did) and clears the fence.
    int finish(int rc, bool synced = false) {
        if (!begun_ || rc != 0) return rc;
        begun_ = false;
        if (!host_) return fence_.end(st_);
        const int e = synced ? 0 : P::sync_stream(st_);
        fence_.end_synced();
        return e == 0 ? 0 : P::fail(e, "hipStreamSynchronize(stream)");
    }
    int finish_synced(int rc) { return finish(rc, true); }

private:
    std::lock_guard<std::mutex> lk_;
    std::optional<typename P::DeviceScope> dev_;
    Fence<P>& fence_;
    Stream own_, st_{};
    bool host_ = false, begun_ = false;
};

}  // namespace imgrec
