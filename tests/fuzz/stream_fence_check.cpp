// stream_fence_check.cpp — host check of csrc/stream_fence.h (tests/test_stream_fence_cpu.py builds
// it with -fsanitize=address,undefined and runs it with leak detection on).  The fence and the
// operation scope run over a stream API that logs every call and can be told to fail the n-th one.
// The expected call logs are literals, written down from the index's former fence_begin /
// fence_end / fence_end_synced and StreamHandoff::begin / end: they pin what the scope must still
// do, they are not derived from it.  Every expectation is a CHECK that aborts with its line.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../image_recommender_amd/csrc/stream_fence.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::abort();                                                 \
        }                                                                 \
    } while (0)

namespace {

constexpr int kEHIP = -2;
using Log = std::vector<std::string>;

// Streams are small integers (A, B, the owner's own H); an event is a heap block, so one that is
// never destroyed is a leak the sanitizer reports.  A failing call is logged with a '!'.
struct Fake {
    using Stream = int;
    using Event = int*;
    static inline Log log;
    static inline long calls = 0, fail_at = -1;      // the failable call with this ordinal fails
    static inline int fails = 0;                     // fail() calls: error texts written
    static inline std::string err;
    static inline int device = 3;                    // the caller's current device
    struct DeviceScope {
        int old;
        explicit DeviceScope(int dev) : old(device) { device = dev; }
        ~DeviceScope() { device = old; }
    };
    static int call(const std::string& what) {
        const bool bad = calls++ == fail_at;
        log.push_back(what + (bad ? "!" : ""));
        return bad ? 700 : 0;
    }
    static std::string name(Stream s) { return s == 1 ? "A" : s == 2 ? "B" : s == 9 ? "H" : "?"; }
    static int create_event(Event* e) {
        const int rc = call("create");
        if (rc == 0) *e = new int(0);
        return rc;
    }
    static void destroy_event(Event e) { log.push_back("destroy"); delete e; }
    static int record(Event e, Stream s) { CHECK(e); return call("record " + name(s)); }
    static int wait(Stream s, Event e) { CHECK(e); return call("wait " + name(s)); }
    static int sync_stream(Stream s) { return call("sync " + name(s)); }
    static int sync_device() { return call("sync_device"); }
    static void clear_error() { log.push_back("clear"); }
    static int fail(int e, const char* what) {
        CHECK(e == 700);
        ++fails;
        err = std::string(what) + " failed";
        return kEHIP;
    }
    static void fresh() {
        log.clear();
        calls = 0;
        fail_at = -1;
        fails = 0;
        err.clear();
    }
};
constexpr int A = 1, B = 2, H = 9, kOwnerDevice = 5;
using Fence = imgrec::Fence<Fake>;
using Scope = imgrec::OpScope<Fake>;

// an index-like owner (its event made at creation, a device and a stream of its own) ...
struct Owner {
    std::mutex mu;
    Fence fence;
    explicit Owner(bool lazy) {
        fence.lazy = lazy;
        CHECK(fence.create() == 0);
        Fake::fresh();
    }
    // the lock released and the caller's device back: after every operation
    void idle() {
        CHECK(mu.try_lock());
        mu.unlock();
        CHECK(Fake::device == 3);
    }
    int device_op(int st, int rc = 0) {
        {
            Scope op(mu, kOwnerDevice, fence, H);
            CHECK(Fake::device == kOwnerDevice);
            CHECK(op.begin(st) == 0 && op.stream() == st);
            rc = op.finish(rc);
        }
        idle();
        return rc;
    }
    int host_op(int rc = 0) {
        {
            Scope op(mu, kOwnerDevice, fence, H);
            CHECK(op.begin_host() == 0 && op.stream() == H);
            rc = op.finish(rc);
        }
        idle();
        return rc;
    }
};
// ... and a workspace-like one: no device of its own, the event made by its first operation
struct Handoff {
    std::mutex mu;
    Fence fence;
    int op(int st) {
        int rc;
        {
            Scope op(mu, -1, fence, 0);
            CHECK(Fake::device == 3);
            rc = op.begin(st);
            rc = op.finish(rc);
        }
        CHECK(mu.try_lock());
        mu.unlock();
        return rc;
    }
};

void success_logs() {
    {   // eager: A, A, B
        Owner o(false);
        CHECK(o.device_op(A) == 0 && o.device_op(A) == 0 && o.device_op(B) == 0);
        CHECK((Fake::log == Log{"record A", "record A", "wait B", "record B"}));
        CHECK(o.fence.set && o.fence.recorded && o.fence.stream == B);
    }
    {   // eager: A, host, B — the host form waits for A, drains its own stream and leaves no fence
        Owner o(false);
        CHECK(o.device_op(A) == 0 && o.host_op() == 0);
        CHECK(!o.fence.set && !o.fence.recorded);
        CHECK(o.device_op(B) == 0);
        CHECK((Fake::log == Log{"record A", "wait H", "sync H", "record B"}));
    }
    {   // lazy: A, A, A, B — no record until the switch, then one record on A and one wait on B
        Owner o(true);
        CHECK(o.device_op(A) == 0 && o.device_op(A) == 0 && o.device_op(A) == 0);
        CHECK(Fake::log.empty() && o.fence.set && !o.fence.recorded && o.fence.stream == A);
        CHECK(o.device_op(B) == 0);
        CHECK((Fake::log == Log{"record A", "wait B"}));
        CHECK(o.fence.set && !o.fence.recorded && o.fence.stream == B);
    }
    {   // lazy, the record failing: a device synchronisation, a cleared fence, OK, and no wait
        Owner o(true);
        CHECK(o.device_op(A) == 0);
        Fake::fail_at = 0;
        {
            Scope op(o.mu, kOwnerDevice, o.fence, H);
            CHECK(op.begin(B) == 0);
            CHECK(!o.fence.set && !o.fence.recorded);
            CHECK(op.finish(0) == 0);
        }
        o.idle();
        CHECK((Fake::log == Log{"record A!", "clear", "sync_device"}));
        CHECK(Fake::fails == 0 && Fake::err.empty());
        CHECK(o.device_op(B) == 0);                  // the next operation: nothing to wait for
        CHECK(Fake::log.size() == 3);
    }
    {   // a host form, then any stream: no wait
        Owner o(false);
        CHECK(o.host_op() == 0 && o.device_op(B) == 0);
        CHECK((Fake::log == Log{"sync H", "record B"}));
    }
    {   // a host form whose body's last step synchronised the stream: cleared without another wait
        Owner o(false);
        CHECK(o.device_op(A) == 0);
        {
            Scope op(o.mu, kOwnerDevice, o.fence, H);
            CHECK(op.begin_host() == 0 && op.finish_synced(0) == 0);
        }
        o.idle();
        CHECK((Fake::log == Log{"record A", "wait H"}));
        CHECK(!o.fence.set);
    }
}

void handoff_logs() {
    Fake::fresh();
    {   // A, A, B: the event made by the first call
        Handoff w;
        CHECK(w.op(A) == 0 && w.op(A) == 0 && w.op(B) == 0);
        CHECK((Fake::log == Log{"create", "record A", "record A", "wait B", "record B"}));
    }
    CHECK(Fake::log.back() == "destroy");
    Fake::fresh();
    {   // the event's creation failing: the call fails with that error and makes no other call; the
        // next call tries again
        Handoff w;
        Fake::fail_at = 0;
        CHECK(w.op(A) == kEHIP && Fake::fails == 1);
        CHECK(Fake::err == "hipEventCreateWithFlags(&fence, hipEventDisableTiming) failed");
        CHECK((Fake::log == Log{"create!"}));
        CHECK(w.op(A) == 0);
        CHECK((Fake::log == Log{"create!", "create", "record A"}));
    }
}

// An operation that fails with code -7 and the text "original" after it began; clean_fails: the
// clean-up's own first call fails too.
int failing_op(Owner& o, int st, bool host, bool clean_fails) {
    int rc;
    {
        Scope op(o.mu, kOwnerDevice, o.fence, H);
        CHECK((host ? op.begin_host() : op.begin(st)) == 0);
        Fake::err = "original";
        if (clean_fails) Fake::fail_at = Fake::calls;
        rc = op.finish(-7);
        CHECK(rc == -7);
    }
    o.idle();
    CHECK(Fake::err == "original" && Fake::fails == 0);
    return rc;
}

void error_exits() {
    {   // device form, eager: the fence names st and is recorded
        Owner o(false);
        failing_op(o, A, false, false);
        CHECK((Fake::log == Log{"record A"}));
        CHECK(o.fence.set && o.fence.recorded && o.fence.stream == A);
        CHECK(o.device_op(B) == 0);                  // ... so the next stream waits for it
        CHECK((Fake::log == Log{"record A", "wait B", "record B"}));
    }
    {   // device form, lazy: the fence remembers st
        Owner o(true);
        failing_op(o, A, false, false);
        CHECK(Fake::log.empty() && o.fence.set && !o.fence.recorded && o.fence.stream == A);
    }
    {   // device form, the clean-up's record failing: st stays remembered, the text is the original
        Owner o(false);
        failing_op(o, A, false, true);
        CHECK((Fake::log == Log{"record A!", "clear"}));
        CHECK(o.fence.set && !o.fence.recorded && o.fence.stream == A);
    }
    {   // a return before finish() is the same exit
        Owner o(false);
        {
            Scope op(o.mu, kOwnerDevice, o.fence, H);
            CHECK(op.begin(B) == 0);
        }
        o.idle();
        CHECK((Fake::log == Log{"record B"}));
    }
    {   // host form: synchronised before the scope ends, the fence clear
        Owner o(false);
        CHECK(o.device_op(A) == 0);
        failing_op(o, H, true, false);
        CHECK((Fake::log == Log{"record A", "wait H", "sync H"}));
        CHECK(!o.fence.set && !o.fence.recorded);
    }
    {   // host form, the clean-up's synchronisation failing
        Owner o(false);
        failing_op(o, H, true, true);
        CHECK((Fake::log == Log{"sync H!"}));
        CHECK(!o.fence.set);
    }
    {   // a successful host form whose own synchronisation fails reports that, with the fence clear
        Owner o(false);
        Fake::fail_at = 0;
        CHECK(o.host_op() == kEHIP && Fake::fails == 1);
        CHECK(Fake::err == "hipStreamSynchronize(stream) failed");
        CHECK((Fake::log == Log{"sync H!"}));
        CHECK(!o.fence.set);
    }
    {   // a begin that fails (the wait) is not begun: nothing to clean up
        Owner o(false);
        CHECK(o.device_op(A) == 0);
        Fake::fail_at = Fake::calls;
        {
            Scope op(o.mu, kOwnerDevice, o.fence, H);
            CHECK(op.begin(B) == kEHIP);
        }
        o.idle();
        CHECK((Fake::log == Log{"record A", "wait B!"}));
        CHECK(Fake::err == "hipStreamWaitEvent(st, fence, 0) failed");
    }
}

void never_begun() {
    Owner o(false);
    CHECK(o.device_op(A) == 0);
    Fake::fresh();
    {
        Scope op(o.mu, kOwnerDevice, o.fence, H);
        CHECK(Fake::device == kOwnerDevice);
        CHECK(op.finish(0) == 0 && op.finish_synced(0) == 0 && op.finish(-7) == -7);
    }
    o.idle();
    CHECK(Fake::log.empty() && Fake::calls == 0);
    CHECK(o.fence.set && o.fence.recorded && o.fence.stream == A);     // untouched
}

}  // namespace

int main() {
    success_logs();
    handoff_logs();
    error_exits();
    never_begun();
    std::printf("stream_fence_check: ok\n");
    return 0;
}
