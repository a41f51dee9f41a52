// Stand-alone host program for a sanitizer build (make sanitize-device-buffer): the branches of tsdf_amd/csrc/device_buffer.hpp,
// handle_order.hpp and handle_counters.hpp (the counter block) that a machine WITH a device never takes.  Run where there is no device,
// every hipMalloc fails; the program checks what a failed growth leaves behind, that releasing an empty handle does nothing, the order in
// which the frame of a host variant reports errors, what a handle's stream order does without an event, and what a counter block's
// failed create and its releases leave.  With a device the allocations succeed and the same invariants are checked on that side.
// Nothing is launched.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "device_buffer.hpp"
#include "handle_counters.hpp"
#include "handle_order.hpp"

static char g_message[512];
static hipError_t g_failed_with = hipSuccess;   // what hip_fail was last given
static const char *g_failed_what = nullptr;

namespace tsdf {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof(g_message), fmt, ap);
    va_end(ap);
}
int hip_fail(hipError_t e, const char *what) {
    g_failed_with = e;
    g_failed_what = what;
    return e == hipErrorOutOfMemory ? TSDF_ERR_NOMEM : TSDF_ERR_DEVICE;
}
}  // namespace tsdf

using namespace tsdf;

static int failures = 0;
#define EXPECT(cond, what)                                         \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAIL %s (line %d)\n", what, __LINE__);    \
            failures++;                                            \
        }                                                          \
    } while (0)

// a handle as the library makes them: a plain struct, all zero
struct Handle {
    float *floats;
    size_t floats_cap;
    void *bytes;
    size_t bytes_cap;
    unsigned *pairs;
    size_t pairs_cap;
};

int main() {
    Handle h;
    std::memset(&h, 0, sizeof(h));

    // release and free-all of an empty handle: nothing happens, nothing is touched
    device_release(h.floats, h.floats_cap);
    device_release(h.bytes, h.bytes_cap);
    device_free_all(h.floats, h.bytes, h.pairs);
    Handle zero;
    std::memset(&zero, 0, sizeof(zero));
    EXPECT(std::memcmp(&h, &zero, sizeof(h)) == 0, "release of an empty handle changes it");

    // want <= cap: nothing is done, not even with a pointer that is no allocation
    h.floats = reinterpret_cast<float *>(&h);
    h.floats_cap = 8;
    EXPECT(device_reserve(h.floats, h.floats_cap, (size_t)8) == hipSuccess && h.floats == reinterpret_cast<float *>(&h) && h.floats_cap == 8,
           "a reserve within the capacity touched the array");
    h.floats = nullptr;
    h.floats_cap = 0;
    EXPECT(device_reserve(h.floats, h.floats_cap, (size_t)0) == hipSuccess && !h.floats && h.floats_cap == 0, "a reserve of nothing");

    // growth, twice: a failure leaves the array empty, and the next call tries (and fails) again
    for (int round = 0; round < 2; round++) {
        const hipError_t e = device_reserve(h.floats, h.floats_cap, (size_t)100);
        if (e == hipSuccess) EXPECT(h.floats && h.floats_cap == 100, "a successful reserve");
        else EXPECT(!h.floats && h.floats_cap == 0, "a failed reserve does not leave the array empty");
        const hipError_t eb = device_reserve_bytes(h.bytes, h.bytes_cap, (size_t)100);
        if (eb == hipSuccess) EXPECT(h.bytes && h.bytes_cap == 100, "a successful reserve in bytes");
        else EXPECT(!h.bytes && h.bytes_cap == 0, "a failed reserve in bytes does not leave the array empty");
        const hipError_t eu = device_reserve_units(h.pairs, h.pairs_cap, (size_t)100, 2 * sizeof(unsigned));
        if (eu == hipSuccess) EXPECT(h.pairs && h.pairs_cap == 100, "a successful reserve in units");
        else EXPECT(!h.pairs && h.pairs_cap == 0, "a failed reserve in units does not leave the array empty");
        EXPECT(e == eb && e == eu, "the three forms disagree");
        if (round == 0) std::printf("hipMalloc here: %s\n", hipGetErrorString(e));
    }
    device_release(h.floats, h.floats_cap);
    device_release(h.bytes, h.bytes_cap);
    device_free_all(h.pairs);
    h.pairs_cap = 0;
    EXPECT(std::memcmp(&h, &zero, sizeof(h)) == 0, "release does not leave an empty handle");

    // the frame of a host variant
    const hipError_t sync_here = hipStreamSynchronize(nullptr);
    (void)hipGetLastError();
    HostStage st;
    g_message[0] = 0;
    const int rc = st.begin(nullptr, 4096, "caller: couldn't allocate %zu bytes");
    if (rc != TSDF_OK) {
        EXPECT(rc == TSDF_ERR_NOMEM && !st.buf && std::strcmp(g_message, "caller: couldn't allocate 4096 bytes") == 0,
               "a failed begin: TSDF_ERR_NOMEM with the caller's text");
    } else {
        EXPECT(st.buf && st.ok(), "a successful begin");
    }
    // (finish on whatever begin left -- a null buffer is fine -- in the order: the call's rc, the first copy failure, the synchronisation)
    char host[16] = {0};
    auto staged = [&](hipError_t copy_error) {
        HostStage s;
        s.stream = nullptr;
        s.buf = nullptr;
        s.e = copy_error;
        g_failed_with = hipSuccess;
        g_failed_what = nullptr;
        return s;
    };
    {
        HostStage s = staged(hipErrorInvalidValue);
        EXPECT(s.finish(TSDF_ERR_INVALID, "what") == TSDF_ERR_INVALID && g_failed_what == nullptr, "finish: the call's rc comes first");
    }
    {
        HostStage s = staged(hipErrorInvalidValue);
        EXPECT(s.finish(TSDF_OK, "what") == TSDF_ERR_DEVICE && g_failed_with == hipErrorInvalidValue && g_failed_what && !std::strcmp(g_failed_what, "what"),
               "finish: then the first copy failure");
    }
    {
        HostStage s = staged(hipSuccess);
        const int got = s.finish(TSDF_OK, "what");
        if (sync_here == hipSuccess) EXPECT(got == TSDF_OK && g_failed_what == nullptr, "finish: nothing failed");
        else EXPECT(got != TSDF_OK && g_failed_with == sync_here && g_failed_what && !std::strcmp(g_failed_what, "what"), "finish: then the synchronisation's failure");
    }
    {   // a copy that failed stops the copies behind it: the first failure is the one reported
        HostStage s = staged(hipErrorInvalidValue);
        s.up(host, host, sizeof(host));
        s.down(host, host, sizeof(host));
        EXPECT(s.e == hipErrorInvalidValue && !s.ok(), "up / down after a failure");
    }
    (void)st.finish(TSDF_OK, "what");
    (void)hipGetLastError();

    // the stream order of a handle (handle_order.hpp)
    HandleOrder none;
    std::memset(&none, 0, sizeof(none));
    auto untouched = [](const HandleOrder &o) { return o.device == 0 && !o.done && !o.pending; };
    {   // destroy of a handle that was never created: nothing happens
        HandleOrder o = none;
        o.destroy();
        EXPECT(untouched(o), "destroy of a zeroed handle order changes it");
    }
    {   // nothing in flight: join and wait return at once and touch neither the event (there is none) nor the error plumbing
        HandleOrder o = none;
        g_failed_what = nullptr;
        EXPECT(o.join(nullptr, "order") == TSDF_OK && o.wait("wait") == TSDF_OK && g_failed_what == nullptr, "join / wait with nothing pending");
        EXPECT(untouched(o), "join / wait with nothing pending change the handle order");
    }
    {   // create: without a device it fails and leaves no event, and destroy after it is clean; with one, the whole cycle
        HandleOrder o = none;
        const hipError_t e = o.create();
        (void)hipGetLastError();
        if (e != hipSuccess) {
            EXPECT(!o.done && !o.pending, "a failed create leaves an event or pending work");
            o.destroy();
            EXPECT(!o.done && !o.pending, "destroy after a failed create");
        } else {
            EXPECT(o.done && !o.pending, "a successful create");
            EXPECT(o.leave(nullptr, "event") == TSDF_OK && o.pending == 1, "leave");
            EXPECT(o.join(nullptr, "order") == TSDF_OK && o.pending == 1, "join keeps the work pending");
            EXPECT(o.wait("wait") == TSDF_OK && o.pending == 0, "wait");
            o.destroy();
            EXPECT(!o.done && !o.pending, "destroy");
        }
        std::printf("hipGetDevice / event here: %s\n", hipGetErrorString(e));
    }

    // the counter block of a handle (handle_counters.hpp), over a word array and over a struct of named words
    struct Named {
        unsigned long long a, b;
        unsigned rounds[4];
    };
    auto empty = [](const auto &b) { return !b.dev && !b.host; };
    {   // release of a block that was never created, and a second release: nothing happens
        CounterBlock<unsigned long long, 8> w;
        std::memset(&w, 0, sizeof(w));
        w.release();
        w.release();
        EXPECT(empty(w), "release of a zeroed counter block changes it");
        static_assert(CounterBlock<unsigned long long, 8>::device_bytes() == 64 && CounterBlock<Named>::device_bytes() == sizeof(Named), "the bytes a block holds");
    }
    {   // a half-created block: the mirror alone (hipHostFree of a null pointer and hipFree of a null pointer are both fine)
        CounterBlock<Named> w;
        std::memset(&w, 0, sizeof(w));
        if (hipHostMalloc((void **)&w.host, sizeof(Named), hipHostMallocDefault) != hipSuccess) w.host = nullptr;
        (void)hipGetLastError();
        w.release();
        EXPECT(empty(w), "release of a half-created counter block");
        w.release();
        EXPECT(empty(w), "a second release of a counter block");
    }
    {   // create: without a device it fails and leaves an empty block; with one, a zeroed mirror and the ranges
        CounterBlock<Named> w;
        std::memset(&w, 0xff, sizeof(w));   // (create does not read what the block held)
        const hipError_t e = w.create();
        (void)hipGetLastError();
        if (e != hipSuccess) {
            EXPECT(empty(w), "a failed create does not leave the counter block empty");
        } else {
            Named zero_words;
            std::memset(&zero_words, 0, sizeof(zero_words));
            EXPECT(w.dev && w.host && std::memcmp(w.host, &zero_words, sizeof(Named)) == 0, "a successful create: both sides, the mirror zeroed");
            w.host->b = 7;
            w.host->rounds[3] = 9;
            EXPECT(w.reset(nullptr) == hipSuccess && w.download(w.dev->rounds, 4, nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                       w.host->b == 7 && w.host->rounds[3] == 0,
                   "a range lands at its own place in the mirror and nowhere else");
            EXPECT(w.download(nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess && w.host->b == 0, "the whole block lands");
        }
        w.release();
        EXPECT(empty(w), "release after create");
        w.release();
        EXPECT(empty(w), "a second release after create");
        std::printf("counter block create here: %s\n", hipGetErrorString(e));
    }

    std::printf(failures ? "device buffer host checks: %d FAILED\n" : "device buffer host checks ok\n", failures);
    return failures ? 1 : 0;
}
