// The owning buffer types of goworld_amd/csrc/gwaoi_mem.h, alone (no library, no world).
//
// Without a device every HIP allocation and creation call fails cleanly, which pins down the
// failure states: a non-zero status, an empty object, no-op reset() and destruction.  With a
// device the same checks run on the success states, and the group failure is an allocation no
// device can serve behind ones it can.  Prints "ok".
#include "gwaoi_mem.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

namespace {

template <class B>
bool empty(const B &b) {
    return b.get() == nullptr && b.cap() == 0;
}

// after alloc(n) returned rc: allocated with n elements, or empty with a status and an error
template <class B>
void check_alloc(const B &b, int rc, size_t n) {
    if (rc == GWAOI_OK) {
        CHECK(b.get() != nullptr && b.cap() == n && b.error() == hipSuccess);
    } else {
        CHECK(rc == GWAOI_ENOMEM || rc == GWAOI_EDEVICE);
        CHECK((rc == GWAOI_ENOMEM) == (b.error() == hipErrorOutOfMemory));
        CHECK(empty(b) && b.error() != hipSuccess);
    }
}

template <class B, class... Flags>
void buffer_checks(Flags... flags) {
    {
        B b;  // empty: reset and destruction are no-ops
        CHECK(empty(b) && !b);
        b.reset();
        CHECK(empty(b));
    }
    B a;
    int rc = a.alloc(100, flags...);
    check_alloc(a, rc, 100);
    rc = a.alloc(0, flags...);  // max(n, 1) elements, the old allocation released
    check_alloc(a, rc, 1);
    rc = a.alloc(300, flags...);
    check_alloc(a, rc, 300);
    auto *p = a.get();
    const size_t cap = a.cap();
    B b(std::move(a));  // move construction leaves the source empty
    CHECK(empty(a) && b.get() == p && b.cap() == cap);
    B c;
    (void)c.alloc(7, flags...);
    c = std::move(b);  // move assignment releases the target's own and leaves the source empty
    CHECK(empty(b) && c.get() == p && c.cap() == cap);
    B &self = c;
    c = std::move(self);
    CHECK(c.get() == p && c.cap() == cap);
    c.reset();
    CHECK(empty(c));
    c.reset();
}

template <class H, class Raw>
void handle_checks(unsigned flags) {
    {
        H h;
        CHECK(!h);
        h.reset();
        CHECK(!h);
    }
    H a;
    const int rc = a.create(flags);
    CHECK(rc == GWAOI_OK || rc == GWAOI_EDEVICE);
    CHECK((rc == GWAOI_OK) == (bool)a);
    const Raw raw = a;
    H b(std::move(a));
    CHECK(!a && (Raw)b == raw);
    H c;
    (void)c.create(flags);
    c = std::move(b);
    CHECK(!b && (Raw)c == raw);
    c.reset();
    CHECK(!c);
    c.reset();
}

}  // namespace

int main() {
    buffer_checks<gw::DevBuf<float>>();
    buffer_checks<gw::DevBuf<unsigned long long>>();
    buffer_checks<gw::PinnedBuf<uint32_t>>();
    buffer_checks<gw::PinnedBuf<char>>(gw::PinnedBuf<char>::kMapped);
    {
        gw::PinnedBuf<uint32_t> m;  // mapped memory carries its device address; unmapped has none
        if (m.alloc(16, m.kMapped) == GWAOI_OK) CHECK(m.dev() != nullptr);
        else CHECK(m.dev() == nullptr);
        gw::PinnedBuf<uint32_t> moved(std::move(m));
        CHECK(m.dev() == nullptr);
        if (moved.alloc(16) == GWAOI_OK) CHECK(moved.dev() == nullptr);
    }
    handle_checks<gw::Event, hipEvent_t>(hipEventDisableTiming);
    handle_checks<gw::Event, hipEvent_t>(hipEventDefault);
    handle_checks<gw::Stream, hipStream_t>(hipStreamNonBlocking);

    // a group grows together or not at all: the last member's allocation cannot be served (2^60
    // bytes), with or without a device, and every member is empty afterwards -- the ones
    // allocated before it in this call, and the one that still held an older allocation
    gw::DevBuf<uint32_t> g0, g1;
    gw::PinnedBuf<uint32_t> g2;
    gw::DevBuf<char> big;
    (void)g1.alloc(10);
    std::string msg;
    int rc = gw::alloc_all(msg, g0, 64, g1, 64, g2, 64, big, (size_t)1 << 60);
    CHECK(rc != GWAOI_OK && !msg.empty());
    CHECK(empty(g0) && empty(g1) && empty(g2) && empty(big));
    msg.clear();
    rc = gw::alloc_all(msg, g0, 64, g2, 64);  // and a group that can be served holds all of it
    if (rc == GWAOI_OK) CHECK(g0.cap() == 64 && g2.cap() == 64 && msg.empty());
    else CHECK(empty(g0) && empty(g2) && !msg.empty());
    msg.clear();
    rc = gw::alloc_pinned(msg, g2, 8);
    CHECK(rc == GWAOI_OK ? g2.cap() == 8 : (rc == GWAOI_EDEVICE && empty(g2) && !msg.empty()));
    std::puts("ok");
    return 0;
}
