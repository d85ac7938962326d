// Host resource ownership: the one place in csrc/ that allocates and frees device memory, pinned
// host memory, events and streams.  Four move-only owners; an owner struct holds them as members,
// so `delete` of the struct releases everything and no destroy list can miss one.  Not part of the
// public ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/gwaoi.h"

namespace gw {

void world_set_error(gwaoi_world *w, const char *msg);  // gwaoi_world.cpp

// Where an error message goes: an owner's own string, or a world's last_error.
inline void set_error(std::string &dst, const std::string &msg) { dst = msg; }
inline void set_error(gwaoi_world *w, const std::string &msg) { world_set_error(w, msg.c_str()); }

// Returns GWAOI_EDEVICE from the enclosing function, with the message in `sink` (see set_error),
// when a HIP call fails.
#define HIP_TRY(sink, expr)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            gw::set_error(sink, std::string(#expr) + ": " + hipGetErrorString(e_));          \
            return GWAOI_EDEVICE;                                                            \
        }                                                                                    \
    } while (0)

inline int alloc_status(hipError_t e) {
    return e == hipSuccess ? GWAOI_OK : e == hipErrorOutOfMemory ? GWAOI_ENOMEM : GWAOI_EDEVICE;
}

// A hipMalloc allocation of cap() elements.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)), err_(o.err_) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    // Frees what it holds, then allocates max(n, 1) elements.  On failure the buffer is empty and
    // error() tells why.
    int alloc(size_t n) {
        reset();
        if (n == 0) n = 1;
        err_ = hipMalloc((void **)&p_, n * sizeof(T));
        if (err_ != hipSuccess) p_ = nullptr;
        else cap_ = n;
        return alloc_status(err_);
    }
    void reset() {
        if (p_) (void)hipFree((void *)p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }
    hipError_t error() const { return err_; }  // of the last alloc

  private:
    T *p_ = nullptr;
    size_t cap_ = 0;
    hipError_t err_ = hipSuccess;
};

// A hipHostMalloc allocation of cap() elements.  Mapped memory (kMapped) also has dev(), the
// address a kernel writes it through.
template <class T>
class PinnedBuf {
  public:
    static constexpr unsigned kMapped = hipHostMallocMapped | hipHostMallocCoherent;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept
        : p_(std::exchange(o.p_, nullptr)), dev_(std::exchange(o.dev_, nullptr)), cap_(std::exchange(o.cap_, 0)),
          err_(o.err_) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            dev_ = std::exchange(o.dev_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    int alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        reset();
        if (n == 0) n = 1;
        err_ = hipHostMalloc((void **)&p_, n * sizeof(T), flags);
        if (err_ != hipSuccess) {
            p_ = nullptr;
            return alloc_status(err_);
        }
        cap_ = n;
        if ((flags & hipHostMallocMapped) && (err_ = hipHostGetDevicePointer((void **)&dev_, p_, 0)) != hipSuccess)
            reset();
        return alloc_status(err_);
    }
    void reset() {
        if (p_) (void)hipHostFree((void *)p_);
        p_ = dev_ = nullptr;
        cap_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }
    size_t cap() const { return cap_; }
    hipError_t error() const { return err_; }

  private:
    T *p_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0;
    hipError_t err_ = hipSuccess;
};

// A hipEvent_t or hipStream_t, created with flags.
template <class H, hipError_t (*Create)(H *, unsigned), hipError_t (*Destroy)(H)>
class Handle {
  public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    int create(unsigned flags) {
        reset();
        if (Create(&h_, flags) == hipSuccess) return GWAOI_OK;
        h_ = nullptr;
        return GWAOI_EDEVICE;
    }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    operator H() const { return h_; }

  private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

template <class X>
constexpr bool kMoveOnly = std::is_nothrow_move_constructible<X>::value && std::is_nothrow_move_assignable<X>::value &&
                           !std::is_copy_constructible<X>::value && !std::is_copy_assignable<X>::value;
static_assert(kMoveOnly<DevBuf<int>> && kMoveOnly<PinnedBuf<int>> && kMoveOnly<Event> && kMoveOnly<Stream>,
              "an owner is never copied");

// Allocates a group of buffers that grow together, given as (buffer, elements) pairs: either all
// of them hold their new allocation, or (after the first failure, whose message goes to `sink`)
// every one of them is empty.
inline void reset_all() {}
template <class B, class... Rest>
void reset_all(B &b, size_t, Rest &&...rest) {
    b.reset();
    reset_all(rest...);
}
template <class Sink>
int alloc_each(Sink &) {
    return GWAOI_OK;
}
template <class Sink, class B, class... Rest>
int alloc_each(Sink &sink, B &b, size_t n, Rest &&...rest) {
    if (const int rc = b.alloc(n)) {
        set_error(sink, std::string("allocation of ") + std::to_string(n * sizeof(*b.get())) + " bytes: " +
                            hipGetErrorString(b.error()));
        return rc;
    }
    return alloc_each(sink, rest...);
}
template <class Sink, class... Pairs>
int alloc_all(Sink &&sink, Pairs &&...pairs) {
    const int rc = alloc_each(sink, pairs...);
    if (rc) reset_all(pairs...);
    return rc;
}

// One pinned buffer, for the owners to which a failed pinned allocation is a device error
// whatever HIP called it.
template <class Sink, class T>
int alloc_pinned(Sink &&sink, PinnedBuf<T> &b, size_t n, unsigned flags = hipHostMallocDefault) {
    if (b.alloc(n, flags) == GWAOI_OK) return GWAOI_OK;
    set_error(sink, std::string("hipHostMalloc: ") + hipGetErrorString(b.error()));
    return GWAOI_EDEVICE;
}

}  // namespace gw
