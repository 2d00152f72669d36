// ofdm_owned.hpp — move-only owners of the HIP resources that the host files
// hold: each releases its handle in its destructor, so a context, a plan or a
// temporary that goes away (on an error path too) frees what it had.
#pragma once
#include <hip/hip_runtime.h>

namespace ofdm {

// H: the raw handle (a pointer type, null = empty); Release: what frees it.
// Converts to H where a raw handle is wanted; put() empties the owner and
// gives the address for the HIP call that creates the resource.
template <class H, auto Release>
class Owned {
    H h_ = nullptr;

public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            (void)reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { (void)reset(); }

    H get() const { return h_; }
    operator H() const { return h_; }
    hipError_t reset()
    {
        const H h = h_;
        h_ = nullptr;
        return h ? Release(h) : hipSuccess;
    }
    H* put()
    {
        (void)reset();
        return &h_;
    }
};

template <class T>
using DevBuf = Owned<T*, hipFree>;            // hipMalloc'd
using HostBlock = Owned<void*, hipHostFree>;  // hipHostMalloc'd (pinned)
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

}  // namespace ofdm
