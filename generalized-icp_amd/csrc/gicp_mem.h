// gicp_mem.h — the host layer's owning buffers: DevBuf<T> for device memory, PinnedBuf<T> for
// pinned host memory.  A buffer owns its pointer and its capacity together, is move-only and frees itself,
// so no capacity can outlive its allocation and no owner needs a release list.  Free of HIP headers: the
// runtime is reached through the four functions below (defined once, in gicp_capi.cpp), which lets a
// stand-alone host program exercise this header over malloc (tests/native/mem_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>

namespace gicp {

// what a failing call reports to the C-ABI boundary: a GICP_E_* code and the text of gicp_last_error
struct Fail {
    int code;
    std::string msg;
};

// The seam.  The allocators take bytes (> 0) and throw Fail{GICP_E_HIP, ...} on failure; the frees ignore
// errors (and leave none behind in the runtime's last-error state).
void* dev_alloc(size_t bytes);
void dev_free(void* p) noexcept;
void* pinned_alloc(size_t bytes);
void pinned_free(void* p) noexcept;

template <class T, void* (*Alloc)(size_t), void (*Free)(void*) noexcept>
class OwnedBuf {
public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~OwnedBuf() { reset(); }

    // exactly max(n, 1) elements, whatever was held before (contents dropped).  The old block is freed first;
    // if the allocation throws, the buffer is empty, so the next call allocates again.
    void alloc(size_t n) {
        reset();
        n = std::max<size_t>(n, 1);
        p_ = static_cast<T*>(Alloc(n * sizeof(T)));
        cap_ = n;
    }
    // grow-only: reallocates (contents dropped) only when n exceeds the capacity, then with headroom, so a
    // stream of similar-sized clouds allocates once
    void reserve(size_t n) {
        if (p_ && n <= cap_) return;
        alloc(std::max<size_t>({n, (size_t)(cap_ * 1.125), 1}));
    }
    void reset() noexcept {
        if (p_) Free(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    bool empty() const { return !p_; }
    size_t capacity() const { return cap_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }   // launch sites and views pass a buffer where they passed its pointer
    T* operator->() const { return p_; }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements
};

template <class T>
using DevBuf = OwnedBuf<T, dev_alloc, dev_free>;
template <class T>
using PinnedBuf = OwnedBuf<T, pinned_alloc, pinned_free>;

// Allocate, initialise, publish: a buffer that needs initial contents is allocated as a local, `init(pointer)`
// fills it (and throws if it cannot), and only then does it become `member`.  A failure leaves `member` empty
// and frees the local, so the caller's "if (member.empty())" block runs again on the next call.
template <class Buf, class Init>
void alloc_init(Buf& member, size_t n, Init&& init) {
    Buf b;
    b.alloc(n);
    init(b.get());
    member = std::move(b);
}

}  // namespace gicp
