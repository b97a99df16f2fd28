// device_mem.h — who owns a block of device or pinned memory: Buf<T, Mem>, a move-only pointer + capacity (in elements) that
// frees itself.  No HIP call in here: the memory comes from the policy Mem (static alloc(bytes) -> nullptr on failure, static
// release(p)); the library hands in hipMalloc / hipFree and hipHostMalloc / hipHostFree (gorder_hip.hip), tests/cabi/device_mem.cpp
// a counting malloc, so the ownership rules can be driven without a device.  Also the replica rule of the accumulator blocks.
#ifndef GORDER_DEVICE_MEM_H
#define GORDER_DEVICE_MEM_H

#include <stddef.h>
#include <stdint.h>

namespace gorder {

enum class Reserve { Kept, Grew, Failed };

template <typename T, typename Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept { swap(o); }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { reset(); swap(o); }
        return *this;
    }
    ~Buf() { reset(); }

    // exactly n elements in place of what was there (n == 0: nothing); false when the allocator fails (empty then)
    bool alloc(size_t n) {
        reset();
        if (n && (p_ = static_cast<T *>(Mem::alloc(n * sizeof(T))))) cap_ = n;
        return !n || p_;
    }
    // room for `need` elements, contents NOT kept: nothing happens when it fits, otherwise the old block is freed first and
    // need + need / 2 are asked for (Grew: a new block that holds nothing yet; Failed: empty, capacity 0)
    Reserve reserve(size_t need) {
        if (need <= cap_) return Reserve::Kept;
        return alloc(need + need / 2) ? Reserve::Grew : Reserve::Failed;
    }
    void reset() {
        if (p_) Mem::release(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void swap(Buf &o) noexcept {
        T *p = p_; p_ = o.p_; o.p_ = p;
        size_t c = cap_; cap_ = o.cap_; o.cap_ = c;
    }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }
    operator T *() const { return p_; }      // (the kernels' argument structs take it as the pointer it owns)

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// replicas of an accumulator block of `words` u64 against contention on its words: as many as wanted, halved while the
// replicas together would pass 64 MiB (never fewer than one)
constexpr size_t kReplicaBytesMax = (size_t)64 << 20;
inline uint32_t replica_count(uint32_t wanted, size_t words) {
    while (wanted > 1 && (size_t)wanted * words * sizeof(uint64_t) > kReplicaBytesMax) wanted /= 2;
    return wanted;
}

}  // namespace gorder

#endif
