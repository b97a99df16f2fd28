// Drives gorder_amd/csrc/device_mem.h (who owns the library's device and pinned blocks) without a device: a counting malloc
// policy that can be told to fail on the k-th allocation stands in for hipMalloc / hipFree.  Built with
// -fsanitize=address,undefined by tests/test_device_mem_cpu.py; exit status 0 and "device_mem ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace {

struct CountingMem {
    static size_t live, allocs, frees, fail_at;      // fail_at: the allocation (counted from 1) that fails, 0 = none
    static std::vector<char> log;                    // 'a' per allocation asked for, 'f' per block freed, in order
    static size_t last_bytes;
    static void *alloc(size_t bytes) {
        log.push_back('a');
        last_bytes = bytes;
        if (++allocs == fail_at) return nullptr;
        live++;
        return malloc(bytes);
    }
    static void release(void *p) {
        log.push_back('f');
        frees++;
        live--;
        free(p);
    }
    static void restart(size_t fail = 0) { live = allocs = frees = 0; fail_at = fail; log.clear(); last_bytes = 0; }
};
size_t CountingMem::live = 0, CountingMem::allocs = 0, CountingMem::frees = 0, CountingMem::fail_at = 0, CountingMem::last_bytes = 0;
std::vector<char> CountingMem::log;

using Buf = gorder::Buf<uint32_t, CountingMem>;
using gorder::Reserve;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int reserve_rules() {
    CountingMem::restart();
    {
        Buf b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0) == Reserve::Kept && CountingMem::allocs == 0);        // nothing asked for, nothing done
        CHECK(b.reserve(100) == Reserve::Grew);
        CHECK(b.capacity() == 150 && CountingMem::last_bytes == 150 * sizeof(uint32_t) && CountingMem::allocs == 1);
        uint32_t *first = b.get();
        for (size_t k = 0; k < 150; k++) first[k] = (uint32_t)k;                  // the whole capacity is there to write
        // a request that fits: no reallocation, the same block
        for (size_t need : {(size_t)0, (size_t)1, (size_t)100, (size_t)150})
            CHECK(b.reserve(need) == Reserve::Kept && b.get() == first && b.capacity() == 150 && CountingMem::allocs == 1);
        // one more: need + need / 2, and the old block goes before the new one is asked for
        CountingMem::log.clear();
        CHECK(b.reserve(151) == Reserve::Grew && b.capacity() == 151 + 75 && CountingMem::last_bytes == 226 * sizeof(uint32_t));
        CHECK(CountingMem::log.size() == 2 && CountingMem::log[0] == 'f' && CountingMem::log[1] == 'a');
        CHECK(CountingMem::live == 1);
        uint32_t *p = b;                                                          // the implicit conversion is the pointer
        CHECK(p == b.get() && p != nullptr);
        // exact allocation, and alloc(0) leaves nothing
        CHECK(b.alloc(7) && b.capacity() == 7 && CountingMem::last_bytes == 7 * sizeof(uint32_t) && CountingMem::live == 1);
        CHECK(b.alloc(0) && b.get() == nullptr && b.capacity() == 0 && CountingMem::live == 0);
    }
    CHECK(CountingMem::live == 0 && CountingMem::allocs == CountingMem::frees);
    return 0;
}

int failure_rules() {
    // the first allocation fails: empty
    CountingMem::restart(1);
    {
        Buf b;
        CHECK(b.reserve(10) == Reserve::Failed && b.get() == nullptr && b.capacity() == 0);
        CHECK(b.alloc(10) && b.get() != nullptr && b.capacity() == 10);           // (the next allocation works)
    }
    CHECK(CountingMem::live == 0);
    // a growth fails: the old block is gone already (freed first), pointer null, capacity 0 — and the buffer works again after
    CountingMem::restart(2);
    {
        Buf b;
        CHECK(b.reserve(10) == Reserve::Grew && b.capacity() == 15);
        CHECK(b.reserve(16) == Reserve::Failed && b.get() == nullptr && b.capacity() == 0 && CountingMem::live == 0);
        CHECK(b.reserve(4) == Reserve::Grew && b.capacity() == 6 && CountingMem::live == 1);
        CountingMem::fail_at = CountingMem::allocs + 1;
        CHECK(!b.alloc(3) && b.get() == nullptr && b.capacity() == 0 && CountingMem::live == 0);
    }
    CHECK(CountingMem::live == 0 && CountingMem::frees == 2);
    return 0;
}

int move_swap_reset() {
    CountingMem::restart();
    {
        Buf a, b;
        CHECK(a.alloc(8) && b.alloc(3));
        uint32_t *pa = a.get(), *pb = b.get();
        a.swap(b);
        CHECK(a.get() == pb && a.capacity() == 3 && b.get() == pa && b.capacity() == 8 && CountingMem::frees == 0);
        Buf c(std::move(b));                                                      // move construction empties the source
        CHECK(c.get() == pa && c.capacity() == 8 && b.get() == nullptr && b.capacity() == 0 && CountingMem::frees == 0);
        a = std::move(c);                                                         // move assignment frees what the target held
        CHECK(a.get() == pa && a.capacity() == 8 && c.get() == nullptr && c.capacity() == 0);
        CHECK(CountingMem::frees == 1 && CountingMem::live == 1);
        Buf &self = a;
        a = std::move(self);                                                      // (onto itself: nothing happens)
        CHECK(a.get() == pa && CountingMem::frees == 1);
        Buf empty;
        a.swap(empty);                                                            // the grow-and-keep idiom: the old block leaves with the local
        CHECK(a.get() == nullptr && empty.get() == pa);
    }
    CHECK(CountingMem::live == 0 && CountingMem::allocs == 2 && CountingMem::frees == 2);
    // reset() and then the destructor: freed exactly once
    CountingMem::restart();
    {
        Buf b;
        CHECK(b.alloc(5));
        b.reset();
        CHECK(b.get() == nullptr && b.capacity() == 0 && CountingMem::frees == 1 && CountingMem::live == 0);
        b.reset();
        CHECK(CountingMem::frees == 1);
    }
    CHECK(CountingMem::frees == 1 && CountingMem::allocs == 1 && CountingMem::live == 0);
    return 0;
}

// the way the library builds a feature: five buffers one after the other, leaving at the first failure
bool five_buffers(size_t &made) {
    Buf a, b, c, d, e;
    Buf *all[5] = {&a, &b, &c, &d, &e};
    made = 0;
    for (Buf *x : all) {
        if (made % 2 ? x->reserve(10 + made) == Reserve::Failed : !x->alloc(10 + made)) return false;
        made++;
    }
    return CountingMem::live == 5;
}

int injected_failures() {
    for (size_t k = 1; k <= 5; k++) {
        CountingMem::restart(k);
        size_t made = 0;
        CHECK(!five_buffers(made) && made == k - 1);
        CHECK(CountingMem::live == 0 && CountingMem::frees == k - 1 && CountingMem::allocs == k);
    }
    CountingMem::restart(6);                                                      // (no failure within the five)
    size_t made = 0;
    CHECK(five_buffers(made) && made == 5 && CountingMem::live == 0 && CountingMem::frees == 5);
    return 0;
}

int replica_rule() {
    using gorder::replica_count;
    const size_t cap_words = ((size_t)64 << 20) / 8;                              // 64 MiB of u64
    CHECK(gorder::kReplicaBytesMax == (size_t)64 << 20);
    // replicas of exactly 64 MiB together are kept; one word more halves them
    CHECK(replica_count(32, cap_words / 32) == 32);
    CHECK(replica_count(32, cap_words / 32 + 1) == 16);
    CHECK(replica_count(1, cap_words) == 1 && replica_count(2, cap_words / 2) == 2 && replica_count(2, cap_words / 2 + 1) == 1);
    // halved as often as it takes, a count that is no power of two included
    CHECK(replica_count(32, cap_words / 4) == 4 && replica_count(32, cap_words / 4 + 1) == 2);
    CHECK(replica_count(24, cap_words / 6) == 6 && replica_count(24, cap_words / 6 + 1) == 3);
    CHECK(replica_count(1024, 1) == 1024 && replica_count(32, 0) == 32);
    // never below one, however large the block
    CHECK(replica_count(32, cap_words) == 1 && replica_count(32, cap_words + 1) == 1 && replica_count(32, cap_words * 1000) == 1);
    CHECK(replica_count(1, cap_words * 1000) == 1 && replica_count(3, cap_words * 1000) == 1);
    return 0;
}

}  // namespace

int main() {
    if (reserve_rules() || failure_rules() || move_swap_reset() || injected_failures() || replica_rule()) return 1;
    printf("device_mem ok\n");
    return 0;
}
