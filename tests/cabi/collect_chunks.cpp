// Drives gorder_amd/csrc/collect_store.h (the host side of gorder_hip_set_collect) without a device: bit-packed flag rows
// of 1, 63, 64, 65 and 129 molecules and rows of normals are appended batch by batch across chunk boundaries, cleared,
// appended again into the kept chunks, unpacked and compared.  Built with -fsanitize=address,undefined by
// tests/test_collect_cpu.py; exit status 0 and "collect_chunks ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "collect_store.h"

namespace {

size_t live_allocations = 0;
void *count_alloc(size_t bytes) { live_allocations++; return malloc(bytes); }
void count_free(void *p) { live_allocations--; free(p); }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_random() {       // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// append `batches` of flag rows for n_mol molecules the way the library does — pack into a staging block, reserve, copy the
// pieces — and read them back
int flags_round(gorder::CollectStore &store, size_t n_mol, const std::vector<size_t> &batches, uint64_t first_frame) {
    const size_t words = gorder::collect_flag_words(n_mol);
    std::vector<uint8_t> given;
    std::vector<uint64_t> frames_given;
    for (size_t n_rows : batches) {
        std::vector<uint64_t> staging(n_rows * words), frames(n_rows);
        for (size_t r = 0; r < n_rows; r++) {
            std::vector<uint8_t> row(n_mol);
            for (uint8_t &f : row) f = (uint8_t)(next_random() & 1u);
            gorder::collect_pack_flags(row.data(), n_mol, staging.data() + r * words);
            given.insert(given.end(), row.begin(), row.end());
            frames[r] = first_frame + 5u * frames_given.size();
            frames_given.push_back(frames[r]);
        }
        std::vector<gorder::CollectPiece> pieces;
        CHECK(store.reserve(frames.data(), n_rows, pieces));
        const char *src = reinterpret_cast<const char *>(staging.data());
        size_t rows = 0;
        for (const gorder::CollectPiece &pc : pieces) {
            memcpy(pc.host, src, pc.rows * store.row_bytes());
            src += pc.rows * store.row_bytes();
            rows += pc.rows;
        }
        CHECK(rows == n_rows);
    }
    CHECK(store.n_rows() == frames_given.size());
    CHECK(store.frames() == frames_given);
    std::vector<uint8_t> got(given.size() + 1, 0xAB);      // (one byte past the end must stay)
    uint64_t seen = 0;
    store.for_each_row([&](uint64_t r, const void *row) {
        gorder::collect_unpack_flags(static_cast<const uint64_t *>(row), n_mol, got.data() + r * n_mol);
        // the bits past the last molecule of a row are 0
        const uint64_t last = static_cast<const uint64_t *>(row)[words - 1];
        if (n_mol % 64u && (last >> (n_mol % 64u))) seen = ~0ull;
        seen++;
    });
    CHECK(seen == frames_given.size());
    CHECK(got.back() == 0xAB);
    CHECK(memcmp(got.data(), given.data(), given.size()) == 0);
    return 0;
}

}  // namespace

int main() {
    const gorder::CollectAlloc alloc{count_alloc, count_free};
    for (size_t n_mol : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)129}) {
        gorder::CollectStore store;
        // chunks of 5 rows: batches of 1, 4 (fills a chunk exactly), 7 (larger than a chunk), 3 + 3 (the second crosses)
        store.configure(gorder::collect_flag_words(n_mol) * sizeof(uint64_t), alloc, 5 * gorder::collect_flag_words(n_mol) * sizeof(uint64_t));
        if (flags_round(store, n_mol, {1, 4, 7, 3, 3, 0, 11}, 0)) return 1;
        const size_t chunks = store.n_chunks();
        CHECK(chunks >= 4);
        store.clear();                                        // gorder_hip_reset: rows gone, chunks kept and filled again
        CHECK(store.n_rows() == 0 && store.n_chunks() == chunks);
        if (flags_round(store, n_mol, {2, 9, 1}, 1000000000000ull)) return 1;
        CHECK(store.n_chunks() == chunks);
        store.clear();
        if (flags_round(store, n_mol, {40}, 7)) return 1;     // more than all kept chunks hold
        CHECK(store.n_chunks() == chunks + 1);
    }
    CHECK(live_allocations == 0);                             // the destructor released every chunk
    {   // the default chunk: 8 MiB or one batch, whichever is larger
        gorder::CollectStore store;
        const size_t row = 129 * 3 * sizeof(float);
        store.configure(row, alloc);
        std::vector<gorder::CollectPiece> pieces;
        std::vector<uint64_t> frames(3, 0);
        CHECK(store.reserve(frames.data(), 3, pieces) && pieces.size() == 1 && store.n_chunks() == 1);
        memset(pieces[0].host, 0x5A, 3 * row);
        const size_t big = gorder::kCollectChunkBytes / row + 10;
        frames.assign(big, 1);
        CHECK(store.reserve(frames.data(), big, pieces) && pieces.size() == 2);
        CHECK(pieces[0].rows == (gorder::kCollectChunkBytes + row - 1) / row - 3 && pieces[1].rows == big - pieces[0].rows);
        for (const gorder::CollectPiece &pc : pieces) memset(pc.host, 0x3C, pc.rows * row);      // every byte handed out is ours
        uint64_t n = 0, bad = 0;
        store.for_each_row([&](uint64_t r, const void *p) {
            const unsigned char want = r < 3 ? 0x5A : 0x3C;
            const unsigned char *b = static_cast<const unsigned char *>(p);
            if (b[0] != want || b[row - 1] != want) bad++;
            n++;
        });
        CHECK(n == big + 3 && bad == 0);
        store.release();
        CHECK(live_allocations == 0);
    }
    {   // an allocator that fails: the call appends nothing
        gorder::CollectStore store;
        store.configure(8, gorder::CollectAlloc{[](size_t) -> void * { return nullptr; }, [](void *) {}}, 16);
        std::vector<gorder::CollectPiece> pieces;
        const uint64_t frames[3] = {0, 1, 2};
        CHECK(!store.reserve(frames, 3, pieces) && pieces.empty() && store.n_rows() == 0);
    }
    puts("collect_chunks ok");
    return 0;
}
