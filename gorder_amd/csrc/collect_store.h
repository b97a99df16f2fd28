// collect_store.h — host side of the per-frame history (gorder_hip_set_collect): rows of one fixed size kept in chunks of
// host memory that never move.  No HIP call in here: the memory comes from an allocator hook (the library hands in
// hipHostMalloc / hipHostFree, tests/cabi/collect_chunks.cpp plain malloc), so the bookkeeping, the bit packing and the
// assembly can be driven without a device.
//
// A batch reserves its rows before the copy that fills them is queued; a chunk handed to a copy is never reallocated or
// freed before release(), so a stream-ordered copy may still be in flight when the next batch reserves.  clear() forgets
// the rows and keeps the chunks for the next run (gorder_hip_reset).
#ifndef GORDER_COLLECT_STORE_H
#define GORDER_COLLECT_STORE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace gorder {

constexpr size_t kCollectChunkBytes = (size_t)8 << 20;   // a chunk is this large, or one batch where that is larger

struct CollectAlloc {
    void *(*alloc)(size_t bytes);      // nullptr on failure
    void (*release)(void *p);
};

// `rows` consecutive rows at `host`: one piece of a reservation (a batch that crosses a chunk boundary gets two or more)
struct CollectPiece {
    void *host;
    size_t rows;
};

// words of a bit-packed flag row: bit (m & 63) of word (m >> 6) = molecule m's flag (k_collect_flags)
inline size_t collect_flag_words(size_t n_mol) { return (n_mol + 63u) / 64u; }

inline void collect_pack_flags(const uint8_t *flags, size_t n_mol, uint64_t *words) {
    for (size_t w = 0; w < collect_flag_words(n_mol); w++) words[w] = 0;
    for (size_t m = 0; m < n_mol; m++)
        if (flags[m]) words[m >> 6] |= (uint64_t)1 << (m & 63u);
}

inline void collect_unpack_flags(const uint64_t *words, size_t n_mol, uint8_t *flags) {
    for (size_t m = 0; m < n_mol; m++) flags[m] = (uint8_t)((words[m >> 6] >> (m & 63u)) & 1u);
}

class CollectStore {
public:
    CollectStore() = default;
    CollectStore(const CollectStore &) = delete;
    CollectStore &operator=(const CollectStore &) = delete;
    ~CollectStore() { release(); }

    // chunk_bytes: tests pass a small value to cross chunk boundaries with little data
    void configure(size_t row_bytes, CollectAlloc alloc, size_t chunk_bytes = kCollectChunkBytes) {
        release();
        row_bytes_ = row_bytes;
        alloc_ = alloc;
        chunk_bytes_ = chunk_bytes;
    }
    bool configured() const { return row_bytes_ != 0; }
    size_t row_bytes() const { return row_bytes_; }
    uint64_t n_rows() const { return (uint64_t)frames_.size(); }
    size_t n_chunks() const { return chunks_.size(); }
    const std::vector<uint64_t> &frames() const { return frames_; }

    // Room for frames.size() more rows, in order, labelled with `frames`; false when the allocator fails (nothing is
    // appended then).  The pieces stay valid until release().
    bool reserve(const uint64_t *frames, size_t n, std::vector<CollectPiece> &pieces) {
        pieces.clear();
        if (!configured()) return false;
        const size_t cur0 = cur_, used0 = cur_ < chunks_.size() ? chunks_[cur_].used : 0;
        size_t left = n;
        while (left) {
            if (cur_ < chunks_.size() && chunks_[cur_].used < chunks_[cur_].cap) {
                Chunk &c = chunks_[cur_];
                const size_t take = left < c.cap - c.used ? left : c.cap - c.used;
                pieces.push_back({c.p + c.used * row_bytes_, take});
                c.used += take;
                left -= take;
            } else if (cur_ + 1 < chunks_.size()) {
                cur_++;                                     // a chunk kept from before clear()
            } else {
                size_t cap = (chunk_bytes_ + row_bytes_ - 1) / row_bytes_;
                if (cap < left) cap = left;                 // one batch, where that is larger
                char *p = static_cast<char *>(alloc_.alloc(cap * row_bytes_));
                if (!p) {                                   // undo: the rows of this call were never there
                    for (size_t k = cur0 + 1; k < chunks_.size(); k++) chunks_[k].used = 0;
                    if (cur0 < chunks_.size()) chunks_[cur0].used = used0;
                    cur_ = cur0;
                    pieces.clear();
                    return false;
                }
                chunks_.push_back({p, cap, 0});
                cur_ = chunks_.size() - 1;
            }
        }
        frames_.insert(frames_.end(), frames, frames + n);
        return true;
    }

    // f(row index, const void *row) for every row, in the order of appending
    template <typename F>
    void for_each_row(F f) const {
        uint64_t r = 0;
        for (const Chunk &c : chunks_)
            for (size_t k = 0; k < c.used; k++) f(r++, static_cast<const void *>(c.p + k * row_bytes_));
    }

    // forget the rows from row `n_rows` on (a batch that failed after it had reserved); the chunks stay
    void truncate(uint64_t n_rows) {
        if (n_rows >= frames_.size()) return;
        frames_.resize((size_t)n_rows);
        size_t left = (size_t)n_rows;
        cur_ = 0;
        for (size_t k = 0; k < chunks_.size(); k++) {
            Chunk &c = chunks_[k];
            c.used = left < c.used ? left : c.used;
            left -= c.used;
            if (c.used) cur_ = k;
        }
    }

    void clear() {
        for (Chunk &c : chunks_) c.used = 0;
        cur_ = 0;
        frames_.clear();
    }

    void release() {
        for (Chunk &c : chunks_) alloc_.release(c.p);
        chunks_.clear();
        cur_ = 0;
        frames_.clear();
    }

private:
    struct Chunk { char *p; size_t cap, used; };   // in rows
    size_t row_bytes_ = 0, chunk_bytes_ = kCollectChunkBytes;
    CollectAlloc alloc_{nullptr, nullptr};
    std::vector<Chunk> chunks_;
    size_t cur_ = 0;                               // the chunk being filled
    std::vector<uint64_t> frames_;                 // per row: the global frame index
};

}  // namespace gorder

#endif
