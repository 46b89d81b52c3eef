// dev_buf.h — the one owner of a grow-only buffer: a pointer, its capacity and its release, tied
// together.  Plain C++17 with no HIP include: the memory space is a policy,
//
//     struct Space {
//         static constexpr bool kSlack = ...;          // regrowth reserves half as much again
//         static int alloc(void** p, size_t bytes);    // 0, or an error code with the error text set
//         static void free(void* p);
//     };
//
// knn_index.h defines the two real spaces (device and page-locked host memory); the host check
// (tests/fuzz/dev_buf_check.cpp) instantiates the same code over a counting heap.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>

namespace imgrec {

// An owned block of `Space` memory, untyped: what the corpus column table (below) handles.
template <typename Space>
class Block {
public:
    Block() = default;
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    Block(Block&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Block& operator=(Block&& o) noexcept {
        Block t(std::move(o));       // (self-move: `t` takes the block and hands it back)
        swap(t);
        return *this;
    }
    ~Block() { reset(); }

    void swap(Block& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); }
    void reset() {
        if (p_) Space::free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // A fresh block of exactly `bytes`: the old one is freed first (the two never coexist); on
    // failure the block is left empty and the space's error code comes back.
    int alloc(size_t bytes) {
        reset();
        const int rc = Space::alloc(&p_, bytes);
        if (rc != 0) p_ = nullptr;
        else bytes_ = bytes;
        return rc;
    }
    void* data() const { return p_; }
    size_t bytes() const { return bytes_; }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// A buffer of T that only grows (workspace reused across calls).  Reads as a T* wherever one is
// expected; contents do not survive a regrowth.
template <typename T, typename Space>
class Buf : public Block<Space> {
public:
    T* get() const { return static_cast<T*>(this->data()); }
    operator T*() const { return get(); }
    size_t cap() const { return this->bytes() / sizeof(T); }     // elements
    int reserve(size_t need) {
        if (cap() >= need) return 0;
        return this->alloc((Space::kSlack ? std::max(need, cap() * 3 / 2) : need) * sizeof(T));
    }
};

// One per-row array of a table whose arrays grow together, and its row stride in bytes.
template <typename Space>
struct Column {
    Block<Space>* buf;
    size_t stride;
};

// Regrow the n columns to `rows` rows each, all or none: every new block is allocated aside (in
// table order), `fill(i, dst, src)` brings column i's old rows over, `done()` waits for the fills,
// and only then do the columns take their new blocks and release the old.  On any failure the
// columns are as they were and the new blocks are gone.
template <typename Space, typename Fill, typename Done>
int regrow_columns(const Column<Space>* cols, int n, size_t rows, Fill&& fill, Done&& done) {
    constexpr int kMax = 8;
    if (n > kMax) return -1;
    Block<Space> fresh[kMax];
    int rc = 0;
    for (int i = 0; i < n && rc == 0; ++i) rc = fresh[i].alloc(rows * cols[i].stride);
    if (rc != 0) return rc;
    for (int i = 0; i < n && rc == 0; ++i) rc = fill(i, fresh[i].data(), cols[i].buf->data());
    const int rd = done();           // (also after a failed fill: its copies may still run)
    if (rc != 0 || rd != 0) return rc != 0 ? rc : rd;
    for (int i = 0; i < n; ++i) cols[i].buf->swap(fresh[i]);
    return 0;
}

}  // namespace imgrec
