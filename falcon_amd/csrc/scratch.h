// Layout of one scratch block (fal_ctx::reserve): plain host C++, no HIP -- tests/test_scratch_cpu.py compiles it on its own.
//
// A host entry point states the arrays it cuts one slot into, once, in the order they lie in the block:
//
//     fal::ScratchLayout L;
//     const auto rank = L.array<int64_t>(n + 1);      // one statement per array: element type, element count
//     const auto comp = L.array<int32_t>(n);
//     L.pad(64);                                      // slack, with the site's reason
//     FAL_TRY(L.reserve(ctx, SLOT_X));                // ONE request for the whole block
//     kernel<<<...>>>(rank, comp, ...);               // a handle converts to its T*
//
// The size of the block and every pointer derive from the same statements.  An array starts at the next multiple of
// alignof(T) behind its predecessor and nothing else is added, so wider arrays in front of narrower ones pack without a gap.
// A negative count, or a block whose size does not fit size_t, makes reserve() fail with FAL_EINTERNAL before the context is
// asked.  A handle gives nullptr until reserve() has succeeded.  The layout holds three words and its handles point at it: it
// stays where it was declared.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/falcon_hip.h"

namespace fal {

class ScratchLayout {
public:
    template <class T>
    struct Array {
        const ScratchLayout* layout;
        size_t offset;
        T* get() const { return layout->base_ ? (T*)(layout->base_ + offset) : nullptr; }
        operator T*() const { return get(); }
    };

    ScratchLayout() = default;
    ScratchLayout(const ScratchLayout&) = delete;
    ScratchLayout& operator=(const ScratchLayout&) = delete;

    template <class T>
    Array<T> array(int64_t count) {
        align(alignof(T));
        const Array<T> a{this, bytes_};
        grow(count, sizeof(T));
        return a;
    }
    void pad(int64_t bytes) { grow(bytes, 1); }
    // the next array starts at a multiple of `to` (a power of two) -- for a block whose consumer wants more than alignof(T)
    void align(size_t to) {
        const size_t gap = (size_t)(0 - bytes_) & (to - 1);
        if (gap > SIZE_MAX - bytes_) bad_ = true;
        else bytes_ += gap;
    }
    size_t bytes() const { return bytes_; }

    template <class Ctx>
    int reserve(Ctx* ctx, int slot) {
        if (bad_) return FAL_EINTERNAL;
        void* p = nullptr;
        const int rc = ctx->reserve(slot, bytes_, &p);
        base_ = rc == FAL_OK ? (char*)p : nullptr;
        return rc;
    }

private:
    void grow(int64_t count, size_t each) {
        if (count < 0 || (uint64_t)count > (SIZE_MAX - bytes_) / each) bad_ = true;
        else bytes_ += (size_t)count * each;
    }
    char* base_ = nullptr;
    size_t bytes_ = 0;
    bool bad_ = false;
};

}  // namespace fal
