// host_rows.hpp -- "only the written entries of a row are copied out": the row copy behind every host form of the token index that
// fills [Q, cap] arrays of the caller (capi_token*.hpp).  Host code without a HIP call, so tools/host_sanitize.cpp drives it under
// the sanitizers.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace sa {

// row lengths that sit `stride` bytes apart, as the `written` of an array of heads does (a plain u32 array: stride 4)
struct StridedLen {
    const void* first;
    size_t stride;
    u32 operator()(u64 i) const {
        u32 v;
        memcpy(&v, static_cast<const unsigned char*>(first) + i * stride, sizeof v);
        return v;
    }
};

// The first min(len(i), cap) cells of every row i of the dense [Q, cap] array src into the same row of dst; every other cell of dst
// stays as it is.  Nothing is touched when cap == 0 (dst and src may be NULL then).
template <class Cell, class Len>
inline void copy_written_rows(Cell* dst, const Cell* src, u64 Q, u32 cap, Len&& len) {
    static_assert(std::is_trivially_copyable<Cell>::value, "rows are copied with memcpy");
    for (u64 i = 0; i < Q && cap; ++i) {
        const u64 l = len(i);
        memcpy(dst + i * cap, src + i * cap, (size_t)(l < cap ? l : cap) * sizeof(Cell));
    }
}

}  // namespace sa
