// orbx_layout.h -- offset arithmetic of one buffer cut into regions.  No HIP: plain C++,
// so that the layouts can be checked on a machine without a GPU (tests/cpp/host_layout.cpp).
#pragma once

#include <cstddef>

namespace orbx {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
// orbx_matcher.cpp's regions: rounded, plus 256 bytes of slack (its kernels stage with
// whole-dword and 16-byte loads)
inline size_t pad(size_t b) { return up256(b) + 256; }

// The regions of one buffer, in order.  Each region's size is written once, in take();
// total() is the allocation that holds exactly the regions taken.  How a region's size is
// rounded belongs to the Layout, chosen where it is made.
struct Layout {
    size_t (*round)(size_t);  // nullptr: regions are packed
    size_t end = 0;
    explicit Layout(size_t (*r)(size_t)) : round(r) {}
    size_t take(size_t bytes) {
        const size_t o = end;
        end += round ? round(bytes) : bytes;
        return o;
    }
    void align256() { end = up256(end); }
    size_t total() const { return end; }
};

}  // namespace orbx
