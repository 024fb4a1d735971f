// host_layout.cpp -- prints orbx::Layout's offsets and total for a list of region sizes.
//
//     host_layout <pad|up256|packed> <bytes | @>...
//
// A number takes a region of that many bytes; @ rounds the cursor up to 256 (align256).
// One line: every region's offset in order, then the total.  No HIP: orbx_layout.h only.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbx_layout.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    size_t (*round)(size_t) = nullptr;
    if (!std::strcmp(argv[1], "pad")) round = orbx::pad;
    else if (!std::strcmp(argv[1], "up256")) round = orbx::up256;
    else if (std::strcmp(argv[1], "packed")) return 2;
    orbx::Layout L(round);
    for (int i = 2; i < argc; i++) {
        if (!std::strcmp(argv[i], "@")) L.align256();
        else std::printf("%zu ", L.take((size_t)std::strtoull(argv[i], nullptr, 10)));
    }
    std::printf("%zu\n", L.total());
    return 0;
}
