// Host-only check of the two planes of the int8 code (code8_scan.hpp) for a sanitizer build: the
// pack / unpack functions over exactly sized heap buffers, and the plane offsets of an index of `cap` rows — every row's
// high and low part must lie inside the cap * d bytes of the allocation, the parts of different rows must not overlap.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I../../minivectordb_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -o code8_planes_host code8_planes_host.hip && ./code8_planes_host
// Runs on the CPU; it never touches a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "code8_scan.hpp"

using namespace mvdb;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);    \
            ++fails;                                              \
        }                                                         \
    } while (0)

static void roundtrip(int d, const std::vector<int8_t>& codes) {
    // heap buffers of the exact sizes: a byte past either end is a sanitizer report
    uint8_t* high = (uint8_t*)std::malloc((size_t)code8_high_stride(d));
    uint8_t* low = (uint8_t*)std::malloc((size_t)code8_low_stride(d));
    int8_t* back = (int8_t*)std::malloc((size_t)d);
    code8_pack_row(d, codes.data(), high, low);
    code8_unpack_row(d, high, low, back);
    CHECK(std::memcmp(back, codes.data(), (size_t)d) == 0);
    for (int t = 0; t < d / 16; ++t) {
        uint32_t h[3], c[4];
        std::memcpy(h, high + 12 * t, 12);
        code8_unpack_high(h, c);
        for (int j = 0; j < 16; ++j) {
            const int8_t top = (int8_t)(c[j / 4] >> (8 * (j % 4)));
            const int8_t code = codes[16 * t + j];
            CHECK(top == (int8_t)(code & ~3) && code - top >= 0 && code - top <= 3);
        }
    }
    std::free(high);
    std::free(low);
    std::free(back);
}

int main() {
    const int dims[] = {384, 512, 1024, 16};
    unsigned s = 12345u;
    for (int d : dims) {
        std::vector<int8_t> c((size_t)d);
        for (int rep = 0; rep < 16; ++rep) {
            for (auto& v : c) {
                s = s * 1664525u + 1013904223u;
                v = (int8_t)((int)((s >> 16) % 255u) - 127);
            }
            roundtrip(d, c);
        }
        for (int v : {127, -127, 0, 124, 3, -125}) {
            std::fill(c.begin(), c.end(), (int8_t)v);
            roundtrip(d, c);
        }
        // the planes of an index: one allocation of cap * d bytes, written row by row through the offsets the library uses
        for (int64_t cap : {1, 7, 1000}) {
            const size_t bytes = (size_t)cap * (size_t)d;
            uint8_t* C8 = (uint8_t*)std::malloc(bytes);
            std::memset(C8, 0xEE, bytes);
            uint8_t* lowp = C8 + code8_low_offset(cap, d);
            CHECK(code8_low_offset(cap, d) + (size_t)cap * code8_low_stride(d) == bytes);
            CHECK(code8_high_stride(d) % 4 == 0 && code8_low_stride(d) % 4 == 0 && code8_high_stride(d) + code8_low_stride(d) == d);
            std::vector<int8_t> all(bytes);
            for (auto& v : all) {
                s = s * 1664525u + 1013904223u;
                v = (int8_t)((int)((s >> 16) % 255u) - 127);
            }
            for (int64_t r = 0; r < cap; ++r)
                code8_pack_row(d, all.data() + r * d, C8 + r * code8_high_stride(d), lowp + r * code8_low_stride(d));
            std::vector<int8_t> back((size_t)d);
            for (int64_t r = cap - 1; r >= 0; --r) {
                code8_unpack_row(d, C8 + r * code8_high_stride(d), lowp + r * code8_low_stride(d), back.data());
                CHECK(std::memcmp(back.data(), all.data() + r * d, (size_t)d) == 0);
            }
            std::free(C8);
        }
    }
    // the integer range of the first stage (code8_qmax): d * 128 * qmax < 2^31
    for (int d : {384, 512, 1024}) CHECK((long long)d * 128 * code8_qmax(d) < (1ll << 31));
    std::printf(fails ? "code8 planes host check: %d FAILED\n" : "code8 planes host check: ok\n", fails);
    return fails ? 1 : 0;
}
