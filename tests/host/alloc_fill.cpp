// The tests-only allocation fill of csrc/devrt.h (ZKHIP_TUNE_ALLOC_FILL) in the emulator's allocator, stand-alone on the CPU
// (tests/test_workspace_reuse.py builds it with ASan + UBSan): off by default; while the word is non-zero every block dev_alloc and
// host_alloc_pinned hand out holds it from the first byte to the last of the block (the size rounded up to 256 bytes, 16 for a
// request of 0), in the word's own byte order where the length is no multiple of 4.
#include <cstdio>
#include <cstring>

#include "devrt.h"

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                \
        }                                                              \
    } while (0)

static bool holds(const void* p, size_t bytes, uint32_t w) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; ++i)
        if (b[i] != (unsigned char)(w >> (8 * (i & 3)))) return false;
    return true;
}

int main() {
    using namespace zk;
    const size_t sizes[] = {0, 1, 3, 4, 5, 255, 256, 257, 4096, (size_t)3 << 20};
    const uint32_t words[] = {0x00000005u, 0x01010101u, 0xA1B2C3D4u};
    int cases = 0;
    CHECK(alloc_fill_word().load() == 0);
    for (uint32_t w : words) {
        alloc_fill_word().store(w);
        for (size_t n : sizes) {
            const size_t block = ((n ? n : 16) + 255) / 256 * 256;
            void* d = dev_alloc(n);
            void* h = host_alloc_pinned(n);
            CHECK(d && holds(d, block, w));
            CHECK(h && holds(h, block, w));
            dev_free(d);
            host_free_pinned(h);
            cases += 2;
        }
    }
    // the fill of a length that is no multiple of 4 ends inside a word
    unsigned char odd[11];
    memset(odd, 0xEE, sizeof odd);
    host_fill_words(odd, 10, 0xA1B2C3D4u);
    CHECK(holds(odd, 10, 0xA1B2C3D4u) && odd[10] == 0xEE);
    // off again: the one branch of an allocation is not taken (what a fresh block holds is not this program's to read)
    alloc_fill_word().store(0);
    CHECK(alloc_fill_word().load() == 0);
    void* d = dev_alloc(64);
    CHECK(d != nullptr);
    dev_free(d);
    ++cases;
    fprintf(stderr, "%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
