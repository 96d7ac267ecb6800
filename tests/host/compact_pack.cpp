// compact_pack.cpp — the host side of compact assignments (csrc/ingest.hip: assignment_pack, assignment_packed_validate,
// assignment_unpack, packed_first_is_one) under ASan + UBSan.  Every buffer is a heap block of exactly its size, so a read or a write
// one byte outside it is a report: packings of assignments of every width mix at block-boundary sizes, a `cap` one byte short, every
// proper prefix and a longer copy of a packing, and 4 000 seeded single-byte mutations of one — each refused, or unpacked into a block
// of exactly the size its header names.  A stand-alone program (tests/test_compact_assignment.py builds and runs it): no device, no
// context, nothing loaded into another process.
//   g++ -O1 -g -std=c++17 -DZK_EMU -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zokrates_amd/csrc tests/host/compact_pack.cpp
#include "ingest.hip"

#include <cstdio>
#include <memory>

using namespace zk;

static int bad = 0;
static void expect(bool ok, const char* what, uint64_t at) {
    if (!ok) { printf("%s (%llu)\n", what, (unsigned long long)at); ++bad; }
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
typedef std::unique_ptr<uint8_t[]> Block;
static Block block(size_t n) { return Block(new uint8_t[n ? n : 1]); }

// m elements: zeros, bytes, 64-bit values and values below 2^252, in runs and singly; element 0 is 1
static Block assignment(uint64_t m) {
    Block z = block(m * 32);
    memset(z.get(), 0, m * 32);
    for (uint64_t i = 0; i < m; ++i) {
        const int c = i == 0 ? 1 : (int)(rnd() % 4);
        uint8_t* v = z.get() + 32 * i;
        if (c == 1) v[0] = i == 0 ? 1 : (uint8_t)(1 + rnd() % 255);
        if (c == 2) { const uint64_t x = rnd() | 256; memcpy(v, &x, 8); }
        if (c == 3) { for (int k = 0; k < 32; ++k) v[k] = (uint8_t)rnd(); v[31] &= 0x0f; v[20] |= 1; }
    }
    return z;
}
// the exact-size packing of z
static Block packing(const uint8_t* z, uint64_t m, uint64_t* len) {
    uint8_t none;
    bool refused = false;
    try { assignment_pack(z, m, &none, 0, len); } catch (const IngestError& e) { refused = e.code == ZKHIP_ERR_BAD_ARG; }
    expect(refused, "a cap of 0 not refused", m);
    Block out = block(*len);
    if (*len > 1) {
        refused = false;
        uint64_t again = 0;
        try { assignment_pack(z, m, out.get(), *len - 1, &again); } catch (const IngestError& e) { refused = e.code == ZKHIP_ERR_BAD_ARG; }
        expect(refused && again == *len, "a cap one byte short not refused", m);
    }
    assignment_pack(z, m, out.get(), *len, len);
    return out;
}
// validate + unpack a buffer held in a block of exactly `len`; returns whether it was accepted
static bool try_unpack(const uint8_t* src, size_t len, uint64_t m_most, const uint8_t* want_z, uint64_t want_m) {
    Block b = block(len);
    memcpy(b.get(), src, len);
    PackedLayout ly;
    try {
        ly = assignment_packed_validate(b.get(), len);
    } catch (const IngestError& e) {
        expect(e.code == ZKHIP_ERR_PARSE && !e.msg.empty(), "a refusal without ZKHIP_ERR_PARSE and a message", len);
        return false;
    }
    if (ly.m > m_most) return false;      // (what zkhip_assignment_unpack refuses for m_cap)
    Block z = block(ly.m * 32);
    assignment_unpack(b.get(), ly, z.get());
    (void)packed_first_is_one(b.get(), ly);
    if (want_z) expect(ly.m == want_m && !memcmp(z.get(), want_z, want_m * 32), "unpack(pack(z)) differs from z", want_m);
    return true;
}

int main() {
    static const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 4099};
    for (uint64_t m : sizes) {
        Block z = assignment(m);
        uint64_t len = 0;
        Block p = packing(z.get(), m, &len);
        expect(len % 16 == 0 && len >= packed_layout(m, 0).payload_off, "length not a multiple of 16", m);
        expect(try_unpack(p.get(), len, m, z.get(), m), "a packing refused", m);
        if (m) expect(packed_first_is_one(p.get(), assignment_packed_validate(p.get(), len)), "element 0 not seen as 1", m);
    }
    // a value canonical in no supported field
    {
        Block z = assignment(9);
        memset(z.get() + 32 * 5, 0xff, 32);
        uint64_t len = 0;
        Block out = block(4096);
        bool refused = false;
        try { assignment_pack(z.get(), 9, out.get(), 4096, &len); } catch (const IngestError& e) { refused = e.code == ZKHIP_ERR_BAD_ARG; }
        expect(refused, "2^256 - 1 packed", 5);
    }
    const uint64_t m = 2100;
    Block z = assignment(m);
    uint64_t len = 0;
    Block p = packing(z.get(), m, &len);
    for (size_t cut = 0; cut < len; cut += cut < 64 ? 1 : 37) expect(!try_unpack(p.get(), cut, m, nullptr, 0), "a proper prefix accepted", cut);
    {
        Block longer = block(len + 16);
        memcpy(longer.get(), p.get(), len);
        memset(longer.get() + len, 0, 16);
        expect(!try_unpack(longer.get(), len + 1, m, nullptr, 0) && !try_unpack(longer.get(), len + 16, m, nullptr, 0), "a longer buffer accepted", len);
    }
    const PackedLayout ly = assignment_packed_validate(p.get(), len);
    int accepted = 0, refused = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        // a quarter of the mutations in each section: the payload is most of the bytes and no rule reads it
        const uint64_t lo[4] = {0, ly.tags_off, ly.index_off, ly.payload_off}, hi[4] = {ly.tags_off, ly.index_off, ly.payload_off, ly.total};
        const size_t at = lo[trial % 4] + rnd() % (hi[trial % 4] - lo[trial % 4]);
        Block q = block(len);
        memcpy(q.get(), p.get(), len);
        q[at] ^= (uint8_t)(1 + rnd() % 255);
        (try_unpack(q.get(), len, m, nullptr, 0) ? accepted : refused)++;
    }
    expect(accepted >= 1000 && refused >= 1500, "mutants: too few accepted or refused", (uint64_t)accepted);
    printf("%d accepted, %d refused; %d failures\n", accepted, refused, bad);
    return bad ? 1 : 0;
}
