// slot_sums_layout.cpp — SlotSums<C> (core.cuh): the layout of a proof slot's window sums, walked to the last byte of buffers of
// exactly the stated sizes.  Built for the emulator target under ASan + UBSan (tests/test_gm17.py); a stand-alone program, no device.
//   g++ -O1 -g -std=c++17 -DZK_EMU -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zokrates_amd/csrc tests/host/slot_sums_layout.cpp
#include "core.cuh"

template <class C>
static int walk(const char* name, int c_z, int s_z, int c_h, int s_h) {
    typedef zk::SlotSums<C> Lay;
    zkhip_ctx ctx;
    zkhip_pk pk;
    pk.z_n = 1000; pk.h_n = 1024;
    pk.c_z = c_z; pk.s_z = s_z; pk.c_h = c_h; pk.s_h = s_h;
    const Lay ly(&ctx, &pk);
    const size_t W = (size_t)ly.Wmax;
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { printf("%s c=(%d,%d) sets=(%d,%d): %s\n", name, c_z, c_h, s_z, s_h, what); ++bad; } };
    expect(W == 2 * (size_t)std::max(s_z, s_h), "Wmax is not two sums per bucket set of the larger MSM");
    expect(ly.b1() == 4 * W * sizeof(typename Lay::G1) && ly.b2() == W * sizeof(typename Lay::G2) && ly.lane_bytes() * 4 == ly.b1(), "sizes of the G1 / G2 parts");
    expect(ly.record_bytes() == ly.b1() + ly.b2() + 24, "size of the host record");

    ProofSlot sl;
    ly.reserve(sl);      // (the emulator's allocator rounds up: the walk below uses buffers of the exact sizes instead)
    expect(sl.ws1.cap == ly.b1() && sl.ws2.cap == ly.b2() && sl.h_ws_cap == ly.record_bytes() && sl.h_ws, "reserve() sizes");
    zk::host_free_pinned(sl.h_ws);
    sl.ws1.release(); sl.ws2.release();
    sl.ws1.p = malloc(ly.b1()); sl.ws2.p = malloc(ly.b2()); sl.h_ws = malloc(ly.record_bytes());   // (freed by the slot's buffers / below)

    // every accessor, written through to its last byte: the sanitizer sees a step past the end of any of the three buffers
    for (int k = 0; k < 4; ++k) {
        memset(ly.ws1(sl, k), 0x10 + k, ly.lane_bytes());
        memset(ly.hs1(sl, k), 0x20 + k, ly.lane_bytes());
        expect((uint8_t*)ly.ws1(sl, k) == (uint8_t*)sl.ws1.p + k * ly.lane_bytes(), "ws1(k)");
        expect((uint8_t*)ly.hs1(sl, k) == (uint8_t*)sl.h_ws + k * ly.lane_bytes(), "hs1(k)");
    }
    expect((uint8_t*)(ly.ws1(sl, 3) + W) == (uint8_t*)sl.ws1.p + ly.b1(), "the H sums end the G1 buffer");
    memset(ly.ws2(sl), 0x30, ly.b2());
    memset(ly.hs2(sl), 0x31, ly.b2());
    expect((uint8_t*)ly.hs2(sl) == (uint8_t*)(ly.hs1(sl, 3) + W) && (uint8_t*)(ly.hs2(sl) + W) == ly.zflag(sl), "the G2 mirror follows the G1 mirror, the zflag word the G2 mirror");
    const uint32_t flag = 0xA5A5A5A5u;
    memcpy(ly.zflag(sl), &flag, 4);
    memset(ly.zflag(sl) + 4, 0, 4);
    memset(ly.verdict(sl), 0x40, 16);
    expect(ly.verdict(sl) == ly.zflag(sl) + 8 && ly.verdict(sl) + 16 == (uint8_t*)sl.h_ws + ly.record_bytes(), "the verdict ends the record");
    expect(ly.zflag_word(sl) == flag, "zflag_word");
    // nothing written through one accessor was overwritten through another
    for (int k = 0; k < 4; ++k) expect(*(uint8_t*)ly.hs1(sl, k) == 0x20 + k && ((uint8_t*)ly.hs1(sl, k))[ly.lane_bytes() - 1] == 0x20 + k, "hs1(k) overlaps");
    expect(*(uint8_t*)ly.hs2(sl) == 0x31 && ((uint8_t*)ly.hs2(sl))[ly.b2() - 1] == 0x31, "hs2 overlaps");
    free(sl.h_ws);
    sl.h_ws = nullptr;
    return bad;
}

int main() {
    int bad = 0;
    const int cs[][4] = {{15, 1, 15, 1}, {17, 1, 16, 2}, {16, 3, 16, 1}, {13, 2, 17, 5}, {2, 1, 2, 1}};
    for (const auto& q : cs) {
        bad += walk<zk::CurveBn254>("bn254", q[0], q[1], q[2], q[3]);
        bad += walk<zk::CurveBls381>("bls12_381", q[0], q[1], q[2], q[3]);
    }
    // a window width this build cannot sort is refused where the layout is made
    try {
        zkhip_ctx ctx;
        zkhip_pk pk;
        pk.z_n = pk.h_n = 1000; pk.c_z = 40; pk.s_z = 1; pk.c_h = 15; pk.s_h = 1;
        zk::SlotSums<zk::CurveBn254> ly(&ctx, &pk);
        printf("c = 40 was accepted\n");
        ++bad;
    } catch (const zk::ApiError& e) {
        if (e.code != ZKHIP_ERR_BAD_ARG) { printf("wrong error code %d\n", e.code); ++bad; }
    }
    printf("%d failures\n", bad);
    return bad != 0;
}
