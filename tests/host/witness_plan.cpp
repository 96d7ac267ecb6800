// witness_plan.cpp — the host side of witness files read on the device (csrc/wplan.h): the plan builder — the two id -> column tables
// and the places of the public inputs — and the checks of a file's framing, over heap blocks of exactly their sizes.  Built under
// ASan + UBSan (tests/test_witness_device.py); a stand-alone program, no device, no library.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I zokrates_amd/csrc tests/host/witness_plan.cpp
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "wplan.h"

using namespace zk;

static int bad = 0;
static void expect(bool ok, const char* what, long a = -1) {
    if (!ok) { printf("FAILED %s (%ld)\n", what, a); ++bad; }
}
// a program of l instance and w witness columns in the order `order`
static zkhip_prog program(int curve, uint64_t l, uint64_t w, std::vector<int64_t> order, std::vector<int64_t> public_args, uint64_t returns) {
    zkhip_prog p;
    p.curve = curve; p.l = l; p.w = w; p.return_count = returns;
    p.order = std::move(order);
    p.public_args = std::move(public_args);
    return p;
}
// what wplan_build says of a program it refuses ("" if it accepts)
static std::string refusal(const zkhip_prog& p, int curve, uint64_t l, uint64_t w) {
    WPlanTables t;
    try {
        wplan_build(p, curve, l, w, t);
    } catch (const IngestError& e) {
        expect(e.code == ZKHIP_ERR_BAD_ARG, "a refusal is ZKHIP_ERR_BAD_ARG", e.code);
        return e.msg;
    }
    return "";
}
// the count witness_header_validate returns for a heap block of exactly `len` bytes whose header says `count`; -1: refused (PARSE)
static long long framing(size_t len, uint64_t count) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[len ? len : 1]);
    if (len >= 8) memcpy(block.get(), &count, 8);
    else memset(block.get(), 0xff, len ? len : 1);
    try {
        return (long long)witness_header_validate(block.get(), len);
    } catch (const IngestError& e) {
        expect(e.code == ZKHIP_ERR_PARSE && e.msg.find("witness file") != std::string::npos, "a framing refusal is ZKHIP_ERR_PARSE and names the file", e.code);
        return -1;
    }
}

int main() {
    // ---- the tables: ~one, two public arguments (ids 7 and 3, in that argument order), ~out_1 then ~out_0 (first seen out of index
    // order), a private argument and sparse further variables
    const std::vector<int64_t> order = {0, 7, 3, -2, -1, 5, 40, 12, 1000};
    const zkhip_prog p = program(ZKHIP_CURVE_BN128, 5, 4, order, {7, 3}, 2);
    WPlanTables t;
    wplan_build(p, ZKHIP_CURVE_BN128, 5, 4, t);
    expect(t.pos.size() == 1001 && t.neg.size() == 2, "the tables are as long as the largest id named + 1", (long)t.pos.size());
    for (size_t j = 0; j < order.size(); ++j) {
        const int64_t id = order[j];
        expect((id >= 0 ? t.pos[(size_t)id] : t.neg[(size_t)(-(id + 1))]) == j, "column of an id", (long)j);
    }
    size_t named = 0;
    for (uint32_t c : t.pos) named += c != WPLAN_NO_COLUMN;
    for (uint32_t c : t.neg) named += c != WPLAN_NO_COLUMN;
    expect(named == order.size(), "every other entry says no column", (long)named);
    expect(t.input_cols == std::vector<uint32_t>({1, 2, 4, 3}), "public arguments in argument order, then ~out_0, ~out_1");
    expect(t.order == order && t.curve == ZKHIP_CURVE_BN128 && t.l == 5 && t.w == 4 && t.returns == 2, "what the plan remembers");
    // a program of ~one alone; one without negative ids (the negative table is empty)
    wplan_build(program(ZKHIP_CURVE_BLS12_381, 1, 0, {0}, {}, 0), ZKHIP_CURVE_BLS12_381, 1, 0, t);
    expect(t.pos.size() == 1 && t.neg.empty() && t.input_cols.empty() && t.pos[0] == 0, "m = 1");
    wplan_build(program(0, 2, 1, {0, 2, 1}, {2}, 0), 0, 2, 1, t);
    expect(t.pos == std::vector<uint32_t>({0, 2, 1}) && t.neg.empty() && t.input_cols == std::vector<uint32_t>({1}), "no outputs");
    // ---- refusals, each naming its reason
    expect(refusal(p, ZKHIP_CURVE_BN128, 5, 4).empty(), "the good program is accepted");
    expect(refusal(p, ZKHIP_CURVE_BLS12_381, 5, 4).find("curve") != std::string::npos, "another curve");
    expect(refusal(p, ZKHIP_CURVE_BN128, 4, 5).find("l = 4") != std::string::npos, "another l");
    expect(refusal(p, ZKHIP_CURVE_BN128, 5, 5).find("w = 5") != std::string::npos, "another w");
    const std::string twice = refusal(program(0, 2, 2, {0, 2, 1, 1}, {2}, 0), 0, 2, 2);
    expect(twice.find("consumed twice (repeated parameter)") != std::string::npos && twice.find("variable _0 ") != std::string::npos && twice.find("columns 2 and 3") != std::string::npos,
           "an id at two columns");
    expect(refusal(program(0, 2, 1, {0, -1, 0}, {}, 1), 0, 2, 1).find("~one") != std::string::npos, "~one at a second column");
    const std::string lost = refusal(program(0, 3, 1, {0, 4, -1, 9}, {4}, 2), 0, 3, 1);
    expect(lost.find("output ~out_1 has no column") != std::string::npos, "an output below R without a column");
    expect(refusal(program(0, 2, 2, {0, 4, -1, 9}, {4}, 1), 0, 2, 2).find("output ~out_0 is not an instance column") != std::string::npos, "an output among the witness columns");
    expect(refusal(program(0, 2, 1, {0, 4, 9}, {5}, 0), 0, 2, 1).find("public argument _4 has no column") != std::string::npos, "a public argument without a column");
    expect(refusal(program(0, 2, 1, {0, 4, 9}, {9}, 0), 0, 2, 1).find("public argument _8 is not an instance column") != std::string::npos, "a public argument among the witness columns");
    expect(refusal(program(0, 1, 1, {0, 1 << 20}, {}, 0), 0, 1, 1).find("no witness file") != std::string::npos, "an id at the range rule's bound");
    expect(refusal(program(0, 1, 1, {0, (1 << 20) - 1}, {}, 0), 0, 1, 1).empty(), "an id just below it");
    expect(refusal(program(0, 2, 0, {0, -(1 << 20) - 1}, {}, 0), 0, 2, 0).find("no witness file") != std::string::npos, "a negative id at the bound");
    expect(!refusal(program(0, 2, 1, {0, 4}, {4}, 0), 0, 2, 1).empty(), "an order shorter than l + w");
    expect(!refusal(program(0, 0, 0, {}, {}, 0), 0, 0, 0).empty(), "no columns at all");

    // ---- the framing of a file: len >= 8, len == 8 + 40 count, the count fits
    expect(framing(0, 0) == -1 && framing(7, 0) == -1, "shorter than its count");
    expect(framing(8, 0) == 0 && framing(48, 1) == 1 && framing(8 + 40 * 257, 257) == 257, "well-framed files");
    expect(framing(8, 1) == -1 && framing(47, 1) == -1 && framing(49, 1) == -1 && framing(48, 0) == -1 && framing(48, 2) == -1, "length against count");
    expect(framing(48, ~0ull) == -1 && framing(48, 1ull << 61) == -1 && framing(48, (1ull << 61) + 1) == -1 && framing(8, 0x6666666666666666ull) == -1,
           "counts whose 40-fold wraps around");
    // ---- the reader's range rule and spelling
    expect(witness_id_bound(0) == 1u << 20 && witness_id_bound(16384) == 1u << 20 && witness_id_bound(16385) == 64 * 16385 && witness_id_bound(1ull << 25) == 1ull << 31 &&
               witness_id_bound((1ull << 32) - 2) == 1ull << 31,
           "min(2^31, max(2^20, 64 count))");
    expect(witness_var_name(0) == "~one" && witness_var_name(1) == "_0" && witness_var_name(41) == "_40" && witness_var_name(-1) == "~out_0" && witness_var_name(-3) == "~out_2",
           "names");
    printf("%d failures\n", bad);
    return bad != 0;
}
